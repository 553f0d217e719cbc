"""numpy restatement of the reference's drawing (mmseg/visualization/local_visualizer.py:79-118, 218-219) -- a test helper, no
conftest: the specification of s2f_seg_draw (spike2former_amd/csrc/segdraw.hip) and ops.seg_draw.  `draw_sem_seg` is the
reference's eight lines as they stand: np.unique, the classes below num_classes, one masked write per class present, the float64
blend, astype(np.uint8).  The reduce_zero_label mapping (LoadAnnotations) and the BGR swap (the reference's caller decodes to RGB)
are written out beside it, and `panel` is add_datasample's concatenation.

One stated deviation, as in include/s2f.h: a NEGATIVE label paints nothing.  The reference would take palette[-1] for it (and an
IndexError below -K); no arg-max produces one.  It is the `ids >= 0` below."""
import numpy as np


def reduce_zero_label(seg):
    """LoadAnnotations(reduce_zero_label=True), mmseg/datasets/transforms/loading.py: 0 -> 255, then - 1, then 254 -> 255"""
    seg = np.array(seg)
    seg[seg == 0] = 255
    seg = seg - 1
    seg[seg == 254] = 255
    return seg


def draw_sem_seg(image, sem_seg, num_classes, palette, alpha):
    """image uint8 [H, W, 3] RGB; sem_seg [1, H, W] (any integer or float dtype); palette: num_classes RGB triples -> uint8 [H, W, 3]"""
    ids = np.unique(sem_seg)[::-1]
    with np.errstate(invalid="ignore"):
        legal_indices = (ids < num_classes) & (ids >= 0)          # `& (ids >= 0)`: the stated deviation
    ids = ids[legal_indices]
    labels = np.array(ids, dtype=np.int64)

    colors = [palette[label] for label in labels]

    mask = np.zeros_like(image, dtype=np.uint8)
    for label, color in zip(labels, colors):
        mask[sem_seg[0] == label, :] = color

    color_seg = (image * (1 - alpha) + mask * alpha).astype(np.uint8)
    return color_seg


def panel(image, palette, gt=None, pred=None, alpha=0.8, bgr=False, rzl=False):
    """what ops.seg_draw returns, from host arrays: image uint8 [H, W, 3]; gt / pred [H, W] or [1, H, W] -> uint8 [H, P W, 3] RGB"""
    image = np.asarray(image)
    if bgr:
        image = image[..., ::-1]
    palette = [list(int(v) for v in c) for c in np.asarray(palette)]
    drawn = []
    if gt is not None:
        gt = np.asarray(gt).reshape(1, *image.shape[:2])
        drawn.append(draw_sem_seg(image, reduce_zero_label(gt) if rzl else gt, len(palette), palette, alpha))
    if pred is not None:
        drawn.append(draw_sem_seg(image, np.asarray(pred).reshape(1, *image.shape[:2]), len(palette), palette, alpha))
    return np.concatenate(drawn, axis=1) if len(drawn) == 2 else drawn[0]


def arithmetic_fixture():
    """-> (image [256, 256, 3] with every channel value = its row, an int64 map = its column, the 256-entry palette
    k -> (k, (7 k + 3) % 256, 255 - k)): every (v, c) pair occurs in every channel"""
    v = np.arange(256, dtype=np.uint8)
    image = np.ascontiguousarray(np.broadcast_to(v[:, None, None], (256, 256, 3)))
    sem = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.int64)[None, :], (256, 256)))
    k = np.arange(256)
    palette = np.stack([k, (7 * k + 3) % 256, 255 - k], axis=1).astype(np.uint8)
    return image, sem, palette


ALPHAS = (0.8, 0.3, 0.7, 0.6, 0.5, 1.0, 0.0)
