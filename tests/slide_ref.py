"""The specification of sliding-window inference (spike2former_amd/csrc/slide.hip, ops.slide_*, EncoderDecoder.slide_inference) in
numpy: the reference's loop (mmseg/models/segmentors/encoder_decoder.py:246-296) restated -- the window list, every window's logits
zero-padded to the full map and added in loop order, the count map, one division -- in float32, one rounding per operation.  A helper
module for the tests, not collected.  The two stand-in networks:

  fake_net   the stand-in of tests/test_a13_callers.py (and of oracle/gen_golden_a13.py, which wrote tests/golden/predict_a13.npz);
             its sin / einsum round differently with the batch composition and the device.
  lin_net    per class, the input channels times exactly representable scalars, summed: separate elementwise multiplications and
             additions only, so a pixel's value does not depend on the batch it sits in, on its memory position or on the device --
             what the bit-identity tests of the batched routes need."""
import types

import numpy as np
import torch

GRIDS = {          # name -> (H, W, crop, stride, (ny, nx, eh, ew))
    "fixture_3x3": (37, 53, (16, 24), (11, 17), (3, 3, 16, 24)),
    "short_1x3": (12, 53, (16, 24), (11, 17), (1, 3, 12, 24)),
    "one_window": (16, 24, (16, 24), (11, 17), (1, 1, 16, 24)),
    "stride_is_crop_2x2": (32, 48, (16, 24), (16, 24), (2, 2, 16, 24)),
    "shifted_back_2x3": (17, 30, (16, 24), (2, 5), (2, 3, 16, 24)),
    "stride_one_5x3": (20, 31, (16, 24), (1, 5), (5, 3, 16, 24)),
}
CITYSCAPES = (1024, 2048, (512, 1024), (341, 683), (3, 3, 512, 1024))

METAS = [dict(ori_shape=(30, 41), img_shape=(37, 53), pad_shape=(37, 53), padding_size=[0, 3, 0, 2]) for _ in range(2)]


def segmentor(test_cfg, K, net, calls=None):
    """EncoderDecoder as tests/test_a13_callers.py builds it: only test_cfg, out_channels, align_corners, decode_head and a stub
    encode_decode exist"""
    from spike2former_amd.segmentor import EncoderDecoder
    m = object.__new__(EncoderDecoder)
    torch.nn.Module.__init__(m)
    m.test_cfg, m.out_channels, m.align_corners = dict(test_cfg), K, False
    m.decode_head = types.SimpleNamespace(threshold=0.3)

    def encode_decode(x, metas):
        if calls is not None:
            calls.append((tuple(x.shape), tuple(metas[0]["img_shape"])))
        return net(x, K)
    m.encode_decode = encode_decode
    return m


def fake_net(x, K):
    w = torch.linspace(-1.0, 1.0, K * 3).view(K, 3).to(x.device)
    return torch.einsum("kc,nchw->nkhw", w, x) + 0.1 * torch.sin(3.0 * x.sum(1, keepdim=True))


def lin_net(x, K):
    planes = []
    for k in range(K):
        acc = x[:, 0] * ((3 * k - 7) / 8.0)
        for c in range(1, x.shape[1]):
            acc = acc + x[:, c] * ((3 * k + c - 7) / 8.0)
        planes.append(acc)
    return torch.stack(planes, 1)


def windows(H, W, crop, stride):
    """the reference's window list [(y1, y2, x1, x2)] in its loop order"""
    (hc, wc), (hs, ws) = crop, stride
    out = []
    for i in range(max(H - hc + hs - 1, 0) // hs + 1):
        for j in range(max(W - wc + ws - 1, 0) // ws + 1):
            y1, x1 = i * hs, j * ws
            y2, x2 = min(y1 + hc, H), min(x1 + wc, W)
            out.append((max(y2 - hc, 0), y2, max(x2 - wc, 0), x2))
    return out


def merge(logits, H, W, crop, stride):
    """logits [n windows, B, K, eh, ew] float32 (all the windows, in order) -> the reference's preds / count_mat [B, K, H, W]"""
    logits = np.asarray(logits, dtype=np.float32)
    wins = windows(H, W, crop, stride)
    assert len(wins) == logits.shape[0]
    B, K = logits.shape[1:3]
    preds = np.zeros((B, K, H, W), np.float32)
    count = np.zeros((B, 1, H, W), np.float32)
    for (y1, y2, x1, x2), lg in zip(wins, logits):
        padded = np.zeros_like(preds)
        padded[:, :, y1:y2, x1:x2] = lg
        preds += padded
        count[:, :, y1:y2, x1:x2] += 1
    assert (count == 0).sum() == 0
    return preds / count


def slide_ref(img, net, K, crop, stride):
    """img [B, 3, H, W] (a torch tensor) -> the merged logits as numpy, `net` run per window at batch B"""
    H, W = img.shape[-2:]
    lg = [net(img[:, :, y1:y2, x1:x2], K).detach().cpu().numpy() for y1, y2, x1, x2 in windows(H, W, crop, stride)]
    return merge(np.stack(lg), H, W, crop, stride)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
