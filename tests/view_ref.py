"""numpy restatement of the device-side test pipeline (s2f_test_views in spike2former_amd/csrc/augment.hip, TestAugment in
spike2former_amd/augment.py) -- a test helper, no conftest.  Built on aug_ref.bilinear_u8, the restatement of the resize step the
kernel shares with the training augmentation: resize -> horizontal flip -> channel swap -> fp32 normalisation -> padding on the
right and at the bottom.  Every float operation is ONE fp32 operation, in the kernel's order."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402


def view(img, H, W, Hp, Wp, flip, mean=None, std=None, bgr_to_rgb=False, pad_val=0.0):
    """img [h0, w0, 3] uint8 BGR -> [3, Hp, Wp] float32"""
    x = R.bilinear_u8(img, H, W)
    if flip:
        x = x[:, ::-1]
    if bgr_to_rgb:
        x = x[..., ::-1]
    x = x.astype(np.float32).transpose(2, 0, 1)
    if mean is not None:
        x = (x - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)
    out = np.full((3, Hp, Wp), pad_val, np.float32)
    out[:, :H, :W] = x
    return out


def views(images, sizes, **kw):
    """images: B pictures of one size; sizes: [(H, W, Hp, Wp, flip)] -> [one [B, 3, Hp, Wp] array per view]"""
    return [np.stack([view(i, *s, **kw) for i in images]) for s in sizes]


def scene(h0, w0, seed, n_classes=6):
    """a noise picture with flat extremes and a grey ramp, and a raw annotation of rectangles with ignored pixels and raw zeros"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    img[:4, :6] = 0
    img[:4, 6:12] = 255
    img[4:8, :12] = np.arange(12, dtype=np.uint8)[None, :, None] * 23
    seg = np.empty((h0, w0), np.uint8)
    classes = rng.permutation(n_classes) + 1
    for i, (y, x) in enumerate((y, x) for y in range(0, h0, 9) for x in range(0, w0, 11)):
        seg[y:y + 9, x:x + 11] = classes[i % n_classes]
    seg[2:4, 3:17] = 255
    seg[20:23, 5:9] = 0
    return img, seg
