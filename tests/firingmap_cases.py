"""The inputs the firing-map tests share (host and GPU files): spike maps with every level and every special value, the shape lists
of the two kernels, and the sentinel windows.  No expected value lives here: those come from tests/firingmap_ref.py."""
import numpy as np
import torch

MAP_P = (1, 3, 63, 64, 65, 257, 1024)
MAP_C = (1, 3, 64, 65)
MAP_TB_B = ((1, 1), (3, 1), (6, 2), (4, 4))
MAP_D = (4, 8, 3)
# (TB, B, C, P): many pixels / few planes, and few pixels / many planes (a 4 x 4 .. 16 x 16 map of 640 channels): both ends of the
# split rule, wide and scalar
MAP_ENDS = ((2, 2, 2, 128 * 128), (2, 1, 3, 100 * 101), (4, 2, 640, 16), (4, 2, 640, 15), (2, 1, 640, 256))

DRAW_SIZES = (((1, 1), (1, 1)), ((1, 1), (5, 7)), ((2, 3), (7, 13)), ((4, 4), (4, 4)), ((16, 16), (64, 64)), ((3, 5), (2, 2)),
              ((2, 2), (3, 600)), ((5, 2), (2100, 3)))
DRAW_A8 = (0, 1, 128, 205, 256)
SENTINEL = 0xA5


def specials(D):
    """values whose plane the contract names: -0.0 (zero), 0.3, -1/D, 65536/D, a subnormal, NaN, +-inf (off the grid, non-zero),
    65535/D (the largest level)"""
    return np.array([-0.0, 0.3, -1.0 / D, 65536.0 / D, 1e-40, np.nan, np.inf, -np.inf, 65535.0 / D], np.float32)


def spike_map(TB, C, P, D, seed, bf16=False, special=True):
    """-> (torch tensor [TB, C, P] fp32 or bf16, the same values for the numpy restatement: float32, or uint16 bf16 bits).  Every level
    0 .. D occurs (given room), about a third of the elements are silent, and the special values are sprinkled in."""
    rng = np.random.default_rng(seed)
    n = TB * C * P
    level = rng.integers(0, D + 1, n)
    level[rng.random(n) < 0.3] = 0
    k = min(n, D + 1)
    level[rng.permutation(n)[:k]] = np.arange(k)
    x = (level.astype(np.float32) / np.float32(D)).astype(np.float32)
    if special and n > 1:
        sp = specials(D)
        where = rng.permutation(n)[:min(len(sp), n // 2)]
        x[where] = sp[:len(where)]
    t = torch.from_numpy(x.reshape(TB, C, P))
    if not bf16:
        return t, t.numpy()
    t = t.to(torch.bfloat16)
    return t, t.view(torch.int16).numpy().view(np.uint16)


def at_offset(t, off, device="cpu", pad=5):
    """`t` as a contiguous view `off` elements into a larger buffer on `device`"""
    big = torch.zeros(off + t.numel() + pad, dtype=t.dtype, device=device)
    view = big[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def sentinel_stats(B, P, device="cpu", front=3, behind=5):
    """-> (the whole int32 buffer filled with a sentinel, its [B, 4, P] slice)"""
    big = torch.full((front + 4 * B * P + behind,), -123456789, dtype=torch.int32, device=device)
    return big, big[front:front + 4 * B * P].view(B, 4, P)


def draw_window(H, W, off, device="cpu"):
    """a strided [H, W, 3] window into a sentinel byte buffer: rows 3 W + 5 bytes apart, one row of sentinels above and below, two
    bytes left and three right of every row, the whole at byte offset `off` -> (buffer, window, the numpy index of the window)"""
    row = 3 * W + 5
    big = torch.full((off + (H + 2) * row,), SENTINEL, dtype=torch.uint8, device=device)
    start = off + row + 2
    return big, torch.as_strided(big, (H, W, 3), (row, 3, 1), start), (start, row)


def expect_window(H, W, off, want):
    """the bytes of draw_window's buffer after `want` [H, W, 3] was written into the window and nothing else"""
    row = 3 * W + 5
    exp = np.full(off + (H + 2) * row, SENTINEL, np.uint8)
    start = off + row + 2
    for y in range(H):
        exp[start + y * row:start + y * row + 3 * W] = want[y].reshape(-1)
    return exp


def draw_plane(h, w, seed, top=1000):
    """an int32 plane with values in 0 .. top, a few negative entries and its maximum present"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, top + 1, (h, w)).astype(np.int32)
    where = rng.permutation(h * w)
    p.flat[where[0]] = top
    if h * w > 2:
        p.flat[where[1]] = -7
    return p
