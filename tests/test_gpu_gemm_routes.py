"""Every route of the 1x1 products (spike2former_amd/ops/gemm.py: spike_gemm, dense_gemm, spike_gemm_siblings, dx_gemm over bmm_small,
and the launchers of csrc/pgemm.hip, gemm_bf16.hip, gemm.hip, dwp.hip, bmm.hip they reach) against the fp64 restatement of
tests/gemm_ref.py, at the smallest shapes that reach it.  Each case is one row whose id names the route; the test first asserts from
the shape the inequality that puts the row there -- the launcher's rule restated in Python below, its constants read from the .hip
sources, through the library's own predicate where one decides (s2f_pgemm_nn_grouped_ok, s2f_spike_gemm_dw_pipe_ok,
s2f_bn_single_pass, s2f_bn_partials_count) -- builds its operands as the model does -- fp32 w / bias leaves, a bf16 Spikes with its
autograd handle, the gradient read from the fp32 leaf behind the neuron -- and proves the route by counting the lib.* calls of the
whole census below: a row lists the launches it must make, every other symbol of the census must stay at zero (the two weight
conversions s2f_pack_bf16x3 / s2f_split_bf16x3 are counted apart, by the rows that say so).

  exact rows      spikes sparse (25 %) multiples of 1/8 in [0, 1], a general map, w and bias multiples of 1/8 in [-1, 1], gy integers
                  in [-2, 2].  Each row first asserts on its own draw (fp64, gemm_ref.abs_sums) that every sum of ABSOLUTE terms stays
                  below 2^24 granules -- 1/64 for y, 1/8 for dx, dw, db -- so every fp32 partial sum is exact in any order (split-K,
                  atomics, matrix-core steps, one or two steps per barrier), and y, dx, dw, db must EQUAL the fp64 values.  The
                  BatchNorm partials of a stats row: the tile sums at granule 1/64 and the tile sums of squares at 1/4096 are asserted
                  below 2^24 granules too, and the partials must EQUAL the fp64 tile sums.
  three terms     the draws above fit the `hi` term of the bf16 x 3 operand split.  These rows give ONE operand 20 significant bits
                  (gemm_ref.wide_values: no entry is representable by two bf16 terms, asserted per entry) and make the other one-hot,
                  or a 0/1 selection matrix with one 1 per row and column, so every non-zero output is ONE product v * 1, equal to the
                  fp64 value only if hi, mid AND lo were multiplied.
  general rows    randn w, bias, gy (fp32 values read back as fp64), spikes stay spikes, a dense map is randn: per entry
                  |got - ref64| <= c A + 1e-30 with A the entry's sum of absolute terms and c (the constants of the convolution and
                  mask-contraction suites)  2e-6 a product with one operand exact in bf16, 4e-6 two general operands (every dx, all of
                  dense_gemm, everything on bmm_small), 2e-6 a bias gradient.  Partials against the fp64 tile sums of the kernel's OWN
                  y: within 1e-5 of the tile sums of |y| (of y^2 for the squares), the bound of test_dense_gemm_groups_forward_backward.
                  The same ratio max |err| / A of a plain fp32 CPU evaluation of gemm_ref is printed next to the kernel's.

The forced-cfg sweep calls the two entry points that take a `cfg` (s2f_pgemm_nn_bf16, s2f_pgemm_dx_f32) with every tile the tables
kNnTiles / kConvTiles (rows tiles) / kTnTiles list, on the exact draw: a (form, cfg) pair the cfg_set(...) tables build EQUALS fp64, a
pair they do not build returns S2F_EINVAL and leaves the output alone.  The forms a `cfg` argument reaches are the plain product,
beta = 1 and the contraction split; the statistics and grouped entry points take no cfg (their tile is the rule's, pinned by the
route rows).  Two rules of the launchers the sweep has to know: rows of N % 8 == 4 send an unknown cfg >= 9 to the rows tile 6 (the
rule for an environment-forced DMA tile), so unknown values are swept at N % 8 == 0; and the contraction split always runs tile 4.

Measured on the MI355X, worst |err| / A over the entries, kernel | fp32 CPU (docs/EXPERIMENTS.md has the same table; `c` of a
bmm_small row stands under y):
  spike_gemm bf16 2x40x72x36                   y 1.5e-7 | 1.5e-7   dx 1.9e-7 | 1.7e-7   dw 1.4e-7 | 9.7e-8   db --
  spike_gemm bf16 2x64x128x136                 y 3.0e-7 | 1.7e-7   dx 2.1e-7 | 2.6e-7   dw 7.2e-8 | 1.2e-7   db --
  spike_gemm bf16 1x100x96x132                 y 1.7e-7 | 1.8e-7   dx 2.0e-7 | 2.0e-7   dw 1.3e-7 | 2.0e-7   db --
  spike_gemm bf16 8x130x128x4096               y 2.8e-7 | 3.2e-7   dx 3.5e-7 | 3.6e-7   dw 2.6e-8 | 1.2e-8   db --
  spike_gemm bf16 8x130x128x3968               y 3.1e-7 | 3.5e-7   dx 3.1e-7 | 3.5e-7   dw 3.7e-8 | 1.2e-8   db --
  spike_gemm bf16 1x40x1024x136                y 1.8e-7 | 9.9e-8   dx 2.4e-7 | 3.4e-7   dw 1.3e-7 | 2.6e-7   db --
  spike_gemm bf16 1x40x1024x132                y 2.0e-7 | 7.3e-8   dx 2.6e-7 | 2.4e-7   dw 1.5e-7 | 1.8e-7   db --
  spike_gemm bf16 2x40x72x36 bias stats        y 1.1e-7 | 1.1e-7   dx 1.8e-7 | 1.9e-7   dw 1.1e-7 | 1.4e-7   db 2.9e-8 | 3.7e-8
  spike_gemm bf16 2x64x128x136 stats           y 3.0e-7 | 1.7e-7   dx 2.1e-7 | 2.6e-7   dw 7.2e-8 | 1.2e-7   db --
  spike_gemm bf16 2x64x32x4                    y 1.6e-7 | 1.0e-7   dx 1.2e-7 | 1.1e-7   dw 1.1e-7 | 8.7e-8   db --
  spike_gemm bf16 2x64x128x4                   y 7.4e-8 | 2.2e-7   dx 1.4e-7 | 1.9e-7   dw 1.3e-7 | 1.2e-7   db --
  spike_gemm bf16 1x40x512x4                   y 6.2e-8 | 1.3e-7   dx 1.5e-7 | 1.8e-7   dw 1.1e-7 | 8.9e-8   db --
  spike_gemm bf16 512x128x32x4                 y 2.2e-7 | 1.9e-7   dx 2.3e-7 | 2.4e-7   dw 1.0e-7 | 2.9e-8   db --
  spike_gemm bf16 512x256x32x4                 y 2.7e-7 | 2.0e-7   dx 2.6e-7 | 3.0e-7   dw 8.9e-8 | 2.9e-8   db --
  spike_gemm fp32-spikes 2x40x72x36            y 1.5e-7 | 1.5e-7   dx 1.9e-7 | 1.7e-7   dw 1.4e-7 | 9.7e-8   db --
  spike_gemm fp32-spikes 2x64x128x36           y 9.5e-8 | 1.9e-7   dx 2.5e-7 | 2.0e-7   dw 1.3e-7 | 1.1e-7   db --
  spike_gemm fp32-spikes 512x128x32x4          y 2.2e-7 | 1.9e-7   dx 2.3e-7 | 2.4e-7   dw 1.2e-7 | 2.9e-8   db --
  spike_gemm fp32-spikes 512x256x32x4          y 2.7e-7 | 2.0e-7   dx 2.6e-7 | 3.0e-7   dw 1.2e-7 | 2.9e-8   db --
  spike_gemm fp32-spikes 2x20x64x256           y 1.8e-7 | 1.5e-7   dx 2.6e-7 | 2.2e-7   dw 5.3e-8 | 6.3e-8   db --
  spike_gemm fp32-spikes 2x130x72x36           y 2.6e-7 | 1.5e-7   dx 1.8e-7 | 2.2e-7   dw 1.4e-7 | 1.2e-7   db --
  spike_gemm fp32-spikes 1x260x256x64          y 1.3e-7 | 1.2e-7   dx 2.0e-7 | 1.7e-7   dw 2.2e-7 | 2.1e-7   db --
  spike_gemm bf16 2x20x64x256                  y 1.8e-7 | 1.5e-7   dx 2.6e-7 | 2.2e-7   dw 5.1e-8 | 6.3e-8   db --
  spike_gemm bf16 2x130x72x36                  y 2.6e-7 | 1.5e-7   dx 1.8e-7 | 2.2e-7   dw 1.4e-7 | 1.2e-7   db --
  spike_gemm bf16 1x260x256x16                 y 1.7e-7 | 1.3e-7   dx 1.6e-7 | 9.6e-8   dw 1.7e-7 | 1.7e-7   db --
  spike_gemm bf16 2x130x128x36                 y 2.1e-7 | 1.8e-7   dx 1.9e-7 | 1.9e-7   dw 1.8e-7 | 1.2e-7   db --
  spike_gemm bf16 2x128x256x64                 y 2.0e-7 | 1.1e-7   dx 2.0e-7 | 2.3e-7   dw 2.0e-7 | 1.4e-7   db --
  spike_gemm bf16 2x8x72x36                    y 1.3e-7 | 1.2e-7   dx 1.7e-7 | 1.7e-7   dw 1.2e-7 | 7.3e-8   db --
  spike_gemm bf16 2x64x32x136                  y 2.0e-7 | 1.5e-7   dx 1.9e-7 | 1.9e-7   dw 7.4e-8 | 9.3e-8   db --
  spike_gemm bf16 1x512x72x36                  y 1.9e-7 | 1.8e-7   dx 1.0e-7 | 1.3e-7   dw 2.0e-7 | 2.0e-7   db --
  dx_gemm ragged 2x40x72x10                    y --   dx 1.5e-7 | 1.7e-7   dw --   db --
  conv._gemm_nc 2x40x72x10 bias                y 9.6e-8 | 9.6e-8   dx 2.2e-7 | 1.9e-7   dw 1.3e-7 | 1.3e-7   db 4.1e-8 | 7.0e-8
  dense_gemm 2x1x40x72x136                     y 1.8e-7 | 2.4e-7   dx 2.3e-7 | 2.0e-7   dw 7.0e-8 | 1.1e-7   db --
  dense_gemm 2x1x64x128x136 stats              y 2.0e-7 | 2.8e-7   dx 2.9e-7 | 2.4e-7   dw 6.5e-8 | 1.1e-7   db --
  dense_gemm 2x3x40x72x136                     y 2.0e-7 | 2.4e-7   dx 2.4e-7 | 2.6e-7   dw 7.7e-8 | 1.2e-7   db --
  dense_gemm 2x2x32x96x256                     y 2.0e-7 | 2.2e-7   dx 3.5e-7 | 2.1e-7   dw 4.5e-8 | 7.4e-8   db --
  dense_gemm 8x2x72x40x3072                    y 3.3e-7 | 4.0e-7   dx 2.9e-7 | 3.2e-7   dw 2.2e-8 | 1.1e-8   db --
  dense_gemm 2x3x40x72x136 stats               y 2.0e-7 | 2.4e-7   dx 2.4e-7 | 2.6e-7   dw 7.7e-8 | 1.2e-7   db --
  dense_gemm 1x5x24x16x128                     y 2.8e-7 | 1.8e-7   dx 2.9e-7 | 1.8e-7   dw 8.3e-8 | 1.6e-7   db --
  dense_gemm 2x2x24x40x36                      y 1.8e-7 | 1.8e-7   dx 1.9e-7 | 1.9e-7   dw 1.3e-7 | 1.3e-7   db --
  dense_gemm 2x2x24x40x130                     y 1.9e-7 | 1.9e-7   dx 2.0e-7 | 2.0e-7   dw 1.1e-7 | 1.1e-7   db --
  siblings G=3 2x64x64x100                     y 2.1e-7 | 2.0e-7   dx 2.3e-7 | 2.3e-7   dw 1.2e-7 | 1.1e-7   db --
  separate G=3 2x64x64x100                     y --   dx --   dw 8.3e-8 | 1.1e-7   db --
  siblings G=1 2x64x64x100                     y 1.8e-7 | 2.0e-7   dx 2.8e-7 | 1.7e-7   dw 7.5e-8 | 9.1e-8   db --
  separate G=1 2x64x64x100                     y --   dx --   dw 1.2e-7 | 9.1e-8   db --
  siblings G=4 2x64x64x100                     y 2.0e-7 | 1.9e-7   dx 2.4e-7 | 2.9e-7   dw 1.1e-7 | 1.1e-7   db --
  separate G=4 2x64x64x100                     y --   dx --   dw 9.1e-8 | 1.1e-7   db --
  siblings G=3 2x40x72x36                      y 1.7e-7 | 2.0e-7   dx 1.9e-7 | 1.8e-7   dw 1.6e-7 | 1.6e-7   db --
  separate G=3 2x40x72x36                      y --   dx --   dw 1.6e-7 | 1.6e-7   db --
  siblings G=2 2x64x128x136                    y 2.1e-7 | 2.4e-7   dx 2.2e-7 | 2.2e-7   dw 1.0e-7 | 1.6e-7   db --
  separate G=2 2x64x128x136                    y --   dx --   dw 1.0e-7 | 1.6e-7   db --
  siblings G=2 8x130x128x4096                  y 3.6e-7 | 3.4e-7   dx --   dw --   db --
  bmm_small plain 3x65x17x66                   y 1.8e-7 | 1.8e-7   dx --   dw --   db --
  bmm_small a-transposed 3x65x17x66            y 1.6e-7 | 1.6e-7   dx --   dw --   db --
  bmm_small b-transposed 3x65x17x66            y 1.6e-7 | 1.6e-7   dx --   dw --   db --
  bmm_small a-batch-expanded 3x65x17x66        y 2.2e-7 | 2.2e-7   dx --   dw --   db --
  bmm_small b-batch-expanded 3x65x17x66        y 2.2e-7 | 2.2e-7   dx --   dw --   db --
  bmm_small slices 3x65x17x66                  y 1.6e-7 | 1.6e-7   dx --   dw --   db --
  bmm_small reduce-batch 3x65x17x66            y 1.8e-7 | 9.7e-8   dx --   dw --   db --
  bmm_small n1 3x65x17x1                       y 1.1e-7 | 1.2e-7   dx --   dw --   db --
  bmm_small m1 3x1x17x66                       y 2.0e-7 | 1.1e-7   dx --   dw --   db --
  i.e. every route is a factor of 5 or more inside its bound (the worst: 3.6e-7 against 2e-6, 3.5e-7 against 4e-6) and within 4.3x of
  the plain fp32 evaluation.  The dw figures move in the last digit from run to run (atomic adds), y and dx repeat.

Not reached here: the settled switches in their off position (SPIKE_GEMM_ENABLED, DENSE_GROUPED, DW_PIPE, BN_PARTIALS = False and
SPIKE_GEMM_TERMS < 3 send a row to a route another row already takes); the eval fusions gemm_bn_lif_eval / dense_gemm_bn_lif_eval,
which existing tests pin bit for bit to the unfused path this suite pins; weight gradients on the side stream (WGRAD_STREAM, off
since its measurement); the SPIKE_GEMM_CHECK assertion; the early returns for gy is None; the token-major linear layers and the mask
contraction, which have their own suites."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref  # noqa: E402
from gemm_ref import draw_eighths, draw_spikes, grid, one_hot, selection, wide_values  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1          # include/s2f.h
# every launch ops/gemm.py (and the queues of ops/core.py) can make for a 1x1 product
CENSUS = ("pgemm_nn_bf16", "pgemm_nn_bf16_stats", "pgemm_nn_bf16_grouped", "spike_gemm_fwd_bf16", "spike_gemm_fwd", "pgemm_dx_f32",
          "pgemm_dx_f32_stats", "pgemm_dx_f32_grouped", "spike_gemm_dw_bf16", "spike_gemm_dw", "spike_gemm_dw_pipe",
          "spike_gemm_dw_pipe_grouped", "spike_gemm_dw_grouped", "gemm_dw_general", "gemm_dw_general_grouped", "bmm_f32")
CONVERSIONS = ("pack_bf16x3", "split_bf16x3", "pack_bf16x3_multi", "split_bf16x3_multi")
SWITCHES = ("BN_PARTIALS_SINGLE", "DEFER_DW", "GRAD_SINKS")
NAMES = ("y", "dx", "dw", "db")
GRANULES = {"y": 64, "dx": 8, "dw": 8, "db": 8, "sum": 64, "squares": 4096}          # per unit
SPIKE_C, BMM_C = 2e-6, 4e-6


# -------------------------------------------------------------------------------------------------------------- the launchers' constants
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spike2former_amd", "csrc")
PGEMM, GEMM_BF16, GEMM, BMM = (open(os.path.join(_CSRC, n)).read() for n in ("pgemm.hip", "gemm_bf16.hip", "gemm.hip", "bmm.hip"))


def _ints(src, pattern):
    m = re.search(pattern, src)
    assert m, pattern
    return tuple(int(v) for v in m.groups())


def _int(src, pattern):
    return _ints(src, pattern)[0]


def _tiles(name):
    """{cfg: (MI, NJ, WMW, WNW, extra)} of a PgTile table of csrc/pgemm.hip"""
    body = re.search(r"constexpr PgTile %s\[\] = \{(.*?)\n\};" % name, PGEMM, re.S).group(1)
    return {int(t[0]): tuple(int(v) for v in t[1:]) for t in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", body)}


def _forms(name):
    """[(the form's fields as written, the set of its cfg_set(...))] of a form table of csrc/pgemm.hip"""
    body = re.search(r"constexpr \w+ %s\[\] = \{(.*?)\n\};" % name, PGEMM, re.S).group(1)
    return [(tuple(f.strip() for f in fields.split(",")), {int(c) for c in cfgs.split(",")})
            for fields, cfgs in re.findall(r"\{([^{}]*?), cfg_set\(([\d, ]+)\)\}", body)]


def _built(name, *fields):
    hit = [cfgs for f, cfgs in _forms(name) if f == tuple(str(v) for v in fields)]
    assert len(hit) == 1, (name, fields)
    return hit[0]


PK = _int(PGEMM, r"constexpr int PK = (\d+);")                                    # contraction elements per pack block
NN_LONG_K = _int(PGEMM, r"if \(K >= (\d+) && \(N & 7\) == 0\) return")             # pick_cfg_nn: the all-DMA tile from here
NN_T7 = _int(PGEMM, r"t7 = t7e \? atoll\(t7e\) : (\d+);")                           # ... the 128 x 128 rows tile from this many tiles
NN_G2_MAXWG = _int(PGEMM, r"atoll\(mw\) : (\d+)\);")                               # nn_super_steps: two steps up to this many workgroups
DX_T3 = _int(PGEMM, r"t3 = t3e \? atoll\(t3e\) : (\d+);")                           # pgemm_dx_impl: tile 3 from this many tiles
DX_KS4_MAXWG = _int(PGEMM, r"\(\(Ki \+ 63\) / 64\) <= (\d+)\) c = 10;")             # ... tile 10 up to this many workgroups
DX_SPLIT_MAXWG, DX_SPLIT_STEPS = _ints(PGEMM, r"wgs \* zsplit < (\d+) && steps / \(zsplit \* 2\) >= (\d+)\)")
NN_TILES, CONV_TILES, TN_TILES = _tiles("kNnTiles"), _tiles("kConvTiles"), _tiles("kTnTiles")
ROWS_TILES = {c for c, t in CONV_TILES.items() if t[4] == 0}                       # extra = CONV: the 1x1 rows forms
NN_PLAIN = _built("kNnForms", 3, 0, "false", "false")
ROWS_PLAIN, ROWS_G2 = (_built("kConvForms", 1, 0, "false", g, "false") & ROWS_TILES for g in (1, 2))          # (the rest: the 3x3 tiles)
ROWS_GROUPED, ROWS_GROUPED_G2 = (_built("kConvForms", 1, 0, "false", g, "true") & ROWS_TILES for g in (1, 2))
TN_STORE, TN_BETA, TN_SPLIT = (_built("kTnForms", e, "false", "false") for e in (0, 1, 2))
TN_GROUPED = _built("kTnForms", 0, "false", "true")
BK, BN = _int(GEMM_BF16, r"constexpr int BK = (\d+);"), _int(GEMM_BF16, r"constexpr int BN = (\d+);")
assert (BK, BN) == (_int(GEMM, r"constexpr int BK = (\d+);"), _int(GEMM, r"constexpr int BN = (\d+);"))
R2_MIN_BLOCKS = _int(GEMM_BF16, r'atoi\(getenv\("S2F_GEMM_MINBLOCKS"\)\) : (\d+);')
assert R2_MIN_BLOCKS == _int(GEMM, r"if \(blocks >= (\d+) \|\| cand == 1\)")
R2_THIN = _int(GEMM_BF16, r"const bool thin = wm == 1 && \(int64_t\)n_tiles \* m_tiles \* batch < (\d+);")
assert R2_THIN == _int(GEMM, r"const bool thin = wm == 1 && \(int64_t\)n_tiles \* m_tiles \* batch < (\d+);")
DW_DEMOTE_BL, DW_DEMOTE_MK = _ints(GEMM_BF16, r"\(int64_t\)batch \* L <= (\d+) && \(int64_t\)M \* K > (\d+)\) tm = 64;")
assert (DW_DEMOTE_BL, DW_DEMOTE_MK) == _ints(GEMM, r"\(int64_t\)batch \* L <= (\d+) && \(int64_t\)M \* K > (\d+)\) tm = 64;")
MAX_JOBS = _int(GEMM_BF16, r"constexpr int kMaxJobs = (\d+);")
BMM_TM, BMM_TN, BMM_TK = _ints(BMM, r"constexpr int kTM = (\d+), kTN = (\d+), kTK = (\d+);")
PGEMM_MIN_N = 128          # ops/gemm.py _PGEMM_MIN_N (asserted against the package in the dense rows)


def cdiv(a, b):
    return -(-a // b)


def up(a, b):
    return cdiv(a, b) * b


def tile_rows(tiles, cfg):
    MI, _, WMW, _, _ = tiles[cfg]
    return 32 * MI * WMW


# -------------------------------------------------------------------------------------------------------------- routes, from the shape
def nn_pg(L):
    """_spike_product: what the packed-weight pipeline takes of a bf16 spike map"""
    return L % 4 == 0 and L >= 8


def nn_cfg(B, M, K, L):
    """pick_cfg_nn"""
    tiles128 = cdiv(L, 128) * B * cdiv(M, 128)
    if K >= NN_LONG_K and L % 8 == 0:
        return 2
    return 7 if (M > 64 and tiles128 >= NN_T7) else (8 if (L >= 128 or M >= 64) else 6)


def nn_form(B, M, K, L):
    """pgemm_nn_impl -> ('dma', cfg, 1) for pg_nn_kernel or ('rows', tile, K steps per barrier) for pg_conv_kernel<CONV = false>"""
    c = nn_cfg(B, M, K, L)
    if c not in (6, 7, 8) and L % 8 == 0:
        return ("dma", c, 1)
    tile = c if c in (7, 8) else 6
    wgs, Kb = cdiv(L, 128) * cdiv(M, tile_rows(CONV_TILES, tile)) * B, cdiv(K, PK)
    two = tile in ROWS_G2 and Kb % 2 == 0 and Kb >= 4 and wgs <= NN_G2_MAXWG          # nn_super_steps, where the form is built
    return ("rows", tile, 2 if two else 1)


def r2_tile(B, M, K, L, bf16):
    """fwd_launch (gemm_bf16.hip) / spike_gemm_launch (gemm.hip) on the split [3, Mpad, Kpad] of ops.split_weight -> (wm, kg)"""
    Mpad, Kpad, n_tiles = up(M, 64), up(K, 32), cdiv(L, BN)
    wm = 1
    for cand in (4, 2, 1):
        if Mpad % (64 * cand) or (cand > 1 and M <= 32 * cand):
            continue
        if n_tiles * (Mpad // (64 * cand)) * B >= R2_MIN_BLOCKS or cand == 1:
            wm = cand
            break
    thin = wm == 1 and n_tiles * (Mpad // 64) * B < R2_THIN
    if not thin:
        return wm, 1
    if bf16:
        return wm, 4 if Kpad >= 16 * BK else 2 if Kpad >= 4 * BK else 1
    return wm, 2 if Kpad >= 4 * BK else 1


def dw_tile(B, M, K, L):
    """dw_launch / spike_dw_launch with x_terms 1 -> (rows of dY per tile, contraction step)"""
    tm = 32 if M <= 32 else 64 if M <= 64 else 128
    if tm == 128 and B * L <= DW_DEMOTE_BL and M * K > DW_DEMOTE_MK:
        tm = 64
    return tm, 64 if (L % 64 == 0 or L >= 512) else 32


def dw_pipe(ops, B, M, K, L):
    """_spike_dw: the pipelined kernel on its own (16-byte aligned operands)"""
    return bool(ops.DW_PIPE) and M >= 128 and K >= 128 and bool(ops.lib.s2f_spike_gemm_dw_pipe_ok(B, M, K, L))


def dx_form(B, Mo, Ki, N, beta=0.0, stats=False):
    """pgemm_dx_impl without a forced cfg -> (tile, contraction splits over gridDim.z)"""
    n_tiles = cdiv(N, 128)
    c = 5 if Ki <= 32 else 3 if (Ki > 64 and n_tiles * B * cdiv(Ki, 128) >= DX_T3) else (7 if beta == 0.0 else 4)
    if c == 7 and Mo >= 128 and n_tiles * B * cdiv(Ki, 64) <= DX_KS4_MAXWG:
        c = 10
    wgs, steps, z = n_tiles * B * cdiv(Ki, 64), cdiv(Mo, 16), 1
    while beta in (0.0, 1.0) and not stats and wgs * z < DX_SPLIT_MAXWG and steps // (z * 2) >= DX_SPLIT_STEPS:
        z *= 2
    return (4, z) if z > 1 else (c, 1)


def dxg_cfg(B, Mo, Ki, N):
    """s2f_pgemm_dx_f32_grouped: the tile rule of the single product, per group"""
    return 5 if Ki <= 32 else 3 if (Ki > 64 and cdiv(N, 128) * B * cdiv(Ki, 128) >= DX_T3) else 7


def dense_fast(L):
    return L % 4 == 0 and L >= PGEMM_MIN_N


# -------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    assert ops._PGEMM_MIN_N == PGEMM_MIN_N
    return ops


@pytest.fixture
def census(ops, monkeypatch):
    """{symbol without its s2f_ prefix: [argument tuples]} of every call since the last clear()"""
    calls = {}

    def wrap(name, fn):
        def counted(*a):
            calls.setdefault(name, []).append(a)
            return fn(*a)
        return counted
    for name in CENSUS + CONVERSIONS:
        monkeypatch.setattr(ops.lib, "s2f_" + name, wrap(name, getattr(ops.lib, "s2f_" + name)))
    return calls


@pytest.fixture
def switches(ops):
    """set(NAME=value, ...) for the switches a row needs; every switch of SWITCHES is put back and the deferred queue dropped"""
    old = {k: getattr(ops, k) for k in SWITCHES}

    def set_(**kw):
        for k, v in kw.items():
            assert k in SWITCHES, k
            setattr(ops, k, v)
    try:
        yield set_
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
        ops.wgrad_drop()


def counts(census):
    return {k: len(v) for k, v in census.items() if v and k in CENSUS}


def conversions(census):
    return {k: len(v) for k, v in census.items() if v and k in CONVERSIONS}


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# -------------------------------------------------------------------------------------------------------------- draws
def draw_product(shape, kind, seed, bias, exact, G=1):
    """-> x [B, G K, L], ws (G x [M, K]), bias [G M] or None, gy [B, G M, L] in fp64 (fp32 values); kind: 'bf16' / 'fp32-spikes' (a
    spike map) or 'dense' (a general fp32 map)"""
    B, M, K, L = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g).double()
    if kind == "dense":
        x = draw_eighths(g, B, G * K, L) if exact else r(B, G * K, L)
    else:
        x = draw_spikes(g, B, G * K, L)
    if exact:
        return x, [draw_eighths(g, M, K) for _ in range(G)], (draw_eighths(g, G * M) if bias else None), grid(g, -2, 2, B, G * M, L)
    return x, [(r(M, K) * K ** -0.5).float().double() for _ in range(G)], (r(G * M) if bias else None), r(B, G * M, L)


def assert_sums_exact(sums):
    for name, a in sums.items():
        if a is None:
            continue
        for t in (a if isinstance(a, list) else [a]):
            assert t.max().item() * GRANULES[name] < 2 ** 24, name


def stacked(d):
    """a result of gemm_ref.product with the list of weight gradients as one tensor [G, M, K]"""
    return {k: (torch.stack(v, 0) if isinstance(v, list) else v) for k, v in d.items()}


# -------------------------------------------------------------------------------------------------------------- runners
def to_spikes(ops, t):
    """fp64 map of multiples of 1/8 in [0, 1] -> (fp32 leaf, bf16 Spikes with its autograd handle): Q_IFNode(8 (k / 8)) = k / 8, and
    d Q_IFNode(8 src) / d src = 8 (1 / 8) = 1 on [0, 1], so src.grad is the gradient of the spike map, bit for bit"""
    src = t.float().cuda().requires_grad_(True)
    s, _ = ops.lif(src * 8.0, None, keep_v=False, spikes=True)
    assert isinstance(s, ops.Spikes) and s.tok is not None and s.data.dtype == torch.bfloat16
    assert torch.equal(s.data.float(), src.detach())
    return src, s


def plain_spikes(ops, t):
    """the same map as a Spikes whose handle asks for no gradient"""
    data = t.to(torch.bfloat16).cuda()
    assert torch.equal(data.double().cpu(), t)
    return ops.Spikes(data, ops._new_tok(data))


def operand(ops, x, kind, grad=True):
    """-> (the fp32 leaf that receives dx or None, what the op is handed)"""
    if kind == "bf16":
        return to_spikes(ops, x) if grad else (None, plain_spikes(ops, x))
    src = x.float().cuda().requires_grad_(grad)
    return src, src


def leaves(ws64):
    return [torch.nn.Parameter(w.float().cuda()) for w in ws64]


def run_product(ops, census, shape, kind, draw, stats=False, ws=None, backward=1, dx=True, w_as="list"):
    """ops.spike_gemm (a spike map, one weight) or ops.dense_gemm (kind 'dense', G weights) -> ({y, dx, dw [G, M, K], db} (None: no
    gradient arrived), the BatchNorm partials handed over with y or None, the launch counts); `backward`: how many times the
    backward pass runs; `dx`: whether the map asks for its gradient; `w_as`: how dense_gemm is handed its weights"""
    B, M, K, L = shape
    x64, ws64, b64, gy64 = draw
    G = len(ws64)
    ws = leaves(ws64) if ws is None else ws
    stack = None
    b = None if b64 is None else torch.nn.Parameter(b64.float().cuda())
    src, xin = operand(ops, x64, kind, grad=dx and gy64 is not None)
    census.clear()
    if kind == "dense":
        assert b is None
        if w_as == "stack":
            stack = torch.nn.Parameter(torch.stack([w.detach() for w in ws], 0))
            y = ops.dense_gemm(xin, stack, stats=stats)
        else:
            y = ops.dense_gemm(xin, ws[0] if (w_as == "matrix" and G == 1) else list(ws), stats=stats)
        fn = "_DenseGemm"
    else:
        assert G == 1
        y = ops.spike_gemm(xin, ws[0], b, stats=stats)
        fn = "_SpikeGemm"
    assert y.shape == (B, G * M, L) and y.dtype == torch.float32
    part = ops.stats_of(y)
    if gy64 is not None:
        assert type(y.grad_fn).__name__.startswith(fn), type(y.grad_fn).__name__
        for i in range(backward):
            y.backward(gy64.float().cuda(), retain_graph=i + 1 < backward)
    if stack is not None:
        dw = stack.grad
    else:
        dw = None if any(w.grad is None for w in ws) else torch.stack([w.grad for w in ws], 0)
    got = {"y": y.detach(), "dx": None if src is None else src.grad, "dw": dw, "db": None if b is None else b.grad}
    return got, part, counts(census)


def describe(name, err, bad):
    """the worst entry with its index, the number of entries off, and the first and last row and column of a matrix on their own"""
    e = err.detach()
    idx = tuple(int(i) for i in torch.unravel_index(e.argmax(), e.shape))
    msg = f"{name}: {int(bad.sum())} of {bad.numel()} entries off, worst {e.max().item():.3e} at {idx}"
    if e.dim() >= 2 and e.shape[-1] > 1 and e.shape[-2] > 1:
        edges = {"first row": (Ellipsis, 0, slice(None)), "last row": (Ellipsis, -1, slice(None)),
                 "first column": (Ellipsis, slice(None), 0), "last column": (Ellipsis, slice(None), -1)}
        msg += "; " + ", ".join(f"{k} {int(bad[i].sum())} off (worst {e[i].max().item():.3e})" for k, i in edges.items())
    return msg


def assert_equal64(got, want, names):
    for name in names:
        a, b = got[name], want[name]
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        a = a.detach().cpu().double()
        assert torch.equal(a, b), describe(name, (a - b).abs(), a != b)


def assert_within(label, got, ref64, ref32, sums, c, names):
    """per entry |got - ref64| <= c A + 1e-30; prints the worst |err| / A of the kernel and of the plain fp32 evaluation"""
    failed = []
    for name in names:
        if ref64[name] is None:
            assert got[name] is None, name
            continue
        A = sums[name]
        assert got[name] is not None and got[name].dtype == torch.float32 and got[name].shape == ref64[name].shape, name
        err = (got[name].detach().cpu().double() - ref64[name]).abs()
        err32 = (ref32[name].double() - ref64[name]).abs()
        print(f"ratio {label} {name}: kernel {(err / (A + 1e-300)).max().item():.2e}  fp32-cpu {(err32 / (A + 1e-300)).max().item():.2e}"
              f"  bound {c[name]:.1e}")
        over = err - c[name] * A
        if over.max().item() > 1e-30:
            failed.append(describe(name, over.clamp_min(0), over > 1e-30))
    assert not failed, failed


def assert_partials(ops, part, y, exact):
    """the BatchNorm partials handed over with y [B, M, L]: [M, B ceil(L / 128), 2] fp32 (sum, sum of squares) per tile of 128 columns.
    Exact draw: the tile sums of |y| below 2^24 granules of 1/64 and those of y^2 below 2^24 granules of 1/4096 (asserted), so the
    partials EQUAL the fp64 tile sums.  General draw: within 1e-5 of the tile sums of |y| resp. y^2 of the kernel's own y."""
    B, M, L = y.shape
    P = int(ops.lib.s2f_bn_partials_count(B, L))
    assert P == B * cdiv(L, gemm_ref.TILE)
    assert part is not None and tuple(part.shape) == (M, P, 2) and part.dtype == torch.float32
    s64, a64 = gemm_ref.partials64(y)
    got = part.detach().cpu().double()
    if exact:
        assert a64[..., 0].max().item() * GRANULES["sum"] < 2 ** 24 and a64[..., 1].max().item() * GRANULES["squares"] < 2 ** 24
        assert torch.equal(gemm_ref.partials(y).double(), s64)
        assert torch.equal(got, s64), describe("partials", (got - s64).abs(), got != s64)
    else:
        over = (got - s64).abs() - 1e-5 * a64
        assert over.max().item() <= 1e-30, describe("partials", over.clamp_min(0), over > 1e-30)


def single_pass_switch(ops, switches, B, M, L):
    """a map this BatchNorm would take in one pass stores partials only under BN_PARTIALS_SINGLE: ask the library, set it if so"""
    assert ops.BN_PARTIALS
    if ops.lib.s2f_bn_single_pass(B, M, L):
        switches(BN_PARTIALS_SINGLE=True)


# -------------------------------------------------------------------------------------------------------------- spike_gemm
#   id, (B, M, K, L), operand, the inequality of the route, the launches, (c of y, c of dw), bias, stats, backward
_DX = {"pgemm_dx_f32": 1}
_PG, _R2, _F32 = {"pgemm_nn_bf16": 1}, {"spike_gemm_fwd_bf16": 1}, {"spike_gemm_fwd": 1}
_DW_R2, _DW_PIPE, _DW_F32 = {"spike_gemm_dw_bf16": 1}, {"spike_gemm_dw_pipe": 1}, {"spike_gemm_dw": 1}


def _row(id_, shape, kind, route, launches, c=(SPIKE_C, SPIKE_C), bias=False, stats=False, backward=True):
    return pytest.param(shape, kind, bias, stats, route, launches, c, backward, id=id_)


def _nn(o, s, form, dx=None, dw=None):
    """a bf16 row: the forward form of s2f_pgemm_nn_bf16, the tile of the input gradient, (rows, step) of the weight gradient or 'pipe'"""
    B, M, K, L = s
    ok = nn_pg(L) and nn_form(*s) == form
    if dx is not None:
        ok = ok and L % 4 == 0 and dx_form(B, M, K, L) == dx
    if dw == "pipe":
        ok = ok and dw_pipe(o, *s)
    elif dw is not None:
        ok = ok and M >= 16 and not dw_pipe(o, *s) and dw_tile(*s) == dw
    return ok


def _r2(o, s, bf16, tile, dw=None):
    """a row on the round-2 kernels: (wm, kg) of the forward, (rows, step) of the weight gradient"""
    B, M, K, L = s
    ok = L % 4 == 0 and (not bf16 or not nn_pg(L)) and r2_tile(B, M, K, L, bf16) == tile
    if dw is not None:
        ok = ok and M >= 16 and not (bf16 and dw_pipe(o, *s)) and dw_tile(*s) == dw
    return ok


ROW_TILE6 = _row("rows-tile-6-n-mod-8-is-4", (2, 40, 72, 36), "bf16",
                 lambda o, *s: s[1] < 64 and s[3] < 128 and s[3] % 8 == 4 and _nn(o, s, ("rows", 6, 1), (7, 1), (64, 32)),
                 {**_PG, **_DX, **_DW_R2})
ROW_TILE8_G2 = _row("rows-tile-8-two-steps-dw-tm64-32-wide", (2, 64, 128, 136), "bf16",
                    lambda o, *s: cdiv(s[2], PK) == 4 and _nn(o, s, ("rows", 8, 2), (7, 1), (64, 32)), {**_PG, **_DX, **_DW_R2})
ROW_PIPE_RAGGED = _row("dw-pipelined-ragged-dx-tile-10", (2, 130, 128, 36), "bf16",
                       lambda o, *s: s[3] % 32 != 0 and _nn(o, s, ("rows", 8, 2), (10, 1), "pipe"), {**_PG, **_DX, **_DW_PIPE})
ROW_L4_KG2 = _row("round2-l4-kg2", (2, 64, 128, 4), "bf16", lambda o, *s: _r2(o, s, True, (1, 2), (64, 32)), {**_R2, **_DX, **_DW_R2})
SPIKE_ROWS = [
    ROW_TILE6,
    ROW_TILE8_G2,
    _row("rows-tile-8-one-step-odd-kb", (1, 100, 96, 132), "bf16",
         lambda o, *s: cdiv(s[2], PK) % 2 == 1 and _nn(o, s, ("rows", 8, 1), (7, 1), (128, 32)), {**_PG, **_DX, **_DW_R2}),
    _row("rows-tile-7-two-steps-512-tiles-dx-tile-3", (8, 130, 128, 4096), "bf16",
         lambda o, *s: cdiv(s[3], 128) * s[0] * cdiv(s[1], 128) == NN_T7 and _nn(o, s, ("rows", 7, 2), (3, 1), "pipe"),
         {**_PG, **_DX, **_DW_PIPE}),
    _row("rows-tile-8-just-below-496-tiles-one-step", (8, 130, 128, 3968), "bf16",
         lambda o, *s: cdiv(s[3], 128) * s[0] * cdiv(s[1], 128) == NN_T7 - 16 and cdiv(s[3], 128) * s[0] * cdiv(s[1], 64) > NN_G2_MAXWG
         and _nn(o, s, ("rows", 8, 1), (3, 1), "pipe"), {**_PG, **_DX, **_DW_PIPE}),
    _row("all-dma-tile-k1024", (1, 40, 1024, 136), "bf16",
         lambda o, *s: s[2] >= NN_LONG_K and s[3] % 8 == 0 and _nn(o, s, ("dma", 2, 1), (7, 1), (64, 32)), {**_PG, **_DX, **_DW_R2}),
    _row("k1024-n-mod-8-is-4-register-staged", (1, 40, 1024, 132), "bf16",
         lambda o, *s: s[2] >= NN_LONG_K and s[3] % 8 == 4 and _nn(o, s, ("rows", 8, 2), (7, 1), (64, 32)), {**_PG, **_DX, **_DW_R2}),
    _row("bias-db-and-no-partials", (2, 40, 72, 36), "bf16", lambda o, *s: _nn(o, s, ("rows", 6, 1), (7, 1), (64, 32)),
         {**_PG, **_DX, **_DW_R2}, bias=True, stats=True),
    _row("stats", (2, 64, 128, 136), "bf16", lambda o, *s: _nn(o, s, ("rows", 8, 2), (7, 1), (64, 32)),
         {"pgemm_nn_bf16_stats": 1, **_DX, **_DW_R2}, stats=True),
    # the round-2 bf16 kernel: rows of L = 4 (less than the 8 columns the packed-weight pipeline asks for)
    _row("round2-l4-kg1-dx-tile-5", (2, 64, 32, 4), "bf16", lambda o, *s: _r2(o, s, True, (1, 1), (64, 32)) and dx_form(*s) == (5, 1),
         {**_R2, **_DX, **_DW_R2}),
    ROW_L4_KG2,
    _row("round2-l4-kg4", (1, 40, 512, 4), "bf16", lambda o, *s: _r2(o, s, True, (1, 4), (64, 32)), {**_R2, **_DX, **_DW_R2}),
    _row("round2-wm2-512-workgroups", (512, 128, 32, 4), "bf16",
         lambda o, *s: s[0] * cdiv(s[3], BN) == R2_MIN_BLOCKS and _r2(o, s, True, (2, 1), (128, 32)), {**_R2, **_DX, **_DW_R2}),
    _row("round2-wm4-512-workgroups", (512, 256, 32, 4), "bf16",
         lambda o, *s: s[0] * cdiv(s[3], BN) == R2_MIN_BLOCKS and _r2(o, s, True, (4, 1), (128, 32)), {**_R2, **_DX, **_DW_R2}),
    # an fp32 spike tensor: the branches of _spike_product / _spike_dw the convolution suite lists as not reached
    _row("fp32-spikes-kg1-dw-tm64", (2, 40, 72, 36), "fp32-spikes", lambda o, *s: _r2(o, s, False, (1, 1), (64, 32)),
         {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-kg2", (2, 64, 128, 36), "fp32-spikes", lambda o, *s: _r2(o, s, False, (1, 2), (64, 32)), {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-wm2", (512, 128, 32, 4), "fp32-spikes", lambda o, *s: _r2(o, s, False, (2, 1), (128, 32)),
         {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-wm4", (512, 256, 32, 4), "fp32-spikes", lambda o, *s: _r2(o, s, False, (4, 1), (128, 32)),
         {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-dw-tm32-64-wide", (2, 20, 64, 256), "fp32-spikes", lambda o, *s: _r2(o, s, False, (1, 1), (32, 64)),
         {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-dw-tm128-dx-tile-10", (2, 130, 72, 36), "fp32-spikes",
         lambda o, *s: _r2(o, s, False, (1, 1), (128, 32)) and dx_form(*s) == (10, 1), {**_F32, **_DX, **_DW_F32}),
    _row("fp32-spikes-dw-demoted-128-to-64", (1, 260, 256, 64), "fp32-spikes",
         lambda o, *s: s[0] * s[3] <= DW_DEMOTE_BL and s[1] * s[2] > DW_DEMOTE_MK and s[1] > 64 and _r2(o, s, False, (1, 2), (64, 64)),
         {**_F32, **_DX, **_DW_F32}),
    # the weight gradient of a bf16 map
    _row("dw-tm32-64-wide", (2, 20, 64, 256), "bf16", lambda o, *s: _nn(o, s, ("rows", 8, 1), (7, 1), (32, 64)), {**_PG, **_DX, **_DW_R2}),
    _row("dw-tm128-k-below-128-dx-tile-10", (2, 130, 72, 36), "bf16",
         lambda o, *s: s[2] < 128 and o.lib.s2f_spike_gemm_dw_pipe_ok(*s) and _nn(o, s, ("rows", 8, 1), (10, 1), (128, 32)),
         {**_PG, **_DX, **_DW_R2}),
    _row("dw-demoted-l16-not-pipelined", (1, 260, 256, 16), "bf16",
         lambda o, *s: s[3] < 32 and not o.lib.s2f_spike_gemm_dw_pipe_ok(*s) and s[1] * s[2] > DW_DEMOTE_MK
         and _nn(o, s, ("rows", 8, 2), (10, 1), (64, 32)), {**_PG, **_DX, **_DW_R2}),
    ROW_PIPE_RAGGED,
    _row("dw-pipelined-whole-32-column-steps", (2, 128, 256, 64), "bf16",
         lambda o, *s: s[3] % 32 == 0 and _nn(o, s, ("rows", 8, 2), (10, 1), "pipe"), {**_PG, **_DX, **_DW_PIPE}),
    _row("dw-m-below-16-on-bmm", (2, 8, 72, 36), "bf16", lambda o, *s: s[1] < 16 and _nn(o, s, ("rows", 6, 1), (7, 1)),
         {**_PG, **_DX, "bmm_f32": 1}, c=(SPIKE_C, BMM_C)),
    # the input gradient
    _row("dx-tile-5-ki32", (2, 64, 32, 136), "bf16", lambda o, *s: s[2] <= 32 and _nn(o, s, ("rows", 8, 1), (5, 1), (64, 32)),
         {**_PG, **_DX, **_DW_R2}),
    _row("dx-contraction-split-over-gridz", (1, 512, 72, 36), "bf16",
         lambda o, *s: cdiv(s[1], 16) == 32 and _nn(o, s, ("rows", 8, 1), (4, 2), (128, 32)), {**_PG, **_DX, **_DW_R2}),
]


def _spike_case(ops, switches, census, shape, kind, bias, stats, on_route, launches, backward, seed, exact):
    B, M, K, L = shape
    assert on_route(ops, *shape), "the shape left its route: see the launch rule restated above"
    wants_part = stats and not bias
    if wants_part:
        single_pass_switch(ops, switches, B, M, L)
    draw = draw_product(shape, kind, seed, bias, exact)
    if not backward:
        draw = draw[:3] + (None,)
    sums = gemm_ref.abs_sums(gemm_ref.product, *draw)
    if exact:
        assert_sums_exact(sums)
    got, part, launched = run_product(ops, census, shape, kind, draw, stats=stats)
    assert launched == launches, launched
    for name, a in census.items():          # no launch adds into anything: there is no sink
        if name in ("spike_gemm_dw_bf16", "gemm_dw_general"):
            assert all(args[-2] == 0 for args in a), name
        if name == "spike_gemm_dw":
            assert all(args[-3] == 0 and args[-2] == 1 for args in a), name          # accumulate, x_terms
        if name == "spike_gemm_dw_pipe":
            assert all(args[7] == 0 for args in a), name
        if name == "bmm_f32" and kind != "dense":
            assert all(args[-2] == 1 for args in a), name          # reduce_batch
    if wants_part:
        # the partials, and y bit for bit what the launch without them stores
        assert_partials(ops, part, got["y"], exact)
        plain, none, _ = run_product(ops, census, shape, kind, draw[:3] + (None,), stats=False)
        assert none is None and torch.equal(plain["y"], got["y"])
    else:
        assert part is None
    return draw, stacked(sums), got


@pytest.mark.parametrize("shape,kind,bias,stats,on_route,launches,c,backward", SPIKE_ROWS)
def test_spike_gemm_route_equals_fp64(ops, switches, census, shape, kind, bias, stats, on_route, launches, c, backward):
    draw, _, got = _spike_case(ops, switches, census, shape, kind, bias, stats, on_route, launches, backward, sum(shape) + int(bias), True)
    assert_equal64(got, stacked(gemm_ref.product(*draw)), NAMES)


@pytest.mark.parametrize("shape,kind,bias,stats,on_route,launches,c,backward", SPIKE_ROWS)
def test_spike_gemm_route_general_operands_within_the_fp32_bound(ops, switches, census, shape, kind, bias, stats, on_route, launches, c,
                                                                  backward):
    draw, sums, got = _spike_case(ops, switches, census, shape, kind, bias, stats, on_route, launches, backward, sum(shape) + 1000, False)
    assert_within("spike_gemm " + kind + " " + "x".join(map(str, shape)) + (" bias" if bias else "") + (" stats" if stats else ""), got,
                  stacked(gemm_ref.product(*draw)), stacked(gemm_ref.product(*draw, torch.float32)), sums,
                  {"y": c[0], "dx": BMM_C, "dw": c[1], "db": SPIKE_C}, NAMES)


def test_contraction_split_fills_its_output_with_zeros_every_time(ops, switches, census):
    """the split form adds its partial products with atomics into a zero-filled dx: two runs into the SAME allocation (the second
    over the first one's result) both EQUAL fp64 -- a missing fill would leave twice the gradient"""
    from spike2former_amd._lib import check
    B, M, K, L = shape = (1, 512, 72, 36)
    assert dx_form(B, M, K, L) == (4, 2) and 4 in TN_SPLIT
    x64, ws64, _, gy64 = draw_product(shape, "bf16", 77, False, True)
    ref = gemm_ref.product(x64, ws64, None, gy64)["dx"]
    pack, gy = ops.pack_weight(ws64[0].float().cuda()), gy64.float().cuda()
    dx = torch.full((B, K, L), float("nan"), device="cuda")
    for _ in range(2):
        census.clear()
        check(ops.lib.s2f_pgemm_dx_f32(pack.data_ptr(), gy.data_ptr(), 0, dx.data_ptr(), 0, B, M, K, L, 0.0, 0, stream()), "dx")
        assert counts(census) == _DX
        assert_equal64({"dx": dx}, {"dx": ref}, ("dx",))
    # beta = 1: the atomics ARE the accumulation
    check(ops.lib.s2f_pgemm_dx_f32(pack.data_ptr(), gy.data_ptr(), 0, dx.data_ptr(), 0, B, M, K, L, 1.0, 0, stream()), "dx")
    assert_equal64({"dx": dx}, {"dx": 2 * ref}, ("dx",))


def test_input_gradient_of_ragged_rows_runs_on_bmm(ops, switches, census):
    """N % 4 != 0: dx_gemm leaves the packed-weight kernel for one strided product on s2f_bmm_f32 (W^T expanded over the batch)"""
    B, M, K, L = shape = (2, 40, 72, 10)
    for exact in (True, False):
        _, ws64, _, gy64 = draw_product(shape, "bf16", 5 + exact, False, exact)
        census.clear()
        dx = ops.dx_gemm(ws64[0].float().cuda(), gy64.float().cuda())
        assert counts(census) == {"bmm_f32": 1} and census["bmm_f32"][0][-2] == 0
        ref = gemm_ref.bmm(ws64[0].t().expand(B, K, M), gy64)
        A = gemm_ref.abs_sums(gemm_ref.bmm, ws64[0].t().expand(B, K, M), gy64)
        if exact:
            assert A.max().item() * 8 < 2 ** 24
            assert_equal64({"dx": dx}, {"dx": ref}, ("dx",))
        else:
            assert_within("dx_gemm ragged 2x40x72x10", {"dx": dx}, {"dx": ref},
                          {"dx": gemm_ref.bmm(ws64[0].t().expand(B, K, M), gy64, False, torch.float32)}, {"dx": A}, {"dx": BMM_C}, ("dx",))


def test_pipeline_refused_by_alignment_takes_the_round2_weight_gradient(ops, switches, census):
    """a bf16 map whose address is 8 but not 16 bytes aligned (a slice of a larger map): the LDS-DMA pipeline copies 16-byte pieces,
    so _spike_dw launches s2f_spike_gemm_dw_bf16, which reads 8-byte pieces -- on the shape whose aligned twin is pipelined"""
    shape, kind, _, _, on_route, launches, _, _ = ROW_PIPE_RAGGED.values
    B, M, K, L = shape
    assert on_route(ops, *shape) and launches["spike_gemm_dw_pipe"] == 1
    x64, ws64, _, gy64 = draw_product(shape, kind, 61, False, True)
    sums = gemm_ref.abs_sums(gemm_ref.product, x64, ws64, None, gy64)
    assert_sums_exact(sums)
    ref = gemm_ref.product(x64, ws64, None, gy64)["dw"][0]
    flat = torch.zeros(B * K * L + 4, dtype=torch.bfloat16, device="cuda")
    x = flat[4:].view(B, K, L)
    x.copy_(x64.to(torch.bfloat16))
    assert x.data_ptr() % 16 == 8 and x.is_contiguous()
    w, gy = ws64[0].float().cuda(), gy64.float().cuda()
    census.clear()
    dw = ops._spike_dw(gy, x, w, B, M, K, L, pipe=True)
    assert counts(census) == _DW_R2, counts(census)
    assert_equal64({"dw": dw}, {"dw": ref}, ("dw",))
    census.clear()
    aligned = x.clone()
    assert aligned.data_ptr() % 16 == 0
    dw = ops._spike_dw(gy, aligned, w, B, M, K, L, pipe=True)
    assert counts(census) == _DW_PIPE, counts(census)
    assert_equal64({"dw": dw}, {"dw": ref}, ("dw",))


# ---- three terms
def _one_product_per_entry(op, args, name):
    ref, A = op(*args), gemm_ref.abs_sums(op, *args)
    r, a = ref[name], A[name]
    r, a = (torch.stack(r, 0), torch.stack(a, 0)) if isinstance(r, list) else (r, a)
    assert torch.equal(a, r.abs()) and bool((r != 0).any())
    return r


FORWARD_KERNELS = [
    pytest.param((1, 40, 1024, 136), "bf16", lambda s: nn_form(*s) == ("dma", 2, 1), _PG, id="pg_nn_kernel"),
    pytest.param((2, 64, 128, 136), "bf16", lambda s: nn_form(*s) == ("rows", 8, 2), _PG, id="pg_conv_kernel-rows-form-two-steps"),
    pytest.param((2, 40, 72, 36), "bf16", lambda s: nn_form(*s) == ("rows", 6, 1), _PG, id="pg_conv_kernel-rows-form-tile-6"),
    pytest.param((8, 130, 128, 4096), "bf16", lambda s: nn_form(*s) == ("rows", 7, 2), _PG, id="pg_conv_kernel-rows-form-tile-7"),
    pytest.param((2, 64, 128, 4), "bf16", lambda s: not nn_pg(s[3]) and r2_tile(*s, True) == (1, 2), _R2, id="sgemm_bf16_kernel"),
    pytest.param((2, 64, 128, 36), "fp32-spikes", lambda s: r2_tile(*s, False) == (1, 2), _F32, id="spike_gemm_kernel"),
]


@pytest.mark.parametrize("shape,kind,on_kernel,launches", FORWARD_KERNELS)
def test_forward_needs_all_three_terms_of_the_weight(ops, switches, census, shape, kind, on_kernel, launches):
    """w with 20 significant bits, a spike map of one 1 per batch element: every non-zero output is ONE product w[m, k] * 1"""
    B, M, K, L = shape
    assert on_kernel(shape)
    g = torch.Generator().manual_seed(L + K)
    w, x = wide_values(g, M, K), one_hot(g, B, K, L)
    ref = _one_product_per_entry(gemm_ref.product, (x, [w], None, None), "y")
    with torch.no_grad():
        got, _, launched = run_product(ops, census, shape, kind, (x, [w], None, None))
    assert launched == launches, launched
    assert conversions(census) == ({"pack_bf16x3": 1} if "pgemm_nn_bf16" in launches else {"split_bf16x3": 1})
    assert_equal64(got, {"y": ref}, ("y",))


@pytest.mark.parametrize("shape,launches,kind", [pytest.param((2, 64, 128, 136), _PG, "pack", id="pack_multi_kernel"),
                                                 pytest.param((2, 64, 128, 4), _R2, "split", id="split_multi_kernel")])
def test_resplit_all_converts_all_three_terms(ops, switches, census, shape, launches, kind):
    """the two _multi kernels behind ops.resplit_all (what a captured step replays): the weight changes through `.data` (no version
    bump), so only resplit_all refreshes its cached conversion -- the product that follows converts nothing itself and must hold
    all 20 bits of the new weight"""
    B, M, K, L = shape
    g = torch.Generator().manual_seed(K + L)
    w0, w, x = draw_eighths(g, M, K), wide_values(g, M, K), one_hot(g, B, K, L)
    ref = _one_product_per_entry(gemm_ref.product, (x, [w], None, None), "y")
    wl = torch.nn.Parameter(w0.float().cuda())
    sp = plain_spikes(ops, x)
    with torch.no_grad():
        census.clear()
        ops.spike_gemm(sp, wl)
        assert counts(census) == launches and conversions(census) == {kind + "_bf16x3": 1}
        wl.data.copy_(w.float())
        census.clear()
        assert ops.resplit_all(wl.device) >= 1
        assert conversions(census).get(kind + "_bf16x3_multi") == 1, conversions(census)
        census.clear()
        y = ops.spike_gemm(sp, wl)
        assert counts(census) == launches and conversions(census) == {}
    assert_equal64({"y": y}, {"y": ref}, ("y",))


DX_FORMS = [
    pytest.param((2, 40, 72, 36), (7, 1), id="plain-tile-7"),
    pytest.param((2, 130, 72, 36), (10, 1), id="plain-tile-10"),
    pytest.param((2, 64, 32, 136), (5, 1), id="plain-tile-5"),
    pytest.param((8, 130, 128, 3072), (3, 1), id="plain-tile-3"),
    pytest.param((1, 512, 72, 36), (4, 2), id="contraction-split"),
]


@pytest.mark.parametrize("wide", ["w-through-the-pack", "gy-through-the-in-kernel-split"])
@pytest.mark.parametrize("shape,form", DX_FORMS)
def test_input_gradient_needs_all_three_terms_of_both_operands(ops, switches, census, shape, form, wide):
    """dx = W^T gy with ONE non-zero product per entry: the 20-bit values in w (three planes of the pack) against one gy entry of 1
    per batch element, then the 20-bit values in gy (split in pg_tn_f32_kernel) against a 0/1 selection matrix w"""
    B, M, K, L = shape
    assert dx_form(B, M, K, L) == form and (form[0] in (TN_SPLIT if form[1] > 1 else TN_STORE))
    g = torch.Generator().manual_seed(M + K + len(wide))
    if wide.startswith("w"):
        w, gy = wide_values(g, M, K), one_hot(g, B, M, L)
    else:
        w, gy = selection(g, M, K), wide_values(g, B, M, L)
    x = draw_spikes(g, B, K, L)
    ref = _one_product_per_entry(gemm_ref.product, (x, [w], None, gy), "dx")
    src, sp = to_spikes(ops, x)
    wl = w.float().cuda()          # no gradient asked for the weight: the input gradient alone is launched
    y = ops.spike_gemm(sp, wl)
    census.clear()
    y.backward(gy.float().cuda())
    assert counts(census) == _DX, counts(census)
    assert_equal64({"dx": src.grad}, {"dx": ref}, ("dx",))


DW_KERNELS = [
    pytest.param((2, 64, 128, 136), "bf16", _DW_R2, id="sgemm_dw_bf16_kernel-tm64-32-wide"),
    pytest.param((2, 20, 64, 256), "bf16", _DW_R2, id="sgemm_dw_bf16_kernel-tm32-64-wide"),
    pytest.param((2, 130, 72, 36), "bf16", _DW_R2, id="sgemm_dw_bf16_kernel-tm128"),
    pytest.param((2, 40, 72, 36), "fp32-spikes", _DW_F32, id="spike_gemm_dw_kernel-x-terms-1"),
    pytest.param((2, 130, 128, 36), "bf16", _DW_PIPE, id="pipelined-ragged"),
    pytest.param((2, 128, 256, 64), "bf16", _DW_PIPE, id="pipelined-whole-steps"),
]


def _wide_gy_one_hot_x(shape, seed):
    """gy with 20 significant bits, a spike map of one 1 per batch element (in a row of its own): dw[m, k] is ONE product"""
    B, M, K, L = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, K, L, dtype=torch.float64)
    for b, k in enumerate(torch.randperm(K, generator=g)[:B].tolist()):
        x[b, k, int(torch.randint(0, L, (1,), generator=g))] = 1.0
    return x, wide_values(g, B, M, L), draw_eighths(g, M, K)


@pytest.mark.parametrize("shape,kind,launches", DW_KERNELS)
def test_weight_gradient_needs_all_three_terms_of_the_gradient(ops, switches, census, shape, kind, launches):
    """dY is split hi + mid + lo inside every weight-gradient kernel"""
    B, M, K, L = shape
    assert dw_pipe(ops, *shape) == ("spike_gemm_dw_pipe" in launches)
    x, gy, w = _wide_gy_one_hot_x(shape, M + L)
    ref = _one_product_per_entry(gemm_ref.product, (x, [w], None, gy), "dw")
    got, _, launched = run_product(ops, census, shape, kind, (x, [w], None, gy), dx=False)
    assert {k: v for k, v in launched.items() if "dw" in k} == launches, launched
    assert_equal64(got, {"dw": ref}, ("dw",))


QUEUE_KERNELS = [
    pytest.param((2, 64, 128, 136), True, "spike_gemm_dw_pipe_grouped", (1, 0, 0), id="pipelined-grouped"),
    pytest.param((2, 40, 72, 16), True, "spike_gemm_dw_grouped", (1, 32), id="round2-grouped-32-wide"),
    pytest.param((2, 24, 40, 64), False, "spike_gemm_dw_grouped", (1, 64), id="round2-grouped-64-wide-map-8-byte-aligned"),
]


@pytest.mark.parametrize("shape,aligned,launch,args", QUEUE_KERNELS)
def test_queued_weight_gradient_needs_all_three_terms_of_the_gradient(ops, switches, census, shape, aligned, launch, args):
    """the grouped kernels of the deferred queue split dY themselves: ONE product per entry into a sink filled with zeros (0.75 plus
    a 20-bit value would round).  The 64-wide class is reached with a map the pipeline cannot read (8 but not 16 bytes aligned)"""
    B, M, K, L = shape
    assert ops.DEFER_DW and ops.DW_PIPE and (L % 64 == 0 or L >= 512) == (args[-1] == 64)
    x, gy, w64 = _wide_gy_one_hot_x(shape, M + L + 1)
    ref = _one_product_per_entry(gemm_ref.product, (x, [w64], None, gy), "dw")[0]
    w = torch.nn.Parameter(w64.float().cuda())
    with _Sink(ops, w) as sink:
        sink.views[0].zero_()
        flat = torch.zeros(B * K * L + 4, dtype=torch.bfloat16, device="cuda")
        xd = flat[(0 if aligned else 4):B * K * L + (0 if aligned else 4)].view(B, K, L)
        xd.copy_(x.to(torch.bfloat16))
        assert xd.data_ptr() % 16 == (0 if aligned else 8)
        assert ops._spike_dw(gy.float().cuda(), xd, w, B, M, K, L, pipe=True) is None
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {launch: 1}, counts(census)
        assert census[launch][0][1:-1] == args
        sink.holds(ref)


# ---- module level
def test_conv_module_sends_ragged_rows_to_dense_gemm_on_bmm(ops, switches, census):
    """spike2former_amd.conv._gemm_nc with bf16 Spikes of L = 10: L % 4 != 0 leaves spike_gemm for dense_gemm on the fp32 view of
    the spikes -- three s2f_bmm_f32 calls (forward, dx, dw over the batch), the bias added outside"""
    from spike2former_amd import conv
    B, M, K, L = shape = (2, 40, 72, 10)
    assert L % 4 != 0 and not dense_fast(L)
    for exact in (True, False):
        x64, ws64, b64, gy64 = draw = draw_product(shape, "bf16", 91 + exact, True, exact)
        sums = stacked(gemm_ref.abs_sums(gemm_ref.product, *draw))
        src, sp = to_spikes(ops, x64)
        w, b = torch.nn.Parameter(ws64[0].float().cuda()), torch.nn.Parameter(b64.float().cuda())
        census.clear()
        y = conv._gemm_nc(w, sp, b, spike_input=True, stats=True)
        assert ops.stats_of(y) is None
        y.backward(gy64.float().cuda())
        assert counts(census) == {"bmm_f32": 3}, counts(census)
        assert [a[-2] for a in census["bmm_f32"]] == [0, 0, 0]          # the batch is summed outside (gw.sum(0))
        got = {"y": y.detach(), "dx": src.grad, "dw": w.grad.unsqueeze(0), "db": b.grad}
        if exact:
            assert_sums_exact(sums)
            assert_equal64(got, stacked(gemm_ref.product(*draw)), NAMES)
        else:
            assert_within("conv._gemm_nc 2x40x72x10 bias", got, stacked(gemm_ref.product(*draw)),
                          stacked(gemm_ref.product(*draw, torch.float32)), sums, {"y": BMM_C, "dx": BMM_C, "dw": BMM_C, "db": SPIKE_C}, NAMES)


# ---- gradient sinks and the deferred queue
class _Sink:
    """FlatGradAllReduce(ws, 1) with its sinks installed, zeroed, and every weight's view pre-filled with 0.75"""

    def __init__(self, ops, *ws):
        from spike2former_amd.dist import FlatGradAllReduce
        assert ops.GRAD_SINKS is None
        self.ops, self.red = ops, FlatGradAllReduce(list(ws), 1)
        self.red.install_sinks()
        self.red.zero()
        self.views = self.red.views
        for w, v in zip(ws, self.views):
            assert ops._sink_for(w) is not None and ops._sink_for(w).data_ptr() == v.data_ptr()
            v.fill_(0.75)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.red.close()
        self.ops.GRAD_SINKS = None
        self.ops.wgrad_drop()
        return False

    def untouched(self):
        return all(bool((v == 0.75).all()) for v in self.views)

    def holds(self, want, i=0):
        got = self.views[i].detach().cpu().double()
        assert torch.equal(got, want), describe(f"sink {i}", (got - want).abs(), got != want)


def _sink_draw(shape, kind, seed, G=1):
    draw = draw_product(shape, kind, seed, False, True, G)
    assert_sums_exact(gemm_ref.abs_sums(gemm_ref.product, *draw))
    return draw, gemm_ref.product(*draw)


PIPE_JOB, R2_JOB = (2, 64, 128, 136), (2, 40, 72, 16)


@pytest.mark.parametrize("shape,launch,args", [pytest.param(PIPE_JOB, "spike_gemm_dw_pipe_grouped", (1, 0, 0), id="a-job-pipe-ok-takes"),
                                               pytest.param(R2_JOB, "spike_gemm_dw_grouped", (1, 32), id="l16-stays-on-the-round2-32-class")])
def test_deferred_weight_gradient_is_one_grouped_launch_at_the_flush(ops, switches, census, shape, launch, args):
    """DEFER_DW with a sink: the backward launches no weight gradient and leaves the sink alone; wgrad_flush() then makes exactly ONE
    grouped launch and dw + 0.75 is there; autograd gets no tensor for the weight"""
    B, M, K, L = shape
    assert ops.DEFER_DW and ops.DW_PIPE and B * L <= ops._DEFER_DW_MAX_CONTRACTION
    assert bool(ops.lib.s2f_spike_gemm_dw_pipe_ok(B, M, K, L)) == (launch == "spike_gemm_dw_pipe_grouped") == (L >= 32)
    draw, ref = _sink_draw(shape, "bf16", 41)
    w = torch.nn.Parameter(draw[1][0].float().cuda())
    with _Sink(ops, w) as sink:
        got, _, launched = run_product(ops, census, shape, "bf16", draw, ws=[w])
        assert launched == {**_PG, **_DX}, launched
        assert w.grad is None and got["dw"] is None and sink.untouched()          # nothing is in the sink before the flush
        assert_equal64(got, ref, ("y", "dx"))
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {launch: 1}, counts(census)
        assert census[launch][0][1:-1] == args          # (jobs, ...): one job, its step class or the pipeline's schedule
        sink.holds(ref["dw"][0] + 0.75)
        census.clear()
        ops.wgrad_flush()          # the queue is empty afterwards
        assert counts(census) == {}


def test_mixed_queue_makes_one_launch_per_class(ops, switches, census):
    """one backward pass over four layers with sinks: two jobs s2f_spike_gemm_dw_pipe_ok takes (one of each step class: they leave
    their classes for the pipeline's ONE list), an L = 16 job (32 class), and an L = 64 job on a map 8 but not 16 bytes aligned, which
    the pipeline's LDS-DMA cannot read (64 class, handed to _spike_dw directly: a forward product asks for 16-byte alignment) -> one
    launch per list with 2, 1 and 1 jobs"""
    shapes = [PIPE_JOB, (2, 40, 72, 64), R2_JOB]
    odd = (2, 24, 40, 64)
    assert [(s[3] % 64 == 0 or s[3] >= 512) for s in shapes + [odd]] == [False, True, False, True]
    draws = [_sink_draw(s, "bf16", 43 + i) for i, s in enumerate(shapes + [odd])]
    ws = [torch.nn.Parameter(d[1][0].float().cuda()) for d, _ in draws]
    with _Sink(ops, *ws) as sink:
        census.clear()
        loss, srcs = 0, []
        for s, (d, _), w in zip(shapes, draws, ws):
            src, sp = to_spikes(ops, d[0])
            srcs.append(src)
            loss = loss + (ops.spike_gemm(sp, w) * d[3].float().cuda()).sum()
        loss.backward()
        B, M, K, L = odd
        flat = torch.zeros(B * K * L + 4, dtype=torch.bfloat16, device="cuda")
        xo = flat[4:].view(B, K, L)
        xo.copy_(draws[3][0][0].to(torch.bfloat16))
        assert xo.data_ptr() % 16 == 8
        assert ops._spike_dw(draws[3][0][3].float().cuda(), xo, ws[3], B, M, K, L, pipe=True) is None
        assert counts(census) == {"pgemm_nn_bf16": 3, "pgemm_dx_f32": 3}, counts(census)
        assert sink.untouched() and all(w.grad is None for w in ws)
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {"spike_gemm_dw_pipe_grouped": 1, "spike_gemm_dw_grouped": 2}, counts(census)
        assert census["spike_gemm_dw_pipe_grouped"][0][1] == 2
        assert sorted(a[1:3] for a in census["spike_gemm_dw_grouped"]) == [(1, 32), (1, 64)]
        for i, (_, ref) in enumerate(draws):
            sink.holds(ref["dw"][0] + 0.75, i)
        for src, (_, ref) in zip(srcs, draws):
            assert_equal64({"dx": src.grad}, ref, ("dx",))


def test_57_jobs_flush_as_56_plus_1(ops, switches, census):
    """a grouped launch takes at most kMaxJobs jobs: 57 equal small layers -> two launches, 56 + 1, every sink dw + 0.75"""
    shape = (1, 16, 32, 16)
    n = MAX_JOBS + 1
    assert n == 57 and not ops.lib.s2f_spike_gemm_dw_pipe_ok(*shape)
    (x64, ws64, _, gy64), ref = _sink_draw(shape, "bf16", 59)
    g = torch.Generator().manual_seed(60)
    w64 = [draw_eighths(g, *ws64[0].shape) for _ in range(n)]
    ws = leaves(w64)
    with _Sink(ops, *ws) as sink:
        src, sp = to_spikes(ops, x64)
        gy = gy64.float().cuda()
        loss = 0
        for w in ws:
            loss = loss + (ops.spike_gemm(sp, w) * gy).sum()
        census.clear()
        loss.backward()
        assert counts(census) == {"pgemm_dx_f32": n} and sink.untouched()
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {"spike_gemm_dw_grouped": 2}, counts(census)
        assert [a[1:3] for a in census["spike_gemm_dw_grouped"]] == [(MAX_JOBS, 32), (1, 32)]
        for i in range(n):          # the weight gradient does not depend on the weight: every sink holds the same dw
            sink.holds(ref["dw"][0] + 0.75, i)
        dx = sum(gemm_ref.product(x64, [w], None, gy64)["dx"] for w in w64)
        assert_equal64({"dx": src.grad}, {"dx": dx}, ("dx",))


@pytest.mark.parametrize("row,acc", [pytest.param(ROW_TILE8_G2.values, ("spike_gemm_dw_bf16", -2), id="round2"),
                                     pytest.param(ROW_PIPE_RAGGED.values, ("spike_gemm_dw_pipe", 7), id="pipelined")])
@pytest.mark.parametrize("times", [1, 2], ids=["one-backward", "two-backwards-into-the-same-sink"])
def test_direct_weight_gradient_accumulates_into_its_sink(ops, switches, census, row, acc, times):
    """DEFER_DW off: the direct launch with accumulate = 1 (no zero fill) leaves times * dw + 0.75 in the sink"""
    shape, kind, _, _, on_route, launches, _, _ = row
    assert on_route(ops, *shape)
    switches(DEFER_DW=False)
    draw, ref = _sink_draw(shape, kind, 31 + times)
    w = torch.nn.Parameter(draw[1][0].float().cuda())
    with _Sink(ops, w) as sink:
        # (two backwards: the map asks for no gradient, so only the weight gradient runs twice)
        got, _, launched = run_product(ops, census, shape, kind, draw, ws=[w], backward=times, dx=times == 1)
        want = {k: v * (times if "dw" in k else 1) for k, v in launches.items() if times == 1 or k != "pgemm_dx_f32"}
        assert launched == want, launched
        assert all(a[acc[1]] == 1 and a[2] == sink.views[0].data_ptr() for a in census[acc[0]])
        assert w.grad is None and got["dw"] is None
        sink.holds(times * ref["dw"][0] + 0.75)
        assert_equal64(got, ref, ("y",) + (("dx",) if times == 1 else ()))


def test_wgrad_drop_empties_the_queue_without_touching_the_sink(ops, switches, census):
    draw, ref = _sink_draw(PIPE_JOB, "bf16", 67)
    w = torch.nn.Parameter(draw[1][0].float().cuda())
    with _Sink(ops, w) as sink:
        run_product(ops, census, PIPE_JOB, "bf16", draw, ws=[w])
        assert sum(len(j) for j in ops._DW_PENDING.values()) == 1
        ops.wgrad_drop()
        assert sum(len(j) for j in ops._DW_PENDING.values()) == 0 and not ops._DWG_PENDING
        census.clear()
        ops.wgrad_flush()
        torch.cuda.synchronize()
        assert counts(census) == {} and sink.untouched()


# -------------------------------------------------------------------------------------------------------------- dense_gemm
#   id, (B, G, M, K, L), the inequality of the route, the launches, stats, general draw too
def _drow(id_, shape, route, launches, stats=False, general=True, w_as="list"):
    return pytest.param(shape, stats, route, launches, general, w_as, id=id_)


def _single(B, G, M, K, L, fwd, bwd):
    """G single launches each way: the forward reads the pack of W^T (Mo = K, Ki = M), the input gradient the pack of W"""
    return dense_fast(L) and (G == 1 or G > 4) and dx_form(B, K, M, L)[0] == fwd and dx_form(B, M, K, L)[0] == bwd


def _grouped(B, G, M, K, L, fwd, bwd):
    return dense_fast(L) and 1 < G <= 4 and dxg_cfg(B, K, M, L) == fwd and dxg_cfg(B, M, K, L) == bwd and {fwd, bwd} <= TN_GROUPED


_DG = lambda G: {"pgemm_dx_f32_grouped": 2, "gemm_dw_general": G}
DENSE_SINGLE = (2, 1, 40, 72, 136)
DENSE_GROUPED = (2, 3, 40, 72, 136)
DENSE_ROWS = [
    _drow("single-fast", DENSE_SINGLE, lambda o, *s: _single(*s, 7, 7), {"pgemm_dx_f32": 2, "gemm_dw_general": 1}, w_as="matrix"),
    _drow("single-stats-forward-tile-10", (2, 1, 64, 128, 136), lambda o, *s: _single(*s, 10, 7),
          {"pgemm_dx_f32_stats": 1, "pgemm_dx_f32": 1, "gemm_dw_general": 1}, stats=True),
    _drow("grouped-tile-7", DENSE_GROUPED, lambda o, *s: _grouped(*s, 7, 7), _DG(3)),
    _drow("grouped-tile-5-forward", (2, 2, 32, 96, 256), lambda o, *s: _grouped(*s, 5, 7), _DG(2)),
    _drow("grouped-tile-3-forward-192-tiles", (8, 2, 72, 40, 3072),
          lambda o, *s: cdiv(s[4], 128) * s[0] * cdiv(s[2], 128) == DX_T3 and _grouped(*s, 3, 7), _DG(2)),
    _drow("grouped-stats", DENSE_GROUPED, lambda o, *s: _grouped(*s, 7, 7), _DG(3), stats=True),
    _drow("grouped-weights-as-a-stack", DENSE_GROUPED, lambda o, *s: _grouped(*s, 7, 7), _DG(3), general=False, w_as="stack"),
    _drow("five-groups-five-single-launches", (1, 5, 24, 16, 128), lambda o, *s: _single(*s, 5, 5),
          {"pgemm_dx_f32": 10, "gemm_dw_general": 5}),
    _drow("slow-l36-on-bmm", (2, 2, 24, 40, 36), lambda o, *s: s[4] % 4 == 0 and not dense_fast(s[4]), {"bmm_f32": 3}),
    _drow("slow-l130-on-bmm", (2, 2, 24, 40, 130), lambda o, *s: s[4] % 4 != 0 and s[4] >= PGEMM_MIN_N, {"bmm_f32": 3}),
    _drow("slow-one-weight-on-bmm", (2, 1, 24, 40, 36), lambda o, *s: not dense_fast(s[4]), {"bmm_f32": 3}, general=False),
]


def _dense_case(ops, switches, census, shape, stats, on_route, launches, w_as, seed, exact):
    B, G, M, K, L = shape
    assert on_route(ops, *shape), "the shape left its route: see the launch rule restated above"
    assert ops.DENSE_GROUPED
    wants_part = stats and dense_fast(L)
    if wants_part:
        single_pass_switch(ops, switches, B, G * M, L)
    draw = draw_product((B, M, K, L), "dense", seed, False, exact, G)
    sums = gemm_ref.abs_sums(gemm_ref.product, *draw)
    if exact:
        assert_sums_exact(sums)
    got, part, launched = run_product(ops, census, (B, M, K, L), "dense", draw, stats=stats, w_as=w_as)
    assert launched == launches, launched
    assert all(a[-2] == 0 for a in census.get("gemm_dw_general", []))          # no launch adds into anything: there is no sink
    if dense_fast(L):
        assert conversions(census) == {"pack_bf16x3": 2 * G}          # the pack of W^T forward, the pack of W backward
    if wants_part:
        assert_partials(ops, part, got["y"], exact)          # the partials of EVERY group's rows
        plain, none, _ = run_product(ops, census, (B, M, K, L), "dense", draw[:3] + (None,), stats=False, w_as=w_as)
        assert none is None and torch.equal(plain["y"], got["y"])
    else:
        assert part is None
    return draw, stacked(sums), got


@pytest.mark.parametrize("shape,stats,on_route,launches,general,w_as", DENSE_ROWS)
def test_dense_gemm_route_equals_fp64(ops, switches, census, shape, stats, on_route, launches, general, w_as):
    draw, _, got = _dense_case(ops, switches, census, shape, stats, on_route, launches, w_as, sum(shape), True)
    assert_equal64(got, stacked(gemm_ref.product(*draw)), NAMES)


@pytest.mark.parametrize("shape,stats,on_route,launches,general,w_as", [r for r in DENSE_ROWS if r.values[4]])
def test_dense_gemm_route_general_operands_within_the_fp32_bound(ops, switches, census, shape, stats, on_route, launches, general, w_as):
    draw, sums, got = _dense_case(ops, switches, census, shape, stats, on_route, launches, w_as, sum(shape) + 1000, False)
    assert_within("dense_gemm " + "x".join(map(str, shape)) + (" stats" if stats else ""), got, stacked(gemm_ref.product(*draw)),
                  stacked(gemm_ref.product(*draw, torch.float32)), sums, {"y": BMM_C, "dx": BMM_C, "dw": BMM_C}, ("y", "dx", "dw"))


def test_dense_gemm_weights_as_views_of_parameters_keep_their_own_gradients(ops, switches, census):
    """w handed over as a list of G parameters, as their stack, and (G = 1) as one matrix: the same values, and each parameter of the
    list receives its own gradient"""
    B, G, M, K, L = DENSE_GROUPED
    draw = draw_product((B, M, K, L), "dense", 71, False, True, G)
    ref = stacked(gemm_ref.product(*draw))
    ws = leaves(draw[1])
    a, _, _ = run_product(ops, census, (B, M, K, L), "dense", draw, ws=ws)
    assert all(w.grad is not None and w.grad.shape == (M, K) for w in ws) and len({w.grad.data_ptr() for w in ws}) == G
    b, _, _ = run_product(ops, census, (B, M, K, L), "dense", draw, w_as="stack")
    for got in (a, b):
        assert_equal64(got, ref, ("y", "dx", "dw"))


@pytest.mark.parametrize("wide", ["x-forward", "x-dw", "gy-dw", "gy-dx"])
@pytest.mark.parametrize("shape", [pytest.param(DENSE_SINGLE, id="single"), pytest.param(DENSE_GROUPED, id="grouped")])
def test_dense_gemm_needs_all_three_terms_of_both_operands(ops, switches, census, shape, wide):
    """both operands of every dense product are split: the map x and the gradient gy inside pg_tn_f32_kernel, both sides of the
    weight gradient inside s2f_gemm_dw_general.  ONE product per output entry: 20-bit x against a selection w (forward), 20-bit x
    against a one-hot gy and 20-bit gy against a one-hot x (dw), 20-bit gy against a selection w (dx)"""
    B, G, M, K, L = shape
    g = torch.Generator().manual_seed(len(wide) + G)
    name = {"x-forward": "y", "x-dw": "dw", "gy-dw": "dw", "gy-dx": "dx"}[wide]
    ws = [selection(g, M, K) for _ in range(G)]
    if wide == "x-forward":
        x, gy = wide_values(g, B, G * K, L), grid(g, -2, 2, B, G * M, L)
    elif wide == "x-dw":
        x, gy = wide_values(g, B, G * K, L), _distinct_rows(g, B, G, M, L)
    elif wide == "gy-dw":
        x, gy = _distinct_rows(g, B, G, K, L), wide_values(g, B, G * M, L)
    else:
        x, gy = draw_eighths(g, B, G * K, L), wide_values(g, B, G * M, L)
    ref = _one_product_per_entry(gemm_ref.product, (x, ws, None, gy), name)
    got, _, launched = run_product(ops, census, (B, M, K, L), "dense", (x, ws, None, gy))
    assert launched == ({"pgemm_dx_f32": 2, "gemm_dw_general": 1} if G == 1 else _DG(G)), launched
    assert_equal64(got, {name: ref}, (name,))


def _distinct_rows(g, B, G, C, L):
    """[B, G C, L] with one entry 1 per (batch element, group), every batch element in a row of its own within the group"""
    t = torch.zeros(B, G * C, L, dtype=torch.float64)
    for gi in range(G):
        for b, c in enumerate(torch.randperm(C, generator=g)[:B].tolist()):
            t[b, gi * C + c, int(torch.randint(0, L, (1,), generator=g))] = 1.0
    return t


@pytest.mark.parametrize("defer", [True, False], ids=["deferred-general-queue", "direct-accumulate"])
def test_dense_gemm_weight_gradients_into_their_sinks(ops, switches, census, defer):
    """G = 3 weights, each a parameter with its own sink, on offset pointers into the full tensors.  DEFER_DW: nothing is launched
    for the weights in backward, then ONE s2f_gemm_dw_general_grouped at the flush (the queue no other suite reaches); without it
    three s2f_gemm_dw_general with accumulate = 1.  Every sink holds dw + 0.75"""
    B, G, M, K, L = DENSE_GROUPED
    switches(DEFER_DW=defer)
    draw, ref = _sink_draw((B, M, K, L), "dense", 73, G)
    ws = leaves(draw[1])
    with _Sink(ops, *ws) as sink:
        got, _, launched = run_product(ops, census, (B, M, K, L), "dense", draw, ws=ws)
        assert all(w.grad is None for w in ws) and got["dw"] is None
        assert_equal64(got, ref, ("y", "dx"))
        if defer:
            assert launched == {"pgemm_dx_f32_grouped": 2}, launched
            assert sink.untouched() and len(ops._DWG_PENDING) == G
            census.clear()
            ops.wgrad_flush()
            assert counts(census) == {"gemm_dw_general_grouped": 1}, counts(census)
            assert census["gemm_dw_general_grouped"][0][1] == G
            census.clear()
            ops.wgrad_flush()
            assert counts(census) == {}
        else:
            assert launched == _DG(G), launched
            assert [a[-2] for a in census["gemm_dw_general"]] == [1] * G
            assert [a[4] for a in census["gemm_dw_general"]] == [v.data_ptr() for v in sink.views]
        for i in range(G):
            sink.holds(ref["dw"][i] + 0.75, i)


@pytest.mark.parametrize("wide", ["x", "gy"])
def test_grouped_general_weight_gradient_needs_all_three_terms_of_both_operands(ops, switches, census, wide):
    """s2f_gemm_dw_general_grouped splits both sides as the single kernel does: ONE product per entry into sinks pre-filled with
    zero (0.75 + a 20-bit value would round)"""
    B, G, M, K, L = DENSE_GROUPED
    g = torch.Generator().manual_seed(len(wide))
    ws64 = [draw_eighths(g, M, K) for _ in range(G)]
    if wide == "x":
        x, gy = wide_values(g, B, G * K, L), _distinct_rows(g, B, G, M, L)
    else:
        x, gy = _distinct_rows(g, B, G, K, L), wide_values(g, B, G * M, L)
    ref = _one_product_per_entry(gemm_ref.product, (x, ws64, None, gy), "dw")
    ws = leaves(ws64)
    with _Sink(ops, *ws) as sink:
        for v in sink.views:
            v.zero_()
        run_product(ops, census, (B, M, K, L), "dense", (x, ws64, None, gy), ws=ws)
        census.clear()
        ops.wgrad_flush()
        assert counts(census) == {"gemm_dw_general_grouped": 1}, counts(census)
        for i in range(G):
            sink.holds(ref[i], i)


# -------------------------------------------------------------------------------------------------------------- spike_gemm_siblings
#   id, G, (B, M, K, L), which map group g reads, the rows form, backward
SIBLINGS = [
    pytest.param(3, (2, 64, 64, 100), (0, 1, 1), ("rows", 8, 1), True, id="q-k-v-with-k-and-v-on-the-same-map"),
    pytest.param(1, (2, 64, 64, 100), (0,), ("rows", 8, 1), True, id="one-group"),
    pytest.param(4, (2, 64, 64, 100), (0, 1, 2, 3), ("rows", 8, 1), True, id="four-groups"),
    pytest.param(3, (2, 40, 72, 36), (0, 1, 2), ("rows", 6, 1), True, id="tile-6"),
    pytest.param(2, (2, 64, 128, 136), (0, 1), ("rows", 8, 2), True, id="two-steps"),
    pytest.param(2, (8, 130, 128, 4096), (0, 0), ("rows", 7, 2), False, id="tile-7-two-groups-forward-only"),
]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("G,shape,maps,form,backward", SIBLINGS)
def test_siblings_equal_fp64_and_the_separate_calls(ops, switches, census, G, shape, maps, form, backward, exact):
    """ONE s2f_pgemm_nn_bf16_grouped forward, one s2f_pgemm_dx_f32_grouped plus G weight gradients backward: against fp64, and bit
    for bit what G spike_gemm calls give for y and dx (and for dw wherever the order of its atomic adds cannot matter: see below), as
    the docstring of _SpikeGemmSiblings promises.  A map two groups read receives the sum of both groups' gradients"""
    B, M, K, L = shape
    tile, steps = form[1], form[2]
    assert nn_form(*shape) == form and bool(ops.lib.s2f_pgemm_nn_grouped_ok(B, M, L, K))
    assert tile in (ROWS_GROUPED_G2 if steps == 2 else ROWS_GROUPED)
    assert not backward or (dxg_cfg(*shape) == dx_form(*shape)[0] == 7 and 7 in TN_GROUPED)
    g = torch.Generator().manual_seed(G + sum(shape) + 1000 * (not exact))
    n_maps = max(maps) + 1
    x64 = [draw_spikes(g, B, K, L) for _ in range(n_maps)]
    if exact:
        w64, gy64 = [draw_eighths(g, M, K) for _ in range(G)], grid(g, -2, 2, G, B, M, L)
    else:
        w64, gy64 = [(torch.randn(M, K, generator=g) * K ** -0.5).double() for _ in range(G)], torch.randn(G, B, M, L, generator=g).double()
    if not backward:
        gy64 = None
    args = ([x64[m] for m in maps], w64, gy64)
    ref, sums = gemm_ref.siblings(*args), gemm_ref.abs_sums(gemm_ref.siblings, *args)

    def fold(d):          # per map: the sum over the groups that read it
        if d["dx"] is None:
            return {"y": d["y"], "dx": None, "dw": None}
        dx = torch.stack([sum(d["dx"][gi] for gi in range(G) if maps[gi] == m) for m in range(n_maps)], 0)
        return {"y": d["y"], "dx": dx, "dw": torch.stack(d["dw"], 0)}
    ref, sums = fold(ref), fold(sums)
    if exact:
        assert_sums_exact(sums)

    def run(together):
        pairs = [to_spikes(ops, x) if backward else (None, plain_spikes(ops, x)) for x in x64]
        ws = leaves(w64)
        xs = [pairs[m][1] for m in maps]
        assert ops.spike_gemm_siblings_ok(xs, ws) or not backward
        census.clear()
        if together:
            y = ops.spike_gemm_siblings(xs, ws)
        else:
            y = torch.stack([ops.spike_gemm(x, w) for x, w in zip(xs, ws)], 0)
        assert y.shape == (G, B, M, L)
        if backward:
            y.backward(gy64.float().cuda())
        got = {"y": y.detach(), "dx": torch.stack([p[0].grad for p in pairs], 0) if backward else None,
               "dw": torch.stack([w.grad for w in ws], 0) if backward else None}
        return got, counts(census)
    with torch.set_grad_enabled(backward):
        got, launched = run(True)
        dw = {} if not backward else ({"spike_gemm_dw_pipe": G} if dw_pipe(ops, *shape) else {"spike_gemm_dw_bf16": G})
        assert launched == {"pgemm_nn_bf16_grouped": 1, **({"pgemm_dx_f32_grouped": 1} if backward else {}), **dw}, launched
        one, launched = run(False)
        assert launched == {"pgemm_nn_bf16": G, **({"pgemm_dx_f32": G} if backward else {}), **dw}, launched
    names = ("y", "dx", "dw") if backward else ("y",)
    for name in names:
        # y and dx are stores of one workgroup each: bit for bit.  dw is the SAME launch either way, G times, but its contraction
        # splits add with fp32 atomics in the order they retire: equal bits only where every partial sum is exact (the exact draw);
        # on the general draw both are held to the fp64 bound below
        if name != "dw" or exact:
            assert torch.equal(got[name], one[name]), name
    if exact:
        assert_equal64(got, ref, names)
    else:
        ref32 = fold(gemm_ref.siblings(*args, torch.float32))
        assert_within(f"siblings G={G} " + "x".join(map(str, shape)), got, ref, ref32, sums, {"y": SPIKE_C, "dx": BMM_C, "dw": SPIKE_C}, names)
        if backward:
            assert_within(f"separate G={G} " + "x".join(map(str, shape)), one, ref, ref32, sums, {"dw": SPIKE_C}, ("dw",))


REFUSED = [
    pytest.param(2, (2, 64, 1024, 128), "bf16", id="k1024-with-n-mod-8-is-0-runs-on-the-all-dma-tile"),
    pytest.param(2, (2, 8, 72, 36), "bf16", id="m-below-16"),
    pytest.param(2, (2, 64, 64, 100), "fp32", id="an-fp32-map"),
    pytest.param(2, (2, 64, 64, 100), "unequal", id="unequal-shapes"),
    pytest.param(5, (2, 64, 64, 100), "bf16", id="five-maps"),
]


@pytest.mark.parametrize("G,shape,what", REFUSED)
def test_siblings_refused(ops, switches, census, G, shape, what):
    """spike_gemm_siblings_ok is False, and where the library itself refuses (a shape off the register-staged form, more than four
    groups) the direct call returns S2F_EINVAL before any launch: the output keeps its fill"""
    B, M, K, L = shape
    g = torch.Generator().manual_seed(G)
    xs = [plain_spikes(ops, draw_spikes(g, B, K, L)) for _ in range(G)]
    ws = [draw_eighths(g, M, K).float().cuda() for _ in range(G)]
    if what == "fp32":
        xs[1] = ops.Spikes(xs[1].data.float(), ops._new_tok(xs[1].data))
    if what == "unequal":
        xs[1] = plain_spikes(ops, draw_spikes(g, B, K, L + 4))
    assert not ops.spike_gemm_siblings_ok(xs, ws)
    library = what == "bf16" and M >= 16
    if library:
        assert G > 4 or not ops.lib.s2f_pgemm_nn_grouped_ok(B, M, L, K)
        packs = [ops.pack_weight(w) for w in ws]
        y = torch.full((G, B, M, L), -7.0, device="cuda")
        census.clear()
        rc = ops.lib.s2f_pgemm_nn_bf16_grouped(ptrs(packs), ptrs([x.data for x in xs]), G, y.data_ptr(), B * M * L, B, M, L, K, stream())
        assert rc == EINVAL and ops.lib.s2f_last_error() != b""
        torch.cuda.synchronize()
        assert bool((y == -7.0).all())


# -------------------------------------------------------------------------------------------------------------- bmm_small
def _bmm_operands(exact, seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [draw_eighths(g, *s) if exact else torch.randn(*s, generator=g).double() for s in shapes]


def _check_bmm(ops, census, label, a_dev, b_dev, a64, b64, reduce_batch, exact):
    census.clear()
    c = ops.bmm_small(a_dev, b_dev, reduce_batch)
    assert counts(census) == {"bmm_f32": 1} and census["bmm_f32"][0][-2] == int(reduce_batch)
    ref, A = gemm_ref.bmm(a64, b64, reduce_batch), gemm_ref.abs_sums(gemm_ref.bmm, a64, b64, reduce_batch)
    if exact:
        assert A.max().item() * 64 < 2 ** 24
        assert_equal64({"c": c}, {"c": ref}, ("c",))
    else:
        assert_within("bmm_small " + label, {"c": c}, {"c": ref}, {"c": gemm_ref.bmm(a64, b64, reduce_batch, torch.float32)}, {"c": A},
                      {"c": BMM_C}, ("c",))


BMM_SHAPE = (3, 65, 17, 66)          # (B, M, K, N): one more than a tile in every direction of the 64 x 64 x 16 kernel


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("layout", ["plain", "a-transposed", "b-transposed", "a-batch-expanded", "b-batch-expanded", "slices", "reduce-batch",
                                    "n1", "m1"])
def test_bmm_small(ops, switches, census, layout, exact):
    """s2f_bmm_f32 reads its operands in place through their strides: transposed views, stride-0 batch expansion, non-contiguous
    slices; reduce_batch sums the batch inside the kernel"""
    B, M, K, N = BMM_SHAPE
    assert (M, N, K) == (BMM_TM + 1, BMM_TN + 2, BMM_TK + 1)
    if layout == "n1":
        N = 1
    if layout == "m1":
        M = 1
    a64, b64 = _bmm_operands(exact, len(layout) + exact, (B, M, K), (B, K, N))
    a, b = a64.float().cuda(), b64.float().cuda()
    if layout == "a-transposed":
        a = a64.transpose(1, 2).contiguous().float().cuda().transpose(1, 2)
        assert not a.is_contiguous()
    elif layout == "b-transposed":
        b = b64.transpose(1, 2).contiguous().float().cuda().transpose(1, 2)
        assert not b.is_contiguous()
    elif layout == "a-batch-expanded":
        a64 = a64[:1].expand(B, M, K)
        a = a64[0].float().cuda().expand(B, M, K)
        assert a.stride(0) == 0
    elif layout == "b-batch-expanded":
        b64 = b64[:1].expand(B, K, N)
        b = b64[0].float().cuda().expand(B, K, N)
        assert b.stride(0) == 0
    elif layout == "slices":
        big_a, big_b = _bmm_operands(exact, 99 + exact, (B, M + 3, 2 * K + 1), (B + 1, K + 2, N + 5))
        a64, b64 = big_a[:, 2:M + 2, 1:2 * K + 1:2], big_b[1:, 1:K + 1, 3:N + 3]
        a, b = big_a.float().cuda()[:, 2:M + 2, 1:2 * K + 1:2], big_b.float().cuda()[1:, 1:K + 1, 3:N + 3]
        assert not a.is_contiguous() and not b.is_contiguous()
    _check_bmm(ops, census, layout + " " + "x".join(map(str, (B, M, K, N))), a, b, a64, b64, layout == "reduce-batch", exact)


def test_bmm_small_empty_operands_launch_nothing(ops, switches, census):
    """K = 0 and B = 0 -> zeros (reduce_batch too), an empty output -> an empty tensor: no launch"""
    dev = "cuda"
    census.clear()
    c = ops.bmm_small(torch.zeros(2, 5, 0, device=dev), torch.zeros(2, 0, 7, device=dev))
    assert c.shape == (2, 5, 7) and bool((c == 0).all())
    c = ops.bmm_small(torch.zeros(2, 5, 0, device=dev), torch.zeros(2, 0, 7, device=dev), True)
    assert c.shape == (5, 7) and bool((c == 0).all())
    c = ops.bmm_small(torch.zeros(0, 5, 3, device=dev), torch.zeros(0, 3, 7, device=dev), True)
    assert c.shape == (5, 7) and bool((c == 0).all())
    assert ops.bmm_small(torch.zeros(0, 5, 3, device=dev), torch.zeros(0, 3, 7, device=dev)).shape == (0, 5, 7)
    assert ops.bmm_small(torch.zeros(2, 0, 3, device=dev), torch.zeros(2, 3, 7, device=dev)).shape == (2, 0, 7)
    assert ops.bmm_small(torch.zeros(2, 5, 3, device=dev), torch.zeros(2, 3, 0, device=dev)).shape == (2, 5, 0)
    assert counts(census) == {}


# -------------------------------------------------------------------------------------------------------------- the forced-cfg sweep
SWEEP = [(3, 100, 72, 136), (2, 130, 160, 132), (1, 40, 1024, 136)]
ALL_CFGS = tuple(range(1, 13))


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_forward_entry_point_runs_every_built_tile_and_refuses_the_rest(ops, switches, census, shape):
    """s2f_pgemm_nn_bf16 with a forced cfg (bias included): the all-DMA tiles of kNnTiles where N % 8 == 0, the rows tiles 6 / 7 / 8
    (one or two steps per barrier by the rule) anywhere -- each EQUALS fp64; anything else is S2F_EINVAL with the output untouched"""
    B, M, K, L = shape
    assert set(NN_TILES) == NN_PLAIN and ROWS_TILES == ROWS_PLAIN and ROWS_G2 < ROWS_PLAIN
    x64, ws64, b64, _ = draw = draw_product(shape, "bf16", sum(shape), True, True)[:3] + (None,)
    assert_sums_exact(gemm_ref.abs_sums(gemm_ref.product, *draw))
    ref = gemm_ref.product(*draw)["y"]
    pack, x, bias = ops.pack_weight(ws64[0].float().cuda()), x64.to(torch.bfloat16).cuda(), b64.float().cuda()
    ran = []
    for cfg in ALL_CFGS:
        built = cfg in ROWS_TILES or (cfg in NN_PLAIN and L % 8 == 0)
        if not built and L % 8 != 0 and cfg > max(ROWS_TILES):
            continue          # rows of N % 8 == 4 send an unknown cfg to the rows tile 6 (see the module docstring)
        y = torch.full((B, M, L), -7.0, device="cuda")
        rc = ops.lib.s2f_pgemm_nn_bf16(pack.data_ptr(), x.data_ptr(), bias.data_ptr(), y.data_ptr(), B, M, L, K, 3, cfg, stream())
        if built:
            assert rc == 0, (cfg, ops.lib.s2f_last_error())
            assert_equal64({f"y cfg {cfg}": y}, {f"y cfg {cfg}": ref}, (f"y cfg {cfg}",))
            ran.append(cfg)
        else:
            assert rc == EINVAL, cfg
            torch.cuda.synchronize()
            assert bool((y == -7.0).all()), cfg
    assert set(ran) == (ROWS_TILES | (NN_PLAIN if L % 8 == 0 else set()))


@pytest.mark.parametrize("shape", SWEEP + [(1, 512, 72, 36)], ids=lambda s: "x".join(map(str, s)))
def test_input_gradient_entry_point_runs_every_built_tile_and_refuses_the_rest(ops, switches, census, shape):
    """s2f_pgemm_dx_f32 with a forced cfg: the store form (beta = 0) on every tile of kTnTiles, beta = 1 on the tiles its form is
    built for (EINVAL on the 32- / 64-row-step tiles: 'the plain store form'), unknown tiles EINVAL; on the contraction-split shape
    every cfg runs the split form's tile 4.  Each run EQUALS fp64 (beta = 1: twice the gradient, over the first run's result)"""
    B, M, K, L = shape
    assert set(TN_TILES) == TN_STORE and TN_BETA == TN_SPLIT and TN_BETA < TN_STORE
    split = dx_form(B, M, K, L)[1] > 1
    assert split == (shape == (1, 512, 72, 36))
    x64, ws64, _, gy64 = draw = draw_product(shape, "bf16", sum(shape) + 1, False, True)
    assert_sums_exact({"dx": 2 * gemm_ref.abs_sums(gemm_ref.product, *draw)["dx"]})
    ref = gemm_ref.product(*draw)["dx"]
    pack, gy = ops.pack_weight(ws64[0].float().cuda()), gy64.float().cuda()
    for cfg in ALL_CFGS:
        dx = torch.full((B, K, L), -7.0, device="cuda")
        call = lambda beta: ops.lib.s2f_pgemm_dx_f32(pack.data_ptr(), gy.data_ptr(), 0, dx.data_ptr(), 0, B, M, K, L, beta, cfg, stream())
        rc = call(0.0)
        if split or cfg in TN_STORE:
            assert rc == 0, (cfg, ops.lib.s2f_last_error())
            assert_equal64({f"dx cfg {cfg}": dx}, {f"dx cfg {cfg}": ref}, (f"dx cfg {cfg}",))
        else:
            assert rc == EINVAL, cfg
            torch.cuda.synchronize()
            assert bool((dx == -7.0).all()), cfg
            dx.copy_(ref)
        rc = call(1.0)
        if split or cfg in TN_BETA:
            assert rc == 0, (cfg, ops.lib.s2f_last_error())
            assert_equal64({f"dx cfg {cfg} beta 1": dx}, {f"dx cfg {cfg} beta 1": 2 * ref}, (f"dx cfg {cfg} beta 1",))
        else:
            assert rc == EINVAL, cfg
            torch.cuda.synchronize()
            assert torch.equal(dx.cpu().double(), ref), cfg
