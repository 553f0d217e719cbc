"""Every route of the DCNv3 sampling core (csrc/dcnv3.hip: s2f_dcnv3_fwd / _bwd on [N, H, W, C] maps, s2f_dcnv3_fwd_cm / _bwd_cm on
channel-major maps) against the fp64 restatement of tests/dcn_ref.py, at the smallest shapes that reach it.  Each case is one row
whose id names the route and the edge.  A row, in this order,

  1. asks the library which kernels its geometry takes (ops.dcnv3_route = s2f_dcnv3_route, the function the four entry points
     dispatch on) and asserts that they are the ones the row is there for -- the band count included;
  2. fills every output with NaN;
  3. calls the entry points (lib.s2f_dcnv3_*, so that the outputs are the NaN-filled buffers and a map may sit off the 16-byte
     grid), and then the autograd wrappers ops.dcnv3_core / ops.dcnv3_core_cm, which must return the same values;
  4. compares y, dx, doffset, dmask with dcn_ref in fp64.

Two draws per row:

  exact     x multiples of 1/8 in [-1, 1], mask multiples of 1/8 in [0, 1] (a ninth of them zero), gy integers in [-2, 2], offsets
            multiples of 1/4 (round(8 randn) / 4, scaled down on the tiny maps), offset_scale in {1, 0.5, 2, 1.5}; one offset pair in
            ten is moved -- a third of those onto the first or last row and column of the padded map (exactly integer positions
            among them), a third just outside it, a third a few multiples of W + 8 away.  Positions are then multiples of 1/8 and
            the bilinear weights of 1/64: every product and every partial sum is a whole number of granules (2^-12 for y, 2^-9 for
            dx and dmask, 2^-10 for doffset), and the row asserts on its own draw (dcn_ref.abs_sums) that every sum of ABSOLUTE
            terms stays below 2^24 granules -- so fp32 is exact in any order, with or without FMA, through the fixed-point
            accumulator and through fp32 atomics, and all four results must EQUAL the fp64 values.  The row also asserts that a
            quarter or more of every result is non-zero and that corners inside and outside the map both occur.
  general   x, mask (signed) and gy randn, offsets 2 randn rounded to multiples of 2^-10; the row asserts that the sampling positions
            evaluated in fp32 and in fp64 are identical, so both sides take the same floor, no sample is excluded and no tolerance
            absorbs a flipped corner.  Per entry |got - ref64| <= 1.01 (T + 6) 2^-24 A + 1e-30 with A the entry's sum of absolute terms
            and T their number (dcn_ref.abs_sums): the worst case of an fp32 sum of T terms in any order plus the roundings inside one
            term -- derived, not tuned.  The row lds-4x4 draws gy with magnitudes spanning 2^-20 .. 2^20.

Route ids of include/s2f.h and the rows that take them (test_every_route_id_has_a_row holds the list to the header):
  S2F_DCN_FWD_K3C8           fwd-k3c8, the geo-* rows with Cg = 8, grid-k3c8, every lds-* / banded-* row with Cg = 8
  S2F_DCN_FWD_VEC4           fwd-vec4-cg4, fwd-vec4-cg16, fwd-vec4-k5, fwd-vec4-k3x1, fwd-vec4-k1x3, geo-sh-ne-sw, grid-vec4, atomic-vec4
  S2F_DCN_FWD_SCALAR         fwd-scalar-cg3, fwd-scalar-misaligned, lds-cg3, atomic-scalar, banded-misaligned
  S2F_DCN_BWD_LDS            lds-1x1, lds-2x3, lds-4x4, lds-9x11-odd, lds-8x8-even, lds-1x255, lds-16x16, lds-1x257, lds-cg4, lds-cg3
  S2F_DCN_BWD_BANDED         banded-37x34-natural (5 bands), banded-forced-2 / -7 / -9, banded-stride2-more-bands-than-rows, banded-misaligned
  S2F_DCN_BWD_ATOMIC_VEC4    atomic-vec4 (Cg = 128), atomic-vec4-forced (Cg = 8, more bands forced than the map has rows)
  S2F_DCN_BWD_ATOMIC_SCALAR  atomic-scalar (Cg = 130), atomic-scalar-misaligned
  S2F_DCN_CM_FWD_K3C8        cm-k3c8-rs12, cm-k3c8-rs8, cm-under-64-pixels, cm-stride2
  S2F_DCN_CM_FWD_GENERIC     cm-generic-cg4, cm-generic-cg16, cm-generic-cg3, cm-generic-1600-pixels, cm-k1x3-cg8
  S2F_DCN_CM_BWD_PLAIN       cm-generic-cg16
  S2F_DCN_CM_BWD_PIPE        cm-generic-cg4, cm-generic-cg3, cm-generic-1600-pixels, cm-k1x3-cg8
  S2F_DCN_CM_BWD_PIPE_K3C8   cm-k3c8-rs12 (N G = 8: cm_slice_of_block permutes), cm-k3c8-rs8 (N G = 3: it does not), cm-stride2

Measured on the MI355X, worst |err| / A over the entries, kernel | fp32 CPU evaluation of dcn_ref (docs/EXPERIMENTS.md has the same
table; the two grid-* rows evaluate dcn_ref on the device), rows as (N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw):
  fwd-k3c8                             (2,9,11,3,8,3,3,1,1,1,1,1,1)     y 1.4e-07 | 1.4e-07   dx 9.5e-08 | 1.9e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.7e-07 | 1.7e-07
  fwd-vec4-cg4                         (2,9,11,3,4,3,3,1,1,1,1,1,1)     y 1.4e-07 | 1.4e-07   dx 7.5e-08 | 2.5e-07   doffset 1.7e-07 | 1.7e-07   dmask 1.5e-07 | 1.5e-07
  fwd-vec4-cg16                        (1,7,9,2,16,3,3,1,1,1,1,1,1)     y 1.5e-07 | 1.5e-07   dx 9.2e-08 | 1.7e-07   doffset 1.3e-07 | 8.5e-08   dmask 1.0e-07 | 9.2e-08
  fwd-vec4-k5                          (1,9,11,2,8,5,5,1,1,2,2,1,1)     y 1.4e-07 | 1.0e-07   dx 4.2e-08 | 2.7e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.4e-07 | 1.4e-07
  fwd-vec4-k3x1                        (1,9,11,2,8,3,1,1,1,1,0,1,1)     y 1.5e-07 | 1.5e-07   dx 1.1e-07 | 1.7e-07   doffset 1.2e-07 | 1.2e-07   dmask 1.2e-07 | 1.2e-07
  fwd-vec4-k1x3                        (1,9,11,2,8,1,3,1,1,0,1,1,1)     y 1.7e-07 | 1.2e-07   dx 1.1e-07 | 1.4e-07   doffset 1.0e-07 | 1.0e-07   dmask 1.1e-07 | 1.1e-07
  fwd-scalar-cg3                       (2,9,11,3,3,3,3,1,1,1,1,1,1)     y 1.3e-07 | 1.7e-07   dx 7.9e-08 | 2.2e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.5e-07 | 1.5e-07
  fwd-scalar-misaligned                (2,9,11,3,8,3,3,1,1,1,1,1,1)     y 1.8e-07 | 1.5e-07   dx 9.7e-08 | 2.0e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.6e-07 | 1.6e-07
  geo-stride2-pad1                     (2,9,11,2,8,3,3,2,2,1,1,1,1)     y 1.3e-07 | 1.5e-07   dx 1.2e-07 | 1.6e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.7e-07 | 1.7e-07
  geo-pad0                             (1,9,11,2,8,3,3,1,1,0,0,1,1)     y 1.1e-07 | 1.2e-07   dx 1.2e-07 | 2.1e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.4e-07 | 1.4e-07
  geo-pad2-dil2                        (1,9,11,2,8,3,3,1,1,2,2,2,2)     y 1.6e-07 | 1.7e-07   dx 9.5e-08 | 2.3e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.2e-07 | 1.2e-07
  geo-sh-ne-sw                         (1,9,11,2,4,3,3,2,1,1,1,1,1)     y 1.3e-07 | 1.3e-07   dx 9.4e-08 | 1.6e-07   doffset 1.2e-07 | 1.2e-07   dmask 1.1e-07 | 1.1e-07
  geo-ph-ne-pw                         (1,9,11,2,8,3,3,1,1,2,0,1,1)     y 1.7e-07 | 1.4e-07   dx 9.9e-08 | 1.9e-07   doffset 1.5e-07 | 1.5e-07   dmask 1.2e-07 | 1.2e-07
  grid-k3c8                            (25,32,32,41,8,3,3,1,1,1,1,1,1)  y 2.6e-07 | 2.4e-07   dx 1.2e-07 | 4.4e-07   doffset 2.7e-07 | 2.0e-07   dmask 2.5e-07 | 1.9e-07
  grid-vec4                            (25,32,32,41,4,3,3,1,1,1,1,1,1)  y 2.3e-07 | 2.2e-07   dx 1.0e-07 | 4.3e-07   doffset 2.7e-07 | 2.5e-07   dmask 2.5e-07 | 2.3e-07
  lds-1x1                              (3,1,1,2,8,3,3,1,1,1,1,1,1)      y 9.9e-08 | 8.6e-08   dx 5.8e-08 | 5.8e-08   doffset 1.2e-07 | 1.2e-07   dmask 1.1e-07 | 1.1e-07
  lds-2x3                              (2,2,3,2,8,3,3,1,1,1,1,1,1)      y 1.5e-07 | 9.3e-08   dx 7.6e-08 | 1.4e-07   doffset 1.1e-07 | 1.1e-07   dmask 1.3e-07 | 1.3e-07
  lds-4x4                              (2,4,4,3,8,3,3,1,1,1,1,1,1)      y 1.3e-07 | 1.2e-07   dx 4.9e-07 | 2.0e-07   doffset 1.9e-07 | 1.9e-07   dmask 1.7e-07 | 1.7e-07
  lds-9x11-odd                         (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.7e-07 | 1.7e-07   dx 7.8e-08 | 2.1e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.5e-07 | 1.5e-07
  lds-8x8-even                         (1,8,8,2,8,3,3,1,1,1,1,1,1)      y 1.3e-07 | 1.4e-07   dx 9.9e-08 | 2.5e-07   doffset 1.1e-07 | 1.1e-07   dmask 1.4e-07 | 1.4e-07
  lds-1x255                            (1,1,255,1,8,3,3,1,1,1,1,1,1)    y 1.5e-07 | 1.5e-07   dx 8.9e-08 | 2.0e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.2e-07 | 1.2e-07
  lds-16x16                            (1,16,16,2,8,3,3,1,1,1,1,1,1)    y 1.5e-07 | 1.2e-07   dx 6.7e-08 | 2.1e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.5e-07 | 1.5e-07
  lds-1x257                            (1,1,257,1,8,3,3,1,1,1,1,1,1)    y 1.6e-07 | 1.6e-07   dx 1.1e-07 | 1.7e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.2e-07 | 1.2e-07
  lds-cg4                              (2,6,5,2,4,3,3,1,1,1,1,1,1)      y 1.5e-07 | 1.1e-07   dx 9.0e-08 | 2.0e-07   doffset 1.3e-07 | 1.3e-07   dmask 1.2e-07 | 1.2e-07
  lds-cg3                              (2,6,5,3,3,3,3,1,1,1,1,1,1)      y 1.6e-07 | 1.3e-07   dx 9.0e-08 | 1.6e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.4e-07 | 1.4e-07
  banded-37x34-natural                 (1,37,34,1,8,3,3,1,1,1,1,1,1)    y 1.7e-07 | 1.4e-07   dx 7.1e-08 | 2.4e-07   doffset 1.7e-07 | 1.7e-07   dmask 1.9e-07 | 1.9e-07
  banded-forced-2                      (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.3e-07 | 1.3e-07   dx 5.5e-08 | 2.2e-07   doffset 1.3e-07 | 1.3e-07   dmask 1.3e-07 | 1.3e-07
  banded-forced-7                      (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.7e-07 | 1.7e-07   dx 7.8e-08 | 2.1e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.5e-07 | 1.5e-07
  banded-forced-9                      (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.5e-07 | 1.7e-07   dx 1.2e-07 | 1.8e-07   doffset 1.5e-07 | 1.5e-07   dmask 1.1e-07 | 1.1e-07
  banded-stride2-more-bands-than-rows  (1,9,11,2,8,3,3,2,2,1,1,1,1)     y 1.3e-07 | 1.1e-07   dx 1.1e-07 | 1.7e-07   doffset 1.1e-07 | 1.1e-07   dmask 1.1e-07 | 1.1e-07
  banded-misaligned                    (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.3e-07 | 1.3e-07   dx 5.5e-08 | 2.2e-07   doffset 1.3e-07 | 1.3e-07   dmask 1.3e-07 | 1.3e-07
  atomic-vec4                          (1,6,5,1,128,3,3,1,1,1,1,1,1)    y 1.3e-07 | 1.4e-07   dx 1.6e-07 | 2.0e-07   doffset 8.9e-08 | 3.9e-08   dmask 6.6e-08 | 3.4e-08
  atomic-scalar                        (1,5,7,1,130,3,3,1,1,1,1,1,1)    y 1.6e-07 | 1.6e-07   dx 2.2e-07 | 2.1e-07   doffset 9.9e-08 | 2.9e-08   dmask 1.2e-07 | 3.5e-08
  atomic-vec4-forced                   (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.5e-07 | 1.7e-07   dx 2.1e-07 | 1.8e-07   doffset 1.5e-07 | 1.5e-07   dmask 1.1e-07 | 1.1e-07
  atomic-scalar-misaligned             (1,9,11,2,8,3,3,1,1,1,1,1,1)     y 1.4e-07 | 1.4e-07   dx 2.1e-07 | 2.2e-07   doffset 1.3e-07 | 1.3e-07   dmask 1.2e-07 | 1.2e-07
  cm-k3c8-rs12                         (2,8,8,4,8,3,3,1,1,1,1,1,1)      y 1.5e-07 | 1.7e-07   dx 9.8e-08 | 2.3e-07   doffset 1.5e-07 | 1.5e-07   dmask 1.4e-07 | 1.4e-07
  cm-k3c8-rs8                          (1,33,34,3,8,3,3,1,1,1,1,1,1)    y 1.7e-07 | 1.6e-07   dx 8.5e-08 | 3.1e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.6e-07 | 1.6e-07
  cm-generic-cg4                       (1,5,7,2,4,3,3,1,1,1,1,1,1)      y 1.0e-07 | 1.0e-07   dx 7.5e-08 | 1.4e-07   doffset 1.6e-07 | 1.6e-07   dmask 1.3e-07 | 1.3e-07
  cm-generic-cg16                      (1,8,9,2,16,3,3,1,1,1,1,1,1)     y 1.5e-07 | 1.4e-07   dx 8.7e-08 | 2.7e-07   doffset 9.7e-08 | 9.5e-08   dmask 8.8e-08 | 8.8e-08
  cm-generic-cg3                       (2,6,5,3,3,3,3,1,1,1,1,1,1)      y 1.6e-07 | 1.3e-07   dx 9.0e-08 | 1.6e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.4e-07 | 1.4e-07
  cm-generic-1600-pixels               (1,40,40,2,4,3,3,1,1,1,1,1,1)    y 1.6e-07 | 1.5e-07   dx 7.7e-08 | 3.8e-07   doffset 1.8e-07 | 1.8e-07   dmask 1.7e-07 | 1.7e-07
  cm-k1x3-cg8                          (1,8,8,3,8,1,3,1,1,0,1,1,1)      y 1.2e-07 | 1.8e-07   dx 9.9e-08 | 1.7e-07   doffset 1.3e-07 | 1.3e-07   dmask 1.2e-07 | 1.2e-07
  cm-under-64-pixels                   (1,5,7,2,8,3,3,1,1,1,1,1,1)      y 1.1e-07 | 1.3e-07   dx 8.2e-08 | 1.4e-07   doffset 1.1e-07 | 1.1e-07   dmask 9.4e-08 | 9.4e-08
  cm-stride2                           (2,9,11,4,8,3,3,2,2,1,1,1,1)     y 1.3e-07 | 1.6e-07   dx 1.1e-07 | 1.6e-07   doffset 1.4e-07 | 1.4e-07   dmask 1.1e-07 | 1.1e-07
  i.e. the bound (T + 6) 2^-24 is 2.5e-6 for y at 3 x 3, 2.3e-6 for doffset / dmask at Cg = 8, 1.3e-6 at Cg = 4, and never below 4.2e-7
  for dx (T = 1): y, doffset and dmask sit a factor of 4.8 or more inside it on every route (the nearest: doffset of grid-vec4, 2.7e-7
  against 1.3e-6) and within 3.5x of the plain fp32 evaluation; dx of the fixed-point routes (LDS, banded, channel-major) is at or below
  the fp32 evaluation on every randn row (4.2e-8 .. 1.2e-7 against 5.8e-8 .. 4.4e-7), dx of the fp32-atomic routes about equal to it
  (1.6e-7 .. 2.2e-7 against 1.8e-7 .. 2.2e-7).  The one figure near its bound is dx of lds-4x4 in the general
  draw, 4.9e-7 (in a host model of the accumulator, which gives the same figure, 0.91 of that entry's bound): the fixed-point accumulator rounds every contribution to 2^-50 of the SLICE's
  max |gy| max |mask|, which is finer than fp32 for an entry near that size and coarser for an entry 2^20 below it; with gy spanning
  2^-20 .. 2^20 a 4 x 4 map still adds some fifty terms into every entry, so every entry holds a large one.  (dx of the atomic
  rows depends on the order of the atomics and moves from run to run.)
  Whole file: 89 tests in 12.5 s: the four grid-* cases 1.0 .. 3.7 s, the first case 1.0 s (it loads the library), every other below 0.1 s.

Not reached here: NaN and Inf operands; the refusals of the channel-major entry points (test_gpu_dcn_channel_major.py); geometries whose
N G b workgroups pass 2^31."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("y", "dx", "doffset", "dmask")
GRANULES = {"y": 2 ** 12, "dx": 2 ** 9, "doffset": 2 ** 10, "dmask": 2 ** 9}          # per unit, exact draw


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def row(id, entry, N, H, W, G, Cg, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), osc=1.0, fwd=None, bwd=None, bands=None, cm_fwd=None, cm_rs=None,
        cm_bwd=None, force=None, misaligned=False, off_mul=1.0, wide_gy=False, blocks=False):
    """entry: "nhwc" (expects fwd, bwd, bands) or "cm" (expects cm_fwd, cm_rs, cm_bwd); the expected values are NAMES of ops.DCN_*"""
    want = {"fwd": fwd, "bwd": bwd, "bands": bands} if entry == "nhwc" else {"cm": 1, "cm_fwd": cm_fwd, "cm_rs": cm_rs, "cm_bwd": cm_bwd}
    assert all(v is not None for v in want.values()), id
    geo = (N, H, W, G, Cg, k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])
    return pytest.param(dict(id=id, entry=entry, geo=geo, osc=osc, want=want, force=force, misaligned=misaligned, off_mul=off_mul,
                             wide_gy=wide_gy, blocks=blocks), id=id)


K3C8 = dict(fwd="FWD_K3C8", bwd="BWD_LDS", bands=1)
CM2 = dict(cm_fwd="CM_FWD_K3C8", cm_rs=12, cm_bwd="CM_BWD_PIPE_K3C8")
ROWS = [
    # ---- [N, H, W, C] forward: 594 work items, a ragged last block
    row("fwd-k3c8", "nhwc", 2, 9, 11, 3, 8, **K3C8),
    row("fwd-vec4-cg4", "nhwc", 2, 9, 11, 3, 4, osc=0.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("fwd-vec4-cg16", "nhwc", 1, 7, 9, 2, 16, osc=2.0, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("fwd-vec4-k5", "nhwc", 1, 9, 11, 2, 8, k=(5, 5), p=(2, 2), osc=1.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    # the two windows that are not square pin the tap order k = i_w Kh + j_h
    row("fwd-vec4-k3x1", "nhwc", 1, 9, 11, 2, 8, k=(3, 1), p=(1, 0), osc=1.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("fwd-vec4-k1x3", "nhwc", 1, 9, 11, 2, 8, k=(1, 3), p=(0, 1), osc=0.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("fwd-scalar-cg3", "nhwc", 2, 9, 11, 3, 3, osc=2.0, fwd="FWD_SCALAR", bwd="BWD_LDS", bands=1),
    row("fwd-scalar-misaligned", "nhwc", 2, 9, 11, 3, 8, osc=1.5, misaligned=True, fwd="FWD_SCALAR", bwd="BWD_LDS", bands=1),
    # ---- geometries, on the routes they land on
    row("geo-stride2-pad1", "nhwc", 2, 9, 11, 2, 8, s=(2, 2), osc=1.5, **K3C8),
    row("geo-pad0", "nhwc", 1, 9, 11, 2, 8, p=(0, 0), osc=0.5, **K3C8),
    row("geo-pad2-dil2", "nhwc", 1, 9, 11, 2, 8, p=(2, 2), d=(2, 2), osc=2.0, **K3C8),
    row("geo-sh-ne-sw", "nhwc", 1, 9, 11, 2, 4, s=(2, 1), osc=1.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("geo-ph-ne-pw", "nhwc", 1, 9, 11, 2, 8, p=(2, 0), osc=0.5, **K3C8),
    # ---- more work items than 4096 blocks x 256 threads: the second trip of the forward kernels' grid-stride loop
    row("grid-k3c8", "nhwc", 25, 32, 32, 41, 8, blocks=True, **K3C8),
    row("grid-vec4", "nhwc", 25, 32, 32, 41, 4, osc=0.5, blocks=True, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    # ---- [N, H, W, C] backward, one workgroup per slice
    row("lds-1x1", "nhwc", 3, 1, 1, 2, 8, osc=0.5, off_mul=0.25, **K3C8),
    row("lds-2x3", "nhwc", 2, 2, 3, 2, 8, osc=0.5, off_mul=0.5, **K3C8),
    row("lds-4x4", "nhwc", 2, 4, 4, 3, 8, osc=1.5, off_mul=0.5, wide_gy=True, **K3C8),          # (the round-6 defect lived here)
    row("lds-9x11-odd", "nhwc", 1, 9, 11, 2, 8, osc=1.5, **K3C8),                  # odd H W: the scalar LDS reads
    row("lds-8x8-even", "nhwc", 1, 8, 8, 2, 8, osc=2.0, **K3C8),                   # even H W: the 16-byte LDS reads
    row("lds-1x255", "nhwc", 1, 1, 255, 1, 8, off_mul=0.5, **K3C8),                             # the 256-pixel chunk: one short of it,
    row("lds-16x16", "nhwc", 1, 16, 16, 2, 8, osc=0.5, **K3C8),                    # exactly one,
    row("lds-1x257", "nhwc", 1, 1, 257, 1, 8, osc=1.5, off_mul=0.5, **K3C8),                    # one pixel into the second
    row("lds-cg4", "nhwc", 2, 6, 5, 2, 4, osc=2.0, off_mul=0.5, fwd="FWD_VEC4", bwd="BWD_LDS", bands=1),
    row("lds-cg3", "nhwc", 2, 6, 5, 3, 3, osc=1.5, fwd="FWD_SCALAR", bwd="BWD_LDS", bands=1),
    # ---- banded: 37 x 34 is the smallest Cg = 8 map here whose slice no longer fits; 5 bands do not divide 37 rows
    row("banded-37x34-natural", "nhwc", 1, 37, 34, 1, 8, fwd="FWD_K3C8", bwd="BWD_BANDED", bands=5),
    row("banded-forced-2", "nhwc", 1, 9, 11, 2, 8, osc=0.5, force=2, fwd="FWD_K3C8", bwd="BWD_BANDED", bands=2),
    row("banded-forced-7", "nhwc", 1, 9, 11, 2, 8, osc=1.5, force=7, fwd="FWD_K3C8", bwd="BWD_BANDED", bands=7),          # two empty bands
    row("banded-forced-9", "nhwc", 1, 9, 11, 2, 8, osc=2.0, force=9, fwd="FWD_K3C8", bwd="BWD_BANDED", bands=9),          # one row each
    row("banded-stride2-more-bands-than-rows", "nhwc", 1, 9, 11, 2, 8, s=(2, 2), force=7, fwd="FWD_K3C8", bwd="BWD_BANDED", bands=7),
    row("banded-misaligned", "nhwc", 1, 9, 11, 2, 8, osc=0.5, force=2, misaligned=True, fwd="FWD_SCALAR", bwd="BWD_BANDED", bands=2),
    # ---- global atomics: the staging term 256 (3 P + Cg) 4 alone leaves no room for one band at these widths
    row("atomic-vec4", "nhwc", 1, 6, 5, 1, 128, osc=1.5, fwd="FWD_VEC4", bwd="BWD_ATOMIC_VEC4", bands=0),
    row("atomic-scalar", "nhwc", 1, 5, 7, 1, 130, osc=0.5, fwd="FWD_SCALAR", bwd="BWD_ATOMIC_SCALAR", bands=0),
    row("atomic-vec4-forced", "nhwc", 1, 9, 11, 2, 8, osc=2.0, force=12, fwd="FWD_K3C8", bwd="BWD_ATOMIC_VEC4", bands=0),
    row("atomic-scalar-misaligned", "nhwc", 1, 9, 11, 2, 8, force=12, misaligned=True, fwd="FWD_SCALAR", bwd="BWD_ATOMIC_SCALAR", bands=0),
    # ---- channel-major
    row("cm-k3c8-rs12", "cm", 2, 8, 8, 4, 8, osc=1.5, **CM2),                                       # N G = 8 workgroups
    row("cm-k3c8-rs8", "cm", 1, 33, 34, 3, 8, cm_fwd="CM_FWD_K3C8", cm_rs=8, cm_bwd="CM_BWD_PIPE_K3C8"),          # 1 122 pixels: two staging chunks
    row("cm-generic-cg4", "cm", 1, 5, 7, 2, 4, osc=0.5, cm_fwd="CM_FWD_GENERIC", cm_rs=4, cm_bwd="CM_BWD_PIPE"),
    row("cm-generic-cg16", "cm", 1, 8, 9, 2, 16, osc=2.0, cm_fwd="CM_FWD_GENERIC", cm_rs=20, cm_bwd="CM_BWD_PLAIN"),
    row("cm-generic-cg3", "cm", 2, 6, 5, 3, 3, osc=1.5, cm_fwd="CM_FWD_GENERIC", cm_rs=3, cm_bwd="CM_BWD_PIPE"),
    row("cm-generic-1600-pixels", "cm", 1, 40, 40, 2, 4, cm_fwd="CM_FWD_GENERIC", cm_rs=4, cm_bwd="CM_BWD_PIPE"),
    row("cm-k1x3-cg8", "cm", 1, 8, 8, 3, 8, k=(1, 3), p=(0, 1), osc=0.5, cm_fwd="CM_FWD_GENERIC", cm_rs=12, cm_bwd="CM_BWD_PIPE"),
    row("cm-under-64-pixels", "cm", 1, 5, 7, 2, 8, osc=2.0, off_mul=0.5, **CM2),
    row("cm-stride2", "cm", 2, 9, 11, 4, 8, s=(2, 2), osc=1.5, **CM2),          # Ho Wo = 30 < H W = 99: the staging loops' two lengths
]


def test_every_route_id_has_a_row(ops):
    """every S2F_DCN_* route id of include/s2f.h is what some row asserts its geometry takes, and stands in the docstring's list"""
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define S2F_DCN_((?:CM_)?(?:FWD|BWD)_\w+)[ \t]+(\d+)[ \t]*$", src, flags=re.M)}
    assert len(ids) == 12 and len(set(ids.values())) == 12
    taken = {v for r in ROWS for v in r.values[0]["want"].values() if isinstance(v, str)}
    assert taken == set(ids), set(ids) ^ taken
    for name, value in ids.items():
        assert getattr(ops, "DCN_" + name) == value
        assert re.search(r"^  S2F_DCN_%s\s" % name, __doc__, flags=re.M), name
    listed = set(re.findall(r"^  S2F_DCN_(\w+)", __doc__, flags=re.M))
    assert listed == set(ids)
    assert len({r.values[0]["id"] for r in ROWS}) == len(ROWS)


# -------------------------------------------------------------------------------------------------------------- draws
def _special_offsets(g, off, geo, osc):
    """one offset pair in ten moved: onto the border cells of the padded map, just outside it, or far outside it"""
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw = geo
    Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    P = Kh * Kw
    o = off.view(N, Ho, Wo, G, P, 2)
    zero = torch.zeros_like(off)
    bx, by = dcn_ref.positions(zero, H, W, G, Kh, Kw, sh, sw, ph, pw, dh, dw, osc)          # the positions without an offset
    shape = (N, Ho, Wo, G, P)
    moved = torch.rand(shape, generator=g) < 0.1
    kind = torch.randint(0, 3, shape, generator=g)
    for axis, base, size in ((0, bx, W + 2 * pw), (1, by, H + 2 * ph)):
        low = torch.rand(shape, generator=g) < 0.5
        j = torch.randint(0, 4, shape, generator=g).double() / 4                       # 0, 1/4, 1/2, 3/4
        mult = torch.randint(1, 4, shape, generator=g).double() * torch.where(low, -1.0, 1.0)
        border = torch.where(low, j, size - 1 - j)                                     # in the first / last cell, the integers included
        outside = torch.where(low, -0.25 - j, size - 1 + 0.25 + j)                     # up to one pixel beyond the first / last position
        far = base + mult * (W + 8)
        target = torch.where(kind == 0, border, torch.where(kind == 1, outside, far)).expand(shape)
        value = torch.round((target - base) / osc * 4) / 4                             # the multiple of 1/4 that comes closest
        o[..., axis] = torch.where(moved, value, o[..., axis])
    return off


def draw(r, kind):
    """(x, offset, mask, gy) on the CPU in fp64, every value one that fp32 holds; [N, H, W, C] layout"""
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw = r["geo"]
    Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    P, C = Kh * Kw, G * Cg
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Cg + (7 if kind == "exact" else 0))
    if kind == "exact":
        x = torch.randint(-8, 9, (N, H, W, C), generator=g).double() / 8
        m = torch.randint(0, 9, (N, Ho, Wo, G * P), generator=g).double() / 8
        gy = torch.randint(-2, 3, (N, Ho, Wo, C), generator=g).double()
        off = torch.round(8 * r["off_mul"] * torch.randn(N, Ho, Wo, G * P * 2, generator=g, dtype=torch.float64)) / 4
        off = _special_offsets(g, off, r["geo"], r["osc"])
    else:
        x = torch.randn(N, H, W, C, generator=g).double()
        m = torch.randn(N, Ho, Wo, G * P, generator=g).double()
        gy = torch.randn(N, Ho, Wo, C, generator=g).double()
        if r["wide_gy"]:
            gy = gy * torch.exp2(torch.randint(-20, 21, gy.shape, generator=g).double())
        off = torch.round(2 * r["off_mul"] * torch.randn(N, Ho, Wo, G * P * 2, generator=g, dtype=torch.float64) * 1024) / 1024
    for t in (x, off, m, gy):
        assert torch.equal(t.float().double(), t)
    return x, off, m, gy


def reference(r, maps, dtype=torch.float64):
    """dcn_ref.dcnv3 -- on the CPU, or for the two large rows on the device, an image at a time"""
    geo = r["geo"][3:] + (r["osc"],)
    if not r["blocks"]:
        return dcn_ref.dcnv3(*maps, *geo, dtype=dtype)
    parts = [dcn_ref.dcnv3(*(t[n:n + 1].cuda() for t in maps), *geo, dtype=dtype) for n in range(maps[0].shape[0])]
    return tuple(torch.cat(p) for p in zip(*parts))


def abs_sums(r, maps):
    geo = r["geo"][3:] + (r["osc"],)
    if not r["blocks"]:
        return dcn_ref.abs_sums(*maps, *geo)
    parts = [dcn_ref.abs_sums(*(t[n:n + 1].cuda() for t in maps), *geo) for n in range(maps[0].shape[0])]
    return tuple(torch.cat(p) for p in zip(*(a for a, _ in parts))), tuple(torch.cat(p) for p in zip(*(t for _, t in parts)))


# -------------------------------------------------------------------------------------------------------------- the entry points
def _device_map(t, misaligned):
    """t as an fp32 device tensor; misaligned: at an odd storage offset (4 bytes past a 16-byte boundary)"""
    if not misaligned:
        return t.float().cuda().contiguous()
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    out = buf[1:].view(t.shape)
    out.copy_(t.float())
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _nan_like(t, misaligned):
    return _device_map(torch.full(t.shape, float("nan")), misaligned)


def run_entry_points(ops, r, maps):
    """y, dx, doffset, dmask in the [N, H, W, C] layout, from lib.s2f_dcnv3_* on NaN-filled outputs"""
    lib = ops.lib
    x, off, m, gy = maps
    mis = r["misaligned"]
    if r["entry"] == "cm":
        x, gy = x.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2)
    dev = [_device_map(t.contiguous(), mis and i in (0, 3)) for i, t in enumerate((x, off, m, gy))]
    y, dx = _nan_like(dev[3], mis), _nan_like(dev[0], mis)
    doff, dm = _nan_like(dev[1], False), _nan_like(dev[2], False)
    sfx = "_cm" if r["entry"] == "cm" else ""
    fwd, bwd = getattr(lib, "s2f_dcnv3_fwd" + sfx), getattr(lib, "s2f_dcnv3_bwd" + sfx)
    assert fwd(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), y.data_ptr(), *r["geo"], r["osc"], None) == 0, lib.s2f_last_error()
    assert bwd(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dx.data_ptr(), doff.data_ptr(), dm.data_ptr(),
               *r["geo"], r["osc"], None) == 0, lib.s2f_last_error()
    torch.cuda.synchronize()
    if r["entry"] == "cm":
        y, dx = y.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)
    return y, dx, doff, dm


def run_wrappers(ops, r, maps):
    """the same through ops.dcnv3_core / ops.dcnv3_core_cm and autograd"""
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw = r["geo"]
    x, off, m, gy = (t.float().cuda() for t in maps)
    cm = r["entry"] == "cm"
    if cm:
        x, gy = x.permute(0, 3, 1, 2).contiguous(), gy.permute(0, 3, 1, 2).contiguous()
    a, b, c = (t.clone().requires_grad_(True) for t in (x, off, m))
    y = (ops.dcnv3_core_cm if cm else ops.dcnv3_core)(a, b, c, Kh, Kw, sh, sw, ph, pw, dh, dw, G, Cg, r["osc"])
    y.backward(gy)
    torch.cuda.synchronize()
    y, dx = y.detach(), a.grad
    if cm:
        y, dx = y.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)
    return y, dx, b.grad, c.grad


# -------------------------------------------------------------------------------------------------------------- the rows
def _route(ops, r):
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw = r["geo"]
    got = ops.dcnv3_route(N, H, W, Kh, Kw, sh, sw, ph, pw, dh, dw, G, Cg, aligned16=not r["misaligned"])
    want = {k: (getattr(ops, "DCN_" + v) if isinstance(v, str) else v) for k, v in r["want"].items()}
    assert {k: got[k] for k in want} == want, (r["id"], got)
    assert bool(got["cm"]) == ops.dcnv3_cm_ok(N, H, W, Kh, Kw, sh, sw, ph, pw, dh, dw, G, Cg)
    if r["entry"] == "nhwc" and r["id"].startswith("grid-"):
        Ho, Wo = dcn_ref.out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
        assert N * Ho * Wo * G > 4096 * 256          # csrc/dcnv3.hip grid_for: at most 4096 blocks of 256 threads


@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("r", ROWS)
def test_route_against_fp64(ops, monkeypatch, r, kind):
    if r["force"] is not None:
        monkeypatch.setenv("S2F_DCN_FORCE_BANDS", str(r["force"]))
    else:
        monkeypatch.delenv("S2F_DCN_FORCE_BANDS", raising=False)
    _route(ops, r)                                                                                      # 1. the route
    N, H, W, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw = r["geo"]
    maps = draw(r, kind)
    ref = reference(r, maps)
    A, T = abs_sums(r, maps)
    px64, py64 = dcn_ref.positions(maps[1], H, W, G, Kh, Kw, sh, sw, ph, pw, dh, dw, r["osc"], torch.float64)
    px32, py32 = dcn_ref.positions(maps[1], H, W, G, Kh, Kw, sh, sw, ph, pw, dh, dw, r["osc"], torch.float32)
    assert torch.equal(px32.double(), px64) and torch.equal(py32.double(), py64), "fp32 and fp64 would sample at different positions"
    if kind == "exact":
        for name, a in zip(NAMES, A):
            assert a.max().item() * GRANULES[name] < 2 ** 24, name
        assert torch.equal(px64 * 8, torch.round(px64 * 8)) and torch.equal(py64 * 8, torch.round(py64 * 8))
        for name, t in zip(NAMES, ref):
            assert (t != 0).double().mean().item() >= 0.25, f"{name}: the draw leaves fewer than a quarter of the entries non-zero"
        ix, iy = torch.floor(px64) - pw, torch.floor(py64) - ph
        inside = [(ix + ex >= 0) & (ix + ex < W) & (iy + ey >= 0) & (iy + ey < H) for ey in (0, 1) for ex in (0, 1)]
        n_in, n_all = sum(int(t.sum()) for t in inside), sum(t.numel() for t in inside)
        assert 0 < n_in < n_all, "corners inside and outside the map must both occur"
        assert bool(((px64 < -8) | (px64 > W + 2 * pw + 8)).any()), "no position far outside the map"
        assert bool(((px64 == torch.floor(px64)) & (px64 >= 0) & (px64 <= W + 2 * pw - 1)).any()), "no exactly integer position on the map"

    def compare(got, what):
        worst = {}
        for name, t, want, a, cnt in zip(NAMES, got, ref, A, T):
            t = t.to(want.device).double()
            assert t.shape == want.shape, (what, name)
            assert not bool(torch.isnan(t).any()), f"{what}: {name} keeps NaN from the pre-filled buffer"
            if kind == "exact":
                assert torch.equal(t, want), f"{what}: {name} differs from fp64 in {int((t != want).sum())} of {t.numel()} entries, " \
                                             f"by up to {(t - want).abs().max().item():.3e}"
            else:
                err = (t - want).abs()
                worst[name] = (err / a.clamp_min(1e-300)).max().item()
                bound = 1.01 * (cnt + 6) * 2.0 ** -24 * a + 1e-30
                bad = err > bound
                assert not bool(bad.any()), f"{what}: {name} outside the fp32 bound in {int(bad.sum())} of {t.numel()} entries, " \
                                            f"worst |err| / bound {(err / bound).max().item():.3e}, worst |err| / A {worst[name]:.3e}"
        return worst

    got = run_entry_points(ops, r, maps)                                                                # 2. - 4.
    worst = compare(got, "entry points")
    if not r["misaligned"] and not r["blocks"]:
        compare(run_wrappers(ops, r, maps), "autograd wrapper")
    if kind == "general":
        cpu32 = reference(r, maps, dtype=torch.float32)
        w32 = {name: ((t.double() - want).abs() / a.clamp_min(1e-300)).max().item() for name, t, want, a in zip(NAMES, cpu32, ref, A)}
        print(f"\nDCNROW {r['id']:38s} {str(r['geo']).replace(' ', ''):36s} " +
              "   ".join(f"{n} {worst[n]:.1e} | {w32[n]:.1e}" for n in NAMES))
