"""The attention backward's three apply products gq, gk, gv as grouped launches (sdsa_apply_jobs_kernel in spike2former_amd/csrc/sdsa.hip:
jobs that take the same workgroup shape share one launch, the job is the grid's z index).

  (a) through s2f_sdsa_apply_jobs, general (randn) go, kv and gkv: one 3-job call EQUALS three 1-job calls, and the 1-job call of the
      fp32 operand equals s2f_sdsa_apply (the single-job kernel the jobs kernel shares its body with).
  (b) through ops.sdsa / ops.sdsa_packed backward on the exact draws of test_gpu_attention (spikes k / 8, integer gradients, power-of-two
      scale, every sum of absolute terms below 2^24 granules -- asserted on the draw): gq, gk, gv EQUAL the fp64 values of attn_ref.
  (c) a malformed job returns the error code before anything is launched: the outputs of ALL jobs of the call keep their sentinel.

Shapes (TB, heads, d, Nq, Nk): the smallest at which the grouping can go wrong; what each exercises is its id and the inequality
asserted on it.  Draws, runners and comparisons are those of tests/test_gpu_attention.py."""
import ctypes
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref  # noqa: E402
import test_gpu_attention as base  # noqa: E402

pytestmark = pytest.mark.gpu

JOB_WORDS = 11          # S2F_SDSA_JOB_WORDS of include/s2f.h


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


def workgroups(TB, heads, N):
    return TB * heads * base.cdiv(N, 256)


def same_shape(TB, heads, d, Nq, Nk):
    """gq and gk / gv take the same workgroup shape: both sides of the 1 024-workgroup threshold alike, or d <= 8 (always four waves)"""
    return d <= 8 or (workgroups(TB, heads, Nq) > 1024) == (workgroups(TB, heads, Nk) > 1024)


SHAPES = [
    pytest.param((2, 2, 32, 100, 100), lambda TB, h, d, Nq, Nk: same_shape(TB, h, d, Nq, Nk) and Nq < 256 and Nq % 256 != 0,
                 id="decoder-self-one-partly-filled-chunk"),
    pytest.param((2, 2, 32, 100, 264), lambda TB, h, d, Nq, Nk: same_shape(TB, h, d, Nq, Nk) and base.cdiv(Nq, 256) < base.cdiv(Nk, 256)
                 and Nk % 16 == 8, id="gq-has-fewer-chunks-than-the-launch-ragged"),
    pytest.param((1, 2, 45, 264, 264), lambda TB, h, d, Nq, Nk: same_shape(TB, h, d, Nq, Nk) and d % 4 != 0 and d > 32,
                 id="eight-waves-jc8-d45"),
    pytest.param((1, 2, 8, 260, 260), lambda TB, h, d, Nq, Nk: d <= 8 and workgroups(TB, h, Nk) <= 1024, id="four-waves-small-grid-d8"),
    pytest.param((8, 8, 32, 100, 4352), lambda TB, h, d, Nq, Nk: workgroups(TB, h, Nk) > 1024 >= workgroups(TB, h, Nq) and d > 8,
                 id="gq-eight-waves-alone-gk-gv-four-waves"),
]


# ---------------------------------------------------------------------------------------------------------------- (a) and (c): the jobs
def job_words(x, x_bs, m, y, y_bs, N, alpha, trans, mask=None, D=0):
    (alpha_bits,) = struct.unpack("<I", struct.pack("<f", alpha))
    return [x.data_ptr(), x_bs, 1 if x.dtype == torch.bfloat16 else 0, 0 if mask is None else mask.data_ptr(), D, m.data_ptr(),
            y.data_ptr(), y_bs, N, alpha_bits, int(trans)]


def apply_jobs(jobs, TB, heads, d):
    """-> the return code of ONE s2f_sdsa_apply_jobs call"""
    from spike2former_amd._lib import lib
    from spike2former_amd.ops.core import _stream
    words = [w for j in jobs for w in j]
    assert len(words) == JOB_WORDS * len(jobs)
    table = (ctypes.c_int64 * len(words))(*words)
    rc = lib.s2f_sdsa_apply_jobs(ctypes.addressof(table), len(jobs), TB, heads, d, _stream())
    torch.cuda.synchronize()
    return rc


def general_triple(TB, heads, d, Nq, Nk, seed, packed=False, masked=False):
    """the backward's three applies on general operands -> (job_of(y_gq, y_gk, y_gv) -> three job word lists, output shapes / strides)"""
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    go = torch.randn(TB, C, Nq, generator=g).cuda()
    kv, gkv = (torch.randn(TB, heads, d, d, generator=g).cuda() for _ in range(2))
    if packed:
        assert Nq == Nk
        qkv = (torch.randint(0, 9, (TB, 3 * C, Nk), generator=g).float() / 8).to(torch.bfloat16).cuda()
        k, v, s_bs = qkv[:, C:2 * C], qkv[:, 2 * C:], 3 * C * Nk
    else:
        k, v = ((torch.randint(0, 9, (TB, C, Nk), generator=g).float() / 8).to(torch.bfloat16).cuda() for _ in range(2))
        s_bs = C * Nk
    mask = None
    if masked:
        bits = torch.rand(TB, C, Nq, generator=g) < 0.5
        mask = attn_ref.pack_mask(bits).cuda()
    scale = d ** -0.5
    keep = (go, kv, gkv, k, v, mask)

    def jobs(ys, y_bs):
        return [job_words(go, C * Nq, kv, ys[0], y_bs[0], Nq, scale, True, mask, 8 if masked else 0),
                job_words(v, s_bs, gkv, ys[1], y_bs[1], Nk, 1.0, True),
                job_words(k, s_bs, gkv, ys[2], y_bs[2], Nk, 1.0, False)]
    return jobs, keep, scale


def outputs(TB, C, Nq, Nk, packed):
    """three sentinel-filled outputs: tensors of their own, or the channel ranges of one [TB, 3C, N] tensor"""
    if packed:
        whole = torch.full((TB, 3 * C, Nq), -7.0, device="cuda")
        return whole, [whole[:, :C], whole[:, C:2 * C], whole[:, 2 * C:]], [3 * C * Nq] * 3
    ys = [torch.full((TB, C, n), -7.0, device="cuda") for n in (Nq, Nk, Nk)]
    return ys, ys, [C * Nq, C * Nk, C * Nk]


def grouped_equals_single(TB, heads, d, Nq, Nk, packed=False, masked=False):
    C = heads * d
    jobs, keep, scale = general_triple(TB, heads, d, Nq, Nk, seed=Nq + Nk + d, packed=packed, masked=masked)
    _, ys3, y_bs = outputs(TB, C, Nq, Nk, packed)
    assert apply_jobs(jobs(ys3, y_bs), TB, heads, d) == 0
    _, ys1, _ = outputs(TB, C, Nq, Nk, packed)
    for j in jobs(ys1, y_bs):
        assert apply_jobs([j], TB, heads, d) == 0
    for name, a, b in zip(("gq", "gk", "gv"), ys3, ys1):
        assert not bool((b == -7.0).all()), name
        assert torch.equal(a, b), name
    return keep, scale, ys1


@pytest.mark.parametrize("shape,on_route", SHAPES)
def test_three_jobs_equal_three_single_jobs(shape, on_route):
    TB, heads, d, Nq, Nk = shape
    assert on_route(*shape)
    (go, kv, *_), scale, ys1 = grouped_equals_single(*shape)
    # the fp32 job against the single-job kernel of the same body
    from spike2former_amd._lib import check, lib
    from spike2former_amd.ops.core import _ptr, _stream
    y = torch.empty_like(go)
    check(lib.s2f_sdsa_apply(_ptr(go), _ptr(kv), _ptr(y), TB, heads, d, Nq, scale, 1, _stream()), "s2f_sdsa_apply")
    assert torch.equal(ys1[0], y)


def test_three_jobs_equal_three_single_jobs_packed():
    grouped_equals_single(2, 2, 32, 256, 256, packed=True)


def test_three_jobs_equal_three_single_jobs_masked_gradient():
    """the gq job carries the straight-through mask, the other two none"""
    TB, heads, d, N = 2, 2, 32, 256
    (go, kv, _, _, _, mask), scale, ys1 = grouped_equals_single(TB, heads, d, N, N, masked=True)
    y = torch.full_like(go, -7.0)
    assert apply_jobs([job_words(go, heads * d * N, kv, y, heads * d * N, N, scale, True)], TB, heads, d) == 0
    assert not torch.equal(y, ys1[0])          # the same job without its mask


def test_fp32_operands_three_jobs_equal_three_single_jobs():
    TB, heads, d, Nq, Nk = 2, 2, 32, 100, 264
    C = heads * d
    g = torch.Generator().manual_seed(5)
    go, v, k = (torch.randn(TB, C, n, generator=g).cuda() for n in (Nq, Nk, Nk))
    kv, gkv = (torch.randn(TB, heads, d, d, generator=g).cuda() for _ in range(2))

    def jobs(ys):
        return [job_words(go, C * Nq, kv, ys[0], C * Nq, Nq, 0.25, True), job_words(v, C * Nk, gkv, ys[1], C * Nk, Nk, 1.0, True),
                job_words(k, C * Nk, gkv, ys[2], C * Nk, Nk, 1.0, False)]
    ys3, ys1 = ([torch.full((TB, C, n), -7.0, device="cuda") for n in (Nq, Nk, Nk)] for _ in range(2))
    assert apply_jobs(jobs(ys3), TB, heads, d) == 0
    for j in jobs(ys1):
        assert apply_jobs([j], TB, heads, d) == 0
    for a, b in zip(ys3, ys1):
        assert torch.equal(a, b) and not bool((b == -7.0).any())


@pytest.mark.parametrize("fault", ["batch-stride-not-a-multiple-of-4", "misaligned-spike-pointer"])
def test_malformed_job_is_an_error_and_writes_nothing(fault):
    from spike2former_amd._lib import lib
    TB, heads, d, Nq, Nk = 2, 2, 32, 100, 100
    C = heads * d
    jobs, keep, _ = general_triple(TB, heads, d, Nq, Nk, seed=3)
    ys, _, y_bs = outputs(TB, C, Nq, Nk, False)
    table = jobs(ys, y_bs)
    bad = table[2]                                   # the LAST job: the two before it are well formed and must not run either
    if fault == "batch-stride-not-a-multiple-of-4":
        bad[1] += 2
        want = -1                                    # S2F_EINVAL
    else:
        bad[0] += 4                                  # two bf16 elements: 4-byte, not 8-byte aligned
        want = -2                                    # S2F_EALIGN
    assert apply_jobs(table, TB, heads, d) == want
    assert lib.s2f_last_error() != b""
    for y in ys:
        assert bool((y == -7.0).all())
    assert apply_jobs([bad], TB, heads, d) == want
    assert bool((ys[2] == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- (b): the backward
@pytest.mark.parametrize("shape,on_route", SHAPES)
def test_bf16_backward_equals_fp64(ops, shape, on_route):
    TB, heads, d, Nq, Nk = shape
    assert on_route(*shape)
    q, k, v, go = base.draw_exact(*shape, seed=d * 1000 + Nq + Nk)
    base.assert_sums_exact(q, k, v, go, heads)
    scale = 0.125
    got = base.run_bf16(ops, q, k, v, go, heads, scale, False)
    base.assert_equal64(got[:4], base.reference(q, k, v, go, heads, scale))


def test_packed_backward_equals_fp64(ops):
    """batch strides 3 C N; the three gradients are channel ranges of one [TB, 3C, N] tensor"""
    shape = (2, 2, 32, 256, 256)
    TB, heads, d, Nq, Nk = shape
    q, k, v, go = base.draw_exact(*shape, seed=77)
    base.assert_sums_exact(q, k, v, go, heads)
    scale = 0.125
    got = base.run_bf16(ops, q, k, v, go, heads, scale, True)
    base.assert_equal64(got[:4], base.reference(q, k, v, go, heads, scale))


def test_fused_neuron_backward_equals_fp64(ops):
    """the gq job carries the straight-through mask (go_mask, D) of the fused forward, gk and gv none"""
    TB, heads, d, N = 2, 2, 32, 256
    q, k, v, g = base.draw_exact(TB, heads, d, N, N, seed=78)
    scale = base.fused_scale(q, k, v, heads)
    o64, _ = attn_ref.forward(q, k, v, heads, scale)
    inr = attn_ref.in_range(o64)
    assert bool(inr.any()) and not bool(inr.all())
    go = attn_ref.fused_grad(o64, g)
    base.assert_sums_exact(q, k, v, go, heads, go_den=8)
    y, _, mask, gq, gk, gv = base.run_fused(ops, q, k, v, g, heads, scale, False)
    assert torch.equal(y.cpu().double(), attn_ref.neuron(o64)[0]) and torch.equal(mask.cpu(), attn_ref.pack_mask(inr))
    base.assert_equal64((gq, gk, gv), attn_ref.backward(q, k, v, go, heads, scale)[:3], base.NAMES[1:])


def test_fp32_backward_equals_fp64(ops):
    """s2f_sdsa_bwd: three fp32 jobs of one shape"""
    shape = (2, 2, 32, 100, 100)
    TB, heads, d, Nq, Nk = shape
    q, k, v, go = base.draw_exact(*shape, seed=79)
    base.assert_sums_exact(q, k, v, go, heads)
    scale = 0.125
    base.assert_equal64(base.run_fp32(ops, q, k, v, go, heads, scale), base.reference(q, k, v, go, heads, scale))
