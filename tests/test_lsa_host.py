"""The device-side Hungarian assignment without a GPU: the C ABI's declaration and validation, and the `assign` argument of the
loss and of the captured step (no silent fall-back to the host route on CPU tensors)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lsa_tables_symbol_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "spike2former_amd", "libs2f_hip.so"))
    from spike2former_amd import _lib, ops
    assert re.search(r"\bint\s+s2f_lsa_tables\s*\(", src)
    assert hasattr(lib, "s2f_lsa_tables") and "s2f_lsa_tables" in _lib.SIGNATURES
    q = int(re.search(r"#define S2F_LSA_MAX_QUERIES (\d+)", src).group(1))
    k = int(re.search(r"#define S2F_LSA_MAX_CLASSES (\d+)", src).group(1))
    assert q >= 100 and 150 <= k < 255 and (ops.LSA_MAX_QUERIES, ops.LSA_MAX_CLASSES) == (q, k)
    assert "lsa.hip" in open(os.path.join(ROOT, "spike2former_amd", "csrc", "Makefile")).read()


def test_lsa_tables_argument_errors_without_a_gpu():
    from spike2former_amd import ops
    from spike2former_amd._lib import lib
    p = ctypes.c_void_p(64)           # never dereferenced: validation fails before any launch
    ok = dict(L=7, B=2, Q=100, K=150)

    def call(ptrs=(p,) * 6, **kw):
        a = dict(ok, **kw)
        return lib.s2f_lsa_tables(*ptrs, a["L"], a["B"], a["Q"], a["K"], None)
    for i in range(6):
        assert call(ptrs=tuple(None if j == i else p for j in range(6))) == -1 and b"null" in lib.s2f_last_error()
    assert call(K=255) == -1 and b"K 255" in lib.s2f_last_error() and b"ignored label" in lib.s2f_last_error()
    assert call(K=0) == -1 and b"K 0" in lib.s2f_last_error()
    assert call(Q=0) == -1 and b"Q 0" in lib.s2f_last_error()
    assert call(L=0) == -1 and call(B=0) == -1
    assert call(Q=ops.LSA_MAX_QUERIES + 1) == -1 and b"Q 257" in lib.s2f_last_error()
    assert call(ptrs=(p, p, ctypes.c_void_p(68), p, p, p)) == -2          # the int64 table on a 4-byte boundary


def _crit():
    from spike2former_amd.loss import MaskFormerLoss
    return MaskFormerLoss(20, 10)


def _cpu_case(crit, L=2, B=1, h=4):
    g = torch.Generator().manual_seed(0)
    cls = torch.randn(L, B, crit.num_queries, crit.num_classes + 1, generator=g)
    masks = torch.randn(L, B, crit.num_queries, h, h, generator=g)
    seg = torch.randint(0, crit.num_classes, (B, 2 * h, 2 * h), generator=g)
    return cls, masks, seg


def test_loss_semantic_rejects_an_unknown_assign():
    crit = _crit()
    cls, masks, seg = _cpu_case(crit)
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="assign must be 'host' or 'device'"):
            crit.loss_semantic(cls, masks, seg, assign=bad)


def test_loss_semantic_device_route_does_not_fall_back_on_cpu_tensors():
    crit = _crit()
    cls, masks, seg = _cpu_case(crit)
    with pytest.raises(RuntimeError, match="assign='device'.*CUDA"):
        crit.loss_semantic(cls, masks, seg, assign="device")
    with pytest.raises(RuntimeError, match="GPU only"):
        crit.match_tables_device(torch.zeros(2, 1, 10, 20), torch.zeros(1, 256))


def test_status_word_raises_the_host_routes_errors():
    crit = _crit()
    crit.raise_for_status(0)
    with pytest.raises(ValueError, match="labels >= num_classes"):
        crit.raise_for_status(1)
    with pytest.raises(ValueError, match="labels >= num_classes"):
        crit.raise_for_status(3)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        crit.raise_for_status(2)


def test_graphed_hungarian_step_checks_assign_before_anything_else():
    from spike2former_amd.graph import GraphedHungarianStep
    x, seg = torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8, dtype=torch.int64)
    for bad in ("gpu", None):
        with pytest.raises(ValueError, match="assign must be 'host' or 'device'"):
            GraphedHungarianStep(None, x, seg, None, assign=bad)
    with pytest.raises(RuntimeError, match="assign='device'.*CUDA"):
        GraphedHungarianStep(None, x, seg, None, assign="device")
