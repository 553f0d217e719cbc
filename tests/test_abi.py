"""CPU: the C-ABI library loads and exports every symbol include/s2f.h declares, and the ctypes table in
spike2former_amd/_lib.py has the same arity (no compute calls here -- there is no GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t|void\s*\*?|const char\s*\*)\s*(s2f_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_header_declares_the_path():
    d = _declared()
    for need in ("s2f_lif_fwd", "s2f_lif_bwd", "s2f_lif_seq_fwd", "s2f_lif_seq_bwd", "s2f_sdsa_fwd", "s2f_sdsa_bwd",
                 "s2f_dcnv3_fwd", "s2f_dcnv3_bwd", "s2f_version", "s2f_last_error"):
        assert need in d


def test_library_exports_every_declared_symbol():
    path = os.path.join(ROOT, "spike2former_amd", "libs2f_hip.so")
    assert os.path.exists(path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(path)
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/s2f.h but not exported"
    lib.s2f_version.restype = ctypes.c_int
    want = int(re.search(r"#define S2F_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "s2f.h")).read()).group(1))
    assert lib.s2f_version() == want
    lib.s2f_lif_mask_words.restype = ctypes.c_int64
    lib.s2f_lif_mask_words.argtypes = [ctypes.c_int64]
    assert [lib.s2f_lif_mask_words(n) for n in (0, 1, 256, 257, 1024)] == [0, 4, 4, 8, 16]


def test_ctypes_table_matches_header():
    from spike2former_amd import _lib
    d = _declared()
    assert set(_lib.SIGNATURES) == set(d)
    for name, (_, args) in _lib.SIGNATURES.items():
        assert len(args) == d[name], f"{name}: ctypes has {len(args)} args, header has {d[name]}"


def test_mirrored_constants_match_the_header():
    """The constants of include/s2f.h that the op layer copies by hand, each against its `#define S2F_<NAME> <integer>` line."""
    import torch
    from spike2former_amd import ops
    src = open(os.path.join(ROOT, "include", "s2f.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define S2F_(\w+)[ \t]+(\d+)[ \t]*$", src, flags=re.M)}
    mirrors = {
        "STAT_SLOTS": ops.STAT_SLOTS, "RESIZE_ALIGN_CORNERS": ops.RESIZE_ALIGN_CORNERS, "RESIZE_SIGMOID": ops.RESIZE_SIGMOID,
        "RESIZE_FLIP_H": ops.RESIZE_FLIP_H, "RESIZE_FLIP_V": ops.RESIZE_FLIP_V,
        "SEG_HIST_MAX_CLASSES": ops.SEG_HIST_MAX_CLASSES, "SEG_CONF_LDS_BYTES": ops.SEG_CONF_LDS_BYTES,
        "SEG_CONF_GLOBAL": ops._SEG_CONF_GLOBAL, "SEG_DRAW_BGR": ops._SEG_DRAW_BGR,
        "AUG_CANDIDATES": ops.AUG_CANDIDATES, "AUG_MAX_CROP": ops.AUG_MAX_CROP, "LSA_MAX_QUERIES": ops.LSA_MAX_QUERIES,
        "LSA_MAX_CLASSES": ops.LSA_MAX_CLASSES, "LSA_TILE_L2": ops.LSA_TILE_L2,
        "CENSUS_FIELDS": ops.CENSUS_FIELDS, "CENSUS_F32": ops._CENSUS_DTYPES[torch.float32],
        "CENSUS_BF16": ops._CENSUS_DTYPES[torch.bfloat16], "TRAIN_LOG_MAX_TERMS": ops.TRAIN_LOG_MAX_TERMS,
        "DCN_ROUTE_FIELDS": ops.DCN_ROUTE_FIELDS, "DCN_FWD_K3C8": ops.DCN_FWD_K3C8, "DCN_FWD_VEC4": ops.DCN_FWD_VEC4,
        "DCN_FWD_SCALAR": ops.DCN_FWD_SCALAR, "DCN_BWD_LDS": ops.DCN_BWD_LDS, "DCN_BWD_BANDED": ops.DCN_BWD_BANDED,
        "DCN_BWD_ATOMIC_VEC4": ops.DCN_BWD_ATOMIC_VEC4, "DCN_BWD_ATOMIC_SCALAR": ops.DCN_BWD_ATOMIC_SCALAR,
        "DCN_CM_FWD_K3C8": ops.DCN_CM_FWD_K3C8, "DCN_CM_FWD_GENERIC": ops.DCN_CM_FWD_GENERIC, "DCN_CM_BWD_PLAIN": ops.DCN_CM_BWD_PLAIN,
        "DCN_CM_BWD_PIPE": ops.DCN_CM_BWD_PIPE, "DCN_CM_BWD_PIPE_K3C8": ops.DCN_CM_BWD_PIPE_K3C8,
    }
    # every S2F_DCN_* id of the header is mirrored, and no two routes share a number
    dcn = {k: v for k, v in header.items() if k.startswith("DCN_")}
    assert set(dcn) == {k for k in mirrors if k.startswith("DCN_")}
    ids = [v for k, v in dcn.items() if k != "DCN_ROUTE_FIELDS"]
    assert len(set(ids)) == len(ids) == 12
    assert len(ops._CENSUS_DTYPES) == 2
    for name, value in mirrors.items():
        assert name in header, f"include/s2f.h has no integer #define S2F_{name}"
        assert type(value) is int and value == header[name], f"ops mirrors S2F_{name} as {value!r}, include/s2f.h says {header[name]}"


def test_argument_errors_are_reported_without_a_gpu():
    """Validation happens before any launch, so the error convention can be checked on CPU."""
    from spike2former_amd._lib import lib
    assert lib.s2f_lif_fwd(None, None, None, None, None, None, None, 16, 1.0, 8, 0, None) == -1
    assert b"null" in lib.s2f_last_error()
    assert lib.s2f_dcnv3_fwd(1, 1, 1, 1, 0, 4, 4, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.s2f_sdsa_fwd(1, 1, 1, 1, 1, 1, 8, 65, 4, 4, 1.0, None) == -1     # head dim > 64


def test_unknown_tile_cfg_is_an_error_before_any_launch():
    """Every entry point whose `cfg` selects a tile from a table refuses a value that is not in the table: S2F_EINVAL and
    "unknown cfg", after the pointer / size preconditions (aligned dummy pointers, valid sizes) and before any launch, so no GPU
    is needed.  (The cfg of the s2f_spike_*_dw_pipe entry points is a schedule flag / bit set, not a table index: every value
    of it runs.)"""
    from spike2former_amd._lib import lib
    P = 1 << 20          # a 16-byte aligned dummy address: never dereferenced on the host
    calls = {
        # (Mo = 64 keeps the contraction unsplit: a split would clear DX with a launch before the tile is chosen)
        "s2f_pgemm_nn_bf16": lambda: lib.s2f_pgemm_nn_bf16(P, P, None, P, 1, 64, 128, 64, 3, 99, None),
        "s2f_pgemm_dx_f32": lambda: lib.s2f_pgemm_dx_f32(P, P, 0, P, 0, 1, 64, 64, 128, 0.0, 99, None),
        "s2f_pgemm_dx_split": lambda: lib.s2f_pgemm_dx_split(P, P, 64 * 128, P, 1, 64, 64, 128, 99, None),
        "s2f_pgemm_conv3x3_bf16": lambda: lib.s2f_pgemm_conv3x3_bf16(P, P, None, P, 1, 64, 32, 16, 16, 99, None),
        "s2f_pgemm_conv3x3_f32": lambda: lib.s2f_pgemm_conv3x3_f32(P, P, P, 1, 64, 32, 16, 16, 99, None),
    }
    for name, call in calls.items():
        assert call() == -1, name          # S2F_EINVAL
        assert b"unknown cfg" in lib.s2f_last_error(), (name, lib.s2f_last_error())
