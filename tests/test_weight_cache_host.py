"""The bookkeeping of the weight-conversion cache, on the CPU: the module that launches gets a recording stand-in for the kernel
library, so the five conversion functions, ops.resplit_all and ops.conversion_state run on CPU tensors and every launch is seen
with its arguments.  Public names only: the one patch target is found from ops.split_weight in the fixture `rec`."""
import ctypes
import gc
import sys

import numpy as np
import pytest
import torch

from spike2former_amd import ops

CPU = torch.device("cpu")
SPLIT, PACK = "s2f_split_bf16x3", "s2f_pack_bf16x3"


def _up(n, m):
    return (n + m - 1) // m * m


def _pack_elems(M, K):
    return (_up(M, 64) // 64) * (_up(K, 32) // 32) * 6144


class _Recorder:
    """Stands in for the ctypes library: every entry point returns 0 and is noted as (name, args).  The fp32 source matrix of a
    per-weight split is copied at launch time (a tap-major source is a temporary that is gone afterwards)."""

    def __init__(self):
        self.calls, self.split_sources = [], []

    def s2f_pack_elems(self, M, K):
        return _pack_elems(M, K)

    def __getattr__(self, name):
        def launch(*args):
            self.calls.append((name, args))
            if name == SPLIT:
                src, _dst, M, K = args[:4]
                self.split_sources.append(np.array((ctypes.c_float * (M * K)).from_address(src), dtype=np.float32).reshape(M, K))
            return 0
        return launch

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(monkeypatch):
    mod = sys.modules[ops.split_weight.__module__]          # the module that launches the conversions
    r = _Recorder()
    monkeypatch.setattr(mod, "lib", r)
    monkeypatch.setattr(mod, "_stream", lambda: 0)
    # ops.begin_step also arms the reduction arena: give it a private one, so that no CPU buffer outlives the test
    monkeypatch.setattr(ops.core, "_ARENA", {"buf": None, "pos": 0, "high": 0, "armed": False})
    ops.clear_conversions()
    yield r
    ops.begin_step()                                         # no device, no capture: only switches the trust off again
    ops.clear_conversions()


def _weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(100, 72, generator=g), torch.randn(40, 32, 3, 3, generator=g)


# the seven layouts in the order the tests convert them: name -> (conversion, which weight, launch, what the launch gets after the
# two pointers).  Splits: (M, K, Mpad, Kpad); packs: (M, K, mode, C).
LAYOUTS = [
    ("split", lambda w, wc: ops.split_weight(w), "w", SPLIT, (100, 72, 128, 96)),
    ("split_tap", lambda w, wc: ops.split_weight_conv3(wc), "wc", SPLIT, (40, 288, 64, 288)),
    ("split_flip", lambda w, wc: ops.split_weight_tconv3(wc), "wc", SPLIT, (32, 360, 128, 384)),
    ("pack", lambda w, wc: ops.pack_weight(w), "w", PACK, (100, 72, 0, 0)),
    ("pack_t", lambda w, wc: ops.pack_weight(w, transposed=True), "w", PACK, (72, 100, 3, 0)),
    ("pack_tap", lambda w, wc: ops.pack_weight_conv3(wc), "wc", PACK, (40, 288, 1, 32)),
    ("pack_flip", lambda w, wc: ops.pack_weight_conv3(wc, transposed=True), "wc", PACK, (32, 360, 2, 40)),
]
MODE_WORDS = {"split": 0, "split_tap": 1 | 32 << 8, "split_flip": 2 | 40 << 8, "pack": 0, "pack_t": 3, "pack_tap": 8193, "pack_flip": 10242}
FIRST = {"split": 0, "split_tap": 12, "split_flip": 30, "pack": 0, "pack_t": 12, "pack_tap": 28, "pack_flip": 46}


def _convert_all(w, wc):
    return {name: fn(w, wc) for name, fn, *_ in LAYOUTS}


def _bump(*ts):
    with torch.no_grad():
        for t in ts:
            t.mul_(1.5)


@pytest.mark.parametrize("name,fn,which,launch,dims", LAYOUTS, ids=[row[0] for row in LAYOUTS])
def test_each_layout_launches_once_then_hits(rec, name, fn, which, launch, dims):
    w, wc = _weights()
    out = fn(w, wc)
    (got, args), = rec.take()
    assert got == launch and args[1] == out.data_ptr() and args[2:] == dims + (0,)
    assert out.dtype == torch.int16 and out.device == CPU
    src = {"w": w, "wc": wc}[which]
    if launch == PACK:
        assert args[0] == src.data_ptr()                     # the pack kernel reads every layout from the weight itself
        assert tuple(out.shape) == (_pack_elems(dims[0], dims[1]),)
    else:
        assert tuple(out.shape) == (3,) + dims[2:]
        # the per-weight split kernel takes no mode: the tap-major and flipped-transposed matrices are ATen copies
        want = {"split": w, "split_tap": wc.permute(0, 2, 3, 1).reshape(40, 288),
                "split_flip": wc.flip(2, 3).permute(1, 2, 3, 0).reshape(32, 360)}[name]
        assert (args[0] == w.data_ptr()) == (name == "split")
        assert np.array_equal(rec.split_sources[0], want.numpy())
    assert fn(w, wc) is out and rec.take() == []


def test_job_rows_after_resplit_all(rec):
    w, wc = _weights()
    outs = _convert_all(w, wc)
    rec.take()
    assert ops.resplit_all(CPU) == 7
    jobs, pack_jobs, bufs = ops.conversion_state()
    assert tuple(jobs.shape) == (3, 8) and tuple(pack_jobs.shape) == (4, 8) and jobs.dtype == pack_jobs.dtype == torch.int64
    assert sorted(b.data_ptr() for b in bufs) == sorted(o.data_ptr() for o in outs.values())
    rows = {r[1]: r for r in jobs.tolist() + pack_jobs.tolist()}          # by destination
    first = {SPLIT: 0, PACK: 0}
    for name, _fn, which, launch, dims in LAYOUTS:
        src = (w if which == "w" else wc).data_ptr()
        M, K = dims[:2]
        assert first[launch] == FIRST[name]
        if launch == SPLIT:
            Mpad, Kpad = dims[2:]
            assert rows[outs[name].data_ptr()] == [src, outs[name].data_ptr(), M, K, Mpad, Kpad, MODE_WORDS[name], first[launch]]
            first[launch] += (Mpad * Kpad + 1023) // 1024          # include/s2f.h: one workgroup per 1024 padded elements
        else:
            assert rows[outs[name].data_ptr()] == [src, outs[name].data_ptr(), M, K, MODE_WORDS[name], first[launch], 0, 0]
            first[launch] += (_up(M, 64) // 64) * (_up(K, 32) // 32) * 2          # two workgroups per 64 x 32 block
    assert rec.take() == [("s2f_split_bf16x3_multi", (jobs.data_ptr(), 3, first[SPLIT], 0)),
                          ("s2f_pack_bf16x3_multi", (pack_jobs.data_ptr(), 4, first[PACK], 0))]
    assert (first[SPLIT], first[PACK]) == (78, 70)


def test_in_place_update_converts_into_the_same_buffer(rec):
    w, wc = _weights()
    outs = _convert_all(w, wc)
    assert ops.resplit_all(CPU) == 7
    tables = ops.conversion_state()[:2]
    ptrs = {k: o.data_ptr() for k, o in outs.items()}
    _bump(w, wc)
    rec.take()
    for name, fn, _which, launch, dims in LAYOUTS:
        out = fn(w, wc)
        (got, args), = rec.take()
        assert got == launch and args[1] == ptrs[name] == out.data_ptr() and args[2:] == dims + (0,)
        assert out is outs[name]
    assert ops.resplit_all(CPU, build=False) == 7                     # the tables were not invalidated ...
    assert ops.conversion_state()[0] is tables[0] and ops.conversion_state()[1] is tables[1]          # ... nor replaced


def test_owner_not_address(rec):
    arr = np.random.default_rng(0).standard_normal((100, 72)).astype(np.float32)
    a, b = torch.from_numpy(arr), torch.from_numpy(arr)
    assert a.data_ptr() == b.data_ptr() and a._version == b._version == 0 and a._base is None and b._base is None
    for fn in (ops.split_weight, ops.pack_weight):
        sa = fn(a)
        sb = fn(b)
        assert len(rec.take()) == 2
        assert sa is not sb and sa.data_ptr() != sb.data_ptr()


def test_concatenation_attributes(rec):
    flat = torch.randn(100 * 72, generator=torch.Generator().manual_seed(1))
    halves = [flat[:50 * 72].view(50, 72), flat[50 * 72:].view(50, 72)]

    def cat(version):                                                  # as backbone_sdtv2._qkv_batched does
        c = ops.cat_params(halves).view(100, 72)
        c._s2f_version, c._s2f_owner = version, halves[0]
        return c
    for fn in (ops.split_weight, ops.pack_weight):
        first, again = cat(5), cat(5)
        assert first is not again and first.data_ptr() == flat.data_ptr()
        out = fn(first)
        assert len(rec.take()) == 1
        assert fn(again) is out and rec.take() == []
        assert fn(cat(6)) is out                                      # reconverted into the same buffer
        (_, args), = rec.take()
        assert args[0] == flat.data_ptr() and args[1] == out.data_ptr()
    assert ops.resplit_all(CPU) == 2                                   # the owner's storage covers the whole concatenation


def test_non_contiguous_source_registers_no_job(rec):
    w, _ = _weights()
    out = ops.split_weight(w.t())
    pk = ops.pack_weight(w.t())
    calls = rec.take()
    assert [c[0] for c in calls] == [SPLIT, PACK]
    assert calls[0][1][1:] == (out.data_ptr(), 72, 100, 128, 128, 0) and calls[0][1][0] != w.data_ptr()
    assert calls[1][1][1:] == (pk.data_ptr(), 72, 100, 0, 0, 0) and calls[1][1][0] != w.data_ptr()
    assert ops.resplit_all(CPU) == 0 and rec.take() == []
    wc = _weights()[1]
    ops.split_weight_conv3(wc)
    assert ops.resplit_all(CPU) == 1
    assert [c[0] for c in rec.take()] == [SPLIT, "s2f_split_bf16x3_multi"]


def test_new_weight_replaces_the_job_tables(rec):
    w, _ = _weights()
    ops.split_weight(w), ops.pack_weight(w)
    assert ops.resplit_all(CPU) == 2
    old = ops.conversion_state()[:2]
    snaps = [t.clone() for t in old]
    w2, _ = _weights(1)
    ops.split_weight(w2), ops.pack_weight(w2)
    assert ops.resplit_all(CPU, build=False) == -1
    assert ops.conversion_state()[0] is old[0] and ops.conversion_state()[1] is old[1]
    assert ops.resplit_all(CPU) == 4
    new = ops.conversion_state()[:2]
    assert new[0] is not old[0] and new[1] is not old[1] and tuple(new[0].shape) == tuple(new[1].shape) == (2, 8)
    assert new[0].data_ptr() != old[0].data_ptr() and new[1].data_ptr() != old[1].data_ptr()
    assert torch.equal(old[0], snaps[0]) and torch.equal(old[1], snaps[1])          # what a captured graph keeps reading
    assert ops.resplit_all(CPU, build=False) == 4


def test_freed_owner_drops_out(rec):
    w, wc = _weights()
    ops.split_weight(w), ops.pack_weight(w), ops.split_weight_conv3(wc)
    assert ops.resplit_all(CPU) == 3
    del w
    gc.collect()
    assert ops.resplit_all(CPU) == 1
    del wc
    gc.collect()
    assert ops.resplit_all(CPU) == 0


def test_capture_protocol(rec, monkeypatch):
    """ops.begin_step is driven on the CPU as it stands: only torch.cuda.is_current_stream_capturing is replaced."""
    capturing = [True]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    w, wc = _weights()
    outs = _convert_all(w, wc)
    wl = _weights(2)[0]
    loose = ops.split_weight(wl.t())                                   # a non-contiguous source: no job, never trusted
    assert ops.resplit_all(CPU) == 7
    jobs, pack_jobs, _ = ops.conversion_state()
    rec.take()

    # tables built: the captured step records the two multi-launches and then trusts every registered conversion
    ops.begin_step(CPU)
    assert rec.take() == [("s2f_split_bf16x3_multi", (jobs.data_ptr(), 3, 78, 0)), ("s2f_pack_bf16x3_multi", (pack_jobs.data_ptr(), 4, 70, 0))]
    _bump(w, wc)
    for name, fn, *_ in LAYOUTS:
        assert fn(w, wc) is outs[name] and fn(w, wc) is outs[name]
    assert rec.take() == []
    assert ops.split_weight(wl.t()) is loose and rec.take() == []
    _bump(wl)
    assert ops.split_weight(wl.t()) is loose and [c[0] for c in rec.take()] == [SPLIT]          # a jobless entry is never adopted

    # a step that begins outside a capture switches the trust off again, also for a capture that does not begin a step
    ops.begin_step(CPU)
    assert rec.take() == [("s2f_split_bf16x3_multi", (jobs.data_ptr(), 3, 78, 0)), ("s2f_pack_bf16x3_multi", (pack_jobs.data_ptr(), 4, 70, 0))]
    capturing[0] = False
    ops.begin_step(CPU)
    assert rec.take() == []
    capturing[0] = True
    _bump(w)
    assert ops.split_weight(w) is outs["split"]
    (got, args), = rec.take()
    assert got == SPLIT and args[1] == outs["split"].data_ptr()

    # stale tables (a weight the tables do not know): no multi-launch; every cached weight converts by its own launch, into its buffer
    w2 = _weights(3)[0]
    extra = ops.pack_weight(w2)
    rec.take()
    ops.begin_step(CPU)
    assert rec.take() == []
    for name, fn, _which, launch, dims in LAYOUTS:
        assert fn(w, wc) is outs[name]
        (got, args), = rec.take()
        assert got == launch and args[1] == outs[name].data_ptr() and args[2:] == dims + (0,)
    assert ops.pack_weight(w2) is extra and len(rec.take()) == 1
    assert ops.conversion_state()[0] is jobs and ops.conversion_state()[1] is pack_jobs          # (building is not allowed in a capture)
