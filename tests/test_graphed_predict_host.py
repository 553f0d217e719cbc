"""CPU: the host side of captured inference -- graph.CapturePolicy with a fake capture (when a key is captured, the LRU, the bounded
sighting table, the key of GraphedPredict), test_cfg['graph'] on inputs that cannot be replayed, the slide-mode precondition, and
the argument checks of s2f_seg_label (no launch is reached)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


class Fake:
    """the three injected functions, recording what they were asked"""

    def __init__(self):
        self.log = []

    def eager(self, x):
        self.log.append(("eager", x))
        return ("eager", x)

    def capture(self, key, x):
        self.log.append(("capture", key, x))
        return {"key": key}, ("warm", x)

    def replay(self, entry, x):
        self.log.append(("replay", entry["key"], x))
        return ("replay", entry["key"], x)


def policy(**kw):
    from spike2former_amd.graph import CapturePolicy
    f = Fake()
    return CapturePolicy(f.eager, f.capture, f.replay, **kw), f


@pytest.mark.parametrize("after", [1, 2, 3])
def test_a_key_is_captured_at_exactly_sighting_capture_after(after):
    p, f = policy(capture_after=after)
    got = [p("a", i)[0] for i in range(after + 2)]
    assert got == ["eager"] * (after - 1) + ["warm", "replay", "replay"]
    assert [e[0] for e in f.log] == ["eager"] * (after - 1) + ["capture", "replay", "replay"]
    assert p.census == dict(captures=1, replays=2, evictions=0, eager=({"sightings": after - 1} if after > 1 else {}))
    # another key counts on its own
    assert p("b", 0)[0] == ("eager" if after > 1 else "warm")
    assert "a" not in p.sightings                      # a captured key leaves the sighting table


def test_lru_order_and_eviction_at_max_graphs():
    p, f = policy(max_graphs=2, capture_after=1)
    p("a", 0), p("b", 0)
    assert list(p.graphs) == ["a", "b"] and p.census["evictions"] == 0
    p("a", 1)                                          # a replay makes `a` the most recently used
    assert list(p.graphs) == ["b", "a"]
    p("c", 0)                                          # ... so the third key drops `b`
    assert list(p.graphs) == ["a", "c"] and p.census["evictions"] == 1
    assert p("b", 1)[0] == "warm"                      # `b` is captured again (and drops `a`)
    assert list(p.graphs) == ["c", "b"]
    assert p.census == dict(captures=4, replays=1, evictions=2, eager={})
    assert len(p.graphs) <= 2


def test_the_eviction_precedes_the_capture():
    """the dropped graph's pool is free before the new capture allocates"""
    from spike2former_amd.graph import CapturePolicy
    live = []
    p = CapturePolicy(lambda x: x, lambda key, x: (live.append(len(p.graphs)) or {"key": key}, x), lambda e, x: x, max_graphs=1,
                      capture_after=1)
    p("a", 0), p("b", 0)
    assert live == [0, 0]


def test_the_sighting_table_is_bounded():
    p, f = policy(capture_after=3, max_sightings=4)
    for i in range(50):
        p(("shape", i), i)
    assert len(p.sightings) == 4 and list(p.sightings) == [("shape", i) for i in range(46, 50)]
    assert p.census["captures"] == 0 and p.census["eager"] == {"sightings": 50} and not p.graphs
    # a key that keeps coming back is not the one forgotten
    p, f = policy(capture_after=3, max_sightings=2)
    p("hot", 0)
    for i in range(5):
        p(("cold", i), 0)
        if i == 0:
            p("hot", 1)
    assert p("hot", 2)[0] == "eager"                   # ("hot" fell out behind four colder keys: its count starts again)
    p, f = policy(capture_after=3, max_sightings=2)
    p("hot", 0), p("cold", 0), p("hot", 1), p("colder", 0)
    assert p("hot", 2)[0] == "warm"                    # seen again in time: "cold" was the oldest entry, not "hot"


def test_bad_policy_arguments():
    from spike2former_amd.graph import CapturePolicy
    for kw in (dict(max_graphs=0), dict(capture_after=0), dict(max_sightings=0)):
        with pytest.raises(ValueError):
            CapturePolicy(None, None, None, **kw)


def _stub_segmentor(test_cfg, K=5, calls=None):
    """slide_ref.segmentor, with the stand-in network behind `_encode_decode`: the class's own encode_decode (the routing under test)
    stays in place"""
    import slide_ref as R
    from spike2former_amd.segmentor import EncoderDecoder
    m = object.__new__(EncoderDecoder)
    torch.nn.Module.__init__(m)
    m.test_cfg, m.out_channels, m.align_corners = dict(test_cfg), K, False
    m.decode_head = types.SimpleNamespace(threshold=0.3)

    def plain(x, metas):
        if calls is not None:
            calls.append(tuple(x.shape))
        return R.lin_net(x, K)
    m._encode_decode = plain
    return m.eval()


def test_a_changed_launch_snapshot_or_route_switch_is_a_new_key():
    from spike2former_amd import fused, maskformer_head, ops
    from spike2former_amd.graph import GraphedPredict
    gp = GraphedPredict(_stub_segmentor({}))
    x, metas = torch.zeros(2, 3, 8, 12), [dict(img_shape=(8, 12))]
    k0 = gp.key(x, metas)
    assert k0 == gp.key(x.clone(), [dict(img_shape=torch.Size((8, 12)))]) and hash(k0) is not None
    assert gp.key(x[:1], metas) != k0 and gp.key(x, [dict(img_shape=(8, 11))]) != k0
    before = ops.cfg.DECODER_SIBLINGS
    ops.cfg.DECODER_SIBLINGS = not before
    try:
        assert gp.key(x, metas) != k0
    finally:
        ops.cfg.DECODER_SIBLINGS = before
    for mod, name in ((fused, "EVAL_FUSION"), (maskformer_head, "PREDICT_LAST_ONLY")):
        was = getattr(mod, name)
        setattr(mod, name, not was)
        try:
            assert gp.key(x, metas) != k0, name
        finally:
            setattr(mod, name, was)
    assert gp.key(x, metas) == k0


@pytest.mark.parametrize("opt", [True, dict(max_graphs=2, capture_after=1)])
def test_graph_option_on_cpu_tensors_is_the_eager_result_with_a_census_reason(opt):
    import slide_ref as R
    x = torch.randn(2, 3, 9, 13, generator=torch.Generator().manual_seed(2))
    m = _stub_segmentor(dict(mode="whole", graph=opt))
    with torch.no_grad():
        got = [m.inference(x, [dict(img_shape=(9, 13))]) for _ in range(3)]
        logits = m(x, mode="logits")
    for g in got + [logits]:
        assert torch.equal(g, R.lin_net(x, 5))
    gp = m.graphed_predict()
    assert gp.census == dict(captures=0, replays=0, evictions=0, eager={"not_cuda": 4})
    assert gp.policy.max_graphs == (2 if isinstance(opt, dict) else 8)
    assert _stub_segmentor(dict(mode="whole")).graphed_predict() is None
    # slide mode with window_batch on CPU tensors: the reference loop, every window through the eager route
    cfg = dict(mode="slide", crop_size=(6, 8), stride=(4, 5), window_batch=2)
    with torch.no_grad():
        a = _stub_segmentor(dict(cfg, graph=opt)).inference(x, [dict(img_shape=(9, 13)) for _ in range(2)])
        b = _stub_segmentor(cfg).inference(x, [dict(img_shape=(9, 13)) for _ in range(2)])
    assert torch.equal(a, b)


def test_a_copied_segmentor_builds_its_own_graphs():
    import copy
    m = _stub_segmentor(dict(mode="whole", graph=True))
    gp = m.graphed_predict()
    assert m.graphed_predict() is gp
    twin = copy.deepcopy(m)
    assert twin.graphed_predict() is not gp and twin.graphed_predict().model is twin


def test_slide_without_window_batch_raises_before_any_window_runs():
    calls = []
    x = torch.zeros(1, 3, 9, 13)
    m = _stub_segmentor(dict(mode="slide", crop_size=(6, 8), stride=(4, 5), graph=True), calls=calls)
    with pytest.raises(ValueError, match="window_batch"):
        m.inference(x, [dict(img_shape=(9, 13))])
    assert calls == []
    m = _stub_segmentor(dict(mode="slide", crop_size=(6, 8), stride=(4, 5)), calls=calls)          # without the option: as before
    m.inference(x, [dict(img_shape=(9, 13))])
    assert len(calls) == 4


def test_seg_label_argument_errors_are_reported_without_a_gpu():
    from spike2former_amd._lib import lib
    P = 1 << 20          # an aligned dummy address: never dereferenced on the host
    ok = dict(x=P, label=P, label_f=None, K=3, ps=64, ld=8, r0=0, c0=0, h=8, w=8, H=5, W=7, flags=0, thr=0.3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s2f_seg_label(a["x"], a["label"], a["label_f"], a["K"], a["ps"], a["ld"], a["r0"], a["c0"], a["h"], a["w"], a["H"],
                                 a["W"], a["flags"], a["thr"], None)
    for kw, word in ((dict(x=None), b"null"), (dict(label=None), b"null"), (dict(K=0), b"bad shape"), (dict(K=-2), b"bad shape"),
                     (dict(H=0), b"bad shape"), (dict(W=0), b"bad shape"), (dict(W=-3), b"bad shape"), (dict(H=65536), b"bad shape"),
                     (dict(h=0), b"window"), (dict(w=-1), b"window"), (dict(h=9), b"window"), (dict(r0=1), b"window"),
                     (dict(c0=1), b"window"), (dict(ps=63), b"window"), (dict(r0=-1), b"window"),
                     (dict(label_f=P), b"exactly one output"), (dict(label=None, label_f=P), b"exactly one output"),
                     (dict(flags=2), b"unknown flags"), (dict(flags=16), b"unknown flags")):
        assert call(**kw) == -1, kw
        assert word in lib.s2f_last_error(), (kw, lib.s2f_last_error())
