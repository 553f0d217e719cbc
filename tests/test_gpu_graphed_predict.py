"""GPU: captured inference (graph.GraphedPredict, test_cfg['graph']) against the eager route of the same model with the option absent
-- which this feature does not touch.  A replay launches the kernels the eager pass launches, on the same inputs, so every comparison
is bit equality.  The tiny models: C1_64 (64 x 64, T = 2, K = 20) and C5_tiny (64 x 96, the SDT-v3 backbone), seeded, eval."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def metas(B, H, W):
    return [dict(img_shape=(H, W), ori_shape=(H, W), pad_shape=(H, W), padding_size=[0, 0, 0, 0]) for _ in range(B)]


def picture(seed, B, H, W):
    """16 x a standard normal picture: at unit amplitude the seeded tiny models' backbone features stay below the decode head's
    firing thresholds in eval mode and the logits do not depend on the picture at all (measured: max |difference| 0 between two
    pictures, 2e-3 at this amplitude) -- a replay that read a stale input would pass unnoticed.  The tests assert the dependence
    where they rely on it."""
    return (16.0 * torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))).cuda()


def configure(model, **test_cfg):
    """the model with this test_cfg and no GraphedPredict of an earlier test"""
    model.test_cfg = dict(test_cfg)
    model.__dict__.pop("_graphed_predict", None)
    return model


def eager(model, x):
    """the reference: the option absent, membranes reset, every launch from Python"""
    import spike2former_amd as s2f
    cfg, gp = model.test_cfg, model.__dict__.pop("_graphed_predict", None)
    model.test_cfg = {k: v for k, v in (cfg or {}).items() if k != "graph"}
    try:
        with torch.no_grad():
            s2f.reset_net(model)
            return model(x, mode="logits").clone()
    finally:
        model.test_cfg = cfg
        if gp is not None:
            model.__dict__["_graphed_predict"] = gp


def membranes_reset(model):
    return all(isinstance(m.v, float) and m.v == 0.0 for m in model.modules() if hasattr(m, "keep_membrane"))


@pytest.fixture(scope="module")
def models():
    import spike2former_amd as s2f
    from spike2former_amd.init_utils import seeded_init
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = seeded_init(s2f.MODELS.build(s2f.model_cfg(name))).cuda().eval()
        return configure(cache[name])
    return get


@pytest.mark.parametrize("after", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["C1_64", "C5_tiny"])
def test_replay_equals_eager_bit_for_bit(models, name, B, after):
    import spike2former_amd as s2f
    model, w = models(name), s2f.WORKLOADS[name]
    H, W = w["H"], w["W"]
    xs = [picture(100 + i, B, H, W) for i in range(3)]
    want = [eager(model, x) for x in xs]
    assert torch.equal(eager(model, xs[0]), want[0]), "two eager passes on one input differ: the precondition of this test"
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])          # a replay on a stale input would show
    flags = [m.keep_membrane for m in model.modules() if hasattr(m, "keep_membrane")]
    configure(model, mode="whole", graph=dict(capture_after=after))
    with torch.no_grad():
        for x, ref in zip(xs, want):
            got = model(x, mode="logits")
            assert got.shape == (B, w["K"], H, W) and torch.equal(got, ref), (got - ref).abs().max().item()
            assert membranes_reset(model)
    census = model.graphed_predict().census
    assert census == dict(captures=1, replays=3 - after, evictions=0, eager=({"sightings": after - 1} if after > 1 else {}))
    assert [m.keep_membrane for m in model.modules() if hasattr(m, "keep_membrane")] == flags          # put back after the capture
    log = model.graphed_predict().capture_log
    assert len(log) == 1 and log[0]["key"] == ((B, 3, H, W), (H, W)) and log[0]["seconds"] > 0


@pytest.mark.parametrize("name", ["C1_64", "C5_tiny"])
def test_replays_follow_the_live_weights(models, name):
    """after the capture: every parameter perturbed in place, one BatchNorm's statistics and affine changed (then all of them: what
    the eval routes fold from a BatchNorm is folded inside the graph), a differently seeded state loaded -- the replay equals a fresh
    eager pass each time, and nothing is captured again"""
    import spike2former_amd as s2f
    model, w = copy.deepcopy(models(name)), s2f.WORKLOADS[name]
    x, m = picture(7, 2, w["H"], w["W"]), metas(2, w["H"], w["W"])
    gp = s2f.GraphedPredict(model, capture_after=1)
    other = copy.deepcopy(model)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for t in other.state_dict().values():
            if t.is_floating_point():
                t.mul_(1.0 + 0.05 * torch.randn(t.shape, generator=g).cuda())
    bns = [b for b in model.modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]

    def change_bn(b):
        b.running_mean.add_(0.05), b.running_var.mul_(1.3), b.weight.mul_(0.8), b.bias.add_(0.1)

    def perturb():
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.01 * p.abs().mean() * torch.randn(p.shape, generator=g).cuda())
    steps = [("capture", lambda: None), ("perturbed", perturb), ("one_bn", lambda: change_bn(bns[len(bns) // 2])),
             ("every_bn", lambda: [change_bn(b) for b in bns]), ("load_state_dict", lambda: model.load_state_dict(other.state_dict()))]
    seen = []
    with torch.no_grad():
        for what, change in steps:
            change()
            got = gp(x, [dict(d) for d in m]).clone()
            ref = eager(model, x)
            assert torch.equal(got, ref), (what, (got - ref).abs().max().item())
            seen.append(ref)
    # the changes were ones the logits show (a single BatchNorm in the middle of a quantised network need not be: its neurons may
    # fire the same spikes)
    for (what, _), a, b in zip(steps[1:], seen, seen[1:]):
        assert what == "one_bn" or not torch.equal(a, b), what
    assert gp.census == dict(captures=1, replays=len(steps) - 1, evictions=0, eager={})


def test_graphed_validation_beside_a_training_graph():
    import spike2former_amd as s2f
    from spike2former_amd import ops
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedStep
    from spike2former_amd.init_utils import seeded_init
    from spike2former_amd.train import FlatAdamW
    w = s2f.WORKLOADS["C1_64"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    img, val = picture(7, 2, w["H"], w["W"]), picture(8, 2, w["H"], w["W"])
    red = FlatGradAllReduce(model.parameters(), 1)
    red.install_sinks()
    s2f.reset_net(model); red.zero()
    s2f.headline_loss(*model(img)).backward()
    ops.wgrad_join(); red.gather(); red.compact()
    opt = FlatAdamW(model, red, lr=0.01, weight_decay=0.005, clip_grad=dict(max_norm=1e9))
    gs = GraphedStep(model, s2f.headline_loss, img, grad_buffer=red, warmup=1, optimizer=opt)
    gp = s2f.GraphedPredict(model, capture_after=1)
    settings = ops.cfg.launch_snapshot()
    results = []
    for _ in range(2):
        gs(), gs()
        model.eval()
        with torch.no_grad():
            got = gp(val, metas(2, w["H"], w["W"])).clone()
        ref = eager(model, val)
        model.train()
        assert torch.equal(got, ref), (got - ref).abs().max().item()
        results.append(ref)
    assert float(gs()) == float(gs.static_loss) and np.isfinite(float(gs.static_loss))          # the training graph still replays
    assert not torch.equal(results[0], results[1])                                              # (the weights did move)
    assert gp.census == dict(captures=1, replays=1, evictions=0, eager={})
    assert ops.cfg.launch_snapshot() == settings and ops.RESPLIT_IN_GRAPH is True
    assert all(m.keep_membrane is False for m in model.modules() if hasattr(m, "keep_membrane"))
    red.close()


def test_cache_evicts_the_least_recently_used_and_captures_again(models):
    model = models("C1_64")
    shapes = {"a": (64, 64), "b": (66, 98), "c": (50, 74)}
    xs = {k: [picture(20 + 3 * i + j, 1, *hw) for j in range(3)] for i, (k, hw) in enumerate(shapes.items())}
    want = {k: [eager(model, x) for x in v] for k, v in xs.items()}
    configure(model, mode="whole", graph=dict(max_graphs=2, capture_after=1))
    # a b a c (drops b) b (captured again, drops a) c
    order = [("a", 0), ("b", 0), ("a", 1), ("c", 0), ("b", 1), ("c", 1), ("b", 2)]
    with torch.no_grad():
        for k, j in order:
            got = model(xs[k][j], mode="logits")
            assert torch.equal(got, want[k][j]), (k, j)
    gp = model.graphed_predict()
    assert gp.census == dict(captures=4, replays=3, evictions=2, eager={})
    assert [key[0][2:] for key in gp.policy.graphs] == [shapes["c"], shapes["b"]]


def test_results_handed_to_the_caller_do_not_alias_a_static_buffer(models):
    model = configure(models("C1_64"), mode="whole", graph=dict(capture_after=1))
    x = [picture(40 + i, 1, 64, 64) for i in range(3)]
    with torch.no_grad():
        model(x[0], mode="logits")                                         # the capture
        a = model(x[1], mode="logits")
        kept = a.clone()
        b = model(x[2], mode="logits")
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, kept) and not torch.equal(a, b)
        ra = model(x[1], mode="predict")
        kept_logits, kept_pred = ra[0].seg_logits.data.clone(), ra[0].pred_sem_seg.data.clone()
        rb = model(x[2], mode="predict")
        assert torch.equal(ra[0].seg_logits.data, kept_logits) and torch.equal(ra[0].pred_sem_seg.data, kept_pred)
        assert torch.equal(kept_logits, kept[0]) and torch.equal(rb[0].seg_logits.data, b[0])
    assert model.graphed_predict().census["replays"] == 4


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("group", [2, 4])
def test_slide_inference_graph_on_equals_graph_off(models, group, B):
    """96 x 160, crop 64, stride 48: 2 x 3 windows; groups of 2, 2, 2 or of 4 and 2 (a second key)"""
    model = models("C1_64")
    cfg = dict(mode="slide", crop_size=(64, 64), stride=(48, 48), window_batch=group)
    xs = [picture(60 + i, B, 96, 160) for i in range(2)]
    configure(model, **cfg)
    want = [eager(model, x) for x in xs]
    configure(model, **cfg, graph=dict(capture_after=1))
    with torch.no_grad():
        for x, ref in zip(xs, want):
            got = model.inference(x, metas(B, 96, 160))
            assert got.shape == ref.shape and torch.equal(got, ref)
    census = model.graphed_predict().census
    assert census == dict(captures=1 if group == 2 else 2, replays=5 if group == 2 else 2, evictions=0, eager={})


def test_tta_merged_prediction_is_equal(models):
    import spike2former_amd as s2f
    import view_ref as VR
    from test_gpu_test_views import make
    model = models("C1_64")
    img, seg = VR.scene(66, 98, seed=6, n_classes=6)
    aug = make(scale_factors=(1.0, 0.75), flips=(False, True), reduce_zero_label=True)
    tta = s2f.MODELS.build(dict(type="SegTTAModel", module=model))
    preds = []
    for cfg in (dict(mode="whole"), dict(mode="whole", graph=dict(capture_after=1))):
        configure(model, **cfg)
        out = tta.test_step(aug([img], [seg], ["img0.png"]))
        preds.append(out[0].pred_sem_seg.data.clone())
    assert preds[0].shape == (1, 66, 98) and torch.equal(preds[0], preds[1])
    assert model.graphed_predict().census == dict(captures=2, replays=2, evictions=0, eager={})          # two sizes, each flipped too


def test_evaluate_totals_are_equal(models):
    import spike2former_amd as s2f
    import view_ref as VR
    from test_gpu_test_views import make
    model = models("C1_64")
    K = s2f.WORKLOADS["C1_64"]["K"]
    pictures = [VR.scene(h, w, seed=30 + i, n_classes=6) + (f"{i}.png",) for i, (h, w) in enumerate([(66, 98), (50, 74)] * 2)]
    aug = make(reduce_zero_label=True)
    runs = []
    for cfg in (dict(mode="whole"), dict(mode="whole", graph=True)):
        configure(model, **cfg)
        metric = s2f.metrics.IoUMetric(label_reduce_zero=aug.reduce_zero_label)
        metric.dataset_meta = dict(classes=[str(i) for i in range(K)])
        seen, compute = {}, metric.compute_metrics

        def keep(totals, seen=seen, compute=compute):
            seen["totals"] = np.asarray(totals).copy()
            return compute(totals)
        metric.compute_metrics = keep
        result = s2f.metrics.evaluate(model, (aug([img], [seg], [path]) for img, seg, path in pictures), metric)
        runs.append((seen["totals"], dict(result)))
    assert runs[0][0].dtype == np.int64 and runs[0][0].sum() > 0 and np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    for k, v in runs[0][1].items():
        assert np.array_equal(np.asarray(v), np.asarray(runs[1][1][k]), equal_nan=True), k
    assert model.graphed_predict().census == dict(captures=2, replays=0, evictions=0, eager={"sightings": 2})


def test_a_model_under_a_firing_recorder_runs_the_eager_route(models):
    import spike2former_amd as s2f
    model = models("C1_64")
    x = picture(70, 1, 64, 64)
    runs = []
    for cfg in (dict(mode="whole"), dict(mode="whole", graph=dict(capture_after=1))):
        configure(model, **cfg)
        s2f.reset_net(model)
        with torch.no_grad(), s2f.FiringRecorder(model) as rec:
            out = model(x, mode="logits").clone()
            rec.collect()
        runs.append((out, rec.result()))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and len(runs[0][1]["t0"]) > 0
    assert model.graphed_predict().census == dict(captures=0, replays=0, evictions=0, eager={"firing_stats": 1})
    hook = next(m for m in model.modules() if hasattr(m, "keep_membrane")).register_forward_hook(lambda *a: None)
    try:
        with torch.no_grad():
            s2f.reset_net(model)
            model(x, mode="logits")
    finally:
        hook.remove()
    assert model.graphed_predict().census["eager"] == {"firing_stats": 1, "forward_hooks": 1}
