"""csrc/segmetric.hip on the MI355X: `s2f_seg_hist` against the reference's recorded areas (tests/golden/metric_iou.npz) and against the
op's CPU arithmetic over sizes, class counts, contention patterns and alignments the fixture is too small for; accumulation and bit
repeatability; hipGraph capture of IoUMetric.process; the evaluation loop end to end on the tiny model.  Every test runs under the
conftest's STRICT census: none may leave the kernel for the torch path."""
import dataclasses

import numpy as np
import pytest
import torch

from test_metric import case_maps, want_totals


@pytest.fixture(scope="module")
def g(golden):
    return golden("metric_iou.npz")


def zeros(K, dev="cuda"):
    return torch.zeros(3, K, dtype=torch.int64, device=dev)


def both(pred, label, K, **kw):
    """-> (kernel totals copied to the host, CPU-path totals) of CUDA maps"""
    from spike2former_amd import ops
    got = ops.seg_hist(pred, label, zeros(K), **kw).cpu()
    want = ops.seg_hist(pred.cpu(), label.cpu(), zeros(K, "cpu"), **kw)
    return got, want


# ------------------------------------------------------------------------------------------------------------------ 8. the fixture
@pytest.mark.gpu
def test_kernel_equals_every_recorded_case(g):
    from spike2former_amd import ops
    for name in (str(n) for n in g["cases"]):
        want = want_totals(g, [name])
        float_pred = bool(g[f"{name}.float_pred"])
        for pd in ((torch.float32, torch.int64) if float_pred else (torch.int64,)):
            for ld in (torch.uint8, torch.int64):
                pred, label, K = case_maps(g, name, pd, ld)
                pred, label = pred.cuda(), label.cuda()
                assert torch.equal(ops.seg_hist(pred, label, zeros(K)).cpu(), want), (name, pd, ld)
                assert torch.equal(ops.seg_hist(pred[None], label[None], zeros(K)).cpu(), want), (name, pd, ld)
                # the other layout of the same label: a transposed-stored one made contiguous, a contiguous one read through strides
                if bool(g[f"{name}.transposed"]):
                    other = label.t().contiguous()
                    assert other.shape == pred.shape
                else:
                    other = label.t().contiguous().t()
                    assert other.shape == pred.shape and (not other.is_contiguous() or min(other.shape) == 1)
                assert torch.equal(ops.seg_hist(pred, other, zeros(K)).cpu(), want), (name, pd, ld, "other layout")
                # reduce_zero_label: the raw annotation that LoadAnnotations would have mapped to this label
                lab = label.to(torch.int64)
                alt = (torch.arange(lab.numel(), device="cuda").view(lab.shape) % 2) * 255          # 0 and 255 both mean "ignore"
                raw = torch.where(lab == 255, alt, lab + 1).to(ld)
                assert torch.equal(ops.seg_hist(pred, raw, zeros(K), reduce_zero_label=True).cpu(), want), (name, pd, ld, "raw")


# ------------------------------------------------------------------------------------------------------------------ 9. the sweep
SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 4097), (512, 683), (1024, 2048)]


def pattern(kind, H, W, K, gen):
    """-> (pred int64, label uint8-range int64) on the CPU"""
    if kind == "one_class":          # every pixel the same pair: all 64 lanes of every wave on one bin
        c = min(K - 1, 7)
        return torch.full((H, W), c, dtype=torch.int64), torch.full((H, W), c, dtype=torch.int64)
    if kind == "stripes":            # vertical stripes one pixel wide: neighbouring lanes never share a key
        cols = torch.arange(W)
        pred = (cols % min(K, 37)).expand(H, W).clone()
        label = ((cols * 3 + 1) % min(K, 41)).expand(H, W).clone()
        return pred, label
    pred = torch.randint(0, K + 2, (H, W), generator=gen)
    label = torch.randint(0, min(K + 2, 255), (H, W), generator=gen)
    label[torch.rand(H, W, generator=gen) < 0.1] = 255
    return pred, label


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 19, 150, 2048])
def test_kernel_equals_the_cpu_path_over_sizes_patterns_and_alignments(K):
    from spike2former_amd import ops
    assert ops.SEG_HIST_MAX_CLASSES == 2048
    gen = torch.Generator().manual_seed(1000 + K)
    for H, W in SIZES:
        for kind in ("one_class", "stripes", "noise"):
            pred, label = pattern(kind, H, W, K, gen)
            for ld in (torch.uint8, torch.int64):
                got, want = both(pred.cuda(), label.to(ld).cuda(), K)
                assert torch.equal(got, want), (K, H, W, kind, ld)
                assert int(want[2].sum()) > 0 or kind == "noise"
            if K <= 2:
                got, want = both(pred.float().cuda(), label.to(torch.uint8).cuda(), K)
                assert torch.equal(got, want), (K, H, W, kind, "float32")
    # views that start off a 16-byte boundary: the scalar head and tail of the 16-byte path, and the element-wise label path
    for H, W in ((1, 4097), (37, 53), (512, 683)):
        n = H * W
        pred, label = pattern("noise", 1, n + 8, K, gen)
        pred, label = pred.flatten().cuda(), label.flatten().cuda()
        for po in (0, 1, 3):
            for lo in (0, 1, 2, 3, 4):
                for ld in (torch.uint8, torch.int64):
                    p, l = pred[po:po + n].view(H, W), label.to(ld)[lo:lo + n].view(H, W)
                    got, want = both(p, l, K)
                    assert torch.equal(got, want), (K, H, W, po, lo, ld)
                if K <= 2:
                    p = pred.float()[po:po + n].view(H, W)
                    got, want = both(p, label.to(torch.uint8)[lo:lo + n].view(H, W), K)
                    assert torch.equal(got, want), (K, H, W, po, lo, "float32")


# ------------------------------------------------------------------------------------------------------------------ 10. accumulation
@pytest.mark.gpu
def test_fifty_calls_accumulate_and_repeat_bitwise():
    from spike2former_amd import ops
    K = 150
    gen = torch.Generator().manual_seed(50)
    imgs = []
    for i in range(5):
        pred, label = pattern("noise" if i % 2 else "stripes", 200, 301, K, gen)
        imgs.append((pred.cuda(), label.to(torch.uint8).cuda()))
    singles = [ops.seg_hist(p, l, zeros(K)) for p, l in imgs]
    runs = []
    for _ in range(2):
        t = zeros(K)
        for i in range(50):
            ops.seg_hist(*imgs[i % 5], t)
        runs.append(t.cpu())
    assert torch.equal(runs[0], sum(singles).cpu() * 10)
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------------------------ 11. capture
@pytest.mark.gpu
def test_process_is_capturable_in_a_graph(g):
    import spike2former_amd as s2f
    from test_metric import _samples
    names = ["k150_blocky", "k150_noise"]
    samples = _samples(g, names, as_dict=False)
    for d in samples:
        d.pred_sem_seg.data = d.pred_sem_seg.data.cuda()
        d.gt_sem_seg.data = d.gt_sem_seg.data.cuda()
    m = s2f.IoUMetric()
    m.dataset_meta = dict(classes=[str(i) for i in range(150)])
    m.process({}, samples)                     # eager: creates the accumulator, so nothing is allocated under capture
    eager = m._totals.cpu()
    assert torch.equal(eager, want_totals(g, names))
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):              # one stream, no parallel branches
        m.process({}, samples)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m._totals.cpu(), 3 * eager)


# ------------------------------------------------------------------------------------------------------------------ 12. end to end
def _tiny(H=66, W=98):
    import spike2former_amd as s2f
    from oracle import s2f_oracle as so
    cfg = dataclasses.replace(so.CONFIGS["C1_64"], H=H, W=W, B=1)
    st = so.make_params(cfg)
    model = s2f.MODELS.build(s2f.model_cfg("C1_64"))
    model.load_state_dict({k: v.detach() for k, v in st.items()}, strict=True)
    return s2f, cfg, model.cuda()


def _label(gen, H, W, K):
    lab = torch.randint(0, K, (H // 8 + 1, W // 8 + 1), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W]
    lab[:3] = 255
    return lab.to(torch.uint8)[None].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("tta", [False, True])
def test_evaluate_end_to_end_on_the_tiny_model(tta):
    s2f, cfg, model = _tiny()
    from spike2former_amd import ops
    from spike2former_amd.data_preprocessor import SegDataSample
    K, ori = cfg.num_classes, (61, 90)
    gen = torch.Generator().manual_seed(77)
    batches = []
    for i in range(4):
        img = torch.randn(3, cfg.H, cfg.W, generator=gen)
        meta = dict(img_shape=(cfg.H, cfg.W), ori_shape=ori, pad_shape=(cfg.H, cfg.W), padding_size=[0, 5, 0, 3], img_path=f"img{i}.png")
        first = SegDataSample(gt_sem_seg=_label(gen, *ori, K), metainfo=dict(meta, flip=False))
        if tta:
            second = SegDataSample(metainfo=dict(meta, flip=True, flip_direction="horizontal"))
            batches.append(dict(inputs=[[img], [img.flip(-1)]], data_samples=[[first], [second]]))
        else:
            batches.append(dict(inputs=[img], data_samples=[first]))
    seen = []

    class Recording(s2f.IoUMetric):
        def process(self, data_batch, data_samples):
            super().process(data_batch, data_samples)
            seen.extend((d.pred_sem_seg.data.cpu(), d.gt_sem_seg.data.cpu()) for d in data_samples)          # the test's copies

    metric = Recording(iou_metrics=["mIoU", "mDice", "mFscore"])
    metric.dataset_meta = dict(classes=[str(i) for i in range(K)])
    runner = s2f.MODELS.build(dict(type="SegTTAModel", module=model)) if tta else model
    before = dict(ops.FALLBACKS)
    got = s2f.evaluate(runner, batches, metric)
    assert dict(ops.FALLBACKS) == before
    assert len(seen) == 4 and all(p.shape == (1, *ori) and p.dtype == torch.int64 and p.device.type == "cpu" for p, _ in seen)
    totals = torch.zeros(3, K, dtype=torch.int64)
    for p, l in seen:
        ops.seg_hist(p, l, totals)
    assert int(totals[2].sum()) == sum(int((l != 255).sum()) for _, l in seen) > 0
    want = metric.compute_metrics(totals)
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
    assert not bool(metric._totals.any())
