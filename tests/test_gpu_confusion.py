"""csrc/segmetric.hip on the MI355X: `s2f_seg_confusion`, both routes (the per-workgroup LDS table and the global atomics), against
the numpy restatement of tests/test_confusion.py (`ref_confusion`: the participation rule, then the reference's
tools/analysis_tools/confusion_matrix.py:46-65 bincount) at the edges of the shared front end -- scalar head and tail, the wave
peeling, the dtypes and layouts, the class counts around the LDS budget, the grid-stride loop -- and against `s2f_seg_hist`, whose
three rows are the table's diagonal and marginals; capture in a graph; the evaluation loop with both metrics on the tiny model.
Every comparison is exact (torch.equal); every test runs under the conftest's STRICT census."""
import numpy as np
import pytest
import torch

from test_confusion import ref_confusion

ROUTES = [None, "global"]
PEEL_MAX_ROUNDS = 4          # csrc/segmetric.hip SEG_PEEL_MAX_ROUNDS


def check(pred, label, K, route, **kw):
    """the kernel's matrix of CUDA maps == the numpy reference of the same maps"""
    from spike2former_amd import ops
    got = ops.seg_confusion(pred, label, torch.zeros(K, K, dtype=torch.int64, device="cuda"), route=route, **kw).cpu()
    want = torch.from_numpy(ref_confusion(pred, label, K, kw.get("ignore_index", 255), kw.get("reduce_zero_label", False)))
    assert torch.equal(got, want), (K, route, tuple(pred.shape), kw, int((got - want).abs().sum()))
    return got


def noise(seed, H, W, K, bad=True):
    """-> CPU (pred int64, label uint8): uniform noise over the classes, 10 % ignored; bad: also labels / predictions outside them"""
    gen = torch.Generator().manual_seed(seed)
    pred = torch.randint(-1 if bad else 0, K + 1 if bad else K, (H, W), generator=gen)
    label = torch.randint(0, min(K + 2 if bad else K, 255), (H, W), generator=gen)
    label[torch.rand(H, W, generator=gen) < 0.1] = 255
    return pred, label.to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ head and tail
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_scalar_head_and_tail(route):
    K = 5
    for i, (H, W) in enumerate([(1, 1), (1, 3), (1, 4), (1, 7), (1, 9), (3, 3)]):
        pred, label = noise(20 + i, H, W, K)
        got = check(pred.cuda(), label.cuda(), K, route)
        assert int(got.sum()) <= H * W
    # a prediction view 1, 2, 3 elements past a 16-byte boundary: 1 - 3 (fp32) or 1 (int64) head pixels, and every tail length
    big_p, big_l = noise(30, 1, 64, K, bad=False)
    big_p, big_l = big_p.flatten().cuda(), big_l.flatten().cuda()
    assert big_p.data_ptr() % 16 == 0 and big_l.data_ptr() % 16 == 0
    for off in (1, 2, 3):
        for n in (1, 2, 5, 17, 18, 19, 20, 21):
            for p in (big_p, big_p.float()):
                for lab in (big_l, big_l.to(torch.int64)):
                    check(p[off:off + n].view(1, n), lab[off:off + n].view(1, n), K, route)
                    check(p[off:off + n].view(1, n), lab[:n].view(1, n), K, route)           # the label aligned, the prediction not


# ------------------------------------------------------------------------------------------------------------------ peeling
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_wave_peeling_patterns(route):
    K, H, W = 19, 64, 64
    rows, cols = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    # one pair everywhere: every lane uniform with weight 4, one round retires the wave
    got = check(torch.full((H, W), 3).cuda(), torch.full((H, W), 7, dtype=torch.uint8).cuda(), K, route)
    assert int(got[7, 3]) == H * W and int(got.sum()) == H * W
    # a checkerboard of two pairs with period 1: no lane is uniform
    odd = (rows + cols) % 2
    check((odd * 5 + 1).cuda(), (odd * 2 + 4).to(torch.uint8).cuda(), K, route)
    # vertical stripes of width 4 (every lane uniform, 16 pairs per row) and of width 6 (every third lane on a boundary)
    for width in (4, 6):
        stripe = cols // width
        check((stripe % K).contiguous().cuda(), ((stripe * 3 + 1) % K).to(torch.uint8).cuda(), K, route)
    # more than SEG_PEEL_MAX_ROUNDS + 1 distinct pairs inside every wave: groups of 4 pixels cycling through 8 pairs, so each of
    # the 64 lanes of a wave is uniform and holds one of 8 keys, 8 lanes each -- the peeling gives up and the rest add themselves
    grp = (torch.arange(H * W) // 4) % 8
    assert grp[:256].unique().numel() == 8 > PEEL_MAX_ROUNDS + 1
    got = check((grp + 2).view(H, W).cuda(), (grp * 2).to(torch.uint8).view(H, W).cuda(), K, route)
    assert int((got != 0).sum()) == 8 and int(got[0, 2]) == H * W // 8
    # ... and 7 pairs on 32, 16, 8, 4, 2, 1, 1 lanes of every wave: two full rounds, a third that ends the peeling, 8 lanes left over
    lanes = torch.tensor([0] * 32 + [1] * 16 + [2] * 8 + [3] * 4 + [4] * 2 + [5, 6])
    grp = lanes.repeat(H * W // 256).repeat_interleave(4)
    got = check((grp + 2).view(H, W).cuda(), (grp * 2).to(torch.uint8).view(H, W).cuda(), K, route)
    assert int(got[0, 2]) == H * W // 2 and int(got[12, 8]) == H * W // 64


# ------------------------------------------------------------------------------------------------------------------ types and layout
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_types_layouts_ignore_index_and_invalid_predictions(route):
    K, H, W = 7, 37, 53
    pred, label = noise(40, H, W, K)
    assert int((pred == -1).sum()) and int((pred == K).sum()) and int((label == 255).sum()) and int((label == K).sum())
    fpred = pred.float()
    gen = torch.Generator().manual_seed(41)
    fpred[torch.rand(H, W, generator=gen) < 0.05] = 2.5
    fpred[torch.rand(H, W, generator=gen) < 0.05] = float("nan")
    for p in (pred.cuda(), fpred.cuda()):
        for ld in (torch.uint8, torch.int64):
            lab = label.to(ld).cuda()
            base = check(p, lab, K, route)
            check(p[None], lab[None], K, route)
            # the label stored transposed ([W, H]): read in place, the same matrix
            lt = lab.t().contiguous()
            assert lt.shape == (W, H) and torch.equal(check(p, lt, K, route), base)
            # ... and a contiguous-shaped label read through strides
            assert torch.equal(check(p, lt.t(), K, route), base)
            check(p, lab, K, route, ignore_index=3)
            check(p, lab, K, route, reduce_zero_label=True)
            check(p, lab, K, route, ignore_index=3, reduce_zero_label=True)
    # int64 labels outside uint8's range, negative ones included
    wide = label.to(torch.int64)
    wide[0, :5] = torch.tensor([-1, -255, 256, 2 ** 40, 255])
    check(pred.cuda(), wide.cuda(), K, route)
    check(pred.cuda(), wide.cuda(), K, route, ignore_index=-1)


# ------------------------------------------------------------------------------------------------------------------ K
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 19, 150, 171])
@pytest.mark.parametrize("route", ROUTES)
def test_class_counts(K, route):
    pred, label = noise(50 + K, 61, 67, K)
    check(pred.cuda(), label.cuda(), K, route)
    check(pred.cuda(), label.to(torch.int64).cuda(), K, route)
    # the last class in the last row and column of the table
    last = check(torch.full((8, 8), K - 1).cuda(), torch.full((8, 8), K - 1, dtype=torch.uint8).cuda(), K, route)
    assert int(last[K - 1, K - 1]) == 64


@pytest.mark.gpu
def test_the_last_k_of_the_lds_route_and_the_first_of_the_global_one():
    from spike2former_amd import ops
    k_lds = int((ops.SEG_CONF_LDS_BYTES // 4) ** 0.5)
    assert 4 * k_lds * k_lds <= ops.SEG_CONF_LDS_BYTES < 4 * (k_lds + 1) ** 2 and k_lds == 181
    for K in (k_lds, k_lds + 1):
        pred, label = noise(60 + K, 97, 131, K)
        pred, label = pred.cuda(), label.cuda()
        auto = check(pred, label, K, None)
        assert torch.equal(auto, check(pred, label, K, "global"))
        # every bin of the table is reachable: the pairs (c, K - 1 - c) and the corners
        c = torch.arange(K).repeat_interleave(4)[None]
        check((K - 1 - c).cuda(), c.to(torch.uint8).cuda(), K, None)


@pytest.mark.gpu
def test_k_2048_on_the_global_route():
    K = 2048
    gen = torch.Generator().manual_seed(70)
    pred = torch.randint(-1, K + 1, (32, 32), generator=gen)
    label = torch.randint(-1, K + 1, (32, 32), generator=gen)
    label[0, :4] = 255
    pred[1, :2], label[1, :2] = K - 1, K - 1
    for route in ROUTES:          # the automatic choice at this K is the global route too
        got = check(pred.cuda(), label.cuda(), K, route)
        assert int(got[K - 1, K - 1]) >= 2


# ------------------------------------------------------------------------------------------------------------------ grid-stride
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_the_grid_stride_loop_and_a_second_call_add(route):
    """600 x 900 = 135 000 groups of 4 pixels: more than the global route's 512 workgroups of 256 lanes cover in one pass, and 33
    workgroup-passes of 1024 lanes x 4 trips on the LDS route: every workgroup's loop runs more than once"""
    from spike2former_amd import ops
    K, H, W = 19, 600, 900
    gen = torch.Generator().manual_seed(80)
    blocks = torch.randint(0, K, (H // 20, W // 20), generator=gen).repeat_interleave(20, 0).repeat_interleave(20, 1)
    pred = torch.where(torch.rand(H, W, generator=gen) < 0.2, torch.randint(0, K, (H, W), generator=gen), blocks)
    label = blocks.to(torch.uint8)
    label[torch.rand(H, W, generator=gen) < 0.05] = 255
    pred, label = pred.cuda(), label.cuda()
    first = check(pred, label, K, route)
    acc = first.cuda()
    pred2, label2 = noise(81, H, W, K)
    ops.seg_confusion(pred2.cuda(), label2.cuda(), acc, route=route)
    assert torch.equal(acc.cpu(), first + torch.from_numpy(ref_confusion(pred2, label2, K)))


# ------------------------------------------------------------------------------------------------------------------ the existing kernel
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_consistency_with_seg_hist(route):
    from spike2former_amd import ops
    K = 150
    pred, label = noise(90, 97, 131, K, bad=False)          # every prediction and every non-ignored label is a class
    pred, label = pred.cuda(), label.cuda()
    m = check(pred, label, K, route)
    t = ops.seg_hist(pred, label, torch.zeros(3, K, dtype=torch.int64, device="cuda")).cpu()
    assert torch.equal(m.diagonal(), t[0]) and torch.equal(m.sum(0), t[1]) and torch.equal(m.sum(1), t[2])
    assert int(m.sum()) == int((label != 255).sum())
    # with invalid ones the diagonal still agrees
    pred, label = noise(91, 97, 131, K)
    m = check(pred.cuda(), label.cuda(), K, route)
    t = ops.seg_hist(pred.cuda(), label.cuda(), torch.zeros(3, K, dtype=torch.int64, device="cuda")).cpu()
    assert torch.equal(m.diagonal(), t[0])


# ------------------------------------------------------------------------------------------------------------------ capture
@pytest.mark.gpu
@pytest.mark.parametrize("route,K", [(None, 19), (None, 150), ("global", 19)])
def test_one_call_is_capturable_in_a_graph(route, K):
    from spike2former_amd import ops
    pred, label = noise(100, 97, 131, K)
    pred, label = pred.cuda(), label.cuda()
    single = check(pred, label, K, route)          # eager first: nothing is set up under capture
    acc = torch.zeros(K, K, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # one launch on one stream, no parallel branches
        ops.seg_confusion(pred, label, acc, route=route)
    acc.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), 3 * single)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.gpu
def test_evaluate_with_both_metrics_on_the_tiny_model():
    import dataclasses
    import spike2former_amd as s2f
    from oracle import s2f_oracle as so
    from spike2former_amd import ops
    from spike2former_amd.data_preprocessor import SegDataSample
    cfg = dataclasses.replace(so.CONFIGS["C1_64"], H=66, W=98, B=1)
    st = so.make_params(cfg)
    model = s2f.MODELS.build(s2f.model_cfg("C1_64"))
    model.load_state_dict({k: v.detach() for k, v in st.items()}, strict=True)
    model = model.cuda()
    K, ori = cfg.num_classes, (61, 90)
    gen = torch.Generator().manual_seed(110)
    batches, pixels = [], 0
    for i in range(2):
        img = torch.randn(3, cfg.H, cfg.W, generator=gen)
        lab = torch.randint(0, K, (ori[0] // 8 + 1, ori[1] // 8 + 1), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)
        lab = lab[:ori[0], :ori[1]].to(torch.uint8)
        lab[:3] = 255
        pixels += int((lab != 255).sum())
        meta = dict(img_shape=(cfg.H, cfg.W), ori_shape=ori, pad_shape=(cfg.H, cfg.W), padding_size=[0, 5, 0, 3], img_path=f"img{i}.png",
                    flip=False)
        batches.append(dict(inputs=[img], data_samples=[SegDataSample(gt_sem_seg=lab[None].contiguous(), metainfo=meta)]))
    names = [str(i) for i in range(K)]
    iou, cm = s2f.IoUMetric(), s2f.ConfusionMatrix(prefix="cm")
    iou.dataset_meta = cm.dataset_meta = dict(classes=names)
    before = dict(ops.FALLBACKS)
    got = s2f.evaluate(model, batches, [iou, cm])
    assert dict(ops.FALLBACKS) == before
    assert list(got) == ["aAcc", "mIoU", "mAcc", "cm/aAcc", "cm/mIoU", "cm/mAcc"]
    for k in ("aAcc", "mIoU", "mAcc"):
        assert got[k] == got[f"cm/{k}"] or (np.isnan(got[k]) and np.isnan(got[f"cm/{k}"])), (k, got)
    assert cm.matrix.shape == (K, K) and int(cm.matrix.sum()) == pixels > 0          # the arg-max is always a class
    assert cm._acc.is_cuda and not bool(cm._acc.any())
