"""The device-side training augmentation under the second resize rule -- RandomChoiceResize over ResizeShortestEdge, the
`train_pipeline` of the ADE20K, Cityscapes and COCO-Stuff MaskFormer configs -- against the numpy restatement tests/aug_ref.py.  The
kernels are those of tests/test_gpu_augment.py; what is new is the host side that produces the table's (H, W)
(spike2former_amd.augment.shortest_edge_size, TrainAugment(scales=..., max_size=...)), so these tests run the sizes that rule
produces: an enlargement that ends one pixel short of the cap, a portrait picture, a reduction to less than the crop.  As there:
the integers equal the restatement, the image equals it bit for bit, and every output is pre-filled before the launches."""
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as R  # noqa: E402
from test_augment_host import preprocessor  # noqa: E402
from test_gpu_augment import SOURCES, entry, make, prefilled, ref_kwargs, region_map, run_and_compare, scene  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROPS = ((32, 32), (30, 30))          # 16-byte stores, scalar stores

# (h0, w0), scale, max_size -> (H, W) (tests/test_shortest_edge_host.py has the whole table)
ROWS = [
    ((17, 28), 48, 60, (36, 59)),          # x 2.1, the long edge one short of the cap (rounded twice)
    ((37, 53), 48, 60, (42, 60)),          # capped
    ((53, 37), 48, 60, (60, 42)),          # portrait
    ((20, 27), 33, 1000, (33, 45)),        # an odd short edge, no cap
    ((64, 96), 12, 1000, (12, 18)),        # x 1 / 5.3: smaller than the crop in both directions, padding right and bottom
]


def shortest_edge(crop, scales, max_size, **kw):
    return make(crop, scale=None, scales=scales, max_size=max_size, **kw)


# ------------------------------------------------------------------------------------------------ 1. the sizes of the rule
@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("src, scale, max_size, size", ROWS)
def test_sizes_of_the_rule(src, scale, max_size, size, crop):
    from spike2former_amd.augment import shortest_edge_size
    assert shortest_edge_size(*src, scale, max_size) == size
    img, seg = scene(*src, seed=60)
    aug = shortest_edge(crop, [scale], max_size)
    drawn = aug.draw([src])[0]
    assert (int(drawn["H"]), int(drawn["W"])) == size          # one scale: whatever the variate, this size
    my, mx = R.margins(*size, crop)
    got_in, got_seg = run_and_compare(aug, [img], [seg], [entry(aug, *src, *size, origins=(my, mx))])
    if size[0] < crop[0] and size[1] < crop[1]:
        assert (got_seg[0, size[0]:] == 255).all() and (got_seg[0, :, size[1]:] == 255).all()
        assert (got_in[0, :, size[0]:] == 0).all() and (got_in[0, :, :, size[1]:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("cat_max_ratio", (1.0, 0.75))
@pytest.mark.parametrize("crop", CROPS)
def test_batch_of_three_sizes_with_drawn_parameters(crop, cat_max_ratio):
    """B = 3, three source sizes, parameters from TrainAugment.draw in the new mode with every transform on, with and without the
    crop rule (two launches / one): outputs, every flag and the chosen candidate equal the restatement"""
    from spike2former_amd.augment import shortest_edge_size
    scales = [24, 31, 48, 57]
    pairs = [scene(h, w, seed=70 + i) for i, (h, w) in enumerate(SOURCES)]
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    aug = shortest_edge(crop, scales, 60, batch=3, cat_max_ratio=cat_max_ratio, flip_prob=0.5, photometric=True,
                        reduce_zero_label=True, seed=crop[0])
    seen = set()
    for _ in range(3):
        params = aug.draw([s.shape for s in segs])
        for p, s in zip(params, segs):
            assert (int(p["H"]), int(p["W"])) in {shortest_edge_size(*s.shape, k, 60) for k in scales}
            seen.add((int(p["H"]), int(p["W"])))
        out = prefilled(aug, 3)
        staged = aug.stage(images, segs, params)
        aug.launch(out)
        want = [R.pipeline(i, s, p, crop, **ref_kwargs(aug)) for i, s, p in zip(images, segs, staged)]
        assert np.array_equal(out[1].cpu().numpy(), np.stack([w["seg"] for w in want]))
        assert np.array_equal(out[0].cpu().numpy(), np.stack([w["inputs"] for w in want]))
        if cat_max_ratio < 1.0:
            assert aug._flags.cpu().tolist() == [[int(f) for f in w["flags"]] for w in want]
        else:
            assert [w["choice"] for w in want] == [0, 0, 0]
    assert len(seen) > 3


# ------------------------------------------------------------------------------------------------ 3. graph capture
def test_graph_replays_follow_the_drawn_scales():
    pairs = [scene(h, w, seed=80 + i) for i, (h, w) in enumerate(SOURCES)]
    images, segs = [p[0] for p in pairs], [p[1] for p in pairs]
    crop = (32, 32)
    aug = shortest_edge(crop, [24, 31, 48, 57], 60, batch=3, cat_max_ratio=0.75, photometric=True, flip_prob=0.5, seed=9)
    out = prefilled(aug, 3)
    first = aug.stage(images, segs, aug.draw([s.shape for s in segs]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.launch(out)                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # the two launches: one chain
        aug.launch(out)
    sizes = []
    for k, table in enumerate((first, None)):
        table = aug.stage(images, segs, table if table is not None else aug.draw([s.shape for s in segs]))
        sizes.append([(int(p["H"]), int(p["W"])) for p in table])
        out[0].fill_(float("nan"))
        out[1].fill_(7)
        graph.replay()
        want_in, want_seg, _ = R.batch(images, segs, table, crop, **ref_kwargs(aug))
        assert np.array_equal(out[1].cpu().numpy(), want_seg), k
        assert np.array_equal(out[0].cpu().numpy(), want_in), k
    assert all(a != b for a, b in zip(*sizes)), "the two draws were to pick different scales for every picture"
    del graph


# ------------------------------------------------------------------------------------------------ 4. the training step
def test_training_step_fed_from_the_ade20k_pipeline():
    """TrainAugment.from_cfg on the ADE20K MaskFormer config's own train_pipeline, its sizes replaced by the tiny configuration's,
    writing GraphedHungarianStep(assign="device")'s static buffers in place: they equal the restatement, the losses are finite"""
    import spike2former_amd as s2f
    from spike2former_amd.augment import TrainAugment, shortest_edge_size
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    crop = (w["H"], w["W"])
    scales = [32, 48, 64, 96]
    with open(os.path.join(ROOT, "tests", "golden", "train_pipelines.json")) as f:
        pipeline = json.load(f)["SDTv2_maskformer_DCNpixelDecoder_ade20k.py"]["train_pipeline"]
    kinds = [t["type"] for t in pipeline]
    pipeline = [dict(t) for t in pipeline]
    pipeline[kinds.index("RandomChoiceResize")].update(scales=scales, max_size=160)
    pipeline[kinds.index("RandomCrop")].update(crop_size=crop)
    aug = TrainAugment.from_cfg(pipeline, preprocessor(crop), batch_size=2, max_source_pixels=70 * 90, seed=11, rank=0)
    assert aug.scales == tuple(scales) and aug.max_size == 160 and aug.cat_max_ratio == 0.75 and aug.reduce_zero_label is True
    assert aug.photometric is not None and aug.flip_prob == 0.5 and aug.crop_size == crop

    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    s2f.set_keep_membrane(model, False)
    red = FlatGradAllReduce(model.parameters(), 1)
    rng = np.random.default_rng(50)
    shapes = ((70, 90), (64, 48))
    images = [rng.integers(0, 256, (h, ww, 3), dtype=np.uint8) for h, ww in shapes]
    segs = [region_map(h, ww, rng.permutation(w["K"])[:5 + i]) for i, (h, ww) in enumerate(shapes)]
    example_in = torch.randn(2, 3, *crop, generator=torch.Generator().manual_seed(5)).cuda()
    example_seg = torch.from_numpy(np.stack([region_map(*crop, [1, 2, 3]), region_map(*crop, [4, 5])])).cuda()
    step = GraphedHungarianStep(model, example_in, example_seg, red, warmup=1, assign="device")
    table = aug.draw(shapes)
    for p, s in zip(table, shapes):
        assert (int(p["H"]), int(p["W"])) in {shortest_edge_size(*s, k, 160) for k in scales}
    want_in, want_seg, _ = R.batch(images, segs, table, crop, **ref_kwargs(aug))
    step.static_in.fill_(float("nan"))
    step.static_seg.fill_(7)
    aug(images, segs, table, out=(step.static_in, step.static_seg))
    got = step()
    step.check()
    got = {k: float(v) for k, v in got.items()}
    assert np.array_equal(step.static_in.cpu().numpy(), want_in) and np.array_equal(step.static_seg.cpu().numpy(), want_seg)
    assert all(np.isfinite(v) for v in got.values()) and len(got) > 0
    del step
    for p in model.parameters():
        p.grad = None
    gc.collect()
