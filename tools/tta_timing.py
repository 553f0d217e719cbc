"""Wall time of one test-time-augmented image on the C2 model (eval, B = 1, T = 4): the reference's ADE20K tta_pipeline --
ratios 0.5 .. 1.75 x {no flip, horizontal flip} = 12 views of a 512 x 683 image (ade20k.py:28-43) -- through SegTTAModel.test_step,
and the eager single-view predict at 512 x 683 for comparison.  Median of 3 after one warm-up.
    python tools/tta_timing.py > tta_timing.txt"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import spike2former_amd as s2f
from spike2former_amd import ops
from spike2former_amd.data_preprocessor import SegDataSample
from spike2former_amd.init_utils import seeded_init

ops.STRICT = True
dev = torch.device("cuda", 0)
model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C2"))).to(dev).eval()
s2f.set_keep_membrane(model, False)
tta = s2f.MODELS.build(dict(type="SegTTAModel", module=model))
ori = (512, 683)
img = torch.randn(1, 3, *ori, generator=torch.Generator().manual_seed(7))
views, samples = [], []
for r in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75):
    size = (int(ori[0] * r + 0.5), int(ori[1] * r + 0.5))
    x = F.interpolate(img, size=size, mode="bilinear", align_corners=False)[0]
    for flip in (False, True):
        views.append([(x.flip(-1) if flip else x).to(dev)])
        samples.append([SegDataSample(metainfo=dict(ori_shape=ori, img_shape=size, pad_shape=size, padding_size=[0, 0, 0, 0],
                                                    flip=flip, flip_direction="horizontal" if flip else None))])


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[1]


def one_view():
    s2f.reset_net(model)
    with torch.no_grad():
        return model(views[4][0][None], [SegDataSample(metainfo=dict(samples[4][0].metainfo))], mode="predict")


t_pred = timed(one_view)
t_tta = timed(lambda: tta.test_step(dict(inputs=views, data_samples=samples)))
print(f"C2 eval B=1 T=4: eager predict at 512x683 {t_pred:.2f} ms; 12-view TTA image (6 ratios x 2 flips, {views[0][0].shape[-2:]} .. "
      f"{views[-1][0].shape[-2:]}) {t_tta:.2f} ms; fall-backs {dict(ops.FALLBACKS) or 'none'}")
