"""Host: the inputs of tests/step_rig.py, pinned.  The captured-step tests quote figures measured on the MI355X (run-to-run gaps of
the weights and moments); they hold for exactly these pictures, label maps and constants.  The digests were
taken from make_batches and region_map as tests/test_gpu_train_loop.py held them before the rig had a module of its own: SHA-256 over
dtype, shape and bytes."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_rig as rig  # noqa: E402

# per batch: (the two pictures, the two label maps)
BATCHES = [
    (["5f9a92e0fdb6aa57a32f99a7141b566dde03a94a23bdf1398490b128eeb7ec6f", "9570f569e97cb46db8252c1b3365259b36d8d08e8283c481dde3d42915b68472"],
     ["2c5a7f97946ac591f3bc8c72215cd19dca28bb9a2a6ea349a1b0e7e0cbc9e15a", "668c08b2447f929cf9c858f88e48b5aa95969cb535972fe7165c516eeff69547"]),
    (["521b4cfdc8955169e7f86e05c94449e98a911c5de82cf14c576da2e6430947ab", "8380f3a02cfe6afa2604f1d6774bbf56ffb22ee1cb950d7cd246248ad9952e9b"],
     ["db4032b34954ca77aa6bce732b637b51ecb16c09c5a29236c0aff4bd64864be1", "b44465e1b9e75b1888cedc1f1e7aff1e5d94faa2bab3ed562fc4bb21c09638d4"]),
    (["1683d6ecd56af541e7ca9d0b66ff82ab8c0781a5453bf984f9830da05bf2ba32", "b7943302bc28a16abbb06b5614366d82da9d643650d09631c3c1ef4d36af351a"],
     ["9a84eda77a3f720c4bc48e385f75d531d67005d2245ffa89ad9e68a168fe2ef1", "5f50c194f6dd8ee0768334f5a43b121c9cd6fd8fc8f0f870c3bfb7e535594639"]),
]
EXAMPLE_SEG = ["cb33df238eb96639dd02afd67d09dd7dd696b9b789aafcba8d08329d856304df", "25ebe54734dabdc7d567cd80ad9ec5490240d1b5924c1119a5f61c14a86330ec"]
K, CROP = 20, (64, 64)          # C1_64


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def test_the_pictures_and_label_maps_are_the_ones_the_figures_were_measured_on():
    import spike2former_amd as s2f
    w = s2f.WORKLOADS["C1_64"]
    assert (w["K"], (w["H"], w["W"])) == (K, CROP)
    got = [([digest(a) for a in images], [digest(a) for a in segs]) for images, segs in rig.make_batches(K)]
    assert got == BATCHES
    assert [digest(rig.region_map(*CROP, classes)) for classes in ([1, 2, 3], [4, 5])] == EXAMPLE_SEG
    example_in, example_seg = rig.examples(CROP)
    assert example_in.shape == (2, 3, *CROP) and [digest(a) for a in example_seg.numpy()] == EXAMPLE_SEG


def test_the_constants_are_the_ones_the_figures_were_measured_on():
    assert rig.NORM == dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], bgr_to_rgb=True)
    assert rig.SHAPES == ((70, 90), (64, 48))
    assert rig.CLIP == dict(max_norm=0.01, norm_type=2)
    assert rig.PARAMWISE == dict(custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=1.0)})
