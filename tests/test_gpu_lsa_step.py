"""The real training step with the assignment on the device (loss_semantic(assign="device"), GraphedHungarianStep(assign="device"))
against the host route on the tiny config C1_64 -- the reference of every comparison is the host route (scipy's assignment)."""
import gc
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASSES = (5, 6, 16)          # per map; 16 > Q = 10: the solver's other orientation


def region_maps(B, H, W, K, n, seed):
    """[B, 1, H, W] semantic maps of n classes each, as a 4 x 4 grid of rectangles (+ a strip of the ignored label)."""
    g = torch.Generator().manual_seed(seed)
    seg = torch.empty(B, 1, H, W, dtype=torch.int64)
    for b in range(B):
        classes = torch.randperm(K, generator=g)[:n]
        for i, (y0, x0) in enumerate((y, x) for y in range(0, H, H // 4) for x in range(0, W, W // 4)):
            seg[b, 0, y0:y0 + H // 4, x0:x0 + W // 4] = classes[i % n]
        seg[b, 0, :2, 3:17] = 255
    return seg


def setup(n_pairs=3):
    import spike2former_amd as s2f
    from spike2former_amd.dist import FlatGradAllReduce
    from spike2former_amd.init_utils import seeded_init
    w = s2f.WORKLOADS["C1_64"]
    model = seeded_init(s2f.MODELS.build(s2f.model_cfg("C1_64"))).cuda().train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    s2f.set_keep_membrane(model, False)
    imgs = [torch.randn(2, 3, w["H"], w["W"], generator=torch.Generator().manual_seed(5 + i)).cuda() for i in range(n_pairs)]
    segs = [region_maps(2, w["H"], w["W"], w["K"], N_CLASSES[i], 6 + i).cuda() for i in range(n_pairs)]
    red = FlatGradAllReduce(model.parameters(), 1)
    return s2f, model, sd, imgs, segs, red


def drop(model):
    for p in model.parameters():
        p.grad = None
    gc.collect()


def close(got, want, rel):
    return all(abs(got[k] - want[k]) <= rel * max(abs(want[k]), 1e-3) for k in want)


def test_loss_semantic_device_route_is_the_host_route():
    s2f, model, sd, imgs, segs, red = setup()
    crit, ignore = model.decode_head.criterion, model.decode_head.ignore_index
    for img, seg in zip(imgs, segs):
        res = {}
        for assign in ("host", "device"):
            model.load_state_dict(sd); s2f.reset_net(model); red.zero()
            cls, masks = model(img)
            if assign == "device":
                with torch.no_grad():
                    cost, count = crit.costs_all_classes(cls, masks, crit.seg_as_u8(seg[:, 0], ignore))
                    got = crit.match_tables_device(cost, count)
                    want = crit.match_tables(cost.cpu().numpy(), count.cpu().numpy())
                assert int(got[3].item()) == 0
                for g, w_ in zip(got[:3], want):
                    assert np.array_equal(g.cpu().numpy(), w_) and g.cpu().numpy().dtype == w_.dtype
            losses = crit.loss_semantic(cls, masks, seg[:, 0], ignore, assign=assign)
            sum(losses.values()).backward()
            s2f.ops.wgrad_join()
            red.gather()
            res[assign] = ({k: float(v) for k, v in losses.items()}, red.flat.clone())
            del losses, cls, masks
        assert list(res["device"][0]) == list(res["host"][0])
        assert res["device"][0] == res["host"][0]                                 # same kernels on the same tables: bit-identical
        wg = res["host"][1]
        assert (res["device"][1] - wg).abs().max().item() <= 1e-4 * wg.abs().max().item()
    drop(model)


def _tables_are_the_hosts(step):
    """the tables of the last replay against match_tables on the costs of the same outputs, downloaded"""
    torch.cuda.synchronize()
    with torch.no_grad():
        cost, count = step.crit.costs_all_classes(step.outs[0], step.outs[1], step.static_seg)
    want = step.crit.match_tables(cost.cpu().numpy(), count.cpu().numpy())
    got = (step.tgt_labels, step.row_class, step.num_masks)
    differ = sum(int(not np.array_equal(g.cpu().numpy(), w_)) for g, w_ in zip(got, want))
    assert differ == 0, "a (layer, image) problem was assigned differently from scipy"          # zero allowed on these seeds


def test_device_graph_step_is_the_host_graph_step(monkeypatch):
    from spike2former_amd.graph import GraphedHungarianStep
    s2f, model, sd, imgs, segs, red = setup()
    order = (0, 1, 2, 0)
    model.load_state_dict(sd)
    host = GraphedHungarianStep(model, imgs[0], segs[0], red, warmup=1)
    assert host.assign == "host" and hasattr(host, "graph_b") and hasattr(host, "host_cost")
    want = []
    for i in order:
        model.load_state_dict(sd)
        got = host(imgs[i], segs[i])
        torch.cuda.synchronize()
        want.append(({k: float(v) for k, v in got.items()}, red.flat.clone()))
    host.check()                                              # nothing to report on the host route
    del host, got
    drop(model)

    model.load_state_dict(sd)
    step = GraphedHungarianStep(model, imgs[0], segs[0], red, warmup=1, assign="device")
    # one graph: no second graph, no pinned cost / table buffers
    assert step.assign == "device" and step.two_graphs is False
    for name in ("graph_a", "graph_b", "graph_tail", "host_cost", "host_count", "host_tgt", "host_rows", "host_avg"):
        assert not hasattr(step, name), name

    def no_wait(*a, **k):
        raise AssertionError("the device step waited for the GPU inside __call__")
    for n, i in enumerate(order):
        model.load_state_dict(sd)
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", no_wait)
            m.setattr(torch.cuda.Stream, "synchronize", no_wait)
            m.setattr(torch.cuda.Event, "synchronize", no_wait)
            got = step(imgs[i], segs[i])
        step.check()
        _tables_are_the_hosts(step)
        wl, wg = want[n]
        gl = {k: float(v) for k, v in got.items()}
        print(f"replay {n} (map of {N_CLASSES[i]} classes): max rel loss gap "
              f"{max(abs(gl[k] - wl[k]) / max(abs(wl[k]), 1e-3) for k in wl):.2e}, "
              f"grad gap / max|g| {(red.flat - wg).abs().max().item() / wg.abs().max().item():.2e}")
        assert list(gl) == list(wl)
        assert close(gl, wl, 1e-6), (n, gl, wl)
        assert (red.flat - wg).abs().max().item() <= 1e-4 * wg.abs().max().item(), n
    del step, got
    drop(model)


def test_device_graph_step_with_the_optimizer_captured():
    from spike2former_amd.graph import GraphedHungarianStep
    from spike2former_amd.train import FlatAdamW
    s2f, model, sd, imgs, segs, red = setup()
    lr = 0.001

    def run(assign):
        model.load_state_dict(sd)
        opt = FlatAdamW(model, red, lr=lr, weight_decay=0.005, clip_grad=dict(max_norm=0.01, norm_type=2))
        step = GraphedHungarianStep(model, imgs[0], segs[0], red, warmup=1, optimizer=opt, assign=assign)
        model.load_state_dict(sd)
        losses, params = [], [torch.cat([p.detach().flatten() for p in model.parameters()]).clone()]
        for i in (0, 1, 2):
            got = step(imgs[i], segs[i])
            step.check()
            torch.cuda.synchronize()
            losses.append({k: float(v) for k, v in got.items()})
            params.append(torch.cat([p.detach().flatten() for p in model.parameters()]).clone())
        if assign == "device":
            assert step.two_graphs is False and not hasattr(step, "graph_b")
        del step, got, opt
        drop(model)
        return losses, params

    l_a, p_a = run("host")
    l_b, p_b = run("host")
    l_d, p_d = run("device")
    assert torch.equal(p_a[0], p_d[0])                                                                     # the same start
    assert all(np.isfinite(v) for it in l_d for v in it.values())
    assert all((p_d[it + 1] - p_d[it]).abs().max().item() > 0 for it in range(3))                          # parameters move
    assert close(l_d[0], l_a[0], 1e-6), (l_d[0], l_a[0])
    # AdamW's first steps are ~ lr * sign(g): the flat buffer's admitted atomic noise can flip small entries, so the bound is what two
    # runs of the HOST route differ by from the same start (A/A), or the largest change a sign flip of one update can make (2 lr)
    for it in (1, 3):          # (after three updates: printed for the record, no bound is defined for it)
        aa = (p_a[it] - p_b[it]).abs().max().item()
        ab = (p_d[it] - p_a[it]).abs().max().item()
        print(f"parameters after {it} update(s): host vs host {aa:.3e}, device vs host {ab:.3e} (lr {lr})")
        if it == 1:
            assert ab <= max(2 * aa, 2 * lr), (aa, ab)


def test_out_of_range_label_gives_nan_losses_and_check_raises():
    from spike2former_amd.graph import GraphedHungarianStep
    s2f, model, sd, imgs, segs, red = setup(2)
    model.load_state_dict(sd)
    step = GraphedHungarianStep(model, imgs[0], segs[0], red, warmup=1, assign="device")
    bad = segs[1].clone()
    bad[1, 0, 40:44, 40:44] = 200                      # K = 20: neither a class nor the ignored label
    model.load_state_dict(sd)
    got = step(imgs[1], bad)
    with pytest.raises(ValueError, match="labels >= num_classes"):
        step.check()
    assert all(np.isnan(float(v)) for k, v in got.items() if k.endswith(("loss_mask", "loss_dice")))
    assert np.isnan(float(sum(got.values())))
    # the word is consumed: the next step on a clean map runs and is clean
    model.load_state_dict(sd)
    got = step(imgs[1], segs[1])
    step.check()
    assert all(np.isfinite(float(v)) for v in got.values())
    # without check(): the following __call__ reports what the previous replay left
    model.load_state_dict(sd)
    step(imgs[1], bad)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="labels >= num_classes"):
        step(imgs[1], segs[1])
    del step, got
    drop(model)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.timeout(900)
def test_two_graph_form_under_a_process_group_is_the_single_graph(tmp_path):
    """ONE fresh child with S2F_FORCE_DIST=1 (backend nccl = RCCL, world 1) captures the device step as graph A | graph B; a second
    child without a process group captures it as one graph.  Same losses and gradients (bounds of the graph-vs-eager test)."""
    outs = {}
    for tag, extra in (("rccl", {"S2F_FORCE_DIST": "1", "MASTER_PORT": str(_free_port())}), ("plain", {})):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
        env.pop("S2F_DIST_BACKEND", None)
        if tag == "plain":
            env.pop("S2F_FORCE_DIST", None)
        out = str(tmp_path / f"{tag}.pt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lsa_rccl_worker.py"), out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=400)          # a child process: nothing is re-exec'ed
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert f"backend {'nccl' if tag == 'rccl' else 'none'} two_graphs {tag == 'rccl'}" in r.stdout, r.stdout[-1000:]
        outs[tag] = torch.load(out)
    for (la, fa), (lb, fb) in zip(outs["rccl"]["steps"], outs["plain"]["steps"]):
        assert list(la) == list(lb) and close(la, lb, 1e-6), (la, lb)
        assert (fa - fb).abs().max().item() <= 1e-4 * fb.abs().max().item()
