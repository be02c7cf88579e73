"""RPVNet on the GPU (HIP kernels) against what the REAL reference produced for the same batch and parameters
(tests/golden/model_rpvnet.npz, tests/golden/make_golden_rpvnet.py), with the bars tests/test_gpu_spvcnn_model.py sets for SPVCNN:
logits within 1e-3, loss within 1e-3, the stored gradients within 2e-2 (BatchNorm in training mode) / 1e-4 (on running statistics) of
the reference's norm tensor by tensor, every parameter's gradient norm as there (profiles/rpvnet_float64.txt keeps the measured
distances).  The fixture stores every `logit_step`-th row of the per-voxel logits and `strided_sample`s of gradients above `full_below`
elements; both are compared on the same elements.

Evaluation branch: logits within 1e-3; `point_predict` equal at every point whose reference top-2 margin exceeds 2e-3.  Two training
steps from one state give the same bits for the loss, the logits and every parameter's gradient - what the float atomics of the
reference's `denselize` cannot give - once torch.backends.cudnn.deterministic keeps the library's own convolutions to deterministic
solvers.  The chain (`_RANGE_TAIL_KERNEL = False`) and the planes layout meet the same bars as the kernel
path.  `evaluate(on_device=True)` returns the host path's matrix and payloads bit for bit in its three modes.  A step runs on inputs
built by `build_range_inputs`.  Under autocast the model runs and its logits stay within 4 x the distance that half storage moves a
float64 evaluation."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rpvnet_ref as R  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, IF_DIST=True, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
LOGIT_TOL = 1e-3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_rpvnet.npz"), allow_pickle=False))


def _model(g, **kw):
    from taseg_amd.pcseg.model.segmentor.fusion.rpvnet import RPVNet
    model = RPVNet(make_model_cfg("RPVNet", **{**CFG, **kw}), 20)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return fill_parameters(model, seed=int(g["param_seed"])).cuda()


def _image(g):
    h, w = (int(v) for v in g["hw"])
    b = len(g["num_points"])
    rows = np.tile(np.array([-10, -10, 0, 0, 0], dtype=np.float32), (b * h * w, 1))
    rows[g["image_at"]] = g["image_values"]
    return np.ascontiguousarray(rows.reshape(b, h, w, 5).transpose(0, 3, 1, 2))


def _batch(g):
    from taseg_amd.torchsparse import SparseTensor
    coords = torch.from_numpy(g["coords"]).cuda()
    pc = torch.zeros((len(g["point_batch"]), 4), dtype=torch.int32)
    pc[:, 3] = torch.from_numpy(g["point_batch"].astype(np.int32))
    pc = pc.cuda()
    return {"lidar": SparseTensor(torch.from_numpy(g["feats"]).cuda(), coords),
            "targets": SparseTensor(torch.from_numpy(g["labels"].astype(np.int64)).cuda(), coords),
            "inverse_map": SparseTensor(torch.from_numpy(g["inverse_map"].astype(np.int64)).cuda(), pc),
            "targets_mapped": SparseTensor(torch.from_numpy(g["point_labels"]).cuda(), pc),
            "range_image": torch.from_numpy(_image(g)).cuda(), "range_pxpy": torch.from_numpy(g["range_pxpy"]).cuda(),
            "num_points": torch.from_numpy(g["num_points"]), "offset": torch.tensor([0], device="cuda"), "name": g["name"].tolist()}


def _step(model, g, bn_training=True, amp=False, batch=None):
    model.train()
    if not bn_training:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    got = {}
    hook = model.classifier.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().float()))
    bd = _batch(g) if batch is None else batch
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        ret, tb, disp = model(bd)
    hook.remove()
    model.zero_grad()
    ret["loss"].float().backward()
    assert int(bd["_plan"]["range_err"]) == 0
    return ret, tb, got["logits"], {n: p.grad for n, p in model.named_parameters()}


def _against_the_fixture(g, tag, model, tb, logits, grads):
    training = tag == "train"
    logits = logits.cpu().numpy()[::int(g["logit_step"])]
    print(f"{tag}: max |logits - ref| {np.abs(logits - g[f'{tag}_logits']).max():.2e} (logits up to {np.abs(logits).max():.1f}), loss "
          f"{float(tb['loss']):.6f} vs {float(g[f'{tag}_loss']):.6f}")
    assert logits.shape == g[f"{tag}_logits"].shape and np.abs(logits - g[f"{tag}_logits"]).max() <= LOGIT_TOL
    assert abs(float(tb["loss"]) - float(g[f"{tag}_loss"])) <= 1e-3
    tol = 2e-2 if training else 1e-4
    seen = 0
    for k in g:
        if k.startswith(f"{tag}_grad/"):
            a, b = grads[k.split("/", 1)[1]].detach().cpu(), g[k]
            a = (a if a.numel() <= int(g["full_below"]) else strided_sample(a)).numpy()
            rel = np.linalg.norm(a - b) / np.linalg.norm(b)
            print(f"{k}: |got - ref| / |ref| = {rel:.2e}")
            assert a.shape == b.shape and rel <= tol, k
            seen += 1
    assert seen >= 15
    norms = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
    worst = np.abs(norms - g[f"{tag}_gradnorms"]) / (1e-6 + (5e-2 if training else 1e-3) * np.abs(g[f"{tag}_gradnorms"]))
    print(f"{tag}: worst gradient norm at {worst.max():.3g} of its allowance")
    assert np.allclose(norms, g[f"{tag}_gradnorms"], rtol=5e-2 if training else 1e-3, atol=1e-6)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_vs_reference_golden(g, training):
    model = _model(g)
    ret, tb, logits, grads = _step(model, g, training)
    _against_the_fixture(g, "train" if training else "eval", model, tb, logits, grads)


def test_chain_and_planes_layout_meet_the_same_bars(g, monkeypatch):
    """`_RANGE_TAIL_KERNEL = False` (the chain spdevoxelize + range_to_point + relu(bn(y))) and options.image_layout = 'nchw' (the
    four hand-overs convert) are the same network"""
    from taseg_amd.options import options
    from taseg_amd.torchsparse.nn import functional as F
    monkeypatch.setattr(F, "_RANGE_TAIL_KERNEL", False)
    model = _model(g)
    ret, tb, logits, grads = _step(model, g)
    _against_the_fixture(g, "train", model, tb, logits, grads)
    monkeypatch.setattr(F, "_RANGE_TAIL_KERNEL", True)
    monkeypatch.setattr(options, "image_layout", "nchw")
    model = _model(g)
    ret, tb, logits, grads = _step(model, g)
    _against_the_fixture(g, "train", model, tb, logits, grads)


def test_local_batch_norm_modules_give_the_bits_of_the_sync_modules_in_one_process(g, monkeypatch):
    """IF_DIST False - which the reference cannot run - is the same network on nn.BatchNorm1d / BatchNorm2d: the fixture's bars, and,
    without a process group, the kernels the SyncBatchNorm modules of IF_DIST True take - the same bits (the library's dense
    convolutions kept to deterministic solvers, as in the two-steps test)"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(g, IF_DIST=False)
    ret, tb, logits, grads = _step(model, g)
    _against_the_fixture(g, "train", model, tb, logits, grads)
    dist = _step(_model(g), g)
    assert torch.equal(dist[2], logits) and torch.equal(dist[0]["loss"], ret["loss"])


def test_evaluation_branch(g):
    model = _model(g).eval()
    with torch.no_grad():
        out = model(_batch(g))
    assert set(out) == {"point_predict", "point_labels", "name", "point_predict_logits"} and out["name"] == g["name"].tolist()
    n_pts = g["num_points"].tolist()
    assert [len(p) for p in out["point_predict"]] == n_pts == [len(p) for p in out["point_labels"]]
    logits = np.concatenate(out["point_predict_logits"])
    per_scan = [int((g["coords"][:, 3] == b).sum()) for b in range(len(n_pts))]
    rows = g["inverse_map"].astype(np.int64) + np.concatenate([[0], np.cumsum(per_scan)])[g["point_batch"]]
    step = int(g["logit_step"])
    kept = rows % step == 0
    want = g["branch_logits"][rows[kept] // step]
    print(f"evaluation branch: max |logits - ref| {np.abs(logits[kept] - want).max():.2e}")
    assert kept.sum() > len(rows) // (2 * step) and np.abs(logits[kept] - want).max() <= LOGIT_TOL
    sure = g["branch_margin"] > float(g["margin"])
    assert sure.mean() >= 0.99
    pred = np.concatenate(out["point_predict"])
    assert np.array_equal(pred[sure], g["branch_point_predict"][sure].astype(pred.dtype))
    assert np.array_equal(np.concatenate(out["point_labels"]), g["branch_point_labels"])
    with pytest.raises(TypeError):                                 # reproduced: rpvnet.py:751-752 passes ensemble=True
        with torch.no_grad():
            model.forward_ensemble(_batch(g))


def test_two_training_steps_from_one_state_give_the_same_bits(g, monkeypatch):
    """Everything this project computes is run-to-run identical; the dense convolutions of the range branch are the library's
    (MIOpen behind nn.Conv2d), which at stage 4 picks a solver that adds with float atomics unless PyTorch's own switch asks for
    deterministic ones - so the switch is part of the statement: with torch.backends.cudnn.deterministic = True the loss, the logits,
    every gradient and every running statistic have the same bits (measured without it: the first tensor to differ is
    range_branch.stage4.conv2's output, profiles/rpvnet_float64.txt)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    runs = []
    for _ in range(2):
        model = _model(g, IF_DIST=False)
        ret, tb, logits, grads = _step(model, g)
        runs.append((ret["loss"].detach().clone(), logits, grads, {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def test_a_step_on_inputs_from_build_range_inputs(g):
    """the device stage on the batch's own rows and the fixture's cuts gives the reference's inputs - outside the rows its bound
    leaves undecided - and the model trains on them"""
    from taseg_amd.data.range import build_range_inputs
    bd = _batch(g)
    want_image, want_pxpy = bd.pop("range_image"), bd.pop("range_pxpy")
    image, pxpy, err = build_range_inputs(bd["lidar"], g["cuts"].tolist(), tuple(int(v) for v in g["hw"]), batch_dict=bd)
    assert int(err) == 0 and image.shape == want_image.shape and pxpy.shape == want_pxpy.shape
    moved = (pxpy != want_pxpy).any(1).cpu().numpy()
    px64 = R.proj_x64(g["feats"], g["coords"][:, 3], g["cuts"], int(g["hw"][1]))
    near = np.abs(px64 - np.floor(px64) - 0.5) <= R.stage_delta(int(g["hw"][1]))
    assert near.mean() <= 0.01 and not (moved & ~near).any()
    if not moved.any():
        assert torch.equal(image, want_image)
    model = _model(g)
    ret, tb, logits, grads = _step(model, g, batch=bd)
    assert bool(torch.isfinite(ret["loss"]).all())
    if not moved.any():
        assert abs(float(tb["loss"]) - float(g["train_loss"])) <= 1e-3


@pytest.mark.parametrize("predictions", [False, True], ids=["matrix", "payloads"])
def test_evaluate_on_device_equals_the_host_path(g, predictions):
    from taseg_amd.pcseg.eval import evaluate
    model = _model(g).eval()
    host = evaluate(model, [_batch(g), _batch(g)], 20, predictions=predictions, prefetch=False)
    dev = evaluate(model, [_batch(g), _batch(g)], 20, predictions=predictions, prefetch=False, on_device=True)
    assert np.array_equal(host["hist"], dev["hist"]) and host["hist"].sum() > 0
    assert np.array_equal(host["iou"], dev["iou"], equal_nan=True)
    if predictions:
        assert len(host["predictions"]) == len(dev["predictions"]) == 4
        for a, b in zip(host["predictions"], dev["predictions"]):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_tta_votes_on_device_equal_the_host_path(g):
    """the third mode of evaluate(on_device=True): the scenes of a batch as the votes of one scan (here the same scan twice)"""
    from taseg_amd.pcseg.eval import evaluate
    from taseg_amd.torchsparse import SparseTensor
    model = _model(g).eval()

    def votes():
        bd = _batch(g)
        n0 = int((g["coords"][:, 3] == 0).sum())
        p0 = int(g["num_points"][0])
        c = torch.cat([bd["lidar"].C[:n0], bd["lidar"].C[:n0]])
        c[n0:, 3] = 1
        f = torch.cat([bd["lidar"].F[:n0], bd["lidar"].F[:n0] * 1.01])
        pc = torch.cat([bd["inverse_map"].C[:p0], bd["inverse_map"].C[:p0]])
        pc[p0:, 3] = 1
        inv = torch.cat([bd["inverse_map"].F[:p0], bd["inverse_map"].F[:p0]])
        lab = torch.cat([bd["targets_mapped"].F[:p0], bd["targets_mapped"].F[:p0]])
        pxpy = torch.cat([bd["range_pxpy"][:n0], bd["range_pxpy"][:n0]])
        pxpy[n0:, 0] = 1
        image = torch.cat([bd["range_image"][:1], bd["range_image"][:1] * 1.01])
        return {"lidar": SparseTensor(f, c), "inverse_map": SparseTensor(inv, pc), "targets_mapped": SparseTensor(lab, pc),
                "range_image": image, "range_pxpy": pxpy, "num_points": torch.tensor([p0, p0]), "name": ["scan/a/b.bin", "scan/a/b.bin"]}

    host = evaluate(model, [votes()], 20, tta_votes=2, prefetch=False)
    dev = evaluate(model, [votes()], 20, tta_votes=2, prefetch=False, on_device=True)
    assert len(host["predictions"]) == len(dev["predictions"]) == 1
    assert np.array_equal(host["predictions"][0], dev["predictions"][0])


class _Done(Exception):
    pass


def _float64_logits(g, round_half, monkeypatch):
    """Logits of the training-mode forward in float64 on tensor ops: SPVCNN's evaluator (tests/test_gpu_spvcnn_model.py) for the voxel
    and point branches; the range branch as its own modules in double (hooks round every Conv2d / BatchNorm2d / AvgPool2d output);
    `point_to_range`, `range_to_point` and the hand-over as index_add / gather.  round_half: every tensor the autocast run stores in
    half is rounded to half on the way, and the weights autocast casts (Linear, Conv2d and their biases; sparse convolutions with both
    channel counts multiples of 32)."""
    import taseg_amd.torchsparse.nn as spnn
    from taseg_amd.torchsparse.nn import functional as F
    from taseg_amd.torchsparse.utils import make_ntuple
    q = (lambda t: t.half().double()) if round_half else (lambda t: t)
    model = _model(g, IF_DIST=False).double().train()

    def conv64(self, x):
        dense = self.in_channels % 32 == 0 and self.out_channels % 32 == 0
        if tuple(make_ntuple(self.kernel_size, ndim=3)) == (1, 1, 1):
            return x._like(x.F @ (q(self.kernel) if dense else self.kernel))
        kmap, out_coords, out_stride = F.conv_geometry(x, self.kernel_size, self.stride, make_ntuple(self.dilation, ndim=3), self.transposed)
        n_in, n_out = kmap.sizes
        w = (q(self.kernel) if dense else self.kernel).view(-1, self.in_channels, self.out_channels)
        out = torch.zeros((n_in if self.transposed else n_out, self.out_channels), dtype=torch.float64, device=x.F.device)
        pairs, off = kmap.nbmaps, 0
        for k, size in enumerate(kmap.nbsizes.tolist()):
            p = pairs[off:off + size]
            src, dst = (p[:, 1], p[:, 0]) if self.transposed else (p[:, 0], p[:, 1])
            out.index_add_(0, dst, x.F[src] @ w[k])
            off += size
        return F._conv_output(x, out, out_coords, out_stride)

    def rounded(fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            if isinstance(out, tuple):
                out[0].F = q(out[0].F)
            else:
                out.F = q(out.F)
            return out
        return wrapped

    def devox64(feats, idx, w, order=None):
        live = ((idx >= 0) & (w != 0)).double() * w.double()
        return (feats[idx.clamp(min=0).long()] * live.unsqueeze(-1)).sum(1)

    def tail64(y, bn, vox, idx, w, order, fmap, plan):
        rows = fmap.permute(0, 2, 3, 1).reshape(-1, fmap.shape[1])
        return q((devox64(vox, idx, w) + devox64(rows, plan["bidx"], plan["bw"])) + torch.relu(bn(q(y))))

    mean64 = F.spvoxelize_mean                                      # (double rows: index_add of feat / cnt)
    bd = _batch(g)
    model.prepare(bd)
    bd["lidar"].F = bd["lidar"].F.double()
    bd["range_image"] = bd["range_image"].double()
    monkeypatch.setattr(spnn.Conv3d, "forward", conv64)
    monkeypatch.setattr(spnn, "conv_bn_act", rounded(spnn.conv_bn_act))
    monkeypatch.setattr(F, "spdevoxelize", lambda f, i, w, order=None: q(devox64(f, i, w)))
    monkeypatch.setattr(F, "spvoxelize", lambda f, i, c: q(mean64(f, i, c.shape[0])))
    monkeypatch.setattr(F, "spvoxelize_mean", lambda f, i, m, groups=None: q(mean64(f, i, m)))
    monkeypatch.setattr(F, "range_point_tail", tail64)
    hooks = [m.register_forward_hook(lambda m, i, o: q(o)) for m in model.range_branch.modules()
             if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.AvgPool2d))]
    if round_half:
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)):
                    m.weight.copy_(q(m.weight))
                    m.bias.copy_(q(m.bias))
    got = {}

    def grab(m, i, o):
        got["logits"] = o.detach()
        raise _Done

    hook = model.classifier.register_forward_hook(grab)
    with torch.no_grad(), pytest.raises(_Done):
        model(bd)
    hook.remove()
    for h in hooks:
        h.remove()
    monkeypatch.undo()
    return got["logits"]


def test_autocast_runs_and_stays_close_to_fp32(g, monkeypatch):
    """Bar, taken as tests/test_gpu_spvcnn_model.py takes its own: 4 x the distance a float64 evaluation moves when every tensor the
    autocast run stores in half is rounded to half (`_float64_logits`) - the format's own error on this network and batch, measured
    without the code under test; printed, and kept in profiles/rpvnet_float64.txt."""
    fp32 = _step(_model(g, IF_DIST=False), g)
    amp = _step(_model(g, IF_DIST=False), g, amp=True)
    assert bool(torch.isfinite(amp[0]["loss"]).all())
    exact = _float64_logits(g, False, monkeypatch)
    print(f"fp32 logits vs the float64 evaluation: {float((fp32[2].double() - exact).abs().max()):.3e}")
    assert float((fp32[2].double() - exact).abs().max()) <= LOGIT_TOL              # the float64 evaluation is this network
    half64 = float((_float64_logits(g, True, monkeypatch) - exact).abs().max())
    d = float((fp32[2] - amp[2]).abs().max())
    print(f"autocast: max |logits - fp32| {d:.3e} (logits up to {float(fp32[2].abs().max()):.2f}); half-rounded float64 evaluation "
          f"moves {half64:.3e}: bar {4 * half64:.3e}")
    assert d <= 4.0 * half64
    assert all(p is not None and bool(torch.isfinite(p).all()) for p in amp[3].values())
