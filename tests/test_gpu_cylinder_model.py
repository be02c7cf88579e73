"""Cylinder_TS on the GPU (HIP kernels) against what the REAL reference produced for the same batch and parameters
(tests/golden/model_cylinder.npz, tests/golden/make_golden_cylinder.py), with the bars tests/test_gpu_model.py sets for the same
comparison: voxel and point logits within 1e-3, both losses within 1e-3, the stored gradients within 2e-2 (BatchNorm in training
mode) / 1e-4 (on running statistics) of the reference's norm tensor by tensor, every parameter's gradient norm as there.  Gradients of
tensors above `full_below` elements are stored as `strided_sample`s and compared on the same elements.

Evaluation branch: logits within 1e-3; `point_predict` equal at every point whose reference top-2 margin exceeds 2e-3 (a point below
it may flip on a 1e-3 difference; the fixture leaves at most 1 % of the points out, checked on the host).  Two training steps from
one state give the same bits.  Under autocast the model runs and its voxel logits stay within 4 x the distance that
half storage moves a float64 evaluation (see the test)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_dim=9, INIT_SIZE=16, LABEL_SMOOTHING=0.0, POINT_REFINEMENT=True, DROPOUT_P=0.0)
LOGIT_TOL = 1e-3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_cylinder.npz"), allow_pickle=False))


def _model(g, **kw):
    from taseg_amd.pcseg.model import build_network
    return fill_parameters(build_network(make_model_cfg("Cylinder_TS", **CFG, **kw), 20), seed=int(g["param_seed"])).cuda()


def _batch(g):
    bd = {k[len("batch_"):]: torch.from_numpy(v).cuda() for k, v in g.items() if k.startswith("batch_") and k != "batch_name"}
    for k in ("point_coord", "voxel_coord", "point_label", "voxel_label", "inverse_map", "num_points"):
        bd[k] = bd[k].long()                                       # collate_batch's types (semantickitti_cylinder.py:192-200)
    bd["name"] = g["batch_name"].tolist()
    return bd


def _step(model, g, bn_training=True, amp=False):
    model.train()
    if not bn_training:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    got = {}
    hooks = [model.logits.register_forward_hook(lambda m, i, o: got.update(logits=o.F.detach().float(), coords=o.C)),
             model.point_logits.register_forward_hook(lambda m, i, o: got.__setitem__("point_logits", o.detach().float()))]
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        ret, tb, disp = model(_batch(g))
    for h in hooks:
        h.remove()
    model.zero_grad()
    ret["loss"].float().backward()
    return ret, tb, disp, got, {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_vs_reference_golden(g, training):
    tag = "train" if training else "eval"
    model = _model(g)
    ret, tb, disp, got, grads = _step(model, g, training)
    assert np.array_equal(got["coords"].cpu().numpy(), g["voxel_order"])           # voxel rows in ascending-hash order, as the reference's
    logits, point_logits = got["logits"].cpu().numpy(), got["point_logits"].cpu().numpy()
    print(f"{tag}: max |voxel logits - ref| {np.abs(logits - g[f'{tag}_logits']).max():.2e}, point logits "
          f"{np.abs(point_logits - g[f'{tag}_point_logits']).max():.2e}, loss {tb['loss']:.6f} vs {float(g[f'{tag}_loss']):.6f}, "
          f"loss_point {tb['loss_point']:.6f} vs {float(g[f'{tag}_loss_point']):.6f}")
    assert np.abs(logits - g[f"{tag}_logits"]).max() <= LOGIT_TOL
    assert np.abs(point_logits - g[f"{tag}_point_logits"]).max() <= LOGIT_TOL
    assert set(tb) == set(disp) == {"loss", "loss_point"} and set(ret) == {"loss"}
    assert abs(tb["loss"] - float(g[f"{tag}_loss"])) <= 1e-3
    assert abs(tb["loss_point"] - float(g[f"{tag}_loss_point"])) <= 1e-3
    assert abs(float(ret["loss"]) - float(g[f"{tag}_loss_total"])) <= 2e-3
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
    assert seen >= 5
    norms = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
    assert np.allclose(norms, g[f"{tag}_gradnorms"], rtol=5e-2 if training else 1e-3, atol=1e-6)


def test_evaluation_branch(g):
    model = _model(g).eval()
    with torch.no_grad():
        out = model(_batch(g))
    assert set(out) == {"point_predict", "point_labels", "name", "point_predict_logits"} and out["name"] == g["batch_name"].tolist()
    n_pts = g["batch_num_points"].tolist()
    assert [len(p) for p in out["point_predict"]] == n_pts == [len(p) for p in out["point_labels"]]
    logits = np.concatenate(out["point_predict_logits"])
    want = g["eval_logits"][g["branch_point_row"]]                 # (the maker asserts this is the reference's output bit for bit)
    assert logits.shape == want.shape and np.abs(logits - want).max() <= LOGIT_TOL
    sure = g["branch_margin"] > float(g["margin"])
    assert sure.mean() >= 0.99
    pred = np.concatenate(out["point_predict"])
    assert np.array_equal(pred[sure], g["branch_point_predict"][sure])
    assert np.array_equal(np.concatenate(out["point_labels"]), g["branch_point_labels"])
    with pytest.raises(UnboundLocalError):                         # reproduced: cylinder_ts.py:576-586 binds the logits on one branch only
        with torch.no_grad():
            model.forward_ensemble(_batch(g))


def test_two_training_steps_from_one_state_give_the_same_bits(g):
    runs = []
    for _ in range(2):
        model = _model(g)
        ret, tb, _, got, grads = _step(model, g)
        runs.append((ret["loss"].detach().clone(), got["logits"], got["point_logits"], grads,
                     {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]), [k for k in a[3] if not torch.equal(a[3][k], b[3][k])]
    assert all(torch.equal(a[4][k], b[4][k]) for k in a[4])


def test_sync_batch_norm_modules_run_the_same_kernels_in_one_process(g):
    """IF_DIST True builds SyncBatchNorm modules; without a process group they take the local-statistics kernels: same bits"""
    plain = _step(_model(g), g)
    dist = _step(_model(g, if_dist=True), g)
    assert torch.equal(plain[3]["logits"], dist[3]["logits"]) and torch.equal(plain[0]["loss"], dist[0]["loss"])


def _float64_logits(g, round_half, monkeypatch):
    """Voxel logits of the training-mode forward in float64: the model in double on tensor ops - Linear / BatchNorm modules in double,
    the convolutions as per-offset matmul + index_add_ over the model's own kernel maps, the gate, the maximum and the row gather in
    their tensor-op forms.  round_half: every tensor the autocast run STORES in half is rounded to half on the way (and carried on in
    float64) - the outputs of every Linear, BatchNorm, convolution, leaky_bn / bn_act, the gate and the skip sums, and the weights
    the half kernels and autocast's matmuls cast (Linear; convolutions with both channel counts multiples of 32)."""
    import taseg_amd.torchsparse.nn as spnn
    from taseg_amd.torchsparse.nn import functional as F
    from taseg_amd.torchsparse.utils import make_ntuple
    q = (lambda t: t.half().double()) if round_half else (lambda t: t)
    model = _model(g).double().train()

    def conv64(self, x):
        kmap, out_coords, out_stride = F.conv_geometry(x, self.kernel_size, self.stride, make_ntuple(self.dilation, ndim=3), self.transposed)
        n_in, n_out = kmap.sizes
        half_kernel = self.in_channels % 32 == 0 and self.out_channels % 32 == 0
        w = q(self.kernel) if half_kernel else self.kernel
        feats = q(x.F)                                             # (a skip sum in front of the convolution is stored in half)
        out = torch.zeros((n_in if self.transposed else n_out, self.out_channels), dtype=torch.float64, device=feats.device)
        pairs, off = kmap.nbmaps, 0
        for k, size in enumerate(kmap.nbsizes.tolist()):
            p = pairs[off:off + size]
            src, dst = (p[:, 1], p[:, 0]) if self.transposed else (p[:, 0], p[:, 1])
            out.index_add_(0, dst, feats[src] @ w[k])
            off += size
        if self.bias is not None:
            out = out + self.bias
        return F._conv_output(x, q(out), out_coords, out_stride)

    def rounded(fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            out.F = q(out.F)
            return out
        return wrapped

    monkeypatch.setattr(spnn.Conv3d, "forward", conv64)
    monkeypatch.setattr(spnn, "leaky_bn", rounded(spnn.leaky_bn))          # (double rows: the tensor-op forms of both)
    monkeypatch.setattr(spnn, "bn_act", rounded(spnn.bn_act))
    gate = F.sigmoid3_gate
    monkeypatch.setattr(F, "sigmoid3_gate", lambda *a: q(gate(*a)))
    hooks = []
    for seq in (model.PPmodel, model.fea_compression, model.change_dim, model.point_logits):
        for m in seq.modules():
            if m is model.PPmodel[0]:
                continue                                           # (float rows in, float rows out: autocast leaves batch_norm's dtype alone)
            if isinstance(m, (torch.nn.Linear, torch.nn.modules.batchnorm._BatchNorm)):
                hooks.append(m.register_forward_hook(lambda mod, i, o: q(o)))
                if isinstance(m, torch.nn.Linear) and round_half:
                    with torch.no_grad():
                        m.weight.copy_(q(m.weight))
    got = {}
    hooks.append(model.logits.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.F.detach())))
    bd = _batch(g)
    bd["point_feature"] = bd["point_feature"].double()
    with torch.no_grad():
        model(bd)
    for h in hooks:
        h.remove()
    monkeypatch.undo()
    return got["logits"]


def test_autocast_runs_and_stays_close_to_fp32(g, monkeypatch):
    """Bar.  4e-2 proved tighter than half storage allows on this fixture (training-mode logits reach 8.6; the autocast run sat at
    4.8e-2): as the issue provides for that case, the bar is 4 x the distance a float64 evaluation moves when every tensor the
    autocast run stores in half is rounded to half (`_float64_logits`) - the format's own error on this network and batch, measured
    without the code under test; printed, and kept in profiles/cylinder_float64.txt."""
    fp32 = _step(_model(g), g)
    amp = _step(_model(g), g, amp=True)
    exact = _float64_logits(g, False, monkeypatch)
    assert float((fp32[3]["logits"].double() - exact).abs().max()) <= LOGIT_TOL       # the float64 evaluation is this network
    half64 = float((_float64_logits(g, True, monkeypatch) - exact).abs().max())
    d = float((fp32[3]["logits"] - amp[3]["logits"]).abs().max())
    dp = float((fp32[3]["point_logits"] - amp[3]["point_logits"]).abs().max())
    print(f"autocast: max |voxel logits - fp32| {d:.3e} (logits up to {float(fp32[3]['logits'].abs().max()):.2f}), point logits {dp:.3e}; "
          f"half-rounded float64 evaluation moves {half64:.3e}: bar {4 * half64:.3e}")
    assert d <= 4.0 * half64
    assert all(p is not None and bool(torch.isfinite(p).all()) for p in amp[4].values())
