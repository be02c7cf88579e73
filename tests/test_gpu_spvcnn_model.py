"""SPVCNN on the GPU (HIP kernels) against what the REAL reference produced for the same batch and parameters
(tests/golden/model_spvcnn.npz, tests/golden/make_golden_spvcnn.py), with the bars tests/test_gpu_model.py sets for MinkUNet against
its golden: logits within 1e-3, loss within 1e-3, the stored gradients within 2e-2 (BatchNorm in training mode) / 1e-4 (on running
statistics) of the reference's norm tensor by tensor, every parameter's gradient norm as there.  The fixture stores every
`logit_step`-th row of the per-voxel logits and `strided_sample`s of gradients above `full_below` elements; both are compared on the
same elements.

Index reuse: idx_query / counts taken from column 0 of the trilinear map equal the hash chain of minkunet/utils.py::point_to_voxel at
strides 16 and 4.  Evaluation branch: logits within 1e-3; `point_predict` equal at every point whose reference top-2 margin exceeds
2e-3 (the fixture leaves at most 1 % of the points out).  Two training steps from one state give the same bits for the loss and for
every parameter's gradient - what the float atomics of `spvoxelize` cannot give at stride 16.  Under autocast the model runs and its
logits stay within 4 x the distance that half storage moves a float64 evaluation (see the test).  `evaluate(on_device=True)` returns
the host path's matrix and payloads bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
LOGIT_TOL = 1e-3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_spvcnn.npz"), allow_pickle=False))


def _model(g, **kw):
    from taseg_amd.pcseg.model.segmentor.fusion.spvcnn import SPVCNN
    return fill_parameters(SPVCNN(make_model_cfg("SPVCNN", **CFG, **kw), 20), seed=int(g["param_seed"])).cuda()


def _batch(g):
    from taseg_amd.torchsparse import SparseTensor
    coords = torch.from_numpy(g["coords"]).cuda()
    pc = torch.zeros((len(g["point_batch"]), 4), dtype=torch.int32)
    pc[:, 3] = torch.from_numpy(g["point_batch"])
    pc = pc.cuda()
    return {"lidar": SparseTensor(torch.from_numpy(g["feats"]).cuda(), coords),
            "targets": SparseTensor(torch.from_numpy(g["labels"]).cuda(), coords),
            "inverse_map": SparseTensor(torch.from_numpy(g["inverse_map"]).cuda(), pc),
            "targets_mapped": SparseTensor(torch.from_numpy(g["point_labels"]).cuda(), pc),
            "num_points": torch.from_numpy(g["num_points"]), "offset": torch.tensor([0], device="cuda"), "name": g["name"].tolist()}


def _step(model, g, bn_training=True, amp=False):
    model.train()
    if not bn_training:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    got = {}
    hook = model.classifier.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().float()))
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        ret, tb, disp = model(_batch(g))
    hook.remove()
    model.zero_grad()
    ret["loss"].float().backward()
    return ret, tb, got["logits"], {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_vs_reference_golden(g, training):
    tag = "train" if training else "eval"
    model = _model(g)
    ret, tb, logits, grads = _step(model, g, training)
    logits = logits.cpu().numpy()[::int(g["logit_step"])]
    print(f"{tag}: max |logits - ref| {np.abs(logits - g[f'{tag}_logits']).max():.2e}, loss {float(tb['loss']):.6f} vs "
          f"{float(g[f'{tag}_loss']):.6f}")
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
    assert seen >= 10
    norms = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
    assert np.allclose(norms, g[f"{tag}_gradnorms"], rtol=5e-2 if training else 1e-3, atol=1e-6)


def test_point_to_voxel_index_from_the_trilinear_column_equals_the_hash_chain(g):
    from taseg_amd import backend as B
    from taseg_amd.pcseg.model.segmentor.fusion.spvcnn import utils as U
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet import utils as MU
    from taseg_amd.torchsparse import PointTensor, SparseTensor
    model = _model(g)
    plan = model.prepare(_batch(g))
    piece = B.voxelize_mean_piece_rows()
    assert int(g["piece_rows"]) == piece
    for s in (16, 4, 1):
        key = (s, s, s)
        vox = plan["cmaps"][key]
        x = SparseTensor(torch.zeros((vox.shape[0], 4), device="cuda"), vox, s)
        chain = PointTensor(torch.ones((plan["point_coords"].shape[0], 4), device="cuda"), plan["point_coords"])
        MU.point_to_voxel(x, chain)                                               # sphash + sphashquery + spcount
        want_idx, want_counts = chain.additional_features["idx_query"][key], chain.additional_features["counts"][key]
        idx, counts, groups = plan["p2v"][key]
        assert bool((want_idx >= 0).all()) and torch.equal(idx.long(), want_idx.long()) and torch.equal(counts.long(), want_counts.long())
        cached = PointTensor(chain.F, plan["point_coords"], idx_query=plan["tri_idx"], weights=plan["tri_w"])
        got = U.point_to_voxel_index(x, cached)                                   # the column of the cached trilinear map
        assert torch.equal(got[0].long(), want_idx.long()) and torch.equal(got[1].long(), want_counts.long())
        bare = U.point_to_voxel_index(x, PointTensor(chain.F, plan["point_coords"]))      # nothing cached: the hash chain
        assert torch.equal(bare[0].long(), want_idx.long()) and torch.equal(bare[2][0], groups[0])
        assert int(counts.max()) == int(g["most_rows"][{1: 0, 4: 1, 16: 2}[s]])
    assert int(plan["p2v"][(16, 16, 16)][1].max()) > piece                        # stride 16 cuts a voxel into pieces on this batch


def test_evaluation_branch(g):
    model = _model(g).eval()
    with torch.no_grad():
        out = model(_batch(g))
    assert set(out) == {"point_predict", "point_labels", "name", "point_predict_logits"} and out["name"] == g["name"].tolist()
    n_pts = g["num_points"].tolist()
    assert [len(p) for p in out["point_predict"]] == n_pts == [len(p) for p in out["point_labels"]]
    logits = np.concatenate(out["point_predict_logits"])
    per_scan = [int((g["coords"][:, 3] == b).sum()) for b in range(len(n_pts))]
    rows = g["inverse_map"] + np.concatenate([[0], np.cumsum(per_scan)])[g["point_batch"]]
    step = int(g["logit_step"])
    kept = rows % step == 0                                        # the points whose voxel row the fixture stores
    want = g["branch_logits"][rows[kept] // step]
    assert kept.sum() > len(rows) // (2 * step) and np.abs(logits[kept] - want).max() <= LOGIT_TOL
    sure = g["branch_margin"] > float(g["margin"])
    assert sure.mean() >= 0.99
    pred = np.concatenate(out["point_predict"])
    assert np.array_equal(pred[sure], g["branch_point_predict"][sure].astype(pred.dtype))
    assert np.array_equal(np.concatenate(out["point_labels"]), g["branch_point_labels"])
    with pytest.raises(TypeError):                                 # reproduced: spvcnn.py:483-484 passes ensemble=True
        with torch.no_grad():
            model.forward_ensemble(_batch(g))


def test_two_training_steps_from_one_state_give_the_same_bits(g):
    runs = []
    for _ in range(2):
        model = _model(g)
        ret, tb, logits, grads = _step(model, g)
        runs.append((ret["loss"].detach().clone(), logits, grads, {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def test_sync_batch_norm_modules_run_the_same_kernels_in_one_process(g):
    """IF_DIST True builds SyncBatchNorm modules; without a process group they take the local-statistics kernels: same bits"""
    plain = _step(_model(g), g)
    dist = _step(_model(g, if_dist=True), g)
    assert torch.equal(plain[2], dist[2]) and torch.equal(plain[0]["loss"], dist[0]["loss"])


class _Done(Exception):
    pass


def _float64_logits(g, round_half, monkeypatch):
    """Logits of the training-mode forward in float64: the model in double on tensor ops - Linear / BatchNorm modules in double, the
    convolutions as per-offset matmul + index_add_ over the model's own kernel maps, voxelisation and devoxelisation as index_add /
    gather.  round_half: every tensor the autocast run stores in half is rounded to half on the way (and carried on in float64) - the
    outputs of voxelisation, devoxelisation, every convolution block, every Linear and point tail - and the weights autocast and the
    half kernels cast (Linear; convolutions with both channel counts multiples of 32)."""
    import taseg_amd.torchsparse.nn as spnn
    from taseg_amd.torchsparse.nn import functional as F
    from taseg_amd.torchsparse.utils import make_ntuple
    q = (lambda t: t.half().double()) if round_half else (lambda t: t)
    model = _model(g).double().train()

    def conv64(self, x):
        if tuple(make_ntuple(self.kernel_size, ndim=3)) == (1, 1, 1):                # conv.py:135-140: a matmul over the rows
            dense = self.in_channels % 32 == 0 and self.out_channels % 32 == 0
            return x._like(x.F @ (q(self.kernel) if dense else self.kernel))
        kmap, out_coords, out_stride = F.conv_geometry(x, self.kernel_size, self.stride, make_ntuple(self.dilation, ndim=3), self.transposed)
        n_in, n_out = kmap.sizes
        w = q(self.kernel) if (self.in_channels % 32 == 0 and self.out_channels % 32 == 0) else self.kernel
        w = w.view(-1, self.in_channels, self.out_channels)
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
            if isinstance(out, tuple):                              # passthrough=True: (output, input')
                out[0].F = q(out[0].F)
            else:
                out.F = q(out.F)
            return out
        return wrapped

    def devox64(feats, idx, w, order=None):
        live = ((idx >= 0) & (w != 0)).double() * w.double()
        return q((feats[idx.clamp(min=0).long()] * live.unsqueeze(-1)).sum(1))

    mean64 = F.spvoxelize_mean                                      # (double rows: index_add of feat / cnt)
    bd = _batch(g)
    model.prepare(bd)                                               # the index plan: coordinates only, before anything is patched
    bd["lidar"].F = bd["lidar"].F.double()
    monkeypatch.setattr(spnn.Conv3d, "forward", conv64)
    monkeypatch.setattr(spnn, "conv_bn_act", rounded(spnn.conv_bn_act))
    monkeypatch.setattr(F, "spdevoxelize", devox64)
    monkeypatch.setattr(F, "spvoxelize", lambda f, i, c: q(mean64(f, i, c.shape[0])))
    monkeypatch.setattr(F, "spvoxelize_mean", lambda f, i, m, groups=None: q(mean64(f, i, m)))
    monkeypatch.setattr(F, "point_tail", lambda y, bn, vox, idx, w, order=None: q(devox64(vox, idx, w) + torch.relu(bn(q(y)))))
    if round_half:
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.Linear):
                    m.weight.copy_(q(m.weight))
    got = {}

    def grab(m, i, o):
        got["logits"] = o.detach()
        raise _Done

    hook = model.classifier.register_forward_hook(grab)
    with torch.no_grad(), pytest.raises(_Done):
        model(bd)
    hook.remove()
    monkeypatch.undo()
    return got["logits"]


def test_autocast_runs_and_stays_close_to_fp32(g, monkeypatch):
    """Bar, taken as tests/test_gpu_cylinder_model.py takes its own: 4 x the distance a float64 evaluation moves when every tensor the
    autocast run stores in half is rounded to half (`_float64_logits`) - the format's own error on this network and batch, measured
    without the code under test; printed, and kept in profiles/spvcnn_step.txt."""
    fp32 = _step(_model(g), g)
    amp = _step(_model(g), g, amp=True)
    assert bool(torch.isfinite(amp[0]["loss"]).all())
    exact = _float64_logits(g, False, monkeypatch)
    assert float((fp32[2].double() - exact).abs().max()) <= LOGIT_TOL              # the float64 evaluation is this network
    half64 = float((_float64_logits(g, True, monkeypatch) - exact).abs().max())
    d = float((fp32[2] - amp[2]).abs().max())
    print(f"autocast: max |logits - fp32| {d:.3e} (logits up to {float(fp32[2].abs().max()):.2f}); half-rounded float64 evaluation "
          f"moves {half64:.3e}: bar {4 * half64:.3e}")
    assert d <= 4.0 * half64
    assert all(p is not None and bool(torch.isfinite(p).all()) for p in amp[3].values())


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
        return {"lidar": SparseTensor(f, c), "inverse_map": SparseTensor(inv, pc), "targets_mapped": SparseTensor(lab, pc),
                "num_points": torch.tensor([p0, p0]), "name": ["scan/a/b.bin", "scan/a/b.bin"]}

    host = evaluate(model, [votes()], 20, tta_votes=2, prefetch=False)
    dev = evaluate(model, [votes()], 20, tta_votes=2, prefetch=False, on_device=True)
    assert len(host["predictions"]) == len(dev["predictions"]) == 1
    assert np.array_equal(host["predictions"][0], dev["predictions"][0])
