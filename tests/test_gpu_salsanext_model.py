"""SalsaNext on the GPU against what the REAL reference produced for the same batch and parameters (tests/golden/model_salsanext.npz,
tests/golden/make_golden_salsanext.py), with the bars the project holds RPVNet's range branch to (tests/test_gpu_rpvnet_model.py):
logits within 1e-3, loss within 1e-3, the stored gradients within 2e-2 (BatchNorm in training mode) / 1e-4 (on running statistics) of
the reference's norm tensor by tensor, every parameter's gradient norm as there; profiles/salsanext_float64.txt keeps the measured
distances.  Both LOSS settings; the Dropout2d modules in eval mode on both sides.

Evaluation branch: the arg-max equal at every pixel whose reference top-2 margin exceeds 2e-3.  Two training steps from one state
give the same bits once torch.backends.cudnn.deterministic keeps the library's own convolutions to deterministic solvers.  Under
autocast the logits stay within 4 x the distance that half storage moves a float64 evaluation of the same model.
`evaluate_range_view` returns the matrices and payload bytes of the same loop done with host-side numpy on the model's outputs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import range_view_ref as R  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_salsanext.npz"), allow_pickle=False))


def _model(g, loss="dice", top_k=1.0):
    from taseg_amd.pcseg.model.segmentor.range.salsanext.model.semantic.salsanext import SalsaNext
    cfg = make_model_cfg("SalsaNext", LOSS=loss, IF_LS_LOSS=True, IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=top_k)
    return fill_parameters(SalsaNext(cfg, 20), seed=int(g["param_seed"])).cuda()


def _batch(g):
    return {"scan_rv": torch.from_numpy(g["scan_rv"]).cuda(), "label_rv": torch.from_numpy(g["label_rv"].astype(np.int64)).cuda()}


def _modes(model, bn_training=True):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d) or (not bn_training and isinstance(m, torch.nn.modules.batchnorm._BatchNorm)):
            m.eval()
    return model


def _step(model, g, bn_training=True, amp=False):
    _modes(model, bn_training)
    got = {}
    hook = model.logits.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().float()))
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        ret, tb, disp = model(_batch(g))
    hook.remove()
    model.zero_grad()
    ret["loss"].float().backward()
    return ret, tb, got["logits"], {n: p.grad for n, p in model.named_parameters()}


def _rows(logits, g):
    return logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1])[::int(g["logit_step"])].cpu().numpy()


@pytest.mark.parametrize("loss", ["wce", "dice"])
@pytest.mark.parametrize("tag", ["train", "eval"])
def test_model_vs_reference_golden(g, loss, tag):
    training = tag == "train"
    model = _model(g, loss)
    ret, tb, logits, grads = _step(model, g, training)
    rows = _rows(logits, g)
    print(f"{loss} {tag}: max |logits - ref| {np.abs(rows - g[f'{tag}_logits']).max():.2e} (logits up to {np.abs(rows).max():.1f}), loss "
          f"{float(tb['loss']):.6f} vs {float(g[f'{loss}_{tag}_loss']):.6f}")
    assert rows.shape == g[f"{tag}_logits"].shape and np.abs(rows - g[f"{tag}_logits"]).max() <= LOGIT_TOL
    assert abs(float(tb["loss"]) - float(g[f"{loss}_{tag}_loss"])) <= 1e-3
    tol = 2e-2 if training else 1e-4
    seen, worst_rel = 0, 0.0
    for k in g:
        if k.startswith(f"{loss}_{tag}_grad/"):
            a, b = grads[k.split("/", 1)[1]].detach().cpu(), g[k]
            a = (a if a.numel() <= int(g["full_below"]) else strided_sample(a)).numpy().reshape(b.shape)
            rel = np.linalg.norm(a - b) / np.linalg.norm(b)
            worst_rel = max(worst_rel, rel)
            assert rel <= tol, (k, rel)
            seen += 1
    assert seen >= 15
    norms = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
    want = g[f"{loss}_{tag}_gradnorms"]
    worst = np.abs(norms - want) / (1e-6 + (5e-2 if training else 1e-3) * np.abs(want))
    print(f"{loss} {tag}: {seen} stored gradients, worst |got - ref| / |ref| {worst_rel:.2e} (bar {tol:g}); worst gradient norm at "
          f"{worst.max():.3g} of its allowance")
    assert np.allclose(norms, want, rtol=5e-2 if training else 1e-3, atol=1e-6)


def test_top_k_percent_pixels(g):
    ret, tb, _, _ = _step(_model(g, "wce", top_k=0.5), g)
    assert abs(float(tb["loss"]) - float(g["wce_topk_train_loss"])) <= 1e-3


def test_evaluation_branch(g):
    model = _model(g).eval()
    with torch.no_grad():
        out = model(_batch(g))
    assert set(out) == {"point_predict", "point_labels"} and out["point_labels"].shape == (2, 32, 64)
    rows = _rows(out["point_predict"].float(), g)
    print(f"evaluation branch: max |logits - ref| {np.abs(rows - g['eval_logits']).max():.2e}")
    assert np.abs(rows - g["eval_logits"]).max() <= LOGIT_TOL
    sure = g["branch_margin"] > 2e-3
    assert sure.mean() >= 0.99
    assert np.array_equal(out["point_predict"].argmax(1).cpu().numpy()[sure], g["branch_argmax"][sure])


def test_two_training_steps_from_one_state_give_the_same_bits(g, monkeypatch):
    """as for RPVNet: the library's dense convolutions (MIOpen behind nn.Conv2d) kept to deterministic solvers by PyTorch's own switch;
    everything this project computes - the row kernels, the Lovasz kernels - is run-to-run identical"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    runs = []
    for _ in range(2):
        model = _model(g)
        ret, tb, logits, grads = _step(model, g)
        runs.append((ret["loss"].detach().clone(), logits, grads, {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def _float64_logits(g, round_half):
    """Logits of the training-mode forward in float64 on the modules themselves (no helper of unet2d.py takes a double map).
    round_half: every tensor the autocast run stores in half - the output of every Conv2d, BatchNorm2d and AvgPool2d - is rounded to
    half on the way, and the weights and biases autocast casts (Conv2d)."""
    q = (lambda t: t.half().double()) if round_half else (lambda t: t)
    model = _modes(_model(g).double())
    hooks = [m.register_forward_hook(lambda m, i, o: q(o)) for m in model.modules()
             if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.AvgPool2d))]
    if round_half:
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.copy_(q(m.weight))
                    m.bias.copy_(q(m.bias))
    with torch.no_grad():
        logits = model.forward_logits(torch.from_numpy(g["scan_rv"]).cuda().double())
    for h in hooks:
        h.remove()
    return logits


def test_autocast_runs_and_stays_close_to_fp32(g):
    """Bar, taken as tests/test_gpu_rpvnet_model.py takes its own: 4 x the distance a float64 evaluation moves when every tensor the
    autocast run stores in half is rounded to half - the format's own error on this network and batch, measured without the code under
    test; printed, and kept in profiles/salsanext_float64.txt."""
    fp32 = _step(_model(g), g)
    amp = _step(_model(g), g, amp=True)
    assert bool(torch.isfinite(amp[0]["loss"]).all())
    exact = _float64_logits(g, False)
    print(f"fp32 logits vs the float64 evaluation: {float((fp32[2].double() - exact).abs().max()):.3e}")
    assert float((fp32[2].double() - exact).abs().max()) <= LOGIT_TOL              # the float64 evaluation is this network
    half64 = float((_float64_logits(g, True) - exact).abs().max())
    d = float((fp32[2] - amp[2]).abs().max())
    print(f"autocast: max |logits - fp32| {d:.3e} (logits up to {float(fp32[2].abs().max()):.2f}); half-rounded float64 evaluation "
          f"moves {half64:.3e}: bar {4 * half64:.3e}; loss {float(amp[1]['loss']):.6f} vs fp32 {float(fp32[1]['loss']):.6f}")
    assert d <= 4.0 * half64
    assert all(p is not None and bool(torch.isfinite(p).all()) for p in amp[3].values())


def _eval_batches():
    from taseg_amd.data.range_view import build_range_view_batch
    out = []
    for seeds, lens in (((61, 62), (1500, 1200)), ((63,), (1700,))):
        scans = []
        for s, n in zip(seeds, lens):
            scans.append({"points": torch.from_numpy(R.synth_cloud(s, n, far=30.0)).cuda(),
                          "labels": torch.from_numpy(np.random.RandomState(s).randint(0, 20, n).astype(np.int32)).cuda(),
                          "name": "data/sequences/08/velodyne/%06d.bin" % s})
        out.append(build_range_view_batch(scans, (32, 64)))
    return out


@pytest.mark.parametrize("mode", ["pixels", "knn", "payloads"])
def test_evaluate_range_view_equals_the_host_loop(g, mode, tmp_path):
    from taseg_amd.data.range_view import knn_weight
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg.eval import _class_payload, fast_hist_crop, remap_labels, remap_lut
    from taseg_amd.pcseg.range_eval import evaluate_range_view
    model = _model(g).eval()
    batches = _eval_batches()
    params = dict(knn=5, search=5, sigma=1.0, cutoff=1.0)
    if mode == "pixels":
        got = evaluate_range_view(model, batches, 20)
    elif mode == "knn":
        got = evaluate_range_view(model, batches, 20, knn=params)
    else:
        got = evaluate_range_view(model, batches, 20, knn=params, predictions=True, remap=LEARNING_MAP_INV, save_dir=str(tmp_path))
    # the same loop with host-side numpy on the model's outputs
    hist, payloads = np.zeros((19, 19), dtype=np.int64), []
    for batch in batches:
        with torch.no_grad():
            ret = model(batch)
        classes = ret["point_predict"].argmax(1).cpu().numpy()
        if mode == "pixels":
            hist += fast_hist_crop(classes, ret["point_labels"].cpu().numpy(), np.arange(19))
            continue
        labels, err, _ = R.knn32(batch["proj_range"].cpu().numpy(), classes, batch["unproj_range"].cpu().numpy(), batch["proj_x"].cpu().numpy(),
                                 batch["proj_y"].cpu().numpy(), batch["batch"].cpu().numpy(), knn_weight(5, 1.0).numpy(), 5, 5, 1.0, 20)
        assert err == 0
        hist += fast_hist_crop(labels, batch["point_labels"].cpu().numpy(), np.arange(19))
        offset = batch["offset"].numpy()
        for k in range(len(offset) - 1):
            payloads.append(remap_labels(_class_payload(labels[offset[k]:offset[k + 1]], "semantickitti"), remap_lut(LEARNING_MAP_INV))
                            .reshape(-1, 1).astype(np.uint32))
    assert np.array_equal(got["hist"], hist) and hist.sum() > 0 and got["err"] == 0
    if mode == "payloads":
        assert len(got["predictions"]) == len(payloads) == 3
        for a, b, seed in zip(got["predictions"], payloads, (61, 62, 63)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
            path = os.path.join(str(tmp_path), "sequences", "08", "predictions", "%06d.label" % seed)
            assert open(path, "rb").read() == b.tobytes()
    with pytest.raises(ValueError):
        evaluate_range_view(model, batches, 20, predictions=True)
