"""What the FIDNet / CENet tests share (tests/test_fid_host.py on the CPU, tests/test_gpu_fidnet_model.py and
tests/test_gpu_cenet_model.py on the device): the fixtures, the stored configurations, one training step, and the comparison with the
REAL reference's results under the bars of tests/test_gpu_salsanext_model.py.  Not a test module."""
import os

import numpy as np
import torch

from taseg_amd.data.synthetic import make_model_cfg, strided_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", f"model_{name}.npz"), allow_pickle=False))


def cfg(name, loss="dice", top_k=1.0, if_bn=True, **kw):
    return make_model_cfg(name, IF_BN=if_bn, IF_INTENSITY=True, IF_RANGE=True, WITH_NORM=False, LOSS=loss, IF_LS_LOSS=True, IF_BD_LOSS=True,
                          TOP_K_PERCENT_PIXELS=top_k, **kw)


def build(name, **kw):
    from taseg_amd.pcseg.model.segmentor.range.cenet.model.semantic.cenet import CENet
    from taseg_amd.pcseg.model.segmentor.range.fidnet.model.semantic.fidnet import FIDNet
    return (FIDNet if name == "fidnet" else CENet)(cfg("FIDNet" if name == "fidnet" else "CENet", **kw), 20)


def variant(name, variant):
    """the build arguments of a stored run"""
    return {"loss": variant} if name == "fidnet" else {"IF_AUX": variant == "aux"}


def head(name, model):
    return model.semantic_head.semantic_output if name == "fidnet" else model.semantic_output


def run_step(model, head, g, bn_training=True, device="cpu", amp=False):
    model.train()
    for m in model.modules():
        if not bn_training and isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    got = {}
    hook = head.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().float()))
    batch = {"scan_rv": torch.from_numpy(g["scan_rv"]).to(device), "label_rv": torch.from_numpy(g["label_rv"].astype(np.int64)).to(device)}
    with torch.autocast(torch.device(device).type, dtype=torch.float16, enabled=amp):
        ret, tb, disp = model(batch)
    hook.remove()
    model.zero_grad()
    ret["loss"].float().backward()
    return ret, tb, got["logits"], {n: p.grad for n, p in model.named_parameters()}


def check_against_golden(g, variant, tag, model, tb, logits, grads, min_seen=15):
    """the bars of tests/test_gpu_salsanext_model.py: logits and loss 1e-3, stored gradients 2e-2 / 1e-4 of the reference's norm, every
    gradient norm (rtol 5e-2 / 1e-3, atol 1e-6).  A stored gradient or a norm that misses its bar is held to 4 x the distance the
    float32 reference ITSELF lies from the float64 evaluation of its own expression (the fixture's `dist64/<parameter>`, the worst of
    the run's stored tensors), and the test says so.  These trunks are LeakyReLU behind BatchNorm 34 layers deep: an element at a kink
    takes the other slope in another evaluation, which moves a gradient by a step, not by a rounding (FIDNet on running statistics:
    1.6e-4 at backend.conv2.weight).  The biases of the convolutions in front of a training-mode BatchNorm (`zero_in_training`) have a
    zero gradient in exact arithmetic: their norms are held to 1e-5 absolutely, the bound the fixture's generator asserts of the
    reference's own.  profiles/fidnet_float64.txt has the numbers."""
    training = tag == "train"
    rows = logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1])[::int(g["logit_step"])].cpu().numpy()
    print(f"{variant} {tag}: max |logits - ref| {np.abs(rows - g[f'{tag}_logits']).max():.2e} (logits up to {np.abs(rows).max():.1f}), loss "
          f"{float(tb['loss']):.6f} vs {float(g[f'{variant}_{tag}_loss']):.6f}")
    assert rows.shape == g[f"{tag}_logits"].shape and np.abs(rows - g[f"{tag}_logits"]).max() <= 1e-3
    assert abs(float(tb["loss"]) - float(g[f"{variant}_{tag}_loss"])) <= 1e-3
    tol = 2e-2 if training else 1e-4
    seen, worst_rel = 0, 0.0
    own = 4.0 * max(float(g[k]) for k in g if k.startswith(f"{variant}_{tag}_dist64/"))
    for k in g:
        if k.startswith(f"{variant}_{tag}_grad/"):
            a, b = grads[k.split("/", 1)[1]].detach().cpu(), g[k]
            a = (a if a.numel() <= int(g["full_below"]) else strided_sample(a)).numpy().reshape(b.shape)
            rel = np.linalg.norm(a - b) / np.linalg.norm(b)
            if rel > tol:                                  # (held by the reference's own distance instead, and said so)
                print(f"  {k}: {rel:.2e} is over {tol:g}; 4 x the reference's own distance from float64 is {own:.2e}")
            worst_rel = max(worst_rel, rel / (tol if rel <= tol else own))
            assert rel <= max(tol, own), (k, rel)
            seen += 1
    assert seen >= min_seen
    names = [n for n, _ in model.named_parameters()]
    norms = np.array([float(grads[n].norm()) for n in names])
    want = g[f"{variant}_{tag}_gradnorms"]
    rtol = 5e-2 if training else 1e-3
    allowed = 1e-6 + rtol * np.abs(want)
    zero = np.isin(names, g["zero_in_training"]) if training else np.zeros(len(names), dtype=bool)
    if zero.any():
        print(f"  zero-in-exact-arithmetic gradients: norms up to {norms[zero].max():.2e} (reference's up to {want[zero].max():.2e}), bar 1e-5")
    assert (norms[zero] <= 1e-5).all() and (want[zero] <= 1e-5).all(), [n for n, z, v in zip(names, zero, norms) if z and v > 1e-5]
    err = np.abs(norms - want)
    over = (err > allowed) & ~zero
    print(f"{variant} {tag}: {seen} stored gradients, worst |got - ref| / |ref| at {worst_rel:.3g} of its bar ({tol:g}, or 4 x the reference's "
          f"own distance from float64); worst gradient norm at {(err / allowed)[~zero].max():.3g} of its allowance")
    if over.any():                                         # (as for the stored gradients: the reference's own distance, and said so)
        print(f"  {int(over.sum())} gradient norms are over rtol {rtol:g}; 4 x the reference's own distance from float64 is {own:.2e}")
    assert (err[over] <= 1e-6 + max(rtol, own) * np.abs(want)[over]).all(), [n for n, o in zip(names, over) if o]


# ------------------------------------------------------------------------------------------------------------ on the device

def device_model(name, g, **kw):
    from taseg_amd.data.synthetic import fill_parameters
    return fill_parameters(build(name, **kw), seed=int(g["param_seed"])).cuda()


def logit_rows(logits, g):
    return logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1])[::int(g["logit_step"])].cpu().numpy()


def float64_logits(name, g, round_half):
    """Logits of the training-mode forward in float64 on the modules themselves (a double map takes neither kernel path).
    round_half: every tensor the autocast run stores in half - the output of every Conv2d and BatchNorm2d and of the three
    interpolations - is rounded to half on the way, and the weights and biases autocast casts (Conv2d)."""
    import taseg_amd.pcseg.model.segmentor.range.functional as RF
    q = (lambda t: t.half().double()) if round_half else (lambda t: t)
    model = device_model(name, g, **variant(name, "dice" if name == "fidnet" else "aux")).double().train()
    hooks = [m.register_forward_hook(lambda m, i, o: q(o)) for m in model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d))]
    if round_half:
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.copy_(q(m.weight))
                    if m.bias is not None:
                        m.bias.copy_(q(m.bias))
    plain = RF.F.interpolate
    RF.F = type("F", (), {"interpolate": staticmethod(lambda *a, **k: q(plain(*a, **k)))})
    try:
        with torch.no_grad():
            logits = model.forward_logits(torch.from_numpy(g["scan_rv"]).cuda().double())
    finally:
        RF.F = torch.nn.functional
        for h in hooks:
            h.remove()
    return logits


def check_model_vs_golden(name, var, tag, kernels):
    """one step on the device against the fixture, through the kernel paths or the chain (both options off)"""
    from taseg_amd.options import options
    g = golden(name)
    model = device_model(name, g, **variant(name, var))
    from taseg_amd import backend as B
    calls = {"fid_upcat_rows_forward": 0, "fid_upcat_rows_backward": 0, "bn_leaky_act_train_forward": 0, "bn_leaky_act_train_backward": 0}
    plain = {k: getattr(B, k) for k in calls}

    def counted(k):
        def fn(*a, **kw):
            calls[k] += 1
            return plain[k](*a, **kw)
        return fn

    for k in calls:
        setattr(B, k, counted(k))
    try:
        with options.override(image_fid_upcat=kernels, image_fused_bn=kernels):
            ret, tb, logits, grads = run_step(model, head(name, model), g, tag == "train", device="cuda")
    finally:
        for k in calls:
            setattr(B, k, plain[k])
    # no quiet fall-back: one decoder call per direction; every BatchNorm in front of a LeakyReLU through the node in training mode
    # (the maps of the 1/8 level included: 2 x 8 pixels), none of either through the chain
    fused = sum(isinstance(m, torch.nn.BatchNorm2d) for n, m in model.named_modules() if "downsample" not in n)
    want = {"fid_upcat_rows_forward": 1, "fid_upcat_rows_backward": 1, "bn_leaky_act_train_forward": fused if tag == "train" else 0,
            "bn_leaky_act_train_backward": fused if tag == "train" else 0}
    assert calls == (want if kernels else dict.fromkeys(calls, 0)), calls
    check_against_golden(g, var, tag, model, tb, logits, grads)


def check_top_k_and_evaluation_branch(name, var):
    g = golden(name)
    model = device_model(name, g, top_k=0.5, **variant(name, var))
    _, tb, _, _ = run_step(model, head(name, model), g, device="cuda")
    assert abs(float(tb["loss"]) - float(g[f"{var}_topk_train_loss"])) <= 1e-3
    model = device_model(name, g, **variant(name, "dice" if name == "fidnet" else "aux")).eval()
    with torch.no_grad():
        out = model({"scan_rv": torch.from_numpy(g["scan_rv"]).cuda(), "label_rv": torch.from_numpy(g["label_rv"].astype(np.int64)).cuda()})
    assert set(out) == {"point_predict", "point_labels"} and out["point_labels"].shape == (2, 16, 64)
    rows = logit_rows(out["point_predict"].float(), g)
    print(f"evaluation branch: max |logits - ref| {np.abs(rows - g['eval_logits']).max():.2e}")
    assert np.abs(rows - g["eval_logits"]).max() <= 1e-3
    sure = g["branch_margin"] > 2e-3
    assert sure.mean() >= 0.9
    assert np.array_equal(out["point_predict"].argmax(1).cpu().numpy()[sure], g["branch_argmax"][sure])


def check_two_steps_give_the_same_bits(name, var, monkeypatch):
    """the library's dense convolutions (MIOpen behind nn.Conv2d) kept to deterministic solvers by PyTorch's own switch; the kernel
    paths on: the decoder's adjoint is a gather in a fixed order, where ATen's adds with float atomics"""
    from taseg_amd.options import options
    assert options.image_fid_upcat and options.image_fused_bn
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    g = golden(name)
    runs = []
    for _ in range(2):
        model = device_model(name, g, **variant(name, var))
        ret, tb, logits, grads = run_step(model, head(name, model), g, device="cuda")
        runs.append((ret["loss"].detach().clone(), logits, grads, {k: v.clone() for k, v in model.state_dict().items() if "running" in k}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def check_autocast(name):
    """Bar, taken as tests/test_gpu_salsanext_model.py takes its own: 4 x the distance a float64 evaluation moves when every tensor the
    autocast run stores in half is rounded to half - the format's own error on this network and batch, measured without the code under
    test; printed, and kept in profiles/fidnet_float64.txt."""
    g = golden(name)
    var = "dice" if name == "fidnet" else "aux"
    model = device_model(name, g, **variant(name, var))
    fp32 = run_step(model, head(name, model), g, device="cuda")
    model = device_model(name, g, **variant(name, var))
    amp = run_step(model, head(name, model), g, device="cuda", amp=True)
    assert bool(torch.isfinite(amp[0]["loss"]).all())
    exact = float64_logits(name, g, False)
    print(f"fp32 logits vs the float64 evaluation: {float((fp32[2].double() - exact).abs().max()):.3e}")
    assert float((fp32[2].double() - exact).abs().max()) <= 1e-3                   # the float64 evaluation is this network
    half64 = float((float64_logits(name, g, True) - exact).abs().max())
    d = float((fp32[2] - amp[2]).abs().max())
    print(f"autocast: max |logits - fp32| {d:.3e} (logits up to {float(fp32[2].abs().max()):.2f}); half-rounded float64 evaluation "
          f"moves {half64:.3e}: bar {4 * half64:.3e}; loss {float(amp[1]['loss']):.6f} vs fp32 {float(fp32[1]['loss']):.6f}")
    assert d <= 4.0 * half64
    assert all(p is not None and bool(torch.isfinite(p).all()) for p in amp[3].values())


def check_evaluate_range_view_pixels(name):
    """`evaluate_range_view` in "pixels" mode equals the same loop done with host-side numpy on the model's outputs"""
    import range_view_ref as R
    from taseg_amd.data.range_view import build_range_view_batch
    from taseg_amd.pcseg.eval import fast_hist_crop
    from taseg_amd.pcseg.range_eval import evaluate_range_view
    g = golden(name)
    model = device_model(name, g, **variant(name, "dice" if name == "fidnet" else "aux")).eval()
    batches = []
    for seeds, lens in (((61, 62), (1500, 1200)), ((63,), (1700,))):
        scans = [{"points": torch.from_numpy(R.synth_cloud(s, n, far=30.0)).cuda(),
                  "labels": torch.from_numpy(np.random.RandomState(s).randint(0, 20, n).astype(np.int32)).cuda(),
                  "name": "data/sequences/08/velodyne/%06d.bin" % s} for s, n in zip(seeds, lens)]
        batches.append(build_range_view_batch(scans, (32, 64)))
    got = evaluate_range_view(model, batches, 20)
    hist = np.zeros((19, 19), dtype=np.int64)
    for batch in batches:
        with torch.no_grad():
            ret = model(batch)
        hist += fast_hist_crop(ret["point_predict"].argmax(1).cpu().numpy(), ret["point_labels"].cpu().numpy(), np.arange(19))
    assert np.array_equal(got["hist"], hist) and hist.sum() > 0 and got["err"] == 0
