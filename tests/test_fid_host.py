"""The interpolation decoder's references (tests/fid_ref.py) and FIDNet / CENet without a GPU.

The restatement of csrc/fid.hip's rule is held to `F.interpolate(..., mode='bilinear', align_corners=True)` + `torch.cat` on the CPU: in
float32 it meets the derived bar (fid_ref.forward_bar) against the float64 evaluation, ATen's own float32 result meets the same bar,
and the number of elements where the two float32 results differ in bits is printed (ATen's CPU kernel evaluates the same interpolant
through precomputed weights in another order: equal bits are not expected of it).  The adjoint satisfies <upcat(x), g> = <x, upcat^T(g)>
in float64; the gather ranges taken from the tables reach every (fine index, corner) pair exactly once; the ordered float32 adjoint
meets its bar against float64.

Both models against what the REAL reference produced (tests/golden/model_fidnet.npz, model_cenet.npz): state_dict keys, order and shapes
for every stored configuration; on the CPU (the module fallbacks of `_bn_act` and `fid_upcat`, in the layout and at the thread count
the fixtures were made with) logits and losses within 1e-3, the
stored gradients within 2e-2 / 1e-4 of the reference's norms, every gradient norm, the evaluation branch's arg-max where the top-2
margin exceeds 2e-3.  The reference's module paths bind after install_as_dropin(); the registry still refuses both names."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as FR
from fid_models import build as _build, cfg as _cfg, check_against_golden, golden as _golden, head as _head, run_step, variant as _variant
from taseg_amd.data.synthetic import fill_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (T, H, W), the three levels: a level of one row; odd sizes and non-dyadic scales; out == 1 rows and a one-pixel level; the model's
SHAPES = [((2, 8, 16), ((4, 8), (2, 4), (1, 2))), ((1, 9, 13), ((5, 7), (3, 4), (2, 2))), ((1, 1, 7), ((1, 4), (1, 2), (1, 1))),
          ((1, 16, 64), ((8, 32), (4, 16), (2, 8)))]


def maps(shape, sizes, channels, seed, dtype=np.float32):
    (T, H, W), (ca, cb, cl) = shape, channels
    rs = np.random.RandomState(seed)
    x, x1 = rs.randn(T, H, W, ca).astype(dtype), rs.randn(T, H, W, cb).astype(dtype)
    return x, x1, [(rs.randn(T, h, w, cl) * 2 + 0.5).astype(dtype) for h, w in sizes]


def aten_chain(x, x1, coarse):
    nchw = lambda a: torch.from_numpy(a).permute(0, 3, 1, 2)  # noqa: E731
    res = [F.interpolate(nchw(v), size=x.shape[1:3], mode='bilinear', align_corners=True) for v in coarse]
    return torch.cat([nchw(x), nchw(x1), *res], dim=1).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape,sizes", SHAPES)
def test_restatement_and_aten_meet_the_bar_against_float64(shape, sizes):
    x, x1, coarse = maps(shape, sizes, (8, 4, 8), 5)
    cat32, _ = FR.upcat(x, x1, coarse, np.float32)
    cat64, _ = FR.upcat(x, x1, coarse, np.float64)
    aten64 = aten_chain(*(a.astype(np.float64) for a in (x, x1)), [v.astype(np.float64) for v in coarse])
    assert np.abs(cat64 - aten64).max() <= 1e-12                             # the float64 evaluation is ATen's interpolant
    aten32 = aten_chain(x, x1, coarse)
    bars = FR.forward_bar(coarse, shape[1], shape[2])
    assert np.array_equal(cat32[..., :12], np.concatenate([x, x1], axis=3))
    for k in range(3):
        sl = slice(12 + 8 * k, 20 + 8 * k)
        e_mine, e_aten = np.abs(cat32[..., sl] - cat64[..., sl]).max(), np.abs(aten32[..., sl] - cat64[..., sl]).max()
        differ = int((cat32[..., sl].view(np.uint32) != aten32[..., sl].view(np.uint32)).sum())
        print(f"{shape} level {sizes[k]}: restatement {e_mine:.2e}, ATen {e_aten:.2e}, bar {bars[k]:.2e}; {differ} of {cat32[..., sl].size} "
              "elements differ in bits between the two float32 results")
        assert e_mine <= bars[k] and e_aten <= bars[k]


@pytest.mark.parametrize("shape,sizes", SHAPES)
def test_adjoint_identity_and_ordered_sum(shape, sizes):
    channels = (8, 4, 8)
    x, x1, coarse = maps(shape, sizes, channels, 6, np.float64)
    rs = np.random.RandomState(7)
    g = rs.randn(*x.shape[:3], 12 + 24)
    gres = [rs.randn(*x.shape[:3], 8) for _ in range(3)]
    cat, res = FR.upcat(x, x1, coarse, np.float64)
    gx, gx1, gk = FR.upcat_adjoint(g, channels, sizes, gres, np.float64)
    lhs = (cat * g).sum() + sum((r * gr).sum() for r, gr in zip(res, gres))
    rhs = (x * gx).sum() + (x1 * gx1).sum() + sum((v * gv).sum() for v, gv in zip(coarse, gk))
    assert abs(lhs - rhs) <= 1e-10 * (np.abs(cat * g).sum() + 1)
    # autograd of the ATen chain in float64 agrees as well
    leaves = [torch.from_numpy(a).permute(0, 3, 1, 2).requires_grad_() for a in (x, x1, *coarse)]
    ups = [F.interpolate(v, size=x.shape[1:3], mode='bilinear', align_corners=True) for v in leaves[2:]]
    out = (torch.cat([leaves[0], leaves[1], *ups], 1) * torch.from_numpy(g).permute(0, 3, 1, 2)).sum()
    out = out + sum((u * torch.from_numpy(gr).permute(0, 3, 1, 2)).sum() for u, gr in zip(ups, gres))
    out.backward()
    for leaf, mine in zip(leaves, (gx, gx1, *gk)):
        assert np.abs(leaf.grad.permute(0, 2, 3, 1).numpy() - mine).max() <= 1e-11
    # the ordered float32 sum (fp32 lanes and half lanes: another S) within its bar
    g32, gres32 = g.astype(np.float32), [a.astype(np.float32) for a in gres]
    for lanes in (4, 8):
        _, _, gk32 = FR.upcat_adjoint(g32, channels, sizes, gres32, np.float32, lanes)
        _, _, gk64 = FR.upcat_adjoint(g32, channels, sizes, gres32, np.float64, lanes)
        for got, ref, bar in zip(gk32, gk64, FR.adjoint_bar(g32, channels, sizes, gres32, lanes)):
            assert got.dtype == np.float32 and (np.abs(got - ref) <= bar).all()
            print(f"{shape} lanes {lanes}: worst err / bar {float((np.abs(got - ref) / bar).max()):.3g}")


@pytest.mark.parametrize("fine,coarse", sorted({(o, i) for (_, H, W), sizes in SHAPES for h, w in sizes for o, i in ((H, h), (W, w))}))
def test_gather_ranges_cover_every_corner_exactly_once(fine, coarse):
    reached, every = FR.covered_pairs(fine, coarse)
    assert sorted(reached) == sorted(every) and len(set(reached)) == len(reached) == 2 * fine
    i0, lam, first = FR.tables(fine, coarse)
    assert first[0] == 0 and first[coarse] == fine and (np.diff(first) >= 0).all() and (lam >= 0).all() and (lam < 1).all()


# ---------------------------------------------------------------------------------------------------------------------- models

@pytest.mark.parametrize("name", ["fidnet", "cenet"])
def test_state_dict_keys_order_and_shapes(name):
    g = _golden(name)
    tags = [k.split("/", 1)[1] for k in g if k.startswith("keys/")]
    assert len(tags) == (4 if name == "fidnet" else 8)
    for tag in tags:
        parts = tag.split("_")
        kw = {"loss": parts[0], "if_bn": parts[1] == "bn1"}
        if name == "cenet":
            kw["IF_AUX"] = parts[2] == "aux1"
        sd = _build(name, **kw).state_dict()
        assert list(sd.keys()) == list(g[f"keys/{tag}"]), tag
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g[f"shapes/{tag}"]), tag
        assert ("WCE.weight" in sd) == (parts[0] == "wce")


@contextlib.contextmanager
def reference_conditions():
    """the conditions the fixtures were made under: the "nchw" layout (on the CPU "nhwc" sends ATen to its channels-last convolutions,
    which add in another order) and one thread (the sums of a convolution's gradient are cut by the thread count) - so that the step
    does not depend on what ran before it"""
    from taseg_amd.options import options
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with options.override(image_layout="nchw"):
            yield
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("name,variant", [("fidnet", "wce"), ("fidnet", "dice"), ("cenet", "aux"), ("cenet", "noaux")])
@pytest.mark.parametrize("tag", ["train", "eval"])
def test_model_on_the_cpu_vs_reference_golden(name, variant, tag):
    g = _golden(name)
    model = fill_parameters(_build(name, **_variant(name, variant)), seed=int(g["param_seed"]))
    with reference_conditions():
        ret, tb, logits, grads = run_step(model, _head(name, model), g, tag == "train")
    check_against_golden(g, variant, tag, model, tb, logits, grads)


@pytest.mark.parametrize("name,variant", [("fidnet", "wce"), ("cenet", "aux")])
def test_top_k_and_evaluation_branch(name, variant):
    g = _golden(name)
    model = fill_parameters(_build(name, top_k=0.5, **_variant(name, variant)), seed=int(g["param_seed"]))
    with reference_conditions():
        _, tb, _, _ = run_step(model, _head(name, model), g)
    assert abs(float(tb["loss"]) - float(g[f"{variant}_topk_train_loss"])) <= 1e-3
    model = fill_parameters(_build(name, **_variant(name, "dice" if name == "fidnet" else "aux")), seed=int(g["param_seed"])).eval()
    with torch.no_grad():
        out = model({"scan_rv": torch.from_numpy(g["scan_rv"]), "label_rv": torch.from_numpy(g["label_rv"].astype(np.int64))})
    assert set(out) == {"point_predict", "point_labels"} and out["point_labels"].shape == (2, 16, 64)
    sure = g["branch_margin"] > 2e-3
    assert sure.mean() >= 0.9                      # (FIDNet's evaluation logits stay below 0.6 on this batch: 96 % of the pixels)
    assert np.array_equal(out["point_predict"].argmax(1).numpy()[sure], g["branch_argmax"][sure])


def test_reproduced_quirks():
    from taseg_amd.pcseg.model.segmentor.base_segmentors import BaseSegmentor
    from taseg_amd.pcseg.model.segmentor.range.cenet.model.semantic.cenet import CENet
    from taseg_amd.pcseg.model.segmentor.range.fidnet.model.semantic.fidnet import FIDNet
    cfg = _cfg("FIDNet")
    cfg["IF_INTENSITY"] = False                      # with IF_RANGE True: none of the four stems
    model = FIDNet(cfg, 20)
    assert not hasattr(model.backend, "conv1") and not any(k.startswith("backend.conv1") for k in model.state_dict())
    with pytest.raises(AttributeError):
        model({"scan_rv": torch.zeros(1, 6, 8, 16), "label_rv": torch.zeros(1, 8, 16, dtype=torch.long)})
    cenet = CENet(_cfg("CENet", IF_AUX=False), 20)
    assert not isinstance(cenet, BaseSegmentor) and not hasattr(cenet, "name") and not hasattr(cenet, "aux_head1")
    assert isinstance(cenet.conv1.relu, torch.nn.LeakyReLU)


def test_reference_module_paths_bind_and_the_registry_refuses():
    code = ("import taseg_amd\nnames = taseg_amd.install_as_dropin()\n"
            "from pcseg.model.segmentor.range.fidnet.model.semantic.fidnet import FIDNet, BasicBlock, SemanticHead, Backbone\n"
            "from pcseg.model.segmentor.range.fidnet.model.semantic import FIDNet as again\n"
            "from pcseg.model.segmentor.range.cenet.model.semantic.cenet import CENet, BasicConv2d\n"
            "import taseg_amd.pcseg.model.segmentor.range.fidnet.model.semantic.fidnet as f\n"
            "import taseg_amd.pcseg.model.segmentor.range.cenet.model.semantic.cenet as c\n"
            "assert FIDNet is f.FIDNet is again and CENet is c.CENet\n"
            "assert names['pcseg.model.segmentor.range.fidnet.model.semantic.fidnet'] is f\n"
            "assert names['pcseg.model.segmentor.range.cenet.model.semantic.cenet'] is c\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)
    from taseg_amd.pcseg.model import build_network, segmentor
    for name in ("FIDNet", "CENet"):
        assert name in segmentor._OUT_OF_SCOPE and name not in segmentor.__all__
        with pytest.raises(NotImplementedError):
            build_network(_cfg(name, IF_AUX=True), 20)


def test_options_off_is_the_aten_chain():
    """on the CPU both settings of image_fid_upcat are the chain; the option exists, is typed, and the levels come out when asked for"""
    from taseg_amd.options import options
    from taseg_amd.pcseg.model.segmentor.range.functional import fid_upcat
    x, x1, coarse = maps((1, 9, 13), ((5, 7), (3, 4), (2, 2)), (8, 4, 8), 9)
    t = [torch.from_numpy(a).permute(0, 3, 1, 2) for a in (x, x1, *coarse)]
    want = torch.from_numpy(aten_chain(x, x1, coarse)).permute(0, 3, 1, 2)
    assert options.image_fid_upcat is True
    with pytest.raises(TypeError):
        options.image_fid_upcat = 2
    for on in (True, False):
        with options.override(image_fid_upcat=on):
            cat, res = fid_upcat(*t, levels=True)
            assert torch.equal(cat, want) and torch.equal(fid_upcat(*t), want)
            assert all(torch.equal(r, want[:, 12 + 8 * k: 20 + 8 * k]) for k, r in enumerate(res))
