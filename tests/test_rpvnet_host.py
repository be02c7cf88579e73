"""RPVNet on the host.  The plan restatement (tests/rpvnet_ref.py) gives the pixels of the reference's tensor expression bit for bit and
corners / weights that reproduce F.grid_sample; the stand-in `denselize` of the golden maker equals `spvoxelize_mean`'s host branch;
the state_dict is the reference's (tests/golden/model_rpvnet.npz, made by tests/golden/make_golden_rpvnet.py from the REAL reference)
for both blocks; the reference's import path binds after install_as_dropin; the registry still refuses the name; the range-stage
restatement equals the reference fixture (tests/golden/range_stage.npz) outside the rows its own bound leaves undecided.
tests/test_gpu_rpvnet_*.py and tests/test_gpu_range_stage.py compare the HIP path with the same files and restatements."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import rpvnet_ref as R
from taseg_amd import _lib
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg
from taseg_amd.pcseg.model.segmentor.fusion.rpvnet import RPVNet, SalsaNext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, IF_DIST=True, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
NEW_ENTRY_POINTS = (("ts_range_plan", 10), ("ts_range_point_tail_forward", 19), ("ts_range_inputs", 13))
SIZES = [(64, 2048), (16, 512), (4, 128)]


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_rpvnet.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def stage():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "range_stage.npz"), allow_pickle=False))


# ---------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restated_pixels_equal_the_tensor_expression(hw):
    """rpvnet.py:88 as the reference writes it, on every column and ring the dataset produces"""
    h, w = hw
    pxpy, xs, ys = R.kitti_pxpy()
    t = torch.from_numpy(pxpy)
    want = torch.cat([t[:, :1], (t[:, 1:] + 1) / 2 * torch.Tensor([w - 1, h - 1])], 1).int().numpy()
    x, y = R.pixels32(pxpy, h, w)
    assert np.array_equal(x, want[:, 1]) and np.array_equal(y, want[:, 2])
    pix, _, _, err = R.plan32(pxpy, 1, h, w)
    assert err == 0 and np.array_equal(pix, y * w + x)
    if hw == (64, 2048):
        # truncation, not rounding: these columns and rings land one pixel below their own index - reproduced, not repaired
        assert int((x[:2048] < xs).sum()) == 319 and int((y[2048:] < ys).sum()) == 23
        assert not (x[:2048] > xs).any() and ((xs - x[:2048]) <= 1).all()
    else:
        per_pixel = np.bincount(x[:2048], minlength=w)
        assert per_pixel.min() == 1 and per_pixel.max() == {512: 5, 128: 17}[w]


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (4, 128), (64, 2048)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restated_corners_reproduce_grid_sample(hw):
    """out = sum_k bw[k] f[bidx[k]] with the restated float32 corners against F.grid_sample(bilinear, zeros, align_corners=False) as
    the reference calls it, per sample; both are float32 evaluations of one continuous interpolant: each within bar_grid_value"""
    h, w = hw
    b, c, n = 2, 3, 400
    pxpy = np.concatenate([R.random_pxpy(n, b, 3), R.kitti_pxpy()[0][::37]])
    pxpy = np.ascontiguousarray(pxpy[np.argsort(pxpy[:, 0], kind="stable")])
    fm = np.random.RandomState(4).randn(b, c, h, w).astype(np.float32)
    pix, bidx, bw, err = R.plan32(pxpy, b, h, w)
    assert err == 0
    rows = fm.transpose(0, 2, 3, 1).reshape(-1, c).astype(np.float64)
    live = bidx[:, :4] >= 0
    ours = (np.where(live[:, :, None], rows[np.clip(bidx[:, :4], 0, None)], 0.0) * bw[:, :4, None].astype(np.float64)).sum(1)
    theirs = []
    for s in range(b):
        grid = torch.from_numpy(pxpy[pxpy[:, 0] == s][:, 1:]).unsqueeze(0).unsqueeze(0)
        theirs.append(torch.nn.functional.grid_sample(torch.from_numpy(fm[s:s + 1]), grid, mode="bilinear", padding_mode="zeros",
                                                      align_corners=False)[0, :, 0].t())
    theirs = torch.cat(theirs).double().numpy()
    bar = 2 * R.bar_grid_value(np.abs(fm).max(), h, w)
    err = np.abs(ours - theirs)
    print(f"grid_sample {h}x{w}: worst err / bar {err.max() / bar:.3g}")
    assert (err <= bar).all()
    # and the exact weights: the float32 ones sum to 1 within the same coordinate error wherever all four corners are inside
    _, bw64 = R.bilinear64(pxpy, b, h, w)
    inside = live.all(1)
    assert np.abs(bw64[inside].sum(1) - 1).max() < 1e-12 if inside.any() else True
    assert np.abs(bw[inside, :4].astype(np.float64).sum(1) - 1).max() <= 4 * (R.coord_err(w) + R.coord_err(h)) if inside.any() else True


def test_host_plan_of_the_op_equals_the_restatement():
    from taseg_amd.torchsparse.nn import functional as F
    flagged = np.array([[3, 0, 0], [-1, 0, 0], [0.5, 0, 0], [0, np.nan, 0], [1, 0, np.inf], [0, 1.0000001, 0]], dtype=np.float32)
    pxpy = np.concatenate([R.random_pxpy(200, 3, 9), flagged])
    plan = F.range_plan(torch.from_numpy(pxpy), 3, 4, 128)
    pix, bidx, bw, err = R.plan32(pxpy, 3, 4, 128)
    assert np.array_equal(plan["pix"].numpy(), pix) and np.array_equal(plan["bidx"].numpy(), bidx)
    assert np.array_equal(plan["bw"].numpy().view(np.uint32), bw.view(np.uint32)) and int(plan["range_err"]) == err == 7


def test_stand_in_denselize_equals_the_host_mean():
    """the golden maker's stand-in for the reference's CUDA-only extension against functional.spvoxelize_mean's host branch"""
    text = open(os.path.join(ROOT, "tests", "golden", "make_golden_rpvnet.py")).read()
    ns = {"torch": torch}
    for name in ("map_count", "denselize"):              # the two functions alone: the maker's imports need the reference
        body = re.search(r"^def " + name + r"\(.*?(?=^\S)", text, flags=re.S | re.M).group(0)
        exec(body, ns)
    from taseg_amd.torchsparse.nn import functional as F
    b, h, w, c = 2, 4, 16, 5
    pxpy = R.random_pxpy(300, b, 21)
    x, y = R.pixels32(pxpy, h, w)
    ipxpy = torch.from_numpy(np.stack([pxpy[:, 0].astype(np.int32), x, y], 1))
    feat = torch.from_numpy(np.random.RandomState(2).randn(300, c)).requires_grad_()
    cm = ns["map_count"](ipxpy, b, h, w)
    theirs = ns["denselize"](feat, cm, ipxpy)
    plan = F.range_plan(torch.from_numpy(pxpy), b, h, w)
    feat2 = feat.detach().clone().requires_grad_()
    ours = F.point_to_range(feat2, plan, b, h, w)
    assert theirs.shape == ours.shape == (b, c, h, w) and (ours.detach() - theirs.detach()).abs().max() <= 1e-12
    assert np.array_equal(cm.numpy().reshape(-1), np.bincount(plan["pix"].numpy(), minlength=b * h * w))
    gout = torch.from_numpy(np.random.RandomState(3).randn(b, c, h, w))
    theirs.backward(gout)
    ours.backward(gout)
    assert (feat.grad - feat2.grad).abs().max() <= 1e-12


# --------------------------------------------------------------------------------------------------------------------- the model
def test_state_dict_and_parameters_equal_the_reference(g):
    assert repr(sorted(CFG.items())) == str(g["cfg"])
    model = fill_parameters(RPVNet(make_model_cfg("RPVNet", **CFG), 20), seed=int(g["param_seed"]))
    assert model.name == "rpvnet"
    sd = model.state_dict()
    assert list(sd.keys()) == g["state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["state_shapes"].tolist()
    assert [zlib.crc32(v.numpy().tobytes()) for v in sd.values()] == g["param_crc"].tolist()
    keys = list(sd.keys())
    assert keys.index("classifier.0.bias") + 1 == keys.index("point_transforms.0.0.weight")
    assert keys[-1] == "range_branch.up4.bn1.num_batches_tracked" and "range_branch.stem.0.conv1.weight" in keys
    assert len(model.point_transforms) == 4 and model.point_transforms[0][0].in_features == 4
    assert all(isinstance(t[1], torch.nn.SyncBatchNorm) for t in model.point_transforms)
    assert isinstance(model.range_branch, SalsaNext) and isinstance(model.range_branch.stem[0].bn1, torch.nn.SyncBatchNorm)
    assert not hasattr(model.range_branch, "classifier")


def test_bottleneck_and_local_batch_norm_variants(g):
    bott = RPVNet(make_model_cfg("RPVNet", **{**CFG, "BLOCK": "Bottleneck"}), 20).state_dict()
    assert list(bott.keys()) == g["bottleneck_state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in bott.values()] == g["bottleneck_state_shapes"].tolist()
    # the stated difference: with IF_DIST False the transforms are nn.BatchNorm1d under the same keys (the reference cannot run them)
    local = RPVNet(make_model_cfg("RPVNet", **{**CFG, "IF_DIST": False}), 20)
    assert list(local.state_dict().keys()) == g["state_keys"].tolist()
    assert all(type(t[1]) is torch.nn.BatchNorm1d for t in local.point_transforms)
    assert type(local.range_branch.stem[0].bn1) is torch.nn.BatchNorm2d


def test_defaults_are_the_reference_s():
    cfg = make_model_cfg("RPVNet", in_dim=4)
    for key in ("cr", "NUM_LAYER", "BLOCK", "PLANES"):
        cfg.pop(key, None)
    model = RPVNet(cfg, 20)
    assert model.num_layer == [2, 3, 4, 6, 2, 2, 2, 2] and model.block.expansion == 4                  # Bottleneck
    assert model.stem[0].kernel.shape[-1] == int(1.75 * 32) == model.range_branch.cs[0] and model.range_branch.cr == 1.75


def test_multi_scale_other_than_concat_builds_no_classifier():
    """reproduced (rpvnet.py:567-569, :706-716, :751-752)"""
    model = RPVNet(make_model_cfg("RPVNet", MULTI_SCALE="sum", **CFG), 20)
    assert not hasattr(model, "classifier") and not any(k.startswith("classifier") for k in model.state_dict())
    with pytest.raises(TypeError):
        model.forward_ensemble({})


def test_header_signatures_and_build_flags_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taseg_hip.h")).read(), flags=re.S)
    for name, n_args in NEW_ENTRY_POINTS:
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1).strip()
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    from taseg_amd.csrc import build
    for src in ("rpvnet.hip", "range_stage.hip", "spvcnn.hip"):
        assert src in build.SOURCES and "-ffp-contract=off" in build.EXTRA[src]
    assert any(d.endswith("point_tail.h") for d in build._deps())


def test_reference_import_path_binds_after_install_as_dropin():
    code = ("import taseg_amd; names = taseg_amd.install_as_dropin()\n"
            "from pcseg.model.segmentor.fusion.rpvnet import RPVNet\n"
            "from pcseg.model.segmentor.fusion.rpvnet.rpvnet import SalsaNext\n"
            "import taseg_amd.pcseg.model.segmentor.fusion.rpvnet as mine\n"
            "assert RPVNet is mine.RPVNet and names['pcseg.model.segmentor.fusion.rpvnet'] is mine\n"
            "print('RPVNET_DROPIN_OK')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RPVNET_DROPIN_OK" in r.stdout, r.stdout + r.stderr


def test_the_registry_still_refuses_the_name():
    """as SPVCNN: tests/test_cylinder_host.py pins `_OUT_OF_SCOPE` and the NotImplementedError; the class is reached by its module path"""
    from taseg_amd.pcseg.model import build_network, segmentor
    assert "RPVNet" in segmentor._OUT_OF_SCOPE and "RPVNet" not in segmentor.__all__
    with pytest.raises(NotImplementedError):
        build_network(make_model_cfg("RPVNet", **CFG), 20)


# --------------------------------------------------------------------------------------------------------------- the range stage
def test_range_stage_restatement_equals_the_reference_fixture(stage):
    """every integer and every image pixel, except at the rows whose float64 proj_x lies within delta of a half-integer (the
    reference's float32 arctan2 may err by 4 ulp of pi, which the chain's roundings carry to delta columns: rpvnet_ref.stage_delta)
    and at the pixels those rows touch in either version; at most 1 % of the rows may be left out"""
    h, w = (int(v) for v in stage["hw"])
    delta = R.stage_delta(w)
    print(f"delta = {delta:.4g} columns")
    assert delta == float(stage["delta"]) and delta < 1e-3
    pts, batch, cuts = stage["points"], stage["batch"], stage["cuts"]
    from taseg_amd.data.range import draw_range_cut
    assert np.array_equal(cuts, [draw_range_cut(np.random.RandomState(s)) for s in (5, 6)])
    px64 = R.proj_x64(pts, batch, cuts, w)
    assert np.array_equal(px64, stage["proj_x64"])
    near = np.abs(px64 - np.floor(px64) - 0.5) <= delta
    assert near.mean() <= 0.01
    ours = R.range_stage32(pts, batch, cuts, h, w)
    assert ours["err"] == 0
    keep = ~near
    assert np.array_equal(ours["col"][keep], stage["col"][keep]) and np.array_equal(ours["row"], stage["row"])
    assert np.array_equal(ours["pxpy"][keep].view(np.uint32), stage["range_pxpy"][keep].view(np.uint32))
    assert np.array_equal(ours["pxpy"][:, [0, 2]], stage["range_pxpy"][:, [0, 2]])
    want = np.tile(np.array([-10, -10, 0, 0, 0], dtype=np.float32), (len(cuts) * h * w, 1))
    want[stage["image_at"]] = stage["image_values"]
    got = ours["image"].transpose(0, 2, 3, 1).reshape(-1, 5)
    skip = np.zeros(len(want), dtype=bool)
    base = batch[near].astype(np.int64) * h * w + stage["row"][near].astype(np.int64) * w
    skip[base + stage["col"][near]] = True
    skip[base + ours["col"][near]] = True
    assert np.array_equal(got[~skip].view(np.uint32), want[~skip].view(np.uint32))
    cells = batch.astype(np.int64) * h * w + stage["row"] * w + stage["col"]
    assert len(np.unique(cells)) < len(cells)                   # the fixture holds pixels with two rows: the later one wins
