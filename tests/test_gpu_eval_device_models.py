"""Evaluation on the device for the TIAF and KD segmentors, and label export from validation batches (-m gpu): the `defer` and
`device_tail` keywords of MinkUNetMsMm / MinkUNetMsMmNus / MinkUNetMsKd, the replace ensemble through one row index,
pcseg.eval.evaluate(predictions=True, remap=...) on both paths.

Every comparison is exact, as in tests/test_gpu_eval_device.py: both paths run the same forward pass on the same batch, integers
are integers, and the float32 vote sums are formed in one fixed order.  The batches are the smallest the stages' own tests use
(tests/golden/tiaf_data.npz, tiaf_nus.npz, multiscan.npz + kd_stage.npz): two scans of 1500 / 700 points per batch, so scene
boundaries fall inside a wave, and a `point_mask` that drops the history rows."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from taseg_amd.data.synthetic import TIAF_CFG, fill_parameters, make_model_cfg  # noqa: E402
from test_gpu_tiaf_nus_aug import g, inputs  # noqa: E402,F401  (fixtures: tiaf_nus.npz and its samples on the device)

NAMES = ["MinkUNetMsMm", "MinkUNetMsMmNus", "MinkUNetMsKd"]
CLASSES = {"MinkUNetMsMm": 20, "MinkUNetMsMmNus": 17, "MinkUNetMsKd": 20}
VOTES = 3


@pytest.fixture(scope="module", autouse=True)
def reproducible_convolutions():
    """The vendor library's default solvers for UNet2D's convolutions are not bit-reproducible from call to call (image logits
    differ by ~1e-6 between two fp32 passes on one batch; tests/test_gpu_tiaf.py notes the same for fp16), and host path and device
    path are two forward passes.  With its deterministic solvers two passes of the TIAF models give the same bits, so that every
    comparison below can be exact."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def fresh(bd):
    """the batch as a data stage hands it over: new SparseTensor objects (a forward pass narrows / replaces their F), no index plan"""
    from taseg_amd.torchsparse import SparseTensor
    return {k: SparseTensor(v.F, v.C) if isinstance(v, SparseTensor) else v for k, v in bd.items() if k not in ("_plan", "image_input")}


def build_model(name, seed=3, **over):
    from taseg_amd.pcseg.model import build_network
    if name == "MinkUNetMsKd":
        kw = dict(SAMPLING_TYPE="random", MAX_VOXEL=100000, FEAT_KD="mse", FEAT_KD_WEIGHT=10.0)
    elif name.startswith("MinkUNetMsMm"):
        kw = dict(TIAF_CFG)
    else:
        kw = {}
    kw.update(over)
    # (the fusion head of the TIAF models is cr 1.0 wide; nuScenes clouds carry four features)
    cfg = make_model_cfg(name, in_dim=4 if name in ("MinkUNet", "MinkUNetMsMmNus") else 5, cr=1.0 if name.startswith("MinkUNetMsMm") else 0.5,
                         num_layer=[1] * 8, **kw)
    return fill_parameters(build_network(cfg, CLASSES.get(name, 20)), seed=seed).cuda().eval()


def spread_heads(model, batch):
    """fill_parameters' heads see rectified features that share one direction, so every point gets the same class and a payload
    would be a constant.  The batch's mean feature is taken out of the rows of the last linear layer of every head (W mean = 0),
    the bias dropped: the logits are centred per class over the batch, and the arg-max varies from point to point."""
    heads = [model.classifier[0]] + ([model.classifier_fusion[3]] if hasattr(model, "classifier_fusion") else [])
    mean = {}
    hooks = [h.register_forward_hook(lambda mod, i, o: mean.__setitem__(mod, i[0].detach().float().mean(0))) for h in heads]
    try:
        with torch.no_grad():
            model(fresh(batch))
    finally:
        for h in hooks:
            h.remove()
    with torch.no_grad():
        for h in heads:
            mu = mean[h]
            h.weight.sub_(torch.outer(h.weight @ mu, mu) / (mu @ mu)).mul_(8.0)
            h.bias.zero_()
    return model


def distinct(payloads):
    return len({int(v) for p in payloads for v in np.unique(p)})


@pytest.fixture(scope="module")
def models(batches):
    return {name: spread_heads(build_model(name), batches[name][0]) for name in NAMES}


@pytest.fixture(scope="module")
def batches(g, inputs, g_multiscan):  # noqa: F811
    """per model (validation batch of two scans, three-vote TTA batch of one scan)"""
    import test_gpu_kd_stage as K
    import test_gpu_tiaf_aug as TA
    import test_gpu_tiaf_nus_aug as TN
    from taseg_amd.data import augment as A
    from taseg_amd.data import kd as KD
    from taseg_amd.data import nuscenes_tiaf as NT
    from taseg_amd.data import tiaf as TF
    gt = dict(np.load(os.path.join(GOLDEN, "tiaf_data.npz"), allow_pickle=False))
    frames, s = [TA.device_frames(gt, b) for b in range(2)], TA.setup(gt)
    s["crop"] = (64, 192)               # UNet2D halves the maps four times: the fixture's 64 x 180 images, padded to a multiple of 16
    out = {"MinkUNetMsMm": (
        TA.build("batched", frames, s, None, None),
        TF.build_tiaf_tta_batch(frames[0], 0, VOTES, np.random.RandomState(1), s["steps"], s["multiscan"], s["step_image"], s["proj"],
                                s["crop"], TA.VOXEL, name=s["name"]))}
    out["MinkUNetMsMmNus"] = (NT.build_nusc_tiaf_batch_from_keyframes(TN._fresh(inputs, g)),
                              NT.build_nusc_tiaf_tta_batch(TN._fresh(inputs, g)[0], 0, VOTES, np.random.RandomState(1)))
    gk = dict(np.load(os.path.join(GOLDEN, "kd_stage.npz"), allow_pickle=False))
    scans = K.kd_scans(g_multiscan, gk)[:2]
    steps, steps_gt = g_multiscan["steps"].tolist(), gk["steps_gt"].tolist()
    rng = np.random.RandomState(1)
    out["MinkUNetMsKd"] = (KD.build_kd_batch(scans, 0.05, steps, steps_gt),
                           KD.build_kd_batch([scans[0]] * VOTES, 0.05, steps, steps_gt, aug=[A.draw_tta_params(rng, v) for v in range(VOTES)]))
    for val, tta in out.values():
        assert len(val["name"]) == 2 and len(tta["name"]) == VOTES
        assert 0 < int(val["point_mask"].sum()) < val["point_mask"].numel()         # the mask drops rows
    return out


def same_dictionaries(got, want):
    assert got["name"] == want["name"]
    for key in ("point_predict", "point_labels", "point_predict_logits"):
        assert len(got[key]) == len(want[key]), key
        for a, b in zip(got[key], want[key]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), key


# ------------------------------------------------------------------------------------------------ 1. validation
@pytest.mark.parametrize("name", NAMES)
def test_validation_on_device_gives_the_host_matrix(models, batches, name):
    from taseg_amd.pcseg import eval as E
    model, C, val = models[name].train(), CLASSES[name], batches[name][0]
    try:
        host = E.evaluate(model, (fresh(val) for _ in range(2)), C)
        dev = E.evaluate(model, (fresh(val) for _ in range(2)), C, on_device=True)
        assert model.training                                      # the caller's mode is restored
        model.eval()
        assert dev["hist"].shape == (C - 1, C - 1) and dev["hist"].dtype == host["hist"].dtype and host["hist"].sum() > 1000
        assert np.array_equal(dev["hist"], host["hist"]) and dev["miou"] == host["miou"] and np.array_equal(dev["iou"], host["iou"])
        dev = E.evaluate(model, (fresh(val) for _ in range(2)), C, on_device=True, prefetch=False)
        assert np.array_equal(dev["hist"], host["hist"]) and not model.training
        assert set(dev) == {"iou", "miou", "hist"}
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------------ 2. TTA
@pytest.mark.parametrize("name", NAMES)
def test_tta_on_device_gives_the_host_payload_and_sums(models, batches, name):
    from taseg_amd.pcseg import eval as E
    model, C, tta = models[name], CLASSES[name], batches[name][1]
    run = lambda **kw: E.evaluate(model, (fresh(tta) for _ in range(2)), C, tta_votes=VOTES, **kw)  # noqa: E731
    host = run()
    dev = run(on_device=True)
    assert set(dev) == {"predictions"} and len(dev["predictions"]) == 2
    for a, b in zip(dev["predictions"], host["predictions"]):
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape and a.shape[1] == 1 and len(a) > 500 and np.array_equal(a, b)
    assert distinct(host["predictions"]) > 3                       # (not a constant)
    with torch.no_grad():
        total = E.accumulate_votes(model(fresh(tta)), VOTES)
    everything = run(on_device=True, scores="all")
    assert np.array_equal(everything["predictions"][1], host["predictions"][1])
    assert everything["scores"][0].dtype == np.float32 and np.array_equal(everything["scores"][0].view(np.uint32), total.view(np.uint32))
    top3 = run(on_device=True, scores="top3")["scores"][0]
    assert np.array_equal(top3, np.sort(total, 1)[:, ::-1][:, :3])
    with pytest.raises(ValueError, match="votes"):
        E.evaluate(model, [fresh(tta)], C, tta_votes=VOTES + 1, on_device=True)


@pytest.mark.parametrize("name", NAMES)
def test_tta_under_autocast_sums_the_half_votes_in_float32(models, batches, name, monkeypatch):
    """the rule of tests/test_gpu_eval_device.py's autocast test, on the votes of the SAME forward pass: the arguments the model
    hands to the tail (exactly the host tail's), un-voxelised by the host tail."""
    from taseg_amd.pcseg import eval as E
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet import minkunet as M
    model, C, tta = models[name], CLASSES[name], batches[name][1]
    seen = []

    class Capture(M.DeviceEvalTail):
        def run(self, *a, **kw):
            seen.append((a, kw))
            return super().run(*a, **kw)
    monkeypatch.setattr(M, "DeviceEvalTail", Capture)
    with torch.autocast("cuda", dtype=torch.float16):
        dev = E.evaluate(model, [fresh(tta)], C, tta_votes=VOTES, on_device=True, scores="all")
    (a, kw), = seen
    assert a[0].dtype == torch.float16 and set(kw) == {"point_mask", "num_points_ms", "names"} and kw["names"] == tta["name"]
    per_vote = M.unvoxelise_predictions(*a, False, **kw)["point_predict_logits"]
    assert per_vote[0].dtype == np.float16
    total = per_vote[0].astype(np.float32)
    for v in range(1, VOTES):
        total += per_vote[v].astype(np.float32)              # NOT accumulate_votes on float16 arrays: that rounds after every vote
    assert np.array_equal(dev["scores"][0].view(np.uint32), total.view(np.uint32))
    assert np.array_equal(dev["predictions"][0][:, 0], np.argmax(total, 1))


# ------------------------------------------------------------------------------------------------ 3. the replace ensemble
def test_replace_ensemble_is_exercised_and_leaves_the_classifier_rows_alone(models, batches):
    from taseg_amd.pcseg import eval as E
    model, val = models["MinkUNetMsMm"], batches["MinkUNetMsMm"][0]
    assert model.ensemble_type == "replace"
    grabbed = {}
    hooks = [model.classifier.register_forward_hook(lambda mod, i, o: grabbed.update(out_ms=o, copy=o.clone())),
             model.classifier_fusion.register_forward_hook(lambda mod, i, o: grabbed.update(fusion=o.clone()))]
    try:
        with torch.no_grad():
            first = model(fresh(val))
    finally:
        for h in hooks:
            h.remove()
    rows, overlap_rows = grabbed["out_ms"].shape[0], grabbed["fusion"].shape[0]
    assert 0 < overlap_rows < rows, (overlap_rows, rows)
    # the rows the classifier returned are the caller's: the ensemble wrote into a tensor of its own
    assert torch.equal(grabbed["out_ms"], grabbed["copy"])
    with torch.no_grad():
        second = model(fresh(val))
    same_dictionaries(second, first)
    plain = build_model("MinkUNetMsMm", ENSEMBLE_TYPE=None)
    plain.load_state_dict(model.state_dict())
    with torch.no_grad():
        without = plain(fresh(val))
    differ = sum(int((a != b).sum()) for a, b in zip(first["point_predict"], without["point_predict"]))
    assert differ > 0                   # a tail that read the un-replaced rows would give other matrices below
    host, host_plain = E.evaluate(model, [fresh(val)], 20), E.evaluate(plain, [fresh(val)], 20)
    assert not np.array_equal(host["hist"], host_plain["hist"])
    assert np.array_equal(E.evaluate(model, [fresh(val)], 20, on_device=True)["hist"], host["hist"])
    assert np.array_equal(E.evaluate(plain, [fresh(val)], 20, on_device=True)["hist"], host_plain["hist"])
    # what the ensemble writes is the fusion head's output, row for row, in the order of the overlap mask
    seen = []

    class Capture:
        def run(self, out, *a, **kw):
            seen.append(out)
    hooks = [model.classifier.register_forward_hook(lambda mod, i, o: grabbed.update(out_ms=o)),
             model.classifier_fusion.register_forward_hook(lambda mod, i, o: grabbed.update(fusion=o))]
    try:
        with torch.no_grad():
            model(fresh(val), device_tail=Capture())
    finally:
        for h in hooks:
            h.remove()
    changed = (seen[0] != grabbed["out_ms"]).any(1)
    assert int(changed.sum()) == overlap_rows and torch.equal(seen[0][changed], grabbed["fusion"])


# ------------------------------------------------------------------------------------------------ 4. defer
@pytest.mark.parametrize("name", NAMES)
def test_deferred_tail_gives_the_dictionary_of_the_plain_call(models, batches, name):
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import PendingPredictions
    model, (val, tta) = models[name], batches[name]
    with torch.no_grad():
        want, want_tta = model(fresh(val)), model(fresh(tta), return_tta=True)
        p1 = model(fresh(val), defer=True)
        p2 = model(fresh(tta), return_tta=True, defer=True)
        p3 = model(fresh(val), defer=True)
    for pend, ref in ((p1, want), (p2, want_tta), (p3, want)):
        assert isinstance(pend, PendingPredictions)
        same_dictionaries(pend.result(), ref)
    assert len(want["point_predict"]) == 2 and len(want_tta["point_predict"]) == VOTES


# ------------------------------------------------------------------------------------------------ 5. labels from validation batches
SINGLE = ["MinkUNet", "MinkUNetMs"]
LENGTHS = (1500, 1237)                     # unequal scans: the second payload starts inside a wave of the launch


@pytest.fixture(scope="module")
def single(g_multiscan):
    """MinkUNet and MinkUNetMs with a two-scan batch of unequal scan lengths (multiscan.npz, the second scan cut short)"""
    from taseg_amd.data.stage import build_multiscan_batch
    from test_gpu_augment import kitti_scan
    scans = []
    for b, n in enumerate(LENGTHS):
        s = kitti_scan(g_multiscan, b)
        s["points"][-1], s["labels"][-1] = s["points"][-1][:n].contiguous(), s["labels"][-1][:n].contiguous()
        s["name"] = f"/data/sequences/0{b}/velodyne/00005{b}.bin"
        scans.append(s)
    batch = build_multiscan_batch(scans, 0.05, g_multiscan["steps"].tolist())
    assert batch["num_points"].reshape(-1).tolist() == list(LENGTHS)
    return {name: spread_heads(build_model(name), batch) for name in SINGLE}, batch


def same_payloads(got, want, dtype=np.uint32):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype == dtype and a.ndim == 2 and a.shape == b.shape and a.shape[1] == 1 and np.array_equal(a, b)


@pytest.mark.parametrize("name", SINGLE)
def test_predictions_of_validation_batches(single, name, tmp_path):
    from taseg_amd.pcseg import eval as E
    (models, batch), n_batches = single, 3
    model = models[name]
    run = lambda **kw: E.evaluate(model, (fresh(batch) for _ in range(n_batches)), 20, **kw)  # noqa: E731
    plain = run()
    with torch.no_grad():
        logits = model(fresh(batch))["point_predict_logits"]
    want = [E.vote_payload(x) for x in logits] * n_batches
    assert [len(w) for w in want[:2]] == list(LENGTHS) and distinct(want) > 3
    host = run(predictions=True)
    dev = run(predictions=True, on_device=True)
    for out in (host, dev):
        assert set(out) == {"iou", "miou", "hist", "predictions"}
        same_payloads(out["predictions"], want)
        assert np.array_equal(out["hist"], plain["hist"]) and out["miou"] == plain["miou"]
    assert np.array_equal(run(on_device=True)["hist"], plain["hist"])
    same_payloads(run(predictions=True, on_device=True, prefetch=False)["predictions"], want)
    # save_dir: one file per scan under the trainer's layout, holding the payload bytes; without predictions=True it stays ignored
    run(save_dir=str(tmp_path / "ignored")), run(save_dir=str(tmp_path / "ignored"), on_device=True)
    assert not (tmp_path / "ignored").exists()
    for kind, kw in (("host", {}), ("dev", {"on_device": True})):
        out = run(predictions=True, save_dir=str(tmp_path / kind), **kw)
        for scan_name, payload in zip(batch["name"], out["predictions"]):
            path = E._prediction_path(str(tmp_path / kind), scan_name, "semantickitti")
            assert path.endswith(".label") and open(path, "rb").read() == payload.tobytes() and len(payload) in LENGTHS


@pytest.mark.parametrize("name", SINGLE)
def test_predictions_for_nuscenes_and_the_errors_of_the_host_path(single, name):
    from taseg_amd.pcseg import eval as E
    models, batch = single
    model = models[name]
    bias = model.classifier[0].bias
    kept = bias.detach().clone()
    run = lambda bd, **kw: E.evaluate(model, [fresh(bd), fresh(bd)], 20, predictions=True, **kw)  # noqa: E731
    try:
        with torch.no_grad():
            bias[0] = -1e4                                   # class 0 never wins: a valid nuScenes payload
        want = run(batch)["predictions"]
        assert all((w != 0).all() for w in want)
        for kw in ({}, {"on_device": True}):
            out = run(batch, dataset="nuscenes", **kw)["predictions"]
            same_payloads(out, [w.astype(np.uint8) for w in want], np.uint8)
        with torch.no_grad():
            bias[0] = 1e4                                    # class 0 everywhere: refused where the host path refuses it
        for kw in ({}, {"on_device": True}):
            with pytest.raises(ValueError, match="class 0"):
                run(batch, dataset="nuscenes", **kw)
            assert all((p == 0).all() for p in run(batch, **kw)["predictions"])           # fine for SemanticKITTI
    finally:
        with torch.no_grad():
            bias.copy_(kept)
    # an inverse map outside its scene: IndexError at the read, on both paths
    from taseg_amd.torchsparse import SparseTensor
    key = "inverse_map" if name == "MinkUNet" else "inverse_map_ms"
    bad = dict(batch)
    f = batch[key].F.clone()
    f[7] = 10 ** 6
    bad[key] = SparseTensor(f, batch[key].C)
    for kw in ({}, {"on_device": True}):
        with pytest.raises(IndexError):
            run(bad, **kw)
    # labels and predictions of a scan that differ in length: the scan contributes nothing - raised with the payload (flag bit 3)
    short = dict(batch)
    short["targets_mapped"] = SparseTensor(batch["targets_mapped"].F[:-3], batch["targets_mapped"].C[:-3])
    with pytest.raises(IndexError, match="differ in length"):
        run(short, on_device=True)


# ------------------------------------------------------------------------------------------------ 6. remap
@pytest.mark.parametrize("name", SINGLE)
def test_remap_on_both_paths_and_in_both_modes(single, g_eval_ms, name):
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    from test_gpu_parity_r2 import _eval_batch
    models, batch = single
    model, lut = models[name], E.remap_lut(LEARNING_MAP_INV)
    through = lambda plain: [E.remap_labels(p, lut).reshape(-1, 1) for p in plain]  # noqa: E731
    plain = E.evaluate(model, [fresh(batch)], 20, predictions=True)
    assert distinct(plain["predictions"]) > 3                                             # (more than a constant goes through the table)
    for kw in ({}, {"on_device": True}):
        for remap in (LEARNING_MAP_INV, lut):
            out = E.evaluate(model, [fresh(batch)], 20, predictions=True, remap=remap, **kw)
            same_payloads(out["predictions"], through(plain["predictions"]))
            assert np.array_equal(out["hist"], plain["hist"])
    votes = int(g_eval_ms["votes"])
    tta = lambda **kw: E.evaluate(model, [_eval_batch(g_eval_ms, "tta_")], 20, tta_votes=votes, **kw)  # noqa: E731
    plain_tta = tta()["predictions"]
    assert distinct(plain_tta) > 3
    same_payloads(tta(on_device=True)["predictions"], plain_tta)                          # without remap: as before
    for kw in ({}, {"on_device": True}, {"on_device": True, "scores": "top3"}):
        same_payloads(tta(remap=LEARNING_MAP_INV, **kw)["predictions"], through(plain_tta))
    # nuScenes payloads through a table: narrowed to uint8 on both paths, and class 0 is still looked for BEFORE the table
    shift = np.arange(1, 21, dtype=np.int32)                                              # no class maps to 0
    has_zero = any((p == 0).any() for p in plain_tta)
    for kw in ({}, {"on_device": True}):
        if has_zero:
            with pytest.raises(ValueError, match="class 0"):
                tta(remap=shift, dataset="nuscenes", **kw)
        else:
            same_payloads(tta(remap=shift, dataset="nuscenes", **kw)["predictions"], [(p + 1).astype(np.uint8) for p in plain_tta], np.uint8)


def test_exported_labels_come_back_as_the_pseudo_classes_of_the_data_stage(single, g_multiscan, tmp_path):
    """the recipe's "history predictions" step in one validation pass: scans of a SemanticKITTI tree at two per batch -> .label
    files of raw ids -> multiscan_sample(pseudo_subdir=...)"""
    from taseg_amd.data import semantickitti as SK
    from taseg_amd.data.stage import build_multiscan_batch
    from taseg_amd.pcseg import eval as E
    from test_semantickitti_reader import _write_tree
    g = g_multiscan
    Tn, steps = int(g["T"]), g["steps"].tolist()
    root = tmp_path / "sequences"
    lengths = [1500 - 37 * t for t in range(Tn + 1)]
    _write_tree(str(root), 0, [g[f"b0_points_t{t}"][:n] for t, n in enumerate(lengths)],
                [g[f"b0_rawlabels_t{t}"][:n] for t, n in enumerate(lengths)], [g[f"b0_pose_t{t}"] for t in range(Tn + 1)])
    seq = SK.KittiSequence(str(root), 0)
    scans = [SK.multiscan_sample(seq, t, 0, steps) for t in range(Tn + 1)]
    make = lambda: (build_multiscan_batch(scans[i:i + 2], 0.05, steps) for i in range(0, Tn + 1, 2))  # noqa: E731
    model = single[0]["MinkUNet"]
    classes = E.evaluate(model, make(), 20, predictions=True)["predictions"]
    assert [len(c) for c in classes] == lengths
    out = E.evaluate(model, make(), 20, predictions=True, on_device=True, remap=SK.LEARNING_MAP_INV, save_dir=str(tmp_path))
    assert sorted(os.listdir(os.path.join(seq.dir, "predictions"))) == [f"{t:06d}.label" for t in range(Tn + 1)]
    for t in range(Tn + 1):
        assert np.array_equal(seq.raw_labels(t, "predictions"), out["predictions"][t][:, 0])
    back = SK.multiscan_sample(seq, Tn, Tn, steps, pseudo_subdir="predictions")
    assert len(back["pseudo"]) == Tn
    for t in range(Tn):
        assert np.array_equal(back["pseudo"][t].cpu().numpy(), classes[t][:, 0].astype(np.int64))
