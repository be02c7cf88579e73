"""The cylinder data stage on the GPU (csrc/cylinder_stage.hip behind taseg_amd.data.cylinder).

1. Against the numpy restatement with the header's rules (tests/cylinder_stage_ref.py; tests/test_cylinder_stage_host.py holds it to the
   real reference): EVERY key bit for bit, the `phi_deg` column included - sizes around the wave and the workgroup, one and three
   samples with a single-point sample among longer ones, rows of 4 and 5 columns, 1 .. 32 classes, one cell holding every row, every
   row its own cell, rows at the origin, both signs of a zero y behind the sensor, rows on and beyond the faces of the space, ties
   between every pair of neighbouring classes, ignored rows; two calls give the same bits.
2. Against the REAL reference (tests/golden/cylinder_stage.npz cases a, a2, b, c, d and the evaluation batch of model_cylinder.npz): every
   integer key and 8 feature columns bit for bit; `phi_deg` within 2.07e-7 |value| of float64 (three float32 roundings + float32(pi)'s
   distance from pi) and within that + `phi_ref_ulp` float32 ulp of the reference's own value (numpy's float32 arctan2 is not correctly
   rounded; the fixture stores how far it lies from float64).
3. End to end: Cylinder_TS with the golden's parameters on the batch this stage builds gives model_cylinder.npz's logits and losses
   within the bars of tests/test_gpu_cylinder_model.py.
4. Refusals raise and leave the device usable.  With aug=None no augment launch is issued."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cylinder_stage_ref as R  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from taseg_amd.data.synthetic import synth_scan  # noqa: E402

RECIPE = ([0, -180, -4], [50, 180, 2])
GRID = [96, 80, 16]
COARSE = [24, 20, 8]


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "cylinder_stage.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def cloud():
    """one seeded scan of 1000 rows with a fifth column, and labels 0 .. 19: every synthetic input below is cut from it"""
    pts, lab = synth_scan(51, n_points=1000, n_beams=16, n_az=360)
    rs = np.random.RandomState(3)
    return np.concatenate([pts, rs.rand(len(pts), 1).astype(np.float32)], 1), rs.randint(0, 20, len(pts)).astype(np.int64)


def device_batch(points, labels, lo, hi, grid, aug=None, names=None, **kw):
    from taseg_amd.data import CylinderGrid, build_cylinder_batch
    scans = [{"points": torch.from_numpy(np.ascontiguousarray(p)).cuda(), "labels": torch.from_numpy(np.asarray(l)).cuda(),
              "name": names[b] if names else "s%d" % b} for b, (p, l) in enumerate(zip(points, labels))]
    return build_cylinder_batch(scans, CylinderGrid(lo, hi, grid), aug=aug, **kw)


def to_numpy(bd):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in bd.items()}


def assert_equal_bits(bd, want, who=""):
    """every key of collate_batch, with its dtype, bit for bit"""
    got = to_numpy(bd)
    assert set(got) == set(R.KEYS) | {"name"}, who
    assert not bd["num_points"].is_cuda and all(bd[k].is_cuda for k in R.KEYS if k != "num_points")
    for k in R.KEYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape, (who, k, a.shape, b.shape)
        if k.endswith("feature"):
            assert a.dtype == np.float32
            diff = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            assert len(diff) == 0, (who, k, diff[:5].tolist(), a[tuple(diff[0])], b[tuple(diff[0])])
        else:
            assert a.dtype == (np.int32 if k == "offset" else np.int64), (who, k, a.dtype)
            assert np.array_equal(a, b), (who, k, np.argwhere(a != b)[:5].tolist())


def check(points, labels, lo=RECIPE[0], hi=RECIPE[1], grid=GRID, who="", **kw):
    bd = device_batch(points, labels, lo, hi, grid, **kw)
    want = R.restate_batch(points, labels, lo, hi, grid, **kw)
    assert_equal_bits(bd, want, who)
    return bd, want


# ------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("n_samples", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_samples_and_row_widths(cloud, n, n_samples):
    pts, lab = cloud
    sizes = [n] if n_samples == 1 else [n, 1, max(n // 2, 2)]          # a single-point sample among longer ones
    starts = [0, 400, 500]
    for f in (4, 5):
        points = [pts[s:s + k, :f] for s, k in zip(starts, sizes)]
        labels = [lab[s:s + k] for s, k in zip(starts, sizes)]
        for grid in (GRID, COARSE):
            check(points, labels, grid=grid, who=f"n={n} B={n_samples} F={f} grid={grid}")


@pytest.mark.parametrize("num_classes", [1, 17, 20, 23, 32])
def test_class_counts_and_ignored_rows(cloud, num_classes):
    pts, _ = cloud
    rs = np.random.RandomState(num_classes)
    lab = rs.randint(0, num_classes, len(pts)).astype(np.int64)
    lab[rs.rand(len(pts)) < 0.15] = 67
    check([pts[:, :4], pts[:300, :4]], [lab, lab[:300]], grid=COARSE, num_classes=num_classes, who=f"C={num_classes}")
    # the highest class alone in a voxel of its own, beside a voxel of ignored rows: lane C - 1 of the vote is read
    alone = np.array([[40.0, 1.0, -1.0, 0.0]] * 3 + [[45.0, 1.0, -1.0, 0.0]] * 2, dtype=np.float32)
    _, want = check([alone], [np.array([num_classes - 1, 67, num_classes - 1, 67, 67])], grid=COARSE, num_classes=num_classes)
    assert want["voxel_label"].tolist() == [num_classes - 1, 0]
    # another ignore label, inside the class range: its rows are not counted although they name a class
    lab2 = rs.randint(0, num_classes, len(pts)).astype(np.int64)
    check([pts[:, :4]], [lab2], grid=COARSE, num_classes=num_classes, ignore_label=0, who=f"C={num_classes} ignore 0")


def test_one_cell_holds_every_row(cloud):
    rs = np.random.RandomState(5)
    pts = np.zeros((1000, 4), dtype=np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = 10.1 + 0.02 * rs.rand(1000), 0.05 * rs.rand(1000), -1.0 + 0.02 * rs.rand(1000)
    lab = rs.randint(0, 20, 1000).astype(np.int64)
    lab[::7] = 67
    _, want = check([pts], [lab], who="one cell")
    assert len(want["voxel_coord"]) == 1 and want["parts"][0]["counter"].sum() == (lab != 67).sum()
    # the same run with the winner decided by ONE vote in its last rows, and all of it ignored
    lab2 = np.where(np.arange(1000) < 499, 7, 3).astype(np.int64)
    lab2[-1] = 67
    _, want = check([pts], [lab2], who="one cell, 499 : 500")
    assert want["voxel_label"].tolist() == [3]
    lab2[:] = np.where(np.arange(1000) < 500, 7, 3)
    _, want = check([pts], [lab2], who="one cell, 500 : 500")
    assert want["voxel_label"].tolist() == [3]                        # the tie goes to the lower class
    _, want = check([pts], [np.full(1000, 67, dtype=np.int64)], who="one cell, all ignored")
    assert want["voxel_label"].tolist() == [0]


def test_every_row_its_own_cell():
    lo, hi = RECIPE
    step = (np.array(hi) - np.array(lo)) / (np.array(GRID) - 1)
    cx, cy = np.meshgrid(np.arange(2, 42, 2), np.arange(1, 79, 3), indexing="ij")
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    rho, phi = (cx + 0.5) * step[0], np.deg2rad((cy + 0.5) * step[1] - 180.0)
    pts = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(len(cx), -1.0), np.linspace(0, 1, len(cx))], 1).astype(np.float32)
    order = np.random.RandomState(2).permutation(len(pts))             # voxel order != input order
    pts, lab = pts[order], (np.arange(len(pts)) % 20).astype(np.int64)
    _, want = check([pts], [lab], who="own cells")
    assert len(want["voxel_coord"]) == len(pts) and not np.array_equal(want["parts"][0]["inds"], np.arange(len(pts)))
    assert np.array_equal(want["voxel_label"], lab[want["parts"][0]["inds"]])


def test_origin_zero_signs_and_the_faces_of_the_space():
    z = np.float32(-1.0)
    rows = [
        # at the origin, every combination of zero signs (arctan2 = 0, -0, pi, -pi)
        (0.0, 0.0, z), (0.0, -0.0, z), (-0.0, 0.0, z), (-0.0, -0.0, z), (0.0, 0.0, 0.0),
        # y = +0 and y = -0 behind the sensor: +180 and -180 degrees, the last and the first azimuth cell
        (-10.0, 0.0, z), (-10.0, -0.0, z), (-1e-3, 0.0, z), (-49.0, -0.0, z),
        # exactly on the maximum of rho (3-4-5 triangle: sqrt is exact) and beyond it; on and beyond both z faces
        (50.0, 0.0, z), (30.0, 40.0, z), (60.0, 0.0, z), (300.0, -400.0, z), (10.0, 1.0, 2.0), (10.0, 1.0, 2.5), (10.0, 1.0, 1e9),
        (10.0, 1.0, -4.0), (10.0, 1.0, -4.5), (10.0, 1.0, np.nextafter(np.float32(2.0), np.float32(0.0))), (0.0, 7.0, z), (0.0, -7.0, z),
    ]
    pts = np.array([(x, y, zz, 0.5) for x, y, zz in rows], dtype=np.float32)
    lab = (np.arange(len(pts)) % 20).astype(np.int64)
    _, want = check([pts], [lab], who="faces, recipe space")
    pc = want["point_coord"]
    assert pc[5, 1] == GRID[1] - 1 and pc[6, 1] == 0 and pc[9, 0] == pc[10, 0] == pc[11, 0] == GRID[0] - 1
    assert want["point_feature"][5, R.PHI_COLUMN] == 180.0 and want["point_feature"][6, R.PHI_COLUMN] == -180.0
    assert np.signbit(want["point_feature"][1, R.PHI_COLUMN]) and want["point_feature"][2, R.PHI_COLUMN] == 180.0
    # a space narrower than the data on every axis: rows exactly on each maximum (phi = 90 degrees exactly) and beyond it
    lo, hi, grid = [5, -90, -1.5], [20, 90, 0.5], [32, 24, 8]
    rows = [(0.0, 10.0, 0.5), (0.0, 20.0, 0.5), (-1.0, 10.0, 0.6), (0.0, -10.0, -1.5), (1.0, -10.0, -1.6), (12.0, 16.0, 0.0), (3.0, 4.0, 0.0),
            (2.0, 1.0, 0.0), (25.0, 1.0, -2.0), (-3.0, -1.0, 3.0)]
    pts = np.array([(x, y, zz, 0.25) for x, y, zz in rows], dtype=np.float32)
    _, want = check([pts], [np.arange(len(pts), dtype=np.int64)], lo=lo, hi=hi, grid=grid, who="faces, narrow space")
    assert want["point_feature"][0, R.PHI_COLUMN] == 90.0 and (want["point_coord"][[0, 1, 2], 1] == grid[1] - 1).all()
    assert want["point_coord"][5, 0] == grid[0] - 1 and want["point_coord"][6, 0] == 0


def test_ties_between_every_pair_of_neighbouring_classes():
    """voxel j holds k rows of class j + 1 THEN k rows of class j (the lower class wins although the higher comes first), for runs
    shorter and longer than the 32 lanes of a voxel's group; then voxels of three-way ties and one where a late row breaks the tie"""
    lo, hi = RECIPE
    step = (np.array(hi) - np.array(lo)) / (np.array(GRID) - 1)
    for num_classes, k in ((20, 1), (20, 3), (32, 17), (32, 40)):
        pts, lab = [], []
        for j in range(num_classes - 1):
            centre = ((j + 2.5) * step[0], 0.0, -1.0, 0.0)
            pts += [centre] * (2 * k)
            lab += [j + 1] * k + [j] * k
        # three classes tied; the middle one ahead by a single late row; ignored rows that would have changed the winner
        far = ((num_classes + 5.5) * step[0], 0.0, -1.0, 0.0)
        pts += [far] * 6
        lab += [9, 5, 7, 5, 9, 7]
        far2 = ((num_classes + 7.5) * step[0], 0.0, -1.0, 0.0)
        pts += [far2] * 7
        lab += [9, 5, 7, 5, 9, 7, 7]
        far3 = ((num_classes + 9.5) * step[0], 0.0, -1.0, 0.0)
        pts += [far3] * 6
        lab += [4, 67, 67, 67, 2, 67]
        pts, lab = np.array(pts, dtype=np.float32), np.array(lab, dtype=np.int64)
        _, want = check([pts, pts[:5]], [lab, lab[:5]], num_classes=num_classes, who=f"ties C={num_classes} k={k}")
        first = want["voxel_label"][:num_classes + 2]
        assert first.tolist() == list(range(num_classes - 1)) + [5, 7, 2], (num_classes, k, first)


def test_two_calls_give_the_same_bits(cloud, g):
    pts, lab = cloud
    a = device_batch([pts[:, :4], pts[:257, :4]], [lab, lab[:257]], *RECIPE, COARSE)
    b = device_batch([pts[:, :4], pts[:257, :4]], [lab, lab[:257]], *RECIPE, COARSE)
    assert all(torch.equal(a[k], b[k]) for k in R.KEYS)
    ins = R.case_inputs(g, "a")
    a, b = (device_batch(ins[0], ins[1], ins[3], ins[4], ins[5], aug=ins[6]) for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in R.KEYS)


# ------------------------------------------------------------------------------------------------- 2. against the reference
@pytest.mark.parametrize("tag", ["a", "a2", "b", "c"])
def test_batches_match_the_reference(g, tag):
    pts, labs, names, lo, hi, grid, aug = R.case_inputs(g, tag)
    bd = device_batch(pts, labs, lo, hi, grid, aug=aug, names=names)
    assert bd["name"] == names
    got = to_numpy(bd)
    R.check_against_reference(got, R.reference(g, tag), float(g["phi_ref_ulp"]), tag)
    assert np.array_equal(got["voxel_feature"].view(np.uint32), got["point_feature"][g[f"{tag}_inds"]].view(np.uint32))
    assert_equal_bits(bd, R.restated(g, tag), tag)                     # ... and the restatement, the augmentation included


def test_tta_views_match_the_reference(g):
    from taseg_amd.data import CylinderGrid, build_cylinder_tta_batch
    scan = {"points": torch.from_numpy(g["d_points0"]).cuda(), "labels": torch.from_numpy(g["d_labels0"]).cuda(),
            "name": g["d_names"].tolist()[0]}
    before = scan["points"].clone()
    grid = CylinderGrid(g["d_space_min"].tolist(), g["d_space_max"].tolist(), g["d_grid"].tolist())
    bd = build_cylinder_tta_batch(scan, 0, int(g["d_views"]), np.random.RandomState(int(g["d_draw_seed"])), grid)
    assert torch.equal(scan["points"], before)                         # the resident scan is not written
    assert bd["name"] == g["d_names"].tolist() * 3 and bd["num_points"].tolist() == [len(before)] * 3
    got = to_numpy(bd)
    R.check_against_reference(got, R.reference(g, "d"), float(g["phi_ref_ulp"]), "d")
    assert np.array_equal(got["voxel_feature"].view(np.uint32), got["point_feature"][g["d_inds"]].view(np.uint32))
    assert_equal_bits(bd, R.restated(g, "d"), "d")


@pytest.fixture(scope="module")
def model_batch():
    """the two scans of tests/golden/model_cylinder.npz (make_golden_cylinder.py:36, :87-89) through this stage"""
    m = dict(np.load(os.path.join(GOLDEN, "model_cylinder.npz"), allow_pickle=False))
    scans = [synth_scan(seed, n_points=1000, n_beams=16, n_az=360) for seed in (33, 34)]
    bd = device_batch([p for p, _ in scans], [l.astype(np.int64) for _, l in scans], *RECIPE, m["grid"].tolist(), names=m["batch_name"].tolist())
    return m, bd


def test_the_model_fixtures_batch_matches_the_reference(g, model_batch):
    m, bd = model_batch
    got = to_numpy(bd)
    ref = {k: m["batch_" + k] for k in R.KEYS if k != "voxel_feature"}
    ref["voxel_feature"] = got["voxel_feature"]                        # (not stored there; checked as rows of point_feature below)
    R.check_against_reference(got, ref, float(g["phi_ref_ulp"]), "model_cylinder")
    assert len(np.unique(got["inverse_map"][:1000])) == int(got["offset"][0])       # inverse_map is local to its sample
    # voxel_feature = point_feature[inds]: the first point of every voxel in input order
    first = {}
    for i, c in enumerate(map(tuple, got["point_coord"].tolist())):
        first.setdefault(c, i)
    rows = np.array([first[tuple(c)] for c in got["voxel_coord"].tolist()])
    assert np.array_equal(got["voxel_feature"].view(np.uint32), got["point_feature"][rows].view(np.uint32))
    assert bd["name"] == m["batch_name"].tolist()


# ------------------------------------------------------------------------------------------------- 3. end to end
def test_cylinder_ts_on_the_built_batch_gives_the_goldens_logits_and_losses(model_batch):
    import test_gpu_cylinder_model as M                               # the bars and the model of the existing comparison
    m, bd = model_batch
    model = M._model(m).train()
    got = {}
    hooks = [model.logits.register_forward_hook(lambda mod, i, o: got.update(logits=o.F.detach().float(), coords=o.C)),
             model.point_logits.register_forward_hook(lambda mod, i, o: got.__setitem__("point_logits", o.detach().float()))]
    ret, tb, _ = model(dict(bd))
    for h in hooks:
        h.remove()
    assert np.array_equal(got["coords"].cpu().numpy(), m["voxel_order"])
    logits, point_logits = got["logits"].cpu().numpy(), got["point_logits"].cpu().numpy()
    print(f"max |voxel logits - ref| {np.abs(logits - m['train_logits']).max():.2e}, point logits "
          f"{np.abs(point_logits - m['train_point_logits']).max():.2e}, loss {tb['loss']:.6f} vs {float(m['train_loss']):.6f}, "
          f"loss_point {tb['loss_point']:.6f} vs {float(m['train_loss_point']):.6f}")
    assert np.abs(logits - m["train_logits"]).max() <= M.LOGIT_TOL
    assert np.abs(point_logits - m["train_point_logits"]).max() <= M.LOGIT_TOL
    assert abs(tb["loss"] - float(m["train_loss"])) <= 1e-3
    assert abs(tb["loss_point"] - float(m["train_loss_point"])) <= 1e-3
    assert abs(float(ret["loss"].detach()) - float(m["train_loss_total"])) <= 2e-3


# ------------------------------------------------------------------------------------------------- 4. refusals, structure
def test_refusals_raise_and_leave_the_device_usable(cloud):
    from taseg_amd import backend as B
    from taseg_amd.data import CylinderGrid, build_cylinder_batch
    pts, lab = cloud
    pts4 = pts[:300, :4]
    bad_label = lab[:300].copy()
    bad_label[123] = 20
    with pytest.raises(ValueError, match="label"):
        device_batch([pts4], [bad_label], *RECIPE, GRID, num_classes=20)
    bad_label[123] = -1
    with pytest.raises(ValueError, match="label"):
        device_batch([pts4], [bad_label], *RECIPE, GRID)
    for column, value in ((0, np.nan), (1, np.inf), (2, np.nan)):
        nan_row = pts4.copy()
        nan_row[77, column] = value
        with pytest.raises(ValueError, match="non-finite"):
            device_batch([pts4, nan_row], [lab[:300], lab[:300]], *RECIPE, GRID)
    grid = CylinderGrid(*RECIPE, GRID)
    cpu = {"points": torch.from_numpy(pts4), "labels": torch.from_numpy(lab[:300]), "name": ""}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_cylinder_batch([cpu], grid)
    with pytest.raises(TypeError, match="F >= 4"):
        device_batch([pts[:300, :3]], [lab[:300]], *RECIPE, GRID)
    with pytest.raises(B.BackendError, match="classes"):
        device_batch([pts4], [lab[:300]], *RECIPE, GRID, num_classes=33)
    one = {"points": torch.from_numpy(pts4[:1]).cuda(), "labels": torch.from_numpy(lab[:1]).cuda(), "name": ""}
    with pytest.raises(ValueError, match="0 <= batch < 1024"):
        build_cylinder_batch([one] * 1025, grid)
    # a sample index of 1024 inside the rows: refused at the read, as sparse_quantize refuses it - and nothing written out of bounds
    rows = torch.from_numpy(pts4).cuda()
    sample = torch.zeros(300, dtype=torch.int32, device="cuda")
    sample[200:] = 1024
    cells, _, _, flags = B.cylinder_cells(rows, grid.space(), sample)
    _, _, _, counts, flags = B.cylinder_voxels(cells, torch.from_numpy(lab[:300]).cuda(), 2, flags=flags)
    assert flags.tolist() == [0, 0, 4] and int(counts[2]) <= 300
    with pytest.raises(B.BackendError):
        B.cylinder_voxels(cells, torch.from_numpy(lab[:300]).cuda(), 1025)
    # 1024 samples of one row each are within the range
    many = build_cylinder_batch([one] * 1024, grid)
    assert many["offset"].tolist() == list(range(1, 1025)) and many["inverse_map"].eq(0).all()
    check([pts4], [lab[:300]], who="after the refusals")


def test_no_augment_launch_without_aug(cloud, monkeypatch):
    from taseg_amd import backend as B
    from taseg_amd.data import cylinder as C
    pts, lab = cloud
    calls = []
    real = B.stage_augment
    monkeypatch.setattr(B, "stage_augment", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    device_batch([pts[:, :4], pts[:10, :4]], [lab, lab[:10]], *RECIPE, GRID)
    assert calls == []
    from taseg_amd.data.augment import AugParams
    resident = torch.from_numpy(np.ascontiguousarray(pts[:, :4])).cuda()
    before = resident.clone()
    C.build_cylinder_batch([{"points": resident, "labels": torch.from_numpy(lab).cuda(), "name": ""}],
                           C.CylinderGrid(*RECIPE, GRID), aug=[AugParams(scale=1.01, scale_on=True)])
    assert calls == [1] and torch.equal(resident, before)              # one launch, and the resident scan is not written
