"""The range-view projection and kNN step on the GPU (csrc/range_view.hip behind taseg_amd.data.range_view.build_range_view_batch
and pcseg.model.segmentor.range.utils.KNN): every output equals the numpy restatement of tests/range_view_ref.py BIT FOR BIT - on the
clouds of the reference fixture (tests/golden/range_view.npz; tests/test_range_view_host.py compares that restatement with the
reference's own output) and on hand-made rows - and the kNN labels equal the reference's recorded ones at every decided point.  Two
runs give the same bits; the winner of a pixel does not depend on the order the rows arrive in."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import range_view_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS_F, KEYS_I = ("scan_rv", "proj_range", "unproj_range"), ("proj_idx", "proj_x", "proj_y")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "range_view.npz"), allow_pickle=False))


def _scans(points, labels, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [{"points": torch.from_numpy(points[a:b]).cuda(), "labels": None if labels is None else torch.from_numpy(labels[a:b]).cuda(),
             "name": "scan%d" % i} for i, (a, b) in enumerate(zip(offs[:-1], offs[1:]))]


def _same(points, labels, lens, hw, fov=(3.0, -25.0)):
    from taseg_amd.data.range_view import build_range_view_batch
    bd = {}
    got = build_range_view_batch(_scans(points, labels, lens), hw, fov, batch_dict=bd)
    again = build_range_view_batch(_scans(points, labels, lens), hw, fov)
    b = len(lens)
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    batch = np.repeat(np.arange(b), lens)
    want = R.project32(points, batch, first, b, hw[0], hw[1], *fov, labels=labels)
    for key in KEYS_F:
        assert torch.equal(got[key].view(torch.int32), again[key].view(torch.int32)), key
        assert np.array_equal(got[key].cpu().numpy().view(np.uint32), want[key].view(np.uint32)), key
    for key in KEYS_I:
        assert got[key].dtype == torch.int32 and np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert got["scan_rv"].shape == (b, 6) + tuple(hw) and got["mask_rv"].shape == (b, 1) + tuple(hw)
    assert torch.equal(got["mask_rv"][:, 0], got["scan_rv"][:, 5])
    if labels is not None:
        assert got["label_rv"].dtype == torch.int64 and got["label_rv"].shape == (b, 1) + tuple(hw)
        assert np.array_equal(got["label_rv"].cpu().numpy(), want["label_rv"])
    else:
        assert "label_rv" not in got
    assert int(got["range_view_err"]) == want["err"]
    assert got["scan_name"] == ["scan%d" % i for i in range(b)] and got["offset"].tolist() == [0] + np.cumsum(lens).tolist()
    assert bd["scan_rv"] is got["scan_rv"] and bd["range_view_err"] is got["range_view_err"]
    assert np.array_equal(got["batch"].cpu().numpy(), batch)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}, want


@pytest.mark.parametrize("tag", ["", "_wide"])
def test_projection_equals_the_restatement_on_the_fixture_clouds(g, tag):
    hw = tuple(int(v) for v in g["hw" + tag])
    lens = np.bincount(g["batch"]).tolist()
    got, want = _same(g["points"], g["labels"], lens, hw, tuple(float(v) for v in g["fov"]))
    assert got["range_view_err"] == 0
    cells = g["batch"].astype(np.int64) * hw[0] * hw[1] + want["proj_y"] * hw[1] + want["proj_x"]
    assert len(np.unique(cells)) < len(cells)                          # pixels with more than one row are in there
    # ... and equals the reference's recorded columns and rows outside the undecided rows
    keep = ~R.project_undecided(g["points"], hw[0], hw[1], *g["fov"])
    assert np.array_equal(got["proj_x"][keep], g["proj_x" + tag][keep]) and np.array_equal(got["proj_y"][keep], g["proj_y" + tag][keep])


def test_projection_on_hand_made_rows():
    h, w = 16, 32
    f = np.float32
    up, down = np.deg2rad(20.0), np.deg2rad(-40.0)
    rows = np.array([
        # x, y, z, remission                               scan 0 (7 rows)
        [5, 1, 0, 0.1],                                    # 0: the scan's row 0 wins its pixel (equal depths: the lowest index): mask 0
        [5, 1, 0, 0.2],                                    # 1: the same point again
        [1, 5, 0, 0.25],                                   # 2: the same depth, another pixel
        [4 * np.cos(up), 0, 4 * np.sin(up), 0.3],          # 3: above the field of view (3 degrees): clamped to row 0
        [4 * np.cos(down), 0, 4 * np.sin(down), 0.4],      # 4: below it (-25 degrees): clamped to row H - 1
        [-7, 0.0, 0.5, 0.5],                               # 5: yaw = -pi: proj_x = 0
        [-7, -0.0, 0.5, 0.55],                             # 6: yaw = +pi: proj_x = W, clamped to W - 1
        #                                                  scan 1 (6 rows); scan 2 is empty
        [0, 0, 0, 0.6],                                    # 7: the origin: flagged, takes no part
        [np.nan, 1, 1, 0.7],                               # 8: NaN: flagged
        [10, 1, 0, 0.8],                                   # 9: farther than row 11 in the same pixel: loses
        [3, -3, -0.4, 0.9],                                # 10
        [5, 0.5, 0, 0.95],                                 # 11: nearer: wins
        [0, 0, 2, 0.97],                                   # 12: straight up: z / depth = 1
    ], dtype=f)
    labels = np.arange(1, 14, dtype=np.int32)
    lens = [7, 6, 0]
    got, want = _same(rows, labels, lens, (h, w))
    assert got["range_view_err"] == (R.ERR_ORIGIN | R.ERR_NONFINITE)
    assert got["proj_x"][[7, 8]].tolist() == [-1, -1] and got["unproj_range"][[7, 8]].tolist() == [-1, -1]
    y, x = got["proj_y"][0], got["proj_x"][0]
    assert (y, x) == (got["proj_y"][1], got["proj_x"][1])
    assert got["proj_idx"][0, y, x] == 0 and got["scan_rv"][0, 5, y, x] == 0 and got["scan_rv"][0, 3, y, x] == f(0.1)
    assert got["label_rv"][0, 0, y, x] == 1
    assert got["proj_y"][3] == 0 and got["proj_y"][4] == h - 1 and got["proj_y"][12] == 0
    assert got["proj_x"][5] == 0 and got["proj_x"][6] == w - 1
    y, x = got["proj_y"][11], got["proj_x"][11]
    assert (y, x) == (got["proj_y"][9], got["proj_x"][9]) and got["proj_idx"][1, y, x] == 4 and got["scan_rv"][1, 5, y, x] == 1
    assert got["label_rv"][1, 0, y, x] == 12
    bg = np.array([-1 / f(50), -1 / f(50), -1 / f(3), -1, -1 / f(80), 0], dtype=f)
    assert (got["scan_rv"][2] == bg[:, None, None]).all() and (got["proj_range"][2] == -1).all() and (got["proj_idx"][2] == -1).all()
    # the flagged rows leave every other value unchanged
    clean = np.array([0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12])
    got2, _ = _same(rows[clean], labels[clean], [7, 4, 0], (h, w))
    assert got2["range_view_err"] == 0
    assert np.array_equal(got2["scan_rv"][0].view(np.uint32), got["scan_rv"][0].view(np.uint32))
    assert np.array_equal(got2["proj_range"].view(np.uint32), got["proj_range"].view(np.uint32))
    assert np.array_equal(got2["proj_x"], got["proj_x"][clean])
    # the rows of scan 0 in another order: the winner is still the lowest index of the smallest depth - now the other row of the pair
    perm = np.array([1, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    got3, _ = _same(rows[perm], labels[perm], lens, (h, w))
    y, x = got3["proj_y"][0], got3["proj_x"][0]
    assert got3["scan_rv"][0, 3, y, x] == f(0.2) and got3["label_rv"][0, 0, y, x] == 2
    # without labels, and no rows at all: background everywhere
    _same(rows, None, lens, (h, w))
    got4, _ = _same(rows[:0], labels[:0], [0, 0], (h, w))
    assert got4["range_view_err"] == 0 and (got4["proj_idx"] == -1).all() and (got4["label_rv"] == 0).all()


def test_projection_flags_a_batch_index_outside_the_batch():
    from taseg_amd import backend as B
    rows = R.synth_cloud(3, 10)
    batch = np.array([0, 0, 0, 0, 0, 1, 1, 1, 5, -1], dtype=np.int32)
    first = np.array([0, 5], dtype=np.int32)
    out = B.rv_project(torch.from_numpy(rows).cuda(), torch.from_numpy(batch).cuda(), torch.from_numpy(first).cuda(), 2, 16, 32)
    want = R.project32(rows, batch, first, 2, 16, 32)
    assert int(out["err"]) == want["err"] == R.ERR_BATCH
    assert np.array_equal(out["proj_x"].cpu().numpy(), want["proj_x"]) and out["proj_x"][8:].tolist() == [-1, -1]
    assert np.array_equal(out["scan_rv"].cpu().numpy().view(np.uint32), want["scan_rv"].view(np.uint32))
    assert out["label_rv"] is None


def _knn(case, search, knn, cutoff, nclasses):
    from taseg_amd.pcseg.model.segmentor.range.utils import KNN
    mod = KNN({"knn": knn, "search": search, "sigma": 1.0, "cutoff": cutoff}, nclasses)
    dev = {k: torch.from_numpy(v).cuda() for k, v in case.items()}
    label, err = mod.forward_batch(dev["proj_range"], dev["unproj_range"], dev["proj_class"], dev["px"], dev["py"], dev["batch"])
    again, _ = mod.forward_batch(dev["proj_range"], dev["unproj_range"], dev["proj_class"], dev["px"], dev["py"], dev["batch"])
    assert label.dtype == torch.int64 and torch.equal(label, again)
    return label.cpu().numpy(), int(err), mod, dev


@pytest.mark.parametrize("name", list(R.knn_cases()))
def test_knn_equals_the_restatement_everywhere_and_the_reference_where_decided(g, name):
    from taseg_amd.data.range_view import knn_weight
    spec, search, knn, cutoff, nclasses, continuous = R.knn_cases()[name]
    case = R.knn_case_inputs(spec)
    label, err, mod, dev = _knn(case, search, knn, cutoff, nclasses)
    want, want_err, undecided = R.knn32(case["proj_range"], case["proj_class"], case["unproj_range"], case["px"], case["py"],
                                        case["batch"], knn_weight(search, 1.0).numpy(), knn, search, cutoff, nclasses)
    assert err == want_err == 0
    assert np.array_equal(label, want)
    ref = g["knn_" + name].astype(np.int64)
    assert np.array_equal(label[~undecided], ref[~undecided])
    if continuous:
        assert not undecided.any()
    # the reference's own call, one scan: the same labels as the batched call gives that scan
    b = int(case["batch"][0]) if len(case["batch"]) else 0
    at = torch.from_numpy(np.flatnonzero(case["batch"] == b)).cuda()
    one = mod(dev["proj_range"][b], dev["unproj_range"][at], dev["proj_class"][b], dev["px"][at], dev["py"][at])
    assert np.array_equal(one.cpu().numpy(), want[at.cpu().numpy()])


def test_knn_hand_made_points_and_flags():
    case = R.hand_knn_case()
    label, err, _, _ = _knn(case, 3, 9, 0.0, 20)
    assert label.tolist() == [3, 9, 4] and err == 0                    # a count tie: the lowest class wins
    label, err, _, _ = _knn(case, 3, 5, 1.0, 20)
    assert label[1] == 1 and err == 0                                  # every vote cut off or unlabelled: class 1
    bad = dict(case)
    bad["px"] = np.array([4, 12, 16], dtype=np.int32)                  # outside the image
    label2, err2, _, _ = _knn(bad, 3, 5, 1.0, 20)
    assert err2 == R.ERR_PIXEL and label2[2] == 0 and np.array_equal(label2[:2], label[:2])
    bad = dict(case)
    bad["batch"] = np.array([0, 1, -1], dtype=np.int32)
    label3, err3, _, _ = _knn(bad, 3, 5, 1.0, 20)
    assert err3 == R.ERR_BATCH and label3.tolist() == [int(label[0]), 0, 0]


def test_knn_refuses_what_it_does_not_support():
    from taseg_amd import _lib
    case = R.hand_knn_case()
    for search, knn, nclasses in ((9, 5, 20), (5, 26, 20), (5, 0, 20), (5, 5, 33)):
        with pytest.raises(_lib.BackendError, match="code -4"):
            _knn(case, search, knn, 1.0, nclasses)


def test_knn_after_the_projection_of_the_fixture_clouds(g):
    """the two kernels together, as evaluation uses them: project, take a per-pixel class (here the projected label), vote"""
    from taseg_amd.data.range_view import build_range_view_batch, knn_weight
    from taseg_amd.pcseg.model.segmentor.range.utils import KNN
    hw = tuple(int(v) for v in g["hw"])
    lens = np.bincount(g["batch"]).tolist()
    got = build_range_view_batch(_scans(g["points"], g["labels"], lens), hw)
    cls = got["label_rv"][:, 0].int()
    label, err = KNN(nclasses=20).forward_batch(got["proj_range"], got["unproj_range"], cls, got["proj_x"], got["proj_y"], got["batch"])
    want, _, _ = R.knn32(got["proj_range"].cpu().numpy(), cls.cpu().numpy(), got["unproj_range"].cpu().numpy(), got["proj_x"].cpu().numpy(),
                         got["proj_y"].cpu().numpy(), g["batch"], knn_weight(5, 1.0).numpy(), 5, 5, 1.0, 20)
    assert int(err) == 0 and np.array_equal(label.cpu().numpy(), want)
