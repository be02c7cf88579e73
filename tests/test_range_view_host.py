"""The range-view projection and kNN step without a GPU: the numpy restatements of tests/range_view_ref.py (which the GPU tests hold
the kernels to, bit for bit) against the REFERENCE's recorded outputs (tests/golden/range_view.npz: its own LaserScan, dataset tail
and KNN on the CPU), outside the rows range_view_ref declares undecided; the conditions on how many those may be; the hand-made kNN
points' labels worked out by hand; header, _lib.py, backend.py and the build flags agree on the new entry points."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import range_view_ref as R
from taseg_amd import _lib, backend
from taseg_amd.data.range_view import knn_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = (("ts_rv_project", 21), ("ts_rv_knn", 18))


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "range_view.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def ours(g):
    h, w = (int(v) for v in g["hw"])
    return R.project32(g["points"], g["batch"], g["first"], 2, h, w, *g["fov"], labels=g["labels"])


@pytest.mark.parametrize("tag", ["", "_wide"])
def test_projection_restatement_equals_the_reference_outside_undecided_rows(g, tag):
    """every column and row, except at the rows whose float64 proj_x / proj_y lies within project_delta of a cell edge (the
    reference's float32 arctan2 / arcsin may err by 4 ulp); at most 1 % of the rows may be undecided"""
    h, w = (int(v) for v in g["hw" + tag])
    mine = R.project32(g["points"], g["batch"], g["first"], 2, h, w, *g["fov"])
    undecided = R.project_undecided(g["points"], h, w, *g["fov"])
    print("undecided rows at %d x %d: %d of %d" % (h, w, undecided.sum(), len(undecided)))
    assert undecided.mean() <= 0.01
    assert mine["err"] == 0
    keep = ~undecided
    assert np.array_equal(mine["proj_x"][keep], g["proj_x" + tag][keep])
    assert np.array_equal(mine["proj_y"][keep], g["proj_y" + tag][keep])


def test_projection_depths_and_images_equal_the_reference(g, ours):
    """depths bit-equal at every row; every pixel's six values, range, index and label, except the pixels an undecided row touches
    in either version"""
    h, w = (int(v) for v in g["hw"])
    assert np.array_equal(ours["unproj_range"].view(np.uint32), g["unproj_range"].view(np.uint32))
    undecided = R.project_undecided(g["points"], h, w, *g["fov"])
    cell = lambda px, py: g["batch"].astype(np.int64) * h * w + py.astype(np.int64) * w + px      # noqa: E731
    tainted = np.union1d(cell(ours["proj_x"], ours["proj_y"])[undecided], cell(g["proj_x"], g["proj_y"])[undecided])
    # the reference's images, densely
    n_pix = 2 * h * w
    bg = np.array([-1 / np.float32(50), -1 / np.float32(50), -1 / np.float32(3), -1, -1 / np.float32(80), 0], dtype=np.float32)
    scan = np.tile(bg, (n_pix, 1))
    rng, idx, lab = np.full(n_pix, -1, dtype=np.float32), np.full(n_pix, -1, dtype=np.int32), np.zeros(n_pix, dtype=np.int64)
    at = g["image_at"]
    scan[at], rng[at], idx[at], lab[at] = g["image_scan"], g["image_range"], g["image_idx"], g["image_label"]
    keep = np.setdiff1d(np.arange(n_pix), tainted)
    assert len(keep) > 0.98 * n_pix
    mine = ours["scan_rv"].transpose(0, 2, 3, 1).reshape(-1, 6)
    assert np.array_equal(mine[keep].view(np.uint32), scan[keep].view(np.uint32))
    assert np.array_equal(ours["proj_range"].reshape(-1)[keep].view(np.uint32), rng[keep].view(np.uint32))
    assert np.array_equal(ours["proj_idx"].reshape(-1)[keep], idx[keep])
    assert np.array_equal(ours["label_rv"].reshape(-1)[keep], lab[keep])
    assert ours["label_rv"].shape == (2, 1, h, w) and ours["label_rv"].dtype == np.int64
    # the fixture has pixels with more than one row, and the reproduced oddity: a pixel won by row 0 of a scan has mask 0
    assert len(at) < len(g["points"])
    zero = np.flatnonzero(idx == 0)
    assert len(zero) >= 1 and (scan[zero, 5] == 0).all() and (scan[zero, 4] > 0).all()


@pytest.mark.parametrize("name", list(R.knn_cases()))
def test_knn_restatement_equals_the_reference_at_every_decided_point(g, name):
    spec, search, knn, cutoff, nclasses, continuous = R.knn_cases()[name]
    case = R.knn_case_inputs(spec)
    label, err, undecided = R.knn32(case["proj_range"], case["proj_class"], case["unproj_range"], case["px"], case["py"],
                                    case["batch"], knn_weight(search, 1.0).numpy(), knn, search, cutoff, nclasses)
    ref = g["knn_" + name].astype(np.int32)
    print("%s: %d points, %d undecided, %d differ" % (name, len(ref), undecided.sum(), (label != ref).sum()))
    assert err == 0 and len(ref) == len(label)
    assert np.array_equal(label[~undecided], ref[~undecided])
    if continuous:
        assert not undecided.any()                                    # a condition of the issue, not a measurement
    elif not isinstance(spec, str):
        assert (~undecided).mean() >= 0.8
        assert undecided.any()                                        # boundary ties do occur on the quantised ranges


def test_knn_cases_cover_borders_corners_and_short_neighbourhoods():
    case = R.knn_case_inputs(R.knn_cases()["s5_k5"][0])
    cells = set(zip(case["px"].tolist(), case["py"].tolist()))
    assert {(0, 0), (15, 0), (0, 7), (15, 7)} <= cells and len(cells) == 8 * 16
    spec = R.knn_cases()["s3_k9_empty"][0]
    case = R.knn_case_inputs(spec)
    assert 0.5 < (case["proj_range"] < 0).mean() < 0.7
    d, _, _ = R.knn_window(case["proj_range"], case["proj_class"], case["unproj_range"], case["px"], case["py"], case["batch"],
                           knn_weight(3, 1.0).numpy(), 3)
    assert (np.isfinite(d).sum(1) < 9).any()                          # fewer than K finite neighbours occur (the padding is finite)
    batch = R.knn_case_inputs(R.knn_cases()["s5_k5_batch"][0])["batch"]
    assert set(batch.tolist()) == {0, 2}                              # two scans plus an empty one


def test_hand_made_knn_points():
    case = R.hand_knn_case()
    args = (case["proj_range"], case["proj_class"], case["unproj_range"], case["px"], case["py"], case["batch"])
    label, err, _ = R.knn32(*args, knn_weight(3, 1.0).numpy(), 9, 3, 0.0, 20)
    assert label.tolist() == [3, 9, 4] and err == 0                   # the count tie: the lowest class; no cutoff: the neighbours
    label, err, _ = R.knn32(*args, knn_weight(3, 1.0).numpy(), 5, 3, 1.0, 20)
    assert label[1] == 1                                              # every vote cut off or unlabelled: class 1
    # a px outside the image: label 0 and the flag; every other label unchanged
    px = case["px"].copy()
    px[2] = 16
    label2, err2, _ = R.knn32(args[0], args[1], args[2], px, args[4], args[5], knn_weight(3, 1.0).numpy(), 5, 3, 1.0, 20)
    assert err2 == R.ERR_PIXEL and label2[2] == 0 and np.array_equal(label2[:2], label[:2])


@pytest.mark.parametrize("search", [3, 5, 7])
def test_knn_weight_is_one_minus_the_gaussian(search):
    w = knn_weight(search, 1.0)
    assert w.dtype.is_floating_point and w.shape == (search * search,)
    assert np.allclose(w.numpy(), R.knn_weight64(search, 1.0), rtol=0, atol=4 * 2.0 ** -24)
    assert (w.numpy() > 0).all() and (w.numpy() < 1).all()


def test_projection_hand_made_rows_in_the_restatement():
    """equal depths in one pixel: the lower index wins; row 0 of a scan winning a pixel: mask 0; the origin and a NaN row set their
    bits and change nothing else"""
    rows = np.array([[5, 1, 0, 0.1], [5, 1, 0, 0.2], [5, 1, 0, 0.3], [np.nan, 1, 1, 0.4], [0, 0, 0, 0.5], [-3, 2, -0.5, 0.6]], dtype=np.float32)
    batch = np.array([0, 0, 0, 1, 1, 1])
    got = R.project32(rows, batch, [0, 3], 2, 16, 32)
    assert got["err"] == (R.ERR_NONFINITE | R.ERR_ORIGIN)
    assert got["proj_x"][3] == got["proj_x"][4] == -1 and got["unproj_range"][3] == -1
    y, x = got["proj_y"][0], got["proj_x"][0]
    assert got["proj_idx"][0, y, x] == 0 and got["scan_rv"][0, 5, y, x] == 0 and got["scan_rv"][0, 3, y, x] == np.float32(0.1)
    y, x = got["proj_y"][5], got["proj_x"][5]
    assert got["proj_idx"][1, y, x] == 2 and got["scan_rv"][1, 5, y, x] == 1
    clean = R.project32(rows[[0, 1, 2, 5]], np.array([0, 0, 0, 1]), [0, 3], 2, 16, 32)
    assert clean["err"] == 0
    assert np.array_equal(clean["scan_rv"][0], got["scan_rv"][0]) and np.array_equal(clean["proj_range"], got["proj_range"])


def test_header_signatures_backend_and_build_flags_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taseg_hip.h")).read(), flags=re.S)
    for name, n_args in NEW_ENTRY_POINTS:
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1).strip()
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "ts_rv_project" in inspect.getsource(backend.rv_project) and "ts_rv_knn" in inspect.getsource(backend.rv_knn)
    from taseg_amd.csrc import build
    assert "range_view.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["range_view.hip"]
    from taseg_amd.data import range_view as D
    for bit in ("BATCH", "PIXEL", "NONFINITE", "ORIGIN"):
        value = int(re.search(r"#define TS_RV_ERR_%s (\d+)" % bit, header).group(1))
        assert value == getattr(D, "ERR_" + bit) == getattr(R, "ERR_" + bit)


def test_backend_refuses_host_tensors():
    import torch
    with pytest.raises(RuntimeError):
        backend.rv_knn(torch.zeros(1, 8, 16), torch.zeros(1, 8, 16, dtype=torch.int32), torch.zeros(2), torch.zeros(2, dtype=torch.int32),
                       torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), knn_weight(5, 1.0), 5, 5, 1.0, 20)


def test_reference_import_path_binds_after_install_as_dropin():
    code = ("import taseg_amd; names = taseg_amd.install_as_dropin()\n"
            "from pcseg.model.segmentor.range.utils import KNN\n"
            "import taseg_amd.pcseg.model.segmentor.range.utils as mine\n"
            "assert KNN is mine.KNN and names['pcseg.model.segmentor.range.utils'] is mine\n"
            "k = KNN()\n"
            "assert (k.knn, k.search, k.sigma, k.cutoff, k.nclasses) == (5, 5, 1.0, 1.0, 20)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_the_registry_still_refuses_the_range_view_names():
    from taseg_amd.pcseg.model import segmentor
    for name in ("RangeNet++", "SalsaNext", "FIDNet", "CENet"):
        assert name in segmentor._OUT_OF_SCOPE and name not in segmentor.__all__
