"""Host-side checks of the cylinder data stage (no GPU): the ABI of the new entry points, CylinderGrid's doubles, and the numpy
restatement of the stage with the header's rules (tests/cylinder_stage_ref.py) against what the REAL reference's dataset code produced
(tests/golden/cylinder_stage.npz, made by tests/golden/make_golden_cylinder_stage.py, and the evaluation batch of model_cylinder.npz):
every key equal, the `phi_deg` feature column within the stated distance - the device takes the float64 arc tangent rounded once, numpy's
float32 arctan2 is not correctly rounded.  The restatement is what tests/test_gpu_cylinder_stage.py holds the device to bit for bit."""
import os
import re

import numpy as np
import pytest

import cylinder_stage_ref as R
from conftest import GOLDEN, ROOT
from taseg_amd.data.synthetic import synth_scan

ENTRY_POINTS = ("ts_cylinder_cells", "ts_cylinder_voxels_workspace_bytes", "ts_cylinder_voxels")
CASES = ("a", "a2", "b", "c", "d")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "cylinder_stage.npz"), allow_pickle=False))


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_header_table_and_argument_counts_agree():
    from taseg_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taseg_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in include/taseg_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len([a for a in m.group(2).split(",") if a.strip()]), name
        assert (res is _lib._sz) == (m.group(1) == "size_t"), name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in ENTRY_POINTS)
    assert lib.ts_cylinder_voxels_workspace_bytes(1000, 3) > 1000 * (2 * 8 + 5 * 4)
    from taseg_amd import backend as B
    words = re.search(r"#define\s+TS_CYL_FLAG_WORDS\s+(\d+)", text)
    assert words and int(words.group(1)) == B.CYL_FLAG_WORDS
    from taseg_amd.data import cylinder as C
    for name, value in (("NONFINITE", C.FLAG_NONFINITE), ("LABEL", C.FLAG_LABEL), ("RANGE", C.FLAG_RANGE)):
        assert int(re.search(r"#define\s+TS_CYL_FLAG_%s\s+(\d+)" % name, text).group(1)) == value


def test_the_new_file_is_built_without_contraction():
    from taseg_amd.csrc import build
    assert "cylinder_stage.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["cylinder_stage.hip"]


# ------------------------------------------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("lo, hi, grid", [([0, -180, -4], [50, 180, 2], [480, 360, 32]), ([0, -180, -4], [50, 180, 2], [96, 80, 16]),
                                          ([5, -90, -1.5], [20, 90, 0.5], [32, 24, 8]), ([0.5, -180.0, -3.0], [51.2, 180.0, 1.8], [7, 11, 3])])
def test_grid_intervals_are_the_references_doubles(lo, hi, grid):
    from taseg_amd.data import CylinderGrid
    cg = CylinderGrid(lo, hi, grid)
    want = (np.array(hi) - np.array(lo)) / (np.array(grid) - 1)            # semantickitti_cylinder.py:149-151
    assert cg.intervals.dtype == np.float64 and np.array_equal(cg.intervals, want)
    assert np.array_equal(cg.space(), np.concatenate([np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64), want]))
    assert CylinderGrid(np.array(lo), np.array(hi), np.array(grid)) == cg  # numpy numbers are taken as the numbers they hold
    with pytest.raises(Exception):
        cg.grid_size = (1, 2, 3)                                           # frozen
    assert hash(cg) == hash(CylinderGrid(tuple(lo), tuple(hi), tuple(grid)))


def test_grid_refuses_what_has_no_cells():
    from taseg_amd.data import CylinderGrid
    with pytest.raises(ValueError):
        CylinderGrid([0, -180, -4], [50, 180, 2], [480, 360, 1])
    with pytest.raises(ValueError):
        CylinderGrid([0, 180, -4], [50, 180, 2], [480, 360, 32])
    with pytest.raises(TypeError):
        CylinderGrid([0, -180], [50, 180, 2], [480, 360, 32])


# ------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(g, tag):
    R.check_against_reference(R.restated(g, tag), R.reference(g, tag), float(g["phi_ref_ulp"]), tag)


def test_restatement_reproduces_the_model_fixtures_batch(g):
    m = dict(np.load(os.path.join(GOLDEN, "model_cylinder.npz"), allow_pickle=False))
    scans = [synth_scan(seed, n_points=1000, n_beams=16, n_az=360) for seed in (33, 34)]       # make_golden_cylinder.py:36, :87-89
    got = R.restate_batch([p for p, _ in scans], [l.astype(np.int64) for _, l in scans], [0, -180, -4], [50, 180, 2], m["grid"].tolist())
    ref = {k: m["batch_" + k] for k in R.KEYS if k != "voxel_feature"}
    inds = np.concatenate([p["inds"] + o for p, o in zip(got["parts"], (0, 1000))])
    ref["voxel_feature"] = ref["point_feature"][inds]                      # (that fixture does not store it: the model never reads it)
    assert len(ref["point_coord"]) == 2000
    R.check_against_reference(got, ref, float(g["phi_ref_ulp"]), "model_cylinder")


def test_each_wrong_reading_misses_the_fixture(g):
    """a dropped + 0.5, cell arithmetic in float32 and interval = range / grid are each caught by the fixture"""
    def misses(defect):
        bad = []
        for tag in CASES:
            got, ref = R.restated(g, tag, defect=defect), R.reference(g, tag)
            same = np.array_equal(got["point_coord"], ref["point_coord"].astype(np.int64)) and np.array_equal(
                np.delete(got["point_feature"], R.PHI_COLUMN, 1).view(np.uint32), np.delete(ref["point_feature"], R.PHI_COLUMN, 1).view(np.uint32))
            if not same:
                bad.append(tag)
        return bad
    assert misses(None) == []
    for defect in ("no_half", "float32_cells", "range_over_grid"):
        caught = misses(defect)
        print(defect, "caught by", caught)
        assert caught, defect


# ------------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_conditions(g):
    assert float(g["phi_ref_ulp"]) > 0.5                                   # the reference's phi_deg is NOT the rounded float64 value
    for tag in CASES:
        pts = R.case_inputs(g, tag)[0]
        assert all(990 <= len(p) <= 1000 and p.dtype == np.float32 for p in pts), tag      # at most 1 % of a scan removed
        assert not any(k.startswith(tag + "_") and "mask" in k for k in g)
        assert np.array_equal(R.restated(g, tag)["point_coord"], g[f"{tag}_point_coord"].astype(np.int64)), tag   # EVERY row
    b = R.restated(g, "b")["parts"][0]
    top = b["counter"].max(1)
    assert (((b["counter"] == top[:, None]).sum(1) > 1) & (top > 0)).sum() >= 1            # a voxel tied at the top
    assert (top == 0).sum() >= 1                                                           # a voxel of ignored points only
    assert np.bincount(b["inverse_map"]).max() > 16                                        # a run longer than 16 rows
    assert 0.05 < (g["b_labels0"] == 67).mean() < 0.2
    pol, lo, hi = R.polar(g["c_points0"]), g["c_space_min"], g["c_space_max"]
    for d in range(3):
        assert (pol[:, d] < lo[d]).any() and (pol[:, d] > hi[d]).any(), d                  # clipped on all six faces
    pc = g["c_point_coord"][:, :3]
    assert (pc.min(0) == 0).all() and (pc.max(0) == g["c_grid"] - 1).all()
    assert int(g["d_views"]) == 3 and len(g["d_point_coord"]) == 3 * len(g["d_points0"])
    assert sorted(set(g["d_point_coord"][:, 3].tolist())) == [0, 1, 2]
    assert bool(g["a_rotate"]) and not bool(g["a2_rotate"])


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_cpu_tensors_and_oversized_batches_fail_loudly():
    import torch
    from taseg_amd.data import CylinderGrid, build_cylinder_batch, build_cylinder_tta_batch
    from taseg_amd import backend as B
    grid = CylinderGrid([0, -180, -4], [50, 180, 2], [96, 80, 16])
    scan = {"points": torch.zeros((5, 4)), "labels": torch.zeros(5, dtype=torch.int64), "name": "s"}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_cylinder_batch([scan], grid)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_cylinder_tta_batch(scan, 0, 3, np.random.RandomState(0), grid)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.cylinder_cells(scan["points"], grid.space())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.cylinder_voxels(torch.zeros((5, 4), dtype=torch.int32), scan["labels"], 1)
    with pytest.raises(ValueError, match="0 <= batch < 1024"):
        build_cylinder_batch([scan] * 1025, grid)
    with pytest.raises(ValueError, match="no scans"):
        build_cylinder_batch([], grid)
