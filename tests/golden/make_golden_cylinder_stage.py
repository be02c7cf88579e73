"""Golden vectors of the cylinder data stage (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_cylinder_stage.py        ->  tests/golden/cylinder_stage.npz  (data only)

The REAL reference's dataset code - SemkittiCylinderDataset.get_single_sample, voxelize_with_label, collate_batch, collate_batch_tta
(pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:104-249) and its torchsparse sparse_quantize - runs on the CPU through
the import environment of _ref_env.py, exactly as make_golden_cylinder.py:67-90 drives it: an `object.__new__` dataset over a list
of `xyzret` / `labels` / `path` dicts; no reference code in this file.  `np.random.seed(s)` precedes every case, so
`np.random.RandomState(s)` reproduces its draws (taseg_amd/data/augment.py).

Inputs: synth_scan(seed, n_points=1000, n_beams=16, n_az=360), stored.  Cases:
  a_   training batch of 3 scans, grid 96 x 80 x 16, FLIP / SCALE / TRANSFORM / ROTATE on;   a2_  the same with ROTATE_AUG off
       (the scale multiplies the float32 cloud in float32)
  b_   the vote: one scan on a coarse 24 x 20 x 8 grid over the recipe's space, ~10 % of the labels set to 67 and every point of two
       voxels set to 67
  c_   clipping: the space [5, -90, -1.5] .. [20, 90, 0.5] - rows beyond both ends of every axis
  d_   three TTA views of one scan through collate_batch_tta

Conditions, asserted here and again in tests/test_cylinder_stage_host.py: the numpy restatement with the device's phi rule
(tests/cylinder_stage_ref.py) gives the reference's `point_coord` at EVERY row of every case - a row whose cell differs is removed
from its input scan before anything is stored (at most 1 % of a scan; no exclusion mask is stored); case b holds a voxel tied at the
top, a voxel of ignored points only and a run longer than 16 rows; case c holds clipped rows on all six faces.  `phi_ref_ulp`: the
largest distance, in float32 ulp, of the reference's own `phi_deg` from the float64 value arctan2(y, x) / pi * 180 of the float32
rows it was computed from.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_env  # noqa: E402
import cylinder_stage_ref as R  # noqa: E402
from taseg_amd.data.augment import draw_train_params, draw_tta_params  # noqa: E402
from taseg_amd.data.synthetic import synth_scan  # noqa: E402

torch.set_num_threads(1)
POINTS, SCALE_RANGE = 1000, [0.95, 1.05]
RECIPE_MIN, RECIPE_MAX = [0, -180, -4], [50, 180, 2]
CASES = {
    "a": dict(seeds=(41, 42, 43), space_min=RECIPE_MIN, space_max=RECIPE_MAX, grid=[96, 80, 16], draw_seed=7, rotate=True),
    "a2": dict(seeds=(41, 42, 43), space_min=RECIPE_MIN, space_max=RECIPE_MAX, grid=[96, 80, 16], draw_seed=8, rotate=False),
    "b": dict(seeds=(44,), space_min=RECIPE_MIN, space_max=RECIPE_MAX, grid=[24, 20, 8]),
    "c": dict(seeds=(45,), space_min=[5, -90, -1.5], space_max=[20, 90, 0.5], grid=[32, 24, 8]),
    "d": dict(seeds=(46,), space_min=RECIPE_MIN, space_max=RECIPE_MAX, grid=[96, 80, 16], draw_seed=9, views=3),
}


class FreshScans(list):
    """the scans of a case; every access hands out copies, as the reference's file-backed dataset does (get_single_sample augments
    the rows it was handed in place, :115, :132)"""

    def __getitem__(self, i):
        d = list.__getitem__(self, i)
        return {"xyzret": d["xyzret"].copy(), "labels": d["labels"].copy(), "path": d["path"]}


def setup():
    _ref_env.setup_torchsparse()
    _ref_env.setup_pcseg()
    for alias, typ in (("int", int), ("bool", bool), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)                              # aliases numpy >= 1.24 dropped (semantickitti_cylinder.py:153)
    from pcseg.data.dataset.semantickitti.semantickitti_cylinder import SemkittiCylinderDataset
    return SemkittiCylinderDataset


def dataset(cls, case, scans):
    ds = object.__new__(cls)
    ds.class_names = ["c%d" % i for i in range(20)]
    ds.cylinder_space_max, ds.cylinder_space_min = np.array(case["space_max"]), np.array(case["space_min"])
    ds.grid_size = np.array(case["grid"])
    ds.training, ds.if_tta = "rotate" in case, "views" in case
    ds.if_flip = ds.if_scale = ds.if_jitter = True
    ds.if_rotate = case.get("rotate", True)
    ds.scale_axis, ds.scale_range = "xyz", SCALE_RANGE
    ds.point_cloud_dataset = FreshScans({"xyzret": p, "labels": l, "path": name} for p, l, name in scans)
    return ds


def run_reference(cls, case, scans):
    ds = dataset(cls, case, scans)
    if "draw_seed" in case:
        np.random.seed(case["draw_seed"])
    if "views" in case:
        return cls.collate_batch_tta([[ds.get_single_sample(0, v) for v in range(case["views"])]])
    return cls.collate_batch([ds.get_single_sample(i) for i in range(len(scans))])


def draws(case):
    if "draw_seed" not in case:
        return None
    rng = np.random.RandomState(case["draw_seed"])
    if "views" in case:
        return [draw_tta_params(rng, v, SCALE_RANGE) for v in range(case["views"])]
    return [draw_train_params(rng, True, True, SCALE_RANGE, True, case["rotate"]) for _ in case["seeds"]]


def restate(case, scans):
    views = case.get("views", 1)
    pts, labs = [p for p, _, _ in scans] * views, [l for _, l, _ in scans] * views
    return R.restate_batch(pts, labs, case["space_min"], case["space_max"], case["grid"], aug=draws(case))


def vote_labels(case, point, label):
    """case b's labels: ~10 % ignored, and every point of the two most populated voxels but one ignored"""
    rs = np.random.RandomState(1)
    label = label.copy()
    label[rs.rand(len(label)) < 0.10] = 67
    part = R.restate_sample(point, label, case["space_min"], case["space_max"], case["grid"])
    size = np.bincount(part["inverse_map"])
    for v in np.argsort(-size, kind="stable")[1:3]:
        label[part["inverse_map"] == v] = 67
    return label


def main(fname="cylinder_stage.npz"):
    cls = setup()
    out, worst = {}, 0.0
    for tag, case in CASES.items():
        scans = []
        for seed in case["seeds"]:
            pts, lab = synth_scan(seed, n_points=POINTS, n_beams=16, n_az=360)
            lab = lab.astype(np.int64)
            if tag == "b":
                lab = vote_labels(case, pts, lab)
            scans.append((pts, lab, "scan%d" % seed))
        # rows whose cell differs under the device's phi rule leave the INPUT (at most 1 % of a scan), then everything is recomputed
        for _ in range(4):
            ref, mine = run_reference(cls, case, scans), restate(case, scans)
            differ = (ref["point_coord"].numpy() != mine["point_coord"]).any(1)
            if not differ.any():
                break
            n0, kept = 0, []
            for p, l, name in scans:
                bad = np.zeros(len(p), dtype=bool)
                for v in range(case.get("views", 1)):
                    bad |= differ[n0 + v * len(p):n0 + (v + 1) * len(p)] if "views" in case else differ[n0:n0 + len(p)]
                n0 += len(p)
                assert bad.sum() <= len(p) // 100, (tag, name, int(bad.sum()))
                kept.append((p[~bad], l[~bad], name))
            scans = kept
        assert not differ.any(), tag
        for k in R.KEYS:
            got = ref[k].numpy()
            if k == "point_feature" or k == "voxel_feature":
                same = np.delete(got, R.PHI_COLUMN, 1).view(np.uint32) == np.delete(mine[k], R.PHI_COLUMN, 1).view(np.uint32)
                assert same.all(), (tag, k)
            else:
                assert got.dtype == mine[k].dtype and np.array_equal(got, mine[k]), (tag, k)
        # the reference's own phi_deg against float64, on the float32 rows it was computed from (columns 6, 7 of its features)
        feat = ref["point_feature"].numpy()
        exact = R.phi_deg64(feat[:, 6:8])
        worst = max(worst, float((np.abs(feat[:, R.PHI_COLUMN].astype(np.float64) - exact) / R.ulp32(exact)).max()))
        mine_phi = mine["point_feature"][:, R.PHI_COLUMN].astype(np.float64)
        assert (np.abs(mine_phi - exact) <= 2.07e-7 * np.abs(exact)).all(), tag
        for b, (p, l, name) in enumerate(scans):
            out[f"{tag}_points{b}"], out[f"{tag}_labels{b}"] = p, l
        out[f"{tag}_names"] = np.array([name for _, _, name in scans])
        for k in ("space_min", "space_max", "grid"):
            out[f"{tag}_{k}"] = np.array(case[k])
        for k in ("draw_seed", "views", "rotate"):
            if k in case:
                out[f"{tag}_{k}"] = np.array(case[k])
        for k in R.KEYS:
            out[f"{tag}_{k}"] = ref[k].numpy()
        out[f"{tag}_point_coord"] = out[f"{tag}_point_coord"].astype(np.int32)
        out[f"{tag}_voxel_coord"] = out[f"{tag}_voxel_coord"].astype(np.int32)
        del out[f"{tag}_voxel_feature"]                          # = point_feature[inds]: asserted here, rebuilt by the tests
        inds = np.concatenate([p["inds"] + o for p, o in zip(mine["parts"], np.cumsum([0] + [len(p["point_coord"]) for p in mine["parts"]]))])
        assert np.array_equal(ref["voxel_feature"].numpy().view(np.uint32), feat[inds].view(np.uint32)), tag
        out[f"{tag}_inds"] = inds.astype(np.int32)
        print(tag, "points", len(feat), "voxels", len(inds), "rows removed", POINTS * len(scans) - sum(len(p) for p, _, _ in scans))
        if tag == "b":
            counter = mine["parts"][0]["counter"]
            top = counter.max(1)
            tied = int((((counter == top[:, None]).sum(1) > 1) & (top > 0)).sum())
            ignored = int((top == 0).sum())
            longest = int(np.bincount(mine["inverse_map"]).max())
            print("  vote: tied at the top", tied, "all ignored", ignored, "longest run", longest, "ignored rows", int((scans[0][1] == 67).sum()))
            assert tied >= 1 and ignored >= 1 and longest > 16
        if tag == "c":
            pc, g = out["c_point_coord"][:, :3], np.array(case["grid"])
            pol = R.polar(scans[0][0])
            faces = [int((pol[:, d] < case["space_min"][d]).sum()) for d in range(3)] + [int((pol[:, d] > case["space_max"][d]).sum()) for d in range(3)]
            print("  clipped rows below / above per axis", faces)
            assert min(faces) >= 1 and (pc.min(0) == 0).all() and (pc.max(0) == g - 1).all()
    out["phi_ref_ulp"] = np.array(worst)
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB; the reference's phi_deg is up to %.2f float32 ulp from the float64 value" % worst)


if __name__ == "__main__":
    main()
