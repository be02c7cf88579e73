"""The cylinder data stage restated in numpy with the rules of include/taseg_hip.h (ts_cylinder_cells, ts_cylinder_voxels): what
tests/test_cylinder_stage_host.py checks against the real reference's output (tests/golden/cylinder_stage.npz, model_cylinder.npz) and
tests/test_gpu_cylinder_stage.py checks the device against, bit for bit.  Shared with tests/golden/make_golden_cylinder_stage.py, which
asserts the fixture conditions with it.  No reference code here: semantickitti_cylinder.py:104-219 is the specification.

The one rule that is NOT the reference's: phi = float32(arctan2(float64(y), float64(x))) - numpy's float32 arctan2 is not correctly
rounded; every other step is the reference's arithmetic in the reference's precision."""
from fractions import Fraction

import numpy as np

from taseg_amd.data.augment import draw_tta_params, draw_train_params

KEYS = ("point_coord", "voxel_coord", "point_feature", "voxel_feature", "point_label", "voxel_label", "inverse_map", "num_points",
        "offset")
PHI_COLUMN = 4
SCALE_RANGE = [0.95, 1.05]
# phi_deg against float64: three float32 roundings (the arc tangent, the division, the product: 2^-24 each = 1.79e-7) + float32(pi)'s
# relative distance of 2.78e-8 from pi
PHI_BOUND = 2.07e-7


def _fma(a, b, c):
    """a * b + c with ONE rounding, element by element (exact rational arithmetic)"""
    b, c = np.broadcast_to(np.asarray(b, dtype=np.float64), a.shape), np.broadcast_to(np.asarray(c, dtype=np.float64), a.shape)
    return np.array([float(Fraction(float(u)) * Fraction(float(v)) + Fraction(float(w))) for u, v, w in zip(a, b, c)])


def augment(xyz32, p):
    """aug_points (seg_utils.py:43-100) under the AugParams p, stored back into float32 rows: float64 in the reference's order, the
    rotation as np.dot's fused-multiply-add chain in k order, ONE rounding; without the rotation the scale multiplies in float32; a
    step that is off is skipped"""
    x, y, z = (xyz32[:, i].astype(np.float64) for i in range(3))
    if p.rotate_on:
        x, y = _fma(y, -p.s, x * p.c), _fma(y, p.c, x * p.s)
    if p.scale_on:
        if p.rotate_on:
            x, y, z = x * p.scale, y * p.scale, z * p.scale
        else:
            f = np.float32(p.scale)
            x, y, z = ((v.astype(np.float32) * f).astype(np.float64) for v in (x, y, z))
    if p.flip_on:
        x, y = (-x if p.flip & 1 else x), (-y if p.flip & 2 else y)
    if p.translate_on:
        x, y, z = x + p.translate[0], y + p.translate[1], z + p.translate[2]
    return np.stack([x, y, z], 1).astype(np.float32)


def phi_deg64(point):
    """arctan2(y, x) / pi * 180 in float64 of the stored float32 rows: what `phi_deg` is measured against"""
    return np.arctan2(point[:, 1].astype(np.float64), point[:, 0].astype(np.float64)) / np.pi * 180.0


def ulp32(value):
    """the float32 ulp at |value| (float64 array)"""
    return np.spacing(np.abs(value).astype(np.float32)).astype(np.float64)


def polar(point):
    """float32 [n, 3]: rho, phi in degrees, z (:19-22, :144-145) with the header's phi"""
    x, y = point[:, 0], point[:, 1]
    rho = np.sqrt(x ** 2 + y ** 2)
    phi = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    pol = np.stack((rho, phi, point[:, 2]), axis=1)
    pol[:, 1] = pol[:, 1] / np.pi * 180.
    assert pol.dtype == np.float32
    return pol


def restate_sample(point, label, space_min, space_max, grid_size, num_classes=20, ignore_label=67, defect=None):
    """One sample (:144-172).  defect: None, or one wrong reading of the reference switched on - "no_half" (the + 0.5 of the centres
    dropped), "float32_cells" (the clip and the cell arithmetic kept in float32), "range_over_grid" (interval = range / grid)."""
    pol = polar(point)
    max_bound, min_bound, grid = np.array(space_max), np.array(space_min), np.array(grid_size)
    intervals = (max_bound - min_bound) / (grid if defect == "range_over_grid" else grid - 1)
    if defect == "float32_cells":
        lo32, hi32 = min_bound.astype(np.float32), max_bound.astype(np.float32)
        cell = np.floor((np.clip(pol, lo32, hi32) - lo32) / intervals.astype(np.float32)).astype(np.int64)
    else:
        cell = np.floor((np.clip(pol, min_bound, max_bound) - min_bound) / intervals).astype(np.int64)
    # torchsparse's sparse_quantize: np.unique of the ravelled (x, y, z) - ascending, first occurrence, inverse
    c0 = cell - cell.min(0)
    span = c0.max(0) + 1
    key = (c0[:, 0] * span[1] + c0[:, 1]) * span[2] + c0[:, 2]
    _, inds, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    label = np.asarray(label).astype(np.int64)
    counted = label != ignore_label
    if ((label[counted] < 0) | (label[counted] >= num_classes)).any():
        raise IndexError("label outside [0, num_classes)")
    counter = np.zeros((len(inds), num_classes), dtype=np.int64)
    np.add.at(counter, (inverse[counted], label[counted]), 1)
    voxel_label = np.argmax(counter, axis=1)
    half = 0.0 if defect == "no_half" else 0.5
    centre = (cell.astype(np.float32) + half) * intervals + min_bound
    feature = np.concatenate([centre, pol, point[:, :2], point[:, 3:]], axis=1).astype(np.float32)
    return {"point_coord": cell, "voxel_coord": cell[inds], "point_feature": feature, "voxel_feature": feature[inds],
            "point_label": label, "voxel_label": voxel_label.astype(np.int64), "inverse_map": inverse.astype(np.int64), "inds": inds,
            "counter": counter}


def restate_batch(points, labels, space_min, space_max, grid_size, aug=None, **kw):
    """collate_batch / collate_batch_tta (:176-249) of the samples; aug: one AugParams per sample or None"""
    parts = []
    for b, (point, label) in enumerate(zip(points, labels)):
        point = point.copy()
        if aug is not None:
            point[:, :3] = augment(point[:, :3], aug[b])
        parts.append(restate_sample(point, label, space_min, space_max, grid_size, **kw))
    pad = lambda a, b: np.concatenate([a, np.full((len(a), 1), b, a.dtype)], 1)  # noqa: E731
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("point_feature", "voxel_feature", "point_label", "voxel_label", "inverse_map")}
    out["point_coord"] = np.concatenate([pad(p["point_coord"], b) for b, p in enumerate(parts)])
    out["voxel_coord"] = np.concatenate([pad(p["voxel_coord"], b) for b, p in enumerate(parts)])
    out["num_points"] = np.array([len(p["point_coord"]) for p in parts], dtype=np.int64)
    out["offset"] = np.cumsum([len(p["voxel_coord"]) for p in parts]).astype(np.int32)
    out["parts"] = parts
    return out


# ---------------------------------------------------------------------------------------------- the fixture's cases and the comparison
def case_inputs(g, tag):
    """(points, labels, names, space_min, space_max, grid, aug) of a case; a TTA case lists its scan once per view"""
    n = len(g[f"{tag}_names"])
    pts, labs = [g[f"{tag}_points{b}"] for b in range(n)], [g[f"{tag}_labels{b}"] for b in range(n)]
    names = g[f"{tag}_names"].tolist()
    aug = None
    if f"{tag}_draw_seed" in g:
        rng = np.random.RandomState(int(g[f"{tag}_draw_seed"]))
        if f"{tag}_views" in g:
            views = int(g[f"{tag}_views"])
            aug = [draw_tta_params(rng, v, SCALE_RANGE) for v in range(views)]
            pts, labs, names = pts * views, labs * views, names * views
        else:
            aug = [draw_train_params(rng, True, True, SCALE_RANGE, True, bool(g[f"{tag}_rotate"])) for _ in range(n)]
    return pts, labs, names, g[f"{tag}_space_min"].tolist(), g[f"{tag}_space_max"].tolist(), g[f"{tag}_grid"].tolist(), aug


def restated(g, tag, **kw):
    pts, labs, _, lo, hi, grid, aug = case_inputs(g, tag)
    return restate_batch(pts, labs, lo, hi, grid, aug=aug, **kw)


def reference(g, tag):
    ref = {k: g[f"{tag}_{k}"] for k in KEYS if k != "voxel_feature"}
    ref["voxel_feature"] = ref["point_feature"][g[f"{tag}_inds"]]          # (the maker asserts this IS the reference's voxel_feature)
    return ref


def check_against_reference(got, ref, phi_ref_ulp, who):
    """every integer key and 8 of the feature columns equal; phi_deg within PHI_BOUND of float64 and that + phi_ref_ulp of the reference"""
    for k in ("point_coord", "voxel_coord", "point_label", "voxel_label", "inverse_map", "num_points", "offset"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), ref[k].astype(np.int64)), (who, k)
    for k in ("point_feature", "voxel_feature"):
        a, b = np.asarray(got[k]), ref[k]
        assert a.dtype == np.float32 and a.shape == b.shape, (who, k)
        assert np.array_equal(np.delete(a, PHI_COLUMN, 1).view(np.uint32), np.delete(b, PHI_COLUMN, 1).view(np.uint32)), (who, k)
        exact = phi_deg64(b[:, 6:8])                                     # columns 6, 7: the float32 x, y the polar transform read
        err64 = np.abs(a[:, PHI_COLUMN].astype(np.float64) - exact)
        err_ref = np.abs(a[:, PHI_COLUMN].astype(np.float64) - b[:, PHI_COLUMN].astype(np.float64))
        print(f"{who} {k}: phi_deg max |got - float64| / |float64| {np.max(err64 / np.maximum(np.abs(exact), 1e-300)):.3e}, "
              f"max |got - reference| {np.max(err_ref / ulp32(exact)):.2f} ulp, rows that differ {int((err_ref > 0).sum())}")
        assert (err64 <= PHI_BOUND * np.abs(exact)).all(), (who, k)
        assert (err_ref <= PHI_BOUND * np.abs(exact) + phi_ref_ulp * ulp32(exact)).all(), (who, k)
