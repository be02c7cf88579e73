"""The host side of the nuScenes TIAF stage's augmentation and TTA views (taseg_amd/data/nuscenes_tiaf.py) against the fixture the
REAL reference produced (tests/golden/tiaf_nus_aug.npz; its inputs are those of tests/golden/tiaf_nus.npz): the draws, the record
table's layout, and the two row rules the kernel adds behind the projection - augmentation and clamp - restated in numpy."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from taseg_amd.data import augment as A
from taseg_amd.data import nuscenes_tiaf as T

VOXEL = 0.1


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_nus.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_nus_aug.npz"), allow_pickle=False))


def train_params(ga, case):
    """the case's AugParams, one per sample, drawn as the stage's caller draws them: one generator, one sample after the other"""
    flip, scale, jitter, rotate = (bool(v) for v in ga[f"{case}_switches"])
    rng = np.random.RandomState(int(ga[f"{case}_seed"]))
    return [A.draw_train_params(rng, flip=flip, scale=scale, jitter=jitter, rotate=rotate) for _ in range(2)]


def tta_params(ga):
    rng = np.random.RandomState(int(ga["tta_seed"]))
    return [A.draw_tta_params(rng, v) for v in range(*ga["tta_votes"].tolist())]


@pytest.mark.parametrize("case", ["train", "norot"])
def test_training_draws_reproduce_the_reference(ga, case):
    params = train_params(ga, case)
    assert [p.theta for p in params] == ga[f"{case}_theta"].tolist()
    assert [p.scale for p in params] == ga[f"{case}_scale"].tolist()
    assert [p.flip for p in params] == ga[f"{case}_flip"].tolist()
    assert [list(p.translate) for p in params] == ga[f"{case}_noise"].tolist()
    rotate = bool(ga[f"{case}_switches"][3])
    assert all(p.rotate_on == rotate and bool(p.bits & A.SCALE_F32) == (not rotate) for p in params)


def test_tta_draws_reproduce_the_reference(ga):
    """one scale per vote and nothing else: NuscenesMsMmDataset.__getitem__ draws no mix coin"""
    params = tta_params(ga)
    votes = range(*ga["tta_votes"].tolist())
    assert [p.theta for p in params] == ga["tta_theta"].tolist() == [A.TTA_ANGLES[v] * np.pi / 8.0 for v in votes]
    assert [p.scale for p in params] == ga["tta_scale"].tolist()
    assert not any(p.flip_on or p.translate_on for p in params)


def test_record_table_has_the_headers_layout(tmp_path):
    from taseg_amd import backend as B
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    names = T.CAM_FRAME_DTYPE.names
    offs = ", ".join(f"offsetof(TsNuscCamFrame, {n})" for n in names)
    fmt = " ".join(["%zu"] * (1 + len(names)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "taseg_hip.h"\nint main(void) {\n'
                   f'  printf("{fmt}\\n", sizeof(TsNuscCamFrame), {offs});\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert seen == [T.CAM_FRAME_DTYPE.itemsize] + [T.CAM_FRAME_DTYPE.fields[n][1] for n in names]
    assert B.NUSC_CAM_FRAME_BYTES == T.CAM_FRAME_DTYPE.itemsize == 584
    assert T.CAM_FRAME_DTYPE["cam"].shape == (57,) and T.CAM_FRAME_DTYPE["move"].shape == (12,)
    assert ctypes.sizeof(ctypes.c_double) * (57 + 12) == T.CAM_FRAME_DTYPE.fields["row_offset"][1]


class TsNuscCamFrame(ctypes.Structure):
    """include/taseg_hip.h's struct, field for field"""
    _fields_ = [("cam", ctypes.c_double * 57), ("move", ctypes.c_double * 12), ("row_offset", ctypes.c_float),
                ("paint_dist", ctypes.c_float), ("sample", ctypes.c_int32), ("img_w", ctypes.c_int32), ("img_h", ctypes.c_int32),
                ("crop_top", ctypes.c_int32), ("first", ctypes.c_int32), ("src", ctypes.c_int32)]


def test_record_table_matches_a_ctypes_mirror_of_the_struct():
    """the same layout check without a C compiler: the platform's C layout rules through ctypes"""
    names = [f[0] for f in TsNuscCamFrame._fields_]
    assert list(T.CAM_FRAME_DTYPE.names) == names
    assert ctypes.sizeof(TsNuscCamFrame) == T.CAM_FRAME_DTYPE.itemsize
    assert [getattr(TsNuscCamFrame, n).offset for n in names] == [T.CAM_FRAME_DTYPE.fields[n][1] for n in names]
    assert [getattr(TsNuscCamFrame, n).size for n in names] == [T.CAM_FRAME_DTYPE.fields[n][0].itemsize for n in names]
    with open(os.path.join(ROOT, "include", "taseg_hip.h")) as f:
        body = f.read().split("typedef struct TsNuscCamFrame {")[1].split("} TsNuscCamFrame;")[0]
    declared = [part.strip().split("[")[0] for line in body.splitlines() if ";" in line
                for part in line.split(";")[0].split(None, 1)[1].split(",")]
    assert declared == names                                   # the mirror lists the header's fields, in the header's order


def test_tta_batch_without_votes_is_refused():
    with pytest.raises(ValueError, match="no votes"):
        T.build_nusc_tiaf_tta_batch({}, 3, 3, np.random.RandomState(0))
    with pytest.raises(ValueError, match="no samples"):
        T.build_nusc_tiaf_batch_from_keyframes([])


# ---------------------------------------------------------------------------------------- rules (e) and (f) in numpy
def _fma(a, b, c):
    """a * b + c with ONE rounding, element by element (exact rational arithmetic; Fraction -> float rounds correctly)"""
    b, c = np.broadcast_to(np.asarray(b, dtype=np.float64), a.shape), np.broadcast_to(np.asarray(c, dtype=np.float64), a.shape)
    return np.array([float(Fraction(float(u)) * Fraction(float(v)) + Fraction(float(w))) for u, v, w in zip(a, b, c)])


def augment(xyz32, p):
    """rule (e): float64 in the reference's order, the rotation as np.dot's fused-multiply-add chain, ONE rounding to float32;
    without the rotation the scale multiplies in float32; a step that is off is skipped"""
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


def fov_voxels(g, b, p):
    """{voxel: feature row} of sample b's FOV cloud under p: tiaf_nus.npz's un-augmented `xyzret_fov_ms` through rule (e), rule (f)
    against the augmented single-frame cloud's corner, then rounded and shifted by the augmented, clamped fused cloud's minimum
    (nuscenes_voxel_ms_mm.py:92-140, 184-193); a voxel's row is its first point"""
    fov = g[f"b{b}_xyzret_fov_ms"].copy()
    fov[:, :3] = augment(fov[:, :3], p)
    point, fused = augment(g[f"b{b}_xyzret"][:, :3], p), augment(g[f"b{b}_xyzret_ms"][:, :3], p)
    lo = point.min(0)
    fused = fused[(fused >= lo).all(1)]
    kept = fov[(fov[:, :3] >= lo).all(1)]                                           # rule (f)
    shift = np.round(fused / VOXEL).astype(np.int32).min(0)
    pc = np.round(kept[:, :3] / VOXEL).astype(np.int32) - shift
    out = {}
    for c, row in zip(map(tuple, pc.tolist()), kept):
        out.setdefault(c, row)
    return out, len(fov) - len(kept)


def _check(ga, prefix, b, entry, want, removed):
    C, F = ga[prefix + "lidar_fov_ms_C"], ga[prefix + "lidar_fov_ms_F"]
    mine = C[:, 3] == entry
    assert removed > 0 and len(want) == int(mine.sum()) > 0, (prefix, b, entry)
    for c, row in zip(map(tuple, C[mine, :3].tolist()), F[mine]):
        assert row.tobytes() == want[c].tobytes(), (prefix, b, entry, c)


@pytest.mark.parametrize("case", ["train", "norot"])
def test_augmentation_and_clamp_restated_reproduce_the_fov_cloud(g, ga, case):
    for b, p in enumerate(train_params(ga, case)):
        want, removed = fov_voxels(g, b, p)
        _check(ga, f"{case}_batch_", b, b, want, removed)
        assert removed == int(ga[f"{case}_fov_removed_kept"][b][0])


def test_tta_views_restated_reproduce_the_fov_cloud(g, ga):
    for i, p in enumerate(tta_params(ga)):
        want, removed = fov_voxels(g, int(ga["tta_sample"]), p)
        _check(ga, "tta_batch_", int(ga["tta_sample"]), i, want, removed)


def test_cases_share_the_inputs_of_the_unaugmented_fixture(g, ga):
    """the new fixture stores draws and outputs alone, and is the smaller file"""
    assert not any(k.startswith(("b0_", "b1_")) for k in ga)
    assert os.path.getsize(os.path.join(GOLDEN, "tiaf_nus_aug.npz")) <= os.path.getsize(os.path.join(GOLDEN, "tiaf_nus.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "tiaf_nus_aug.npz")) < 1 << 20
    for case in ("train", "norot", "tta"):
        assert (ga[f"{case}_fov_removed_kept"][:, 0] > 0).all() and (ga[f"{case}_fov_removed_kept"][:, 1] > 0).all()
