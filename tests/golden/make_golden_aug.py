"""Golden vectors of the point augmentation and the TTA views (build container only; reads /root/reference).

    python tests/golden/make_golden_aug.py

Runs the REAL reference dataset code - `get_single_sample` of semantickitti_voxel_ms.py, nuscenes_voxel_ms.py and
semantickitti_voxel.py with `training=True` / `TTA: True`, which call `aug_points_ms` / `aug_points`
(tools/utils/common/seg_utils.py:43-166) - on the inputs already stored in multiscan.npz / multiscan_nus.npz, after
`np.random.seed(seed)`.  Stored (data only): the seeds, the values the reference DREW (numpy's generator functions are wrapped
while it runs: theta, scale, flip type, noise), the augmented xyz of `point` / `point_ms` and the collated batches under the keys
of multiscan.npz.

  multiscan_aug.npz       SemanticKITTI multi-scan, training: all four augmentations (seeds 0, 2, 4: flip types 0 .. 3; seed 0 as a
                          batch of two samples), rotate only, nothing enabled (asserted equal to multiscan.npz, not stored again)
  multiscan_aug_tta.npz   one TTA batch, votes 0 .. 9 (collate_batch_tta)
  multiscan_aug_misc.npz  scale + translation WITHOUT rotation (the one combination numpy scales in float32); one nuScenes multi-scan
                          training sample; one single-frame `aug_points` sample (semantickitti_voxel.py)
(three files: together they pass the repository's limit for one committed file.  The coordinates of `targets` / `targets_ms` /
`targets_mapped` are those of `lidar` / `lidar_ms` / `inverse_map` - asserted here, stored once.)

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through taseg_amd.data.augment's draw
functions gives the recorded draws, and the float64 formula of ts_stage_augment (include/taseg_hip.h; the rotation as the
fused-multiply-add chain np.dot performs) applied to the input cloud gives the reference's float32 xyz bit for bit.
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_r2 as R2  # noqa: E402  (arranges the reference's imports; the pyquaternion stand-in)

_ref_env = R2._ref_env
from taseg_amd.data import augment as A  # noqa: E402

VOXEL = 0.05
BATCH_SPARSE = ("lidar", "lidar_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms")       # the keys of multiscan.npz
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map"}   # stored once: asserted equal here
BATCH_DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask")


def dump_batch(prefix, batch):
    out = {}
    for key in BATCH_SPARSE:
        if key in SAME_COORDS:
            assert np.array_equal(batch[key].C.numpy(), batch[SAME_COORDS[key]].C.numpy()), key
        else:
            out[f"{prefix}{key}_C"] = batch[key].C.numpy()
        out[f"{prefix}{key}_F"] = batch[key].F.numpy()
    for key in BATCH_DENSE:
        out[f"{prefix}{key}"] = batch[key].numpy()
    return out


class Frames(list):
    """the frame reader hands out fresh arrays on every access (it reads files); the voxel datasets augment in place"""

    def __getitem__(self, i):
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in list.__getitem__(self, i).items()}


class Draws:
    """records what the reference draws from numpy's global generator while it runs"""

    def __enter__(self):
        self.log, self.real = [], {n: getattr(np.random, n) for n in ("uniform", "choice", "normal")}
        for name, fn in self.real.items():
            setattr(np.random, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        def call(*a, **k):
            v = fn(*a, **k)
            self.log.append((name, a, v))
            return v
        return call

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(np.random, name, fn)


def fma(a, b, c):
    """a * b + c with ONE rounding, element by element (exact rational arithmetic; Fraction -> float rounds correctly)"""
    b, c = np.broadcast_to(np.asarray(b, dtype=np.float64), a.shape), np.broadcast_to(np.asarray(c, dtype=np.float64), a.shape)
    return np.array([float(Fraction(float(u)) * Fraction(float(v)) + Fraction(float(w))) for u, v, w in zip(a, b, c)])


def formula(xyz32, p):
    """ts_stage_augment on the host: float64, the reference's order, ONE rounding to float32; steps that are off are skipped.
    The rotation is np.dot's arithmetic, dgemm's fused-multiply-add chain in k order: it differs from `x*c + y*(-s)` by an ulp of
    the double, which decides the float32 result where the two products cancel - the synthetic scans have points at exactly 45
    degrees of azimuth and TTA vote 3 rotates by pi/4."""
    x, y, z = (xyz32[:, i].astype(np.float64) for i in range(3))
    if p.rotate_on:
        x, y = fma(y, -p.s, x * p.c), fma(y, p.c, x * p.s)
    if p.scale_on:
        if p.rotate_on:
            x, y, z = x * p.scale, y * p.scale, z * p.scale
        else:          # float32 array * Python float: numpy multiplies in float32
            f = np.float32(p.scale)
            x, y, z = ((v.astype(np.float32) * f).astype(np.float64) for v in (x, y, z))
    if p.flip_on:
        if p.flip & 1:
            x = -x
        if p.flip & 2:
            y = -y
    if p.translate_on:
        x, y, z = x + p.translate[0], y + p.translate[1], z + p.translate[2]
    if not (p.rotate_on or p.scale_on or p.flip_on or p.translate_on):
        return xyz32.copy()
    return np.stack([x, y, z], 1).astype(np.float32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_replay(log, params, switches=None, tta=False):
    """the recorded draws of the reference == what the draw functions took from RandomState(seed)"""
    it = iter(log)
    for p in params:
        if not tta and p.rotate_on:
            name, _, v = next(it)
            assert name == "uniform" and float(v) == p.theta, (name, v, p.theta)
        if p.scale_on:
            name, _, v = next(it)
            assert name == "uniform" and float(v) == p.scale
        if p.flip_on:
            name, _, v = next(it)
            assert name == "choice" and int(v[0]) == p.flip
        if p.translate_on:
            for k in range(3):
                name, _, v = next(it)
                assert name == "normal" and float(v[0]) == p.translate[k]
    assert next(it, None) is None, "the reference drew more than the replay"


def store_params(out, c, params):
    out[f"{c}_theta"] = np.array([p.theta for p in params], dtype=np.float64)
    out[f"{c}_scale"] = np.array([p.scale for p in params], dtype=np.float64)
    out[f"{c}_flip"] = np.array([p.flip for p in params], dtype=np.int64)
    out[f"{c}_noise"] = np.array([p.translate for p in params], dtype=np.float64)


def kitti_entries(g):
    lm = g["learning_map"]
    T = int(g["T"])
    return [{"xyzret": g[f"b{b}_points_t{T}"], "labels": lm[g[f"b{b}_rawlabels_t{T}"] & 0xFFFF].astype(np.uint8),
             "path": f"/data/sequences/00/velodyne/{T:06d}.bin", "xyzret_ms": g[f"b{b}_raw_data_ms"],
             "labels_ms": g[f"b{b}_labels_ms"].astype(np.uint8)} for b in range(2)]


def make_vox(cls, entries, in_dim, voxel, training, switches=(True, True, True, True), scale_range=(0.9, 1.1)):
    vox = object.__new__(cls)
    vox.point_cloud_dataset = Frames(entries)
    vox.in_feature_dim, vox.training, vox.if_tta, vox.voxel_size, vox.num_points = in_dim, training, False, voxel, 3000000
    vox.if_flip, vox.if_scale, vox.if_jitter, vox.if_rotate = switches
    vox.scale_axis, vox.scale_range = "xyz", list(scale_range)
    vox.votes_min, vox.votes_max = 0, 10
    return vox


def run_ms_case(out, c, vox, cls, entries, in_dim, seed, which, switches):
    """one training batch of the samples `which`: the reference after np.random.seed(seed); replay + formula checked"""
    flip, scale, jitter, rotate = switches
    np.random.seed(seed)
    with Draws() as d:
        samples = [vox.get_single_sample(b) for b in which]
    rng = np.random.RandomState(seed)
    params = [A.draw_train_params(rng, flip=flip, scale=scale, scale_range=vox.scale_range, jitter=jitter, rotate=rotate)
              for _ in which]
    check_replay(d.log, params)
    out[f"{c}_seed"], out[f"{c}_samples"] = np.array(seed), np.array(which)
    out[f"{c}_switches"] = np.array(switches)                # flip, scale, jitter, rotate
    store_params(out, c, params)
    for i, (b, p) in enumerate(zip(which, params)):
        # the sample's `point` / `point_ms` before the clamp: the same library call on fresh copies, same draws
        e = entries[b]
        pt = e["xyzret"][:, :in_dim].astype(np.float32)
        pt_ms = e["xyzret_ms"][:, :in_dim].astype(np.float32)
        from tools.utils.common.seg_utils import aug_points_ms
        np.random.seed(seed)
        for _ in range(i + 1):
            a, a_ms = aug_points_ms(xyz=pt[:, :3].copy(), xyz_ms=pt_ms[:, :3].copy(), if_flip=flip, if_scale=scale,
                                    scale_axis="xyz", scale_range=vox.scale_range, if_jitter=jitter, if_rotate=rotate)
        want, want_ms = pt.copy(), pt_ms.copy()
        want[:, :3], want_ms[:, :3] = a, a_ms                # the store into the float32 arrays (semantickitti_voxel_ms.py:90)
        assert same_bits(formula(pt[:, :3], p), np.ascontiguousarray(want[:, :3])), (c, i, "point")
        assert same_bits(formula(pt_ms[:, :3], p), np.ascontiguousarray(want_ms[:, :3])), (c, i, "point_ms")
        # ... and they are what the sample was built from: representatives = first point of every voxel, in voxel order
        clamp = (want_ms[:, :3] >= want[:, :3].min(0)).all(1)
        s = samples[i]
        first = np.unique(np.asarray(s["inverse_map"].F), return_index=True)[1]
        first_ms = np.unique(np.asarray(s["inverse_map_ms"].F), return_index=True)[1]
        assert same_bits(np.asarray(s["lidar"].F), want[first]) and same_bits(np.asarray(s["lidar_ms"].F), want_ms[clamp][first_ms])
        out[f"{c}_point_xyz_{i}"] = np.ascontiguousarray(want[:, :3])
        out[f"{c}_point_ms_xyz_{i}"] = np.ascontiguousarray(want_ms[:, :3])
    out.update(dump_batch(f"{c}_batch_", cls.collate_batch(samples)))
    return params


def kitti_cases(out, g, plan):
    """SemanticKITTI multi-scan training cases (name, seed, samples of multiscan.npz, (flip, scale, jitter, rotate))"""
    _, SemVoxMs, _ = _ref_env.setup_datasets()
    entries = kitti_entries(g)
    flips = []
    for c, seed, which, switches in plan:
        vox = make_vox(SemVoxMs, entries, 5, VOXEL, True, switches)
        params = run_ms_case(out, c, vox, SemVoxMs, entries, 5, seed, which, switches)
        flips += [p.flip for p in params if p.flip_on]
    out["cases"] = np.array([c for c, _, _, _ in plan])
    return flips


def gen_kitti(g, fname="multiscan_aug.npz"):
    _, SemVoxMs, _ = _ref_env.setup_datasets()
    entries = kitti_entries(g)
    out = {"backend": np.array(R2.BACKEND_DESC)}
    # all four augmentations: seed 0 draws flip types 3 and 0 for its two samples, seed 2 draws 2, seed 4 draws 1
    plan = [("train_s0", 0, [0, 1], (True, True, True, True)), ("train_s2", 2, [0], (True, True, True, True)),
            ("train_s4", 4, [1], (True, True, True, True)), ("rotate_s5", 5, [0], (False, False, False, True))]
    flips = kitti_cases(out, g, plan)
    cases = out["cases"].tolist()
    assert set(flips) == {0, 1, 2, 3}, flips
    # training with nothing enabled: the un-augmented batch of multiscan.npz, tensor for tensor
    vox = make_vox(SemVoxMs, entries, 5, VOXEL, True, (False, False, False, False))
    np.random.seed(0)
    with Draws() as d:
        batch = SemVoxMs.collate_batch([vox.get_single_sample(0), vox.get_single_sample(1)])
    assert not d.log
    for key in ("lidar", "lidar_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms"):
        assert np.array_equal(batch[key].C.numpy(), g[f"batch_{key}_C"]) and np.array_equal(batch[key].F.numpy(), g[f"batch_{key}_F"])
    for key in ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask"):
        assert np.array_equal(batch[key].numpy(), g[f"batch_{key}"])
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; cases", cases, "flip types", flips)


def gen_tta(g, fname="multiscan_aug_tta.npz", seed=11, sample=0):
    _, SemVoxMs, _ = _ref_env.setup_datasets()
    entries = kitti_entries(g)
    vox = make_vox(SemVoxMs, [entries[sample]], 5, VOXEL, False)
    vox.if_tta = True
    np.random.seed(seed)
    with Draws() as d:
        batch = SemVoxMs.collate_batch_tta([vox[0]])
    rng = np.random.RandomState(seed)
    params = [A.draw_tta_params(rng, v, vox.scale_range) for v in range(10)]
    check_replay(d.log, params, tta=True)
    assert [p.theta for p in params] == [cnt * np.pi / 8.0 for cnt in (0, 1, -1, 2, -2, 6, -6, 7, -7, 8)]
    out = {"backend": np.array(R2.BACKEND_DESC), "tta_seed": np.array(seed), "tta_sample": np.array(sample),
           "tta_votes": np.array([0, 10])}
    store_params(out, "tta", params)
    # the float64 formula against the batch: the features of vote v's single-frame cloud are rows of the augmented scan
    pt = entries[sample]["xyzret"][:, :4].astype(np.float32)
    lidar_c, lidar_f = batch["lidar"].C.numpy(), batch["lidar"].F.numpy()
    for v, p in enumerate(params):
        want = pt.copy()
        want[:, :3] = formula(pt[:, :3], p)
        rows = {r.tobytes() for r in want}
        assert all(r.tobytes() in rows for r in lidar_f[lidar_c[:, 3] == v]), ("tta vote", v)
    out.update(dump_batch("tta_batch_", batch))
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; scales", [round(p.scale, 4) for p in params])


def gen_misc(g, fname="multiscan_aug_misc.npz"):
    _, _, SemVox = _ref_env.setup_datasets()
    R2._install_pyquaternion()
    _ref_env._pkg("pcseg.data.dataset.nuscenes", os.path.join(_ref_env.REF, "pcseg", "data", "dataset", "nuscenes"))
    for name in ("float", "bool"):
        if not hasattr(np, name):
            setattr(np, name, float if name == "float" else bool)        # aliases numpy >= 1.24 dropped
    from pcseg.data.dataset.nuscenes.nuscenes_voxel_ms import NuscVoxelMsDataset
    gn = dict(np.load(os.path.join(HERE, "multiscan_nus.npz"), allow_pickle=False))
    out = {"backend": np.array(R2.BACKEND_DESC)}
    kitti_cases(out, g, [("scale_jitter_s6", 6, [1], (False, True, True, False))])
    entries = [{"xyzret": gn[f"b{b}_xyzret"], "labels": gn[f"b{b}_labels"].astype(np.uint8), "path": f"s{b}",
                "xyzret_ms": gn[f"b{b}_xyzret_ms"], "labels_ms": gn[f"b{b}_labels_ms"].astype(np.uint8)} for b in range(2)]
    vox = make_vox(NuscVoxelMsDataset, entries, 4, 0.1, True)
    run_ms_case(out, "nus_s3", vox, NuscVoxelMsDataset, entries, 4, 3, [0], (True, True, True, True))
    # single frame: semantickitti_voxel.py:78-155 with aug_points
    seed, b = 2, 1
    e = kitti_entries(g)[b]
    sv = make_vox(SemVox, [{k: e[k] for k in ("xyzret", "labels", "path")}], 4, VOXEL, True)
    sv.eval_range = [0, 10000]
    np.random.seed(seed)
    with Draws() as d:
        sample = sv.get_single_sample(0)
    p = A.draw_train_params(np.random.RandomState(seed))
    check_replay(d.log, [p])
    c = "single_s2"
    out[f"{c}_seed"], out[f"{c}_samples"] = np.array(seed), np.array([b])
    store_params(out, c, [p])
    pt = e["xyzret"][:, :4].astype(np.float32)
    want = formula(pt[:, :3], p)
    pc = np.round(want / VOXEL).astype(np.int32)
    assert np.array_equal(pc - pc.min(0), sample["inverse_map"].C), "single frame: formula != reference"
    inds = np.unique(np.asarray(sample["inverse_map"].F), return_index=True)[1]
    out[f"{c}_point_xyz_0"] = want
    batch = SemVox.collate_batch([sample])
    assert same_bits(batch["lidar"].F.numpy(), np.concatenate([want, pt[:, 3:]], 1)[inds])
    for key in ("lidar", "targets", "targets_mapped", "inverse_map"):
        if key in SAME_COORDS:
            assert np.array_equal(batch[key].C.numpy(), batch[SAME_COORDS[key]].C.numpy()), key
        else:
            out[f"{c}_batch_{key}_C"] = batch[key].C.numpy()
        out[f"{c}_batch_{key}_F"] = batch[key].F.numpy()
    out[f"{c}_batch_num_points"] = batch["num_points"].numpy()
    out[f"{c}_batch_offset"] = batch["offset"].numpy()
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB")


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    g = dict(np.load(os.path.join(HERE, "multiscan.npz"), allow_pickle=False))
    gen_kitti(g)
    gen_tta(g)
    gen_misc(g)
