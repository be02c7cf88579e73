"""Point augmentation and TTA views on the device (-m gpu): ts_stage_augment and the `aug=` path of the data stage against the
reference's own dataset code (tests/golden/multiscan_aug*.npz: `get_single_sample` under training=True / TTA: True after
np.random.seed(seed), tools/utils/common/seg_utils.py:43-166), bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, nus_sample

pytestmark = pytest.mark.gpu

from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import nuscenes as N  # noqa: E402
from taseg_amd.data import stage as S  # noqa: E402
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI, fill_parameters, make_model_cfg  # noqa: E402
from taseg_amd.torchsparse import SparseTensor  # noqa: E402

BATCH_SPARSE = ("lidar", "lidar_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms", "targets_mapped",
                "targets_mapped_ms")
BATCH_DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask")
# the reference gives these tensors the coordinates of another one of the batch (asserted by the generator), stored once
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map", "targets_mapped_ms": "inverse_map_ms"}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_aug():
    return _load("multiscan_aug.npz")


@pytest.fixture(scope="module")
def g_aug_misc():
    return _load("multiscan_aug_misc.npz")


@pytest.fixture(scope="module")
def g_aug_tta():
    return _load("multiscan_aug_tta.npz")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), what


def case_params(g, c, switches=None):
    """the case's AugParams: its seed through the draw functions (tests/test_augment_host.py pins them to the stored draws)"""
    flip, scale, jitter, rotate = (bool(v) for v in (g[f"{c}_switches"] if switches is None else switches))
    rng = np.random.RandomState(int(g[f"{c}_seed"]))
    return [A.draw_train_params(rng, flip=flip, scale=scale, jitter=jitter, rotate=rotate) for _ in g[f"{c}_samples"]]


def check_kernel(pts, p, want_xyz, what):
    """out-of-place and in-place: xyz == the fixture's bits, every other column == the input's bits"""
    src = T(pts)
    keep = src.clone()
    out = A.augment_points(src, p)
    assert out.data_ptr() != src.data_ptr() and torch.equal(src, keep), what          # the input stays as it was
    same_bits(out[:, :3], want_xyz, what + " xyz")
    same_bits(out[:, 3:], pts[:, 3:], what + " other columns")
    inplace = src.clone()
    ret = A.augment_points(inplace, p, out=inplace)
    assert ret.data_ptr() == inplace.data_ptr()
    same_bits(inplace, out, what + " in place")


# ------------------------------------------------------------------------------------------------ 1. kernel against the golden
def test_kernel_matches_the_reference_bits(g_multiscan, g_multiscan_nus, g_aug, g_aug_misc):
    g, Tn = g_multiscan, int(g_multiscan["T"])
    strides, seen = set(), []
    for ga in (g_aug, g_aug_misc):
        for c in ga["cases"].tolist():
            seen.append(c)
            for i, (b, p) in enumerate(zip(ga[f"{c}_samples"].tolist(), case_params(ga, c))):
                for pts, key in ((g[f"b{b}_points_t{Tn}"], "point"), (g[f"b{b}_raw_data_ms"], "point_ms")):
                    check_kernel(pts, p, ga[f"{c}_{key}_xyz_{i}"], f"{c} sample {i} {key}")
                    strides.add(pts.shape[1])
    assert strides == {4, 5} and seen == ["train_s0", "train_s2", "train_s4", "rotate_s5", "scale_jitter_s6"]
    # rows of several samples in one launch, each with its own record
    c = "train_s0"
    ps = case_params(g_aug, c)
    clouds = [g[f"b{b}_raw_data_ms"] for b in g_aug[f"{c}_samples"].tolist()]
    idx = torch.cat([torch.full((len(x),), i, dtype=torch.int32) for i, x in enumerate(clouds)]).cuda()
    out = A.augment_points(T(np.concatenate(clouds)), ps, idx)
    same_bits(out[:, :3], np.concatenate([g_aug[f"{c}_point_ms_xyz_{i}"] for i in range(len(clouds))]), "two records, one launch")
    # nuScenes (4 columns: the time column is cut, IN_FEATURE_DIM 4) and the single-frame aug_points sample
    gn = g_multiscan_nus
    p = case_params(g_aug_misc, "nus_s3", (True,) * 4)[0]
    b = int(g_aug_misc["nus_s3_samples"][0])
    check_kernel(gn[f"b{b}_xyzret"][:, :4], p, g_aug_misc["nus_s3_point_xyz_0"], "nuScenes point")
    check_kernel(gn[f"b{b}_xyzret_ms"][:, :4], p, g_aug_misc["nus_s3_point_ms_xyz_0"], "nuScenes point_ms")
    p = case_params(g_aug_misc, "single_s2", (True,) * 4)[0]
    b = int(g_aug_misc["single_s2_samples"][0])
    check_kernel(g[f"b{b}_points_t{Tn}"], p, g_aug_misc["single_s2_point_xyz_0"], "single frame")


# ------------------------------------------------------------------------------------------------ 2. no-op
@pytest.mark.parametrize("cols", [3, 4, 5])
def test_nothing_enabled_returns_the_input_bits(cols):
    rng = np.random.RandomState(3)
    pts = rng.standard_normal((4099, cols)).astype(np.float32) * 30
    pts[::5] = -0.0
    pts[1::7, 0] = 0.0
    pts[2::11, 2] = np.float32(1e-42)            # a subnormal
    for p in (A.AugParams(), A.AugParams(c=0.3, s=0.7, scale=1.07, flip=3, translate=(0.1, 0.2, 0.3))):   # values without bits
        src = T(pts)
        same_bits(A.augment_points(src, p), pts, "no-op")
        A.augment_points(src, p, out=src)
        same_bits(src, pts, "no-op in place")
    if cols == 4:
        # rows that start 4 bytes off a 16-byte boundary take the plain-load path
        flat = torch.zeros(4 * len(pts) + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(-1, 4)
        view.copy_(T(pts))
        assert view.data_ptr() % 16 == 4
        same_bits(A.augment_points(view, A.AugParams()), pts, "no-op, unaligned")
        p = A.draw_train_params(np.random.RandomState(1))
        same_bits(A.augment_points(view, p), A.augment_points(T(pts), p), "unaligned rows == aligned rows")


# ------------------------------------------------------------------------------------------------ 3. stage against the golden
def kitti_scan(g, b):
    Tn, lm = int(g["T"]), g["learning_map"]
    return {"points": [T(g[f"b{b}_points_t{t}"]) for t in range(Tn + 1)],
            "labels": [T(lm[g[f"b{b}_rawlabels_t{t}"]]) for t in range(Tn + 1)],
            "poses": [T(g[f"b{b}_pose_t{t}"]) for t in range(Tn + 1)], "name": str(b)}


def check_batch(batch, g, prefix, sparse=BATCH_SPARSE, dense=BATCH_DENSE):
    for key in sparse:
        if f"{prefix}{key}_F" not in g:
            assert key.startswith("targets_mapped"), key          # multiscan.npz's keys do not hold them
            continue
        want_c = g[f"{prefix}{key}_C"] if f"{prefix}{key}_C" in g else g[f"{prefix}{SAME_COORDS[key]}_C"]
        want_f = g[f"{prefix}{key}_F"]
        got_c, got_f = batch[key].C.cpu().numpy(), batch[key].F.cpu().numpy()
        assert got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (prefix, key, "C")
        if want_f.dtype == np.float32:
            same_bits(got_f, want_f, (prefix, key, "F"))
        else:
            assert got_f.shape == want_f.shape and np.array_equal(got_f, want_f), (prefix, key, "F")
    for key in dense:
        want = g[prefix + key].reshape(-1)
        got = batch[key].cpu().numpy().reshape(-1)
        assert got.shape == want.shape and np.array_equal(got, want), (prefix, key)


def same_batches(a, b):
    assert set(a) == set(b)
    for key, v in a.items():
        w = b[key]
        if isinstance(v, SparseTensor):
            assert v.C.dtype == w.C.dtype and v.F.dtype == w.F.dtype and torch.equal(v.C, w.C), key
            assert torch.equal(v.F.view(torch.int32) if v.F.dtype == torch.float32 else v.F,
                               w.F.view(torch.int32) if w.F.dtype == torch.float32 else w.F), key
        elif isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and v.shape == w.shape and v.device == w.device and torch.equal(v, w), key
        else:
            assert v == w, key


def test_kitti_stage_with_aug_matches_the_reference(g_multiscan, g_aug, g_aug_misc):
    g = g_multiscan
    steps = g["steps"].tolist()
    for g_aug, c in [(g_aug, c) for c in g_aug["cases"].tolist()] + [(g_aug_misc, c) for c in g_aug_misc["cases"].tolist()]:
        scans = [kitti_scan(g, b) for b in g_aug[f"{c}_samples"].tolist()]
        resident = [p.clone() for s in scans for p in s["points"]]
        aug = case_params(g_aug, c)
        batched = S.build_multiscan_batch(scans, 0.05, steps, aug=aug)
        check_batch(batched, g_aug, f"{c}_batch_")
        per_sample = S.build_multiscan_batch_per_sample(scans, 0.05, steps, aug=aug)
        check_batch(per_sample, g_aug, f"{c}_batch_")
        same_batches(batched, per_sample)
        # packed records are the same thing
        same_batches(batched, S.build_multiscan_batch(scans, 0.05, steps, aug=A.pack_params(aug)))
        assert all(torch.equal(a, b) for a, b in zip(resident, [p for s in scans for p in s["points"]])), "resident scans changed"
    # aug=None is the path of before, and records without bits give its tensors too: both == multiscan.npz
    scans = [kitti_scan(g, 0), kitti_scan(g, 1)]
    plain = S.build_multiscan_batch(scans, 0.05, steps)
    check_batch(plain, g, "batch_")
    for fn in (S.build_multiscan_batch, S.build_multiscan_batch_per_sample):
        off = fn(scans, 0.05, steps, aug=[A.AugParams(), A.AugParams()])
        check_batch(off, g, "batch_")
        same_batches(off, plain)
    with pytest.raises(ValueError):
        S.build_multiscan_batch(scans, 0.05, steps, aug=[A.AugParams()])


def nus_samples(g):
    steps, lm = g["steps"].tolist(), g["learning_map"]
    out = []
    for b in range(2):
        _, seq, index, pts, pseudo, labels = nus_sample(g, b)
        offsets = N.select_sweeps(seq, index, int(g["multiscan"]), float(g["step"]))
        out.append(dict(points=T(g[f"b{b}_points_cur"]), labels=T(lm[g[f"b{b}_rawlabels_cur"]]),
                        hist_points=[T(pts[d]) for d in offsets],
                        hist_labels=[T(np.asarray(labels[d], dtype=np.int64)) for d in offsets],
                        hist_pseudo=[T(pseudo[d].astype(np.int64)) for d in offsets],
                        params=torch.from_numpy(N.sweep_params(seq, index, offsets)).cuda(), name=f"s{b}"))
    return out, steps


def test_nuscenes_stage_with_aug_matches_the_reference(g_multiscan_nus, g_aug_misc):
    samples, steps = nus_samples(g_multiscan_nus)
    c = "nus_s3"
    aug = case_params(g_aug_misc, c, (True,) * 4)
    one = [samples[b] for b in g_aug_misc[f"{c}_samples"].tolist()]
    batched = N.build_nuscenes_batch(one, 0.1, steps, aug=aug)
    check_batch(batched, g_aug_misc, f"{c}_batch_")
    same_batches(batched, N.build_nuscenes_batch_per_sample(one, 0.1, steps, aug=aug))
    # a whole batch, one record per sample, also with a sample that has no sweeps
    rng = np.random.RandomState(21)
    bare = dict(samples[1], hist_points=[], hist_labels=[], hist_pseudo=[], params=samples[1]["params"][:0])
    three = [samples[0], bare, samples[1]]
    aug3 = [A.draw_train_params(rng) for _ in three]
    same_batches(N.build_nuscenes_batch(three, 0.1, steps, aug=aug3), N.build_nuscenes_batch_per_sample(three, 0.1, steps, aug=aug3))
    check_batch(N.build_nuscenes_batch(samples, 0.1, steps, aug=[A.AugParams()] * 2), g_multiscan_nus, "batch_")
    check_batch(N.build_nuscenes_batch(samples, 0.1, steps), g_multiscan_nus, "batch_")


def test_single_frame_sample_with_aug_matches_the_reference(g_multiscan, g_aug_misc):
    g, c = g_multiscan, "single_s2"
    b = int(g_aug_misc[f"{c}_samples"][0])
    Tn = int(g["T"])
    p = case_params(g_aug_misc, c, (True,) * 4)[0]
    pts, lab = T(g[f"b{b}_points_t{Tn}"]), T(g["learning_map"][g[f"b{b}_rawlabels_t{Tn}"]])
    batch = S.collate_batch([S.voxelize_sample(pts, lab, 0.05, "x", aug=p)])
    check_batch(batch, g_aug_misc, f"{c}_batch_", sparse=("lidar", "targets", "targets_mapped", "inverse_map"),
                dense=("num_points", "offset"))
    same_batches(batch, S.collate_batch([S.voxelize_sample(pts, lab, 0.05, "x", aug=[p])]))
    same_batches(S.collate_batch([S.voxelize_sample(pts, lab, 0.05, "x")]),
                 S.collate_batch([S.voxelize_sample(pts, lab, 0.05, "x", aug=A.AugParams())]))


# ------------------------------------------------------------------------------------------------ 4. TTA
def test_tta_batch_matches_collate_batch_tta_and_votes_accumulate(g_multiscan, g_aug_tta):
    from taseg_amd.pcseg import eval as E
    from taseg_amd.pcseg.model import build_network
    g, gt = g_multiscan, g_aug_tta
    steps = g["steps"].tolist()
    scan = kitti_scan(g, int(gt["tta_sample"]))
    lo, hi = gt["tta_votes"].tolist()
    batch = S.build_tta_batch(scan, lo, hi, np.random.RandomState(int(gt["tta_seed"])), 0.05, steps)
    check_batch(batch, gt, "tta_batch_")
    assert len(batch["name"]) == hi - lo
    model = fill_parameters(build_network(make_model_cfg("MinkUNetMs", in_dim=5, cr=0.5, num_layer=[1] * 8), 20), seed=3).cuda().eval()
    with torch.no_grad():
        ret = model(batch)
    total = E.accumulate_votes(ret, hi - lo)
    n = scan["points"][-1].shape[0]
    assert total.shape == (n, 20) and np.isfinite(total).all()
    assert np.allclose(total, np.sum([ret["point_predict_logits"][v] for v in range(hi - lo)], 0), rtol=0, atol=1e-4)


def test_nuscenes_tta_batch(g_multiscan_nus):
    samples, steps = nus_samples(g_multiscan_nus)
    batch = N.build_tta_batch(samples[0], 2, 6, np.random.RandomState(4), 0.1, steps)
    rng = np.random.RandomState(4)
    aug = [A.draw_tta_params(rng, v) for v in range(2, 6)]
    same_batches(batch, N.build_nuscenes_batch_per_sample([samples[0]] * 4, 0.1, steps, aug=aug))
    assert batch["num_points"].view(-1).tolist() == [samples[0]["points"].shape[0]] * 4


# ------------------------------------------------------------------------------------------------ 5. at size
def formula64(pts, p):
    """ts_stage_augment restated in numpy: float64 in the reference's order (seg_utils.py:115-164), one rounding to float32"""
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    if p.rotate_on:
        x, y = x * p.c + y * (-p.s), x * p.s + y * p.c
    if p.scale_on:
        x, y, z = x * p.scale, y * p.scale, z * p.scale
    if p.flip_on and p.flip & 1:
        x = -x
    if p.flip_on and p.flip & 2:
        y = -y
    if p.translate_on:
        x, y, z = x + p.translate[0], y + p.translate[1], z + p.translate[2]
    return np.stack([x, y, z], 1).astype(np.float32)


def ulp_distance(a, b):
    def ordered(v):
        i = np.ascontiguousarray(v).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def test_batched_stage_with_aug_at_bench_size():
    """two samples of 120k points with four history scans, voxel 0.05 m (bench.py's 4-scan TFA shape): the batched path with aug
    == collate_batch of voxelize_sample_ms fed with clouds augmented by augment_points, tensor for tensor and bit for bit; and
    augment_points against float64 numpy: every value within one float32 ulp, at most 1 in 10^6 different at all.  The kernel
    rotates with dgemm's fused-multiply-add chain (what np.dot does), formula64 with two rounded products: an ulp of the double
    apart, which survives the rounding to float32 only on a double-rounding tie or where the products cancel (a point whose
    azimuth plus the drawn angle is a multiple of 90 degrees to ~1e-9 rad) - the reference's own np.dot against the explicit
    products differed on 0 of 7.2 M values, so the cap only guards such a tie."""
    import bench
    scans, _ = bench.make_multiscans(0, 2, 120000)
    rng = np.random.RandomState(17)
    aug = [A.draw_train_params(rng) for _ in scans]
    batched = S.build_multiscan_batch(scans, 0.05, FLEXIBLE_STEPS_KITTI, aug=aug)
    samples, n_values, n_diff, worst = [], 0, 0, 0
    for s, p in zip(scans, aug):
        pts, lab, poses = s["points"], s["labels"], s["poses"]
        t = len(pts) - 1
        assert pts[t].shape[0] == 120000 and t == 4
        raw_all, lab_all, keep = S._fuse_history(pts[t], lab[t], pts[:t], lab[:t], poses[t], poses[:t], [i - t for i in range(t)],
                                                 FLEXIBLE_STEPS_KITTI)
        cur_aug, raw_aug = A.augment_points(pts[t], p), A.augment_points(raw_all, p)
        samples.append(S.voxelize_sample_ms(cur_aug, lab[t].long(), raw_aug, lab_all, 0.05, s.get("name", ""), keep=keep))
        for got, src in ((cur_aug, pts[t]), (raw_aug, raw_all)):
            got, src = got.cpu().numpy(), src.cpu().numpy()
            d = ulp_distance(got[:, :3], formula64(src, p))
            n_values += d.size
            n_diff += int((d != 0).sum())
            worst = max(worst, int(d.max()))
            assert np.array_equal(bits(got[:, 3:]), bits(src[:, 3:]))
    print(f"augment_points vs float64 numpy: {n_values} values, {n_diff} differ, worst {worst} ulp")
    assert worst <= 1
    assert n_diff * 10 ** 6 <= n_values
    same_batches(batched, S.collate_batch(samples))


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_same_seed_gives_the_same_batches(g_multiscan):
    g = g_multiscan
    steps = g["steps"].tolist()
    scans = [kitti_scan(g, 0), kitti_scan(g, 1)]

    def run(seed):
        rng = np.random.RandomState(seed)
        return S.build_multiscan_batch(scans, 0.05, steps, aug=[A.draw_train_params(rng) for _ in scans])

    a, b, c = run(123), run(123), run(124)
    same_batches(a, b)
    assert not torch.equal(a["lidar"].F, c["lidar"].F)
    t1 = S.build_tta_batch(scans[0], 0, 10, np.random.RandomState(8), 0.05, steps)
    t2 = S.build_tta_batch(scans[0], 0, 10, np.random.RandomState(8), 0.05, steps)
    same_batches(t1, t2)
