"""The TIAF recipe's training augmentation, image flip and TTA views on the device (-m gpu): the per-sample path
(build_tiaf_sample(aug=, flips=) + build_tiaf_batch) and the batched builder on csrc/tiaf_stage.hip (build_tiaf_batch_from_frames,
build_tiaf_tta_batch), each bit for bit against what the REAL reference's dataset code produced (tests/golden/tiaf_aug.npz, inputs
in tests/golden/tiaf_data.npz); ts_tiaf_image_stack against its rule restated in numpy; ts_tiaf_fov_cloud against the chain of
operators it replaces."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SPARSE = ("lidar", "lidar_ms", "lidar_fov_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms", "targets_mapped",
          "targets_mapped_ms")
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map", "targets_mapped_ms": "inverse_map_ms"}
DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img")
VOXEL = 0.05


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_data.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_aug.npz"), allow_pickle=False))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wide_image(seed, h, w):
    """the images of case `wide` (tests/golden/make_golden_tiaf_aug.py `wide_image`), from the stored seed"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8), rs.randint(0, 20, size=(h, w, 1)).astype(np.float32)


def device_frames(g, b, images=None):
    from taseg_amd.data import semantickitti as SK
    t_cur, step = int(g["T"]), int(g["step_image"])
    frames = {}
    for t in range(t_cur + 1):
        raw = g[f"b{b}_rawlabels_t{t}"].astype(np.int64)
        f = {"points": T(g[f"b{b}_points_t{t}"]), "labels": T(SK._LUT[raw]), "pseudo": T(SK._CANON[raw]), "pose": T(g[f"b{b}_pose_t{t}"])}
        if (t_cur - t) % step == 0:
            img, sem = images[t] if images is not None else (g[f"b{b}_image_t{t}"], g[f"b{b}_semantic_t{t}"])
            f["image"], f["semantic"] = T(img), T(sem)
        frames[t - t_cur] = f
    return frames


@pytest.fixture(scope="module")
def frames(g):
    return [device_frames(g, b) for b in range(2)]


@pytest.fixture(scope="module")
def wide_frames(g, ga):
    h, w = ga["wide_image_shape"].tolist()
    t_cur, step = int(g["T"]), int(g["step_image"])
    cams = [t for t in range(t_cur + 1) if (t_cur - t) % step == 0]
    return [device_frames(g, b, {t: wide_image(int(s), h, w) for t, s in zip(cams, ga["wide_image_seeds"][b])}) for b in range(2)]


def setup(g):
    name = f"/data/sequences/00/velodyne/{int(g['T']):06d}.bin"
    return dict(steps=g["steps"].tolist(), multiscan=int(g["multiscan"]), step_image=int(g["step_image"]),
                crop=(int(g["height"]), int(g["width"])), proj=T(g["proj"]), name=name)


def draws(seed, deltas, training=True):
    """flips, (coin), augmentation of one sample from RandomState(seed): tests/test_tiaf_aug_host.py pins them to the golden's"""
    from taseg_amd.data import augment as A
    from taseg_amd.data import mix as M
    from taseg_amd.data.tiaf import draw_image_flips
    rng = np.random.RandomState(seed)
    flips = draw_image_flips(rng, deltas)
    M.draw_coin(rng)
    return flips, (A.draw_train_params(rng) if training else None)


def build(kind, frames_list, s, aug, flips):
    from taseg_amd.data import tiaf as TF
    if kind == "per_sample":
        return TF.build_tiaf_batch([
            TF.build_tiaf_sample(f, s["steps"], s["multiscan"], s["step_image"], s["proj"], s["crop"], VOXEL, name=s["name"],
                                 aug=None if aug is None else aug[b], flips=None if flips is None else flips[b])
            for b, f in enumerate(frames_list)])
    return TF.build_tiaf_batch_from_frames(frames_list, s["steps"], s["multiscan"], s["step_image"], [s["proj"]] * len(frames_list),
                                           s["crop"], VOXEL, names=[s["name"]] * len(frames_list), aug=aug, flips=flips)


def check_sparse(batch, want, prefix, keys, fallback=None, fallback_prefix="batch_"):
    """C and F of every sparse key, bit for bit; a key the golden does not store again is read from `fallback` (tiaf_data.npz)"""
    for key in keys:
        src, pre = (want, prefix) if f"{prefix}{key}_F" in want else (fallback, fallback_prefix)
        ckey = f"{pre}{key}_C" if f"{pre}{key}_C" in src else f"{pre}{SAME_COORDS[key]}_C"
        assert np.array_equal(batch[key].C.cpu().numpy(), src[ckey]), key
        got, ref = batch[key].F.cpu().numpy(), src[f"{pre}{key}_F"]
        assert got.shape == ref.shape, key
        if ref.dtype == np.float32:
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), key
        else:
            assert np.array_equal(got.astype(ref.dtype), ref), key


def check_dense(batch, want, prefix, repeat=1):
    for key in DENSE:
        assert np.array_equal(batch[key].cpu().numpy().reshape(-1), want[f"{prefix}{key}"].reshape(-1)), key
    img, sem = batch["image_ms"].cpu().numpy(), batch["semantic_map_ms"].cpu().numpy()
    assert list(img.shape) == want[f"{prefix}image_ms_shape"].tolist() and img.dtype == np.float32
    sub, ref = np.concatenate([want[f"{prefix}image_ms_sub"]] * repeat), np.concatenate([want[f"{prefix}semantic_map_ms"]] * repeat)
    assert np.array_equal(img[:, :, ::3, ::3].view(np.uint32), sub.view(np.uint32))
    assert sem.shape == ref.shape and np.array_equal(sem.view(np.uint32), ref.view(np.uint32))


def test_batched_builder_without_flip_and_augmentation_equals_the_reference_golden(g, frames):
    batch = build("batched", frames, setup(g), None, None)
    for key in ("lidar", "lidar_ms", "lidar_fov_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms", "targets_mapped",
                "targets_mapped_ms"):
        assert np.array_equal(batch[key].C.cpu().numpy(), g[f"batch_{key}_C"]), key
        got = batch[key].F.cpu().numpy()
        assert np.array_equal(got.astype(g[f"batch_{key}_F"].dtype), g[f"batch_{key}_F"]), key
    for key in ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img"):
        assert np.array_equal(batch[key].cpu().numpy().reshape(-1), g[f"batch_{key}"].reshape(-1)), key
    img = batch["image_ms"].cpu().numpy()
    assert list(img.shape) == g["batch_image_ms_shape"].tolist() and np.array_equal(img[:, :, ::3, ::3], g["batch_image_ms_sub"])
    assert np.array_equal(batch["semantic_map_ms"].cpu().numpy(), g["batch_semantic_map_ms"])


@pytest.mark.parametrize("kind", ["per_sample", "batched"])
def test_training_batch_with_flips_and_augmentation_equals_the_reference(g, ga, frames, kind):
    deltas = ga["train_camera_deltas"].tolist()
    flips, aug = zip(*[draws(seed, deltas) for seed in ga["train_seeds"].tolist()])
    batch = build(kind, frames, setup(g), list(aug), list(flips))
    check_sparse(batch, ga, "train_batch_", SPARSE)
    check_dense(batch, ga, "train_batch_")
    assert batch["name"] == [setup(g)["name"]] * 2


@pytest.mark.parametrize("kind", ["per_sample", "batched"])
def test_wide_images_the_flip_moves_the_crop(g, ga, wide_frames, kind):
    deltas = ga["wide_camera_deltas"].tolist()
    flips = [draws(seed, deltas, training=False)[0] for seed in ga["wide_seeds"].tolist()]
    batch = build(kind, wide_frames, setup(g), None, flips)
    check_sparse(batch, ga, "wide_batch_", SPARSE, fallback=g)             # the LiDAR keys are tiaf_data.npz's
    check_dense(batch, ga, "wide_batch_")
    # without the flip other points pass the crop test
    plain = build(kind, wide_frames, setup(g), None, None)
    assert plain["lidar_fov_ms"].C.shape != batch["lidar_fov_ms"].C.shape or not torch.equal(plain["lidar_fov_ms"].C, batch["lidar_fov_ms"].C)


@pytest.mark.parametrize("kind", ["per_sample", "batched"])
def test_tta_views_equal_the_reference(g, ga, frames, kind):
    from taseg_amd.data import augment as A
    from taseg_amd.data import mix as M
    from taseg_amd.data import tiaf as TF
    s = setup(g)
    lo, hi = ga["tta_votes"].tolist()
    f = frames[int(ga["tta_sample"])]
    rng = np.random.RandomState(int(ga["tta_seed"]))
    if kind == "per_sample":
        aug = [(M.draw_coin(rng), A.draw_tta_params(rng, v))[1] for v in range(lo, hi)]
        batch = build(kind, [f] * (hi - lo), s, aug, None)
    else:
        batch = TF.build_tiaf_tta_batch(f, lo, hi, rng, s["steps"], s["multiscan"], s["step_image"], s["proj"], s["crop"], VOXEL,
                                        name=s["name"])
    check_sparse(batch, ga, "tta_batch_", SPARSE)
    check_dense(batch, ga, "tta_batch_", repeat=hi - lo)


# ------------------------------------------------------------------------------------------------ ts_tiaf_image_stack
def np_image_stack(images, semantic, flips, crop):
    """the rule of include/taseg_hip.h in numpy: BGR / 255 through the table, the flip BEFORE the top-left crop, zero padding"""
    table = np.arange(256, dtype=np.float32) / 255.
    H, W = crop
    out = np.zeros((len(images), 3, H, W), np.float32)
    sem = np.zeros((len(images), 1, H, W), np.float32)
    for t, (im, fl) in enumerate(zip(images, flips)):
        r, c = min(H, im.shape[0]), min(W, im.shape[1])
        src = im[:, ::-1] if fl else im
        out[t, :, :r, :c] = table[src[:r, :c, ::-1]].transpose(2, 0, 1)
        if semantic is not None:
            m = semantic[t][:, ::-1] if fl else semantic[t]
            sem[t, 0, :r, :c] = m[:r, :c, 0]
    return out, sem


@pytest.mark.parametrize("with_semantic", [True, False])
@pytest.mark.parametrize("hw,crop", [((64, 180), (60, 192)), ((56, 200), (60, 192)), ((60, 192), (60, 192)), ((61, 193), (60, 192)),
                                     ((9, 10), (7, 13))])
def test_image_stack_equals_its_rule(hw, crop, with_semantic):
    from taseg_amd import backend as B
    from taseg_amd.data.tiaf import _unit_table
    rs = np.random.RandomState(hw[0] * 1000 + hw[1])
    n = 17                                                                   # one more than a launch takes: the wrapper splits
    images = [rs.randint(0, 256, size=(hw[0], hw[1], 3)).astype(np.uint8) for _ in range(n)]
    semantic = [rs.randint(0, 20, size=(hw[0], hw[1], 1)).astype(np.float32) for _ in range(n)] if with_semantic else None
    flips = [bool(t % 3 != 1) for t in range(n)]                             # both values inside either launch
    dev_images = [T(im) for im in images]
    # one image off every alignment: a view one byte into a buffer
    buf = torch.empty(images[2].size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = dev_images[2].reshape(-1)
    dev_images[2] = buf[1:].view(hw[0], hw[1], 3)
    got, got_sem = B.tiaf_image_stack(dev_images, None if semantic is None else [T(m) for m in semantic], flips,
                                      _unit_table(torch.device("cuda", torch.cuda.current_device())), crop)
    want, want_sem = np_image_stack(images, semantic, flips, crop)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if with_semantic:
        assert np.array_equal(got_sem.cpu().numpy().view(np.uint32), want_sem.view(np.uint32))
    else:
        assert got_sem is None


def test_image_stack_checks_its_arguments():
    from taseg_amd import backend as B
    table = torch.zeros(256, device="cuda")
    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        B.tiaf_image_stack([img.float()], None, None, table, (4, 4))
    with pytest.raises(ValueError):
        B.tiaf_image_stack([img], None, [True, False], table, (4, 4))
    with pytest.raises(RuntimeError):
        B.tiaf_image_stack([img.cpu()], None, None, table, (4, 4))
    with pytest.raises(TypeError):
        B.tiaf_image_stack([img], [torch.zeros((3, 4, 1), device="cuda")], None, table, (4, 4))


# ------------------------------------------------------------------------------------------------ ts_tiaf_fov_cloud
def fov_case(g, fov_dist):
    """two samples, frames of 300, 0 and 517 rows (an empty frame; a frame and sample boundary inside a block of 256 rows), the
    first frame flipped, the other two pose-fused, a NaN row in the last"""
    from taseg_amd.data import augment as A
    rs = np.random.RandomState(44)
    lengths, sample, flags = [300, 0, 517], [0, 0, 1], [(True, False), (False, True), (False, True)]
    pts = [np.stack([rs.uniform(-5, 30, n), rs.uniform(-12, 12, n), rs.uniform(-3, 2, n), rs.uniform(0, 1, n)], 1).astype(np.float32)
           for n in lengths]
    pts[2][100, 2] = np.nan
    aug = [A.draw_train_params(np.random.RandomState(5)), A.draw_tta_params(np.random.RandomState(6), 3)]
    pose0, pose = [g["b0_pose_t8"], g["b1_pose_t8"]], [g["b0_pose_t8"], g["b0_pose_t4"], g["b1_pose_t4"]]
    return dict(lengths=lengths, sample=sample, flags=flags, pts=pts, aug=aug, pose0=pose0, pose=pose, fov_dist=fov_dist,
                img=(180, 64), crop=(60, 192), row_offset=[0.0, 60.0, 60.0])


def fov_chain(c, proj):
    """project_fov -> mask -> fuse_scan -> augment_points, per sample: the rows before the clamp"""
    from taseg_amd import backend as B
    from taseg_amd.data.augment import augment_points
    w, h = c["img"]
    clouds = [[], []]
    for f, (p, b, (flip, fuse)) in enumerate(zip(c["pts"], c["sample"], c["flags"])):
        p = T(p)
        pix, ok = B.project_fov(p, proj, (w, h), (c["crop"][0], w) if flip else c["crop"], c["row_offset"][f])
        col = (w - 1) - pix[:, 1] if flip else pix[:, 1]
        ok = ok & (col < c["crop"][1])
        if c["fov_dist"] > 0:
            ok = ok & (torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) <= c["fov_dist"])
        rows = p[ok]
        if fuse:
            rows = B.fuse_scan(rows.contiguous(), T(c["pose0"][b]), T(c["pose"][f]))
        clouds[b].append(torch.cat([rows, pix[ok, :1], col[ok].unsqueeze(1)], 1))
    return [augment_points(torch.cat(cl, 0), c["aug"][b]) for b, cl in enumerate(clouds)]


@pytest.mark.parametrize("fov_dist", [-1.0, 12.5])
def test_fov_cloud_equals_the_chain_it_replaces(g, fov_dist):
    from taseg_amd import backend as B
    from taseg_amd.data import tiaf as TF
    from taseg_amd.data.augment import pack_params
    from taseg_amd.data.stage import rows_index32
    c = fov_case(g, fov_dist)
    proj = T(g["proj"])
    before = fov_chain(c, proj)
    # lo: the 30 % quantile of every sample's x, everything in y and z - some rows of every sample survive, not all
    lo = np.stack([[np.quantile(a.cpu().numpy()[:, 0], 0.3), -1e9, -1e9] for a in before]).astype(np.float32)
    want = [a[(a[:, :3] >= T(lo[b])).all(1)].cpu().numpy() for b, a in enumerate(before)]
    assert all(0 < len(wb) < len(a) for wb, a in zip(want, before))
    entries, first = [], 0
    for f, (n, b, (flip, fuse)) in enumerate(zip(c["lengths"], c["sample"], c["flags"])):
        entries.append((proj, T(c["pose0"][b]), T(c["pose"][f]), {
            "row_offset": c["row_offset"][f], "fov_dist": fov_dist, "sample": b, "img_w": c["img"][0], "img_h": c["img"][1],
            "flags": TF.FLIP * flip + TF.FUSE * fuse, "first": first, "src": first}))
        first += n
    dev = proj.device
    args = (T(np.concatenate(c["pts"])), rows_index32(c["lengths"], dev), TF._frame_records(entries, dev), 2, c["crop"])
    kw = dict(aug=T(pack_params(c["aug"])), lo=T(lo))
    out, s64, s32, counts = B.tiaf_fov_cloud(*args, **kw)
    counts = counts.tolist()
    assert counts == [len(wb) for wb in want]
    kept = sum(counts)
    got = out[:kept].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.concatenate(want).view(np.uint32))          # rows, order, bits
    assert not np.isnan(got).any()                                                            # the NaN row is gone
    assert s64[:kept].tolist() == s32[:kept].tolist() == [0] * counts[0] + [1] * counts[1]
    again = B.tiaf_fov_cloud(*args, **kw)
    assert torch.equal(again[0][:kept].view(torch.int32), out[:kept].view(torch.int32)) and again[3].tolist() == counts
    if fov_dist > 0:
        off = B.tiaf_fov_cloud(*args[:2], TF._frame_records([(*e[:3], {**e[3], "fov_dist": -1.0}) for e in entries], dev), 2, c["crop"], **kw)
        assert sum(off[3].tolist()) > kept                                                    # the distance test dropped rows


def test_fov_cloud_without_records_of_augmentation_and_clamp_and_shared_rows(g):
    """aug = lo = NULL: the rows of ts_project_fov's mask as they are; two records reading the same point rows give them twice"""
    from taseg_amd import backend as B
    from taseg_amd.data import tiaf as TF
    from taseg_amd.data.stage import rows_index32
    c = fov_case(g, -1.0)
    proj, p = T(g["proj"]), T(c["pts"][0])
    pix, ok = B.project_fov(p, proj, c["img"], c["crop"], 0.0)
    want = torch.cat([p[ok], pix[ok]], 1)
    rec = lambda b, first: (proj, T(c["pose0"][0]), T(c["pose"][0]), {  # noqa: E731
        "row_offset": 0.0, "fov_dist": -1.0, "sample": b, "img_w": c["img"][0], "img_h": c["img"][1], "flags": 0, "first": first, "src": 0})
    n = len(c["pts"][0])
    out, s64, _, counts = B.tiaf_fov_cloud(p, rows_index32([n, n], p.device), TF._frame_records([rec(0, 0), rec(1, n)], p.device), 2, c["crop"])
    k = int(ok.sum())
    assert counts.tolist() == [k, k] and 0 < k < n
    assert torch.equal(out[:k].view(torch.int32), want.view(torch.int32)) and torch.equal(out[k:2 * k].view(torch.int32), want.view(torch.int32))
    assert s64[:2 * k].tolist() == [0] * k + [1] * k


def test_fov_cloud_more_than_256_blocks_of_shared_rows(g):
    """220 records over three samples read the same 300 point rows: 66 000 virtual rows, 258 blocks, so every thread of the scan
    owns two block counts and the last chunks are partial or empty; the rows of ts_project_fov's mask once per record"""
    from taseg_amd import backend as B
    from taseg_amd.data import tiaf as TF
    from taseg_amd.data.stage import rows_index32
    c = fov_case(g, -1.0)
    proj, p = T(g["proj"]), T(c["pts"][0])
    pix, ok = B.project_fov(p, proj, c["img"], c["crop"], 0.0)
    want = torch.cat([p[ok], pix[ok]], 1)
    n, k, n_rec = len(c["pts"][0]), int(ok.sum()), 220
    assert n * n_rec > 256 * 257 and 0 < k < n
    sample = [0] * 100 + [1] * 7 + [2] * 113
    pose0, pose = T(c["pose0"][0]), T(c["pose"][0])
    entries = [(proj, pose0, pose, {"row_offset": 0.0, "fov_dist": -1.0, "sample": b, "img_w": c["img"][0], "img_h": c["img"][1],
                                    "flags": 0, "first": r * n, "src": 0}) for r, b in enumerate(sample)]
    out, s64, s32, counts = B.tiaf_fov_cloud(p, rows_index32([n] * n_rec, p.device), TF._frame_records(entries, p.device), 3, c["crop"])
    assert counts.tolist() == [100 * k, 7 * k, 113 * k]
    assert torch.equal(out[:n_rec * k].view(torch.int32), want.repeat(n_rec, 1).view(torch.int32))
    want_s = torch.tensor(sample, device=p.device).repeat_interleave(k)
    assert torch.equal(s64[:n_rec * k], want_s) and torch.equal(s32[:n_rec * k], want_s.int())


def test_fov_cloud_checks_its_arguments(g):
    from taseg_amd import backend as B
    p = torch.zeros((4, 4), device="cuda")
    f = torch.zeros(4, dtype=torch.int32, device="cuda")
    rec = torch.zeros((1, 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        B.tiaf_fov_cloud(p, f, rec, 65, (4, 4))
    with pytest.raises(ValueError):
        B.tiaf_fov_cloud(p, f, torch.zeros((1025, 256), dtype=torch.uint8, device="cuda"), 1, (4, 4))
    with pytest.raises(TypeError):
        B.tiaf_fov_cloud(p, f, rec[:, :255], 1, (4, 4))
    with pytest.raises(TypeError):
        B.tiaf_fov_cloud(p, f.long(), rec, 1, (4, 4))
    with pytest.raises(TypeError):
        B.tiaf_fov_cloud(p[:, :3], f, rec, 1, (4, 4))
    with pytest.raises(ValueError):
        B.tiaf_fov_cloud(p, f, rec, 1, (4, 4), lo=torch.zeros((2, 3), device="cuda"))
    with pytest.raises(RuntimeError):
        B.tiaf_fov_cloud(p.cpu(), f, rec, 1, (4, 4))
    # an all-zero record: img_w = 0, nothing projects into it
    assert B.tiaf_fov_cloud(p, f, rec, 1, (4, 4))[3].tolist() == [0]


def test_more_samples_than_the_kernel_takes_fall_back_to_the_per_sample_path(g, frames, monkeypatch):
    from taseg_amd import backend as B
    s = setup(g)
    want = build("batched", frames, s, None, None)
    monkeypatch.setattr(B, "TIAF_MAX_SAMPLES", 1)
    monkeypatch.setattr(B, "tiaf_fov_cloud", lambda *a, **k: pytest.fail("the batched kernel ran"))
    got = build("batched", frames, s, None, None)
    for key in ("lidar_fov_ms", "lidar_ms"):
        assert torch.equal(got[key].C, want[key].C) and torch.equal(got[key].F, want[key].F)
    assert torch.equal(got["image_ms"], want["image_ms"]) and torch.equal(got["semantic_map_ms"], want["semantic_map_ms"])
