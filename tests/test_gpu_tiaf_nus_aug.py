"""nuScenes TIAF stage with augmentation, TTA views and the batched camera side (taseg_amd/data/nuscenes_tiaf.py,
csrc/nusc_tiaf_stage.hip) on the device: the three batches the REAL reference produced (tests/golden/tiaf_nus_aug.npz, inputs from
tests/golden/tiaf_nus.npz) bit for bit on both paths, and ts_nusc_fov_cloud at its edges against the chain of operators it
replaces (ts_project_cam -> index -> ts_fuse_sweeps -> augment_points -> clamp)."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from taseg_amd.data import augment as A
from taseg_amd.data import nuscenes_tiaf as T
from taseg_amd.data.nuscenes import NuscSequence, rotation_matrix, select_sweeps, sweep_params

pytestmark = pytest.mark.gpu

IMG_H, IMG_W = 68, 96
SPARSE = ("lidar", "lidar_ms", "lidar_fov_ms", "targets_fov_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms",
          "targets_mapped", "targets_mapped_ms")
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map", "targets_mapped_ms": "inverse_map_ms",
               "targets_fov_ms": "lidar_ms"}
DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_nus.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_nus_aug.npz"), allow_pickle=False))


def _half(img_u8):
    """the reference's resize (nuscenes_ms_mm.py:380): PIL bilinear to half size - host work, as file decoding is"""
    from PIL import Image
    im = Image.fromarray(img_u8)
    return np.asarray(im.resize((int(im.size[0] * 0.5), int(im.size[1] * 0.5)), Image.BILINEAR))


@pytest.fixture(scope="module")
def inputs(g):
    """the arguments of build_nusc_tiaf_sample for the two samples of tiaf_nus.npz, by name, resident on the device - built once"""
    out, dev, lm = [], "cuda", g["learning_map"]
    for b in range(2):
        p = f"b{b}_"
        seq = NuscSequence(is_key=g[p + "is_key"], key_index=g[p + "key_index"], timestamps=g[p + "timestamps"],
                           scene_tokens=g[p + "scene_tokens"].tolist(), local_indexes=g[p + "local_indexes"], s2l_r=g[p + "s2l_r"],
                           s2l_t=g[p + "s2l_t"], global_indexes=g[p + "global_indexes"], l2e_q=g[p + "key_l2e_q"],
                           l2e_t=g[p + "key_l2e_t"], e2g_q=g[p + "key_e2g_q"], e2g_t=g[p + "key_e2g_t"])
        index, views = int(g[p + "index"]), g[p + "cfg_used_view"].tolist()
        offsets = select_sweeps(seq, index, int(g["multiscan"]), float(g["step"]))
        hl = [torch.from_numpy(lm[g[f"{p}rawlabels_d{-d}"]] if f"{p}rawlabels_d{-d}" in g else
                               np.zeros(len(g[f"{p}points_d{-d}"]), np.int64)).to(dev) for d in offsets]
        fsa = dict(points=torch.from_numpy(g[f"{p}key{index}_points"]).to(dev),
                   labels=torch.from_numpy(lm[g[f"{p}key{index}_rawlabels"]]).to(dev),
                   hist_points=[torch.from_numpy(g[f"{p}points_d{-d}"]).to(dev) for d in offsets], hist_labels=hl,
                   hist_pseudo=[torch.from_numpy(g[f"{p}pseudo_d{-d}"].astype(np.int64)).to(dev) for d in offsets],
                   params=torch.from_numpy(sweep_params(seq, index, offsets)).to(dev))
        n_keys = len(seq.global_indexes)
        cam_frames = {}
        for d in g[p + "image_keyframes"].tolist():
            for v in views:
                i = index + d
                cam_frames[(i, v)] = dict(pose_q=g[f"{p}key{i}_view{v}_pose_q"], pose_t=g[f"{p}key{i}_view{v}_pose_t"],
                                          image=torch.from_numpy(_half(g[f"{p}key{i}_view{v}_image"]).copy()).to(dev),
                                          semantic=torch.from_numpy(g[f"{p}key{i}_view{v}_semantic"]).to(dev))
        out.append(dict(
            fsa=fsa, seq=seq, index=index,
            key_points={i: torch.from_numpy(g[f"{p}key{i}_points"]).to(dev) for i in range(n_keys)},
            key_labels={i: torch.from_numpy(lm[g[f"{p}key{i}_rawlabels"]]).to(dev) for i in range(n_keys)},
            lidar_cs=(g[p + "lidar_cs_q"], g[p + "lidar_cs_t"]),
            view_cs={v: (g[f"{p}view{v}_cs_q"], g[f"{p}view{v}_cs_t"], g[f"{p}view{v}_intrinsic"]) for v in views},
            cam_frames=cam_frames, steps=g["steps"].tolist(), multiscan_image=int(g[p + "cfg_multiscan_image"]),
            step_image=float(g[p + "cfg_step_image"]), interval=int(g[p + "cfg_interval"]), used_view=views,
            paint_dist=float(g[p + "cfg_paint_dist"]), full_image_size=(IMG_W, IMG_H), voxel_size=0.1, rng=None, name=f"s{b}"))
    return out


def _fresh(inputs, g):
    """the inputs with a fresh keyframe-selection generator each (random.sample fills sample 1's image keyframes up)"""
    return [{**inp, "rng": random.Random(int(g[f"b{b}_cfg_rng"]))} for b, inp in enumerate(inputs)]


def _train_params(ga, case):
    flip, scale, jitter, rotate = (bool(v) for v in ga[f"{case}_switches"])
    rng = np.random.RandomState(int(ga[f"{case}_seed"]))
    return [A.draw_train_params(rng, flip=flip, scale=scale, jitter=jitter, rotate=rotate) for _ in range(2)]


def _same(batch, want, prefix, image, semantic, maps=None):
    for key in SPARSE:
        coords = SAME_COORDS.get(key, key)
        assert np.array_equal(batch[key].C.cpu().numpy(), want[f"{prefix}{coords}_C"]), key
        got = batch[key].F.cpu().numpy()
        assert np.array_equal(got, want[f"{prefix}{key}_F"]) and (got.dtype == np.float32) == (want[f"{prefix}{key}_F"].dtype == np.float32), key
    for key in DENSE:
        assert np.array_equal(batch[key].cpu().numpy().reshape(-1), want[f"{prefix}{key}"].reshape(-1)), key
    assert np.array_equal(batch["image_ms"].cpu().numpy(), image)
    assert np.array_equal(batch["semantic_map_ms"].cpu().numpy(), semantic)
    if maps is not None:
        for key in ("depth_map_ms", "lidar_map_ms"):
            assert list(batch[key].shape) == want[f"{maps}{key}_shape"].tolist() and not bool(batch[key].any()), key
    else:
        assert "depth_map_ms" not in batch and "lidar_map_ms" not in batch


@pytest.mark.parametrize("path", ["per_sample", "batched"])
@pytest.mark.parametrize("case", ["train", "norot"])
def test_training_batches_match_the_reference(g, ga, inputs, case, path):
    aug = _train_params(ga, case)
    if path == "per_sample":
        batch = T.build_nusc_tiaf_batch([T.build_nusc_tiaf_sample(**inp, aug=p) for inp, p in zip(_fresh(inputs, g), aug)])
    else:
        batch = T.build_nusc_tiaf_batch_from_keyframes(_fresh(inputs, g), aug=aug, zero_maps=True)
    _same(batch, ga, f"{case}_batch_", g["batch_image_ms"], g["batch_semantic_map_ms"], maps=f"{case}_batch_")


@pytest.mark.parametrize("path", ["per_sample", "batched"])
def test_tta_batch_matches_the_reference(g, ga, inputs, path):
    lo, hi = ga["tta_votes"].tolist()
    inp = _fresh(inputs, g)[int(ga["tta_sample"])]
    rng = np.random.RandomState(int(ga["tta_seed"]))
    if path == "per_sample":
        frames = T.select_image_keyframes(inp["seq"], inp["index"], inp["multiscan_image"], inp["step_image"], inp["rng"])
        batch = T.build_nusc_tiaf_batch([T.build_nusc_tiaf_sample(**inp, aug=A.draw_tta_params(rng, v), image_keyframes=frames)
                                         for v in range(lo, hi)])
    else:
        batch = T.build_nusc_tiaf_tta_batch(inp, lo, hi, rng, zero_maps=True)
    image = np.concatenate([g["b0_image_ms"]] * (hi - lo)).transpose(0, 3, 1, 2)
    semantic = np.concatenate([g["b0_semantic_map_ms"]] * (hi - lo)).transpose(0, 3, 1, 2)
    _same(batch, ga, "tta_batch_", image, semantic, maps="tta_batch_")


def test_batched_path_without_augmentation_is_the_unaugmented_fixture_and_the_per_sample_path(g, inputs):
    batch = T.build_nusc_tiaf_batch_from_keyframes(_fresh(inputs, g))
    ref = T.build_nusc_tiaf_batch([T.build_nusc_tiaf_sample(**inp) for inp in _fresh(inputs, g)])
    for key in ("lidar", "lidar_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms", "targets_mapped", "targets_mapped_ms",
                "lidar_fov_ms", "targets_fov_ms"):
        for part in ("C", "F"):
            got = getattr(batch[key], part).cpu().numpy()
            assert np.array_equal(got, g[f"batch_{key}_{part}"]), key
            assert np.array_equal(got, getattr(ref[key], part).cpu().numpy()), key
    for key in ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img", "image_ms", "semantic_map_ms"):
        assert np.array_equal(batch[key].cpu().numpy().reshape(-1), g[f"batch_{key}"].reshape(-1)), key
        assert torch.equal(batch[key], ref[key]), key
    assert "depth_map_ms" not in batch and list(ref["depth_map_ms"].shape) == g["batch_depth_map_ms_shape"].tolist()
    assert batch["name"] == ref["name"] == ["s0", "s1"]


def test_above_the_limits_the_builders_fall_back_to_the_per_sample_path(g, ga, inputs, monkeypatch):
    """more samples than TS_TIAF_MAX_SAMPLES / more records than TS_TIAF_MAX_FRAMES: the limits lowered so that the fixture's
    batches pass them - the same tensors, through build_nusc_tiaf_sample, and the kernel is not called"""
    from taseg_amd import backend as B

    def no_kernel(*a, **k):
        raise AssertionError("the batched kernel was called above the limits")
    monkeypatch.setattr(B, "nusc_fov_cloud", no_kernel)
    monkeypatch.setattr(B, "TIAF_MAX_SAMPLES", 1)                      # two samples: over
    batch = T.build_nusc_tiaf_batch_from_keyframes(_fresh(inputs, g), aug=_train_params(ga, "train"), zero_maps=True)
    _same(batch, ga, "train_batch_", g["batch_image_ms"], g["batch_semantic_map_ms"], maps="train_batch_")
    monkeypatch.setattr(B, "TIAF_MAX_SAMPLES", 64)
    monkeypatch.setattr(B, "TIAF_MAX_FRAMES", 17)                      # 6 + 12 = 18 records, three votes of 6 records: over
    batch = T.build_nusc_tiaf_batch_from_keyframes(_fresh(inputs, g), aug=_train_params(ga, "norot"))
    _same(batch, ga, "norot_batch_", g["batch_image_ms"], g["batch_semantic_map_ms"])
    lo, hi = ga["tta_votes"].tolist()
    batch = T.build_nusc_tiaf_tta_batch(_fresh(inputs, g)[0], lo, hi, np.random.RandomState(int(ga["tta_seed"])), zero_maps=True)
    _same(batch, ga, "tta_batch_", np.concatenate([g["b0_image_ms"]] * (hi - lo)).transpose(0, 3, 1, 2),
          np.concatenate([g["b0_semantic_map_ms"]] * (hi - lo)).transpose(0, 3, 1, 2), maps="tta_batch_")


def test_samples_that_shape_the_image_tensor_differently_are_refused(g, inputs):
    a, b = _fresh(inputs, g)                 # (a call consumes the keyframe-selection generators: fresh ones for every call)
    with pytest.raises(ValueError, match="share full_image_size and crop_top"):
        T.build_nusc_tiaf_batch_from_keyframes([a, {**b, "crop_top": 4}])
    a, b = _fresh(inputs, g)
    with pytest.raises(ValueError, match="share full_image_size and crop_top"):
        T.build_nusc_tiaf_batch_from_keyframes([a, {**b, "full_image_size": (IMG_W, IMG_H + 2)}])
    a, b = _fresh(inputs, g)
    frames = {k: {**f, "image": f["image"][:, :-2].contiguous(), "semantic": f["semantic"][:, :-2].contiguous()}
              for k, f in b["cam_frames"].items()}
    with pytest.raises(ValueError, match="share one size"):
        T.build_nusc_tiaf_batch_from_keyframes([a, {**b, "cam_frames": frames}])


# ------------------------------------------------------------------------------------------------ the kernel at its edges
def _camera(rs, yaw_deg, crop_top=2):
    """a camera of 96 x 68 pixels looking along `yaw` in the lidar's x-y plane, every stage of the chain a slightly perturbed rigid
    motion (so that no product is exact)"""
    def rot(q):
        q = np.asarray(q, dtype=np.float64)
        return rotation_matrix(q / np.linalg.norm(q))
    a = np.deg2rad(yaw_deg)
    to_ego = np.stack([[np.sin(a), -np.cos(a), 0.0], [0.0, 0.0, -1.0], [np.cos(a), np.sin(a), 0.0]], axis=1)     # camera -> ego
    cam = np.zeros(57, dtype=np.float64)
    cam[0:9], cam[9:12] = rot([1.0, 0.001, -0.002, 0.003]).reshape(-1), [0.9, 0.01, 1.8]
    pose = rot([0.98, 0.002, 0.001, 0.2])
    cam[12:21], cam[21:24] = pose.reshape(-1), [410.25, 1180.5, 0.3]
    cam[24:27], cam[27:36] = [410.26, 1180.49, 0.3], np.ascontiguousarray(pose.T).reshape(-1)
    cam[36:39], cam[39:48] = [1.5, 0.1, 1.5], np.ascontiguousarray((to_ego @ rot([1.0, 0.002, 0.001, -0.001])).T).reshape(-1)
    cam[48:57] = np.array([[70.0 + rs.rand(), 0.0, IMG_W / 2 - 1.3], [0.0, 71.0, IMG_H / 2 + 0.7], [0.0, 0.0, 1.0]]).reshape(-1)
    return cam


def _move(rs, identity=False):
    if identity:          # (what relative_transform(current, current) gives: an identity with rounding dust)
        return np.concatenate([(np.eye(3) + 1e-17).reshape(-1), [1e-16, 0.0, -1e-16]])
    q = np.array([1.0, 0.002, -0.001, 0.05 * rs.randn()])
    return np.concatenate([rotation_matrix(q / np.linalg.norm(q)).reshape(-1), rs.randn(3) * [2.0, 0.5, 0.05]])


def _record(rs, src, n, sample, yaw=0.0, paint=-1.0, crop_top=2, image=0, identity=False):
    return dict(cam=_camera(rs, yaw), move=_move(rs, identity), row_offset=float(32 * image), paint_dist=paint, sample=sample,
                img_w=IMG_W, img_h=IMG_H, crop_top=crop_top, src=src, n=n)


def _points(rs, n, nan_rows=0):
    pts = (rs.randn(n, 4) * [12.0, 12.0, 1.5, 50.0] + [0.0, 0.0, -0.5, 100.0]).astype(np.float32)
    for r in rs.choice(n, nan_rows, replace=False) if nan_rows else ():
        pts[r, rs.randint(0, 3)] = np.nan
    return pts


DEAD = 1 << 20           # a crop_top no pixel reaches: the view keeps nothing


def _case(name):
    """(points, labels, pre_keep or None, records, n_samples, aug or None, lo or None)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    aug = lo = keep = None
    nb = 1
    if name.startswith("rows_"):
        n = int(name[5:])
        pts, recs = _points(rs, n), [_record(rs, 0, n, 0, identity=True)]
    elif name == "boundary_in_a_wave_and_an_empty_record":
        pts, nb = _points(rs, 500), 2
        recs = [_record(rs, 0, 100, 0), _record(rs, 100, 37, 0, yaw=180.0, image=1), _record(rs, 137, 0, 1, yaw=90.0),
                _record(rs, 137, 363, 1, yaw=10.0, identity=True)]
    elif name == "a_view_and_a_whole_sample_keep_nothing":
        pts, nb = _points(rs, 900), 3
        recs = [_record(rs, 0, 300, 0), _record(rs, 0, 300, 0, crop_top=DEAD, image=1), _record(rs, 300, 300, 1, crop_top=DEAD),
                _record(rs, 300, 300, 1, paint=1e-6, image=1), _record(rs, 600, 300, 2, yaw=200.0)]
    elif name == "a_block_without_survivors":
        pts = _points(rs, 1100)
        recs = [_record(rs, 0, 512, 0), _record(rs, 512, 256, 0, crop_top=DEAD, image=1), _record(rs, 768, 332, 0, yaw=170.0, image=2)]
    elif name == "pre_keep_paint_and_nan":
        pts, nb = _points(rs, 1000, nan_rows=60), 2
        keep = (rs.rand(1000) < 0.7).astype(np.uint8)
        recs = [_record(rs, 0, 600, 0, paint=15.0), _record(rs, 0, 600, 0, yaw=180.0, image=1),
                _record(rs, 600, 400, 1, paint=9.0), _record(rs, 600, 400, 1, yaw=180.0, paint=-1.0, image=1)]
        lo = np.array([[-40.0, -40.0, -1.0], [-40.0, np.nan, -40.0]], dtype=np.float32)         # (a NaN corner keeps nothing)
    elif name == "clamp_rejects_only_after_the_augmentation":
        pts, nb = _points(rs, 700), 2
        recs = [_record(rs, 0, 350, 0), _record(rs, 350, 350, 1, identity=True)]
        # x -> -x turns the rows in front of the camera negative: corners that pass every un-augmented row cut the far ones
        aug = [A.AugParams(flip=1, flip_on=True, translate=(0.0, 0.0, 1.0), translate_on=True),
               A.AugParams(flip=3, flip_on=True, scale=1.05, scale_on=True)]                              # (scaled in float32)
        lo = np.array([[-8.0, -80.0, -80.0], [-9.0, -80.0, -80.0]], dtype=np.float32)
    elif name == "views_of_a_tta_batch_share_the_point_rows":
        pts, nb = _points(rs, 400), 3
        recs = [_record(np.random.RandomState(1), 0, 400, b, identity=True) for b in range(3)]
        rng = np.random.RandomState(2)
        aug = [A.draw_tta_params(rng, v) for v in (3, 4, 9)]
        lo = np.array([[-7.0, -7.0, -3.0]] * 3, dtype=np.float32)
    elif name == "sixty_four_samples":
        pts, nb = _points(rs, 64 * 10), 64
        recs = [_record(rs, 10 * b, 10, b, yaw=45.0 * b) for b in range(64)]
        aug = [A.draw_train_params(np.random.RandomState(b), rotate=bool(b % 2)) for b in range(64)]
    elif name == "three_samples_past_256_blocks":
        # 66 000 virtual rows = 258 blocks: the shared scan's threads sum chunks of two block counts (one up to 256 blocks)
        pts, nb = _points(rs, 22000), 3
        recs = [_record(rs, 0, 22000, 0, identity=True), _record(rs, 0, 22000, 1, yaw=120.0), _record(rs, 0, 22000, 2, yaw=240.0)]
        aug = [A.AugParams(scale=1.05, scale_on=True, translate=(0.1, -0.2, 0.05), translate_on=True),
               A.draw_tta_params(np.random.RandomState(3), 3), A.AugParams(flip=3, flip_on=True)]
        lo = np.array([[8.0, -80.0, -80.0], [-80.0, -80.0, -0.6], [-80.0, -80.0, 0.1]], dtype=np.float32)
    elif name == "sample_and_point_rows_out_of_range":
        pts, nb = _points(rs, 300), 2
        recs = [_record(rs, 0, 100, 0), _record(rs, 100, 100, -1), _record(rs, 100, 100, 2), _record(rs, 280, 50, 1),
                _record(rs, -10, 30, 1, image=1)]
    else:
        raise KeyError(name)
    labels = rs.randint(0, 17, size=len(pts)).astype(np.int64)
    return pts, labels, keep, recs, nb, aug, lo


def _table(recs):
    table, first = np.zeros(len(recs), dtype=T.CAM_FRAME_DTYPE), 0
    for t, r in zip(table, recs):
        for k in ("cam", "move", "row_offset", "paint_dist", "sample", "img_w", "img_h", "crop_top", "src"):
            t[k] = r[k]
        t["first"] = first
        first += r["n"]
    return torch.from_numpy(table.view(np.uint8).reshape(len(recs), T.CAM_FRAME_DTYPE.itemsize)).cuda()


def _device(case):
    pts, labels, keep, recs, nb, aug, lo = case
    frame = torch.from_numpy(np.repeat(np.arange(len(recs), dtype=np.int32), [r["n"] for r in recs])).cuda()
    return dict(points=torch.from_numpy(pts).cuda(), labels=torch.from_numpy(labels).cuda(), frame=frame, records=_table(recs),
                n_samples=nb, pre_keep=None if keep is None else torch.from_numpy(keep).cuda(),
                aug=None if aug is None else torch.from_numpy(A.pack_params(aug)).cuda(), lo=None if lo is None else torch.from_numpy(lo).cuda())


def _chain(d, recs):
    """what the kernel replaces, a record at a time: ego-box byte, paint radius, ts_project_cam, boolean index, ts_fuse_sweeps
    (flagB), augment_points, clamp"""
    from taseg_amd import backend as B
    n_points, nb = d["points"].shape[0], d["n_samples"]
    fov, labs, samples = [], [], []
    for r in recs:
        if not 0 <= r["sample"] < nb:
            continue
        a, b = max(r["src"], 0), min(r["src"] + r["n"], n_points)
        if b <= a:
            continue
        pts, lab = d["points"][a:b], d["labels"][a:b]
        if d["pre_keep"] is not None:
            sel = d["pre_keep"][a:b].bool()
            pts, lab = pts[sel], lab[sel]
        if r["paint_dist"] > 0:
            near = torch.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) <= r["paint_dist"]
            pts, lab = pts[near], lab[near]
        pts = pts.contiguous()
        pix, ok = B.project_cam(pts, torch.from_numpy(r["cam"]).cuda(), (r["img_w"], r["img_h"]), r["crop_top"], r["row_offset"])
        pts, pix, lab = pts[ok], pix[ok], lab[ok]
        params = np.zeros((1, 28), dtype=np.float64)
        params[0, 13:25], params[0, 25] = r["move"], 1.0
        five = torch.cat([pts, torch.zeros((pts.shape[0], 1), dtype=torch.float32, device="cuda")], 1).contiguous()
        moved, _ = B.fuse_sweeps(five, torch.zeros(pts.shape[0], dtype=torch.int32, device="cuda"), torch.from_numpy(params).cuda())
        cloud = torch.cat([moved[:, :4], pix], 1)
        if d["aug"] is not None and cloud.shape[0]:
            cloud = A.augment_points(cloud, d["aug"][r["sample"]:r["sample"] + 1])
        if d["lo"] is not None:
            inside = (cloud[:, :3] >= d["lo"][r["sample"]]).all(1)
            cloud, lab = cloud[inside], lab[inside]
        fov.append(cloud)
        labs.append(lab)
        samples.append(torch.full((cloud.shape[0],), r["sample"], dtype=torch.int64, device="cuda"))
    return torch.cat(fov, 0), torch.cat(labs, 0), torch.cat(samples, 0)


CASES = ["rows_1", "rows_255", "rows_256", "rows_257", "rows_%d" % (64 * 256 + 3), "boundary_in_a_wave_and_an_empty_record",
         "a_view_and_a_whole_sample_keep_nothing", "a_block_without_survivors", "pre_keep_paint_and_nan",
         "clamp_rejects_only_after_the_augmentation", "views_of_a_tta_batch_share_the_point_rows", "sixty_four_samples",
         "sample_and_point_rows_out_of_range", "three_samples_past_256_blocks"]


@pytest.mark.parametrize("name", CASES)
def test_fov_cloud_kernel_equals_the_chain_it_replaces(name):
    from taseg_amd import backend as B
    case = _case(name)
    d = _device(case)
    want, want_lab, want_sample = _chain(d, case[3])
    out, lab, sample, sample32, counts = B.nusc_fov_cloud(**d)
    again = B.nusc_fov_cloud(**d)
    n = int(counts.sum())
    assert counts.tolist() == torch.bincount(want_sample, minlength=d["n_samples"]).tolist()
    assert n == want.shape[0] and (n > 0 or name == "rows_1")
    assert np.array_equal(out[:n].cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))         # bit for bit
    assert torch.equal(lab[:n], want_lab) and torch.equal(sample[:n], want_sample) and torch.equal(sample32[:n].long(), want_sample)
    # two runs, the same bytes
    assert torch.equal(again[4], counts) and all(torch.equal(a[:n].view(torch.int32) if a.dtype == torch.float32 else a[:n], b)
                                                 for a, b in zip(again[:4], (out[:n].view(torch.int32), lab[:n], sample[:n], sample32[:n])))
    if name == "a_view_and_a_whole_sample_keep_nothing":
        assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    if name == "pre_keep_paint_and_nan":
        assert counts[0] > 0 and counts[1] == 0 and not bool(torch.isnan(out[:n, :3]).any())
    if name == "clamp_rejects_only_after_the_augmentation":
        bare, free = B.nusc_fov_cloud(**{**d, "aug": None})[4], B.nusc_fov_cloud(**{**d, "aug": None, "lo": None})[4]
        unclamped = B.nusc_fov_cloud(**{**d, "lo": None})[4]
        assert torch.equal(bare, free) and torch.equal(unclamped, free)       # the corners pass every un-augmented row ...
        assert (counts < free).all() and (counts > 0).all()                   # ... and not every augmented one
    if name == "sample_and_point_rows_out_of_range":
        assert int(counts[0]) > 0
    if name == "three_samples_past_256_blocks":                               # every sample keeps some rows and loses some to its corner
        free = torch.bincount(_chain({**d, "lo": None}, case[3])[2], minlength=3)
        assert d["frame"].shape[0] == 66000 and (counts > 0).all() and (counts < free).all()


def _raw_call(d, out, capacity):
    """ts_nusc_fov_cloud on outputs the caller made (the wrapper sizes them itself)"""
    from taseg_amd import _lib as L
    lib = L.load()
    m, nb = d["frame"].shape[0], d["n_samples"]
    lab, s64 = torch.full((out.shape[0],), -7, dtype=torch.int64, device="cuda"), torch.full((out.shape[0],), -7, dtype=torch.int64, device="cuda")
    s32, counts = torch.full((out.shape[0],), -7, dtype=torch.int32, device="cuda"), torch.full((nb,), -7, dtype=torch.int64, device="cuda")
    ws_bytes = lib.ts_nusc_fov_cloud_workspace_bytes(m, nb)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = lib.ts_nusc_fov_cloud(L.ptr(d["points"]), L.ptr(d["labels"]), L.ptr(d["pre_keep"]), d["points"].shape[0], L.ptr(d["frame"]), m,
                               L.ptr(d["records"]), d["records"].shape[0], L.ptr(d["aug"]), L.ptr(d["lo"]), nb, L.ptr(out), L.ptr(lab),
                               L.ptr(s64), L.ptr(s32), capacity, L.ptr(counts), L.ptr(ws), ws_bytes, L.stream())
    torch.cuda.synchronize()
    return rc, lab, s64, s32, counts


def test_rows_behind_the_survivors_keep_the_sentinel_and_a_small_capacity_is_refused():
    case = _case("pre_keep_paint_and_nan")
    d = _device(case)
    m = d["frame"].shape[0]
    sentinel = -12345.0
    out = torch.full((m + 5, 6), sentinel, dtype=torch.float32, device="cuda")
    rc, lab, s64, s32, counts = _raw_call(d, out, m + 5)
    n = int(counts.sum())
    assert rc == 0 and 0 < n < m
    want = _chain(d, case[3])[0]
    assert torch.equal(out[:n], want)
    assert bool((out[n:] == sentinel).all()) and bool((lab[n:] == -7).all()) and bool((s64[n:] == -7).all()) and bool((s32[n:] == -7).all())
    # capacity < n_rows: an error, nothing launched - no output is touched, the counts included
    out2 = torch.full((m, 6), sentinel, dtype=torch.float32, device="cuda")
    rc, lab, s64, s32, counts = _raw_call(d, out2, m - 1)
    assert rc != 0
    assert bool((out2 == sentinel).all()) and bool((lab == -7).all()) and bool((counts == -7).all())
