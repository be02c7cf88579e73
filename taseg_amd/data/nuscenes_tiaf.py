"""nuScenes TIAF (temporal image aggregation and fusion) data stage on the device - the camera side of
R/pcseg/data/dataset/nuscenes/nuscenes_ms_mm.py:196-401 and the voxelisation / collate of
nuscenes_voxel_ms_mm.py:77-262, next to the nuScenes FSA stage of taseg_amd.data.nuscenes:

  host (a few 3x3 products per image keyframe)
      select_image_keyframes   which keyframes' camera images join the stack (:204-236): the keyframe nearest to every
                               STEP_IMAGE metres of driven distance up to MULTISCAN_IMAGE, filled up from the passed-over
                               ones with random.sample (the caller's `rng`), plus the current one
      camera_chain             the 57 doubles ts_project_cam consumes: lidar -> ego -> global -> camera ego -> camera
                               (calibrated-sensor / ego-pose records, :349-367) and the intrinsic
  device, per image keyframe
      ts_fuse_sweeps           the keyframe's points and those of its MULTISCAN_INTERVAL predecessors in ITS lidar frame,
                               ego box cut, time delta to the current keyframe (:246-295); paint radius (:297-300)
      ts_project_cam           per used camera: projection, in-image test, half-resolution pixel, top rows cut, the row
                               shifted by HEIGHT * (position of the image in the stack)            (:349-398)
      ts_fuse_sweeps           the kept points into the current lidar frame (:305; float64 product rounded once)
      image                    half-resolution uint8 RGB -> float32 BGR / 255, the two top rows cut (:381-386)
  sample / batch               the three clouds (current, fused, FOV) voxelised with ONE coordinate shift, the FOV cloud
                               clamped to the current cloud's corner (stage.voxelize_fov); sparse collate + image stacks
                               as NCHW + offset_img

Two ways to build a batch, the same tensors bit for bit:
  build_nusc_tiaf_sample + build_nusc_tiaf_batch   per sample, per image keyframe and per view, from the operators every stage
                        shares (ts_fuse_sweeps, ts_project_cam, a boolean index, ts_stage_augment, the ATen clamp) - the cross-check
  build_nusc_tiaf_batch_from_keyframes             the camera side of the whole batch as ONE ts_fuse_sweeps over every image
                        keyframe's rows, one record table, ts_nusc_fov_cloud (csrc/nusc_tiaf_stage.hip: ego box, paint radius,
                        projection, move, augmentation and clamp per (point row, camera record) pair, one stable compaction with
                        one host read) and ts_tiaf_image_stack, the frames straight into the NCHW planes with the cut rows as a
                        pointer offset; the LiDAR side stays per sample.  build_nusc_tiaf_tta_batch: the TTA views on it.
                        The default: 3.35 against 7.35 ms at the recipe's shape (profiles/nusc_tiaf_stage.txt).

Training augments the three clouds of a sample with ONE draw (aug_points_rgb_ms, nuscenes_voxel_ms_mm.py:92-104) before both clamps
and the three voxelisations.  The draws stay on the host, on a `np.random.RandomState` consumed as the reference consumes numpy's
global generator: `augment.draw_train_params(rng)` per sample, exactly as for FSA - NuscenesMsMmDataset.__getitem__ draws no image
flip and no mix coin - and under TTA one scale per vote (`augment.draw_tta_params`).  The image keyframes' random fill-up is Python's
`random.sample` on the first read of a sample only (the reference caches the selection per sample token): `rng` of the sample's
arguments, or `image_keyframes` for a selection made earlier.

    aug = [draw_train_params(rng) for _ in inputs]                      # inputs[b]: the arguments of build_nusc_tiaf_sample, by name
    batch = build_nusc_tiaf_batch_from_keyframes(inputs, aug=aug)
    tta = build_nusc_tiaf_tta_batch(inputs[0], 0, 10, rng)

Reproduced rather than repaired: `targets_fov_ms` pairs the FOV labels with `lidar_ms.C`, the fused cloud's coordinates (:197); the
current keyframe's rows go through the rounded identity relative_transform(current, current) gives (nuscenes_ms_mm.py:305); the TTA
scale comes from SCALE_AUG_RANGE (the `scale_aug_range` assignment of :110 names an attribute nothing reads); `depth_map_ms` /
`lidar_map_ms` are all zeros at full resolution (the batched builders make them only under zero_maps=True).
Not here: file decoding (JPEG, .npy semantic maps) and PIL's bilinear half-size resize (:380), host work as in the reference - the
stage starts from resident half-resolution uint8 images; IMAGE_JITTER and IMAGE_FLIP (the recipe sets both False, and the nuScenes
file never applies a flip); PolarMix / LaserMix (the recipe sets AUGMENT 'none').  Bit-exact against the reference's dataset code:
tests/golden/tiaf_nus.npz, tests/golden/tiaf_nus_aug.npz.
"""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import backend as B
from ..torchsparse import SparseTensor
from .augment import augment_points, draw_tta_params
from .nuscenes import NuscSequence, _current_keyframe, fuse_sweeps, relative_transform, rotation_matrix
from .stage import _aug_records, _one_aug, clamp_corner, rows_index32, voxelize_fov, voxelize_sample_ms
from .tiaf import _camera_batch_head, _camera_batch_tail, _unit_table, bgr_unit, build_tiaf_batch

__all__ = ["select_image_keyframes", "camera_chain", "frame_cloud", "fov_points", "half_image", "build_nusc_tiaf_sample",
           "build_nusc_tiaf_batch", "build_nusc_tiaf_batch_from_keyframes", "build_nusc_tiaf_tta_batch", "CAM_FRAME_DTYPE"]

# TsNuscCamFrame of include/taseg_hip.h: the per-(keyframe, view) record of ts_nusc_fov_cloud
CAM_FRAME_DTYPE = np.dtype([("cam", "<f8", 57), ("move", "<f8", 12), ("row_offset", "<f4"), ("paint_dist", "<f4"), ("sample", "<i4"),
                            ("img_w", "<i4"), ("img_h", "<i4"), ("crop_top", "<i4"), ("first", "<i4"), ("src", "<i4")])


def _scene_of(seq: NuscSequence, key: int):
    return seq.scene_tokens[int(seq.global_indexes[key])]


def select_image_keyframes(seq: NuscSequence, index: int, multiscan_image: int, step_image: float, rng) -> List[int]:
    """Keyframe offsets (ascending, the current one = 0 last) whose images are stacked (nuscenes_ms_mm.py:204-236).
    `rng.sample` plays the part of the reference's global random.sample."""
    if multiscan_image == 0:
        return [0]
    n_keys = len(seq.global_indexes)
    delta, total, dist = 0, [], []
    while not dist or dist[-1] <= multiscan_image * step_image:
        delta -= 1
        other = (index + delta) % n_keys            # a negative index wraps, as the reference's list indexing does
        if _scene_of(seq, other) != _scene_of(seq, index):
            dist.append(1000)
            break
        _, trans = relative_transform(seq, index, other)       # the lidar origin of that keyframe in the current frame
        total.append(delta)
        dist.append(float(np.linalg.norm(trans[:2], ord=2)))
    cur, picked, passed = 1, [], []
    for i in range(len(total)):
        if dist[i] - cur * step_image > 0 or (dist[i] < dist[i + 1] and abs(dist[i] - cur * step_image) < abs(dist[i + 1] - cur * step_image)):
            picked.append(total[i])
            cur += 1
        else:
            passed.append(total[i])
        if cur > multiscan_image:
            break
    if len(picked) < multiscan_image and passed:
        picked += rng.sample(passed, min(multiscan_image - len(picked), len(passed)))
    return sorted(set(picked)) + [0]


def camera_chain(lidar_cs_q, lidar_cs_t, lidar_pose_q, lidar_pose_t, cam_pose_q, cam_pose_t, cam_cs_q, cam_cs_t,
                 intrinsic) -> np.ndarray:
    """[57] float64 for ts_project_cam (layout: include/taseg_hip.h)."""
    out = np.zeros(57, dtype=np.float64)
    out[0:9] = rotation_matrix(lidar_cs_q).reshape(-1)
    out[9:12] = lidar_cs_t
    out[12:21] = rotation_matrix(lidar_pose_q).reshape(-1)
    out[21:24] = lidar_pose_t
    out[24:27] = cam_pose_t
    out[27:36] = np.ascontiguousarray(rotation_matrix(cam_pose_q).T).reshape(-1)
    out[36:39] = cam_cs_t
    out[39:48] = np.ascontiguousarray(rotation_matrix(cam_cs_q).T).reshape(-1)
    out[48:57] = np.asarray(intrinsic, dtype=np.float64).reshape(-1)
    return out


def _move(points5: torch.Tensor, seq: NuscSequence, key0: int, frames: Sequence[int], lengths: Sequence[int], stamp0: int):
    """ts_fuse_sweeps over the concatenated clouds of keyframes `frames` (rows of `lengths`): frame f into the lidar frame of
    key0 (no product for f == key0... unless `always`), column 4 = time delta to `stamp0`; returns (moved, outside-ego-box)"""
    params = np.zeros((len(frames), 28), dtype=np.float64)
    for i, f in enumerate(frames):
        if f != key0:
            rot, trans = relative_transform(seq, key0, f)
            params[i, 13:22], params[i, 22:25], params[i, 25] = rot.reshape(-1), trans, 1.0
        params[i, 26] = stamp0 / 1e6 - seq.timestamps[int(seq.global_indexes[f])] / 1e6
    dev = points5.device
    idx = torch.repeat_interleave(torch.arange(len(frames), dtype=torch.int32), torch.tensor(list(lengths))).to(dev)
    return B.fuse_sweeps(points5.contiguous(), idx, torch.from_numpy(params).to(dev))


def _cloud_keyframes(seq: NuscSequence, index: int, delta: int, prev_delta: Optional[int], interval: int) -> List[int]:
    """image keyframe index + delta and those of its `interval` predecessors that lie in the scene and were not already part of the
    previous image keyframe's cloud (nuscenes_ms_mm.py:262-279)"""
    i = index + delta
    frames = [i]
    for meta in range(-interval, 0):
        j = i + meta
        if j < 0 or j >= len(seq.global_indexes) or _scene_of(seq, j) != _scene_of(seq, index):
            continue
        if prev_delta is not None and delta + meta <= prev_delta:
            continue
        frames.append(j)
    return frames


def frame_cloud(seq: NuscSequence, index: int, delta: int, prev_delta: Optional[int], interval: int,
                key_points: Dict[int, torch.Tensor], key_labels: Dict[int, torch.Tensor], paint_dist: float):
    """The cloud image keyframe index + delta projects (nuscenes_ms_mm.py:246-300): (raw [m,5] float32 in ITS lidar frame,
    labels [m])."""
    i = index + delta
    frames = _cloud_keyframes(seq, index, delta, prev_delta, interval)
    pts = torch.cat([key_points[f] for f in frames], 0)
    lab = torch.cat([key_labels[f].long() for f in frames], 0)
    moved, no_ego = _move(pts, seq, i, frames, [key_points[f].shape[0] for f in frames],
                          int(seq.timestamps[int(seq.global_indexes[index])]))
    moved, lab = moved[no_ego], lab[no_ego]
    if paint_dist > 0:
        radius = torch.sqrt(moved[:, 0] * moved[:, 0] + moved[:, 1] * moved[:, 1])
        near = radius <= paint_dist
        moved, lab = moved[near], lab[near]
    return moved, lab


def fov_points(cloud: torch.Tensor, labels: torch.Tensor, cam: torch.Tensor, image_size, crop_top: int, height: int,
               img_batch: int):
    """get_fov_points (:329-401) on the device: ([m, 6] = x, y, z, intensity, row + height * img_batch, col; labels [m])."""
    pts = cloud[:, :4].contiguous()
    pix, keep = B.project_cam(pts, cam, image_size, crop_top, float(height * img_batch))
    return torch.cat([pts[keep], pix[keep]], 1), labels[keep]


def half_image(image_u8: torch.Tensor, crop_top: int = 2) -> torch.Tensor:
    """[h, w, 3] uint8 RGB at half resolution -> float32 BGR / 255 (taseg_amd.data.tiaf.bgr_unit) without the top rows (:381-386)"""
    return bgr_unit(image_u8)[crop_top:].contiguous()


def _lidar_side(fsa: Dict, steps, in_feature_dim: int, voxel_size: float, name: str, rec: Optional[torch.Tensor]):
    """The single-frame and fused clouds of one sample: the FSA stage (voxel_ms_mm.py:80-87, 127-186 == nuscenes_voxel_ms.py), both
    through the sample's augmentation record `rec` (float64 [1, 8] on the device, or None) first (:92-125).  Returns (the sample of
    voxelize_sample_ms with its "_shift", the - augmented - single-frame cloud)."""
    raw, lab_all, keep = fuse_sweeps(fsa["points"], fsa["labels"], fsa["hist_points"], fsa["hist_labels"], fsa["hist_pseudo"],
                                     fsa["params"], steps)
    point = _current_keyframe(fsa["points"], in_feature_dim)
    fused = raw[:, :in_feature_dim].contiguous()
    if rec is not None:
        point, fused = augment_points(point, rec), augment_points(fused, rec)
    return voxelize_sample_ms(point, fsa["labels"].long(), fused, lab_all, voxel_size, name, keep=keep, return_shift=True), point


def build_nusc_tiaf_sample(fsa: Dict, seq: NuscSequence, index: int, key_points: Dict[int, torch.Tensor],
                           key_labels: Dict[int, torch.Tensor], lidar_cs, view_cs: Dict[int, tuple],
                           cam_frames: Dict[tuple, Dict], steps: Sequence[int], multiscan_image: int, step_image: float,
                           interval: int, used_view: Sequence[int], paint_dist: float, full_image_size, voxel_size: float,
                           rng, in_feature_dim: int = 4, crop_top: int = 2, name: str = "", aug=None, zero_maps: bool = True,
                           image_keyframes: Optional[Sequence[int]] = None) -> Dict:
    """One sample of NuscVoxelMsMmDataset (nuscenes_voxel_ms_mm.py:77-223) from resident tensors.

    fsa          the FSA inputs of the keyframe, as taseg_amd.data.nuscenes.build_nuscenes_batch takes them (points, labels,
                 hist_points / hist_labels / hist_pseudo, params)
    key_points / key_labels   {keyframe: raw [n,5] float32 / mapped labels} of the keyframes the image side touches
    lidar_cs     (rotation q, translation) of the lidar's calibrated sensor; the lidar's ego pose = the keyframe's e2g pose
    view_cs      {view: (rotation q, translation, intrinsic [3,3])} of the cameras' calibrated sensors
    cam_frames   {(keyframe, view): dict(pose_q, pose_t, image uint8 [h,w,3] RGB at HALF resolution, semantic [h,w,1])}
    full_image_size   (W, H) of the camera images before the half-size resize
    aug          the sample's AugParams: ONE record augments the single-frame cloud, the fused cloud and the [m, 6] FOV cloud
                 (augment_points) before both clamps and the three voxelisations (:92-135).  None: the path without it, launch
                 for launch.
    zero_maps    False leaves the all-zero `depth_map_ms` / `lidar_map_ms` (:346-347) out
    image_keyframes   the image keyframes selected earlier (the reference caches them per sample token: `rng` is then not used)"""
    frames = list(image_keyframes) if image_keyframes is not None else \
        select_image_keyframes(seq, index, multiscan_image, step_image, rng)
    w_full, h_full = full_image_size
    height = h_full // 2 - crop_top
    dev = fsa["points"].device
    fov, fov_lab, images, semantic = [], [], [], []
    for batch_idx, d in enumerate(frames):
        i = index + d
        if i < 0 or i >= len(seq.global_indexes) or _scene_of(seq, i) != _scene_of(seq, index):
            continue
        cloud, lab = frame_cloud(seq, index, d, frames[batch_idx - 1] if batch_idx > 0 else None, interval, key_points,
                                 key_labels, paint_dist)
        for view_idx, v in enumerate(used_view):
            rec = cam_frames[(i, v)]
            chain = camera_chain(lidar_cs[0], lidar_cs[1], seq.e2g_q[i], seq.e2g_t[i], rec["pose_q"], rec["pose_t"],
                                 view_cs[v][0], view_cs[v][1], view_cs[v][2])
            pts, pl = fov_points(cloud, lab, torch.from_numpy(chain).to(dev), (w_full, h_full), crop_top, height,
                                 batch_idx * len(used_view) + view_idx)
            # into the current lidar frame - the current keyframe too: its (R, T) is a rounded identity (:305)
            rot, trans = relative_transform(seq, index, i)
            params = np.zeros((1, 28), dtype=np.float64)
            params[0, 13:22], params[0, 22:25], params[0, 25] = rot.reshape(-1), trans, 1.0
            five = torch.cat([pts[:, :4], torch.zeros((pts.shape[0], 1), dtype=torch.float32, device=dev)], 1).contiguous()
            moved, _ = B.fuse_sweeps(five, torch.zeros(pts.shape[0], dtype=torch.int32, device=dev), torch.from_numpy(params).to(dev))
            fov.append(torch.cat([moved[:, :4], pts[:, 4:]], 1))
            fov_lab.append(pl)
            images.append(half_image(rec["image"], crop_top))
            semantic.append(rec["semantic"].float()[crop_top:].contiguous())
    fov, fov_lab = torch.cat(fov, 0), torch.cat(fov_lab, 0)
    fov_all, fov_lab_all = fov, fov_lab                                  # the reference's xyzret_fov_ms / labels_fov_ms
    rec = None if aug is None else torch.from_numpy(_one_aug(aug)).to(dev, non_blocking=True)
    sample, point = _lidar_side(fsa, steps, in_feature_dim, voxel_size, name, rec)
    if rec is not None:
        fov = augment_points(fov, rec)
    _pair_fov_labels(sample, voxelize_fov(sample, point, fov, voxel_size, fov_lab))     # clamp_fov_mask (:133-135), lidar_fov_ms
    sample["image_ms"] = torch.stack(images, 0)
    sample["semantic_map_ms"] = torch.stack(semantic, 0)
    n_img = len(images)
    if zero_maps:
        sample["depth_map_ms"] = torch.zeros((n_img, h_full - crop_top, w_full, 1), dtype=torch.float32, device=dev)   # (:346-347)
        sample["lidar_map_ms"] = torch.zeros((n_img, h_full - crop_top, w_full, 4), dtype=torch.float32, device=dev)
    sample["_image_keyframes"], sample["_fov_points"], sample["_fov_labels"] = frames, fov_all, fov_lab_all   # (diagnostics)
    return sample


def _pair_fov_labels(sample: Dict, fov_lab: torch.Tensor) -> None:
    """targets_fov_ms: the reference pairs the FOV labels with the FUSED cloud's coordinates (:197) - kept as it is"""
    sample["targets_fov_ms"] = SparseTensor(fov_lab, sample["lidar_ms"].C)


def build_nusc_tiaf_batch(samples: List[Dict]) -> Dict:
    """collate_batch of nuscenes_voxel_ms_mm.py:225-262 on device tensors (samples built with zero_maps=False: without the two
    all-zero maps): tiaf.build_tiaf_batch."""
    return build_tiaf_batch(samples)


_SAMPLE_DEFAULTS = {"in_feature_dim": 4, "crop_top": 2, "name": ""}


def _valid_keyframes(seq: NuscSequence, index: int, frames: Sequence[int]):
    """(position in the image stack, offset, previous offset) of the image keyframes that exist in the scene (:239-245)"""
    out = []
    for batch_idx, d in enumerate(frames):
        i = index + d
        if i < 0 or i >= len(seq.global_indexes) or _scene_of(seq, i) != _scene_of(seq, index):
            continue
        out.append((batch_idx, d, frames[batch_idx - 1] if batch_idx > 0 else None))
    return out


def _camera_records(inputs: List[Dict], frames_of: List[List[int]], entry_input: Sequence[int], dev):
    """The camera side's inputs of a batch whose entry b is inputs[entry_input[b]] (a sample, or one view of THE sample):
    (points5 [n, 5] raw rows of every image keyframe's cloud, labels [n], sweep index [n] int32, the [S, 28] table that moves every
    cloud into its image keyframe's lidar frame - all on the device, for ONE ts_fuse_sweeps -, the CAM_FRAME_DTYPE table on the host,
    the virtual rows per record, and per input its (image, semantic map) in stack order)."""
    rows, labels, lengths, params, start_of, images_of = [], [], [], [], {}, []
    for k, inp in enumerate(inputs):
        seq, index = inp["seq"], inp["index"]
        stamp0 = int(seq.timestamps[int(seq.global_indexes[index])])
        pictures = []
        for batch_idx, d, prev in _valid_keyframes(seq, index, frames_of[k]):
            i = index + d
            src, n = sum(lengths), 0
            for f in _cloud_keyframes(seq, index, d, prev, inp["interval"]):
                row = np.zeros(28, dtype=np.float64)
                if f != i:
                    rot, trans = relative_transform(seq, i, f)
                    row[13:22], row[22:25], row[25] = rot.reshape(-1), trans, 1.0
                row[26] = stamp0 / 1e6 - seq.timestamps[int(seq.global_indexes[f])] / 1e6
                params.append(row)
                rows.append(inp["key_points"][f])
                labels.append(inp["key_labels"][f].long())
                lengths.append(int(inp["key_points"][f].shape[0]))
                n += lengths[-1]
            start_of[(k, d)] = (src, n)
            for v in inp["used_view"]:
                frame = inp["cam_frames"][(i, v)]
                pictures.append((frame["image"], frame["semantic"]))
        images_of.append(pictures)
    table, virt, first = [], [], 0
    for b, k in enumerate(entry_input):
        inp = inputs[k]
        seq, index, views = inp["seq"], inp["index"], inp["used_view"]
        w_full, h_full = inp["full_image_size"]
        crop_top = inp.get("crop_top", _SAMPLE_DEFAULTS["crop_top"])
        height = h_full // 2 - crop_top
        for batch_idx, d, _ in _valid_keyframes(seq, index, frames_of[k]):
            i = index + d
            rot, trans = relative_transform(seq, index, i)       # the current keyframe's too: a rounded identity (:305)
            src, n = start_of[(k, d)]
            for view_idx, v in enumerate(views):
                frame, cs = inp["cam_frames"][(i, v)], inp["view_cs"][v]
                rec = np.zeros((), dtype=CAM_FRAME_DTYPE)
                rec["cam"] = camera_chain(inp["lidar_cs"][0], inp["lidar_cs"][1], seq.e2g_q[i], seq.e2g_t[i], frame["pose_q"],
                                          frame["pose_t"], cs[0], cs[1], cs[2])
                rec["move"][:9], rec["move"][9:] = rot.reshape(-1), trans
                rec["row_offset"], rec["paint_dist"] = float(height * (batch_idx * len(views) + view_idx)), float(inp["paint_dist"])
                rec["sample"], rec["img_w"], rec["img_h"], rec["crop_top"] = b, int(w_full), int(h_full), int(crop_top)
                rec["first"], rec["src"] = first, src
                table.append(rec)
                virt.append(n)
                first += n
    idx = rows_index32(lengths, dev)
    return (torch.cat(rows, 0), torch.cat(labels, 0), idx, torch.from_numpy(np.stack(params, 0)).to(dev, non_blocking=True),
            np.stack(table, 0), virt, images_of)


def _build_camera_batch(inputs: List[Dict], frames_of: List[List[int]], votes: Optional[int], aug, zero_maps: bool) -> Dict:
    """build_nusc_tiaf_batch_from_keyframes (votes None) and build_nusc_tiaf_tta_batch (votes: the number of views of the ONE sample
    of `inputs`): entry b of the batch is sample b, or view b of the sample"""
    dev = inputs[0]["fsa"]["points"].device
    nb, rec_dev = _camera_batch_head(len(inputs), votes, aug, dev)
    entry_input = list(range(nb)) if votes is None else [0] * nb
    # the image planes and the zero maps of a batch are ONE tensor each: what shapes them has to agree between the samples
    shaping = {(tuple(inp["full_image_size"]), inp.get("crop_top", _SAMPLE_DEFAULTS["crop_top"])) for inp in inputs}
    if len(shaping) != 1:
        raise ValueError("the samples of a batch share full_image_size and crop_top (got %s)" % sorted(shaping))
    # LiDAR side, per entry: the FSA fuse, both clouds through the entry's record, the two voxelisations
    samples, los = [], []
    for b, k in enumerate(entry_input):
        inp = inputs[k]
        sample, point = _lidar_side(inp["fsa"], inp["steps"], inp.get("in_feature_dim", _SAMPLE_DEFAULTS["in_feature_dim"]),
                                    inp["voxel_size"], inp.get("name", _SAMPLE_DEFAULTS["name"]),
                                    None if rec_dev is None else rec_dev[b:b + 1])
        samples.append(sample)
        los.append(clamp_corner(point))
    # camera side: every image keyframe's cloud once, into ITS lidar frame in one launch; a record per (entry, keyframe, view)
    points5, labels, sweep, params, table, virt, images_of = _camera_records(inputs, frames_of, entry_input, dev)
    moved, no_ego = B.fuse_sweeps(points5.contiguous(), sweep, params)
    records = torch.from_numpy(table.view(np.uint8).reshape(len(table), CAM_FRAME_DTYPE.itemsize)).to(dev, non_blocking=True)
    fov, fov_lab, _, _, counts = B.nusc_fov_cloud(moved[:, :4].contiguous(), labels, rows_index32(virt, dev), records, nb,
                                                  pre_keep=no_ego, aug=rec_dev, lo=torch.stack(los, 0))
    # images: the cut top rows are a pointer offset into the resident half-resolution frames
    images, semantic, per_entry = [], [], []
    for k, inp in enumerate(inputs):
        crop_top = inp.get("crop_top", _SAMPLE_DEFAULTS["crop_top"])
        per_entry.append(len(images_of[k]))
        for image, sem in images_of[k]:
            images.append(image[crop_top:])
            semantic.append((sem if sem.dtype == torch.float32 else sem.float())[crop_top:])
    planes = {tuple(im.shape[:2]) for im in images}
    if len(planes) != 1:
        raise ValueError("the half-resolution camera images of a batch share one size (got %s)" % sorted(planes))
    image_ms, semantic_ms = B.tiaf_image_stack(images, semantic, None, _unit_table(dev), planes.pop())
    out = _camera_batch_tail(samples, [inputs[k]["voxel_size"] for k in entry_input], fov, fov_lab, counts, per_entry, votes, image_ms,
                             semantic_ms, labelled=_pair_fov_labels)
    image_ms = out["image_ms"]
    if zero_maps:                                                       # (:346-347: all zeros at FULL resolution)
        inp = inputs[0]
        w_full, h_full = inp["full_image_size"]
        rows = h_full - inp.get("crop_top", _SAMPLE_DEFAULTS["crop_top"])
        out["depth_map_ms"] = torch.zeros((image_ms.shape[0], 1, rows, w_full), dtype=torch.float32, device=dev)
        out["lidar_map_ms"] = torch.zeros((image_ms.shape[0], 4, rows, w_full), dtype=torch.float32, device=dev)
    return out


def _records_of(inputs: List[Dict], frames_of: List[List[int]], entries: int) -> int:
    return sum(len(_valid_keyframes(inp["seq"], inp["index"], fr)) * len(inp["used_view"]) for inp, fr in zip(inputs, frames_of)) * entries


def _per_sample_batch(inputs: List[Dict], frames_of: List[List[int]], aug, zero_maps: bool) -> Dict:
    """The cross-check path as the fallback of both builders: entry b from inputs[b] with the b-th record of `aug`"""
    rec = None if aug is None else _aug_records(aug, len(inputs))
    return build_nusc_tiaf_batch([build_nusc_tiaf_sample(**{**inp, "image_keyframes": fr, "zero_maps": zero_maps},
                                                         aug=None if rec is None else rec[b:b + 1])
                                  for b, (inp, fr) in enumerate(zip(inputs, frames_of))])


def _select(inp: Dict) -> List[int]:
    if inp.get("image_keyframes") is not None:
        return list(inp["image_keyframes"])
    return select_image_keyframes(inp["seq"], inp["index"], inp["multiscan_image"], inp["step_image"], inp["rng"])


def build_nusc_tiaf_batch_from_keyframes(inputs: List[Dict], aug=None, zero_maps: bool = False) -> Dict:
    """build_nusc_tiaf_batch([build_nusc_tiaf_sample(**inputs[b], aug=aug[b]) ...]) with the camera side of the WHOLE batch on
    csrc/nusc_tiaf_stage.hip: the same dictionary, bit for bit.  inputs[b]: the arguments of build_nusc_tiaf_sample for sample b, by
    name - the datasets' settings may differ between samples (views, interval, PAINT_DIST, image keyframes), except
    full_image_size, crop_top and the size of the half-resolution images, which shape the batch's one image tensor (checked);
    aug: one AugParams per sample or None.
    The LiDAR side stays per sample (the FSA fuse, voxelize_sample_ms on the augmented clouds).  The camera side: ONE
    ts_fuse_sweeps over the rows of every image keyframe of the batch (each cloud into its keyframe's lidar frame, the ego-box
    byte), the record table of every (sample, keyframe, view) in one upload - WHOLE 584-byte records, where tiaf._frame_records
    uploads the host's few fields and gathers resident matrices on the device: here the camera chain and the move are products
    of quaternions the host makes per call, so there is nothing resident to gather -, ts_nusc_fov_cloud (three launches: ego box,
    PAINT_DIST, camera chain and frustum, the move into the current frame, augmentation and the clamp to the sample's augmented
    single-frame minimum per virtual row, one stable compaction), ONE host read of the per-sample counts, then the FOV voxelisation
    per sample with the sample's shift; the images in one ts_tiaf_image_stack launch per 16 frames, the two cut rows a pointer
    offset.  `depth_map_ms` / `lidar_map_ms` - all zeros at full resolution in the reference - only under zero_maps.  More than 64
    samples or 1024 camera records: the per-sample path."""
    nb = len(inputs)
    if nb == 0:
        raise ValueError("no samples")
    frames_of = [_select(inp) for inp in inputs]
    if nb > B.TIAF_MAX_SAMPLES or _records_of(inputs, frames_of, 1) > B.TIAF_MAX_FRAMES:
        return _per_sample_batch(inputs, frames_of, aug, zero_maps)
    return _build_camera_batch(inputs, frames_of, None, aug, zero_maps)


def build_nusc_tiaf_tta_batch(inp: Dict, votes_min: int, votes_max: int, rng: np.random.RandomState,
                              scale_range: Sequence[float] = (0.9, 1.1), zero_maps: bool = False) -> Dict:
    """The reference's `__getitem__` under `TTA: True` + `collate_batch_tta` (nuscenes_voxel_ms_mm.py:68-73, 106-125, 272-318): the
    sample `inp` (the arguments of build_nusc_tiaf_sample, by name) `votes_max - votes_min` times as batch entries, entry i rotated
    by TTA_ANGLES[votes_min + i] * pi / 8 and scaled by a draw from `rng` (augment.draw_tta_params: SCALE_AUG_RANGE - the
    `scale_aug_range` assignment of :110 names an attribute nothing reads).  `rng` gives one scale per vote and nothing else:
    NuscenesMsMmDataset.__getitem__ draws no mix coin.  The image keyframes are selected once (the reference caches them per sample
    token, so `random.sample` runs on the first read only); the views' records read the same point rows, and the image stack is
    built once and repeated."""
    votes = list(range(votes_min, votes_max))
    if not votes:
        raise ValueError("no votes: votes_min %d, votes_max %d" % (votes_min, votes_max))
    aug = [draw_tta_params(rng, v, scale_range) for v in votes]
    frames = _select(inp)
    if len(votes) > B.TIAF_MAX_SAMPLES or _records_of([inp], [frames], len(votes)) > B.TIAF_MAX_FRAMES:
        return _per_sample_batch([inp] * len(votes), [frames] * len(votes), aug, zero_maps)
    return _build_camera_batch([inp], [frames], len(votes), aug, zero_maps)
