"""TIAF (temporal image aggregation and fusion) data stage on the device - the camera side of
R/pcseg/data/dataset/semantickitti/semantickitti_ms_mm.py:304-461 and the voxelisation / collate of
semantickitti_voxel_ms_mm.py:79-330, next to the LiDAR multi-scan stage of taseg_amd.data.stage:

  per frame with an image (the current one and every STEP_IMAGE-th history frame up to MULTISCAN_IMAGE):
      projection        points in front of the camera -> pixel (row, col) through P2 @ Tr, frustum test, IMAGE_FLIP of the
                        column, crop test, the row shifted by HEIGHT * (position of the frame in the image stack)   (:419-457)
      pose fuse         the kept points into the current frame (history frames only)                               (:368)
      image             uint8 RGB -> float32 BGR / 255, IMAGE_FLIP, top-left crop, zero padded to HEIGHT x WIDTH     (:432-452)
  sample                ring id column of the single-frame cloud (:131-141), the three clouds (current, fused, FOV) augmented with
                        ONE draw (aug_points_rgb_ms, voxel_ms_mm.py:92-124), voxelised with ONE coordinate shift (the fused
                        cloud's minimum), FOV cloud clamped to the current cloud's corner like the fused one      (:126-204)
  batch                 sparse collate + image stacks concatenated along the frame axis as NCHW + offset_img (:223-269); under
                        `TTA: True` the sample once per vote (collate_batch_tta, :271-330)

Two ways to build a batch, the same tensors bit for bit:
  build_tiaf_sample + build_tiaf_batch   per sample and per frame, from the operators every stage shares (ts_project_fov, a boolean
                        index, ts_fuse_scan, ts_stage_augment; the image as table gather, zeros and a slice copy) - the cross-check
  build_tiaf_batch_from_frames           the camera side of the whole batch on two kernels (csrc/tiaf_stage.hip): ts_tiaf_fov_cloud,
                        all seven per-row steps and ONE stable compaction with one host read, and ts_tiaf_image_stack, the frames
                        straight into the NCHW planes; the LiDAR side stays per sample.  build_tiaf_tta_batch: the TTA views on it.

The random draws stay on the host, on a `np.random.RandomState` consumed as the reference consumes numpy's global generator, ONE
SAMPLE AFTER THE OTHER: first the image flips of the sample's camera frames, oldest frame first (`draw_image_flips`: the dataset's
`__getitem__` runs before the voxel dataset's augmentation), then the mix coin every `__getitem__` draws and, under AUGMENT 'none',
does not use (`mix.draw_coin`, semantickitti_ms_mm.py:178), then `augment.draw_train_params` (uniform, uniform, choice(4, 1), three
normal - `aug_points_rgb_ms` draws exactly as `aug_points_ms`):

    flips, _ = draw_image_flips(rng, frames), draw_coin(rng)                     # {delta: bool}, the unused coin
    aug = draw_train_params(rng)
    batch = build_tiaf_batch_from_frames([frames], steps, multiscan, step_image, [proj], crop, voxel, aug=[aug], flips=[flips])

Reproduced rather than repaired: the TTA scale comes from SCALE_AUG_RANGE (the `scale_aug_range = [0.95, 1.05]` assignment of :109
names an attribute nothing reads); the flip mirrors the full-width image BEFORE the crop, so a wide image shows its right part.
Not here: file decoding (PNG, .npy semantic maps); IMAGE_JITTER (`color_jitter` needs mmcv's photometric distortion; no golden can
be made without it); `depth_map_ms` / `lidar_map_ms` (all zeros in the reference); PolarMix / LaserMix inside the TIAF dataset
(the recipe sets AUGMENT 'none').  The nuScenes recipe's stage: data/nuscenes_tiaf.py.  Bit-exact against the
reference's dataset code: tests/golden/tiaf_data.npz, tests/golden/tiaf_aug.npz.
"""
from functools import lru_cache
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import backend as B
from .augment import augment_points, draw_tta_params
from .mix import draw_coin
from .stage import (_aug_records, _fuse_history, _one_aug, clamp_corner, collate_batch, rows_index32, voxelize_fov,
                    voxelize_fov_cloud, voxelize_sample_ms)

__all__ = ["ring_id", "fov_points", "crop_image", "draw_image_flips", "build_tiaf_sample", "build_tiaf_batch",
           "build_tiaf_batch_from_frames", "build_tiaf_tta_batch", "FRAME_DTYPE"]

# TsTiafFrame of include/taseg_hip.h: the per-frame record of ts_tiaf_fov_cloud
FRAME_DTYPE = np.dtype([("proj", "<f8", 12), ("pose0", "<f4", 16), ("pose", "<f4", 16), ("row_offset", "<f4"), ("fov_dist", "<f4"),
                        ("sample", "<i4"), ("img_w", "<i4"), ("img_h", "<i4"), ("flags", "<i4"), ("first", "<i4"), ("src", "<i4")])
_HOST_FIELDS = np.dtype([(n, FRAME_DTYPE.fields[n][0]) for n in FRAME_DTYPE.names[3:]])       # what the host knows: 32 bytes
FLIP, FUSE = 1, 2                                      # TS_TIAF_FLIP, TS_TIAF_FUSE


def draw_image_flips(rng: np.random.RandomState, camera_deltas, image_flip: bool = True, flip_ratio: float = 0.5) -> Dict[int, bool]:
    """The IMAGE_FLIP decisions of one sample (semantickitti_ms_mm.py:436): `rng.rand() < flip_ratio` once per camera frame, in
    the order `multiscan_fuse` walks the frames (:328-373) - delta ascending: oldest frame first, the current frame last.
    camera_deltas: the frame offsets (<= 0) of the camera frames that EXIST, or the frames dictionary of build_tiaf_sample (its
    entries with an image) - a frame the reference cannot read (`try / except: continue` at the head of a sequence) is not in
    it and draws nothing.  image_flip off: no draw at all (the reference's `and` short-circuits).  Within a sample these draws
    come first, then mix.draw_coin (:178), then augment.draw_train_params."""
    if isinstance(camera_deltas, Mapping):
        camera_deltas = [d for d, f in camera_deltas.items() if "image" in f]
    out = {}
    for d in sorted(int(d) for d in camera_deltas):
        out[d] = bool(image_flip and rng.rand() < flip_ratio)
    return out


def ring_id(points: torch.Tensor) -> torch.Tensor:
    """get_kitti_points_ringID (semantickitti_ms_mm.py:131-141) on the device: float32 [n]."""
    yaw = -torch.atan2(points[:, 1], -points[:, 0])
    proj_x = 0.5 * (yaw / torch.pi + 1.0)
    wrap = torch.zeros_like(proj_x)
    wrap[1:] = ((proj_x[1:] < 0.2) & (proj_x[:-1] > 0.8)).to(proj_x.dtype)
    return torch.clamp(torch.cumsum(wrap, 0), 0, 63)


def fov_points(points: torch.Tensor, proj: torch.Tensor, image_size, crop, img_batch: int) -> torch.Tensor:
    """[m, 6] = (x, y, z, intensity, row + HEIGHT * img_batch, col) of the points that project into the cropped image."""
    pts = points[:, :4].contiguous()
    pix, keep = B.project_fov(pts, proj, image_size, crop, float(crop[0] * img_batch))
    return torch.cat([pts[keep], pix[keep]], 1)


@lru_cache(maxsize=None)
def _unit_table(device) -> torch.Tensor:
    """float32 [256] on `device`: the 256 quotients i / 255 as numpy rounds them (correctly), kept per device"""
    return torch.from_numpy(np.arange(256, dtype=np.float32) / 255.).to(device)


def bgr_unit(image_u8: torch.Tensor) -> torch.Tensor:
    """[h, w, 3] uint8 RGB -> float32 BGR / 255 (numpy's `image[:, :, ::-1] / 255.`).  The 256 possible quotients come from a table
    of correctly rounded float32 divisions: the device's division by a scalar is a multiplication by the reciprocal and differs
    in the last bit."""
    if image_u8.dtype != torch.uint8:
        raise TypeError("camera images must be uint8")
    return _unit_table(image_u8.device)[image_u8.flip(2).long()]


def _pad(t: torch.Tensor, crop) -> torch.Tensor:
    out = torch.zeros((crop[0], crop[1], t.shape[2]), dtype=torch.float32, device=t.device)
    r, c = min(crop[0], t.shape[0]), min(crop[1], t.shape[1])
    out[:r, :c] = t[:r, :c]
    return out


def crop_image(image_u8: torch.Tensor, crop) -> torch.Tensor:
    """[h, w, 3] uint8 RGB -> float32 [HEIGHT, WIDTH, 3] BGR / 255 (bgr_unit), zero padded (semantickitti_ms_mm.py:432-447)"""
    return _pad(bgr_unit(image_u8), crop)


def _lidar_inputs(frames, steps, multiscan):
    """(single-frame cloud with the ring id as 5th column (:266-267), its labels, the un-filtered stack [current | history] with
    the time flag (:159), its labels, the keep mask) of one sample's frames"""
    cur = frames[0]
    hist = [d for d in sorted(frames) if -multiscan <= d < 0]
    raw_all, lab_all, keep = _fuse_history(cur["points"], cur["labels"], [frames[d]["points"] for d in hist],
                                           [frames[d]["labels"] for d in hist], cur["pose"], [frames[d]["pose"] for d in hist], hist,
                                           steps, [frames[d]["pseudo"] for d in hist])
    point = torch.cat([cur["points"][:, :4], ring_id(cur["points"]).unsqueeze(1)], 1).contiguous()
    return point, cur["labels"].long(), raw_all, lab_all, keep


def _camera_deltas(frames) -> List[int]:
    """the camera frames of a sample, newest first (the reference inserts at the front while walking delta upwards, :369-373)"""
    return sorted((d for d in frames if "image" in frames[d]), reverse=True)


def build_tiaf_sample(frames: Dict[int, Dict], steps: Sequence[int], multiscan: int, step_image: int, proj: torch.Tensor,
                      crop, voxel_size: float, name: str = "", fov_dist: float = -1.0, aug=None,
                      flips: Optional[Mapping[int, bool]] = None) -> Dict:
    """frames[delta] (delta = 0 current, < 0 history) = dict(points [n,4], labels [n] classes, pseudo [n] canonical classes
    or -1, pose [4,4] float32, and - for the frames with |delta| % step_image == 0 - image [h,w,3] uint8 RGB,
    semantic [h,w,1]).  Returns the reference's sample dictionary (semantickitti_voxel_ms_mm.py:205-227).
    aug: the sample's AugParams - the two LiDAR clouds through voxelize_sample_ms(aug=), the [m, 6] FOV cloud through
    augment_points before its clamp, which then sees the augmented single-frame cloud (:92-133).  flips: {delta: bool}
    (draw_image_flips) - a flipped frame's pixel column is mirrored BEFORE the crop test (:441, :454), its image and semantic map
    before the crop (:437-440).  aug=None, flips=None is the path without either, launch for launch."""
    point, labels, raw_all, lab_all, keep = _lidar_inputs(frames, steps, multiscan)
    pose0 = frames[0]["pose"]
    sample = voxelize_sample_ms(point, labels, raw_all, lab_all, voxel_size, name, keep=keep, return_shift=True, aug=aug)
    fov, images, semantic = [], [], []
    for d in _camera_deltas(frames):
        f = frames[d]
        h, w = f["image"].shape[0], f["image"].shape[1]
        image, sem = f["image"], f["semantic"].float()
        if flips is not None and flips.get(d, False):
            # the crop test on the mirrored column: ts_project_fov with the image's own width as crop passes every column
            pts = f["points"][:, :4].contiguous()
            pix, ok = B.project_fov(pts, proj, (w, h), (crop[0], w), float(crop[0] * (abs(d) // step_image)))
            col = (w - 1) - pix[:, 1]
            ok = ok & (col < crop[1])
            pts = torch.cat([pts[ok], pix[ok, :1], col[ok].unsqueeze(1)], 1)
            image, sem = image.flip(1), sem.flip(1)
        else:
            pts = fov_points(f["points"], proj, (w, h), crop, abs(d) // step_image)
        if fov_dist > 0:
            radius = torch.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1])
            pts = pts[radius <= fov_dist]
        if d != 0:
            moved = B.fuse_scan(pts[:, :4].contiguous(), pose0, f["pose"])
            pts = torch.cat([moved, pts[:, 4:]], 1)
        fov.append(pts)
        images.append(crop_image(image, crop))
        semantic.append(_pad(sem, crop))
    fov = torch.cat(fov, 0)
    if aug is not None:
        rec = torch.from_numpy(_one_aug(aug)).to(point.device, non_blocking=True)
        fov, point = augment_points(fov, rec), augment_points(point, rec)
    voxelize_fov(sample, point, fov, voxel_size)           # lidar_fov_ms
    sample["image_ms"] = torch.stack(images, 0)
    sample["semantic_map_ms"] = torch.stack(semantic, 0)
    return sample


def build_tiaf_batch(samples: List[Dict]) -> Dict:
    """collate_batch of semantickitti_voxel_ms_mm.py:223-266 / nuscenes_voxel_ms_mm.py:225-262 on device tensors: the sparse
    collate, the image stacks the samples carry (any of image_ms, depth_map_ms, lidar_map_ms, semantic_map_ms) concatenated along
    the frame axis as NCHW, offset_img; the samples' diagnostic keys ("_...") are left out."""
    stacks = {k: [s.pop(k) for s in samples] for k in ("image_ms", "depth_map_ms", "lidar_map_ms", "semantic_map_ms")
              if k in samples[0]}
    for s in samples:
        for k in ("_image_keyframes", "_fov_points", "_fov_labels"):
            s.pop(k, None)
    out = collate_batch(samples)
    dev = stacks["image_ms"][0].device
    out["offset_img"] = torch.cumsum(torch.tensor([i.shape[0] for i in stacks["image_ms"]]), 0).int().to(dev)
    for k, v in stacks.items():
        out[k] = torch.cat(v, 0).permute(0, 3, 1, 2).contiguous()
    return out


def _frame_records(entries, dev) -> torch.Tensor:
    """uint8 [F, 256] on the device: the TsTiafFrame table of ts_tiaf_fov_cloud.  entries: per frame (proj float64 [3, 4], pose0,
    pose float32 [4, 4] - device tensors, kept resident -, and the host's fields as a FRAME_DTYPE-named dict).  What the host knows
    (32 bytes per frame) is uploaded in one copy; the matrices are gathered beside it on the device (three stacks, one cat)."""
    host = np.zeros(len(entries), dtype=_HOST_FIELDS)
    for i, (_, _, _, fields) in enumerate(entries):
        for k, v in fields.items():
            host[i][k] = v
    tail = torch.from_numpy(host.view(np.uint8).reshape(len(entries), _HOST_FIELDS.itemsize)).to(dev, non_blocking=True)
    proj = torch.stack([e[0].to(dev) for e in entries], 0).reshape(len(entries), 12)
    pose0 = torch.stack([e[1].to(dev) for e in entries], 0).reshape(len(entries), 16)
    pose = torch.stack([e[2].to(dev) for e in entries], 0).reshape(len(entries), 16)
    if proj.dtype != torch.float64 or pose0.dtype != torch.float32 or pose.dtype != torch.float32:
        raise TypeError("proj must be float64 [3, 4], poses float32 [4, 4]")
    return torch.cat([proj.view(torch.uint8), pose0.view(torch.uint8), pose.view(torch.uint8), tail], 1)


def _camera_batch_head(n_inputs: int, votes: Optional[int], aug, dev):
    """(nb, the [nb, 8] augmentation records on the device or None): entry b of the batch is input b, or view b of the ONE input"""
    nb = n_inputs if votes is None else votes
    return nb, None if aug is None else torch.from_numpy(_aug_records(aug, nb)).to(dev, non_blocking=True)


def _camera_batch_tail(samples, voxel_sizes, fov, fov_lab, counts, per_input, votes, image_ms, semantic_ms, labelled=None) -> Dict:
    """The end of both datasets' batched camera side.  samples: voxelize_sample_ms's per entry; fov (fov_lab, or None): the compacted
    FOV cloud of the batch, counts [nb]: its rows per entry, on the device; labelled(sample, the labels of its FOV voxels): what a
    dataset with FOV labels adds; per_input: the images per input; image_ms / semantic_ms: their planes, repeated under `votes`."""
    at = 0
    for s, voxel_size, n in zip(samples, voxel_sizes, counts.tolist()):     # the one host read of the camera side
        lab = voxelize_fov_cloud(s, fov[at:at + n], voxel_size, None if fov_lab is None else fov_lab[at:at + n])
        if labelled is not None:
            labelled(s, lab)
        at += n
    out = collate_batch(samples)
    if votes is not None:                                               # the same images for every view: built once, repeated
        per_input = per_input * votes
        image_ms, semantic_ms = image_ms.repeat(votes, 1, 1, 1), semantic_ms.repeat(votes, 1, 1, 1)
    out["offset_img"] = torch.cumsum(torch.tensor(per_input), 0).int().to(image_ms.device)
    out["image_ms"], out["semantic_map_ms"] = image_ms, semantic_ms
    return out


def _build_camera_batch(frames_list, votes, steps, multiscan, step_image, projs, crop, voxel_size, names, fov_dist, aug, flips) -> Dict:
    """build_tiaf_batch_from_frames (votes None) and build_tiaf_tta_batch (votes: the number of views of the ONE sample of
    frames_list): entry b of the batch is sample b, or view b of the sample"""
    dev = frames_list[0][0]["points"].device
    nb, rec_dev = _camera_batch_head(len(frames_list), votes, aug, dev)
    # LiDAR side, per sample: the current scan and the fused history through the sample's record, the two voxelisations
    samples, los, lidar = [], [], {}
    for b in range(nb):
        frames = frames_list[0 if votes is not None else b]
        if id(frames) not in lidar:
            lidar[id(frames)] = _lidar_inputs(frames, steps, multiscan)
        point, labels, raw_all, lab_all, keep = lidar[id(frames)]
        if rec_dev is not None:
            point, raw_all = augment_points(point, rec_dev[b:b + 1]), augment_points(raw_all, rec_dev[b:b + 1])
        samples.append(voxelize_sample_ms(point, labels, raw_all, lab_all, voxel_size, names[b], keep=keep, return_shift=True))
        los.append(clamp_corner(point))
    # camera side: the rows of every camera frame of every sample once, a record per (batch entry, frame)
    rows, lengths, images, semantic, img_flips, per_sample, starts = [], [], [], [], [], [], {}
    for frames in frames_list:
        cams = _camera_deltas(frames)
        per_sample.append(len(cams))
        for d in cams:
            starts[(id(frames), d)] = sum(lengths)
            rows.append(frames[d]["points"][:, :4])
            lengths.append(int(frames[d]["points"].shape[0]))
    entries, virt, first = [], [], 0
    for b in range(nb):
        k = 0 if votes is not None else b
        frames = frames_list[k]
        for d in _camera_deltas(frames):
            f = frames[d]
            flip = bool(flips is not None and flips[b] is not None and flips[b].get(d, False))
            n = int(f["points"].shape[0])
            entries.append((projs[k], frames[0]["pose"], f["pose"], {
                "row_offset": float(crop[0] * (abs(d) // step_image)), "fov_dist": float(fov_dist), "sample": b,
                "img_w": int(f["image"].shape[1]), "img_h": int(f["image"].shape[0]), "flags": FLIP * flip + FUSE * (d != 0),
                "first": first, "src": starts[(id(frames), d)]}))
            virt.append(n)
            first += n
            if votes is None or b == 0:
                images.append(f["image"])
                semantic.append(f["semantic"] if f["semantic"].dtype == torch.float32 else f["semantic"].float())
                img_flips.append(flip)
    fov, _, _, counts = B.tiaf_fov_cloud(torch.cat(rows, 0), rows_index32(virt, dev), _frame_records(entries, dev), nb, crop,
                                         aug=rec_dev, lo=torch.stack(los, 0))
    image_ms, semantic_ms = B.tiaf_image_stack(images, semantic, img_flips, _unit_table(dev), crop)
    return _camera_batch_tail(samples, [voxel_size] * nb, fov, None, counts, per_sample, votes, image_ms, semantic_ms)


def _per_sample_batch(frames_list, steps, multiscan, step_image, projs, crop, voxel_size, names, fov_dist, aug, flips) -> Dict:
    """The cross-check path as the fallback of both builders: entry b from frames_list[b] with the b-th record of `aug`"""
    rec = None if aug is None else _aug_records(aug, len(frames_list))
    return build_tiaf_batch([build_tiaf_sample(f, steps, multiscan, step_image, projs[b], crop, voxel_size, names[b], fov_dist,
                                               aug=None if rec is None else rec[b:b + 1], flips=None if flips is None else flips[b])
                             for b, f in enumerate(frames_list)])


def build_tiaf_batch_from_frames(frames_list: List[Dict[int, Dict]], steps: Sequence[int], multiscan: int, step_image: int, projs,
                                 crop, voxel_size: float, names: Optional[List[str]] = None, fov_dist: float = -1.0, aug=None,
                                 flips: Optional[List[Optional[Mapping[int, bool]]]] = None) -> Dict:
    """build_tiaf_batch([build_tiaf_sample(frames_list[b], ..., projs[b], aug=aug[b], flips=flips[b]) ...]) with the camera side of
    the WHOLE batch on csrc/tiaf_stage.hip: the same dictionary, bit for bit.  projs: one float64 [3, 4] device tensor per sample
    (sequences differ) or one for all; aug: one AugParams per sample or None; flips: one {delta: bool} (or None) per sample or None.
    The LiDAR side stays per sample (_fuse_history, ring_id, voxelize_sample_ms on the augmented clouds).  The camera side:
    the rows of all camera frames in one cat, the frame table in one small upload beside three stacks and a cat of the resident
    matrices, ts_tiaf_fov_cloud (three launches: projection, flip, crop, FOV_DIST, pose fuse, augmentation and the clamp to the
    sample's augmented single-frame minimum per row, one stable compaction), ONE host read of the per-sample counts, then the FOV
    voxelisation per sample with the sample's shift; the images in one ts_tiaf_image_stack launch per 16 frames, written into the
    final [N, 3, H, W] / [N, 1, H, W] tensors.  More than 64 samples or 1024 camera frames: the per-sample path."""
    nb = len(frames_list)
    names = [""] * nb if names is None else list(names)
    projs = [projs] * nb if isinstance(projs, torch.Tensor) else list(projs)
    if len(names) != nb or len(projs) != nb or (flips is not None and len(flips) != nb):
        raise ValueError("names, projs and flips hold one entry per sample")
    n_frames = sum(len(_camera_deltas(f)) for f in frames_list)
    if nb == 0 or nb > B.TIAF_MAX_SAMPLES or n_frames > B.TIAF_MAX_FRAMES:
        return _per_sample_batch(frames_list, steps, multiscan, step_image, projs, crop, voxel_size, names, fov_dist, aug, flips)
    return _build_camera_batch(frames_list, None, steps, multiscan, step_image, projs, crop, voxel_size, names, fov_dist, aug, flips)


def build_tiaf_tta_batch(frames: Dict[int, Dict], votes_min: int, votes_max: int, rng, steps: Sequence[int], multiscan: int,
                         step_image: int, proj: torch.Tensor, crop, voxel_size: float, name: str = "", fov_dist: float = -1.0,
                         scale_range: Sequence[float] = (0.9, 1.1)) -> Dict:
    """The reference's `__getitem__` under `TTA: True` + `collate_batch_tta` (semantickitti_voxel_ms_mm.py:68-77, 106-124, 271-330):
    the sample `votes_max - votes_min` times as batch entries, entry i rotated by TTA_ANGLES[votes_min + i] * pi / 8 and scaled by a
    draw from `rng` (augment.draw_tta_params: SCALE_AUG_RANGE - the `scale_aug_range` assignment of :109 names an attribute nothing
    reads).  The reference reads the sample again for every vote, and every read draws the mix coin (semantickitti_ms_mm.py:178):
    `rng` gives a coin (not used), then the scale, per vote.  The projection's input rows and the images are the same for every view: the views' frame records read the same point
    rows, and the image stack is built once and repeated.  (No image flip here: evaluation runs without IMAGE_FLIP.)"""
    votes = list(range(votes_min, votes_max))
    aug = [(draw_coin(rng), draw_tta_params(rng, v, scale_range))[1] for v in votes]
    if not votes or len(votes) > B.TIAF_MAX_SAMPLES or len(votes) * len(_camera_deltas(frames)) > B.TIAF_MAX_FRAMES:
        return _per_sample_batch([frames] * len(votes), steps, multiscan, step_image, [proj] * len(votes), crop, voxel_size,
                                 [name] * len(votes), fov_dist, aug, None)
    return _build_camera_batch([frames], len(votes), steps, multiscan, step_image, [proj], crop, voxel_size, [name] * len(votes),
                               fov_dist, aug, None)
