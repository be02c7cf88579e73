"""Device-resident data stage: TASeg's multi-scan temporal aggregation (FSA) + dataset voxelisation.

The reference does this in numpy inside DataLoader workers
(R/pcseg/data/dataset/semantickitti/semantickitti_ms.py:140-149,253-320,403-417 and
semantickitti_voxel_ms.py:77-212); here the same steps run on the GPU on resident scans:

  pose fuse            ts_fuse_scan        p' = ((p R_t^T + t_t) - t_0) R_0, float32, reference summation order
  class-step filter    lookup table        one _kitti_row per history scan, looked up with the point's (pseudo) class
  concat + time flag   torch.cat           current scan first (flag 1), kept history points after it (flag 0)
  moving objects       ts_stage_moving_*   (moving=) the SMSA recipe's static2moving / moving2static on the current scan and the
                                           un-filtered fused history (data/moving.py), before everything below
  scan mixing (mix=)   ts_stage_mix        PolarMix / LaserMix with a partner scan (data/mix.py), on the single-frame pair and on the
                                           fused pair, before the augmentation (semantickitti_ms.py:151-237); _mix_and_voxelize, the
                                           tail both datasets share
  clamp after a mix    ts_stage_clamp_compact   every fused row against its sample's mixed single-frame minimum, one stable compaction
                                           (without mix=: ts_stage_keep_flags, the history rows only; per sample: the ATen clamp)
  augmentation (aug=)  ts_stage_augment    rotate / scale / flip / translate of the current scan and every fused history row with the
                                           sample's AugParams (data/augment.py), before the clamp and both voxelisations
  three clouds         ts_stage_layout_pair   the mask-distillation recipe's student and teacher clouds from one pass over the
                                           history, voxelised with one shift (data/kd.py build_kd_batch)
  voxel coordinates    ts_voxel_coords     int32(round_half_even(xyz / voxel)) - min
  voxel grouping       ts_sparse_quantize  radix sort + first-occurrence representative + inverse map

Outputs have the reference's exact layout and ORDER (batch_dict schema of SURVEY.md appendix C), checked bit
for bit against the reference dataset code in tests (tests/golden/multiscan.npz).
"""
from itertools import accumulate
from typing import Dict, List, Sequence

import numpy as np
import torch

from .. import backend as B
from .augment import augment_points, draw_tta_params, pack_params
from . import mix as M
from . import moving as MV
from ..torchsparse import SparseTensor
from ..options import options

__all__ = ["fuse_multiscan", "voxelize_sample_ms", "voxelize_sample", "collate_batch", "build_multiscan_batch",
           "build_multiscan_batch_per_sample", "build_tta_batch", "moving_tables", "voxelize_batch_ms", "rows_index", "DevicePrefetcher"]

_BATCHED = options.stage_batched
_cache = {}


def _cached(key, make):
    """make() once per key: the device tensors that depend only on a batch's layout (scan lengths, schedule), for every dataset's
    stage.  The last 64 are kept, the oldest dropped - resident synthetic scans repeat their layout every step, so theirs cost
    no upload after the first."""
    hit = _cache.get(key)
    if hit is None:
        hit = make()                   # (may itself go through _cached: the size is checked after it)
        if len(_cache) >= 64:
            _cache.pop(next(iter(_cache)))
        _cache[key] = hit
    return hit


def rows_index(lengths: Sequence[int], device) -> torch.Tensor:
    """int64 [sum(lengths)]: the index of the segment every concatenated row belongs to (built on the device from the lengths,
    cached per layout)"""
    def make():
        lens = torch.tensor(list(lengths), dtype=torch.int64).to(device, non_blocking=True)
        return torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int64, device=device), lens,
                                       output_size=int(sum(lengths)))
    return _cached((tuple(lengths), str(device)), make)


def rows_index32(lengths: Sequence[int], device) -> torch.Tensor:
    """rows_index as int32 (what ts_voxel_coords takes), cached beside it"""
    return _cached(("i32", tuple(lengths), str(device)), lambda: rows_index(lengths, device).int())


def _kitti_row(delta: int, steps: Sequence[int]) -> List[bool]:
    """The SemanticKITTI class-step rule (semantickitti_ms.py:303-308) for one history scan: class c is aggregated from the scan
    `delta` frames away iff steps[c] != 0 and |delta| % steps[c] == 0.  Last column: pseudo class -1 = a label that is no class's
    canonical raw id (e.g. a moving-object id): never kept."""
    return [bool(st) and abs(delta) % st == 0 for st in steps] + [False]


def _step_table(tag: str, rows, owner, device):
    """(table bool [S, C], owner int64 [S]) on the device, cached: rows[s] = the class-step row of history scan / sweep s (either
    dataset's rule; `tag` keeps their keys apart), owner[s] = the sample it belongs to"""
    return _cached((tag, tuple(map(tuple, rows)), tuple(owner), str(device)),
                   lambda: (torch.tensor(rows, dtype=torch.bool).to(device), torch.tensor(owner, dtype=torch.int64).to(device)))


def _step_keep(table, scan_idx, cls, neg_last=False):
    """bool [n]: table[scan_idx[i], cls[i]], the class-step decision of every history row.  table [S, C] bool (one _kitti_row or
    _nusc_row per scan / sweep), scan_idx [n] int32 or int64, cls [n] int64.  neg_last: a negative class reads the table's last
    column (_kitti_row's); without it every class is a column."""
    n_cols = table.shape[1]
    if neg_last:
        cls = torch.where(cls < 0, torch.full_like(cls, n_cols - 1), cls)
    return table.view(-1)[scan_idx.long() * n_cols + cls]


def _deltas(s) -> List[int]:
    """the frame offsets of a scan dict's history scans: its `deltas`, else -T .. -1"""
    t = len(s["points"]) - 1
    return s.get("deltas") or [i - t for i in range(t)]


def _history_index(lengths: Sequence[int], deltas: Sequence[int], steps: Sequence[int], device):
    """Per-layout helpers of one sample, cached: scan index (int32) of every concatenated history point, and the [T, C + 1] table of
    _kitti_row per history scan."""
    def make():
        scan_idx = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int32),
                                           torch.tensor(list(lengths), dtype=torch.int64)).to(device)
        return scan_idx, torch.tensor([_kitti_row(d, steps) for d in deltas], dtype=torch.bool).to(device)
    return _cached(("history", tuple(lengths), tuple(deltas), tuple(steps), str(device)), make)


def _fuse_history(cur_pts, cur_lab, hist_pts, hist_lab, pose0, hist_poses, deltas, steps, hist_pseudo=None):
    """All history scans in one pass: concatenate, transform every point with its scan's pose (ts_fuse_scans),
    look the class-step decision up per point.  Returns the un-filtered stack [current | history] (x, y, z,
    intensity, time flag), its labels and the keep mask; order = current scan first, then history oldest first, each
    in file order - the order the reference's loop produces (semantickitti_ms.py:140-149).

    hist_pseudo[i] (optional): the class whose CANONICAL raw id the point's pseudo label is, or -1 - the reference
    compares the raw pseudo label with LEARNING_MAP_INV[class] (semantickitti_ms.py:303-308), so a raw id that maps to
    a class without being its canonical id (the moving-object ids 252 .. 259) is never aggregated.  Default: the
    annotation classes `hist_lab` (exact when labels only hold canonical ids, as the synthetic scans do)."""
    dev = cur_pts.device
    n_cur = cur_pts.shape[0]
    if len(hist_pts) == 0:
        flag = torch.ones((n_cur, 1), dtype=cur_pts.dtype, device=dev)
        return torch.cat([cur_pts[:, :4], flag], 1), cur_lab.long(), torch.ones(n_cur, dtype=torch.bool, device=dev)
    scan_idx, table = _history_index([p.shape[0] for p in hist_pts], deltas, steps, dev)
    hp = torch.cat([p[:, :4] for p in hist_pts], 0).contiguous()
    hl = torch.cat(hist_lab, 0).long()
    fused = B.fuse_scans(hp, scan_idx, pose0, torch.stack(list(hist_poses), 0))
    keep = _step_keep(table, scan_idx, hl if hist_pseudo is None else torch.cat(hist_pseudo, 0).long(), neg_last=True)
    pts = torch.cat([cur_pts[:, :4], fused], 0)
    flag = torch.zeros((pts.shape[0], 1), dtype=pts.dtype, device=dev)
    flag[:n_cur] = 1                               # append_time_flag (semantickitti_ms.py:253-257)
    mask = torch.cat([torch.ones(n_cur, dtype=torch.bool, device=dev), keep])
    return torch.cat([pts, flag], 1), torch.cat([cur_lab.long(), hl]), mask


def fuse_multiscan(cur_pts, cur_lab, hist_pts: List[torch.Tensor], hist_lab: List[torch.Tensor], pose0,
                   hist_poses: List[torch.Tensor], deltas: Sequence[int], steps: Sequence[int]):
    """Current scan + filtered, pose-aligned history scans -> (raw_data_ms [n, 5], labels_ms [n]).

    cur_pts / hist_pts[i]: float32 [n, 4] (x, y, z, intensity) in their own sensor frames;
    *_lab: class ids (learning-map ids, 0..C-1); poses: 4x4 float32 (world <- sensor);
    deltas[i] < 0 is the frame offset of hist_pts[i].  History order is preserved (oldest first, as the
    reference iterates delta = -MULTISCAN .. -1)."""
    raw, lab, mask = _fuse_history(cur_pts, cur_lab, hist_pts, hist_lab, pose0, hist_poses, deltas, steps)
    return raw[mask], lab[mask]


def _quantize(points, voxel_size, shift=None):
    coords4, mins = B.voxel_coords(points, voxel_size, shift=shift)
    index, inverse = B.sparse_quantize(coords4)
    return coords4[:, :3], mins, index.long(), inverse.long()


def _one_aug(aug):
    """the single sample's record out of aug= (an AugParams or a list holding one)"""
    rec = pack_params(aug)
    if rec.shape[0] != 1:
        raise ValueError("aug holds %d records for one sample" % rec.shape[0])
    return rec


def clamp_corner(points) -> torch.Tensor:
    """points[:, :3].min(0), the corner a sample's fused and FOV clouds are clamped to.  (The min over dim 0 of the [n, 3] slice runs
    in one of torch's slow few-column reductions, 175 us for 35k points: the row-wise minimum of the transposed copy takes ~10 us.)"""
    return points[:, :3].t().contiguous().min(1).values


def voxelize_sample(points, labels, voxel_size, name="", aug=None) -> Dict:
    """Single-frame sample (semantickitti_voxel.py:119-150); aug: the sample's AugParams, applied first (:89-99)."""
    if aug is not None:
        points = augment_points(points, _one_aug(aug))
    pc, _, inds, inverse = _quantize(points, voxel_size)
    return {"name": name, "lidar": SparseTensor(points[inds], pc[inds]), "targets": SparseTensor(labels[inds], pc[inds]),
            "targets_mapped": SparseTensor(labels, pc), "inverse_map": SparseTensor(inverse, pc),
            "num_points": torch.tensor([points.shape[0]])}


def voxelize_sample_ms(points, labels, points_ms, labels_ms, voxel_size, name="", keep=None, return_shift=False, aug=None) -> Dict:
    """Multi-scan sample (semantickitti_voxel_ms.py:121-187): both clouds voxelised, the single-frame one
    shifted by the fused cloud's minimum.  `keep` (optional bool mask over points_ms) is AND-ed with the clamp
    so the class-step filter and the clamp cost one compaction (one host read) instead of two.
    aug: the sample's AugParams - both clouds go through the same kernel with the same record first (:90-119), so the current
    scan's rows carry the same bits in both and the clamp, the voxel coordinates and the features see augmented coordinates."""
    if aug is not None:
        rec = torch.from_numpy(_one_aug(aug)).to(points.device, non_blocking=True)
        points, points_ms = augment_points(points, rec), augment_points(points_ms, rec)
    clamp = (points_ms[:, :3] >= clamp_corner(points)).all(1)             # :121-124
    if keep is not None:
        clamp = clamp & keep
    points_ms, labels_ms = points_ms[clamp].contiguous(), labels_ms[clamp]
    pc_ms, mins_ms, inds_ms, inverse_ms = _quantize(points_ms, voxel_size)
    pc, _, inds, inverse = _quantize(points, voxel_size, shift=mins_ms)   # pc_ -= pc_ms_.min(0)  (:130)
    extra = {"_shift": mins_ms} if return_shift else {}      # the fused cloud's minimum: further clouds of the sample share it
    return {
        **extra,
        "name": name,
        "lidar": SparseTensor(points[inds], pc[inds]), "targets": SparseTensor(labels[inds], pc[inds]),
        "targets_mapped": SparseTensor(labels, pc), "inverse_map": SparseTensor(inverse, pc),
        "num_points": torch.tensor([points.shape[0]]),
        "lidar_ms": SparseTensor(points_ms[inds_ms], pc_ms[inds_ms]),
        "targets_ms": SparseTensor(labels_ms[inds_ms], pc_ms[inds_ms]),
        "targets_mapped_ms": SparseTensor(labels_ms, pc_ms), "inverse_map_ms": SparseTensor(inverse_ms, pc_ms),
        "num_points_ms": torch.tensor([points_ms.shape[0]]),
    }


def voxelize_fov_cloud(sample: Dict, fov, voxel_size, fov_labels=None):
    """The camera samples' third cloud, clamped already: `fov` [m, 6] rounded and shifted like the other two - `sample` is
    voxelize_sample_ms's with return_shift=True, whose "_shift" is taken out - and grouped per voxel into sample["lidar_fov_ms"].
    Returns fov_labels of the voxels' representatives (None without labels)."""
    pc_fov, _, inds_fov, _ = _quantize(fov, voxel_size, shift=sample.pop("_shift"))
    sample["lidar_fov_ms"] = SparseTensor(fov[inds_fov], pc_fov[inds_fov])
    return None if fov_labels is None else fov_labels[inds_fov]


def voxelize_fov(sample: Dict, point, fov, voxel_size, fov_labels=None):
    """voxelize_fov_cloud of `fov` clamped to the single-frame cloud `point`'s corner (semantickitti_voxel_ms_mm.py:124-204 / nuscenes_: 133-204)"""
    inside = (fov[:, :3] >= clamp_corner(point)).all(1)
    return voxelize_fov_cloud(sample, fov[inside].contiguous(), voxel_size, None if fov_labels is None else fov_labels[inside])


def _stack_sparse(items: List[SparseTensor]) -> SparseTensor:
    coords = [torch.cat([t.coords, torch.full((t.coords.shape[0], 1), b, dtype=torch.int32, device=t.coords.device)], 1)
              for b, t in enumerate(items)]
    return SparseTensor(torch.cat([t.feats for t in items], 0), torch.cat(coords, 0).contiguous(), items[0].stride)


def _prefix_mask(n_cur: Sequence[int], n_ms: Sequence[int], device) -> torch.Tensor:
    """point_mask (semantickitti_voxel_ms.py:204-210): bool [sum(n_ms)], true on the first n_cur[b] rows of every fused cloud - the
    current frame where it is the fused cloud's prefix"""
    mask = torch.zeros(sum(n_ms), dtype=torch.bool, device=device)
    at = 0
    for a, m in zip(n_cur, n_ms):
        mask[at:at + a] = True
        at += m
    return mask


def collate_batch(samples: List[Dict]) -> Dict:
    """sparse_collate_fn + offsets + point_mask (semantickitti_voxel_ms.py:189-212), on device."""
    out = {}
    for key, first in samples[0].items():
        col = [s[key] for s in samples]
        if isinstance(first, SparseTensor):
            out[key] = _stack_sparse(col)
        elif isinstance(first, torch.Tensor):
            out[key] = torch.stack(col, 0)
        else:
            out[key] = col
    dev = out["lidar"].coords.device
    for sfx in ("", "_ms"):
        if "lidar" + sfx in out:
            sizes = torch.tensor([s["lidar" + sfx].coords.shape[0] for s in samples])
            out["offset" + sfx] = torch.cumsum(sizes, 0).int().to(dev)
    if "num_points_ms" in out:
        out["point_mask"] = _prefix_mask([int(s["num_points"]) for s in samples], [int(s["num_points_ms"]) for s in samples], dev)
    return out


def _aug_records(aug, n_samples):
    """aug= of a batch -> float64 [B, 8] records, one per sample"""
    rec = pack_params(aug)
    if rec.shape[0] != n_samples:
        raise ValueError("aug holds %d records for %d samples" % (rec.shape[0], n_samples))
    return rec


def _mix_records(mix, partners, n_samples):
    """mix= / partners= of a batch, checked: one MixParams per sample, a partner scan for every sample whose mix moves rows of one"""
    mix = list(mix)
    if len(mix) != n_samples or not all(isinstance(p, M.MixParams) for p in mix):
        raise ValueError("mix must hold one MixParams per sample")
    partners = [None] * n_samples if partners is None else list(partners)
    if len(partners) != n_samples:
        raise ValueError("partners must hold one scan (or None) per sample")
    for p, q in zip(mix, partners):
        # (the reference's LaserMix branch is the identity: it needs no partner)
        if q is None and (p.kind == M.POLAR or (p.kind == M.LASER and p.degrees)):
            raise ValueError("a sample that is mixed needs its partner scan")
    return mix, partners


def _fused_cloud(s, steps):
    """(current scan, its labels, un-filtered stack [current | history] [m, 5], its labels, keep mask) of one scan dict;
    stack[keep] is the fused cloud the reference's `__getitem__` holds when it reaches the mix (semantickitti_ms.py:140-149), for a
    sample and for its partner alike"""
    pts, lab, poses = s["points"], s["labels"], s["poses"]
    t = len(pts) - 1
    raw_all, lab_all, keep = _fuse_history(pts[t], lab[t], pts[:t], lab[:t], poses[t], poses[:t], _deltas(s), steps, s.get("pseudo"))
    return pts[t], lab[t].long(), raw_all, lab_all, keep


def _moving_rows(clouds: List[Dict]):
    """The rows ts_stage_moving_* work on, for scan dicts with `raw_labels`: (points [N, 4] - a fresh tensor: the current scans of
    all clouds, then their history scans pose-fused in one launch -, full labels [N] int64, cloud [N] int32, frame offset [N] int32
    (0 on the current rows), current rows per cloud, history rows per cloud, the walk)."""
    if any(c.get("raw_labels") is None for c in clouds):
        raise ValueError("moving= needs the full labels of every scan: scan dicts with `raw_labels`")
    dev = clouds[0]["points"][-1].device
    walk = _walk_scans(clouds, ())
    (hist_pts, _, _, lengths, owner, pose0s, poses, _), current = walk
    deltas = [d for c in clouds for d in _deltas(c)]
    n_cur = [int(c[0].shape[0]) for c in current]
    n_hist = [c[3] for c in current]
    parts = [c[0][:, :4] for c in current]
    if hist_pts:
        parts.append(B.fuse_scans_batch(torch.cat(hist_pts, 0).contiguous(), rows_index32(lengths, dev), torch.stack(pose0s, 0),
                                        torch.stack(poses, 0)))
    pts = torch.cat(parts, 0)                          # (torch.cat's fresh tensor: the resident scans stay untouched)
    raw = torch.cat([c["raw_labels"][-1].reshape(-1) for c in clouds] +
                    [r.reshape(-1) for c in clouds for r in c["raw_labels"][:-1]], 0).long()
    if raw.shape[0] != pts.shape[0]:
        raise ValueError("raw_labels must hold one label per point of every scan")

    def make():
        seg = rows_index(n_cur + lengths, dev)
        cloud = torch.tensor(list(range(len(clouds))) + owner, dtype=torch.int32).to(dev)[seg]
        delta = torch.tensor([0] * len(clouds) + deltas, dtype=torch.int32).to(dev)[seg]
        return cloud.contiguous(), delta.contiguous()
    cloud32, delta32 = _cached(("moving-rows", tuple(n_cur), tuple(lengths), tuple(owner), tuple(deltas), str(dev)), make)
    return pts, raw, cloud32, delta32, n_cur, n_hist, walk


_MOVING_CAP = 1024         # TS_MOVING_MAX_CANDIDATES: candidates of one call, all clouds together
_SENTINEL = 1 << 62


def moving_tables(scans: List[Dict], partners=None):
    """[(MovingTable of scans[b], MovingTable of partners[b] or None)]: the per-instance statistics the draws of the SMSA recipe's
    moving-object augmentation depend on (data/moving.py `draw_smsa_sample`), for the samples of a batch and their mix partners in
    one go: one pose-fuse launch, the candidates of every cloud - the distinct full labels of its current rows with raw class 18,
    20, 253 or 255 - by a sort of the current rows' (cloud, label) keys, ts_stage_moving_stats (six launches), and ONE host read:
    table sizes, candidates, counts and statistics in one copy."""
    partners = [None] * len(scans) if partners is None else list(partners)
    if len(partners) != len(scans):
        raise ValueError("partners must hold one scan (or None) per sample")
    clouds = list(scans) + [p for p in partners if p is not None]
    pts, raw, cloud32, delta32, n_cur, n_hist, _ = _moving_rows(clouds)
    dev, nc, ncl, cap = pts.device, sum(n_cur), len(clouds), _MOVING_CAP
    cur_raw = raw[:nc]
    cls = cur_raw & 0xFFFF
    cand_row = (cls == 18) | (cls == 20) | (cls == 253) | (cls == 255)
    key = torch.where(cand_row, (cloud32[:nc].long() << 32) | cur_raw, torch.full_like(cur_raw, _SENTINEL))
    key = torch.sort(key).values
    first = key != _SENTINEL
    first[1:] &= key[1:] != key[:-1]
    pos = torch.cumsum(first, 0) - 1
    # candidate i of the batch -> cand[i]; everything else -> the spare cell behind them
    cand = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    cand.scatter_(0, torch.where(first & (pos < cap), pos, torch.full_like(pos, cap)), key & 0xFFFFFFFF)
    per = torch.zeros(ncl + 1, dtype=torch.int64, device=dev)
    per.scatter_add_(0, torch.where(first, key >> 32, torch.full_like(key, ncl)), torch.ones_like(key))
    start = torch.cat([per.new_zeros(1), torch.cumsum(per[:ncl], 0)])
    cap_rows = min(int(pts.shape[0]), 1 << 20)
    counts, stats, matched = B.stage_moving_stats(pts, nc, raw, cloud32, delta32, cand[:cap], start.int(), cap_rows=cap_rows)
    host = torch.cat([start, matched, cand[:cap], counts.view(-1).long(), stats.view(torch.int32).view(-1).long()]).cpu().numpy()
    start, matched, host = host[:ncl + 1], int(host[ncl + 1]), host[ncl + 2:]                   # the host read
    if int(start[-1]) > cap or matched > cap_rows:
        raise ValueError("moving_tables: %d candidates (at most %d), %d of their rows (at most %d) in one call"
                         % (int(start[-1]), cap, matched, cap_rows))
    labels, counts = host[:cap], host[cap:4 * cap].astype(np.int32).reshape(cap, 3)
    stats = host[4 * cap:].astype(np.int32).view(np.float32).reshape(cap, 9)
    tables = [MV.MovingTable(labels[a:b].copy(), counts[a:b].copy(), stats[a:b].copy(), int(nh))
              for a, b, nh in zip(start[:-1], start[1:], n_hist)]
    theirs = iter(tables[len(scans):])
    return [(tables[b], None if p is None else next(theirs)) for b, p in enumerate(partners)]


def _moving_records(moving, partner_moving, n_samples):
    """moving= / partner_moving= of a batch, checked: one MovingParams (or None: nothing moves) per sample"""
    moving = list(moving)
    partner_moving = [None] * n_samples if partner_moving is None else list(partner_moving)
    if len(moving) != n_samples or len(partner_moving) != n_samples or \
            not all(p is None or isinstance(p, MV.MovingParams) for p in moving + partner_moving):
        raise ValueError("moving / partner_moving must hold one MovingParams (or None) per sample")
    return moving, partner_moving


def _moved_clouds(clouds: List[Dict], params):
    """The moving-object augmentation of scan dicts with `raw_labels` (params[i]: the MovingParams of clouds[i] or None): the rows of
    _moving_rows shifted and relabelled by ONE ts_stage_moving_apply launch with the uploaded records.  Returns (current rows of all
    clouds [Nc, 4], their classes int64 - the 26-class map of the rewritten raw classes -, fused history rows [Nh, 4], their
    classes, their pseudo classes - the class whose canonical raw id the ORIGINAL raw class is, else -1: the class-step mask is
    computed before the augmentation, semantickitti_ms_ms.py:440-445 -, the walk)."""
    pts, raw, cloud32, delta32, n_cur, _, walk = _moving_rows(clouds)
    dev, nc = pts.device, sum(n_cur)
    rec_lab, rec_start, rec = MV.pack_moving(params)
    def make():
        canon = np.full(1 << 16, -1, dtype=np.int64)           # every 16-bit raw class: one past the label definition is no class's
        canon[:len(MV.CANONICAL_CLASS)] = MV.CANONICAL_CLASS
        return torch.from_numpy(MV.LABEL_TABLE).to(dev), torch.from_numpy(canon).to(dev)
    lut, canon = _cached(("moving-lut", str(dev)), make)
    lab = B.stage_moving_apply(pts, nc, raw, cloud32, delta32, torch.from_numpy(rec_lab).to(dev, non_blocking=True),
                               torch.from_numpy(rec_start).to(dev, non_blocking=True),
                               torch.from_numpy(rec).to(dev, non_blocking=True), lut)
    if all(c.get("pseudo") is None for c in clouds):
        pseudo = canon[raw[nc:] & 0xFFFF]
    else:
        pseudo = torch.cat([(canon[r.reshape(-1).long() & 0xFFFF] if c.get("pseudo") is None else c["pseudo"][i].long())
                            for c in clouds for i, r in enumerate(c["raw_labels"][:-1])] +
                           [torch.empty(0, dtype=torch.int64, device=dev)], 0)
    return pts[:nc], lab[:nc], pts[nc:], lab[nc:], pseudo, walk


def _fused_cloud_moved(s, steps, params):
    """_fused_cloud of one scan dict after its moving-object augmentation (steps: all 26 classes')"""
    cur, lab, fused, hl, ps, ((_, _, _, lengths, _, _, _, _), _) = _moved_clouds([s], [params])
    dev, n_cur = cur.device, cur.shape[0]
    flag = torch.zeros((n_cur + fused.shape[0], 1), dtype=cur.dtype, device=dev)
    flag[:n_cur] = 1
    raw_all = torch.cat([torch.cat([cur, fused], 0), flag], 1)
    keep = torch.ones(n_cur, dtype=torch.bool, device=dev)
    if lengths:
        scan_idx, table = _history_index(lengths, _deltas(s), steps, dev)
        keep = torch.cat([keep, _step_keep(table, scan_idx, ps, neg_last=True)])
    return cur, lab, raw_all, torch.cat([lab, hl]), keep


def build_multiscan_batch_per_sample(scans: List[Dict], voxel_size: float, steps: Sequence[int], aug=None, mix=None,
                                     partners=None, moving=None, partner_moving=None) -> Dict:
    """build_multiscan_batch sample by sample (fuse, clamp, two voxelisations and ~55 launches per sample, then collate): the
    form the batched stage below replaced; kept as its cross-check (tests) and for TASEG_STAGE_BATCHED=0.  moving= /
    partner_moving=: one ts_stage_moving_apply launch per cloud, no host read of its own."""
    samples = []
    fused_cloud = _fused_cloud
    if moving is not None:
        moving, partner_moving = _moving_records(moving, partner_moving, len(scans))
        steps = MV.pad_steps(steps)
        fused_cloud = None
    rec = None if aug is None else _aug_records(aug, len(scans))
    if mix is not None:
        mix, partners = _mix_records(mix, partners, len(scans))
    for b, s in enumerate(scans):
        one = None if rec is None else rec[b:b + 1]
        cur, lab, raw, lab_ms, keep = _fused_cloud(s, steps) if fused_cloud else _fused_cloud_moved(s, steps, moving[b])
        if mix is None or mix[b].kind == M.NONE:
            # (the class-step filter rides on the clamp's compaction)
            samples.append(voxelize_sample_ms(cur, lab, raw, lab_ms, voxel_size, s.get("name", ""), keep=keep, aug=one))
            continue
        cur, raw, lab_ms = cur[:, :4], raw[keep], lab_ms[keep]
        if partners[b] is None:
            pcur, plab, praw, plab_ms = cur[:0], lab[:0], raw[:0], lab_ms[:0]
        else:
            pcur, plab, praw, plab_ms, pkeep = _fused_cloud(partners[b], steps) if fused_cloud else \
                _fused_cloud_moved(partners[b], steps, partner_moving[b])
            pcur, praw, plab_ms = pcur[:, :4], praw[pkeep], plab_ms[pkeep]
        # the same record on the single-frame pair and on the fused pair (semantickitti_ms.py:182-185, :221-234)
        cur, lab = M.mix_points(cur, lab, pcur, plab, mix[b])
        raw, lab_ms = M.mix_points(raw, lab_ms, praw, plab_ms, mix[b])
        samples.append(voxelize_sample_ms(cur, lab, raw, lab_ms, voxel_size, s.get("name", ""), aug=one))
    return collate_batch(samples)


def voxelize_batch_ms(cur_list: List[torch.Tensor], lab_list: List[torch.Tensor], cur_ms: torch.Tensor, hist_pts: torch.Tensor,
                      hist_lab: torch.Tensor, hist_scan: torch.Tensor, hist_cls: torch.Tensor, table: torch.Tensor,
                      sample_of_scan: torch.Tensor, voxel_size: float, names: List[str], pre_keep=None, neg_col: int = -1) -> Dict:
    """collate_batch([voxelize_sample_ms(...) for every sample]) for the WHOLE batch in one chain of launches
    (semantickitti_voxel_ms.py:121-212 / nuscenes_voxel_ms.py:77-212): the per-sample clamp minima in one launch, the class-step
    rule + pre-filter + clamp in one launch (csrc/stage.hip), ONE compaction, the fused clouds written sample-major with the current
    scan first (no sort), ONE voxelisation of all fused clouds (per-sample minima, batch-keyed radix sort: voxel order (b, x, y, z),
    representative = first point, inverse map) and ONE of the current scans shifted by their fused cloud's minimum, gathers on the
    whole batch.  Four host reads per batch (kept points, kept points per sample, the two voxel counts) instead of three per
    sample.  Same tensors, bit for bit, as the per-sample path.

    cur_list[b] [n_b, F] / lab_list[b] int64: the current scans (single-frame cloud);  cur_ms [sum n_b, Fm]: the same points as
    they appear in the fused clouds (time flag / time column);  hist_*: the transformed history points of all samples, sample-major:
    points [Nh, Fm], labels [Nh] int64, global scan / sweep index [Nh] int32, pseudo class [Nh] int64 (neg_col: the table column of
    a negative class), table [S, C] bool (is class c taken from scan s), sample_of_scan [S] int64; pre_keep [Nh] bool (optional:
    the ego-box filter)."""
    dev = cur_ms.device
    nb = len(cur_list)
    if nb > 64:
        raise ValueError("voxelize_batch_ms: at most 64 samples per batch")
    n_cur = [int(c.shape[0]) for c in cur_list]
    cur = torch.cat(cur_list, 0).contiguous()
    cur_lab = torch.cat(lab_list, 0)
    cur_b = rows_index(n_cur, dev)
    n_c = cur.shape[0]
    if hist_pts.shape[0]:
        lo = B.segment_min3(cur, cur_b, nb)        # minimum of every current scan: the fused cloud is clamped to it (:121-124)
        keep, hist_b = B.stage_keep_flags(hist_pts, hist_scan, hist_cls, table, sample_of_scan, lo, pre_keep=pre_keep, neg_col=neg_col)
        idx = keep.nonzero().squeeze(1)                                 # host read 1 (the compaction's size)
        cur_start = torch.tensor(list(accumulate(n_cur, initial=0)), dtype=torch.int64).to(dev, non_blocking=True)
        kept_start = torch.searchsorted(hist_b[idx], torch.arange(nb + 1, device=dev))
        ms_pts, ms_lab, ms_b, ms_b32, point_mask = B.stage_layout(cur_ms, cur_lab, cur_b, hist_pts, hist_lab, hist_b, idx, cur_start,
                                                                  kept_start)
        kept = (kept_start[1:] - kept_start[:-1]).tolist()              # host read 2 (kept history points per sample)
        n_ms = [a + k for a, k in zip(n_cur, kept)]
    else:
        ms_b, ms_b32, ms_pts, ms_lab = cur_b, cur_b.int(), cur_ms.contiguous(), cur_lab
        point_mask = torch.ones(n_c, dtype=torch.bool, device=dev)
        n_ms = list(n_cur)
    return _voxelize_layout(cur, cur_lab, cur_b, n_cur, ms_pts, ms_lab, ms_b, ms_b32, n_ms, point_mask, voxel_size, names)


def _voxelize_layout(cur, cur_lab, cur_b, n_cur, ms_pts, ms_lab, ms_b, ms_b32, n_ms, point_mask, voxel_size, names,
                     return_shift=False) -> Dict:
    """the two voxelisations and the batch_dict of voxelize_batch_ms, from the clouds laid out sample-major: cur [sum n_cur, F] with
    labels and sample index (int64), the fused clouds ms_pts [sum n_ms, Fm] with labels and sample index (int64 and int32).
    return_shift: returns (batch_dict, the fused clouds' minima [B, 3] int32) - further clouds of the samples share that shift
    (data/kd.py)."""
    dev, nb = cur.device, len(n_cur)
    coords_ms, mins = B.voxel_coords(ms_pts, voxel_size, batch_idx=ms_b32, n_batch=nb)
    index_ms, inverse_ms = B.sparse_quantize(coords_ms)                 # host read 3 (voxels of the fused clouds)
    coords_c, _ = B.voxel_coords(cur, voxel_size, batch_idx=rows_index32(n_cur, dev), n_batch=nb, shift=mins)   # pc_ -= pc_ms_.min(0) (:130)
    index_c, inverse_c = B.sparse_quantize(coords_c)                    # host read 4 (voxels of the current scans)
    vox_ms, offset_ms, inv_ms = B.stage_split_voxels(coords_ms, index_ms, inverse_ms, ms_b, nb)
    vox_c, offset_c, inv_c = B.stage_split_voxels(coords_c, index_c, inverse_c, cur_b, nb)
    index_ms, index_c = index_ms.long(), index_c.long()
    batch = {
        "name": list(names),
        "lidar": SparseTensor(cur[index_c], vox_c), "targets": SparseTensor(cur_lab[index_c], vox_c),
        "targets_mapped": SparseTensor(cur_lab, coords_c), "inverse_map": SparseTensor(inv_c, coords_c),
        "num_points": torch.tensor(n_cur).view(-1, 1),
        "lidar_ms": SparseTensor(ms_pts[index_ms], vox_ms), "targets_ms": SparseTensor(ms_lab[index_ms], vox_ms),
        "targets_mapped_ms": SparseTensor(ms_lab, coords_ms), "inverse_map_ms": SparseTensor(inv_ms, coords_ms),
        "num_points_ms": torch.tensor(n_ms).view(-1, 1),
        "offset": offset_c, "offset_ms": offset_ms, "point_mask": point_mask,
    }
    return (batch, mins) if return_shift else batch


def _walk_scans(clouds: List[Dict], steps: Sequence[int]):
    """One pass over scan dicts (build_multiscan_batch's `scans[b]`).  Returns the history scans of all of them, flat and in order -
    (points [:, :4], labels, pseudo classes or the labels where a dict has none, lengths, owner = index of the dict in `clouds`,
    the owner's current pose per scan, pose, _kitti_row) - and per dict (current scan as stored, its labels int64, first history
    row, history rows)."""
    hist_pts, hist_lab, hist_ps, lengths, owner, pose0s, poses, rows = hist = [], [], [], [], [], [], [], []
    current, n_hist = [], 0
    for b, s in enumerate(clouds):
        pts, ps = s["points"], s["poses"]
        lab = s["labels"] if s.get("labels") is not None else s["raw_labels"]      # (moving=: the classes come from raw_labels)
        t = len(pts) - 1
        deltas = _deltas(s)
        pseudo = s.get("pseudo")
        first = n_hist
        for i in range(t):
            hist_pts.append(pts[i][:, :4])
            hist_lab.append(lab[i])
            hist_ps.append(lab[i] if pseudo is None else pseudo[i])
            lengths.append(int(pts[i].shape[0]))
            owner.append(b)
            pose0s.append(ps[t])
            poses.append(ps[i])
            rows.append(_kitti_row(deltas[i], steps))
            n_hist += lengths[-1]
        current.append((pts[t], lab[t].long(), first, n_hist - first))
    return hist, current


def _mix_and_voxelize(used, heads, fused, fused_lab, fused_keep, mix, aug, voxel_size, time_flag=False) -> Dict:
    """The tail of both datasets' mixed batch.  used[b] = [sample b, its partner or None]; heads: for every cloud of `used` that is
    not None, in order, (head rows [n, F] - current scan or keyframe, cut to the mixed columns -, labels int64, first row and number
    of rows of its history in `fused`); fused [Nh, F], fused_lab int64, fused_keep bool: the fused history rows of all those clouds,
    un-filtered, with the class-step rule (and whatever else drops a row) as a keep byte - no compaction before the mix.
    ts_stage_mix on the single-frame pairs and on the fused pairs of the whole batch (three launches each, their row counts in one
    host read), the augmentation of both clouds through the mix's job column, the minima of the mixed single-frame clouds
    (ts_segment_min3), the clamp of EVERY fused row against them as one stable compaction (ts_stage_clamp_compact: after a mix the
    head is no prefix of the fused cloud any more; semantickitti_voxel_ms.py:121-124) with the second host read, the survivors per
    sample, and both voxelisations.  point_mask stays what the reference's collate_batch makes it (_prefix_mask).
    time_flag: append SemanticKITTI's flag column to the fused rows before their mix - 1 on a head, 0 on history."""
    dev, nb = fused.device, len(used)
    # job-major rows: [head | partner's head] for the single-frame mix, [head | history | partner's head | partner's history] for
    # the fused one
    s_pts, s_lab, s_n = [], [], ([], [])
    m_pts, m_lab, m_keep, m_len, m_n = [], [], [], [], ([], [])
    ones = torch.ones(max(int(h[0].shape[0]) for h in heads), dtype=torch.bool, device=dev)
    heads = iter(heads)
    for pair in used:
        for k, c in enumerate(pair):
            n = nh = 0
            if c is not None:
                head, lab, first, nh = next(heads)
                n = int(head.shape[0])
                s_pts.append(head)
                s_lab.append(lab)
                m_pts += [head, fused[first:first + nh]]
                m_lab += [lab, fused_lab[first:first + nh]]
                m_keep += [ones[:n], fused_keep[first:first + nh]]
            m_len += [n, nh]
            s_n[k].append(n)
            m_n[k].append(n + nh)
    ms_in = torch.cat(m_pts, 0)
    if time_flag:
        flag = (rows_index(m_len, dev) % 2 == 0).to(torch.float32)      # append_time_flag (:253-257): the pieces alternate
        ms_in = torch.cat([ms_in, flag.unsqueeze(1)], 1)
    totals = torch.empty((2, nb), dtype=torch.int64, device=dev)
    cur, cur_lab, cur_b32, _ = B.stage_mix(torch.cat(s_pts, 0), torch.cat(s_lab, 0), mix, *s_n, totals=totals[0])
    ms, ms_lab, ms_b32, _ = B.stage_mix(ms_in, torch.cat(m_lab, 0), mix, *m_n, keep=torch.cat(m_keep, 0), totals=totals[1])
    n_cur, n_mixed = totals.tolist()                                    # host read 1 (rows of both mixes, all samples)
    cur, cur_lab, cur_b32 = cur[:sum(n_cur)], cur_lab[:sum(n_cur)], cur_b32[:sum(n_cur)]
    ms, ms_lab, ms_b32 = ms[:sum(n_mixed)], ms_lab[:sum(n_mixed)], ms_b32[:sum(n_mixed)]
    if aug is not None:
        rec_dev = torch.from_numpy(_aug_records(aug, nb)).to(dev, non_blocking=True)
        augment_points(cur, rec_dev, cur_b32, out=cur)
        augment_points(ms, rec_dev, ms_b32, out=ms)
    cur_b = cur_b32.long()
    lo = B.segment_min3(cur, cur_b, nb)
    ms, ms_lab, ms_b, ms_b32, counts = B.stage_clamp_compact(ms, ms_lab, ms_b32, lo)
    n_ms = counts.tolist()                                              # host read 2 (fused rows per sample)
    kept = sum(n_ms)
    ms, ms_lab, ms_b, ms_b32 = ms[:kept], ms_lab[:kept], ms_b[:kept], ms_b32[:kept]
    return _voxelize_layout(cur, cur_lab, cur_b, n_cur, ms, ms_lab, ms_b, ms_b32, n_ms, _prefix_mask(n_cur, n_ms, dev), voxel_size,
                            [pair[0].get("name", "") for pair in used])


def _build_multiscan_batch_mix(scans, partners, mix, voxel_size, steps, aug, moving=None, partner_moving=None) -> Dict:
    """build_multiscan_batch with mix=: the samples' and the used partners' history scans (_walk_scans) pose-fused in ONE launch
    (fuse_scans_batch), the class-step rule as a keep byte per row (_step_table, _step_keep), then _mix_and_voxelize with the time
    flag: two host reads before the voxelisation.  moving= / partner_moving=: the samples' and the partners' moving-object
    augmentation first, one ts_stage_moving_apply launch for all of them (_moved_clouds), which hands out the current rows, the
    fused history and the pseudo classes of the raw classes as they were."""
    dev = scans[0]["points"][-1].device
    # the clouds that take part, in order: every sample's own, then its partner's where its mix moves rows of one
    used = [[s, partners[b] if mix[b].kind != M.NONE else None] for b, s in enumerate(scans)]
    clouds = [c for pair in used for c in pair if c is not None]
    (hist_pts, hist_lab, hist_ps, lengths, owner, pose0s, poses, rows), current = _walk_scans(clouds, steps)
    if moving is not None:
        params = [q for b, pair in enumerate(used) for c, q in zip(pair, (moving[b], partner_moving[b])) if c is not None]
        cur_all, cur_lab_all, fused, hl, hps, _ = _moved_clouds(clouds, params)
        n_cur = [int(c[0].shape[0]) for c in current]
        current = [(p, l, c[2], c[3]) for p, l, c in zip(torch.split(cur_all, n_cur), torch.split(cur_lab_all, n_cur), current)]
    elif hist_pts:
        hl = torch.cat(hist_lab, 0).long()
        hps = hl if all(c.get("pseudo") is None for c in clouds) else torch.cat(hist_ps, 0).long()
        fused = B.fuse_scans_batch(torch.cat(hist_pts, 0).contiguous(), rows_index32(lengths, dev), torch.stack(pose0s, 0),
                                   torch.stack(poses, 0))
    else:
        fused = torch.empty((0, 4), dtype=torch.float32, device=dev)
        hl = torch.empty(0, dtype=torch.int64, device=dev)
    if hist_pts:
        hkeep = _step_keep(_step_table("kitti-table", rows, owner, dev)[0], rows_index32(lengths, dev), hps, neg_last=True)
    else:
        hkeep = torch.empty(0, dtype=torch.bool, device=dev)
    heads = [(scan[:, :4], lab, first, nh) for scan, lab, first, nh in current]
    return _mix_and_voxelize(used, heads, fused, hl, hkeep, mix, aug, voxel_size, time_flag=True)


def build_multiscan_batch(scans: List[Dict], voxel_size: float, steps: Sequence[int], aug=None, mix=None, partners=None,
                          moving=None, partner_moving=None) -> Dict:
    """scans[b] = dict(points=[T+1 tensors, current LAST], labels=[...], poses=[...], name=str
    [, deltas=[frame offsets of the history scans], pseudo=[pseudo classes of the history scans, see _fuse_history]]).
    Returns the collated batch_dict MinkUNetMs consumes.  The whole batch goes through ONE chain of launches: one pose-fuse
    launch over every history point of every sample of _walk_scans (ts_fuse_scans_batch), the class-step rule as one table
    lookup (_step_table), then voxelize_batch_ms.
    aug: one AugParams per sample (data/augment.py) or None.  With it the current scans and ALL pose-fused history rows are
    augmented in place, one ts_stage_augment launch each (the history rows pick their sample's record through their scan index),
    before the clamp minima are taken - two launches and one small host-to-device copy more than aug=None, the un-augmented path.
    mix: one MixParams per sample (data/mix.py) or None; partners[b]: the scan dict of sample b's partner (None where its mix needs
    none).  With it every sample is mixed with its partner - PolarMix / LaserMix on the single-frame pair and on the fused pair,
    semantickitti_ms.py:151-237 - before the augmentation, and every fused row is clamped by ts_stage_clamp_compact
    (_build_multiscan_batch_mix, _mix_and_voxelize: two host reads before the voxelisation); mix=None is the path without it,
    launch for launch.
    moving: one MovingParams per sample (data/moving.py; None in the list: nothing moves) or None; partner_moving[b]: the
    MovingParams of sample b's partner.  The SMSA recipe (semantickitti_ms_ms.py): scan dicts then carry `raw_labels` - one tensor
    of FULL uint32 labels (any integer dtype wide enough) per scan, parallel to `points` - and `labels` is not read: the classes are
    the 26-class map of the raw classes (data/moving.py LABEL_TABLE), `steps` shorter than 26 counts as 0 for the rest.  The
    instances of the records are shifted and relabelled on the current scans and on the UN-FILTERED fused history - one
    ts_stage_moving_apply launch and three small host-to-device copies for all clouds of the batch, samples and partners, no host
    read - before the keep bytes of the class-step rule (computed from the raw classes as they were) take effect, before the mix
    and the augmentation.  The statistics its draws need come from `moving_tables` before this call (one host read per batch):

        tables = moving_tables(scans, partners)
        mv, mix, pmv = zip(*[draw_smsa_sample(rng, omega, t, pt) for t, pt in tables])

    moving=None is the path without it, launch for launch."""
    if not _BATCHED or not scans or len(scans) > 64:
        return build_multiscan_batch_per_sample(scans, voxel_size, steps, aug=aug, mix=mix, partners=partners, moving=moving,
                                                partner_moving=partner_moving)
    if moving is not None:
        moving, partner_moving = _moving_records(moving, partner_moving, len(scans))
        steps = MV.pad_steps(steps)
    if mix is not None:
        mix, partners = _mix_records(mix, partners, len(scans))
        return _build_multiscan_batch_mix(scans, partners, mix, voxel_size, steps, aug, moving, partner_moving)
    dev = scans[0]["points"][-1].device
    n_cls = len(steps)
    (hist_pts, hist_lab, hist_ps, lengths, scan_sample, pose0s, poses, rows), current = _walk_scans(scans, steps)
    cur_in = [c[0] for c in current]                   # the resident current scans, with all their columns
    lab_list = [c[1] for c in current]
    moved = None
    if moving is not None:
        cur4, cur_lab_all, *moved = _moved_clouds(scans, moving)[:5]
        n_cur = [int(c.shape[0]) for c in cur_in]
        cur_in, lab_list = list(torch.split(cur4, n_cur)), list(torch.split(cur_lab_all, n_cur))
    else:
        cur4 = torch.cat([c[:, :4] for c in cur_in], 0)
    if aug is not None:
        rec = _aug_records(aug, len(scans))
        n_cur = [int(c.shape[0]) for c in cur_in]
        # the records of the samples, then one per history scan (its sample's): ONE upload for both launches
        rec_dev = torch.from_numpy(np.concatenate([rec, rec[np.asarray(scan_sample, dtype=np.int64)]], 0)).to(dev, non_blocking=True)
        # (cur4 is torch.cat's fresh tensor: the resident scans stay untouched)
        augment_points(cur4, rec_dev[:len(scans)], rows_index32(n_cur, dev), out=cur4)
        cur_in = list(torch.split(cur4, n_cur))        # the single-frame clouds ARE the rows the fused clouds start with
    cur_ms = torch.cat([cur4, torch.ones((cur4.shape[0], 1), dtype=cur4.dtype, device=dev)], 1)      # append_time_flag (:253-257)
    if hist_pts:
        table, sample_of_scan = _step_table("kitti-table", rows, scan_sample, dev)
        scan32 = rows_index32(lengths, dev)
        if moved is not None:
            fused, hl, hps = moved
        else:
            hp = torch.cat(hist_pts, 0).contiguous()
            hl = torch.cat(hist_lab, 0).long()
            hps = hl if all(s.get("pseudo") is None for s in scans) else torch.cat(hist_ps, 0).long()
            fused = B.fuse_scans_batch(hp, scan32, torch.stack(pose0s, 0), torch.stack(poses, 0))
        if aug is not None:
            augment_points(fused, rec_dev[len(scans):], scan32, out=fused)
        hist_ms = torch.cat([fused, torch.zeros((fused.shape[0], 1), dtype=fused.dtype, device=dev)], 1)
    else:
        hist_ms = torch.empty((0, 5), dtype=cur4.dtype, device=dev)
        hl = hps = torch.empty(0, dtype=torch.int64, device=dev)
        scan32 = torch.empty(0, dtype=torch.int32, device=dev)
        table = torch.zeros((1, n_cls + 1), dtype=torch.bool, device=dev)
        sample_of_scan = torch.zeros(1, dtype=torch.int64, device=dev)
    return voxelize_batch_ms(cur_in, lab_list, cur_ms, hist_ms, hl, scan32, hps, table, sample_of_scan,
                             voxel_size, [s.get("name", "") for s in scans], neg_col=n_cls)


def build_tta_batch(scan: Dict, votes_min: int, votes_max: int, rng, voxel_size: float, steps: Sequence[int],
                    scale_range: Sequence[float] = (0.9, 1.1)) -> Dict:
    """The reference's `__getitem__` under `TTA: True` + `collate_batch_tta` (semantickitti_voxel_ms.py:66-72, 102-119, 214-238): the
    scan `votes_max - votes_min` times as batch entries, entry i rotated by TTA_ANGLES[votes_min + i] * pi / 8 and scaled by a draw
    from `rng` (np.random.RandomState; SCALE_AUG_RANGE) - the batch whose eval dictionary `pcseg.eval.accumulate_votes` sums."""
    votes = list(range(votes_min, votes_max))
    aug = [draw_tta_params(rng, v, scale_range) for v in votes]
    return build_multiscan_batch([scan] * len(votes), voxel_size, steps, aug=aug)


class DevicePrefetcher:
    """Double-buffered device-side data stage: the batch of step i+1 (temporal aggregation, voxelisation and
    the model's index plan - everything that does not depend on parameters) is built on a second HIP stream
    while the launch stream still executes step i, the role the reference gives its DataLoader workers
    (tools/train.py builds the loader with workers + pin_memory so batch i+1 is ready when step i ends).

    The stage needs a few host reads (voxel counts, pair totals).  On the launch stream each of them would
    drain the whole queue of step i first; on the side stream they only wait for the stage's own kernels, so
    the host keeps running ahead of the device.

        pf = DevicePrefetcher(make_batch, model.prepare)
        for _ in range(steps):
            batch = pf.next()          # staged earlier; the current stream waits on its ready-event
            ... forward ...
            pf.prefetch_early()        # (optional) stage the following batch beside the backward pass
            ... backward / optimizer step on `batch` ...
            pf.prefetch()              # stage the following batch (optional: next() does it if needed)

    Memory: tensors of a staged batch are allocated on the side stream and consumed on the launch stream, so
    the prefetcher keeps every batch alive until an event recorded on the launch stream after its step has
    completed - nothing is returned to the side stream's pool while a kernel of the launch stream may still
    read it.
    """

    def __init__(self, make_batch, prepare=None, device=None, threaded=False, depth=1):
        self.make_batch, self.prepare = make_batch, prepare
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # depth > 1 (threaded only): that many batches staged ahead, each on a stream and a worker thread of its own - for a loop
        # whose pass is shorter than one stage (evaluation under autocast: the index plan is a chain of ~300 small launches and
        # five host reads, 2.7 ms on its own and ~4.7 ms beside a forward pass)
        self.depth = max(int(depth), 1) if threaded else 1
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.depth)]
        self.stream = self.streams[0]
        self._turn = 0
        self._last_made = None       # depth > 1: batches are MADE one after the other (order, and make_batch need not be thread-safe)
        self._staged = []            # FIFO of (batch, ready_event) or Futures of it
        self._inflight = []          # [(batch, done_event)] handed out, possibly still read by the launch stream
        self._current = None
        # threaded=True runs the stage on a worker thread (its host reads release the GIL while they wait).  With the
        # index plan built natively without the interpreter lock (csrc/fastpath) this takes ~2 ms of host time per step
        # off the training thread: +4 ... 6 % where the step is host-bound (AMP at bs 2), nothing where it is device-bound;
        # bench.py switches it on for --amp (TASEG_STAGE_THREAD overrides).  Same batches, same bits either way.
        self._pool = None
        if threaded:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.depth, thread_name_prefix="taseg-stage")

    def _retire(self):
        if self._current is not None:
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            self._inflight.append((self._current, done))
            self._current = None
        live, dead = [], []
        for item in self._inflight:
            (dead if item[1].query() else live).append(item)
        self._inflight = live
        if dead and self._pool is not None:
            # a staged batch is hundreds of tensors and Python objects: letting go of it costs 0.2-0.3 ms, which the training
            # thread of a host-bound step does not have - the stage's own thread drops the last references
            self._pool.submit(dead.clear)
        del dead

    def prefetch_early(self):
        """Start staging the following batch while the CURRENT one is still in use (call it right after the forward pass has
        been issued): the stage then runs beside the backward pass instead of between two steps - what matters when the
        step is host-bound and the stage runs on a worker thread (`threaded=True`; measured: the AMP step at bs 2 waited
        2.6 ms per step for a stage that was started at the end of the previous step).  The current batch is NOT retired
        here; next() / prefetch() do that."""
        if len(self._staged) >= self.depth:
            return
        self._top_up(not self._inflight and self._current is None)

    def prefetch(self):
        if len(self._staged) >= self.depth:
            return
        self._retire()
        self._top_up(not self._inflight)

    def _top_up(self, idle):
        while len(self._staged) < self.depth:
            stream = self.streams[self._turn % self.depth]
            self._turn += 1
            if idle:
                # first use (or idle device): inputs created on the launch stream must be complete
                stream.wait_stream(torch.cuda.current_stream(self.device))
            if self._pool is None:
                self._staged.append(self._stage(stream))
                continue
            made = None
            if self.depth > 1:
                import threading
                made = threading.Event()
            self._staged.append(self._pool.submit(self._stage, stream, self._last_made, made))
            self._last_made = made

    def _stage(self, stream=None, after=None, made=None):
        stream = self.stream if stream is None else stream
        torch.cuda.set_device(self.device)
        with torch.cuda.stream(stream), torch.no_grad():
            try:
                if after is not None:
                    after.wait()             # the batch before this one has been taken from the source
                batch = self.make_batch()
            finally:
                if made is not None:
                    made.set()
            if self.prepare is not None:
                self.prepare(batch)
            ready = torch.cuda.Event()
            ready.record(stream)
        return batch, ready

    def next(self):
        self._retire()               # the previous batch: every launch that reads it has been issued by now
        self.prefetch()
        staged = self._staged.pop(0)
        batch, ready = staged.result() if hasattr(staged, "result") else staged
        torch.cuda.current_stream(self.device).wait_event(ready)
        self._current = batch
        return batch

    def close(self):
        for staged in self._staged:
            if hasattr(staged, "result"):
                try:
                    staged.result()
                except Exception:  # noqa: BLE001 - a stage that failed has nothing left to wait for; next() reports failures
                    pass
        self._retire()
        torch.cuda.synchronize(self.device)
        self._inflight, self._staged = [], []
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
