"""nuScenes multi-scan (FSA) data stage - the temporal aggregation of R/pcseg/data/dataset/nuscenes/nuscenes_ms.py:226-373
and the voxelisation of nuscenes_voxel_ms.py:77-187 on resident sweeps.

Split between host and device the way the work splits:

  host (numpy, a few dozen 3x3 products per sample, results cached per keyframe like the reference's
  `token2samplelist`):
      rotation_matrix      `Quaternion(q).rotation_matrix` of pyquaternion (nuscenes-devkit's quaternion class)
      relative_transform   (R, T) of transform_point (:348-373): lidar frame of `info` -> lidar frame of `info0`
      select_sweeps        which sweeps of the scene to aggregate (:238-276): nearest frame to every multiple of
                           STEP metres of driven distance up to MULTISCAN, plus every keyframe on the way
      sweep_params         per selected sweep the 28 doubles ts_fuse_sweeps consumes
  device (one launch per sample over all selected sweeps):
      ts_fuse_sweeps       ego-box filter on the raw coordinates, sensor -> keyframe -> current-frame transforms in
                           float64 with numpy's rounding points, time delta column
      class-step mask      table lookup on the pseudo labels, one _nusc_row per selected sweep (:322-327)
      scan mixing (mix=)   ts_stage_mix on the single-frame pair and on the fused pair of every sample and its partner keyframe
                           (nuscenes_ms.py:132-214, data/mix.py), before the augmentation; then the clamp of every fused row as one
                           stable compaction (ts_stage_clamp_compact, csrc/compact.hip) - stage._mix_and_voxelize, the tail shared
                           with SemanticKITTI
      augmentation (aug=)  ts_stage_augment on the current keyframes and on every fused sweep row (nuscenes_voxel_ms.py:90-120,
                           data/augment.py), before the clamp and both voxelisations
      voxelisation         the same ts_voxel_coords / ts_sparse_quantize stage as SemanticKITTI (voxel 0.1 m,
                           IN_FEATURE_DIM 4: the time delta column is cut, nuscenes fsa yaml:16,28)

A sequence is described by plain arrays (`NuscSequence`), not by devkit objects: the reference reads these numbers out
of its info pickles (mmdet3d layout) - file IO and the devkit are out of scope, the arithmetic on them is not.
Bit-exact against the reference's dataset code: tests/golden/multiscan_nus.npz.
"""
from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np
import torch

from .. import backend as B
from . import stage as _stage          # (_stage._BATCHED is read at call time)
from . import mix as M
from .augment import augment_points, draw_tta_params
from .stage import (_aug_records, _cached, _mix_and_voxelize, _mix_records, _step_keep, _step_table, collate_batch, rows_index32,
                    voxelize_batch_ms, voxelize_sample_ms)

__all__ = ["NuscSequence", "rotation_matrix", "relative_transform", "select_sweeps", "sweep_params", "fuse_sweeps",
           "build_nuscenes_batch", "build_nuscenes_batch_per_sample", "build_tta_batch"]


@dataclass
class NuscSequence:
    """Frames (keyframes and the sweeps between them) of one or more scenes in time order.

    per frame g:  is_key [F] bool, key_index [F] (row of the key_* arrays or -1), timestamps [F] int64 microseconds,
                  scene_tokens [F], local_indexes [F] (the keyframe whose lidar frame sensor2lidar_* maps into: the
                  next keyframe at or after g), s2l_r [F,3,3] / s2l_t [F,3] float64 (sweeps only)
    per keyframe: global_indexes [K] (its frame number), l2e_q / e2g_q [K,4] (w,x,y,z), l2e_t / e2g_t [K,3]"""
    is_key: np.ndarray
    key_index: np.ndarray
    timestamps: np.ndarray
    scene_tokens: Sequence
    local_indexes: np.ndarray
    s2l_r: np.ndarray
    s2l_t: np.ndarray
    global_indexes: np.ndarray
    l2e_q: np.ndarray
    l2e_t: np.ndarray
    e2g_q: np.ndarray
    e2g_t: np.ndarray


def rotation_matrix(q) -> np.ndarray:
    """pyquaternion's Quaternion(q).rotation_matrix (q = w, x, y, z; normalised unless unit to 1e-14): the lower-right
    3x3 of Q(q) Qbar(q)^T."""
    q = np.array(q, dtype=np.float64)
    n2 = float(q @ q)
    if abs(1.0 - n2) >= 1e-14 and n2 > 0:
        q = q / np.sqrt(n2)
    w, x, y, z = q
    left = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    right = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return (left @ right.T)[1:, 1:]


def relative_transform(seq: NuscSequence, key0: int, key: int):
    """(R [3,3], T [3]) float64 with p_in_frame(key0) = p_in_frame(key) @ R + T (nuscenes_ms.py:348-373)."""
    l2e0, e2g0 = rotation_matrix(seq.l2e_q[key0]), rotation_matrix(seq.e2g_q[key0])
    l2e, e2g = rotation_matrix(seq.l2e_q[key]), rotation_matrix(seq.e2g_q[key])
    back = np.linalg.inv(e2g0).T @ np.linalg.inv(l2e0).T
    rot = (l2e.T @ e2g.T) @ back
    trans = (seq.l2e_t[key] @ e2g.T + seq.e2g_t[key]) @ back
    trans -= seq.e2g_t[key0] @ back + seq.l2e_t[key0] @ np.linalg.inv(l2e0).T
    return rot, trans


def select_sweeps(seq: NuscSequence, index: int, multiscan: int, step: float) -> List[int]:
    """Frame offsets (negative, ascending = oldest first) aggregated into keyframe `index` (nuscenes_ms.py:238-276)."""
    g0 = int(seq.global_indexes[index])
    offsets, dist, delta = [], [], 0
    while not dist or dist[-1] <= multiscan * step:
        delta -= 1
        g = g0 + delta                  # a negative g indexes from the end, as the reference's list does
        if seq.scene_tokens[g] != seq.scene_tokens[g0]:
            dist.append(1000)
            break
        origin = np.zeros((1, 3))
        if not seq.is_key[g]:
            origin = origin @ seq.s2l_r[g].T + seq.s2l_t[g]          # the sweep's sensor origin in its keyframe's frame
        father = int(seq.local_indexes[g])
        if father != index:
            rot, trans = relative_transform(seq, index, father)
            origin = origin @ rot + trans
        offsets.append(delta)
        dist.append(float(np.linalg.norm(origin.reshape(-1)[:2], ord=2)))
    picked, cur = [], 1
    for i in range(len(offsets)):
        if dist[i] - cur * step > 0 or (dist[i] < dist[i + 1] and abs(dist[i] - cur * step) < abs(dist[i + 1] - cur * step)):
            picked.append(offsets[i])
            cur += 1
        if cur > multiscan:
            break
    picked += [d for d in offsets if seq.is_key[g0 + d]]            # every keyframe on the way (:270-272)
    return sorted(set(picked))


def sweep_params(seq: NuscSequence, index: int, offsets: Sequence[int]) -> np.ndarray:
    """[S, 28] float64 for ts_fuse_sweeps: {A[9], a[3], flagA, B[9], b[3], flagB, dt, 0} per selected sweep."""
    g0 = int(seq.global_indexes[index])
    out = np.zeros((len(offsets), 28), dtype=np.float64)
    for i, d in enumerate(offsets):
        g = g0 + d
        if seq.is_key[g]:
            rot, trans = relative_transform(seq, index, int(seq.key_index[g]))
            out[i, 13:22], out[i, 22:25], out[i, 25] = rot.reshape(-1), trans, 1.0
        else:
            out[i, 0:9], out[i, 9:12], out[i, 12] = np.asarray(seq.s2l_r[g]).reshape(-1), seq.s2l_t[g], 1.0
            father = int(seq.local_indexes[g])
            if father != index:
                rot, trans = relative_transform(seq, index, father)
                out[i, 13:22], out[i, 22:25], out[i, 25] = rot.reshape(-1), trans, 1.0
        out[i, 26] = seq.timestamps[g0] / 1e6 - seq.timestamps[g] / 1e6
    return out


def _nusc_row(pos: int, steps: Sequence[int]) -> List[bool]:
    """The nuScenes class-step rule (nuscenes_ms.py:320-328) for the selected sweep at position `pos` (0 = oldest): class c is kept
    iff steps[c] != 0 and (pos + 1) % steps[c] == 0."""
    return [bool(st) and (pos + 1) % st == 0 for st in steps]


def _current_keyframe(points, in_feature_dim=None):
    """The current keyframe as both clouds hold it: a fresh tensor with the time column 0 (nuscenes_ms.py:109), cut to the first
    `in_feature_dim` columns if given.  points: one keyframe [n, 5], or a list of them (concatenated)."""
    cur = torch.cat(points, 0) if isinstance(points, (list, tuple)) else points.clone()
    cur[:, 4] = 0
    return cur if in_feature_dim is None else cur[:, :in_feature_dim].contiguous()


def _layout(lengths, steps, device):
    """per-layout helpers of one sample, cached (stage._cached): sweep index (int32) of every concatenated sweep point and the
    [S, C] table of _nusc_row per sweep"""
    def make():
        idx = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int32), torch.tensor(list(lengths))).to(device)
        return idx, torch.tensor([_nusc_row(pos, steps) for pos in range(len(lengths))], dtype=torch.bool, device=device)
    return _cached(("nusc-layout", tuple(lengths), tuple(steps), str(device)), make)


def fuse_sweeps(cur_pts, cur_lab, hist_pts: List[torch.Tensor], hist_lab: List[torch.Tensor],
                hist_pseudo: List[torch.Tensor], params: torch.Tensor, steps: Sequence[int]):
    """Current keyframe + selected sweeps -> the un-filtered stack (raw [n, 5] = x, y, z, intensity, time delta; labels
    [n]; keep [n]).  `raw[keep]` is the reference's `xyzret_ms` (nuscenes_ms.py:125-127): current scan first (time
    column 0, :109), then the sweeps oldest first, each without its ego-box points and filtered by the class-step rule.
    hist_lab[i]: mapped labels of a keyframe, zeros for a sweep (:297, :318); hist_pseudo[i]: pseudo labels (:323)."""
    dev = cur_pts.device
    cur = _current_keyframe(cur_pts)
    n_cur = cur.shape[0]
    if not hist_pts:
        return cur, cur_lab.long(), torch.ones(n_cur, dtype=torch.bool, device=dev)
    sweep_idx, table = _layout([p.shape[0] for p in hist_pts], steps, dev)
    fused, no_ego = B.fuse_sweeps(torch.cat(hist_pts, 0).contiguous(), sweep_idx, params)
    keep = no_ego & _step_keep(table, sweep_idx, torch.cat(hist_pseudo, 0).long())
    raw = torch.cat([cur, fused], 0)
    lab = torch.cat([cur_lab.long(), torch.cat(hist_lab, 0).long()])
    return raw, lab, torch.cat([torch.ones(n_cur, dtype=torch.bool, device=dev), keep])


def _used_mix(mix, partners, n_samples):
    """mix= / partners= of a batch, checked (stage._mix_records); None where no record mixes: that batch takes the path without"""
    if mix is None:
        return None, None
    mix, partners = _mix_records(mix, partners, n_samples)
    if all(p.kind == M.NONE for p in mix):
        return None, None
    return mix, partners


def _walk_sweeps(clouds: List[Dict], steps: Sequence[int]):
    """One pass over sample dicts (build_nuscenes_batch's `samples[b]`), the counterpart of stage._walk_scans.  Returns the selected
    sweeps of all of them, flat and in order: (points, labels, pseudo labels, lengths, owner = index of the dict in `clouds`,
    _nusc_row by the sweep's position in ITS cloud, the [S, 28] params of every cloud that has sweeps)."""
    pts, lab, pseudo, lengths, owner, rows, params = walk = [], [], [], [], [], [], []
    for b, c in enumerate(clouds):
        for pos, p in enumerate(c["hist_points"]):
            pts.append(p)
            lengths.append(int(p.shape[0]))
            owner.append(b)
            rows.append(_nusc_row(pos, steps))
        lab += list(c["hist_labels"])
        pseudo += list(c["hist_pseudo"])
        if len(c["hist_points"]):
            params.append(c["params"])
    return walk


def _fuse_walk(walk, n_cls, in_feature_dim, device):
    """The sweeps of _walk_sweeps in ONE ts_fuse_sweeps launch -> (fused rows cut to `in_feature_dim` columns (a view), labels
    int64, pseudo labels int64, sweep index int32, no_ego bool, class-step table [S, C], owner of every sweep on the device - the
    cached pair of stage._step_table, keyed by rows AND owners); without sweeps the row tensors are empty and the table is one
    row of zeros"""
    pts, lab, pseudo, lengths, owner, rows, params = walk
    if not pts:
        none = torch.empty(0, dtype=torch.int64, device=device)
        return (torch.empty((0, in_feature_dim), dtype=torch.float32, device=device), none, none,
                torch.empty(0, dtype=torch.int32, device=device), torch.empty(0, dtype=torch.bool, device=device),
                torch.zeros((1, n_cls), dtype=torch.bool, device=device), torch.zeros(1, dtype=torch.int64, device=device))
    stack = torch.cat(pts, 0).contiguous()
    pseudo = torch.cat(pseudo, 0).long()
    lab = torch.cat(lab, 0).long()
    sweep32 = rows_index32(lengths, device)
    table, owner_dev = _step_table("nusc-table", rows, owner, device)
    fused, no_ego = B.fuse_sweeps(stack, sweep32, torch.cat(params, 0) if len(params) > 1 else params[0])
    return fused[:, :in_feature_dim], lab, pseudo, sweep32, no_ego, table, owner_dev


def _build_nuscenes_batch_mix(samples, partners, mix, voxel_size, steps, in_feature_dim, aug) -> Dict:
    """build_nuscenes_batch with mix=: the sweeps of every sample and of every partner that is used in ONE ts_fuse_sweeps launch
    (_walk_sweeps, _fuse_walk); the ego box AND the class-step rule as the keep byte of the fused mix; then the tail both datasets
    share, stage._mix_and_voxelize: two host reads before the voxelisation.  The mix works on the first `in_feature_dim` columns of
    the 5-column rows: the sample's keyframe with column 4 set to 0, the partner's as the file holds it, the sweep rows of both
    with their time lag (see build_nuscenes_batch)."""
    dev, f = samples[0]["points"].device, in_feature_dim
    # the clouds that take part, in order: every sample's own, then its partner's where its mix moves rows of one
    used = [[s, partners[b] if mix[b].kind != M.NONE else None] for b, s in enumerate(samples)]
    walk = _walk_sweeps([c for pair in used for c in pair if c is not None], steps)
    fused, lab_h, pseudo, sweep32, no_ego, table, _ = _fuse_walk(walk, len(steps), f, dev)
    hkeep = no_ego & _step_keep(table, sweep32, pseudo)
    heads, first = [], 0
    for pair in used:
        for k, c in enumerate(pair):
            if c is None:
                continue
            # column 4: 0 on the sample's keyframe (nuscenes_ms.py:109), the file's on the partner's (:136-141)
            key = _current_keyframe(c["points"], f) if k == 0 else c["points"][:, :f]
            nh = sum(int(p.shape[0]) for p in c["hist_points"])
            heads.append((key, c["labels"].reshape(-1).long(), first, nh))
            first += nh
    return _mix_and_voxelize(used, heads, fused, lab_h, hkeep, mix, aug, voxel_size)


def build_nuscenes_batch(samples: List[Dict], voxel_size: float, steps: Sequence[int], in_feature_dim: int = 4, aug=None, mix=None,
                         partners=None) -> Dict:
    """samples[b] = dict(points [n,5], labels [n], hist_points [..], hist_labels [..], hist_pseudo [..],
    params [S,28] float64 tensor, name).  Returns the collated batch_dict MinkUNetMs consumes
    (nuscenes_voxel_ms.py:77-212 == the SemanticKITTI stage on the first `in_feature_dim` columns).
    The whole batch goes through ONE chain of launches: one ts_fuse_sweeps over every sweep point of every sample of _walk_sweeps
    (_fuse_walk: ego box, sensor -> keyframe -> current-frame transforms, time delta), the class-step rule (_nusc_row,
    stage._step_table) as one table lookup, then stage.voxelize_batch_ms (one compaction, one batch-keyed voxelisation per cloud kind).
    aug: one AugParams per sample (data/augment.py) or None = the un-augmented path.  With it the current keyframes and all fused sweep
    rows are augmented in place (one ts_stage_augment launch each, the sweep rows through their sweep index) before the clamp.
    mix: one MixParams per sample (data/mix.py, `draw_mix_params(rng, omega, dataset="nuscenes", n_partners=len(reader))`) or None;
    partners[b]: the sample dict of sample b's partner keyframe - what `NuscInfoReader.sample(p.partner, ...)` returns - or None
    where its record needs none.  With it every sample is mixed with its partner - PolarMix / LaserMix on the single-frame pair and
    on the fused pair, nuscenes_ms.py:132-214 - before the augmentation (_build_nuscenes_batch_mix).  mix=None, and a list whose
    records are all NONE, is the path without it, launch for launch and bit for bit.  What the reference does there is reproduced,
    not repaired:
      * column 4 (:109, :136-141): the sample's keyframe has column 4 set to 0; the partner's keyframe keeps column 4 as the file
        holds it (the ring index), alone and as the head of its fused cloud; the sweep rows of both carry the time lag.  The mix
        runs on the first `in_feature_dim` columns of these 5-column rows: nothing of it shows with 4, all of it with 5;
      * the rotated copies of PolarMix_nuscenes.py:53 carry column 3 only, zeros behind it (`tail_all=False`);
      * a sample or a partner without history (the first keyframe of its scene: `hist_points == []`, :122-131, :151-159) has its
        fused cloud equal to its keyframe;
      * the partner is drawn with `choice(len(infos))` (:133) and may be the sample itself;
      * the recipe's LaserMix branch calls `lasermix_aug` (:161), the identity, and still consumes its strategy draw;
      * nothing mixes outside training: `draw_mix_params(training=False)` returns NONE."""
    mix, partners = _used_mix(mix, partners, len(samples))
    if not _stage._BATCHED or not samples or len(samples) > 64:
        return build_nuscenes_batch_per_sample(samples, voxel_size, steps, in_feature_dim, aug=aug, mix=mix, partners=partners)
    if mix is not None:
        return _build_nuscenes_batch_mix(samples, partners, mix, voxel_size, steps, in_feature_dim, aug)
    dev = samples[0]["points"].device
    f = in_feature_dim
    cur_f = _current_keyframe([s["points"] for s in samples], f)     # (one fresh tensor: the resident scans stay untouched)
    n_cur = [int(s["points"].shape[0]) for s in samples]
    rec = None if aug is None else _aug_records(aug, len(samples))
    if rec is not None:
        augment_points(cur_f, rec, rows_index32(n_cur, dev), out=cur_f)
    cur_list = list(torch.split(cur_f, n_cur))
    lab_list = [s["labels"].long() for s in samples]
    walk = _walk_sweeps(samples, steps)
    hist_ms, lab_h, pseudo, sweep32, no_ego, table, sample_of = _fuse_walk(walk, len(steps), f, dev)
    hist_ms = hist_ms.contiguous()
    if rec is not None and walk[0]:
        augment_points(hist_ms, rec[np.asarray(walk[4], dtype=np.int64)], sweep32, out=hist_ms)
    return voxelize_batch_ms(cur_list, lab_list, cur_f, hist_ms, lab_h, sweep32, pseudo, table, sample_of, voxel_size,
                             [s.get("name", "") for s in samples], pre_keep=no_ego)


def _partner_clouds(s, steps, in_feature_dim):
    """(keyframe, labels, fused cloud, its labels) of a mix partner, on `in_feature_dim` columns: as the sample's, but column 4 of
    the keyframe stays what the file holds (nuscenes_ms.py:136-141, :155)"""
    raw, lab, keep = fuse_sweeps(s["points"], s["labels"], s["hist_points"], s["hist_labels"], s["hist_pseudo"], s["params"], steps)
    n = s["points"].shape[0]
    raw[:n, 4] = s["points"][:, 4]                     # (fuse_sweeps hands out a fresh tensor)
    return s["points"][:, :in_feature_dim].contiguous(), s["labels"].reshape(-1).long(), raw[keep][:, :in_feature_dim].contiguous(), lab[keep]


def build_nuscenes_batch_per_sample(samples: List[Dict], voxel_size: float, steps: Sequence[int], in_feature_dim: int = 4,
                                    aug=None, mix=None, partners=None) -> Dict:
    """build_nuscenes_batch sample by sample (the form the batched stage replaced; its cross-check and TASEG_STAGE_BATCHED=0).
    mix= / partners= as there: `mix_points` on the single-frame pair and on the fused pair of every sample that is mixed (three
    launches and a host read each), then voxelize_sample_ms; the same reproduced-not-repaired points hold."""
    out = []
    rec = None if aug is None else _aug_records(aug, len(samples))
    mix, partners = _used_mix(mix, partners, len(samples))
    f = in_feature_dim
    for b, s in enumerate(samples):
        one = None if rec is None else rec[b:b + 1]
        raw, lab, keep = fuse_sweeps(s["points"], s["labels"], s["hist_points"], s["hist_labels"], s["hist_pseudo"],
                                     s["params"], steps)
        cur, cur_lab = _current_keyframe(s["points"], f), s["labels"].reshape(-1).long()
        if mix is None or mix[b].kind == M.NONE:
            out.append(voxelize_sample_ms(cur, cur_lab, raw[:, :f].contiguous(), lab, voxel_size, s.get("name", ""), keep=keep, aug=one))
            continue
        raw, lab = raw[keep][:, :f].contiguous(), lab[keep]
        if partners[b] is None:
            pcur, plab, praw, plab_ms = cur[:0], cur_lab[:0], raw[:0], lab[:0]
        else:
            pcur, plab, praw, plab_ms = _partner_clouds(partners[b], steps, f)
        # the same record on the single-frame pair and on the fused pair (nuscenes_ms.py:161-164, :198-211)
        cur, cur_lab = M.mix_points(cur, cur_lab, pcur, plab, mix[b])
        raw, lab = M.mix_points(raw, lab, praw, plab_ms, mix[b])
        out.append(voxelize_sample_ms(cur, cur_lab, raw, lab, voxel_size, s.get("name", ""), aug=one))
    return collate_batch(out)


def build_tta_batch(sample: Dict, votes_min: int, votes_max: int, rng, voxel_size: float, steps: Sequence[int],
                    in_feature_dim: int = 4, scale_range: Sequence[float] = (0.9, 1.1)) -> Dict:
    """nuscenes_voxel_ms.py:67-73, 103-120 + collate_batch_tta: the keyframe `votes_max - votes_min` times as batch entries, entry i
    rotated by TTA_ANGLES[votes_min + i] * pi / 8 and scaled by a draw from `rng` (see stage.build_tta_batch)."""
    votes = list(range(votes_min, votes_max))
    aug = [draw_tta_params(rng, v, scale_range) for v in votes]
    return build_nuscenes_batch([sample] * len(votes), voxel_size, steps, in_feature_dim, aug=aug)
