"""Device-resident data stage of the mask-distillation recipe (minkunet_mk34_cr10_fsa_kd.yaml, dataset `semantickitti_ms_kd`): three
clouds per sample.

The reference (R/pcseg/data/dataset/semantickitti/semantickitti_ms_kd.py:121-358, semantickitti_voxel_ms_kd.py:77-245,
tools/utils/common/seg_utils.py:168-239) produces

  point         the current scan
  point_ms      the student's cloud: current scan + the pose-fused history filtered by the PSEUDO labels under FLEXIBLE_STEPS
  point_ms_gt   the teacher's cloud: current scan + the SAME fused history filtered by the ANNOTATIONS under FLEXIBLE_STEPS_GT

mixes all three with one set of PolarMix / LaserMix flags, augments all three with one draw (`aug_points_ms_gt`), clamps both fused
clouds to the single-frame minimum, voxelises all three with ONE coordinate shift (the student cloud's minimum) and collates them
with `offset_ms_gt` / `num_points_ms_gt`.  `build_kd_batch` does the same on resident scans:

  mix=None   one walk over the scans, one pose-fuse launch, (aug=: the two ts_stage_augment launches of build_multiscan_batch),
             ts_segment_min3, ts_stage_layout_pair - both fused clouds from ONE pass over the history (csrc/kd_stage.hip), its
             counts the one host read before the voxelisation; _layout_sequence, the launches it replaces, is kept as its
             baseline and cross-check behind _PAIR_KERNEL -, the two voxelisations of build_multiscan_batch and one more for the
             teacher with the student's shift
  mix=       ts_stage_mix on the single-frame pairs and on 2 B fused jobs (B student pairs, then B teacher pairs), one host read
             of all totals, ts_stage_augment with the records repeated, ts_stage_clamp_compact with the minima repeated (second
             host read), the three voxelisations

Reproduced, not repaired: the head of the PARTNER's teacher cloud is the SAMPLE's current scan when the partner has history
(semantickitti_ms_kd.py:178, :220) and the partner's own scan when it has none (:186, :228), the time flag following that head;
the teacher's labels are all 0, so PolarMix never pastes an instance row into it; LaserMix is the identity; `num_points_ms_gt` is the
row count BEFORE the clamp (semantickitti_voxel_ms_kd.py:88); `point_mask` is "the first num_points rows".
"""
from itertools import accumulate
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import backend as B
from ..torchsparse import SparseTensor
from . import mix as M
from . import stage as S
from .augment import augment_points

__all__ = ["build_kd_batch"]

# The one switch between the two ways to lay the fused clouds out (mix=None): ts_stage_layout_pair, or the launches it replaces
# (_layout_sequence, written as lean as they go).  Measured at the KD benchmark line's stage shape (tools/time_kd_stage.py,
# profiles/kd_stage.txt) the kernel is ahead by far more than the spread of the repetitions, so it is the stage's path; the tool and
# the tests clear this to run the sequence as its baseline and cross-check.  Same tensors either way.
_PAIR_KERNEL = True


def _layout_sequence(cur, cur_lab, cur_b, cur_start, hist, hist_lab, scan32, cls_a, cls_b, table_a, table_b, sample_of_scan, lo,
                     neg_col):
    """backend.stage_layout_pair's outputs by ts_stage_keep_flags -> nonzero (a host read) -> searchsorted -> ts_stage_layout once
    per cloud, on the four-column rows; the time flag is appended to the rows that are KEPT (the is-current byte as a column).
    The teacher's rows before the clamp: one more ts_stage_keep_flags launch against a minimum of -inf, an int32 running sum of
    its bytes, read at the sample edges."""
    dev, nb = cur.device, lo.shape[0]
    cur4 = cur[:, :4].contiguous()
    edges = torch.arange(nb + 1, device=dev)
    out, kept = [], []
    for cls, table in ((cls_a, table_a), (cls_b, table_b)):
        keep, hist_b = B.stage_keep_flags(hist, scan32, cls, table, sample_of_scan, lo, neg_col=neg_col)
        idx = keep.nonzero().squeeze(1)
        kept_start = torch.searchsorted(hist_b[idx], edges)
        pts, lab, b, b32, is_cur = B.stage_layout(cur4, cur_lab, cur_b, hist, hist_lab, hist_b, idx, cur_start, kept_start)
        out.append((torch.cat([pts, is_cur.to(pts.dtype).unsqueeze(1)], 1), lab, b, b32, is_cur))
        kept.append(kept_start[1:] - kept_start[:-1])
    step, _ = B.stage_keep_flags(hist, scan32, cls_b, table_b, sample_of_scan, torch.full_like(lo, float("-inf")), neg_col=neg_col)
    run = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), torch.cumsum(step, 0, dtype=torch.int32)])
    at = run[torch.searchsorted(hist_b, edges)].long()
    kept.append(at[1:] - at[:-1])
    (pa, la, ba, ba32, ia), (pb, _, bb, bb32, _) = out
    return (pa, la, ba, ba32, ia), (pb, bb, bb32), torch.stack(kept, 1)


def _canon_columns(clouds: List[Dict]) -> List[torch.Tensor]:
    """the teacher's class column of every history scan of `clouds`, flat and in _walk_scans' order: `canon[i]` - the class whose
    canonical raw id the ANNOTATION of history scan i is, or -1 (the reference compares `raw & 0xFFFF` with LEARNING_MAP_INV[c] for
    the gt mask too, semantickitti_ms_kd.py:339-344) -, else the labels, as `pseudo` defaults"""
    out = []
    for c in clouds:
        canon = c.get("canon")
        t = len(c["points"]) - 1
        if canon is not None and len(canon) != t:
            raise ValueError("canon must hold one tensor per history scan")
        out += [c["labels"][i] if canon is None else canon[i] for i in range(t)]
    return out


def _teacher_voxels(batch: Dict, shift, gt_pts, gt_b, gt_b32, n_gt: Sequence[int], voxel_size: float, nb: int) -> Dict:
    """the third voxelisation (semantickitti_voxel_ms_kd.py:136-137, :181-195): the teacher's rows rounded and shifted by the
    STUDENT cloud's minimum (`shift`, what _voxelize_layout took), one representative per voxel"""
    coords, _ = B.voxel_coords(gt_pts, voxel_size, batch_idx=gt_b32, n_batch=nb, shift=shift)
    index, inverse = B.sparse_quantize(coords)                         # host read (voxels of the teacher's clouds)
    vox, offset, _ = B.stage_split_voxels(coords, index, inverse, gt_b, nb)
    batch["lidar_ms_gt"] = SparseTensor(gt_pts[index.long()], vox)
    batch["offset_ms_gt"] = offset
    batch["num_points_ms_gt"] = torch.tensor(list(n_gt)).view(-1, 1)
    return batch


def _build_plain(scans, voxel_size, steps, steps_gt, aug) -> Dict:
    dev, nb, n_cls = scans[0]["points"][-1].device, len(scans), len(steps)
    (hist_pts, hist_lab, hist_ps, lengths, scan_sample, pose0s, poses, rows), current = S._walk_scans(scans, steps)
    rows_gt = [S._kitti_row(d, steps_gt) for s in scans for d in S._deltas(s)]
    cur_in, lab_list = [c[0] for c in current], [c[1] for c in current]
    n_cur = [int(c.shape[0]) for c in cur_in]
    if aug is not None:
        rec = S._aug_records(aug, nb)
        rec_dev = torch.from_numpy(np.concatenate([rec, rec[np.asarray(scan_sample, dtype=np.int64)]], 0)).to(dev, non_blocking=True)
        cur = torch.cat([c[:, :4] for c in cur_in], 0)     # (torch.cat's fresh tensor: the resident scans stay untouched)
        augment_points(cur, rec_dev[:nb], S.rows_index32(n_cur, dev), out=cur)
    else:
        cur = torch.cat(cur_in, 0).contiguous()            # the resident scans, with all their columns
    cur_lab = torch.cat(lab_list, 0)
    cur_b = S.rows_index(n_cur, dev)
    if hist_pts:
        table, sample_of_scan = S._step_table("kitti-table", rows, scan_sample, dev)
        table_gt, _ = S._step_table("kitti-table", rows_gt, scan_sample, dev)
        scan32 = S.rows_index32(lengths, dev)
        hl = torch.cat(hist_lab, 0).long()
        hps = hl if all(s.get("pseudo") is None for s in scans) else torch.cat(hist_ps, 0).long()
        hgt = hl if all(s.get("canon") is None for s in scans) else torch.cat(_canon_columns(scans), 0).long()
        fused = B.fuse_scans_batch(torch.cat(hist_pts, 0).contiguous(), scan32, torch.stack(pose0s, 0), torch.stack(poses, 0))
        if aug is not None:
            augment_points(fused, rec_dev[nb:], scan32, out=fused)
    else:
        table = table_gt = torch.zeros((1, n_cls + 1), dtype=torch.bool, device=dev)
        sample_of_scan = torch.zeros(1, dtype=torch.int64, device=dev)
        scan32 = torch.empty(0, dtype=torch.int32, device=dev)
        hl = hps = hgt = torch.empty(0, dtype=torch.int64, device=dev)
        fused = torch.empty((0, 4), dtype=torch.float32, device=dev)
    lo = B.segment_min3(cur, cur_b, nb)            # minimum of every current scan: both fused clouds are clamped to it
    n_c = cur.shape[0]
    cur_start = S._cached(("kd-cur-start", tuple(n_cur), str(dev)),
                          lambda: torch.tensor(list(accumulate(n_cur, initial=0)), dtype=torch.int64).to(dev))
    if _PAIR_KERNEL:
        (ms, ms_lab, ms_b, ms_b32, point_mask), (gt, gt_b, gt_b32), counts = B.stage_layout_pair(
            cur, cur_lab, cur_start, fused, hl, scan32, hps, hgt, table, table_gt, sample_of_scan, lo, neg_col=n_cls)
    else:
        (ms, ms_lab, ms_b, ms_b32, point_mask), (gt, gt_b, gt_b32), counts = _layout_sequence(
            cur, cur_lab, cur_b, cur_start, fused, hl, scan32, hps, hgt, table, table_gt, sample_of_scan, lo, n_cls)
    kept, kept_gt, step_gt = (list(col) for col in zip(*counts.tolist()))          # the host read (rows of both clouds per sample)
    n_ms = [a + k for a, k in zip(n_cur, kept)]
    n_a, n_b = n_c + sum(kept), n_c + sum(kept_gt)
    batch, shift = S._voxelize_layout(cur, cur_lab, cur_b, n_cur, ms[:n_a], ms_lab[:n_a], ms_b[:n_a], ms_b32[:n_a], n_ms,
                                      point_mask[:n_a], voxel_size, [s.get("name", "") for s in scans], return_shift=True)
    return _teacher_voxels(batch, shift, gt[:n_b], gt_b[:n_b], gt_b32[:n_b], [a + k for a, k in zip(n_cur, step_gt)], voxel_size, nb)


def _build_mix(scans, partners, mix, voxel_size, steps, steps_gt, aug) -> Dict:
    """build_kd_batch with mix=: _build_multiscan_batch_mix and _mix_and_voxelize (data/stage.py) with the teacher's jobs appended
    to the student's"""
    dev, nb = scans[0]["points"][-1].device, len(scans)
    used = [[s, partners[b] if mix[b].kind != M.NONE else None] for b, s in enumerate(scans)]
    clouds = [c for pair in used for c in pair if c is not None]
    (hist_pts, hist_lab, hist_ps, lengths, owner, pose0s, poses, rows), current = S._walk_scans(clouds, steps)
    rows_gt = [S._kitti_row(d, steps_gt) for c in clouds for d in S._deltas(c)]
    if hist_pts:
        scan32 = S.rows_index32(lengths, dev)
        hl = torch.cat(hist_lab, 0).long()
        hps = hl if all(c.get("pseudo") is None for c in clouds) else torch.cat(hist_ps, 0).long()
        hgt = hl if all(c.get("canon") is None for c in clouds) else torch.cat(_canon_columns(clouds), 0).long()
        fused = B.fuse_scans_batch(torch.cat(hist_pts, 0).contiguous(), scan32, torch.stack(pose0s, 0), torch.stack(poses, 0))
        keep = S._step_keep(S._step_table("kitti-table", rows, owner, dev)[0], scan32, hps, neg_last=True)
        keep_gt = S._step_keep(S._step_table("kitti-table", rows_gt, owner, dev)[0], scan32, hgt, neg_last=True)
    else:
        fused = torch.empty((0, 4), dtype=torch.float32, device=dev)
        hl = torch.empty(0, dtype=torch.int64, device=dev)
        keep = keep_gt = torch.empty(0, dtype=torch.bool, device=dev)
    heads = [(scan[:, :4], lab, first, nh) for scan, lab, first, nh in current]
    ones = torch.ones(max(int(h[0].shape[0]) for h in heads), dtype=torch.bool, device=dev)
    # job-major rows: [head | partner's head] for the single-frame mix; [head | history | partner's head | partner's history] for
    # a student job, with the pseudo rule's keep bytes; the same pieces for a teacher job with the annotation rule's keep bytes -
    # but the head in front of a partner's history is the SAMPLE's (semantickitti_ms_kd.py:178, :220)
    s_pts, s_lab, s_n = [], [], ([], [])
    m_pts, m_lab, m_keep, m_len, m_n = [], [], [], [], ([], [])
    g_pts, g_keep, g_len, g_n = [], [], [], ([], [])
    it = iter(heads)
    for pair in used:
        own = None
        for k, c in enumerate(pair):
            n = nh = ng = 0
            if c is not None:
                head, lab, first, nh = next(it)
                own = head if own is None else own
                n = int(head.shape[0])
                s_pts.append(head)
                s_lab.append(lab)
                m_pts += [head, fused[first:first + nh]]
                m_lab += [lab, hl[first:first + nh]]
                m_keep += [ones[:n], keep[first:first + nh]]
                ghead = own if len(c["points"]) > 1 else head
                ng = int(ghead.shape[0])
                g_pts += [ghead, fused[first:first + nh]]
                g_keep += [ones[:ng], keep_gt[first:first + nh]]
            m_len += [n, nh]
            g_len += [ng, nh]
            s_n[k].append(n)
            m_n[k].append(n + nh)
            g_n[k].append(ng + nh)
    n_student = sum(m_len)
    ms_in = torch.cat(m_pts + g_pts, 0)
    flag = (S.rows_index(m_len + g_len, dev) % 2 == 0).to(torch.float32)      # append_time_flag (:280-284): the pieces alternate
    ms_in = torch.cat([ms_in, flag.unsqueeze(1)], 1)
    # (the teacher's labels are all 0, :193-194, :252-253: no row of it is an instance row)
    ms_lab_in = torch.cat(m_lab + [torch.zeros(ms_in.shape[0] - n_student, dtype=torch.int64, device=dev)], 0)
    totals = torch.empty(3 * nb, dtype=torch.int64, device=dev)
    cur, cur_lab, cur_b32, _ = B.stage_mix(torch.cat(s_pts, 0), torch.cat(s_lab, 0), mix, *s_n, totals=totals[:nb])
    ms, ms_lab, ms_b32, _ = B.stage_mix(ms_in, ms_lab_in, list(mix) + list(mix), m_n[0] + g_n[0], m_n[1] + g_n[1],
                                        keep=torch.cat(m_keep + g_keep, 0), totals=totals[nb:])
    totals = totals.tolist()                                            # host read 1 (rows of all mixes, all samples)
    n_cur, n_mixed = totals[:nb], totals[nb:]
    cur, cur_lab, cur_b32 = cur[:sum(n_cur)], cur_lab[:sum(n_cur)], cur_b32[:sum(n_cur)]
    ms, ms_lab, ms_b32 = ms[:sum(n_mixed)], ms_lab[:sum(n_mixed)], ms_b32[:sum(n_mixed)]
    if aug is not None:
        rec = S._aug_records(aug, nb)
        rec_dev = torch.from_numpy(np.concatenate([rec, rec], 0)).to(dev, non_blocking=True)      # (job b + B: sample b's teacher)
        augment_points(cur, rec_dev[:nb], cur_b32, out=cur)
        augment_points(ms, rec_dev, ms_b32, out=ms)
    cur_b = cur_b32.long()
    lo = B.segment_min3(cur, cur_b, nb)
    ms, ms_lab, ms_b, ms_b32, counts = B.stage_clamp_compact(ms, ms_lab, ms_b32, lo.repeat(2, 1))
    counts = counts.tolist()                                            # host read 2 (rows of both fused clouds per sample)
    n_ms, n_gt = counts[:nb], counts[nb:]
    a, b = sum(n_ms), sum(n_ms) + sum(n_gt)
    batch, shift = S._voxelize_layout(cur, cur_lab, cur_b, n_cur, ms[:a], ms_lab[:a], ms_b[:a], ms_b32[:a], n_ms,
                                      S._prefix_mask(n_cur, n_ms, dev), voxel_size, [pair[0].get("name", "") for pair in used],
                                      return_shift=True)
    return _teacher_voxels(batch, shift, ms[a:b], ms_b[a:b] - nb, ms_b32[a:b] - nb, n_mixed[nb:], voxel_size, nb)


def build_kd_batch(scans: List[Dict], voxel_size: float, steps: Sequence[int], steps_gt: Optional[Sequence[int]] = None, aug=None,
                   mix=None, partners=None) -> Dict:
    """The batch_dict MinkUNetMsKd consumes: build_multiscan_batch's dictionary plus `lidar_ms_gt`, `offset_ms_gt` and
    `num_points_ms_gt`.  scans[b]: the scan dict of build_multiscan_batch, with one more optional key `canon` - per history scan the
    class whose canonical raw id the ANNOTATION is, or -1 (`multiscan_sample(..., canon=True)`; default: `labels`, as `pseudo`
    defaults).  steps: FLEXIBLE_STEPS, applied to `pseudo` for the student's cloud; steps_gt: FLEXIBLE_STEPS_GT, applied to `canon`
    for the teacher's (default: steps).  aug / mix / partners: as build_multiscan_batch - one AugParams, one MixParams and the
    partner's scan dict per sample; the draws of a training sample are those of the FSA recipe, in its order
    (`draw_mix_params`, then `draw_train_params`).  At most 64 samples, 32 with mix=."""
    if not scans or len(scans) > 64:
        raise ValueError("build_kd_batch: 1 .. 64 samples per batch")
    steps = list(steps)
    steps_gt = steps if steps_gt is None else list(steps_gt)
    if len(steps_gt) != len(steps):
        raise ValueError("steps and steps_gt must hold one step per class")
    if mix is not None:
        if len(scans) > 32:
            raise ValueError("build_kd_batch: at most 32 samples per batch with mix= (two fused jobs per sample)")
        mix, partners = S._mix_records(mix, partners, len(scans))
        return _build_mix(scans, partners, mix, voxel_size, steps, steps_gt, aug)
    return _build_plain(scans, voxel_size, steps, steps_gt, aug)
