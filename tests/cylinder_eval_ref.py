"""A numpy restatement of the evaluation tail for logits rows that are not grouped by scene (include/taseg_hip.h
ts_eval_confusion_rows / ts_eval_votes_rows; Cylinder_TS's evaluation branch, cylinder_ts.py:244-260), written from the header's
rules and not from the kernels: the tests compare the kernels and `pcseg.eval`'s host functions with it.

The layout rule is the kernels' own, so that the restatement also says what a malformed batch gives: cnt_p[s] = the points whose
batch index is s, scene s owns the ARRAY POSITIONS start_p[s] .. start_p[s] + cnt_p[s] - 1 (start_p = the running sum), its kept
points are the first m_s = min(cnt_p[s], max(num_points[s], 0)) of them.  For a column grouped by scene in ascending order these
are the scene's own points."""
import numpy as np

FLAG_RANGE, FLAG_ORDER, FLAG_VOTES, FLAG_NO_ROW = 1, 2, 16, 64


def layout(pts_scene, num_points):
    """(kept: per scene the array positions of its kept points, m [n_scenes], flags)"""
    pts_scene, n_scenes = np.asarray(pts_scene).astype(np.int64), len(num_points)
    inside = (pts_scene >= 0) & (pts_scene < n_scenes)
    flags = 0 if inside.all() else FLAG_RANGE
    if (pts_scene[:-1] > pts_scene[1:]).any():
        flags |= FLAG_ORDER
    cnt = np.bincount(pts_scene[inside], minlength=n_scenes)
    start = np.cumsum(cnt) - cnt
    m = np.minimum(cnt, np.maximum(np.asarray(num_points, np.int64), 0))
    return [np.arange(start[s], start[s] + m[s]) for s in range(n_scenes)], m, flags


def confusion_rows(logits, rows, pts_scene, labels, num_points):
    """(hist [C, C] int64, pred of the kept points scene-major - 0 where the point has no row -, m, flags)"""
    n_vox, C = logits.shape
    kept, m, flags = layout(pts_scene, num_points)
    x = logits.astype(np.float32)
    hist, preds = np.zeros((C, C), np.int64), []
    for p in kept:
        r = np.asarray(rows)[p].astype(np.int64)
        ok = (r >= 0) & (r < n_vox)
        if not ok.all():
            flags |= FLAG_NO_ROW
        pred = np.zeros(len(p), np.int64)
        if ok.any():
            pred[ok] = np.argmax(x[r[ok]], axis=1)               # the first maximum; a NaN wins
        lab = np.asarray(labels)[p].astype(np.int64)
        k = ok & (lab >= 0) & (lab < C)
        np.add.at(hist, (lab[k], pred[k]), 1)
        preds.append(pred)
    return hist, (np.concatenate(preds) if preds else np.zeros(0, np.int64)), m, flags


def votes_rows(logits, rows, pts_scene, num_points):
    """(total [n, C] float32 = ((x_0 + x_1) + x_2) + ... in vote order - a vote without a row leaves its term out -, label [n], flags);
    total and label are None where the votes differ in length (nothing is written)"""
    n_vox, C = logits.shape
    kept, m, flags = layout(pts_scene, num_points)
    if len(set(m.tolist())) != 1:
        return None, None, flags | FLAG_VOTES
    n = int(m[0])
    total, seen = np.zeros((n, C), np.float32), np.zeros(n, bool)
    for p in kept:
        r = np.asarray(rows)[p].astype(np.int64)
        ok = (r >= 0) & (r < n_vox)
        if not ok.all():
            flags |= FLAG_NO_ROW
        x = logits[r[ok]].astype(np.float32)
        first = ok & ~seen
        total[first] = x[first[ok]]
        again = ok & seen
        total[again] += x[again[ok]]
        seen |= ok
    return total, np.argmax(total, axis=1) if n else np.zeros(0, np.int64), flags


def host_dictionary(logits, rows, pts_scene, labels, num_points):
    """the dictionary Cylinder_TS's host branch returns for these arrays (well-formed batch, every row found): per scene
    `logits[rows of the scene's points][:n]`, its arg-max and the labels"""
    out = {"point_predict": [], "point_labels": [], "point_predict_logits": []}
    for s, n in enumerate(num_points):
        p = np.flatnonzero(np.asarray(pts_scene) == s)[:max(int(n), 0)]
        x = logits[np.asarray(rows)[p]]
        out["point_predict"].append(np.argmax(x, axis=1) if len(p) else np.zeros(0, np.int64))
        out["point_labels"].append(np.asarray(labels)[p])
        out["point_predict_logits"].append(x)
    return out
