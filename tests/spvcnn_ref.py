"""The mean-voxelisation rule of include/taseg_hip.h (ts_voxelize_mean_forward) restated in numpy float32, its float64 value and the
bound between the two - test infrastructure shared by tests/test_spvcnn_host.py and tests/test_gpu_spvcnn_kernels.py.

Rule: rows grouped by voxel in ascending row order, rows with idx < 0 or idx >= m left out; cnt = the voxel's number of rows; every
term is float32(feat[row]) / float32(cnt); the run is cut into pieces of P consecutive rows from the voxel's first row; each piece is
summed in ascending order from 0, the piece sums are added in ascending piece order from 0; a voxel of at most P rows is one
sequential sum; a voxel without rows is zeros; a half result is the float32 value rounded once.

Bound.  With u = 2^-24 and gamma(k) = k u / (1 - k u): every term carries one rounding from its division and one from every addition
it passes through that is not an addition to zero - at most P - 1 inside its piece and ceil(cnt / P) - 1 between the pieces.  For
cnt <= P that is 1 + (cnt - 1) = cnt roundings; for cnt = P + r, r >= 1, it is at most P + ceil(r / P) <= P + r = cnt.  So the float32
value is within gamma(cnt) <= gamma(cnt + 1) * sum |feat| / cnt of the exact mean, element by element (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2), and gamma(cnt + 1), the figure the tests use, leaves one rounding to spare."""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
F32 = np.float32


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def groups(idx, m):
    """(offsets [m + 1], entries): the rows of voxel v are entries[offsets[v]:offsets[v + 1]], ascending"""
    idx = np.asarray(idx).astype(np.int64)
    rows = np.flatnonzero((idx >= 0) & (idx < m))
    order = rows[np.argsort(idx[rows], kind="stable")]
    offsets = np.searchsorted(idx[order], np.arange(m + 1))
    return offsets.astype(np.int32), order.astype(np.int32)


def mean32(feat, idx, m, piece):
    """the rule in float32, np.float32 at every step; feat float32 or float16 [n, c] -> float32 [m, c]"""
    f = np.asarray(feat).astype(F32)
    off, ent = groups(idx, m)
    out = np.zeros((m, f.shape[1]), dtype=F32)
    for v in range(m):
        rows = ent[off[v]:off[v + 1]]
        cnt = F32(len(rows))
        acc = np.zeros(f.shape[1], dtype=F32)
        if len(rows) <= piece:
            for r in rows:
                acc = acc + f[r] / cnt
        else:
            for a in range(0, len(rows), piece):
                part = np.zeros(f.shape[1], dtype=F32)
                for r in rows[a:a + piece]:
                    part = part + f[r] / cnt
                acc = acc + part
        out[v] = acc
    return out


def mean64(feat, idx, m):
    """(exact mean in float64 [m, c], bound [m, c] = gamma(cnt + 1) * sum |feat| / cnt, cnt [m])"""
    f = np.asarray(feat).astype(np.float64)
    off, ent = groups(idx, m)
    ref = np.zeros((m, f.shape[1]))
    s = np.zeros_like(ref)
    cnt = (off[1:] - off[:-1]).astype(np.int64)
    for v in range(m):
        rows = ent[off[v]:off[v + 1]]
        if len(rows):
            ref[v] = f[rows].sum(0) / len(rows)
            s[v] = np.abs(f[rows]).sum(0) / len(rows)
    return ref, gamma(cnt + 1)[:, None] * s, cnt


def mean_backward(gout, idx, m):
    """grad_feat[i] = float32(gout[idx[i]]) / float32(cnt), zeros for a row that took no part; float32 [n, c]"""
    g = np.asarray(gout).astype(F32)
    idx = np.asarray(idx).astype(np.int64)
    off, _ = groups(idx, m)
    cnt = (off[1:] - off[:-1]).astype(F32)
    out = np.zeros((len(idx), g.shape[1]), dtype=F32)
    ok = (idx >= 0) & (idx < m)
    out[ok] = g[idx[ok]] / cnt[idx[ok]][:, None]
    return out


def piece_map(piece, c, seed=0):
    """(feat float32 [n, c], idx int32 [n], m): voxels of 0, 1, P, P + 1 and 3 P + 5 rows (and a few of random sizes), their rows
    scattered; some rows with idx = -1 and one with idx = m"""
    rs = np.random.RandomState(100 + seed)
    sizes = [0, 1, piece, piece + 1, 3 * piece + 5, 0, 2, 2 * piece, 4 * piece, 7, piece - 1]
    m = len(sizes)
    idx = np.concatenate([np.full(k, v) for v, k in enumerate(sizes)] + [np.full(9, -1), np.array([m])]).astype(np.int32)
    idx = idx[rs.permutation(len(idx))]
    feat = (rs.randn(len(idx), c) * 3 + 0.5).astype(F32)
    return feat, idx, m
