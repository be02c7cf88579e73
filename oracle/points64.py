"""Float64 reference of the point <-> voxel transfer kernels (csrc/pointops.hip, trilinear_kernel of csrc/coords.hip) with the
ingredients of their rounding bars, a float32 emulation of each operation, and the input families of the tests - test
infrastructure, not product code.

Written from the formulas of torchsparse's voxelize_cuda.cu (out[idx[i]] += feat[i] / counts[idx[i]]), devoxelize_cuda.cu
(out[i] = sum_k w[i,k] feat[idx[i,k]] and its adjoint gfeat[idx[i,k]] += w[i,k] gout[i]) and devoxelize.py:10-48 (the
trilinear weights).  Float32 and half inputs are cast up unchanged.  A term of a devoxelize sum is live when idx >= 0 and
w != 0 - the kernels' rule; a point of a voxelize sum when 0 <= idx < m and counts[idx] != 0.  Every sum returns, per output
row or element, the value in double, t = the number of live terms and S = sum |term|: a float32 sum of t products in ANY order
errs by at most t u S to first order (one rounding per product, at most t - 1 per addition chain), which is what one bar for
the atomic, run-wise, gathered and two-stage forms of the adjoint rests on.  The double sums here are themselves rounded
(t 2^-53 S): 2^-29 of those bars, inside SLACK.

tests/test_points64_host.py checks this file (against oracle/ts_oracle.py, by the adjoint identity, and by mutants of the
emulations that must miss the bars); tests/test_gpu_points_float64.py checks the kernels against it.
"""
import numpy as np

U = 2.0 ** -24            # relative error of one float32 rounding
TINY = 2.0 ** -149        # what one float32 operation may lose to underflow
SLACK = 1.01              # second-order terms of the first-order bounds
UH = 2.0 ** -11           # relative error of one rounding to half
TINY_H = 2.0 ** -25       # half a step of the half denormals
HALF_MAX = 65504.0
E8 = np.float32(1e-8)     # the constant of devoxelize.py:47 as the kernels hold it
TRILINEAR_K = 19          # roundings of one trilinear weight, counted in tests/test_gpu_points_float64.py


def up(a):
    """float32 / half values as doubles, unchanged"""
    return np.asarray(a).astype(np.float64)


def live(idx, w):
    idx, w = np.asarray(idx), np.asarray(w)
    return (idx >= 0) & (w != 0)


def _scatter(rows, vals, m):
    """out[rows[j]] += vals[j] in double (stable grouping, one reduceat)"""
    out = np.zeros((m, vals.shape[1]), dtype=np.float64)
    if len(rows):
        o = np.argsort(rows, kind="stable")
        r = rows[o]
        first = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
        out[r[first]] = np.add.reduceat(vals[o], first, axis=0)
    return out


# ------------------------------------------------------------------------------------------------------------- references
def voxelize_forward64(feat, idx, counts):
    """(ref [m, c], t [m], S [m, c]): the mean of the rows of every voxel's points, terms feat[i] / counts[idx[i]]"""
    f, idx, counts = up(feat), np.asarray(idx).astype(np.int64), np.asarray(counts).astype(np.int64)
    m = counts.shape[0]
    ok = (idx >= 0) & (idx < m)
    ok[ok] &= counts[idx[ok]] != 0
    term = f[ok] / counts[idx[ok]][:, None]
    return _scatter(idx[ok], term, m), np.bincount(idx[ok], minlength=m), _scatter(idx[ok], np.abs(term), m)


def voxelize_backward64(gout, idx, counts, n):
    """(ref [n, c], live [n]): gfeat[i] = gout[idx[i]] / counts[idx[i]], 0 where the point is not live"""
    g, idx, counts = up(gout), np.asarray(idx).astype(np.int64), np.asarray(counts).astype(np.int64)
    assert idx.shape[0] == n
    ok = (idx >= 0) & (idx < counts.shape[0])
    ok[ok] &= counts[idx[ok]] != 0
    ref = np.zeros((n, g.shape[1]), dtype=np.float64)
    ref[ok] = g[idx[ok]] / counts[idx[ok]][:, None]
    return ref, ok


def devoxelize_forward64(feat, idx, w):
    """(ref [n, c], t [n], S [n, c]) of out[i] = sum_k w[i,k] feat[idx[i,k]]"""
    f, idx, w64 = up(feat), np.asarray(idx).astype(np.int64), up(w)
    ok = live(idx, w)
    ref = np.zeros((idx.shape[0], f.shape[1]), dtype=np.float64)
    s = np.zeros_like(ref)
    for k in range(8):
        o = ok[:, k]
        term = w64[o, k, None] * f[idx[o, k]]
        ref[o] += term
        s[o] += np.abs(term)
    return ref, ok.sum(1), s


def adjoint64(gout, idx, w, m):
    """(ref [m, c], t [m], S [m, c]) of gfeat[v] = sum over the live slots (i, k) with idx[i,k] = v of w[i,k] gout[i] - the
    adjoint as an operator, whatever the kernel form"""
    g, idx, w64 = up(gout), np.asarray(idx).astype(np.int64), up(w)
    ok = live(idx, w)
    ref = np.zeros((m, g.shape[1]), dtype=np.float64)
    s = np.zeros_like(ref)
    for k in range(8):
        o = ok[:, k]
        term = w64[o, k, None] * g[o]
        ref += _scatter(idx[o, k], term, m)
        s += _scatter(idx[o, k], np.abs(term), m)
    return ref, np.bincount(idx[ok], minlength=m)[:m], s


def _corner(k, x_innermost=False):
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1) if x_innermost else ((k >> 2) & 1, (k >> 1) & 1, k & 1)


def _lookup(points, vox, s):
    """(corner indices [n, 8] int32 by a dictionary on (x, y, z, b), cell = floor(p / s) in float32 [n, 3])"""
    p = np.asarray(points, dtype=np.float32)
    vox = np.asarray(vox).astype(np.int64)
    table = {tuple(r): i for i, r in enumerate(vox.tolist())}
    assert len(table) == len(vox), "duplicate voxel coordinates: which one a lookup returns is unspecified"
    cell = np.floor(p[:, :3] / np.float32(s))                     # float32, as the reference and the kernel take it
    base = cell.astype(np.int64) * int(s)
    b = p[:, 3].astype(np.int64)
    idx = np.full((len(p), 8), -1, dtype=np.int32)
    for k in range(8):
        cx, cy, cz = _corner(k)
        keys = zip((base[:, 0] + cx * s).tolist(), (base[:, 1] + cy * s).tolist(), (base[:, 2] + cz * s).tolist(), b.tolist())
        idx[:, k] = [table.get(key, -1) for key in keys]
    return idx, cell


def trilinear64(points, vox, s):
    """(idx [n, 8] int32, w [n, 8] float64) for float32 points [n, 4] (x, y, z, batch), int32 voxel coordinates [m, 4] and stride
    s: corner k = ((k>>2)&1, (k>>1)&1, k&1) s from the cell's base, x outermost; weights by devoxelize.py:10-48 in double on the
    float32 floor: products of the distances to the opposite faces, / s^3, 0 where the corner is absent, / (sum + 1e-8f)."""
    idx, cell = _lookup(points, vox, s)
    p = up(points)[:, :3]
    lo = cell.astype(np.float64) * s
    d = (lo + s - p, p - lo)
    w = np.zeros((len(p), 8), dtype=np.float64)
    for k in range(8):
        cx, cy, cz = _corner(k)
        w[:, k] = d[cx][:, 0] * d[cy][:, 1] * d[cz][:, 2] / float(s) ** 3
    w[idx < 0] = 0.0
    return idx, w / (w.sum(1, keepdims=True) + float(E8))


# ----------------------------------------------------------------------------------------------------------------- bars
def bar_sum(t, s, tiny_terms=None):
    """SLACK t u S + t TINY for a float32 sum of t products (or quotients) in any order; t [rows], S [rows, c]"""
    t = np.asarray(t, dtype=np.float64)[:, None]
    return SLACK * t * U * s + (t if tiny_terms is None else tiny_terms) * TINY


def bar_half(e32, ref):
    """a half-storage form: the float32 bar of the same case, carried through one rounding to half"""
    return e32 * (1 + UH) + UH * np.abs(ref) + TINY_H


def bar_trilinear(w64):
    return SLACK * TRILINEAR_K * U * w64 + TINY


# ---------------------------------------------------------------------------------------------------- float32 emulations
F32 = np.float32


def sequence(n, order, seed=0):
    """a visiting order of n things: 'natural', 'reversed' or 'random' (seeded)"""
    a = np.arange(n)
    if order == "reversed":
        return a[::-1].copy()
    if order == "random":
        return np.random.RandomState(seed).permutation(n)
    assert order == "natural", order
    return a


def voxelize_forward32(feat, idx, counts, order="natural"):
    """float32, one point after the other in the given order"""
    f, idx, counts = np.asarray(feat).astype(F32), np.asarray(idx).astype(np.int64), np.asarray(counts)
    m = counts.shape[0]
    ok = (idx >= 0) & (idx < m)
    ok[ok] &= counts[idx[ok]] != 0
    seq = sequence(len(idx), order)
    seq = seq[ok[seq]]
    out = np.zeros((m, f.shape[1]), dtype=F32)
    np.add.at(out, idx[seq], f[seq] / counts[idx[seq]].astype(F32)[:, None])
    return out


def voxelize_backward32(gout, idx, counts, n):
    g, idx, counts = np.asarray(gout).astype(F32), np.asarray(idx).astype(np.int64), np.asarray(counts)
    ok = (idx >= 0) & (idx < counts.shape[0])
    ok[ok] &= counts[idx[ok]] != 0
    out = np.zeros((n, g.shape[1]), dtype=F32)
    out[ok] = g[idx[ok]] / counts[idx[ok]].astype(F32)[:, None]
    return out


def devoxelize_forward32(feat, idx, w, order="natural", swap_corner=False, half_out=False):
    """float32, the eight corners in the given order.  swap_corner (a mutant): the weight of corner k ^ 1."""
    f, idx, w = np.asarray(feat).astype(F32), np.asarray(idx).astype(np.int64), np.asarray(w, dtype=F32)
    ok = live(idx, w)
    out = np.zeros((idx.shape[0], f.shape[1]), dtype=F32)
    for k in sequence(8, order):
        o = ok[:, k]
        out[o] = out[o] + w[o, k ^ 1 if swap_corner else k, None] * f[idx[o, k]]
    return out.astype(np.float16) if half_out else out


def adjoint32(gout, idx, w, m, order="natural", drop_last_of=None, drop_tail4_of=None, swap_corner=False, partial_len=None,
              partial_half=False, half_out=False):
    """float32: every voxel adds its live slots one after the other, in the order in which `order` visits the slots
    (point * 8 + corner).  partial_len: the list is cut into pieces of that many slots, each summed on its own and the
    partial sums added in turn (the two-stage form).  The mutants: drop_last_of = v, the last slot of voxel v's list is left
    out; drop_tail4_of = v, what follows its last whole group of four; swap_corner, the weight of corner k ^ 1;
    partial_half, every partial sum rounded to half."""
    g, idx, w = np.asarray(gout).astype(F32), np.asarray(idx).astype(np.int64), np.asarray(w, dtype=F32)
    flat_idx, flat_w = idx.reshape(-1), w.reshape(-1)
    seq = sequence(flat_idx.shape[0], order)
    slots = seq[live(flat_idx, flat_w)[seq]]
    o = np.argsort(flat_idx[slots], kind="stable")
    slots = slots[o]
    bounds = np.searchsorted(flat_idx[slots], np.arange(m + 1))
    out = np.zeros((m, g.shape[1]), dtype=F32)
    for v in range(m):
        s = slots[bounds[v]:bounds[v + 1]]
        if v == drop_last_of:
            s = s[:-1]
        if v == drop_tail4_of:
            s = s[:len(s) // 4 * 4]
        step = partial_len or max(len(s), 1)
        acc = np.zeros(g.shape[1], dtype=F32)
        for a in range(0, len(s), step):
            part = np.zeros(g.shape[1], dtype=F32)
            for slot in s[a:a + step]:
                part = part + flat_w[slot ^ 1 if swap_corner else slot] * g[slot >> 3]
            if partial_half:
                part = part.astype(np.float16).astype(F32)
            acc = acc + part
        out[v] = acc
    return out.astype(np.float16) if half_out else out


def trilinear32(points, vox, s, order="natural", x_innermost=False, forget_s3=False):
    """trilinear_kernel in numpy float32, the eight weights summed in the given order.  The mutants: x_innermost, the weight of
    corner k computed as if x were the innermost axis; forget_s3, no division by s^3."""
    idx, cell = _lookup(points, vox, s)
    p = np.asarray(points, dtype=F32)[:, :3]
    fs = F32(s)
    lo = cell * fs if s != 1 else np.floor(p)
    hi = lo + fs
    d = (hi - p, p - lo)
    w = np.zeros((len(p), 8), dtype=F32)
    for k in range(8):
        cx, cy, cz = _corner(k, x_innermost)
        v = (d[cx][:, 0] * d[cy][:, 1]) * d[cz][:, 2]
        w[:, k] = v if s == 1 or forget_s3 else v / F32(s * s * s)
    w[idx < 0] = 0
    tot = np.zeros(len(p), dtype=F32)
    for k in sequence(8, order):
        tot = tot + w[:, k]
    return idx, w / (tot + E8)[:, None]


# ------------------------------------------------------------------------------------------------------- input families
CORE_ROWS = 336           # rows of the constructed map's fixed part
CORE_VOXELS = 20          # voxels 0 .. 19 belong to it
CORE_SLOTS = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5, 5: 8, 6: 9, 7: 710, 19: 0}       # live slots of its voxels, by construction
CELLS = (1, 2, 63, 64, 65, 129)                                             # points per cell (identical corner tuples)


def random_map(n, m, seed, first_voxel=0):
    """[n, 8] indices in {-1} + [first_voxel, m) and weights in (0, 0.6), an eighth of them 0, a quarter of the corners absent"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(first_voxel, m, size=(n, 8)).astype(np.int32)
    idx[rs.rand(n, 8) < 0.25] = -1
    w = (rs.rand(n, 8) * 0.6 + 2.0 ** -10).astype(F32)
    w[rs.rand(n, 8) < 0.125] = 0
    return idx, w


def constructed_map(n, seed=0):
    """(idx [n, 8] int32, w [n, 8] float32, m).  For n >= CORE_ROWS: a fixed part, its rows scattered among random rows on
    voxels of their own, with
      voxels of 0 (present with weight zero only), 1, 3, 4, 5, 8, 9 and 710 live slots (CORE_SLOTS) and one never named;
      a voxel twice and three times in one tuple; a tuple of eight -1 with non-zero weights; zero weights on present corners;
      six cells of CELLS points, every cell with a first corner of its own, their points scattered;
      two tuples that share their first present corner (corner 1) and differ at corner 7, alternating.
    For smaller n: random rows only (the sizes 1, 31, 32, 33 around one run of the run-wise kernel)."""
    rs = np.random.RandomState(1000 + seed)
    if n < CORE_ROWS:
        m = 7
        idx, w = random_map(n, m, 2000 + seed)
        return idx, w, m
    rows = [[1, 2, 3, 4, -1, -1, -1, -1], [2, 2, 3, 4, 5, 6, -1, 0], [-1, 3, 3, 4, 5, 6, 5, 6], [4, 4, 5, 5, 6, 6, -1, -1],
            [5, 5, 5, 6, 6, 6, 6, -1], [-1] * 8, [0] * 8]
    zero = [(1, 7), (6, 0), (6, 1), (6, 2), (6, 3), (6, 4), (6, 5), (6, 6), (6, 7)]       # (row, corner) of weight 0
    for j, size in enumerate(CELLS):                        # voxel 7 at one, two or three later corners: 324 + 321 + 65 slots
        t = [8 + j, -1, 14, 7, -1, 7 if size >= 63 else 15, 7 if size == 65 else -1, 16]
        rows += [t] * size
    a, b = [-1, 17, 18, -1, -1, -1, -1, 17], [-1, 17, 18, -1, -1, -1, -1, 18]
    rows += [a, b, a, b, a]
    core = np.array(rows, dtype=np.int32)
    assert core.shape == (CORE_ROWS, 8)
    cw = (rs.rand(CORE_ROWS, 8) * 0.6 + 2.0 ** -10).astype(F32)
    for r, k in zero:
        cw[r, k] = 0
    m = CORE_VOXELS + 13
    xi, xw = random_map(n - CORE_ROWS, m, 3000 + seed, first_voxel=CORE_VOXELS)
    idx, w = np.concatenate([core, xi]), np.concatenate([cw, xw])
    perm = rs.permutation(n)
    idx, w = np.ascontiguousarray(idx[perm]), np.ascontiguousarray(w[perm])
    slots = np.bincount(idx[live(idx, w)], minlength=m)
    assert all(slots[v] == k for v, k in CORE_SLOTS.items()), slots[:CORE_VOXELS]
    return idx, w, m


def exact_case(idx, w, m, c, seed):
    """Inputs on which every float32 partial sum is exact, whatever the order: weights in {0, 2^-j} (j = 0 .. 3) where `w` is
    non-zero, voxel rows of integers in [-8, 8], gradient rows of integers in [0, 32] (half holds them all).  A sum of at most
    60 000 terms of magnitude <= 32 in steps of 1/8 stays below 2^24 steps; the gradients are of one sign, so the partial sum of
    a 64-point segment needs more than the 11 bits of a half.  Returns (w, feat [m, c], gout [n, c]) as float32."""
    rs = np.random.RandomState(4000 + seed)
    n = idx.shape[0]
    assert np.bincount(idx[idx >= 0], minlength=m).max() * 32 * 8 < 2 ** 24
    wx = np.where(np.asarray(w) != 0, 2.0 ** -rs.randint(0, 4, size=(n, 8)), 0.0).astype(F32)
    feat = rs.randint(-8, 9, size=(m, c)).astype(F32)
    gout = rs.randint(0, 33, size=(n, c)).astype(F32)
    return wx, feat, gout


def scan_points(stride, seed=0, n_scan=2600):
    """(points [n, 4] float32 (x, y, z, batch), voxel coordinates [m, 4] int32 unique) of a trilinear map at `stride`:
    points of a synthetic scan in voxel units (genuinely varying fractions, both signs), and by hand
      points on lattice nodes, on faces, one ulp below a lattice plane (with the far corners absent: only then does the
      constant 1e-8 weigh), magnitudes 2^-10 and 4000, a second batch sharing the xyz of a sixth of the first, a batch without voxels.
    Voxels: the corners of the points' cells, 60 % of them kept."""
    from taseg_amd.data.synthetic import synth_scan
    rs = np.random.RandomState(5000 + 10 * seed + stride)
    s = int(stride)
    pts, _ = synth_scan(7 + seed, n_points=20000, n_beams=16, n_az=400)
    xyz = (pts[rs.permutation(len(pts))[:n_scan], :3] / np.float32(0.05)).astype(F32)
    fs = F32(s)
    node = np.array([[3, -2, 5], [0, 0, 0], [-7, 11, -1]], dtype=F32) * fs
    face = np.array([[3.25, -2, 5.5], [-1, 0.75, 0.125], [6.5, 7.5, -4]], dtype=F32) * fs
    below = np.nextafter(np.array([[4, 2.5, 1.5], [-3, -1.25, 2], [8, 8, 8], [1, 1, 0.5]], dtype=F32) * fs, F32(-np.inf))
    small = np.array([[2.0 ** -10, 3 * 2.0 ** -10, 0.5], [-2.0 ** -10, 2.0 ** -10, -0.75]], dtype=F32)
    large = np.array([[4000.3, -3999.7, 12.1], [-4000.0, 3999.999, 4000.5]], dtype=F32)
    hand = np.concatenate([node, face, below, small, large])
    first = np.concatenate([xyz, hand])
    b0 = np.concatenate([first, np.zeros((len(first), 1), F32)], 1)
    n1, n2 = n_scan // 6, n_scan // 60
    b1 = np.concatenate([first[:n1], np.ones((n1, 1), F32)], 1)
    b2 = np.concatenate([first[n1:n1 + n2], np.full((n2, 1), 2, F32)], 1)
    points = np.ascontiguousarray(np.concatenate([b0, b1, b2]).astype(F32))
    assert not ((np.abs(points[:, :3]) > 0) & (np.abs(points[:, :3]) < 2.0 ** -60)).any()
    base = np.floor(points[:, :3] / fs).astype(np.int64) * s
    corners = []
    for k in range(8):
        off = np.array(_corner(k), dtype=np.int64) * s
        corners.append(np.concatenate([base + off, points[:, 3:4].astype(np.int64)], 1))
    vox = np.unique(np.concatenate(corners)[np.concatenate(corners)[:, 3] < 2], axis=0)
    vox = vox[rs.rand(len(vox)) < 0.6]
    # the points one ulp below a plane: drop the voxels on the far side of that plane from their cells, keep the base corner
    lo = len(xyz) + len(node) + len(face)
    gone, kept = set(), []
    for i in range(lo, lo + len(below)):
        bx, by, bz = base[i].tolist()
        for k in range(1, 8):
            cx, cy, cz = _corner(k)
            if cx:
                gone.add((bx + s, by + cy * s, bz + cz * s, 0))
        kept.append((bx, by, bz, 0))
    rows = [r for r in map(tuple, vox.tolist()) if r not in gone] + kept
    vox = np.unique(np.array(rows, dtype=np.int64), axis=0).astype(np.int32)
    return points, np.ascontiguousarray(vox[rs.permutation(len(vox))])
