"""numpy restatements of csrc/range_view.hip (ts_rv_project, ts_rv_knn) under the rules include/taseg_hip.h states, the synthetic
inputs the range-view tests share, and the functions that say which rows are UNDECIDED - where the reference itself may land on
either side:

  projection   a row whose float64 proj_x / proj_y lies within a derived bound of a cell edge (project_delta: the reference's float32
               arctan2 / arcsin are not correctly rounded, and the chain's roundings carry that to a fraction of a cell)
  kNN          a point whose K-th and (K + 1)-th distances are equal while the tied slots would vote differently (the reference's
               topk(sorted=False) states no tie rule; this library's is ascending (distance, slot))
"""
import numpy as np

F32 = np.float32
ERR_BATCH, ERR_PIXEL, ERR_NONFINITE, ERR_ORIGIN = 1, 2, 16, 32


# ------------------------------------------------------------------------------------------------------------ projection
def fov_terms(fov_up, fov_down):
    """(|fov_down|, fov) in radians as laserscan.py:182-184 evaluates them, in double"""
    up = fov_up / 180.0 * np.pi
    down = fov_down / 180.0 * np.pi
    return abs(down), abs(down) + abs(up)


def project32(points, batch, first, b, h, w, fov_up=3.0, fov_down=-25.0, labels=None):
    """ts_rv_project in numpy, bit for bit: the float32 chain with the arctan2 / arcsin of the doubles rounded once"""
    pts = np.ascontiguousarray(points[:, :4], dtype=F32)
    n = len(pts)
    batch = np.asarray(batch).astype(np.int64)
    first = np.asarray(first).astype(np.int64)
    x, y, z, rem = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    in_batch = (batch >= 0) & (batch < b)
    local = np.arange(n, dtype=np.int64) - first[np.clip(batch, 0, b - 1)]
    bad_batch = ~in_batch | (local < 0)
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        depth = np.sqrt((x * x + y * y) + z * z).astype(F32)
        origin = finite & (depth == 0)
        valid = finite & ~origin & ~bad_batch
        yaw = -(np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F32))
        pitch = np.arcsin((z / depth).astype(np.float64)).astype(F32)
        fd, fov = fov_terms(fov_up, fov_down)
        fx = F32(0.5) * (yaw / F32(np.pi) + F32(1.0))
        fy = F32(1.0) - (pitch + F32(fd)) / F32(fov)
        fx = fx * F32(w)
        fy = fy * F32(h)
        assert fx.dtype == F32 and fy.dtype == F32
        fx = np.maximum(F32(0), np.minimum(F32(w - 1), np.floor(fx)))
        fy = np.maximum(F32(0), np.minimum(F32(h - 1), np.floor(fy)))
    col = np.where(valid, np.nan_to_num(fx), -1).astype(np.int32)
    row = np.where(valid, np.nan_to_num(fy), -1).astype(np.int32)
    unproj = np.where(valid, depth, F32(-1)).astype(F32)
    err = (ERR_BATCH if bad_batch.any() else 0) | (ERR_NONFINITE if (~finite).any() else 0) | (ERR_ORIGIN if origin.any() else 0)
    # the winner: smallest depth, lowest local index among equal depths
    table = np.full(b * h * w, np.iinfo(np.uint64).max, dtype=np.uint64)
    at = np.flatnonzero(valid)
    cell = batch[at] * h * w + row[at].astype(np.int64) * w + col[at]
    key = (depth[at].view(np.uint32).astype(np.uint64) << np.uint64(32)) | local[at].astype(np.uint64)
    np.minimum.at(table, cell, key)
    won = table != np.iinfo(np.uint64).max
    idx = np.where(won, (table & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    src = np.where(won, idx + first[np.arange(b * h * w) // (h * w)], 0)
    one = F32(-1)
    if n == 0:                                                         # nothing to index: every pixel is background
        pts, depth = np.zeros((1, 4), dtype=F32), np.zeros(1, dtype=F32)
    vx, vy, vz = (np.where(won, pts[src, k], one).astype(F32) for k in range(3))
    vr = np.where(won, pts[src, 3], one).astype(F32)
    rng = np.where(won, depth[src], one).astype(F32)
    mask = (idx > 0).astype(F32)
    scan = np.stack([vx / F32(50.0), vy / F32(50.0), vz / F32(3.0), vr, rng / F32(80.0), mask]).astype(F32)     # [6, B H W]
    scan_rv = scan.reshape(6, b, h, w).transpose(1, 0, 2, 3).copy()
    out = {"proj_x": col, "proj_y": row, "unproj_range": unproj, "err": err, "scan_rv": scan_rv,
           "proj_range": rng.reshape(b, h, w), "proj_idx": idx.astype(np.int32).reshape(b, h, w), "valid": valid}
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64) if n else np.zeros(1, dtype=np.int64)
        out["label_rv"] = np.where(won, lab[src], 0).astype(np.int64).reshape(b, 1, h, w)
    return out


def proj_xy64(points, h, w, fov_up=3.0, fov_down=-25.0):
    """(proj_x, proj_y, q = z / depth) of the chain in float64 on the float32 coordinates, before the floor"""
    p = np.asarray(points[:, :3], dtype=np.float64)
    with np.errstate(all="ignore"):
        depth = np.sqrt((p ** 2).sum(1))
        q = p[:, 2] / depth
        fd, fov = fov_terms(fov_up, fov_down)
        px = 0.5 * (-np.arctan2(p[:, 1], p[:, 0]) / np.pi + 1.0) * w
        py = (1.0 - (np.arcsin(q) + fd) / fov) * h
    return px, py, q


def project_delta(points, h, w, fov_up=3.0, fov_down=-25.0, ulps=4.0):
    """(delta_x [n], delta_y [n]): how far, in cells, a float32 evaluation of the chain whose arctan2 / arcsin err by `ulps` float32
    ulps may sit from proj_xy64 - derived as rpvnet_ref.stage_delta is, per row where the bound depends on the row.

    proj_x.  |yaw| <= pi, values in [2, 4): ulp 2^-22, so the arctan2 errs by ulps 2^-22 (the negation is exact).  yaw / (float)pi
    errs relatively by |f(pi) - pi| / pi and one rounding of a value <= 1 (2^-24); + 1 rounds a value <= 2 (2^-24); the halving is
    exact; the product with W rounds a value <= W (W 2^-24).
    proj_y.  Each square and each of the two sums rounds once (relative 2^-24 each; the squares are positive, so the sum's relative
    error is at most 3 2^-24), the square root halves that and rounds (2.5 2^-24), the quotient q = z / depth rounds again: 3.5 2^-24
    relative.  arcsin carries an error e of q to e / sqrt(1 - q^2) (to first order; unbounded at |q| = 1, such a row is undecided
    unless the clamp decides it) and errs itself by ulps 2^-23 (|pitch| < 2).  pitch + (float)|fov_down| rounds a value < 2 (2^-24),
    the constant's own rounding is below 2^-26; the quotient v by (float)fov errs relatively by 2^-24 for the divisor and 2^-24 for
    the rounding; u = 1 - v rounds (2^-24 max(1, |u|)); u H rounds (2^-24 |u| H)."""
    _, py, q = proj_xy64(points, h, w, fov_up, fov_down)
    n = len(py)
    f_pi = float(F32(np.pi))
    e_unit = ulps * 2.0 ** -22 / np.pi + abs(f_pi - np.pi) / np.pi + 2 * 2.0 ** -24
    dx = np.full(n, 0.5 * w * e_unit + w * 2.0 ** -24)
    fd, fov = fov_terms(fov_up, fov_down)
    with np.errstate(all="ignore"):
        e_pitch = 3.5 * 2.0 ** -24 * np.abs(q) / np.sqrt(np.maximum(1.0 - q * q, 0.0)) + ulps * 2.0 ** -23
        u = py / h
        v = 1.0 - u
        e_v = (e_pitch + 2.0 ** -24 + 2.0 ** -26) / fov + 2 * 2.0 ** -24 * np.abs(v)
        e_u = e_v + 2.0 ** -24 * np.maximum(1.0, np.abs(u))
        dy = h * e_u + 2.0 ** -24 * np.abs(u) * h
    dy = np.where(np.isfinite(dy), dy, np.inf)
    return dx, dy


def _edge_within(v, delta, size):
    """an integer edge 1 .. size - 1 within delta of v (the edges 0 and `size` are decided by the clamp)"""
    with np.errstate(all="ignore"):
        lo, hi = v - delta, v + delta
        first = np.ceil(lo)                       # the first integer >= lo
        first = np.maximum(first, 1.0)
        return ~(np.isfinite(v)) | ((first <= hi) & (first <= size - 1))


def project_undecided(points, h, w, fov_up=3.0, fov_down=-25.0, ulps=4.0):
    """rows whose column or row the reference's float32 chain may put on either side of a cell edge"""
    px, py, _ = proj_xy64(points, h, w, fov_up, fov_down)
    dx, dy = project_delta(points, h, w, fov_up, fov_down, ulps)
    return _edge_within(px, dx, w) | _edge_within(py, dy, h)


# ------------------------------------------------------------------------------------------------------------------ kNN
def knn_window(proj_range, proj_class, unproj_range, px, py, batch, weight, search):
    """(distance [n, S S] float32, class [n, S S] int64, ok [n]) under the kernel's rules"""
    b, h, w = proj_range.shape
    s_, p = int(search), (int(search) - 1) // 2
    px, py, batch = (np.asarray(a).astype(np.int64) for a in (px, py, batch))
    ok = (batch >= 0) & (batch < b) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    bb, xx, yy = np.where(ok, batch, 0), np.where(ok, px, 0), np.where(ok, py, 0)
    pr = np.pad(np.asarray(proj_range, dtype=F32), ((0, 0), (p, p), (p, p)))
    pc = np.pad(np.asarray(proj_class).astype(np.int64), ((0, 0), (p, p), (p, p)))
    rp = np.asarray(unproj_range, dtype=F32)
    n = len(rp)
    r = np.empty((n, s_ * s_), dtype=F32)
    c = np.empty((n, s_ * s_), dtype=np.int64)
    for s in range(s_ * s_):
        dy, dx = divmod(s, s_)
        r[:, s] = pr[bb, yy + dy, xx + dx]
        c[:, s] = pc[bb, yy + dy, xx + dx]
    r[r < 0] = np.inf
    r[:, (s_ * s_ - 1) // 2] = rp
    with np.errstate(all="ignore"):
        d = (np.abs(r - rp[:, None]) * np.asarray(weight, dtype=F32).reshape(1, -1)).astype(F32)
    d[np.isnan(d)] = np.inf
    return d, c, ok


def knn32(proj_range, proj_class, unproj_range, px, py, batch, weight, k, search, cutoff, nclasses):
    """ts_rv_knn in numpy: (label [n] int32, err, undecided [n] bool)"""
    d, c, ok = knn_window(proj_range, proj_class, unproj_range, px, py, batch, weight, search)
    b = proj_range.shape[0]
    n, ss = d.shape
    order = np.argsort(d, axis=1, kind="stable")                       # ascending (distance, slot)
    ds = np.take_along_axis(d, order, 1)
    cs = np.take_along_axis(c, order, 1)
    if cutoff > 0:
        cs = np.where(ds > F32(cutoff), nclasses, cs)
    sel = cs[:, :k]
    counts = np.stack([(sel == cls).sum(1) for cls in range(1, nclasses)], 1) if n else np.zeros((0, nclasses - 1), dtype=np.int64)
    label = np.where(ok, counts.argmax(1) + 1, 0).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    batch = np.asarray(batch).astype(np.int64)
    err = (ERR_BATCH if ((batch < 0) | (batch >= b)).any() else 0)
    px, py = np.asarray(px).astype(np.int64), np.asarray(py).astype(np.int64)
    h, w = proj_range.shape[1:]
    err |= ERR_PIXEL if ((px < 0) | (px >= w) | (py < 0) | (py >= h)).any() else 0
    # undecided: the K-th and (K + 1)-th distances are equal and the slots of that distance would not all vote alike
    undecided = np.zeros(n, dtype=bool)
    if k < ss and n:
        tie = ds[:, k - 1] == ds[:, k]
        group = ds == ds[:, k - 1:k]
        vote = np.where((cs >= 1) & (cs < nclasses), cs, 0)            # what a slot adds to the counts (0: nothing)
        lo = np.where(group, vote, np.iinfo(np.int64).max).min(1)
        hi = np.where(group, vote, -1).max(1)
        undecided = ok & tie & (lo != hi)
    return label, err, undecided


def hand_knn_case():
    """an 8 x 16 image (every range 10) and three points.  Point 0 at (x 4, y 3), range 10: its 3 x 3 window holds the classes
    3 3 5 / 5 7 0 / 0 0 0 - with K = 9 and no cutoff a count tie of 3 and 5, where the LOWEST class wins.  Point 1 at (x 12, y 5),
    range 100: its pixel has class 0, the eight around it class 9 - with cutoff 1 every neighbour is cut off and the centre
    (distance 0) votes for nothing: class 1; without a cutoff class 9.  Point 2 in the corner (0, 0) with class 4 around it."""
    pr = np.full((1, 8, 16), 10.0, dtype=F32)
    pc = np.zeros((1, 8, 16), dtype=np.int32)
    pc[0, 2:5, 3:6] = np.array([[3, 3, 5], [5, 7, 0], [0, 0, 0]])
    pc[0, 4:7, 11:14] = 9
    pc[0, 5, 12] = 0
    pc[0, 0:2, 0:2] = 4
    return {"proj_range": pr, "proj_class": pc, "unproj_range": np.array([10.0, 100.0, 10.5], dtype=F32),
            "px": np.array([4, 12, 0], dtype=np.int32), "py": np.array([3, 5, 0], dtype=np.int32),
            "batch": np.zeros(3, dtype=np.int32)}


def knn_weight64(search, sigma):
    """1 - gaussian in float64, to cross-check the product's float32 table (taseg_amd.data.range_view.knn_weight)"""
    ax = np.arange(search) - (search - 1) / 2.0
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2.0 * sigma ** 2))
    return (1.0 - g / g.sum()).reshape(-1)


# the kNN cases of the reference fixture (tests/golden/make_golden_range_view.py records the reference's labels for each):
# name -> (kwargs of synth_knn_case or "hand", search, knn, cutoff, nclasses, continuous)
def knn_cases():
    cases = {}
    for s in (3, 5, 7):
        for k in (1, 5, s * s):
            cases["s%d_k%d" % (s, k)] = (dict(seed=100 + 10 * s + k % 7, b=1, h=8, w=16, n=4000, nclasses=20), s, k, 1.0, 20, True)
    cases["s5_k5_nocut"] = (dict(seed=201, b=1, h=8, w=16, n=4000, nclasses=20), 5, 5, 0.0, 20, True)
    cases["s5_k5_c32"] = (dict(seed=202, b=1, h=8, w=16, n=4000, nclasses=32), 5, 5, 1.0, 32, True)
    cases["s7_k49_nocut_c32"] = (dict(seed=203, b=1, h=8, w=16, n=2000, nclasses=32), 7, 49, 0.0, 32, True)
    cases["s5_k5_empty"] = (dict(seed=204, b=1, h=8, w=16, n=4000, nclasses=20, empty=0.6), 5, 5, 1.0, 20, True)
    cases["s3_k9_empty"] = (dict(seed=205, b=1, h=8, w=16, n=4000, nclasses=20, empty=0.6), 3, 9, 1.0, 20, True)
    cases["s5_k5_large"] = (dict(seed=206, b=1, h=64, w=128, n=20000, nclasses=20), 5, 5, 1.0, 20, True)
    cases["s5_k5_batch"] = (dict(seed=207, b=3, h=8, w=16, n=0, nclasses=20, lens=[1500, 0, 2500]), 5, 5, 1.0, 20, True)
    cases["s5_k7_quant"] = (dict(seed=208, b=1, h=8, w=16, n=4000, nclasses=20, quantum=0.25), 5, 7, 1.0, 20, False)
    cases["s5_k5_quant"] = (dict(seed=209, b=1, h=8, w=16, n=4000, nclasses=20, quantum=0.25), 5, 5, 1.0, 20, False)
    cases["s7_k5_quant_nocut"] = (dict(seed=210, b=1, h=8, w=16, n=4000, nclasses=20, quantum=0.25), 7, 5, 0.0, 20, False)
    cases["hand_k9_nocut"] = ("hand", 3, 9, 0.0, 20, False)
    cases["hand_k5_cut"] = ("hand", 3, 5, 1.0, 20, False)
    return cases


def knn_case_inputs(spec):
    return hand_knn_case() if isinstance(spec, str) else synth_knn_case(**spec)


# ------------------------------------------------------------------------------------------------------ synthetic inputs
def synth_cloud(seed, n, far=60.0):
    """a cloud whose pitch spans the field of view and a little beyond it: x, y, z, remission float32"""
    rng = np.random.RandomState(seed)
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.deg2rad(rng.uniform(-27.0, 5.0, n))
    depth = rng.uniform(2.0, far, n)
    pts = np.stack([depth * np.cos(pitch) * np.cos(yaw), depth * np.cos(pitch) * np.sin(yaw), depth * np.sin(pitch),
                    rng.uniform(0, 1, n)], 1)
    return pts.astype(F32)


def synth_knn_case(seed, b, h, w, n, nclasses, empty=0.0, quantum=None, lens=None):
    """a batch for the kNN step: proj_range [b, h, w] (with `empty` of the pixels at -1, ranges optionally quantised), proj_class,
    and n points on random pixels whose range is the pixel's plus noise (or quantised noise)"""
    rng = np.random.RandomState(seed)
    pr = rng.uniform(2.0, 12.0, (b, h, w))
    if quantum:
        pr = np.round(pr / quantum) * quantum
    pr = pr.astype(F32)
    pr[rng.uniform(size=pr.shape) < empty] = -1
    pc = rng.randint(0, nclasses, (b, h, w)).astype(np.int32)
    if lens is None:
        lens = [n // b + (1 if i < n % b else 0) for i in range(b)]
    batch = np.repeat(np.arange(b), lens).astype(np.int32)
    n = len(batch)
    px = rng.randint(0, w, n).astype(np.int32)
    py = rng.randint(0, h, n).astype(np.int32)
    base = np.abs(pr[batch, py, px]).astype(np.float64) if n else np.zeros(0)
    noise = rng.uniform(-1.5, 1.5, n)
    rp = base + noise
    if quantum:
        rp = np.round(rp / quantum) * quantum
    return {"proj_range": pr, "proj_class": pc, "unproj_range": rp.astype(F32), "px": px, "py": py, "batch": batch}
