"""Numpy restatements of what csrc/rpvnet.hip and csrc/range_stage.hip compute - test infrastructure shared by
tests/test_rpvnet_host.py, tests/test_gpu_rpvnet_kernels.py, tests/test_gpu_range_stage.py and tests/test_gpu_rpvnet_model.py.

  plan32         ts_range_plan in float32, np.float32 at every operation: what the kernel must equal BIT FOR BIT.
  tail64         ts_range_point_tail_forward in float64 with the ingredients of its bar.
  range_stage    taseg_amd.data.range.build_range_inputs, the reference's own precisions operation by operation.

Bar of the tail's value.  The kernel forms d = the trilinear sum (t_d live products), r = the bilinear sum (t_r live products), d + r,
the BatchNorm term bn (elementwise: subtract, two products, add - the 8 u S_bn of tests/test_gpu_spvcnn_kernels.py), relu, and
(d + r) + relu(bn).  To first order: t_d u S_d + t_r u S_r (oracle/points64.py: a float32 sum of t products in any order) + u |d + r|
(the addition of the two sums) + 8 u S_bn + u (|d + r| + relu(bn)) (the last addition); SLACK covers the second order; a half result
carries the bar through one rounding to half (points64.bar_half).
"""
import numpy as np

from oracle import points64 as P64

F32 = np.float32
U = P64.U
BN_OPS = 8                    # roundings allowed to the elementwise BatchNorm term, as in the SPVCNN tail test
ERR_BATCH, ERR_NONFINITE, ERR_OUTSIDE = 1, 2, 4


# ------------------------------------------------------------------------------------------------------------------ the plan
def pixels32(pxpy, h, w):
    """(x, y) int32 of rpvnet.py:88: ((p + 1) / 2 * (size - 1)).int() in float32, one rounding per operation"""
    p = np.asarray(pxpy, dtype=F32)
    with np.errstate(invalid="ignore"):
        x = (((p[:, 1] + F32(1)) / F32(2)) * F32(w - 1)).astype(np.int32)
        y = (((p[:, 2] + F32(1)) / F32(2)) * F32(h - 1)).astype(np.int32)
    return x, y


def plan32(pxpy, b, h, w):
    """(pix [n] int32, bidx [n, 8] int32, bw [n, 8] float32, err int): ts_range_plan, float32 operation by operation"""
    p = np.asarray(pxpy, dtype=F32)
    n = len(p)
    bf, px, py = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        bad_b = ~((bf >= 0) & (bf < b)) | (bf != np.trunc(bf))
        bad_f = ~(np.isfinite(px) & np.isfinite(py))
        bad_r = ~bad_f & ((px < -1) | (px > 1) | (py < -1) | (py > 1))
    flag = bad_b * ERR_BATCH + bad_f * ERR_NONFINITE + bad_r * ERR_OUTSIDE
    ok = flag == 0
    pix = np.full(n, -1, dtype=np.int32)
    bidx = np.full((n, 8), -1, dtype=np.int32)
    bw = np.zeros((n, 8), dtype=F32)
    q = p[ok]
    base = q[:, 0].astype(np.int32) * np.int32(h * w)
    x, y = pixels32(q, h, w)
    pix[ok] = base + y * np.int32(w) + x
    ix = ((q[:, 1] + F32(1)) * F32(w) - F32(1)) / F32(2)
    iy = ((q[:, 2] + F32(1)) * F32(h) - F32(1)) / F32(2)
    assert ix.dtype == F32 and iy.dtype == F32
    fx0, fy0 = np.floor(ix), np.floor(iy)
    fx1, fy1 = fx0 + F32(1), fy0 + F32(1)
    x0, y0 = fx0.astype(np.int32), fy0.astype(np.int32)
    wx, wy, xs, ys = (fx1 - ix, ix - fx0), (fy1 - iy, iy - fy0), (x0, x0 + 1), (y0, y0 + 1)
    ci, cw = np.full((len(q), 8), -1, dtype=np.int32), np.zeros((len(q), 8), dtype=F32)
    for k, (jy, jx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):          # nw, ne, sw, se
        inside = (xs[jx] >= 0) & (xs[jx] < w) & (ys[jy] >= 0) & (ys[jy] < h)
        ci[inside, k] = (base + ys[jy] * np.int32(w) + xs[jx])[inside]
        cw[inside, k] = (wx[jx] * wy[jy]).astype(F32)[inside]
    bidx[ok], bw[ok] = ci, cw
    err = int(np.bitwise_or.reduce(flag.astype(np.int64))) if n else 0
    return pix, bidx, bw, err


def bilinear64(pxpy, b, h, w):
    """(bidx [n, 8] int32, bw [n, 8] float64) of the rows plan32 keeps: the same corners, the weights in double from the float32
    px / py - what grid_sample computes, without its roundings"""
    p = np.asarray(pxpy, dtype=F32).astype(np.float64)
    ix, iy = ((p[:, 1] + 1) * w - 1) / 2, ((p[:, 2] + 1) * h - 1) / 2
    x0, y0 = np.floor(ix), np.floor(iy)
    base = p[:, 0].astype(np.int64) * h * w
    bidx, bw = np.full((len(p), 8), -1, dtype=np.int32), np.zeros((len(p), 8))
    for k, (jy, jx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xx, yy = x0 + jx, y0 + jy
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        wgt = (ix - x0 if jx else x0 + 1 - ix) * (iy - y0 if jy else y0 + 1 - iy)
        bidx[inside, k] = (base + yy * w + xx)[inside].astype(np.int32)
        bw[inside, k] = wgt[inside]
    return bidx, bw


def coord_err(size):
    """|float32 ix - exact ix| for ix = ((p + 1) size - 1) / 2 and |p| <= 1: p + 1 errs by <= 2 u, the product by <= 2 u size more
    (and carries the first error size-fold: 4 u size), the subtraction by <= 2 u size more, the halving is exact: 3 u size.  An
    evaluation as (p + 1) (size / 2) - 0.5 (three operations of the same magnitudes) meets the same figure."""
    return P64.SLACK * 3.0 * size * U


def bar_grid_value(fmax, h, w):
    """|a float32 bilinear read - the exact one| for a map with |f| <= fmax.  The interpolant (zeros padding included) is continuous
    and piecewise bilinear in (ix, iy) with slope <= 2 fmax along either axis - also across a pixel border, where the float32 floor
    may pick the neighbouring cell -, so the coordinate errors move the value by <= 2 fmax (coord_err(w) + coord_err(h)); the
    weights' two subtractions and product and the sum of four products add <= 8 u fmax."""
    return 2.0 * fmax * (coord_err(w) + coord_err(h)) + 8.0 * U * fmax


# ------------------------------------------------------------------------------------------------------------------ the tail
def tail64(y, vox, idx, w, pixrows, bidx, bw, mean, invstd, gamma, beta):
    """(ref [n, c], bar [n, c], bn [n, c], bn_bar [n, c], t_d [n], t_r [n]) of ts_range_point_tail_forward in float64"""
    d, t_d, s_d = P64.devoxelize_forward64(vox, idx, w)
    r, t_r, s_r = P64.devoxelize_forward64(pixrows, bidx, bw)
    y64 = P64.up(y)
    is64 = P64.up(invstd)
    bn = (y64 - mean) * is64 * gamma + beta
    s_bn = (np.abs(y64) + np.abs(mean)) * is64 * np.abs(gamma) + np.abs(beta)
    bn_bar = BN_OPS * U * s_bn
    relu = np.maximum(bn, 0.0)
    ref = (d + r) + relu
    bar = P64.bar_sum(t_d, s_d) + P64.bar_sum(t_r, s_r) + bn_bar + P64.SLACK * U * (2 * np.abs(d + r) + relu)
    return ref, bar, bn, bn_bar, t_d, t_r


def tail_inputs(n, c, half, seed, b=2, h=4, w=128, m=37):
    """inputs of one tail case: a random trilinear map (a fifth of the rows without a corner), points over b maps of h x w with
    the hand-placed rows of `edge_pxpy` first, standard-normal rows"""
    rs = np.random.RandomState(seed)
    idx, tw = P64.random_map(n, m, seed)
    idx[1::5] = -1
    store = np.float16 if half else F32
    pxpy = random_pxpy(n, b, seed)
    y = rs.randn(n, c).astype(store)
    vox = rs.randn(m, c).astype(store)
    rows = rs.randn(b * h * w, c).astype(store)
    mean, invstd = (rs.randn(c) * 0.3).astype(F32), (rs.rand(c) + 0.5).astype(F32)
    gamma = ((rs.rand(c) + 0.5) * np.where(np.arange(c) % 3 == 0, -1.0, 1.0)).astype(F32)
    beta = (rs.randn(c) * 0.5).astype(F32)
    return idx, tw, m, pxpy, y, vox, rows, mean, invstd, gamma, beta


def edge_pxpy(b):
    """hand-placed rows: the four image corners (px = +-1, py = +-1) and the centre in sample 0, two edge rows in the LAST sample"""
    rows = [[0, -1, -1], [0, 1, 1], [0, -1, 1], [0, 1, -1], [0, 0, 0], [b - 1, 1, 0.25], [b - 1, -0.5, -1]]
    return np.array(rows, dtype=F32)


def random_pxpy(n, b, seed):
    """[n, 3] float32, batch-sorted: the edge rows (as many as fit), then uniform rows; sample b - 2 (if b > 2) gets no row"""
    rs = np.random.RandomState(7000 + seed)
    edge = edge_pxpy(b)[:n]
    k = n - len(edge)
    batches = [s for s in range(b) if not (b > 2 and s == b - 2)]
    rest = np.stack([rs.choice(batches, size=k).astype(F32), rs.uniform(-1, 1, k).astype(F32), rs.uniform(-1, 1, k).astype(F32)], 1)
    out = np.concatenate([edge, rest.reshape(k, 3)]).astype(F32)
    return np.ascontiguousarray(out[np.argsort(out[:, 0], kind="stable")])


def kitti_pxpy(h=64, w=2048):
    """every (column, ring) pair the dataset can produce, as get_range_image writes them (semantickitti_fusion.py:103-104):
    px = 2 (x / (w - 1) - 0.5), py = 2 (y / (h - 1) - 0.5) in float64, rounded to float32 once.  Returns (pxpy [w + h, 3] with batch 0 -
    the w columns at row 0, then the h rows at column 0 -, the integer columns, the integer rows)"""
    xs, ys = np.arange(w), np.arange(h)
    px = (2.0 * (xs.astype(np.float64) / (w - 1.0) - 0.5)).astype(F32)
    py = (2.0 * (ys.astype(np.float64) / (h - 1.0) - 0.5)).astype(F32)
    cols = np.stack([np.zeros(w, F32), px, np.full(w, py[0], F32)], 1)
    rows = np.stack([np.zeros(h, F32), np.full(h, px[0], F32), py], 1)
    return np.concatenate([cols, rows]).astype(F32), xs, ys


# ------------------------------------------------------------------------------------------------------------- the range stage
STAGE_ERR_BATCH, STAGE_ERR_RING, STAGE_ERR_NONFINITE = 1, 8, 16


def range_stage32(points, batch, cuts, h=64, w=2048):
    """ts_range_inputs in numpy, the reference's own precisions operation by operation (semantickitti_fusion.py:72-111 per sample,
    collate_batch's padding and .float()), the float32 arctan2 taken as (float32)arctan2 of the doubles.
    points [n, >= 5] float32 (x, y, z, reflectivity, ring), batch [n] int, cuts [B] float64.
    Returns dict(col, row int32 [n] (-1 where the row is left out), pxpy float32 [n, 3], image float32 [B, 5, h, w], err int)."""
    p = np.asarray(points, dtype=F32)
    batch = np.asarray(batch).astype(np.int64)
    n, nb = len(p), len(cuts)
    col, row = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    pxpy = np.full((n, 3), np.nan, dtype=F32)
    pxpy[:, 0] = batch.astype(F32)
    image = np.zeros((nb, 5, h, w), dtype=F32)
    finite = np.isfinite(p[:, [0, 1, 2, 4]]).all(1)
    bad_b = (batch < 0) | (batch >= nb)
    with np.errstate(invalid="ignore"):
        bad_ring = finite & ~((p[:, 4] <= F32(h - 1)) & (np.round(p[:, 4]) >= 0))
    err = (STAGE_ERR_BATCH if bad_b.any() else 0) | (STAGE_ERR_RING if bad_ring.any() else 0) | (0 if finite.all() else
                                                                                                 STAGE_ERR_NONFINITE)
    keep = finite & ~bad_b & ~bad_ring
    for b in range(nb):
        rows = np.flatnonzero(keep & (batch == b))
        q = p[rows]
        with np.errstate(divide="ignore"):
            depth = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])        # np.linalg.norm on float32 rows
            inv = F32(1.0) / depth
        yaw = np.arctan2(q[:, 1].astype(np.float64), -q[:, 0].astype(np.float64)).astype(F32) + F32(cuts[b])
        yaw = yaw % F32(2 * np.pi) - F32(np.pi)
        proj_x = F32(0.5) * (yaw / F32(np.pi) + F32(1.0))
        proj_x = proj_x * F32(w - 1)
        assert yaw.dtype == F32 and proj_x.dtype == F32 and depth.dtype == F32
        cx, ry = np.round(proj_x).astype(np.int32), np.round(q[:, 4]).astype(np.int32)
        col[rows], row[rows] = cx, ry
        pxpy[rows, 1] = (2.0 * (cx / (w - 1) - 0.5)).astype(F32)
        pxpy[rows, 2] = (2.0 * (ry / (h - 1) - 0.5)).astype(F32)
        rng, refl, xyz = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
        rng[ry, cx] = inv                                                   # numpy's fancy assignment: the last row wins
        refl[ry, cx] = q[:, 3]
        xyz[ry, cx] = q[:, :3]
        with np.errstate(over="ignore"):
            image[b] = np.concatenate([(25 * (rng - 0.4))[None], (20 * (refl - 0.5))[None], xyz.transpose(2, 0, 1)]).astype(F32)
    return dict(col=col, row=row, pxpy=pxpy, image=image, err=err)


def proj_x64(points, batch, cuts, w=2048):
    """the column coordinate before rounding, the whole chain in float64 with the exact constants, from the float32 rows"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    yaw = np.arctan2(p[:, 1], -p[:, 0]) + np.asarray(cuts, dtype=np.float64)[np.asarray(batch).astype(np.int64)]
    yaw = yaw % (2 * np.pi) - np.pi
    return 0.5 * (yaw / np.pi + 1.0) * (w - 1)


def stage_delta(w=2048, atan_ulps=4.0):
    """How far, in columns, a float32 evaluation of the chain whose arctan2 errs by `atan_ulps` float32 ulps of pi may sit from
    proj_x64.  ulp(pi) = 2^-22 (values in [2, 4)).  In radians: the arctan2 (atan_ulps 2^-22); the cut rounded to float32 (half an
    ulp of a value below 4: 2^-23); the sum (below 8: 2^-22); the remainder (fmod is exact; the + 2 pi of a negative one rounds:
    2^-22; the divisor is (float)(2 pi), not 2 pi, one wrap: |f(2 pi) - 2 pi|); the subtraction of (float)pi (its own error, and a
    rounding below 4: 2^-23).  yaw / (float)pi errs relatively by |f(pi) - pi| / pi and one rounding of a value <= 1 (2^-24); + 1
    rounds a value <= 2 (2^-24); the halving is exact; the product with w - 1 rounds a value < 2048 (2^-14)."""
    f_pi, f_2pi = float(F32(np.pi)), float(F32(2 * np.pi))
    e_yaw = atan_ulps * 2.0 ** -22 + 2.0 ** -23 + 2.0 ** -22 + 2.0 ** -22 + abs(f_2pi - 2 * np.pi) + abs(f_pi - np.pi) + 2.0 ** -23
    e_unit = e_yaw / np.pi + abs(f_pi - np.pi) / np.pi + 2 * 2.0 ** -24
    return 0.5 * (w - 1) * e_unit + 2.0 ** -14
