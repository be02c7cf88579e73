"""References of the interpolation decoder (csrc/fid.hip) and of BatchNorm -> residual -> LeakyReLU (csrc/bn.hip) - test infrastructure,
not product code; numpy (and torch in double for the BatchNorm part), nothing of taseg_amd imported.

Maps are ROWS here: x [T, H, W, Ca], x1 [T, H, W, Cb], three coarse maps [T, hk, wk, Cl]; cat [T, H, W, Ca + Cb + 3 Cl].

1. `tables(out, inn, dtype)`: index i0, lambda and the lower bounds `first` of one axis under the header's rule
       scale = (inn - 1) / (out - 1) (0 when out == 1);  r = scale * y;  i0 = trunc(r) (at most inn - 1);  lam = r - i0
   in float32 (every operation rounded on its own: numpy float32 scalars / arrays) or in float64.
2. `upcat(x, x1, coarse, dtype)`: the decoder,  val = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)  with the four products and
   three sums in that order.  float32: the restatement the kernel must equal bit for bit (half rows: widened first, one rounding at the
   end - `store`).  float64: the exact evaluation the bars are measured against.
3. `upcat_adjoint(grad_cat, channels, sizes, grad_res, dtype, lanes)`: the gather under the header's addition order - fine row y of a
   coarse row's range goes to partial (y - y_lo) % S, a partial adds ascending y, then x, then corner row, then corner column, from 0;
   the partials are added in order; S = `row_split`.  float64 (S irrelevant up to rounding): the exact adjoint.
4. `forward_bar` / `adjoint_bar`: the error bars, derived below.
5. `bn_leaky_ref64`: LeakyReLU(BatchNorm_train(x) [+ residual]) and its backward in float64 with the S of every result, from
   oracle/bn64.py's bn_ref64: the LeakyReLU's backward is the BatchNorm's backward of g * (out > 0 ? 1 : slope).

THE BARS, u = 2^-24.
Interpolation.  scale carries one rounding and r = fl(scale * y) a second: |r32 - r| <= (2u + u^2) r <= 3u (inn - 1) =: delta, growing
with the source coordinate.  i0 and lam = r - i0 are exact functions of r32 (the subtraction of a float's integer part is exact), so
the float32 rule evaluates the piecewise-linear interpolant at a coordinate off by at most delta per axis; the interpolant is
continuous, with slope at most 2 max|v| per axis (the difference of two neighbours), also across a cell boundary where i0 itself
changes: |val(r32) - val(r)| <= 2 max|v| (delta_h + delta_w).  h0 = fl(1 - lam) adds u per axis (times max|v|); the four products and
three sums of convex weights add at most (2u + 2u) max|v| (1 + O(u)).  In all
    |val32 - val64| <= max|v| (2 (delta_h + delta_w) + 8u)                                     forward_bar, per level
and a half store adds 2^-11 |val| + 2^-25.  The two copied slices are exact.
Adjoint.  A coefficient ly * lx inherits the same coordinate error: |coef32 - coef| <= delta_h + delta_w + 4u (two lambdas of at most 1,
a complement's rounding each, the product's rounding); where i0 differs between the two evaluations a corner's weight of at most delta
moves to the neighbouring coarse pixel, inside the same figure.  A coarse pixel with n contributing fine pixels (the size of its range)
therefore sees  n (delta_h + delta_w + 4u) max|g|  from the coefficients, and the sum itself - each term two roundings (the
coefficient's product is counted above, the product with g, and g's own sum with grad_res: c = 3), a chain of at most n_terms + S
additions - gamma(n_terms + S + 3) sum|terms| <= (n_terms + S + 3) u sum|coef| |g| / (1 - ...):
    |adj32 - adj64| <= n (delta_h + delta_w + 4u) max|g| + 1.01 (4 n + S + 3) u * adjoint64(|g|)    adjoint_bar, per coarse pixel
(4 n: every fine pixel of the range can name the coarse pixel through at most four corners).
BatchNorm: LAMBDA(n, c) of oracle/bn64.py plus 2 (the slope's product in either direction), times u times S."""
import numpy as np

U32, U16, SUB = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25


def tables(out, inn, dtype=np.float32):
    """(i0 [out] int, lam [out] dtype, first [inn + 1] int) of one axis"""
    f = dtype
    scale = f(inn - 1) / f(out - 1) if out > 1 else f(0)
    r = (f(scale) * np.arange(out).astype(f)).astype(f)
    i0 = np.minimum(np.trunc(r).astype(np.int64), inn - 1)
    lam = (r - i0.astype(f)).astype(f)
    first = np.searchsorted(i0, np.arange(inn + 1), side="left")
    return i0, lam, first


def row_split(H, hk, Cl, lanes):
    return max(1, min(8, (H // hk) // 2, 256 // (Cl // lanes)))


def store(a, like):
    """the one rounding at a store of `like`'s dtype"""
    return a.astype(like.dtype)


def upcat(x, x1, coarse, dtype=np.float32):
    """(cat, [res_2, res_3, res_4]) in `dtype` arithmetic (not yet rounded to the storage type)"""
    f = dtype
    T, H, W, _ = x.shape
    res = []
    for v in coarse:
        v = v.astype(f)
        i0h, lh, _ = tables(H, v.shape[1], f)
        i0w, lw, _ = tables(W, v.shape[2], f)
        ph, pw = (i0h < v.shape[1] - 1).astype(np.int64), (i0w < v.shape[2] - 1).astype(np.int64)
        h1, w1 = lh[None, :, None, None], lw[None, None, :, None]
        h0, w0 = (f(1) - h1).astype(f), (f(1) - w1).astype(f)
        rows0, rows1 = v[:, i0h], v[:, i0h + ph]
        top = (w0 * rows0[:, :, i0w] + w1 * rows0[:, :, i0w + pw]).astype(f)
        bot = (w0 * rows1[:, :, i0w] + w1 * rows1[:, :, i0w + pw]).astype(f)
        res.append((h0 * top + h1 * bot).astype(f))
    return np.concatenate([x.astype(f), x1.astype(f)] + res, axis=3), res


def upcat_adjoint(grad_cat, channels, sizes, grad_res=None, dtype=np.float32, lanes=4):
    """(grad_x, grad_x1, [grad_xk]) in `dtype` arithmetic under the header's addition order"""
    f = dtype
    ca, cb, cl = channels
    T, H, W, _ = grad_cat.shape
    out = []
    for k, (hk, wk) in enumerate(sizes):
        i0h, lh, fh = tables(H, hk, f)
        i0w, lw, _ = tables(W, wk, f)
        S = row_split(H, hk, cl, lanes)
        g = grad_cat[..., ca + cb + k * cl: ca + cb + (k + 1) * cl].astype(f)
        if grad_res is not None and grad_res[k] is not None:
            g = (g + grad_res[k].astype(f)).astype(f)
        part = np.zeros((S, T, hk, wk, cl), dtype=f)
        for y in range(H):
            ly = (f(1) - lh[y], lh[y])
            ry = (i0h[y], i0h[y] + (1 if i0h[y] < hk - 1 else 0))
            for xx in range(W):
                lx = (f(1) - lw[xx], lw[xx])
                rx = (i0w[xx], i0w[xx] + (1 if i0w[xx] < wk - 1 else 0))
                gv = g[:, y, xx]
                for cy in range(2):
                    s = (y - fh[max(ry[cy] - 1, 0)]) % S
                    for cx in range(2):
                        wgt = f(f(ly[cy]) * f(lx[cx]))
                        part[s, :, ry[cy], rx[cx]] = (part[s, :, ry[cy], rx[cx]] + (wgt * gv).astype(f)).astype(f)
        total = part[0]
        for s in range(1, S):
            total = (total + part[s]).astype(f)
        out.append(total)
    return grad_cat[..., :ca].astype(f), grad_cat[..., ca:ca + cb].astype(f), out


def covered_pairs(H, hk):
    """brute force over one axis: for every coarse index r the fine indices of its range [first[max(r - 1, 0)], first[r + 1]) and, of
    those, the (fine, corner) pairs that name r -> (list of (y, corner, r) the ranges reach, list of all (y, corner, r) there are)"""
    i0, _, first = tables(H, hk)
    reached = []
    for r in range(hk):
        for y in range(first[max(r - 1, 0)], first[r + 1]):
            for corner in range(2):
                if i0[y] + (corner if i0[y] < hk - 1 else 0) == r:
                    reached.append((y, corner, r))
    every = [(y, corner, int(i0[y] + (corner if i0[y] < hk - 1 else 0))) for y in range(H) for corner in range(2)]
    return reached, every


def forward_bar(coarse, H, W):
    """per level: the bound on |val32 - val64| (a scalar each); half storage adds U16 |val| + SUB"""
    bars = []
    for v in coarse:
        dh, dw = 3 * U32 * (v.shape[1] - 1), 3 * U32 * (v.shape[2] - 1)
        bars.append(float(np.abs(v.astype(np.float64)).max()) * (2 * (dh + dw) + 8 * U32))
    return bars


def adjoint_bar(grad_cat, channels, sizes, grad_res=None, lanes=4):
    """per level: the bound on |adj32 - adj64| per coarse pixel and channel [T, hk, wk, Cl]"""
    ca, cb, cl = channels
    T, H, W, _ = grad_cat.shape
    absg = np.abs(grad_cat.astype(np.float64))
    absr = None if grad_res is None else [None if g is None else np.abs(g.astype(np.float64)) for g in grad_res]
    _, _, sums = upcat_adjoint(absg, channels, sizes, absr, np.float64, lanes)
    bars = []
    for k, (hk, wk) in enumerate(sizes):
        _, _, fh = tables(H, hk)
        _, _, fw = tables(W, wk)
        nh = np.array([fh[r + 1] - fh[max(r - 1, 0)] for r in range(hk)])
        nw = np.array([fw[c + 1] - fw[max(c - 1, 0)] for c in range(wk)])
        n = (nh[:, None] * nw[None, :])[None, :, :, None].astype(np.float64)
        gmax = absg[..., ca + cb + k * cl: ca + cb + (k + 1) * cl].max() + (0.0 if absr is None or absr[k] is None else absr[k].max())
        delta = 3 * U32 * (hk - 1) + 3 * U32 * (wk - 1) + 4 * U32
        S = row_split(H, hk, cl, lanes)
        bars.append(n * delta * gmax + 1.01 * (4 * n + S + 3) * U32 * sums[k])
    return bars


def bn_leaky_ref64(x, residual, weight, bias, slope, eps, gy, out):
    """LeakyReLU_slope(BatchNorm_train(x) [+ residual]) in float64 (torch, on the operands' device) and its backward for the gradient gy,
    the branch of every element taken from `out` - the tensor the kernel stored, which the forward check certifies and on which
    leaky_relu_backward decides (out > 0 ? 1 : slope).  Returns bn_ref64's two tuples (y, gx, gres, gw, gb, mean, var), (S of each) and the
    masked gradient g = gy * (out > 0 ? 1 : slope)."""
    import torch
    from oracle.bn64 import bn_ref64
    pos = out > 0
    g = torch.where(pos, gy.double(), gy.double() * slope)
    (y, gx, gres, gw, gb, mean, var), (sy, sgx, sgres, sgw, sgb, smean, svar) = bn_ref64(x, residual, weight, bias, False, eps, g)
    y = torch.where(y > 0, y, y * slope)
    return (y, gx, gres, gw, gb, mean, var), (sy, sgx, sgres, sgw, sgb, smean, svar), g
