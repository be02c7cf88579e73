"""Float64 reference of the two-pass sparse convolution (csrc/conv_pairs.hip, conv_pairs_h.hip, conv_pairs_s.hip), stage by stage,
with the rounding bars of every kernel family - test infrastructure, not product code.  Plain numpy; nothing of taseg_amd is imported.
tests/test_conv64_host.py checks this file (helpers against brute force, a float32 emulation of every stage inside its bar, ten
emulated wrong kernels rejected); tests/test_gpu_conv_float64.py holds the kernels against it.  The cases (count vectors, channel
pairs, operand families) live here so that both files run the same ones.

Stages (include/taseg_hip.h):
    pass 1   z[p, :] = x[nbmaps[p][gather_col], :] @ W_k(p)            pair_gemm64
    pass 2   y[j, :] = sum_k z[pos[k, j], :], k ascending, -1 skipped    gather_sum64
    wgrad    dW[k]   = sum_{p of k} a[nbmaps[p][col_a], :]^T b[nbmaps[p][1 - col_a], :]        wgrad64
Every stage function takes operands already cast to float64 and returns the value with the ingredients of its bar: per output
element S = sum |a_i| |b_i| and N = the number of products a_i b_i that are not zero.

The bars.  u = 2^-24 is one float32 rounding.  The matrix instructions document no rounding for their internal additions, so every
addition inside an MFMA is charged 2u of S - that covers chopping as well as round-to-nearest, and, S bounding every term and
every partial sum, an alignment of the addends to the largest exponent too.  Plain VALU additions are charged u.  SLACK = 1.01
stands for the second-order terms, TINY = 2^-149 is added per product that may underflow.  An addition with an exact zero commits
no rounding: the kernels stage foreign rows, padding columns and the rows behind a tile's last pair as zeros (pair_gemm_kernel's
load_regs, the `rr < np` selects of the fast, split and half kernels), and the accumulators start at +0.  So the count of additions
that round is the count N of non-zero products, not the padded length of the reduction: N = c_red for dense operands, 1 for a
one-hot row - this is the "tighter count from the kernel's own order", read from those staging rules.

  pass 1, f32 MFMA (v_mfma_f32_16x16x4_f32; conv_impl 2, 3, 4, 5): N products, each rounded once (u |a b|) or fused, joined by at
  most N additions:                                |z - z64| <= SLACK N 2u S + N TINY
  pass 1, split bf16 (conv_impl 0, 6, the direct-planes kernel): every operand is x = h + m + l exactly, h = bf16(x),
  m = bf16(x - h), l = x - h - m, |m| <= 2^-9 |x|, |l| <= 2^-18 |x|.  TS_SPLIT_MMA adds six of the nine products, each exact in
  float32 (8 x 8 bits), in the order al bh, ah bl, am bm, am bh, ah bm, ah bh per 32-slice.  The three dropped ones:
  |am bl| + |al bm| + |al bl| <= (2 2^-27 + 2^-36) |a b| < 0.25 u |a b|.  Six terms per product, 6 N additions, partial sums bounded
  by S' = (1 + 2^-8)^2 S:                          |z - z64| <= SLACK (6 N 2u + 0.25 u) S' + 6 N TINY
  pass 2, fp32 (VALU, acc = +0, then k ascending): the first addition 0 + z is exact, L - 1 round:
                                                   |y - sum z| <= SLACK (L - 1) u sum|z|
  with the device's own Z cast up; L = 0: exactly +0; L = 1: the bits of the Z row (a -0 there reads +0: 0 + -0).
  wgrad, offset k with n_k pairs: A_k = m N + ceil(n_k / 128) + 1 additions, m = 1 (f32 MFMA, half) or 6 (split); chunks are at
  least 128 pairs long (ts_wgrad_plan), so the offset is cut into at most ceil(n_k / 128) + 1 partial tiles, which the ordered sum
  or the atomics add:                              |dW - dW64| <= SLACK A_k 2u S (+ 0.25 u S' for split) + n_k TINY
  n_k = 0: exactly +0 everywhere.
  half storage: operands are halves cast up, products exact in float32 (11 x 11 bits), float32 accumulation, ONE rounding of the
  result to half (2^-11 relative, or half the subnormal spacing 2^-25):
    pass 1                                         |z - z64| <= 2^-11 |z64| + SLACK N 2u S + 2^-25
    pass 2                                         |y - sum z| <= 2^-11 |sum z| + SLACK (L - 1) u sum|z| + 2^-25
    wgrad                                          the f32 bar with m = 1 (float32 result)
  A half result whose reference is 65520 or more in magnitude must be inf of its sign (closer than the bar to 65520: either).
"""
import math
import zlib

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
SLACK = 1.01
HALF_U = 2.0 ** -11
HALF_SUB = 2.0 ** -25            # half the spacing 2^-24 of the half subnormals
HALF_INF = 65520.0               # the smallest magnitude that rounds to inf
HALF_MAX = 65504.0
SPLIT_SUM = (1.0 + 2.0 ** -8) ** 2


# ------------------------------------------------------------------------------------------------------------------ checks

class Checks:
    """every check of a case is evaluated; done() prints one line of worst error / bar per stage and fails with the list of those that missed"""

    def __init__(self, cid, title="conv_float64"):
        self.cid, self.title, self.missed, self.n, self.ratios = cid, title, [], 0, {}

    def le(self, stage, what, value, bound):
        self.n += 1
        ratio = value / bound if bound > 0 else (0.0 if value <= bound else math.inf)
        self.ratios[stage] = max(self.ratios.get(stage, 0.0), ratio)
        if not value <= bound:
            self.missed.append(f"{stage} {what}: {value:.3e} > {bound:.3e}")

    def true(self, stage, what, ok):
        self.n += 1
        if not ok:
            self.missed.append(f"{stage} {what}")

    def lines(self):
        """one line per stage: the worst error / bar of the case in that stage"""
        out = [f"{self.title} {self.cid:<40} {stage:<12} error / bar {v:.3f}" for stage, v in self.ratios.items()]
        return out + [f"{self.title} {self.cid:<40} {self.n} checks, {len(self.missed)} missed"]

    def done(self):
        print("\n".join(self.lines()))
        assert not self.missed, f"{self.cid}: {len(self.missed)} of {self.n} checks missed\n  " + "\n  ".join(self.missed[:40])


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------------------------- rulebook

def check_rulebook(nbmaps, nboffs, pos_out, pos_in, n_in, n_out):
    """every index a kernel will follow lies inside its array (host assertion; the device test repeats it before its first launch)"""
    nbmaps, nboffs = np.asarray(nbmaps), np.asarray(nboffs)
    k, p = len(nboffs) - 1, int(nboffs[-1])
    assert nbmaps.dtype == np.int32 and nboffs.dtype == np.int32 and nbmaps.shape == (p, 2)
    assert nboffs[0] == 0 and (np.diff(nboffs) >= 0).all()
    assert pos_out.shape == (k, n_out) and pos_in.shape == (k, n_in) and pos_out.dtype == np.int32 and pos_in.dtype == np.int32
    if p:
        assert nbmaps[:, 0].min() >= 0 and nbmaps[:, 0].max() < n_in, "input row out of range"
        assert nbmaps[:, 1].min() >= 0 and nbmaps[:, 1].max() < n_out, "output row out of range"
    for pos in (pos_out, pos_in):
        assert pos.min(initial=-1) >= -1 and pos.max(initial=-1) < p, "position out of range"
        live = pos[pos >= 0]
        assert len(live) == p and len(np.unique(live)) == p, "every pair has exactly one position"
    for kk in range(k):
        lo, hi = int(nboffs[kk]), int(nboffs[kk + 1])
        for pos, col in ((pos_out, 1), (pos_in, 0)):
            rows = np.nonzero(pos[kk] >= 0)[0]
            assert len(rows) == hi - lo and ((pos[kk][rows] >= lo) & (pos[kk][rows] < hi)).all()
            assert (nbmaps[pos[kk][rows], col] == rows).all(), "a position points at another row's pair"
    return True


def make_rulebook(counts, n_in, n_out, seed):
    """(nbmaps [P, 2] int32 (input row, output row), nboffs [K + 1] int32, pos_out [K, n_out], pos_in [K, n_in]) with counts[k] pairs
    in offset k: output rows distinct and ascending, input rows distinct, as a kernel map has them.  pos_*: pair index or -1."""
    rs = rng("rulebook", tuple(int(c) for c in counts), n_in, n_out, seed)
    k = len(counts)
    nboffs = np.zeros(k + 1, dtype=np.int32)
    nboffs[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    p = int(nboffs[-1])
    nbmaps = np.zeros((p, 2), dtype=np.int32)
    pos_out = np.full((k, n_out), -1, dtype=np.int32)
    pos_in = np.full((k, n_in), -1, dtype=np.int32)
    for kk, c in enumerate(counts):
        assert 0 <= c <= min(n_in, n_out), "more pairs in an offset than rows"
        out_rows = np.sort(rs.permutation(n_out)[:c])
        in_rows = rs.permutation(n_in)[:c]
        at = int(nboffs[kk]) + np.arange(c)
        nbmaps[at, 0], nbmaps[at, 1] = in_rows, out_rows
        pos_out[kk, out_rows], pos_in[kk, in_rows] = at, at
    check_rulebook(nbmaps, nboffs, pos_out, pos_in, n_in, n_out)
    return nbmaps, nboffs, pos_out, pos_in


# ------------------------------------------------------------------------------------------------------------------ stages

def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float64, "operands are cast to float64 by the caller"
    return a


def pair_gemm64(x, w, nbmaps, nboffs, gather_col, transposed):
    """(z, S, N), each [P, c_out].  w [K, c_red, c_out], or [K, c_out, c_red] when transposed."""
    x, w = _f64(x), _f64(w)
    c_out = w.shape[1] if transposed else w.shape[2]
    p = int(nboffs[-1])
    z, s, n = (np.zeros((p, c_out)) for _ in range(3))
    for k in range(len(nboffs) - 1):
        lo, hi = int(nboffs[k]), int(nboffs[k + 1])
        if hi > lo:
            rows = x[nbmaps[lo:hi, gather_col]]
            wk = w[k].T if transposed else w[k]
            z[lo:hi] = rows @ wk
            s[lo:hi] = np.abs(rows) @ np.abs(wk)
            n[lo:hi] = (rows != 0).astype(np.float64) @ (wk != 0).astype(np.float64)
    return z, s, n


def gather_sum64(z, pos):
    """(y, A, L): y[j] = sum over the live positions of z, A[j] = the same of |z| (both [n, c]), L[j] the live count [n]"""
    z = _f64(z)
    k, n = pos.shape
    y, a = np.zeros((n, z.shape[1])), np.zeros((n, z.shape[1]))
    live_count = np.zeros(n, dtype=np.int64)
    for kk in range(k):
        live = pos[kk] >= 0
        y[live] += z[pos[kk][live]]
        a[live] += np.abs(z[pos[kk][live]])
        live_count += live
    return y, a, live_count


def wgrad64(a, b, nbmaps, nboffs, col_a):
    """(dW, S, N, n_k): dW, S, N [K, c_a, c_b], n_k [K]"""
    a, b = _f64(a), _f64(b)
    k = len(nboffs) - 1
    dw, s, n = (np.zeros((k, a.shape[1], b.shape[1])) for _ in range(3))
    for kk in range(k):
        lo, hi = int(nboffs[kk]), int(nboffs[kk + 1])
        if hi > lo:
            ra, rb = a[nbmaps[lo:hi, col_a]], b[nbmaps[lo:hi, 1 - col_a]]
            dw[kk] = ra.T @ rb
            s[kk] = np.abs(ra).T @ np.abs(rb)
            n[kk] = (ra != 0).astype(np.float64).T @ (rb != 0).astype(np.float64)
    return dw, s, n, np.diff(np.asarray(nboffs)).astype(np.int64)


def round_half(v):
    """float64 -> the IEEE half nearest to it (ties to even), as a float64: subnormals kept (spacing 2^-24), 65520 and above -> inf,
    the sign of a zero kept, NaN passed on.  Scaling by a power of two is exact and numpy.rint rounds ties to even."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.frexp(np.where(np.isfinite(a), a, 1.0))[1] - 1            # a = f 2^e, 1 <= f < 2
        q = np.ldexp(1.0, np.maximum(e, -14) - 10)                        # the spacing of the halves around a
        r = np.rint(a / q) * q
        r = np.where(r > HALF_MAX, np.inf, r)
        r = np.where(np.isfinite(a), r, a)
    return np.copysign(r, v)


# -------------------------------------------------------------------------------------------------------------------- bars

def bar_pass1_f32(s, n):
    return SLACK * n * 2 * U * s + n * TINY


def bar_pass1_split(s, n):
    return SLACK * (6 * n * 2 * U + 0.25 * U) * (SPLIT_SUM * s) + 6 * n * TINY


def bar_pass1_half(z64, s, n):
    return HALF_U * np.abs(z64) + SLACK * n * 2 * U * s + HALF_SUB


def bar_pass2(a, live):
    return SLACK * np.maximum(live - 1, 0)[:, None] * U * a


def bar_pass2_half(y64, a, live):
    return HALF_U * np.abs(y64) + bar_pass2(a, live) + HALF_SUB


def wgrad_additions(n, n_k, m):
    return m * n + (-(-np.asarray(n_k) // 128) + 1)[:, None, None]


def bar_wgrad(s, n, n_k, m):
    """m = 1: f32 MFMA and half kernels, m = 6: split"""
    bar = SLACK * wgrad_additions(n, n_k, m) * 2 * U * s + np.asarray(n_k)[:, None, None] * TINY
    return bar + 0.25 * U * SPLIT_SUM * s if m == 6 else bar


# ----------------------------------------------------------------------------------------------------------- stage checks

def check_close(ck, stage, what, got, ref, bar, where=None):
    """every element (of `where`): finite and |got - ref| <= bar; the worst error / bar is the stage's printed figure"""
    got = np.asarray(got, dtype=np.float64)
    if where is not None:
        got, ref, bar = got[where], ref[where], bar[where]
    if got.size == 0:
        return
    finite = np.isfinite(got)
    ck.true(stage, f"{what}: {int((~finite).sum())} of {got.size} elements are not finite", bool(finite.all()))
    err = np.where(finite, np.abs(np.where(finite, got, 0.0) - ref), np.inf)
    safe = np.where(bar > 0, bar, 1.0)
    ratio = np.where(bar > 0, err / safe, np.where(err == 0, 0.0, np.inf))
    worst = int(np.argmax(ratio))
    ck.le(stage, f"{what}: worst error / bar at element {worst} of {got.size} ({int((ratio > 1).sum())} above)", float(ratio.reshape(-1)[worst]), 1.0)


def check_half(ck, stage, what, got, ref, bar):
    """a half result against its float64 reference: |ref| - bar >= 65520 -> inf of the sign; |ref| + bar < 65520 -> finite and inside
    the bar; between, either.  `bar` is the whole half bar (rounding + accumulation + subnormal)."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return
    mag = np.abs(ref)
    acc = bar - HALF_U * mag                                             # what the float32 sum may be off before the rounding
    must_inf, may_inf = mag - acc >= HALF_INF, mag + acc >= HALF_INF
    is_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
    ck.true(stage, f"{what}: {int((must_inf & ~is_inf).sum())} references of 65520 or more did not give inf", bool((is_inf | ~must_inf).all()))
    ck.true(stage, f"{what}: NaN in the result", not bool(np.isnan(got).any()))
    rest = ~(may_inf & is_inf)
    check_close(ck, stage, what, got, ref, bar, where=rest)


def check_pass2(ck, stage, what, got_bits, got, z_bits, z64, pos, half=False, where=None):
    """pass 2 against gather_sum64 of the device's own Z.  got_bits / z_bits: the integer views (int32, or int16 for half).
    where: rows to look at (default all)."""
    y, a, live = gather_sum64(z64, pos)
    rows = np.ones(len(live), dtype=bool) if where is None else where
    none, one, more = rows & (live == 0), rows & (live == 1), rows & (live > 1)
    ck.true(stage, f"{what}: {int((got_bits[none] != 0).sum())} elements of rows without a pair are not +0", bool((got_bits[none] == 0).all()))
    if one.any():
        src = np.zeros(len(live), dtype=np.int64)
        for kk in range(pos.shape[0]):
            src = np.where(pos[kk] >= 0, pos[kk], src)                   # rows with L = 1: their one position
        zb = z_bits[src[one]]
        minus_zero = zb == (np.int16(-32768) if half else np.int32(-2 ** 31))
        same = (got_bits[one] == zb) | (minus_zero & (got_bits[one] == 0))
        ck.true(stage, f"{what}: {int((~same).sum())} elements of rows with one pair do not carry the bits of their Z row", bool(same.all()))
    if more.any():
        if half:
            check_half(ck, stage, what, got[more], y[more], bar_pass2_half(y, a, live)[more])
        else:
            check_close(ck, stage, what, got[more], y[more], bar_pass2(a, live)[more])
    return live


# ------------------------------------------------------------------------------------------------------------------- cases

def _tiny27():
    """0 .. 3 pairs per offset, at most 60 in all and more than 20 offsets that are not empty: the first seed that gives both"""
    for seed in range(1000):
        c = rng("tiny27", seed).randint(0, 4, size=27)
        if c.sum() <= 60 and (c > 0).sum() > 20:
            return [int(v) for v in c]
    raise AssertionError("no seed")


EDGE = [0, 1, 127, 128, 129, 0, 0, 255, 256, 257, 31, 32, 33, 0, 385, 2, 0, 0, 0, 64, 96, 1, 0, 130, 3, 0, 5]
COUNTS = {
    "EDGE": (EDGE, 400),
    "TINY27": (_tiny27(), 64),
    "ONE": ([0] * 13 + [1] + [0] * 13, 64),
    "CENTRE": ([0] * 13 + [300] + [0] * 13, 400),
    "EMPTY": ([0] * 27, 400),
    "K8": ([128, 0, 1, 200, 129, 0, 127, 3], 400),
    "K1": ([257], 400),
}
CHANNELS = [(32, 32), (32, 64), (64, 96), (96, 128), (32, 192), (96, 256), (4, 32), (48, 24), (32, 48), (96, 20)]
FEW_CHANNELS = [(32, 32), (96, 128), (48, 24)]
CASES = [("EDGE", c) for c in CHANNELS] + [(name, c) for name in COUNTS if name != "EDGE" for c in FEW_CHANNELS]
CONTRACT_COUNTS = ("EDGE", "TINY27")
F32_IMPLS = (2, 3, 4, 5)
SPLIT_IMPLS = (0, 6)


def case_id(case):
    return f"{case[0]}-{case[1][0]}to{case[1][1]}"


def rulebook(name):
    """(nbmaps, nboffs, pos_out, pos_in, n) of a count vector, n_in = n_out = n.  For the vectors of the contract checks, the first
    seed whose map has an input row and an output row that three offsets pair: what the NaN checks write into."""
    counts, n = COUNTS[name]
    for seed in range(1, 200):
        book = make_rulebook(counts, n, n, seed)
        if name not in CONTRACT_COUNTS or min(np.bincount(book[0][:, 0]).max(), np.bincount(book[0][:, 1]).max()) >= 3:
            return book + (n,)
    raise AssertionError("no seed")


def families(c_red, half=False):
    f = ["dense", "one_hot"] + (["two_hot"] if c_red == 96 else [])
    return f + ["half_small", "half_large"] if half else f


def is_half_shape(c_red, c_out):
    return c_red % 32 == 0 and c_out % 32 == 0


def _signed(rs, shape, lo, hi):
    return (rs.uniform(lo, hi, size=shape) * rs.choice([-1.0, 1.0], size=shape))


def _normal(rs, shape, half):
    """standard normal entries; for half storage magnitudes of 0.5 .. 1.5 instead, so that no operand is a half subnormal"""
    return _signed(rs, shape, 0.5, 1.5) if half else rs.randn(*shape)


def features(family, n, c, key, half=False):
    """float32 [n, c]: the gathered operand (x of pass 1, A of the weight gradient)"""
    rs = rng("features", family, n, c, key, half)
    rows = np.arange(n)
    if family == "dense":                      # every row on its own power of two, 2^-24 .. 2^24 (half storage: 2^-8 .. 2^8)
        top = 8 if half else 24
        x = _normal(rs, (n, c), half) * np.ldexp(1.0, rs.randint(-top, top + 1, size=(n, 1)))
    elif family == "half_small":               # near 2^-10: products near 2^-20, sums in the half-subnormal range
        x = _signed(rs, (n, c), 0.5, 1.5) * 2.0 ** -10
    else:
        x = np.zeros((n, c))
        big = family == "half_large"
        v = _signed(rs, (n, 2), 100.0, 250.0) if big else _signed(rs, (n, 2), 0.5, 1.5)
        if family == "two_hot":                # the first and the last 32-slice of the reduction
            x[rows, rows % 32] = v[:, 0]
            x[rows, c - 32 + (7 * rows + 5) % 32] = v[:, 1]
        else:                                  # one_hot, half_large: one entry, in a column that walks through all of them
            x[rows, rows % c] = v[:, 0]
    return np.ascontiguousarray(x, dtype=np.float32)


def weights(family, k, c_red, c_out, key, transposed=False, half=False):
    """float32 [K, c_red, c_out] - stored [K, c_out, c_red] when transposed (the same W_k either way)"""
    rs = rng("weights", family, k, c_red, c_out, key, half)
    if family == "half_small":
        w = _signed(rs, (k, c_red, c_out), 0.5, 1.5) * 2.0 ** -10
    elif family == "half_large":               # 250 x 240 = 60 000 < 65 504
        w = rs.uniform(-240.0, 240.0, size=(k, c_red, c_out))
    else:
        w = _normal(rs, (k, c_red, c_out), half) / math.sqrt(c_red)
    w = w.astype(np.float32)
    return np.ascontiguousarray(w.transpose(0, 2, 1)) if transposed else w


def second_operand(family, n, c, key, half=False):
    """float32 [n, c]: the B rows of the weight gradient"""
    rs = rng("second", family, n, c, key, half)
    if family == "half_small":
        b = _signed(rs, (n, c), 0.5, 1.5) * 2.0 ** -10
    elif family == "half_large":
        b = rs.uniform(-240.0, 240.0, size=(n, c))
    else:
        b = _normal(rs, (n, c), half)
    return b.astype(np.float32)


def to_half(a):
    """float32 -> the halves the half kernels receive (numpy rounds to nearest even); none of the families leaves the normal range"""
    h = np.asarray(a, dtype=np.float32).astype(np.float16)
    assert np.isfinite(h).all() and ((h == 0) | (np.abs(h.astype(np.float64)) >= 2.0 ** -14)).all()
    return h
