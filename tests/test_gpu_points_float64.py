"""The point <-> voxel transfer kernels (csrc/pointops.hip, trilinear_kernel of csrc/coords.hip) against float64
(oracle/points64.py), through the C ABI and through autograd (-m gpu).

Every element is compared.  Every check of a case is evaluated; the case fails with the list of those that missed, and prints
one line of error / bar per stage (profiles/points_float64.txt keeps a run's lines).  Every bar is computed from the inputs and
the float64 reference, never from a kernel's output.  u = 2^-24, TINY = 2^-149 (what one float operation may lose to
underflow), SLACK = 1.01 for the second-order terms.  pointops.hip is built without contraction; a contracted multiply-add
would only remove a rounding.  tests/test_points64_host.py shows on the CPU that float32 arithmetic meets these bars in any
order and that a dropped slot, a wrong corner's weight or a forgotten factor misses them.

Sums.  A float32 sum of t live terms, each a rounded product w x (or quotient f / cnt), added in ANY order - a chain, a tree,
atomics in the order the hardware serves them, partial sums of segments - errs by at most (1 + (t - 1)) u S with S = sum |term|:
one rounding for the term and at most t - 1 additions above it (additions of a zero term are exact, so the zero-weight rows the
cell-reduced form adds do not count).  Hence
  voxelize forward, t = live points of the voxel:          |got - ref| <= SLACK t u S + t TINY
  devoxelize forward, t <= 8 live corners:                 |got - ref| <= SLACK t u S + 8 TINY
  the adjoint in all five float32 forms (atomic, run-wise with and without a walk order, inverse map, cell-reduced),
  t_v = live slots of voxel v:                             |got - ref| <= SLACK t_v u S_v + t_v TINY, exactly 0 where t_v = 0
  voxelize backward, one division:                         |got - ref| <= SLACK u |ref| + TINY, exactly 0 for a point without a
                                                           voxel (idx < 0) or of a voxel with counts == 0
A term is live when idx >= 0 and w != 0, the kernels' rule.
Half storage (ts_devoxelize_forward_f16_ld, ts_devoxelize_backward_{csr,cells}_f16_ld): the inputs are half values, the sums
float32 (the partial sums of the cell-reduced form stay float32) and the result is rounded once: with E32 the float32 bar of the
same case,                                                 |got - ref| <= E32 (1 + 2^-11) + 2^-11 |ref| + 2^-25
and |ref| + bar < 65504 is asserted from the reference alone.
The exact family: weights in {0, 2^-j}, rows of small integers, every partial sum a float32 - the result equals the reference
bit for bit in every form (half: the reference rounded once to half), so a dropped or doubled slot fails by a whole number.

Trilinear weights (trilinear_kernel; F.calc_ti_weights evaluates the same expression with torch ops).  Indices are exact;
the weight of an absent corner is exactly 0, and all eight where no corner is present.  A present corner's weight is
  w_k = v_k / (sum_j v_j + 1e-8f),   v_k = ((dx dy) dz) / s^3
dx, dy, dz: differences of the point and a face of its cell - the faces are integers and exact, a difference rounds once (u each,
3 u); two products (2 u); / s^3 with s^3 a power of two is exact: v_k carries 5 u.  The sum is of non-negative terms, so it
inherits their 5 u and adds one u for each of its seven additions and for the addition of the constant (8 u): 13 u; the final
division one more: k = 5 + 13 + 1 = 19,                      |got - w64| <= SLACK 19 u w64 + TINY.
The float64 reference takes floor(p / s) in float32 as the kernel does (exact for the power-of-two strides used here; no point
lies in 0 < |p| < 2^-60) and the constant as float32(1e-8).
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import points64 as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
UNSUPPORTED = -4                               # include/taseg_hip.h TS_ERR_UNSUPPORTED
FILL = 7.0                                     # what output buffers hold before a call
FWD_CAP = 16384 * 256                          # lanes of one grid-stride pass of the devoxelize kernels at their grid cap
VOX_CAP = 8192 * 256                           # the same for the voxelize kernels
ADJOINT_C = [4, 12, 20, 96, 256, 1024]


def _L():
    from taseg_amd import _lib as L
    return L, L.load()


def _B():
    from taseg_amd import backend as B
    return B


class Checks:
    def __init__(self, cid):
        self.cid, self.missed, self.n, self.ratios = cid, [], 0, {}

    def le(self, stage, what, value, bound=1.0):
        self.n += 1
        ratio = value / bound if bound > 0 else (0.0 if value <= bound else math.inf)
        self.ratios[stage] = max(self.ratios.get(stage, 0.0), ratio)
        if not value <= bound:
            self.missed.append(f"{stage} {what}: {value:.3e} > {bound:.3e}")

    def true(self, what, ok):
        self.n += 1
        if not ok:
            self.missed.append(what)

    def done(self):
        print(f"points_float64 {self.cid:<52} error / bar:  " + "  ".join(f"{k} {v:.3f}" for k, v in self.ratios.items())
              + f"  ({self.n} checks)")
        assert not self.missed, f"{self.cid}: {len(self.missed)} of {self.n} checks missed\n  " + "\n  ".join(self.missed[:40])


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def worst(got, ref, bar):
    """largest |got - ref| / bar over every element; inf where a bar of 0 is missed or a value is not finite"""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def randn(key, *shape):
    return rng(*key).randn(*shape).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- voxelize

@pytest.mark.parametrize("n,c,m", [(1, 1, 1), (33, 3, 5), (400, 20, 9), (1025, 256, 300), (8201, 256, 40)])
def test_voxelize(n, c, m):
    """one point; odd channels; voxels of ~45 and of ~200 points (atomics in any order); 8201 x 256 elements = one grid-stride pass
    at the cap of 8192 workgroups and 2304 elements more; points without a voxel and a voxel whose count is 0"""
    L, lib = _L()
    ck = Checks(f"voxelize n={n} c={c} m={m}")
    assert (n * c > VOX_CAP) == (n == 8201)
    rs = rng("vox", n, c)
    idx = rs.randint(-1, m, size=n).astype(np.int32)
    counts = np.bincount(idx[idx >= 0], minlength=m).astype(np.int32)
    if m > 1:
        counts[m - 1] = 0
    feat, gout = randn(("vf", n, c), n, c), randn(("vg", n, c), m, c)
    ref, t, s = P.voxelize_forward64(feat, idx, counts)
    idx_d, counts_d, feat_d, gout_d = dev(idx), dev(counts), dev(feat), dev(gout)
    out = torch.full((m, c), FILL, device=DEV)
    ck.true("TS_OK", lib.ts_voxelize_forward(L.ptr(feat_d), L.ptr(idx_d), L.ptr(counts_d), n, c, m, L.ptr(out), L.stream()) == 0)
    ck.le("forward", "worst error / bar", worst(host(out), ref, P.bar_sum(t, s)))
    ck.true("a voxel without live points is exactly 0", bool((host(out)[t == 0] == 0).all()))
    refb, alive = P.voxelize_backward64(gout, idx, counts, n)
    gf = torch.full((n, c), FILL, device=DEV)
    ck.true("TS_OK", lib.ts_voxelize_backward(L.ptr(gout_d), L.ptr(idx_d), L.ptr(counts_d), n, c, m, L.ptr(gf), L.stream()) == 0)
    ck.le("backward", "worst error / bar", worst(host(gf), refb, P.SLACK * P.U * np.abs(refb) + P.TINY))
    ck.true("a point without a live voxel gets exactly 0", bool((host(gf)[~alive] == 0).all()) and (n == 1 or bool((~alive).any())))
    ck.done()


# ------------------------------------------------------------------------------------------------------- devoxelize forward

def k_forward(feat_d, idx_d, w_d, m, c, ld, col, plain):
    """ts_devoxelize_forward (plain) / _ld / _f16_ld into column block `col` of a [n, ld] matrix pre-filled with FILL"""
    L, lib = _L()
    n = idx_d.shape[0]
    half = feat_d.dtype == torch.float16
    out = torch.full((n, ld), FILL, dtype=feat_d.dtype, device=DEV)
    assert col + c <= ld and feat_d.shape == (m, c) and idx_d.shape == w_d.shape == (n, 8)
    assert int(idx_d.max()) < m and int(idx_d.min()) >= -1
    base = out.data_ptr() + out.element_size() * col
    if half:
        rc = lib.ts_devoxelize_forward_f16_ld(L.ptr(feat_d), L.ptr(idx_d), L.ptr(w_d), n, c, m, base, ld, L.stream())
    elif plain:
        assert ld == c
        rc = lib.ts_devoxelize_forward(L.ptr(feat_d), L.ptr(idx_d), L.ptr(w_d), n, c, m, base, L.stream())
    else:
        rc = lib.ts_devoxelize_forward_ld(L.ptr(feat_d), L.ptr(idx_d), L.ptr(w_d), n, c, m, base, ld, L.stream())
    return rc, out


def check_forward(ck, tag, idx, w, m, c, ld=None, col=0, halves=(False,), exact=False):
    """random rows (and, exact = True, the exact family) through the forward kernels on the map (idx, w) [n, 8] (numpy)"""
    n = idx.shape[0]
    ld = c if ld is None else ld
    if exact:
        w, feat, _ = P.exact_case(idx, w, m, c, c)
    else:
        feat = randn(("feat", tag, c), m, c)
    idx_d, w_d = dev(idx), dev(w)
    for half in halves:
        f = feat.astype(np.float16) if half else feat
        ref, t, s = P.devoxelize_forward64(f, idx, w)
        bar = P.bar_sum(t, s, 8)
        stage = ("forward_f16" if half else "forward") + ("/exact" if exact else "")
        if half:
            ck.true(f"{tag}: |ref| + bar < 65504", float((np.abs(ref) + P.bar_half(bar, ref)).max()) < P.HALF_MAX)
            bar = P.bar_half(bar, ref)
        rc, out = k_forward(dev(f), idx_d, w_d, m, c, ld, col, plain=ld == c and not half)
        got = host(out)
        ck.true(f"{tag} {stage}: TS_OK", rc == 0)
        ck.le(stage, f"{tag}: worst error / bar", worst(got[:, col:col + c], ref, bar))
        ck.true(f"{tag} {stage}: a point without live corners is exactly 0", bool((got[:, col:col + c][t == 0] == 0).all()))
        rest = np.delete(got, np.s_[col:col + c], axis=1)
        ck.true(f"{tag} {stage}: the columns outside the block keep what they held", bool((rest == FILL).all()))
        if exact:
            ck.true(f"{tag} {stage}: not the bits of the reference", same_bits(got[:, col:col + c], ref.astype(got.dtype)))


FORWARD_CASES = [(1, None, 0), (3, None, 0), (4, None, 0), (18, None, 0), (20, None, 0), (96, None, 0), (1024, None, 0),
                 (20, 50, 0), (20, 52, 8)]


@pytest.mark.parametrize("c,ld,col", FORWARD_CASES, ids=lambda v: str(v))
def test_devoxelize_forward(c, ld, col):
    """c % 4 != 0 and ld % 4 != 0: the scalar kernel; else the float4 kernel; ld = 52, col = 8: a column block of a wider matrix.
    Maps: the sizes around one lane group and the constructed map of 400 points (oracle/points64.constructed_map)."""
    ck = Checks(f"devoxelize forward c={c} ld={ld or c} col={col}")
    halves = (False, True) if c % 4 == 0 and (ld or c) % 4 == 0 else (False,)
    for n in (1, 33, 400):
        idx, w, m = P.constructed_map(n)
        check_forward(ck, f"n={n}", idx, w, m, c, ld, col, halves)
    idx, w, m = P.constructed_map(400)
    check_forward(ck, "n=400", idx, w, m, c, ld, col, halves, exact=True)
    ck.done()


def test_devoxelize_forward_past_the_grid_cap():
    """n = 16 400, c = 1024: 4 198 400 lane groups against one pass of 16 384 x 256"""
    n, c, m = 16400, 1024, 50
    assert n * (c // 4) > FWD_CAP
    ck = Checks(f"devoxelize forward n={n} c={c}")
    idx, w = P.random_map(n, m, 77)
    check_forward(ck, "cap", idx, w, m, c)
    ck.done()


# ------------------------------------------------------------------------------------------------------------- the adjoint

def adjoint_forms(g_d, col, c, idx_d, w_d, m, atomic_too=True):
    """every form of the adjoint on column block `col` of the gradient matrix g_d [n, ld] (float32: five forms; half: the two
    half-storage forms) -> {name: (status, result [m, c] pre-filled with FILL)}"""
    L, lib = _L()
    B = _B()
    n, ld = g_d.shape
    half = g_d.dtype == torch.float16
    assert col + c <= ld and col % 4 == 0 and ld % 4 == 0 and c % 4 == 0 and idx_d.shape == w_d.shape == (n, 8)
    assert int(idx_d.max()) < m and int(idx_d.min()) >= -1
    base = g_d.data_ptr() + g_d.element_size() * col
    st = L.stream()
    order = B.devox_order(idx_d, m)
    off, ent = B.devox_csr(idx_d, w_d, m)
    _, walk, seg_start, coff, cent = B.devox_cells(idx_d, w_d, m)
    n_seg = seg_start.shape[0] - 1
    part = torch.empty((max(8 * n_seg, 1), c), dtype=torch.float32, device=DEV)
    new = lambda: torch.full((m, c), FILL, dtype=g_d.dtype, device=DEV)          # noqa: E731
    res = {}
    if half:
        o = new()
        res["csr_f16"] = (lib.ts_devoxelize_backward_csr_f16_ld(base, ld, L.ptr(w_d), L.ptr(off), L.ptr(ent), n, c, m, L.ptr(o), st), o)
        o = new()
        res["cells_f16"] = (lib.ts_devoxelize_backward_cells_f16_ld(base, ld, L.ptr(w_d), L.ptr(walk), L.ptr(seg_start), n_seg, L.ptr(coff),
                                                                    L.ptr(cent), n, c, m, L.ptr(part), L.ptr(o), st), o)
        return res
    if atomic_too:                             # (the atomic kernel has no leading dimension: it reads a contiguous copy)
        gc = g_d[:, col:col + c].contiguous()
        o = new()
        res["atomic"] = (lib.ts_devoxelize_backward(L.ptr(gc), L.ptr(idx_d), L.ptr(w_d), n, c, m, L.ptr(o), st), o)
    for name, ordr in (("runs", None), ("runs+order", order)):
        o = new()
        if ld == c:
            rc = lib.ts_devoxelize_backward_runs(base, L.ptr(idx_d), L.ptr(w_d), L.ptr(ordr), n, c, m, L.ptr(o), st)
        else:
            rc = lib.ts_devoxelize_backward_runs_ld(base, ld, L.ptr(idx_d), L.ptr(w_d), L.ptr(ordr), n, c, m, L.ptr(o), st)
        res[name] = (rc, o)
    o = new()
    if ld == c:
        rc = lib.ts_devoxelize_backward_csr(base, L.ptr(w_d), L.ptr(off), L.ptr(ent), n, c, m, L.ptr(o), st)
    else:
        rc = lib.ts_devoxelize_backward_csr_ld(base, ld, L.ptr(w_d), L.ptr(off), L.ptr(ent), n, c, m, L.ptr(o), st)
    res["csr"] = (rc, o)
    o = new()
    res["cells"] = (lib.ts_devoxelize_backward_cells_ld(base, ld, L.ptr(w_d), L.ptr(walk), L.ptr(seg_start), n_seg, L.ptr(coff), L.ptr(cent),
                                                        n, c, m, L.ptr(part), L.ptr(o), st), o)
    return res


def check_adjoint(ck, tag, idx, w, m, c, wide, exact=False, halves=(False, True)):
    """random gradient rows (exact = True: the exact family) through every form of the adjoint on the map (idx, w) (numpy);
    wide: the rows are columns 8 .. 8 + c of a matrix of c + 12 columns"""
    n = idx.shape[0]
    ld, col = (c + 12, 8) if wide else (c, 0)
    if exact:
        w, _, g = P.exact_case(idx, w, m, c, c + 1)
    else:
        g = randn(("gout", tag, c), n, c)
    wide_g = randn(("wide", tag, c), n, ld)
    wide_g[:, col:col + c] = g
    idx_d, w_d = dev(idx), dev(w)
    for half in halves:
        gm = wide_g.astype(np.float16) if half else wide_g
        ref, t, s = P.adjoint64(gm[:, col:col + c], idx, w, m)
        bar = P.bar_sum(t, s)
        if half:
            ck.true(f"{tag}: |ref| + bar < 65504", float((np.abs(ref) + P.bar_half(bar, ref)).max()) < P.HALF_MAX)
            bar = P.bar_half(bar, ref)
        for name, (rc, out) in adjoint_forms(dev(gm), col, c, idx_d, w_d, m).items():
            stage = name + ("/exact" if exact else "")
            got = host(out)
            ck.true(f"{tag} {stage}: TS_OK", rc == 0)
            ck.le(stage, f"{tag}: worst error / bar", worst(got, ref, bar))
            ck.true(f"{tag} {stage}: a voxel without live slots is exactly 0", bool((got[t == 0] == 0).all()))
            if exact:
                ck.true(f"{tag} {stage}: not the bits of the reference", same_bits(got, ref.astype(got.dtype)))


def adjoint_sizes(c):
    """1, 31, 32, 33: around one 32-point run; 32 (256 / (c / 4)) + 1: one run more than a workgroup of the run-wise kernel takes;
    400 (or that size, where it is larger): the constructed map"""
    edge = 32 * (256 // (c // 4)) + 1
    return sorted({1, 31, 32, 33, edge, max(400, edge)})


@pytest.mark.parametrize("wide", [False, True], ids=["ld=c", "ld>c"])
@pytest.mark.parametrize("c", ADJOINT_C)
def test_adjoint_forms(c, wide):
    """c = 12: 85 lane groups of 3 and an idle lane; c = 1024: one lane group per workgroup"""
    ck = Checks(f"adjoint c={c} {'ld=c+12' if wide else 'ld=c'}")
    sizes = adjoint_sizes(c)
    for n in sizes:
        idx, w, m = P.constructed_map(n)
        check_adjoint(ck, f"n={n}", idx, w, m, c, wide)
    idx, w, m = P.constructed_map(sizes[-1])
    check_adjoint(ck, f"n={sizes[-1]}", idx, w, m, c, wide, exact=True)
    ck.done()


def test_atomic_adjoint_past_the_grid_cap():
    """n = 4 100, c = 1024: 4 198 400 elements against one pass of 16 384 x 256"""
    L, lib = _L()
    n, c, m = 4100, 1024, 50
    assert n * c > FWD_CAP
    ck = Checks(f"adjoint atomic n={n} c={c}")
    idx, w = P.random_map(n, m, 78)
    g = randn(("cap", n, c), n, c)
    ref, t, s = P.adjoint64(g, idx, w, m)
    g_d, idx_d, w_d = dev(g), dev(idx), dev(w)                 # (held: a pointer outlives no temporary)
    out = torch.full((m, c), FILL, device=DEV)
    ck.true("TS_OK", lib.ts_devoxelize_backward(L.ptr(g_d), L.ptr(idx_d), L.ptr(w_d), n, c, m, L.ptr(out), L.stream()) == 0)
    ck.le("atomic", "worst error / bar", worst(host(out), ref, P.bar_sum(t, s)))
    ck.done()


def test_refusals_leave_the_gradient_untouched():
    """c = 6 and c = 1028 at the run-wise, inverse-map and cell-reduced entry points, float and half: status codes, nothing is launched"""
    L, lib = _L()
    n, m = 2, 3
    st = L.stream()
    idx_d, w_d = dev(np.zeros((n, 8), np.int32)), dev(np.full((n, 8), 0.125, np.float32))
    order, seg = dev(np.arange(n, dtype=np.int32)), dev(np.array([0, n], np.int32))
    off, ent = dev(np.zeros(m + 1, np.int32)), dev(np.zeros(8 * n, np.int32))
    for c, ld in ((6, 8), (1028, 1028)):
        part = torch.zeros((8, c), device=DEV)
        for dtype in (torch.float32, torch.float16):
            g = torch.ones((n, ld), dtype=dtype, device=DEV)
            gf = torch.full((m, c), 3.0, dtype=dtype, device=DEV)
            a = (L.ptr(g), ld, L.ptr(w_d))
            if dtype == torch.float32:
                calls = {"runs_ld": lambda: lib.ts_devoxelize_backward_runs_ld(*a[:2], L.ptr(idx_d), L.ptr(w_d), L.ptr(order), n, c, m, L.ptr(gf), st),
                         "csr_ld": lambda: lib.ts_devoxelize_backward_csr_ld(*a, L.ptr(off), L.ptr(ent), n, c, m, L.ptr(gf), st),
                         "cells_ld": lambda: lib.ts_devoxelize_backward_cells_ld(*a, L.ptr(order), L.ptr(seg), 1, L.ptr(off), L.ptr(ent), n, c, m,
                                                                                 L.ptr(part), L.ptr(gf), st)}
                if ld == c:                    # (the entry points without a leading dimension pass ld = c on: 6 is refused as a bad size)
                    calls["runs"] = lambda: lib.ts_devoxelize_backward_runs(a[0], L.ptr(idx_d), L.ptr(w_d), None, n, c, m, L.ptr(gf), st)
                    calls["csr"] = lambda: lib.ts_devoxelize_backward_csr(a[0], L.ptr(w_d), L.ptr(off), L.ptr(ent), n, c, m, L.ptr(gf), st)
            else:
                calls = {"csr_f16_ld": lambda: lib.ts_devoxelize_backward_csr_f16_ld(*a, L.ptr(off), L.ptr(ent), n, c, m, L.ptr(gf), st),
                         "cells_f16_ld": lambda: lib.ts_devoxelize_backward_cells_f16_ld(*a, L.ptr(order), L.ptr(seg), 1, L.ptr(off), L.ptr(ent), n, c,
                                                                                         m, L.ptr(part), L.ptr(gf), st)}
            for name, call in calls.items():
                assert call() == UNSUPPORTED, (name, c)
                assert b"multiple of 4" in lib.ts_last_error(), (name, c)
            torch.cuda.synchronize()
            assert bool((gf == 3.0).all()), (c, dtype)


# ------------------------------------------------------------------------------------------------------------------- plans

@pytest.mark.parametrize("n", [1, 33, 400, 2721])
def test_plan_properties_on_constructed_maps(n):
    B = _B()
    ck = Checks(f"plans n={n}")
    idx, w, m = P.constructed_map(n)
    idx_d, w_d = dev(idx), dev(w)
    order = host(B.devox_order(idx_d, m))
    ck.true("devox_order is a permutation", np.array_equal(np.sort(order), np.arange(n)))
    off, ent = (host(t) for t in B.devox_csr(idx_d, w_d, m))
    flat = idx.reshape(-1)
    alive = np.flatnonzero(P.live(idx, w).reshape(-1))
    want_ent = alive[np.argsort(flat[alive], kind="stable")]
    ck.true("devox_csr offsets", np.array_equal(off, np.searchsorted(flat[want_ent], np.arange(m + 1))))
    ck.true("devox_csr lists exactly the live slots, by voxel, ascending within a voxel", np.array_equal(ent[:len(want_ent)], want_ent))
    for max_len in (1, 64):
        _, walk, seg_start, coff, cent = (host(t) if isinstance(t, torch.Tensor) else t for t in B.devox_cells(idx_d, w_d, m, max_len))
        ck.true(f"max_len {max_len}: the walk is a permutation", np.array_equal(np.sort(walk), np.arange(n)))
        ck.true(f"max_len {max_len}: the segments partition the walk", seg_start[0] == 0 and seg_start[-1] == n
                and bool((np.diff(seg_start) > 0).all()))
        ck.true(f"max_len {max_len}: no segment is longer", int(np.diff(seg_start).max()) <= max_len)
        seg_of = np.repeat(np.arange(len(seg_start) - 1), np.diff(seg_start))
        tuples = idx[walk[seg_start[:-1]]]
        ck.true(f"max_len {max_len}: one tuple per segment", np.array_equal(idx[walk], tuples[seg_of]))
        tflat = tuples.reshape(-1)
        present = np.flatnonzero(tflat >= 0)
        want = present[np.argsort(tflat[present], kind="stable")]
        ck.true(f"max_len {max_len}: the second stage lists every present corner of every segment once",
                np.array_equal(cent[:len(want)], want) and np.array_equal(coff, np.searchsorted(tflat[want], np.arange(m + 1))))
    if n >= P.CORE_ROWS:
        lens = np.diff(seg_start)              # (max_len 64) the cells of 63 and 64 points fit one segment unless a multiple of 64 cuts them
        ck.true("segments of many points exist", int(lens.max()) > 32)
    ck.done()


# --------------------------------------------------------------------------------------------------------------- real maps

@functools.lru_cache(maxsize=None)
def scan(s):
    pts, vox = P.scan_points(s)
    idx, w64 = P.trilinear64(pts, vox, s)
    return pts, vox, idx, w64


@pytest.mark.parametrize("s", [1, 2, 4, 8, 16])
def test_trilinear_map(s):
    B = _B()
    from taseg_amd.torchsparse.nn import functional as F
    ck = Checks(f"trilinear stride={s}")
    pts, vox, idx, w64 = scan(s)
    bar = P.bar_trilinear(w64)
    pts_d = dev(pts)
    idx_d, w_d = B.trilinear_map(pts_d, dev(vox), s)
    got_idx, got = host(idx_d), host(w_d)
    none = ~(idx >= 0).any(1)
    ck.true("some point has no corner, some corner is absent, some present corner weighs 0",
            bool(none.any()) and bool((idx < 0).any()) and bool(((idx >= 0) & (w64 == 0)).any()))
    ck.true("indices are the dictionary's", np.array_equal(got_idx, idx))
    for name, g in (("kernel", got), ("calc_ti_weights", host(F.calc_ti_weights(pts_d, idx_d.t().contiguous(), scale=s)).T)):
        ck.le(name, "worst error / bar", worst(g, w64, bar))
        ck.true(f"{name}: an absent corner weighs exactly 0", bool((g[idx < 0] == 0).all()))
        ck.true(f"{name}: all eight are 0 where no corner is present", bool((g[none] == 0).all()))
    ck.done()


@pytest.mark.parametrize("s", [1, 4, 16])
def test_transfer_on_the_maps_of_a_scan(s):
    """the forward and every form of the adjoint on the map trilinear_kernel gives for ~3 000 points with genuinely varying
    fractions: eight different weights per point"""
    B = _B()
    ck = Checks(f"scan map stride={s}")
    pts, vox, _, _ = scan(s)
    idx_d, w_d = B.trilinear_map(dev(pts), dev(vox), s)
    idx, w, m = host(idx_d), host(w_d), len(vox)
    for c in (20, 96):
        check_forward(ck, f"c={c}", idx, w, m, c, halves=(False, True))
        check_adjoint(ck, f"c={c}", idx, w, m, c, wide=c == 20)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- autograd

def test_spvoxelize_through_autograd():
    from taseg_amd.torchsparse.nn import functional as F
    ck = Checks("autograd spvoxelize")
    n, c, m = 400, 20, 9
    rs = rng("avox")
    idx = rs.randint(-1, m, size=n).astype(np.int32)
    counts = np.bincount(idx[idx >= 0], minlength=m).astype(np.int32)
    counts[m - 1] = 0
    feat, gout = randn(("af",), n, c), randn(("ag",), m, c)
    x = dev(feat).requires_grad_()
    out = F.spvoxelize(x, dev(idx), dev(counts))
    out.backward(dev(gout))
    ref, t, s = P.voxelize_forward64(feat, idx, counts)
    refb, alive = P.voxelize_backward64(gout, idx, counts, n)
    ck.le("forward", "worst error / bar", worst(host(out), ref, P.bar_sum(t, s)))
    ck.le("backward", "worst error / bar", worst(host(x.grad), refb, P.SLACK * P.U * np.abs(refb) + P.TINY))
    ck.true("exact zeros", bool((host(x.grad)[~alive] == 0).all()) and bool((host(out)[t == 0] == 0).all()))
    ck.done()


def plans_of(idx_d, w_d, m):
    B = _B()
    return {"none": None, "walk": B.devox_order(idx_d, m), "csr": B.devox_csr(idx_d, w_d, m), "cells": B.devox_cells(idx_d, w_d, m)}


def test_spdevoxelize_through_autograd():
    """order = None / walk order / inverse map / cell plan in float32; half features under autocast with a plan (the half-storage
    kernels) and without one (the float kernels between casts); c = 6, which falls back to the atomic kernel"""
    from taseg_amd.torchsparse.nn import functional as F
    ck = Checks("autograd spdevoxelize")
    idx, w, m = P.constructed_map(400)
    n = idx.shape[0]
    idx_d, w_d = dev(idx), dev(w)
    plans = plans_of(idx_d, w_d, m)
    for c in (20, 6):
        feat, gout = randn(("sf", c), m, c), randn(("sg", c), n, c)
        ref_f, t_f, s_f = P.devoxelize_forward64(feat, idx, w)
        ref_a, t_a, s_a = P.adjoint64(gout, idx, w, m)
        for name, plan in plans.items():
            x = dev(feat).requires_grad_()
            out = F.spdevoxelize(x, idx_d, w_d, plan)
            out.backward(dev(gout))
            stage = f"c={c}/{name}"
            ck.true(f"{stage}: float32 in, float32 out", out.dtype == x.grad.dtype == torch.float32)
            ck.le(stage, "forward: worst error / bar", worst(host(out), ref_f, P.bar_sum(t_f, s_f, 8)))
            ck.le(stage, "backward: worst error / bar", worst(host(x.grad), ref_a, P.bar_sum(t_a, s_a)))
            ck.true(f"{stage}: a voxel without live slots gets exactly 0", bool((host(x.grad)[t_a == 0] == 0).all()))
            if c == 20 and name in ("csr", "cells"):           # the fixed-order forms: the bits of the C ABI's result
                key = name
                want = adjoint_forms(dev(gout), 0, c, idx_d, w_d, m, atomic_too=False)[key][1]
                ck.true(f"{stage}: the gradient is not the C ABI's bit for bit", same_bits(host(x.grad), host(want)))
    c = 20
    feat, gout = randn(("hf",), m, c).astype(np.float16), randn(("hg",), n, c).astype(np.float16)
    ref_f, t_f, s_f = P.devoxelize_forward64(feat, idx, w)
    ref_a, t_a, s_a = P.adjoint64(gout, idx, w, m)
    bar_f, bar_a = P.bar_half(P.bar_sum(t_f, s_f, 8), ref_f), P.bar_half(P.bar_sum(t_a, s_a), ref_a)
    ck.true("half: |ref| + bar < 65504", float((np.abs(ref_f) + bar_f).max()) < P.HALF_MAX and float((np.abs(ref_a) + bar_a).max()) < P.HALF_MAX)
    for name in ("csr", "cells", "none", "walk"):
        x = dev(feat).requires_grad_()
        with torch.autocast("cuda", dtype=torch.float16):
            out = F.spdevoxelize(x, idx_d, w_d, plans[name])
        out.backward(dev(gout))
        stage = f"half/{name}"
        ck.true(f"{stage}: half in, half out", out.dtype == x.grad.dtype == torch.float16)
        ck.le(stage, "forward: worst error / bar", worst(host(out), ref_f, bar_f))
        ck.le(stage, "backward: worst error / bar", worst(host(x.grad), ref_a, bar_a))
        if name in ("csr", "cells"):                           # stored half: the bits of the half-storage entry points
            want = adjoint_forms(dev(gout), 0, c, idx_d, w_d, m)[name + "_f16"][1]
            ck.true(f"{stage}: the gradient is not the C ABI's bit for bit", same_bits(host(x.grad), host(want)))
            ck.true(f"{stage}: the result is not the C ABI's bit for bit",
                    same_bits(host(out), host(k_forward(dev(feat), idx_d, w_d, m, c, c, 0, False)[1])))
    ck.done()


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
def test_spdevoxelize_cat_through_autograd(half):
    """three sources of 4, 12 and 20 channels on three maps and three different plans into one matrix; the gradient blocks are read
    in place (ld = 36, columns 0, 4 and 16)"""
    from taseg_amd.torchsparse.nn import functional as F
    ck = Checks(f"autograd spdevoxelize_cat {'half' if half else 'float32'}")
    n, cs = 400, (4, 12, 20)
    kinds = ("csr", "cells", "csr") if half else ("walk", "csr", "cells")
    as_in = (lambda a: a.astype(np.float16)) if half else (lambda a: a)
    maps, feats, xs = [], [], []
    for i, (c, kind) in enumerate(zip(cs, kinds)):
        idx, w, m = P.constructed_map(n, seed=i)
        idx_d, w_d = dev(idx), dev(w)
        maps.append((idx, w, m, (idx_d, w_d, plans_of(idx_d, w_d, m)[kind])))
        feats.append(as_in(randn(("cf", i), m, c)))
        xs.append(dev(feats[-1]).requires_grad_())
    gout = as_in(randn(("cg",), n, sum(cs)))
    out = F.spdevoxelize_cat(xs, [mp[3] for mp in maps])
    ck.true("shape and type", out.shape == (n, sum(cs)) and out.dtype == (torch.float16 if half else torch.float32))
    out.backward(dev(gout))
    col = 0
    for i, c in enumerate(cs):
        idx, w, m, _ = maps[i]
        ref_f, t_f, s_f = P.devoxelize_forward64(feats[i], idx, w)
        ref_a, t_a, s_a = P.adjoint64(gout[:, col:col + c], idx, w, m)
        bar_f, bar_a = P.bar_sum(t_f, s_f, 8), P.bar_sum(t_a, s_a)
        if half:
            bar_f, bar_a = P.bar_half(bar_f, ref_f), P.bar_half(bar_a, ref_a)
            ck.true("|ref| + bar < 65504", float((np.abs(ref_f) + bar_f).max()) < P.HALF_MAX and float((np.abs(ref_a) + bar_a).max()) < P.HALF_MAX)
        ck.le(f"source {i}/{kinds[i]}", "forward: worst error / bar", worst(host(out)[:, col:col + c], ref_f, bar_f))
        ck.le(f"source {i}/{kinds[i]}", "backward: worst error / bar", worst(host(xs[i].grad), ref_a, bar_a))
        ck.true(f"source {i}: the gradient has the source's type", xs[i].grad.dtype == xs[i].dtype)
        ck.true(f"source {i}: a voxel without live slots gets exactly 0", bool((host(xs[i].grad)[t_a == 0] == 0).all()))
        col += c
    ck.done()
