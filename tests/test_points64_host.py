"""oracle/points64.py on the CPU: the bars of tests/test_gpu_points_float64.py can be met and they discriminate.

For every family of inputs of the device test (small instances) the float32 emulation of each operation stays inside its
bar in natural, reversed and a seeded random order - the inputs are such that the reference alone passes - and each mutant of
the emulation (a dropped last slot, a dropped tail after the last group of four, the weight of corner k ^ 1, x as the innermost
corner axis, a forgotten / s^3, a partial sum rounded to half) misses one.  adjoint64 agrees with oracle/ts_oracle.py in
double, and <A x, y> = <x, A^T y> to 1e-12.
"""
import functools

import numpy as np
import pytest

from oracle import points64 as P
from oracle import ts_oracle as O

ORDERS = ["natural", "reversed", "random"]
C = 4


def worst(got, ref, bar):
    """largest error / bar; inf where a bar of 0 is missed"""
    err = np.abs(np.asarray(got).astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def family(name):
    """(idx, w, m) of the maps the device test uses, small"""
    if name.startswith("stride"):
        s = int(name[6:])
        pts, vox = P.scan_points(s, n_scan=300)
        idx, w = P.trilinear32(pts, vox, s)
        return idx, w, len(vox)
    if name.startswith("n="):
        return P.constructed_map(int(name[2:]))
    raise KeyError(name)


FAMILIES = ["n=1", "n=31", "n=32", "n=33", "n=400", "stride1", "stride4", "stride16"]


def rows(n, c, seed, half=False):
    x = np.random.RandomState(seed).randn(n, c).astype(np.float32)
    return x.astype(np.float16) if half else x


@pytest.mark.parametrize("name", FAMILIES)
def test_the_emulations_stay_inside_the_bars_in_every_order(name):
    idx, w, m = family(name)
    n = idx.shape[0]
    for half in (False, True):
        feat, gout = rows(m, C, 1, half), rows(n, C, 2, half)
        ref_f, t_f, s_f = P.devoxelize_forward64(feat, idx, w)
        ref_a, t_a, s_a = P.adjoint64(gout, idx, w, m)
        bar_f, bar_a = P.bar_sum(t_f, s_f, 8), P.bar_sum(t_a, s_a)
        assert np.abs(ref_f).max(initial=0) + bar_f.max(initial=0) < P.HALF_MAX and np.abs(ref_a).max() + bar_a.max() < P.HALF_MAX
        if half:
            bar_f, bar_a = P.bar_half(bar_f, ref_f), P.bar_half(bar_a, ref_a)
        for order in ORDERS:
            assert worst(P.devoxelize_forward32(feat, idx, w, order, half_out=half), ref_f, bar_f) <= 1
            assert worst(P.adjoint32(gout, idx, w, m, order, half_out=half), ref_a, bar_a) <= 1
            for piece in (1, 64):
                assert worst(P.adjoint32(gout, idx, w, m, order, partial_len=piece, half_out=half), ref_a, bar_a) <= 1
        dead = t_a == 0
        assert dead.any() or n < 400
        assert (ref_a[dead] == 0).all() and (P.adjoint32(gout, idx, w, m)[dead] == 0).all()


@pytest.mark.parametrize("name", FAMILIES)
def test_voxelize_emulation_stays_inside_the_bars(name):
    idx8, _, m = family(name)
    idx = idx8[:, 1].copy()                                  # a point -> voxel map with absent points
    n = idx.shape[0]
    counts = np.bincount(idx[idx >= 0], minlength=m).astype(np.int32)
    counts[m - 1] = 0                                        # a voxel whose points are dropped by the counts == 0 rule
    feat, gout = rows(n, C, 3), rows(m, C, 4)
    ref, t, s = P.voxelize_forward64(feat, idx, counts)
    for order in ORDERS:
        assert worst(P.voxelize_forward32(feat, idx, counts, order), ref, P.bar_sum(t, s)) <= 1
    refb, alive = P.voxelize_backward64(gout, idx, counts, n)
    got = P.voxelize_backward32(gout, idx, counts, n)
    assert worst(got, refb, P.SLACK * P.U * np.abs(refb) + P.TINY) <= 1
    assert (got[~alive] == 0).all() and (refb[~alive] == 0).all()
    if (counts > 1).any():                                   # a count that is off by one misses
        assert worst(P.voxelize_forward32(feat, idx, np.where(counts > 1, counts - 1, counts)), ref, P.bar_sum(t, s)) > 1


def test_the_slot_mutants_miss_the_adjoint_bar():
    idx, w, m = family("n=400")
    n = idx.shape[0]
    gout = rows(n, C, 2)
    ref, t, s = P.adjoint64(gout, idx, w, m)
    bar = P.bar_sum(t, s)
    # lists of 1, 3 and 9 slots.  On the list of 710 the bar (710 u S, about 7e-3 here) exceeds a single small term: there the
    # exact family below is what catches a dropped slot, by a whole number
    for v in (1, 2, 6):
        assert worst(P.adjoint32(gout, idx, w, m, drop_last_of=v), ref, bar) > 1, v
    for v in (4, 6, 7):                                      # 5 = 4 + 1, 9 = 8 + 1, 710 = 708 + 2
        assert worst(P.adjoint32(gout, idx, w, m, drop_tail4_of=v), ref, bar) > 1, v
    assert worst(P.adjoint32(gout, idx, w, m, drop_tail4_of=3), ref, bar) <= 1         # a list of exactly four has no tail
    assert worst(P.adjoint32(gout, idx, w, m, swap_corner=True), ref, bar) > 1
    assert worst(P.adjoint32(gout, idx, w, m, partial_len=64, partial_half=True), ref, bar) > 1
    feat = rows(m, C, 1)
    ref_f, t_f, s_f = P.devoxelize_forward64(feat, idx, w)
    assert worst(P.devoxelize_forward32(feat, idx, w, swap_corner=True), ref_f, P.bar_sum(t_f, s_f, 8)) > 1


@pytest.mark.parametrize("name", ["stride1", "stride4", "stride16"])
def test_the_slot_mutants_miss_on_a_real_map(name):
    """the maps of real scans have eight different weights per point: the weight of the neighbouring corner is another one"""
    idx, w, m = family(name)
    gout, feat = rows(idx.shape[0], C, 2), rows(m, C, 1)
    ref, t, s = P.adjoint64(gout, idx, w, m)
    bar = P.bar_sum(t, s)
    v = int(np.argmax(t))
    assert worst(P.adjoint32(gout, idx, w, m, drop_last_of=v), ref, bar) > 1
    assert worst(P.adjoint32(gout, idx, w, m, swap_corner=True), ref, bar) > 1
    ref_f, t_f, s_f = P.devoxelize_forward64(feat, idx, w)
    assert worst(P.devoxelize_forward32(feat, idx, w, swap_corner=True), ref_f, P.bar_sum(t_f, s_f, 8)) > 1


@pytest.mark.parametrize("half", [False, True])
def test_the_exact_family_is_exact_in_every_order_and_catches_the_mutants(half):
    idx, w, m = family("n=400")
    wx, feat, gout = P.exact_case(idx, w, m, C, 0)
    ref_a, ref_f = P.adjoint64(gout, idx, wx, m)[0], P.devoxelize_forward64(feat, idx, wx)[0]
    want_a, want_f = (ref_a.astype(np.float16), ref_f.astype(np.float16)) if half else (ref_a.astype(np.float32), ref_f.astype(np.float32))
    if not half:
        assert (want_a == ref_a).all() and (want_f == ref_f).all()
    for order in ORDERS:
        assert np.array_equal(P.adjoint32(gout, idx, wx, m, order, half_out=half), want_a)
        assert np.array_equal(P.adjoint32(gout, idx, wx, m, order, partial_len=64, half_out=half), want_a)
        assert np.array_equal(P.devoxelize_forward32(feat, idx, wx, order, half_out=half), want_f)
    assert not np.array_equal(P.adjoint32(gout, idx, wx, m, drop_last_of=7, half_out=half), want_a)
    assert not np.array_equal(P.adjoint32(gout, idx, wx, m, drop_tail4_of=7, half_out=half), want_a)
    assert not np.array_equal(P.adjoint32(gout, idx, wx, m, partial_len=64, partial_half=True, half_out=half), want_a)


@pytest.mark.parametrize("s", [1, 2, 4, 8, 16])
def test_trilinear_emulation_and_its_mutants(s):
    pts, vox = P.scan_points(s, n_scan=2000)
    idx, w64 = P.trilinear64(pts, vox, s)
    bar = P.bar_trilinear(w64)
    present = (idx >= 0).any(1)
    assert (~present).any() and (w64[~present] == 0).all() and (w64[idx < 0] == 0).all()
    assert ((idx >= 0) & (w64 == 0)).any()                   # a node: present corners of weight exactly 0
    assert np.abs(w64.sum(1)[present] - 1).max() > 0.1       # some sum is far from 1: the constant weighs there
    for order in ORDERS:
        got_idx, got = P.trilinear32(pts, vox, s, order)
        assert np.array_equal(got_idx, idx)
        assert worst(got, w64, bar) <= 1
        assert (got[idx < 0] == 0).all()
    assert worst(P.trilinear32(pts, vox, s, x_innermost=True)[1], w64, bar) > 1
    if s != 1:
        assert worst(P.trilinear32(pts, vox, s, forget_s3=True)[1], w64, bar) > 1
    # the numpy restatement of the reference's own code is an emulation too
    w_ref = O.calc_ti_weights(pts, idx.T, scale=s).T
    assert worst(w_ref, w64, bar) <= 1


@pytest.mark.parametrize("name", FAMILIES)
def test_adjoint64_against_ts_oracle_and_the_adjoint_identity(name):
    idx, w, m = family(name)
    n = idx.shape[0]
    rs = np.random.RandomState(9)
    x, y = rs.randn(m, C), rs.randn(n, C)
    ref_a, _, s_a = P.adjoint64(y, idx, w, m)
    ref_f, _, s_f = P.devoxelize_forward64(x, idx, w)
    assert (np.abs(ref_a - O.devoxelize_backward(y, idx, w, m)) <= 1e-12 * (s_a + 1)).all()
    assert (np.abs(ref_f - O.devoxelize_forward(x, idx, w)) <= 1e-12 * (s_f + 1)).all()
    lhs, rhs = float((ref_f * y).sum()), float((x * ref_a).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, float((s_f * np.abs(y)).sum()))
    # voxelize: mean pooling and its adjoint
    pidx = idx[:, 0].copy()
    counts = np.bincount(pidx[pidx >= 0], minlength=m).astype(np.int32)
    fwd, _, s_v = P.voxelize_forward64(y, pidx, counts)
    bwd, _ = P.voxelize_backward64(x, pidx, counts, n)
    assert abs(float((fwd * x).sum()) - float((y * bwd).sum())) <= 1e-12 * max(1.0, float((s_v * np.abs(x)).sum()))
    assert (np.abs(fwd - O.voxelize_forward(y, pidx, counts)) <= 1e-12 * (s_v + 1)).all()


def test_the_constructed_map_has_what_it_promises():
    idx, w, m = P.constructed_map(400)
    slots = np.bincount(idx[P.live(idx, w)], minlength=m)
    assert {int(slots[v]) for v in range(8)} == {0, 1, 3, 4, 5, 8, 9, 710}
    tuples, counts = np.unique(idx, axis=0, return_counts=True)
    assert set(P.CELLS) <= set(counts.tolist())
    assert (idx == -1).all(1).any() and ((idx >= 0) & (w == 0)).any()
    assert any(len(set(t[t >= 0].tolist())) < (t >= 0).sum() for t in tuples)          # a voxel twice in one tuple
    assert idx.min() == -1 and idx.max() < m
