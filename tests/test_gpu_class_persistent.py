"""The persistent walk of the fp32 class GEMM (csrc/conv_class.hip, class_gemm_p_kernel: it reads the weight slices from the pre-split
bf16 planes of the weight) against the one-workgroup-per-tile kernel it replaces on the plain launch (ts_set_conv_impl(14), or a call
without planes, keeps that one: it splits the fp32 weight itself): the same plan and operands through both, compared BITWISE - Z'
or the result rows of a direct plan, the guard band behind them, the weight-gradient sum where one rides on the launch.  No
tolerance anywhere in this file.  (tests/test_gpu_class_float64.py holds the product itself against float64; its helpers make the
buffers here.)

The plans are written by hand, array by array, so that a case decides which tile a slot of the walk meets in which round: workgroup
`slot` of G takes tile round * G + slot of the list, the slot order reversed every other round; G is read from the device
(ts_conv_class_walk_slots).  `check_plan_arrays` holds every index of a plan against its range before anything is launched on it.
Every output buffer is NaN before each call: a tile nobody ran shows, and so does one that ran twice with different bits."""
import numpy as np
import pytest
import torch

from test_gpu_class_float64 import BAND, DEV, H, T, _L, band_kept, bits_t, buffer  # noqa: E402

pytestmark = pytest.mark.gpu

BM = 128
ONE_TILE_IMPL = 14


def slots_of(c_out, wt):
    L, lib = _L()
    g = int(lib.ts_conv_class_walk_slots(c_out, int(wt)))
    assert g >= 1
    return g


# ---------------------------------------------------------------------------------------------------------------- the plans

class Plan:
    """src [gk, m_pad], tile_info [m_pad / 128, 2], n_tiles [2], rows [m_pad] (direct) - numpy, and on the device"""

    def __init__(self, gk, groups, tiles_per_group, n_in, direct, seed):
        self.gk, self.groups, self.tpg, self.n_in, self.direct = gk, groups, tiles_per_group, n_in, direct
        self.K = gk * groups
        self.m_pad = groups * tiles_per_group * BM
        self.src = np.full((gk, self.m_pad), -1, dtype=np.int32)
        self.slot_mask = np.zeros(self.m_pad, dtype=np.int64)
        self.rows = np.full(self.m_pad, -1, dtype=np.int32) if direct else None
        self.list = []                      # tile numbers in list order
        self.n_listed = None                # n_tiles[0]; None: the whole list
        self.rs = np.random.RandomState(seed)

    def fill_tile(self, t, masks, first_row=1):
        """tile t (0 .. groups * tpg - 1): slot i gets the offsets of masks[i] (scalar: every slot), input rows drawn from
        first_row .. n_in - 1"""
        m = np.broadcast_to(np.asarray(masks, dtype=np.int64), (BM,))
        at = t * BM + np.arange(BM)
        self.slot_mask[at] = m
        for kl in range(self.gk):
            has = ((m >> kl) & 1).astype(bool)
            self.src[kl, at[has]] = self.rs.randint(first_row, self.n_in, size=int(has.sum()))

    def tile_mask(self, t):
        return int(np.bitwise_or.reduce(self.slot_mask[t * BM:(t + 1) * BM]))

    def finish(self, n_dest=None):
        """direct plans: slot -> destination row (a random renaming; slots from n_dest on are padding, rows = -1)"""
        if self.direct:
            n_dest = self.m_pad if n_dest is None else n_dest
            self.n_dest = n_dest
            self.rows[:n_dest] = self.rs.permutation(n_dest)
        else:
            self.n_dest = self.m_pad
        info = np.zeros((self.m_pad // BM, 2), dtype=np.int32)
        for at, t in enumerate(self.list):
            info[at] = (t // self.tpg + 4 * t, self.tile_mask(t))
        n_listed = len(self.list) if self.n_listed is None else self.n_listed
        steps = sum(bin(self.tile_mask(t)).count("1") for t in self.list[:n_listed])
        self.tile_info, self.n_tiles = info, np.array([n_listed, steps], dtype=np.int32)
        check_plan_arrays(self)
        self.dev = dict(src=T(self.src), tile_info=T(self.tile_info), n_tiles=T(self.n_tiles), rows=T(self.rows))
        return self


def check_plan_arrays(p):
    """every index a kernel can form from the plan is inside its array"""
    assert p.src.shape == (p.gk, p.m_pad) and p.src.dtype == np.int32 and p.src.min() >= -1 and p.src.max(initial=-1) < p.n_in
    assert p.m_pad % (p.groups * BM) == 0 and len(p.list) <= p.m_pad // BM and len(set(p.list)) == len(p.list)
    assert 0 <= p.n_tiles[0] <= len(p.list) and p.tile_info.shape == (p.m_pad // BM, 2)
    for at in range(len(p.list)):
        x, m = (int(v) for v in p.tile_info[at])
        assert 0 <= (x >> 2) < p.m_pad // BM and (x & 3) < p.groups and 0 <= m < (1 << p.gk)
        assert p.gk * (x & 3) + (m.bit_length() - 1 if m else 0) < p.K
    if p.direct:
        assert p.groups == 1 and p.rows.min() >= -1 and p.rows.max() < p.n_dest
        live = p.rows[p.rows >= 0]
        assert len(np.unique(live)) == len(live)


def operands(p, c_red, c_out, wt, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((p.n_in, c_red)).astype(np.float32)
    x[0] = np.nan                                                          # no src entry names row 0 (fill_tile draws from 1 on)
    w = (rs.standard_normal((p.K, c_out, c_red) if wt else (p.K, c_red, c_out)) * 0.25).astype(np.float32)
    return T(x), T(w)


def split_planes(wd):
    """the three bf16 planes of a weight, as the optimizer step's batch writes them"""
    L, lib = _L()
    planes = torch.empty(3 * wd.numel(), dtype=torch.int16, device=wd.device)
    L.check(lib.ts_conv_split_planes(L.ptr(wd), wd.shape[0], wd.shape[1], wd.shape[2], L.ptr(planes), L.stream()),
            "ts_conv_split_planes")
    return planes


def launch(p, xd, wd, c_out, wt, mirror, impl, side=None, planes="fresh"):
    """one call on a NaN buffer with the band behind it -> (the whole buffer, the weight-gradient sum or None).  The walk reads the
    weight's planes (handed over as the one-shot hint of the C entry): planes = "fresh" splits them here, a tensor is taken as it
    is, None makes the call without planes."""
    L, lib = _L()
    if isinstance(planes, str):
        planes = split_planes(wd)
    rows = p.n_dest if p.direct else p.m_pad
    z = buffer(rows, c_out, torch.float32, 0)
    d = p.dev
    args = (L.ptr(xd), xd.shape[1], L.ptr(wd), p.K, p.groups, c_out, L.ptr(d["src"]), p.m_pad, L.ptr(d["tile_info"]), L.ptr(d["n_tiles"]),
            int(wt), int(mirror), L.ptr(d["rows"]), L.ptr(z))
    dw = None
    lib.ts_set_conv_impl(impl)
    try:
        if planes is not None:
            lib.ts_conv_planes_hint(L.ptr(wd), L.ptr(planes), *wd.shape)
        if side is None:
            L.check(lib.ts_conv_class_gemm(*args, L.stream()), "ts_conv_class_gemm")
        else:
            part, nboffs, k, chunk, cacb = side
            dw = buffer(k, cacb, torch.float32, 0)
            L.check(lib.ts_conv_class_gemm_wsum(*args, L.ptr(part), L.ptr(nboffs), L.ptr(dw), k, chunk, cacb, L.stream()),
                    "ts_conv_class_gemm_wsum")
        torch.cuda.synchronize()
    finally:
        lib.ts_set_conv_impl(0)
    assert band_kept(z, rows), "the launch wrote behind its rows"
    return z, dw


def same_bits(a, b):
    return bool(torch.equal(bits_t(a), bits_t(b)))


def both(p, c_red, c_out, wt=False, mirror=False, seed=0, side=None, repeat=False):
    """the one-tile kernel and the walk on the same plan and operands: the same bits, band included -> the walk's buffer (host)"""
    xd, wd = operands(p, c_red, c_out, wt, seed)
    old, dw_old = launch(p, xd, wd, c_out, wt, mirror, ONE_TILE_IMPL, side)
    new, dw_new = launch(p, xd, wd, c_out, wt, mirror, 0, side)
    assert same_bits(old, new), f"{int((bits_t(old) != bits_t(new)).any(1).sum())} rows differ"
    if side is not None:
        assert same_bits(dw_old, dw_new) and band_kept(dw_new, side[2]) and not bool(torch.isnan(dw_new[:side[2]]).any())
    if repeat:
        again, _ = launch(p, xd, wd, c_out, wt, mirror, 0, side)
        assert same_bits(new, again)
    return H(new)


def written_rows(p, n_listed=None):
    """rows of the buffer a launch must have written: the slots of the listed tiles (their destination rows on a direct plan)"""
    listed = p.list[:len(p.list) if n_listed is None else n_listed]
    slots = (np.asarray(listed, dtype=np.int64)[:, None] * BM + np.arange(BM)[None, :]).reshape(-1)
    if p.direct:
        slots = p.rows[slots]
        slots = slots[slots >= 0]
    return slots


def check_coverage(p, z):
    """exactly the listed tiles' rows were written, none holds NaN (row 0 of x is NaN: nobody read it)"""
    rows = p.n_dest if p.direct else p.m_pad
    wrote = np.zeros(rows, dtype=bool)
    wrote[written_rows(p, int(p.n_tiles[0]))] = True
    nan_rows = np.isnan(z[:rows]).any(1)
    assert not nan_rows[wrote].any(), "a listed tile's row holds NaN"
    assert np.isnan(z[:rows][~wrote]).all(), "a row outside the listed tiles was written"


def by_length(p, tiles):
    """list order of the device plan: most offsets first"""
    return sorted(tiles, key=lambda t: -bin(p.tile_mask(t)).count("1"))


def random_masks(rs, gk, offsets):
    """a tile whose rows share `offsets` offsets drawn at random"""
    return int(sum(1 << int(k) for k in rs.permutation(gk)[:offsets]))


# ----------------------------------------------------------------------------------------------------------------- the cases

def test_one_listed_tile():
    """100 live rows in one tile, 32 -> 32: every other workgroup of the launch finds nothing"""
    p = Plan(9, 3, 2, 300, False, 1)
    m = np.zeros(BM, dtype=np.int64)
    m[:100] = p.rs.randint(1, 512, size=100)
    p.fill_tile(3, m)
    p.list = [3]
    p.finish()
    z = both(p, 32, 32, repeat=True)
    check_coverage(p, z)
    assert (z[3 * BM + 100:4 * BM].view(np.int32) == 0).all(), "a slot without a neighbour must hold +0"


@pytest.mark.parametrize("extra", ["G", "G+1", "2G+1"])
def test_rounds(extra):
    """direct plan, one group, 32 -> 32, G / G + 1 / 2 G + 1 listed tiles: a forward, a reversed and a forward round"""
    g = slots_of(32, False)
    n = {"G": g, "G+1": g + 1, "2G+1": 2 * g + 1}[extra]
    p = Plan(8, 1, n, 4096, True, 2)
    for t in range(n):
        p.fill_tile(t, random_masks(p.rs, 8, 1 + t % 2))
    p.list = by_length(p, range(n))
    p.finish(n * BM - 37)                                                   # rows = -1 padding in the last tile
    z = both(p, 32, 32, repeat=(extra == "2G+1"))
    check_coverage(p, z)


def test_one_offset_per_tile():
    """every tile a single-bit mask, R = 32: every slice boundary is a tile boundary, the prefetch chain at its shortest"""
    g = slots_of(32, False)
    n = 3 * (g + 2)
    p = Plan(9, 3, n // 3, 4096, False, 3)
    for t in range(n):
        p.fill_tile(t, 1 << (t % 9))
    p.list = list(range(n))
    p.finish()
    check_coverage(p, both(p, 32, 32))
    check_coverage(p, both(p, 32, 32, wt=True, mirror=True, seed=1))


@pytest.mark.parametrize("long_first", [True, False])
def test_mixed_tile_lengths(long_first):
    """a nine-offset tile followed by a one-offset tile in every other slot's walk, the reverse in the slots between"""
    g = slots_of(32, False)
    n = 3 * ((2 * g + 2) // 3 + 1)
    p = Plan(9, 3, n // 3, 4096, False, 4)
    kind = {}
    for s in range(g):                                                      # round 0: tile s, round 1: tile g + (g - 1 - s)
        first_long = (s % 2 == 0) == long_first
        kind[s], kind[g + (g - 1 - s)] = first_long, not first_long
    for t in range(2 * g):
        p.fill_tile(t, 511 if kind[t] else 1 << (t % 9))
    p.list = list(range(2 * g))
    p.finish()
    check_coverage(p, both(p, 64, 32))


def test_straddling_masks_and_dead_slots():
    """a tile straddling two masks, one straddling seven, a row with no neighbour in the group, a slot whose src is -1 for every
    offset: the dead slots hold exact +0, and nobody reads row 0 (NaN)"""
    p = Plan(9, 3, 2, 500, False, 5)
    two = np.where(np.arange(BM) < 70, 0b000000101, 0b110000000)
    seven = np.array([0b1, 0b10, 0b100, 0b1000, 0b10000, 0b100000, 0b1000000])[np.arange(BM) % 7]
    two[5], two[127], seven[64] = 0, 0, 0                                   # dead slots inside live tiles
    p.fill_tile(0, two)
    p.fill_tile(2, seven)
    p.fill_tile(5, 0b10101)
    p.list = by_length(p, [0, 2, 5])
    p.finish()
    for c_red, c_out, wt in ((32, 32, False), (96, 96, False), (96, 64, True), (64, 128, True)):
        z = both(p, c_red, c_out, wt=wt, mirror=wt)
        check_coverage(p, z)
        for slot in (5, 127, 2 * BM + 64):
            assert (z[slot].view(np.int32) == 0).all(), "a dead slot must hold +0"


def test_direct_plans_zero_tiles_inside_the_walk():
    """mask-0 tiles at the start, in the middle and at the end of a workgroup's walk (and a slot that meets nothing else);
    rows = -1 padding in the last tile"""
    g = slots_of(32, False)
    n = 3 * g
    p = Plan(8, 1, n, 4096, True, 6)
    walk = lambda s: [s, g + (g - 1 - s), 2 * g + s]                        # noqa: E731  the three tiles of slot s
    zero = {walk(0)[0], walk(1)[1], walk(2)[2], *walk(3), walk(g - 1)[0], walk(g - 1)[2], n - 1}
    for t in range(n):
        if t not in zero:
            p.fill_tile(t, random_masks(p.rs, 8, 1 + t % 3))
    p.list = list(range(n))
    p.finish(n * BM - 90)
    z = both(p, 32, 32)
    check_coverage(p, z)
    for t in zero:
        dst = p.rows[t * BM:(t + 1) * BM]
        assert (z[dst[dst >= 0]].view(np.int32) == 0).all(), "a tile without neighbours holds +0"
    check_coverage(p, both(p, 32, 64, wt=True, seed=1))


@pytest.mark.parametrize("c_out", [32, 64, 96, 128, 192])
def test_every_instantiation(c_out):
    """forward, transposed with mirror = 1 and mirror = 0, R in {32, 96, 256}, on a plan with fewer tiles than slots; 192 columns
    are two column tiles of 96"""
    p = Plan(9, 3, 4, 700, False, 7)
    live = [0, 1, 2, 5, 6, 9, 10, 11]
    for t in live:
        p.fill_tile(t, np.where(p.rs.rand(BM) < 0.9, random_masks(p.rs, 9, 1 + t % 5), 0))
    p.list = by_length(p, live)
    p.finish()
    for c_red in (32, 96, 256):
        for wt, mirror in ((False, False), (True, True), (True, False)):
            check_coverage(p, both(p, c_red, c_out, wt=wt, mirror=mirror, seed=c_red))


@pytest.mark.parametrize("c_out", [96, 128, 192])
def test_wide_tiles_over_two_rounds(c_out):
    """G + 3 tiles at the wide instantiations (their own G), 32 and 64 reduction columns, both directions"""
    for wt in (False, True):
        g = slots_of(c_out, wt)
        n = 3 * ((g + 3 + 2) // 3)
        p = Plan(9, 3, n // 3, 2048, False, 8)
        for t in range(g + 3):
            p.fill_tile(t, random_masks(p.rs, 9, 1 + t % 3))
        p.list = by_length(p, range(g + 3))
        p.finish()
        check_coverage(p, both(p, 64 if wt else 32, c_out, wt=wt, mirror=wt))


def test_n_tiles_below_the_bound():
    """n_tiles on the device says fewer tiles than the list holds entries (and than the launch's bound): the walk stops there"""
    g = slots_of(32, False)
    n = 3 * ((g + 40) // 3 + 1)
    p = Plan(9, 3, n // 3, 4096, False, 9)
    for t in range(g + 40):
        p.fill_tile(t, random_masks(p.rs, 9, 2))
    p.list = list(range(g + 40))
    p.n_listed = g + 7
    p.finish()
    check_coverage(p, both(p, 32, 32))
    small = Plan(9, 3, 4, 300, False, 10)
    for t in range(12):
        small.fill_tile(t, 0b11)
    small.list = list(range(12))
    small.n_listed = 5
    small.finish()
    check_coverage(small, both(small, 32, 64))


def test_weight_gradient_sum_rides_on_the_launch():
    """side.K > 0: 64 more workgroups form the ordered sum of weight-gradient partials - the same bits from both kernels, on a
    pass-2 plan over two rounds and on a direct plan"""
    rs = np.random.RandomState(11)
    k, chunk, cacb = 4, 128, 96 * 32
    nboffs = np.array([0, 300, 300, 700, 701], dtype=np.int32)             # chunks 0..2 | none | 2..5 | 5
    n_slots = (700 // chunk + 1) + k
    part = T(rs.standard_normal((n_slots, cacb)).astype(np.float32))
    side = (part, T(nboffs), k, chunk, cacb)
    g = slots_of(32, False)
    n = 3 * ((g + 5) // 3 + 1)
    p = Plan(9, 3, n // 3, 2048, False, 12)
    for t in range(g + 5):
        p.fill_tile(t, random_masks(p.rs, 9, 1 + t % 2))
    p.list = by_length(p, range(g + 5))
    p.finish()
    check_coverage(p, both(p, 32, 32, side=side, repeat=True))
    d = Plan(8, 1, 5, 600, True, 13)
    for t in range(4):
        d.fill_tile(t, random_masks(d.rs, 8, 2))
    d.list = by_length(d, range(5))
    d.finish(5 * BM - 11)
    check_coverage(d, both(d, 96, 96, wt=True, side=side))
    want = np.zeros((k, cacb), dtype=np.float32)
    ph = H(part)
    for kk in range(k):
        lo, hi = int(nboffs[kk]), int(nboffs[kk + 1])
        if hi > lo:
            for c in range(lo // chunk, (hi - 1) // chunk + 1):
                want[kk] += ph[c + kk]
    xd, wd = operands(d, 96, 96, True, 0)
    _, dw = launch(d, xd, wd, 96, True, False, 0, side)
    assert np.array_equal(H(dw[:k]).view(np.int32), want.view(np.int32))


def test_planes_refreshed_after_a_weight_change_and_a_call_without_planes():
    """the walk reads the weight through its planes: after one weight element changes, stale planes give the OLD result (they are
    what is read), refreshed planes the new one, and a call without planes takes the one-tile kernel and matches it"""
    p = Plan(9, 3, 2, 300, False, 14)
    for t in range(6):
        p.fill_tile(t, 0b111111111)
    p.list = list(range(6))
    p.finish()
    for c_red, c_out, wt in ((64, 96, False), (96, 64, True)):
        xd, wd = operands(p, c_red, c_out, wt, 0)
        kept = split_planes(wd)
        before, _ = launch(p, xd, wd, c_out, wt, wt, 0, planes=kept)
        wd[4, 3, 5] += 1.0
        torch.cuda.synchronize()
        old, _ = launch(p, xd, wd, c_out, wt, wt, ONE_TILE_IMPL, planes=None)
        stale, _ = launch(p, xd, wd, c_out, wt, wt, 0, planes=kept)
        assert same_bits(stale, before) and not same_bits(stale, old), "the walk did not read the planes it was given"
        kept.copy_(split_planes(wd))                                        # the refresh of the optimizer step
        new, _ = launch(p, xd, wd, c_out, wt, wt, 0, planes=kept)
        bare, _ = launch(p, xd, wd, c_out, wt, wt, 0, planes=None)
        assert same_bits(new, old) and same_bits(bare, old) and not same_bits(before, new)
