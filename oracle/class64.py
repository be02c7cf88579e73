"""Float64 reference of the class-sorted implicit GEMM (csrc/conv_class.hip): its plans, its products, the finish inside the product,
with the rounding bars of the fp32 and the half kernel - test infrastructure, not product code.  Plain numpy; nothing of taseg_amd
is imported.  tests/test_class64_host.py checks this file (helpers against brute force, a float32 emulation of both kernels inside
every bar, twelve emulated wrong kernels rejected); tests/test_gpu_class_float64.py holds the kernels against it.  The cases
(tables, channel pairs, operand families) live here so that both files run the same ones.

The weight-gradient sum that rides on a launch (`side`, an internal argument of ts_conv_class_gemm_ex) and the block calls of
csrc/block.hip, which reach these kernels with it: oracle/block64.py, tests/test_block64_host.py, tests/test_gpu_block_float64.py.

The plan.  nbr [K, n] (input row feeding destination row j through offset k, -1 = none) is cut into `groups` groups of gk = K / groups
offsets.  Per group a row's mask has bit kl set where nbr[gk g + kl][j] >= 0.  class_keys_kernel gives slot g npad + j the key
g 512 + (511 - mask) (padding rows j >= n: mask 0) and a stable radix sort orders them: inside a group ascending 511 - mask, equal keys
ascending row, rows without a neighbour in the group behind every live row, the padding last.  So the whole list is known: plan64
builds it and check_plan compares the device's arrays with it element by element - which holds every property the older tests
assert (every pair once, at the row pos names; dead rows and padding -1; every live tile listed once, longest first, with the union
mask of its rows) and the three they leave out (the key order, the stable order inside a key, every index inside its array).  Only the
order of the tile list inside one mask length is free (it follows the arrival of LDS atomics).  ts_conv_class_plan_pairs sorts
nothing: slot p is rulebook pair p.

The product.  Slot row i of group g (pass-2 plans) or destination row j (direct plans, g = 0) is
    z = sum over the live offsets kl of x[nbr[gk g + kl][j]] @ W_k,      k = gk g + kl,
W_k = W[K - 1 - k]^T when transposed and mirror, W[k]^T when transposed alone, W[k] otherwise (W as stored, [K, a, b]; the transposed
product reduces over b).  class_gemm64 returns z with S = sum_k |x| |W_k|, N = the count of non-zero products, L = the live offsets,
and, for the fp32 bar, the per-offset split bars already summed.

The bars.  u, SLACK, TINY and the charge of 2u per addition inside an MFMA are conv64's (see there).
  fp32, class_gemm_kernel: per offset of the tile's union mask the rows are staged (a slot that lacks the offset as zeros: `rlive`),
  split into h / m / l and multiplied by CG_MMA - TS_SPLIT_MMA's six products in the same order - into acc, which starts at +0 for
  every offset: the pair kernel's split product, bar_pass1_split(S_k, N_k).  Then tot += acc, a VALU add.  tot starts at +0, so the
  first add that carries anything is exact, and for an offset the slot lacks acc is an exact zero: L - 1 adds round, each by at
  most u of a partial sum that sum_k S_k bounds:
        |z - z64| <= sum_k bar_pass1_split(S_k, N_k) + SLACK (L - 1) u sum_k S_k
  L = 0 (a dead slot of a listed tile, a destination row without a pair): +0 + +0, exactly +0 bits.  A one-hot row with L = 1 has
  N = 1: the bar is SLACK 12.25 u SPLIT_SUM S, a few u.
  half, class_gemm_h_kernel: ONE accumulator set across every offset and row chunk of a tile, halves cast up, products exact in
  float32, N additions inside the matrix pipe (an offset the slot lacks, and the zero rows, add exact zeros), then one rounding:
        |z - z64| <= 2^-11 |z64| + SLACK N 2u S + 2^-25,            N, S summed over the live offsets
  with conv64.check_half's 65520 rule.
  pass 2 on plan["pos"] ([groups, n]): conv64.check_pass2 unchanged, on the device's own Z' cast up.
  ts_conv_class_conv[_f16]: no bar of its own - the bits of gather_sum(class_gemm(...), pos); with an addend
  (fp32 sum in group order + addend) rounded once (finish32 below).  Against float64 it is pass 2 with the addend as a fourth row.
"""
import numpy as np

from oracle.conv64 import (HALF_SUB, HALF_U, SLACK, TINY, U, Checks, bar_pass1_split, check_close, check_half,  # noqa: F401
                           check_pass2, features, rng, round_half, to_half, weights)
from oracle import conv64 as C

BM = 128


def npad_of(n):
    return (n + BM - 1) // BM * BM


# -------------------------------------------------------------------------------------------------------------------- plan

def masks(nbr, groups):
    """[groups, n] int64: bit kl of row j in group g is set where nbr[gk g + kl][j] >= 0"""
    k, n = nbr.shape
    assert k % groups == 0 and k // groups <= 9
    gk = k // groups
    live = (nbr >= 0).reshape(groups, gk, n)
    return (live * (1 << np.arange(gk))[None, :, None]).sum(1).astype(np.int64)


def live_rows(nbr, groups):
    """per group the rows with a neighbour in it, ascending"""
    return [np.nonzero(m)[0] for m in masks(nbr, groups)]


def plan64(nbr, groups, direct):
    """the plan ts_conv_class_plan must build: dict(src [gk, m_pad], pos [groups, n] | rows [m_pad], m_pad, tile_mask [m_pad / 128]
    (the union mask of a tile's rows), tile_rows [m_pad / 128] (the real rows a tile holds, dead ones included for direct plans),
    listed (the tiles of the list))"""
    k, n = nbr.shape
    gk, npad = k // groups, npad_of(n)
    m_pad = groups * npad
    msk = masks(nbr, groups)
    src = np.full((gk, m_pad), -1, dtype=np.int32)
    pos = np.full((groups, n), -1, dtype=np.int32)
    rows = np.full(m_pad, -1, dtype=np.int32)
    slot_mask = np.zeros(m_pad, dtype=np.int64)
    for g in range(groups):
        order = np.argsort(511 - msk[g], kind="stable")               # ascending key, equal keys ascending row
        at = g * npad + np.arange(n)
        rows[at] = order
        live = msk[g][order] != 0
        pos[g][order[live]] = at[live]
        src[:, at[live]] = nbr[gk * g:gk * g + gk][:, order[live]]
        slot_mask[at] = msk[g][order]
    tile_mask = np.bitwise_or.reduce(slot_mask.reshape(-1, BM), axis=1)
    tile_rows = (rows >= 0).reshape(-1, BM).sum(1)
    listed = np.nonzero((tile_mask != 0) | (tile_rows > 0 if direct else False))[0]
    out = dict(src=src, rows=rows, m_pad=m_pad, tile_mask=tile_mask, tile_rows=tile_rows, listed=listed)   # rows: the row of every slot
    if not direct:
        out["pos"] = pos
    return out


def plan_pairs64(nbmaps, nboffs, k):
    """the plan ts_conv_class_plan_pairs must build from a rulebook whose input rows are each in one pair: slot p = pair p"""
    p = int(nboffs[-1])
    m_pad = npad_of(p)
    src = np.full((k, m_pad), -1, dtype=np.int32)
    rows = np.full(m_pad, -1, dtype=np.int32)
    k_of = np.repeat(np.arange(k), np.diff(nboffs))
    src[k_of, np.arange(p)] = nbmaps[:, 1]
    rows[:p] = nbmaps[:, 0]
    slot_mask = np.zeros(m_pad, dtype=np.int64)
    slot_mask[:p] = 1 << k_of
    return dict(src=src, rows=rows, m_pad=m_pad, tile_mask=np.bitwise_or.reduce(slot_mask.reshape(-1, BM), axis=1),
                tile_rows=(rows >= 0).reshape(-1, BM).sum(1), listed=np.arange(m_pad // BM))


def _popcount(v):
    return np.array([bin(int(x)).count("1") for x in np.asarray(v).reshape(-1)], dtype=np.int64)


def check_plan(ck, nbr, groups, plan_arrays, direct, n_in=None, want=None):
    """A device plan - plan_arrays: src, pos | rows, tile_info, n_tiles, m_pad as host arrays / ints - against plan64(nbr).  n_in: the
    rows of the gathered operand (default n, a submanifold table).  want: the expected plan where it is not plan64's
    (plan_pairs64).  Returns True when nothing missed: the caller launches nothing on a plan that failed."""
    st = "plan"
    before = len(ck.missed)
    k, n = nbr.shape
    gk, npad = k // groups, npad_of(n)
    n_in = n if n_in is None else n_in
    want = plan64(nbr, groups, direct) if want is None else want
    src, m_pad = np.asarray(plan_arrays["src"]), int(plan_arrays["m_pad"])
    ck.true(st, f"m_pad {m_pad} != {groups} * {npad}", m_pad == want["m_pad"])
    ck.true(st, f"src shape {src.shape}", src.shape == (gk, want["m_pad"]) and src.dtype == np.int32)
    if len(ck.missed) > before:
        return False
    # every index a kernel follows lies inside its array
    ck.true(st, "an index of src outside [-1, n_in)", bool(src.min() >= -1 and src.max() < n_in))
    used = np.zeros(m_pad, dtype=bool)
    if direct:
        rows = np.asarray(plan_arrays["rows"])
        ck.true(st, "rows shape", rows.shape == (m_pad,))
        ck.true(st, "an index of rows outside [-1, n)", bool(rows.min() >= -1 and rows.max() < n))
        real = rows >= 0
        ck.true(st, "the destination rows are not listed exactly once each", np.array_equal(np.sort(rows[real]), np.arange(n)))
        ck.true(st, "src does not hold the table's column of its slot's row",
                np.array_equal(src[:, real], nbr[:, rows[real]]) and bool((src[:, ~real] == -1).all()))
        ck.true(st, "rows: not the stable order of the keys 511 - mask (ascending key, equal keys ascending row, padding last)",
                np.array_equal(rows, want["rows"]))
        used = real
    else:
        pos = np.asarray(plan_arrays["pos"])
        ck.true(st, "pos shape", pos.shape == (groups, n))
        ck.true(st, "an index of pos outside [-1, m_pad)", bool(pos.min() >= -1 and pos.max() < m_pad))
        got = np.full_like(nbr, -1)
        for g in range(groups):
            live = np.nonzero(pos[g] >= 0)[0]
            at = pos[g][live]
            ck.true(st, f"group {g}: two rows share a slot", len(np.unique(at)) == len(live))
            ck.true(st, f"group {g}: a slot outside the group's part of the list", bool(((at >= g * npad) & (at < (g + 1) * npad)).all()))
            inside = (at >= 0) & (at < m_pad)
            got[gk * g:gk * g + gk][:, live[inside]] = src[:, at[inside]]
            dead = np.nonzero(pos[g] < 0)[0]
            ck.true(st, f"group {g}: a row with a neighbour has no slot", bool((nbr[gk * g:gk * g + gk][:, dead] < 0).all()))
            used[at[inside]] = True
        ck.true(st, "src at the slots pos names is not the table", np.array_equal(got, nbr))
        ck.true(st, "a slot no row owns does not hold -1", bool((src[:, ~used] == -1).all()))
        ck.true(st, "pos: not the stable order of the keys 511 - mask (ascending key, equal keys ascending row)", np.array_equal(pos, want["pos"]))
    ck.true(st, "src is not the expected list", np.array_equal(src, want["src"]))
    # the tile list
    n_tiles = np.asarray(plan_arrays["n_tiles"]).reshape(-1)
    nt = int(n_tiles[0])
    ck.true(st, f"{nt} tiles listed, {len(want['listed'])} expected", nt == len(want["listed"]))
    if nt != len(want["listed"]) or nt > m_pad // BM:
        return False
    info = np.asarray(plan_arrays["tile_info"]).reshape(-1, 2)[:nt]
    tiles = info[:, 0] >> 2
    ck.true(st, "a tile is listed twice", len(np.unique(tiles)) == nt)
    ck.true(st, "the listed tiles are not the tiles with a live row", np.array_equal(np.sort(tiles), want["listed"]))
    ok = bool(((tiles >= 0) & (tiles < m_pad // BM)).all())
    ck.true(st, "a listed tile lies outside the list", ok)
    if ok:
        ck.true(st, "a tile's mask is not the union of its rows' masks", np.array_equal(info[:, 1], want["tile_mask"][tiles]))
        ck.true(st, "a tile's group bits are not its group", np.array_equal(info[:, 0] & 3, tiles // (npad // BM) if not direct else 0 * tiles))
    pop = _popcount(info[:, 1])
    ck.true(st, "the tiles are not listed longest first", bool((pop[:-1] >= pop[1:]).all()))
    ck.true(st, f"n_tiles[1] = {int(n_tiles[1])} is not the plan's (tile, offset) steps {int(pop.sum())}", int(n_tiles[1]) == int(pop.sum()))
    return len(ck.missed) == before


# ----------------------------------------------------------------------------------------------------------------- product

class Ref:
    """z, S, N, split (the per-offset split bars, summed) [groups, rows, c]; L [groups, rows]"""

    def __init__(self, z, s, n, live, split):
        self.z, self.S, self.N, self.L, self.split = z, s, n, live, split


def weight_slice(w, k, transposed, mirror):
    """the slice offset k multiplies with, [c_red, c_out]; w as stored"""
    if transposed:
        return w[w.shape[0] - 1 - k].T if mirror else w[k].T
    return w[k]


def class_gemm64(x, w, nbr, groups, transposed, mirror, rows=None, group=None):
    """The product of every (group, destination row) - rows: a subset of the destination rows, group: one group only - as a Ref.
    Row (g, j) is slot row plan.pos[g][j] of a pass-2 plan and destination row j of a direct plan (groups = 1)."""
    assert x.dtype == np.float64 and w.dtype == np.float64
    k_vol, n = nbr.shape
    gk = k_vol // groups
    rows = np.arange(n) if rows is None else np.asarray(rows)
    gs = range(groups) if group is None else (group,)
    c = w.shape[1] if transposed else w.shape[2]
    z, s, cnt, split = (np.zeros((len(gs), len(rows), c)) for _ in range(4))
    live_count = np.zeros((len(gs), len(rows)), dtype=np.int64)
    for gi, g in enumerate(gs):
        for kl in range(gk):
            k = gk * g + kl
            srcs = nbr[k][rows]
            at = np.nonzero(srcs >= 0)[0]
            if not len(at):
                continue
            wk = weight_slice(w, k, transposed, mirror)
            a = x[srcs[at]]
            sk = np.abs(a) @ np.abs(wk)
            nk = (a != 0).astype(np.float64) @ (wk != 0).astype(np.float64)
            z[gi, at] += a @ wk
            s[gi, at] += sk
            cnt[gi, at] += nk
            split[gi, at] += bar_pass1_split(sk, nk)
            live_count[gi, at] += 1
    return Ref(z, s, cnt, live_count, split)


def bar_class_f32(ref):
    return ref.split + SLACK * np.maximum(ref.L - 1, 0)[..., None] * U * ref.S


def bar_class_half(ref):
    return HALF_U * np.abs(ref.z) + SLACK * ref.N * 2 * U * ref.S + HALF_SUB


def bits(a):
    return a.view(np.int16) if a.dtype == np.float16 else a.view(np.int32)


def check_product(ck, stage, what, got, z64, bar, live, where=None):
    """product rows against their references in the same order (live [rows]: L): L = 0 exactly +0 bits, the others inside the bar"""
    rows = np.ones(len(live), dtype=bool) if where is None else where
    none, some = rows & (live == 0), rows & (live > 0)
    ck.true(stage, f"{what}: {int((bits(got)[none] != 0).sum())} elements of rows without a live offset are not +0", bool((bits(got)[none] == 0).all()))
    if some.any():
        if got.dtype == np.float16:
            check_half(ck, stage, what, got[some], z64[some], bar[some])
        else:
            check_close(ck, stage, what, got[some], z64[some], bar[some])


def check_slots(ck, stage, what, z, plan, ref, where=None):
    """Z' of a pass-2 plan: the slot rows pos names against ref [groups, n, c] (where: destination rows to look at), and the dead
    slots of the listed tiles +0"""
    pos = plan["pos"]
    bar = bar_class_half(ref) if z.dtype == np.float16 else bar_class_f32(ref)
    named = np.zeros(plan["m_pad"], dtype=bool)
    for g in range(pos.shape[0]):
        live = pos[g] >= 0
        named[pos[g][live]] = True
        w = live if where is None else live & where
        check_product(ck, stage, f"{what} group {g}", z[pos[g][w]], ref.z[g][w], bar[g][w], ref.L[g][w])
    info = np.asarray(plan["tile_info"]).reshape(-1, 2)[:int(np.asarray(plan["n_tiles"]).reshape(-1)[0])]
    in_listed = np.zeros(plan["m_pad"], dtype=bool)
    for t in info[:, 0] >> 2:
        in_listed[t * BM:(t + 1) * BM] = True
    dead = in_listed & ~named
    ck.true(stage, f"{what}: {int((bits(z)[dead] != 0).sum())} elements of the dead slots of listed tiles are not +0", bool((bits(z)[dead] == 0).all()))


def finish32(z, pos, addend, half):
    """what ts_conv_class_conv stores, from the two-launch form's own Z' rows: float32 sums in group order onto +0, then the addend,
    one rounding to half for half rows"""
    n = pos.shape[1]
    acc = np.zeros((n, z.shape[1]), dtype=np.float32)
    zf = z.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):                    # a half Z' row may hold inf
        for g in range(pos.shape[0]):
            live = pos[g] >= 0
            acc[live] = acc[live] + zf[pos[g][live]]
        if addend is not None:
            acc = acc + addend.astype(np.float32)
        return acc.astype(np.float16) if half else acc


def check_sums(ck, stage, what, got, z, pos):
    """pass 2 (or the finish, the addend a further row) on the device's own Z': conv64.check_pass2 on the rows whose Z' rows are all
    finite.  A half Z' row may hold inf (half_large: up to nine products of 60 000); the rows that add one are held to the float32
    sums in group order instead, NaN where those are NaN."""
    half = z.dtype == np.float16
    fin = np.ones(pos.shape[1], dtype=bool)
    for g in range(pos.shape[0]):
        live = pos[g] >= 0
        fin[live] &= np.isfinite(z[pos[g][live]]).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        check_pass2(ck, stage, what, bits(got), got, bits(z), f64(z), pos, half, where=fin)
        want = finish32(z, pos, None, half)[~fin]
    same = (bits(got[~fin]) == bits(want)) | (np.isnan(got[~fin]) & np.isnan(want))
    ck.true(stage, f"{what}: {int((~same).sum())} elements of rows that add a non-finite Z' row are not the float32 sum in group order", bool(same.all()))


def with_addend(z, pos, addend):
    """(Z' with the addend's rows behind it, pos with a fourth line naming them): the finish with an addend as a pass 2 for check_pass2"""
    n = pos.shape[1]
    line = (z.shape[0] + np.arange(n)).astype(np.int32)[None]
    return np.concatenate([z, addend]), np.concatenate([pos, line])


# ------------------------------------------------------------------------------------------------------------------- cases

SHIFTS = tuple(range(1, 14))              # shift of offset k < 13: nbr[k][j] = j + k + 1 (mod n), then the rows are renamed at random


def sub_table(n, fill, seed):
    """A submanifold-shaped table [27, n]: nbr[13][j] = j, and nbr[k][j] = i <=> nbr[26 - k][i] = j.  fill[k] for k < 13: the rows
    (before renaming) that have offset k - a boolean [n], or a fraction of the rows drawn at random.  Offset k pairs row j with
    j + k + 1 (mod n), offset 26 - k is its inverse; a random renaming of the rows makes it a symmetric random pairing.  The entries of
    a row are distinct input rows (13 distinct shifts and their negatives, n > 26)."""
    rs = rng("sub_table", n, seed)
    nbr = np.full((27, n), -1, dtype=np.int64)
    nbr[13] = np.arange(n)
    for k in range(13):
        f = fill.get(k, 0.0)
        has = np.asarray(f, dtype=bool) if np.ndim(f) else rs.rand(n) < f
        if has.any():
            assert n > 26
            j = np.nonzero(has)[0]
            i = (j + SHIFTS[k]) % n
            nbr[k][j], nbr[26 - k][i] = i, j
    name = rs.permutation(n)                                             # old row -> new row
    out = np.full((27, n), -1, dtype=np.int32)
    out[:, name] = np.where(nbr >= 0, name[np.maximum(nbr, 0)], -1)
    return out


def free_table(k, n, n_in, want, seed):
    """[k, n] from a boolean table `want`: every row's entries are distinct input rows drawn from n_in"""
    rs = rng("free_table", k, n, n_in, seed)
    nbr = np.full((k, n), -1, dtype=np.int32)
    for j in range(n):
        ks = np.nonzero(want[:, j])[0]
        nbr[ks, j] = rs.permutation(n_in)[:len(ks)]
    return nbr


def runs(n, lengths):
    """[len(lengths), n] boolean: run r of consecutive rows has entry r alone"""
    out = np.zeros((len(lengths), n), dtype=bool)
    at = 0
    for r, c in enumerate(lengths):
        out[r, at:at + c] = True
        at += c
    assert at <= n
    return out


def _sub(name):
    if name == "SUB1":                     # one row: its centre alone; z-planes 0 and 2 list no tile
        return sub_table(1, {}, 0)
    if name == "SUB127":                   # z-planes 0 and 2 empty; every row of the centre plane has all nine offsets
        return sub_table(127, {9: 1.0, 10: 1.0, 11: 1.0, 12: 1.0}, 0)
    if name == "SUB128":                   # the centre plane: exactly 128 live rows, one full tile; the outer planes a random third
        return sub_table(128, {k: 0.3 for k in range(13)}, 0)
    if name == "SUB129":                   # the centre plane: 129 live rows, a second tile of one row; z-plane 0: exactly 128 live rows
        rs = rng("SUB129")
        inside = np.zeros(129, dtype=bool)
        inside[rs.permutation(129)[:128]] = True
        fill = {k: inside & (rs.rand(129) < 0.4) for k in range(9)}
        fill[0] = fill[0] | (inside & ~np.any([fill[k] for k in range(9)], axis=0))
        fill.update({k: 0.5 for k in range(9, 13)})
        return sub_table(129, fill, 0)
    if name == "SUB257":                   # z-plane 0: one offset per row in runs, 129 live rows - tile 0 straddles seven masks, tile 1
        r = runs(257, [60, 0, 30, 20, 0, 10, 5, 3, 1])                   # holds one row; the centre plane: three tiles of mixed masks
        fill = {k: r[k] for k in range(9)}
        fill.update({k: 0.6 for k in range(9, 13)})
        return sub_table(257, fill, 0)
    raise KeyError(name)


def _free(name):
    if name == "NONE129":                  # no neighbour anywhere: n_tiles = 0
        return np.full((27, 129), -1, dtype=np.int32), 64
    if name == "FREE257":                  # z-plane 0 empty; plane 1: every row one offset, in runs (tiles that straddle two and
        want = np.zeros((27, 257), dtype=bool)                             # three masks); plane 2: exactly 129 rows, all nine offsets each
        want[9:18] = runs(257, [29, 0, 0, 128, 0, 72, 0, 28, 0])          # sorted: 28 + 72 + 28 | 100 + 28 | 1
        want[18:27, rng("FREE257").permutation(257)[:129]] = True
        return free_table(27, 257, 200, want, 0), 200
    raise KeyError(name)


def down_table(counts, n_coarse, seed):
    """a strided table's shape [8, n_coarse]: counts[k] coarse rows have a child through offset k, every fine row has one parent; the
    fine rows are numbered at random.  Coarse rows no offset draws have no pair."""
    rs = rng("down_table", tuple(counts), n_coarse, seed)
    nbr = np.full((8, n_coarse), -1, dtype=np.int32)
    fine = rs.permutation(int(sum(counts)))
    at = 0
    for k, c in enumerate(counts):
        nbr[k, np.sort(rs.permutation(n_coarse)[:c])] = fine[at:at + c]
        at += c
    return nbr


def children_table(children, seed):
    """a strided table's shape [8, len(children)]: coarse row j has children[j] children (1 .. 8) through offsets drawn at random, every
    fine row one parent; the fine rows are numbered at random"""
    rs = rng("children_table", tuple(children), seed)
    nbr = np.full((8, len(children)), -1, dtype=np.int32)
    fine = rs.permutation(int(sum(children)))
    at = 0
    for j, c in enumerate(children):
        assert 1 <= c <= 8
        nbr[np.sort(rs.permutation(8)[:c]), j] = fine[at:at + c]
        at += c
    return nbr


# D8: 44 coarse rows with 1 to 8 children each - eight rows with all eight (mask 0xFF: a direct tile of eight steps, L = 8), the others
# 1 .. 7 in turn; 205 pairs, every offset used, so every weight slice of a K = 8 kernel is multiplied in either direction
D8_CHILDREN = [8] * 8 + [1 + j % 7 for j in range(36)]
DOWN = {                                   # counts per offset (their sum: the pairs = the fine rows), coarse rows
    "D1": ([0, 0, 0, 1, 0, 0, 0, 0], 1),
    "D128": ([50, 0, 30, 0, 0, 40, 8, 0], 70),                            # one tile of 128 pairs over four offsets
    "D129": ([60, 0, 0, 40, 0, 28, 0, 1], 300),                           # tile 0 straddles three offsets, tile 1 holds one pair; 300 coarse
}                                                                           # rows: a whole tile of destination rows without a pair
DOWNS = tuple(DOWN) + ("D8",)
SUBS = ("SUB1", "SUB127", "SUB128", "SUB129", "SUB257")
FREES = ("NONE129", "FREE257")
EDGE_TABLES = ("SUB129", "SUB257")        # the contract checks; SUB257 carries the whole channel list
CHANNELS = [(32, 32), (32, 64), (64, 96), (96, 128), (96, 96), (128, 192), (256, 128), (192, 96), (160, 64), (384, 256)]
FEW_CHANNELS = [(32, 32), (96, 128), (256, 128)]
REFUSED_CHANNELS = [(48, 32), (32, 20), (32, 24)]
CASES = [("SUB257", c) for c in CHANNELS] + [(t, c) for t in SUBS + FREES + DOWNS if t != "SUB257" for c in FEW_CHANNELS]


def case_id(case):
    return f"{case[0]}-{case[1][0]}to{case[1][1]}"


_TABLES = {}


def table(name):
    """(nbr, n_in, groups, kind) - kind "sub" (symmetric: mirror and the finish apply), "free" (pass 1 and pass 2), "down" (direct)"""
    if name not in _TABLES:
        if name in SUBS:
            nbr = _sub(name)
            t = (nbr, nbr.shape[1], 3, "sub")
        elif name in FREES:
            t = _free(name) + (3, "free")
        elif name == "D8":
            t = (children_table(D8_CHILDREN, 0), int(sum(D8_CHILDREN)), 1, "down")
        else:
            counts, n_coarse = DOWN[name]
            t = (down_table(counts, n_coarse, 0), int(sum(counts)), 1, "down")
        t[0].setflags(write=False)
        check_table(*t)
        _TABLES[name] = t
    return _TABLES[name]


def check_table(nbr, n_in, groups, kind):
    """what the cases promise: indices in range, a row's entries distinct, the symmetry of the submanifold-shaped tables"""
    k, n = nbr.shape
    assert nbr.dtype == np.int32 and nbr.min() >= -1 and nbr.max(initial=-1) < n_in
    for j in range(n):
        e = nbr[:, j][nbr[:, j] >= 0]
        assert len(np.unique(e)) == len(e), "a row lists an input row twice"
    if kind == "sub":
        assert k == 27 and np.array_equal(nbr[13], np.arange(n))
        for kk in range(27):
            j = np.nonzero(nbr[kk] >= 0)[0]
            assert np.array_equal(nbr[26 - kk][nbr[kk][j]], j), "not symmetric under k -> 26 - k"
    if kind == "down":
        e = nbr[nbr >= 0]
        assert np.array_equal(np.sort(e), np.arange(n_in)), "every fine row has one parent"


def rulebook_of(nbr, n_in):
    """(nbmaps [P, 2] (input row, destination row), nboffs [K + 1], pos_in [K, n_in]) of a table, pairs by offset, then destination row"""
    k, n = nbr.shape
    nbmaps, nboffs = [], [0]
    pos_in = np.full((k, n_in), -1, dtype=np.int32)
    for kk in range(k):
        j = np.nonzero(nbr[kk] >= 0)[0]
        pos_in[kk, nbr[kk][j]] = nboffs[-1] + np.arange(len(j))
        nbmaps.append(np.stack([nbr[kk][j], j], 1))
        nboffs.append(nboffs[-1] + len(j))
    return np.concatenate(nbmaps).astype(np.int32).reshape(-1, 2), np.asarray(nboffs, dtype=np.int32), pos_in


def inverse_table(nbr, n_in):
    """[K, n_in]: the destination row input row i feeds through offset k, or -1 (what ts_conv_nbr_transposed builds)"""
    k = nbr.shape[0]
    out = np.full((k, n_in), -1, dtype=np.int32)
    for kk in range(k):
        j = np.nonzero(nbr[kk] >= 0)[0]
        out[kk, nbr[kk][j]] = j
    return out


def families(c_red, half):
    return C.families(c_red, half)


def operands(fam, n_in, k, c_red, c_out, transposed, half):
    """(x [n_in, c_red], w as stored: [K, c_red, c_out], or [K, c_out, c_red] when transposed): float32, or the halves"""
    x = features(fam, n_in, c_red, ("class", transposed), half)
    w = weights(fam, k, c_red, c_out, ("class", transposed), transposed, half)
    if not half:
        return x, w
    small = (w != 0) & (np.abs(w) < 2.0 ** -14)                          # half_large draws weights from (-240, 240): one nearer zero than
    w = np.where(small, np.copysign(np.float32(2.0 ** -14), w), w)       # the smallest normal half is set to it (to_half takes no subnormal)
    return to_half(x), to_half(w)


def addend_for(ref, pos, half):
    """[n, c]: even rows cancel the centre group's own sum (minus its float64 reference, rounded to the storage type) - what is left
    is the outer groups' rows against a large pair of terms, where a wrong order of the additions shows; odd rows dense"""
    n = pos.shape[1]
    c = ref.z.shape[2]
    add = features("dense", n, c, "addend", half).astype(np.float64)
    add[::2] = -ref.z[1][::2]
    add = np.clip(add, -60000.0, 60000.0)
    return add.astype(np.float16) if half else add.astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- LONG

def long_table(cus):
    """three groups, every row live in each, 128 * ceil((2 * 8 * cus + 1) / 3) rows: at least 2 * 8 * cus + 1 listed tiles - a CU holds at
    most 8 workgroups of 256 threads, so more than two rounds of the largest grid the half launch can size.  nbr[k][j] = j + 37 k + 1
    (mod n) under a random mask that keeps at least one offset per group: a row's entries are distinct."""
    tiles = 2 * 8 * cus + 1
    n = BM * (-(-tiles // 3))
    rs = rng("LONG", cus)
    m = rs.randint(1, 512, size=(3, n))
    has = ((m[:, None, :] >> np.arange(9)[None, :, None]) & 1).astype(bool).reshape(27, n)
    nbr = np.where(has, (np.arange(n)[None, :] + 37 * np.arange(27)[:, None] + 1) % n, -1).astype(np.int32)
    return nbr, tiles


# ------------------------------------------------------------------------------------------------------------- the runner
# One walk through a case for both test files.  `drv` makes the calls - the device's entry points, or the host emulation - on
# numpy operands and returns numpy results:
#   drv.plan(nbr, groups, direct) / drv.plan_pairs(nbmaps, nboffs, k, n_pairs) -> dict(src, pos | rows, tile_info, n_tiles, m_pad, ...)
#   drv.nbr_transposed(pos_in, nbmaps, k)                                     -> [k, n_in]
#   drv.gemm(x, w, plan, transposed, fill=0)   Z' [m_pad, c] (pass-2 plans; mirror = transposed) or the result [n, c] (direct plans);
#                                              the buffer holds pattern `fill` (0: NaN, 1: 7.0) before the launch
#   drv.gather_sum(z, plan)                    pass 2 on plan["pos"]
#   drv.conv(x, w, plan, transposed, addend, fill=0)   ts_conv_class_conv[_f16]
#   drv.two_pass(x, w, nbmaps, nboffs, pos, gather_col, transposed)   pair GEMM + pass 2 in fp32, or None where there is none (host)
# and reports what it watches itself (guard bands) to drv.ck.

def f64(a):
    return np.asarray(a).astype(np.float64)


def run_pass2_case(ck, name, c_red, c_out, drv, fams=None, kinds=(False, True), finish=True):
    """a three-group table: the plan, then per storage type, operand family and direction the product, pass 2 and - submanifold-shaped
    tables - the finish inside the product with and without an addend"""
    nbr, n_in, groups, kind = table(name)
    n = nbr.shape[1]
    plan = drv.plan(nbr, groups, False)
    if not check_plan(ck, nbr, groups, plan, False, n_in):
        return                                                            # nothing is launched on a plan that failed
    pos = plan["pos"]
    nt = int(np.asarray(plan["n_tiles"]).reshape(-1)[0])
    for half in kinds:
        sfx = "_half" if half else "_f32"
        for fam in fams or families(c_red, half):
            for transposed in (False, True):
                x, w = operands(fam, n_in, 27, c_red, c_out, transposed, half)
                ref = class_gemm64(f64(x), f64(w), nbr, groups, transposed, transposed)
                what = f"{fam} {'transposed, mirror' if transposed else 'forward'}"
                zs = [drv.gemm(x, w, plan, transposed, fill) for fill in (0, 1)]
                z = zs[0]
                ck.true("class" + sfx, f"{what}: shape {z.shape}", z.shape == (plan["m_pad"], c_out))
                if nt == 0:
                    ck.true("class" + sfx, f"{what}: a launch on an empty tile list wrote to Z'", bool(np.isnan(z).all()) and bool((zs[1] == 7).all()))
                check_slots(ck, "class" + sfx, what, z, plan, ref)
                ys = [drv.gather_sum(zz, plan) for zz in zs]
                ck.true("pass2" + sfx, f"{what}: shape", ys[0].shape == (n, c_out))
                ck.true("pass2" + sfx, f"{what}: the result depends on what Z' held before", np.array_equal(bits(ys[0]), bits(ys[1])))
                check_sums(ck, "pass2" + sfx, what, ys[0], z, pos)
                if kind != "sub" or not finish:
                    continue
                outs = [drv.conv(x, w, plan, transposed, None, fill) for fill in (0, 1)]
                ck.true("finish" + sfx, f"{what}: the result depends on what Z' and the result held before", np.array_equal(bits(outs[0]), bits(outs[1])))
                ck.true("finish" + sfx, f"{what}: {int((bits(outs[0]) != bits(ys[0])).sum())} elements differ from class GEMM + pass 2",
                        np.array_equal(bits(outs[0]), bits(ys[0])))
                add = addend_for(ref, pos, half)
                out = drv.conv(x, w, plan, transposed, add, 0)
                want = finish32(z, pos, add, half)
                ck.true("finish" + sfx, f"{what} + addend: {int((bits(out) != bits(want)).sum())} elements are not (fp32 sum in group order + addend) rounded once",
                        np.array_equal(bits(out), bits(want)))
                z4, pos4 = with_addend(z, pos, add)
                check_sums(ck, "finish" + sfx, f"{what} + addend", out, z4, pos4)


def run_direct_case(ck, name, c_red, c_out, drv, fams=None, kinds=(False, True)):
    """a strided table's shape: the plan of either direction (the inverse table through ts_conv_nbr_transposed, and the sort-free plan of
    the rulebook), and on each the forward and the weight_transposed product"""
    nbr, n_fine, _, _ = table(name)
    n_coarse = nbr.shape[1]
    nbmaps, nboffs, pos_in = rulebook_of(nbr, n_fine)
    pairs = int(nboffs[-1])
    pos_out = np.full((8, n_coarse), -1, dtype=np.int32)
    k_of = np.repeat(np.arange(8), np.diff(nboffs))
    pos_out[k_of, nbmaps[:, 1]] = np.arange(pairs)
    C.check_rulebook(nbmaps, nboffs, pos_out, pos_in, n_fine, n_coarse)
    assert pairs == n_fine
    down = drv.plan(nbr, 1, True)
    ok = check_plan(ck, nbr, 1, down, True, n_fine)
    nbr_t = drv.nbr_transposed(pos_in, nbmaps, 8)
    same = np.array_equal(nbr_t, inverse_table(nbr, n_fine))
    ck.true("plan", "ts_conv_nbr_transposed: not the inverse table", same)
    if not (ok and same):
        return
    up = drv.plan(nbr_t, 1, True)
    up2 = drv.plan_pairs(nbmaps, nboffs, 8, pairs)
    if not (check_plan(ck, nbr_t, 1, up, True, n_coarse) and
            check_plan(ck, nbr_t, 1, up2, True, n_coarse, want=plan_pairs64(nbmaps, nboffs, 8))):
        return
    # (plan, its table, rows of the gathered operand, the rulebook column the two-pass form gathers, its position table)
    sides = (("down", down, nbr, n_fine, 0, pos_out), ("up", up, nbr_t, n_coarse, 1, pos_in), ("up, from the pairs", up2, nbr_t, n_coarse, 1, pos_in))
    for half in kinds:
        stage = "direct_half" if half else "direct_f32"
        for fam in fams or families(c_red, half):
            for transposed in (False, True):
                first = {}
                for side, plan, tab, n_in, gcol, pos in sides:
                    x, w = operands(fam, n_in, 8, c_red, c_out, transposed, half)
                    ref = class_gemm64(f64(x), f64(w), tab, 1, transposed, False)
                    what = f"{fam} {side} {'transposed' if transposed else 'forward'}"
                    ys = [drv.gemm(x, w, plan, transposed, fill) for fill in (0, 1)]
                    y = ys[0]
                    ck.true(stage, f"{what}: shape {y.shape}", y.shape == (tab.shape[1], c_out))
                    ck.true(stage, f"{what}: the result depends on what the buffer held before", np.array_equal(bits(ys[0]), bits(ys[1])))
                    bar = (bar_class_half(ref) if half else bar_class_f32(ref))[0]
                    check_product(ck, stage, what, y, ref.z[0], bar, ref.L[0])
                    if gcol in first:
                        ck.true(stage, f"{what}: other bits than the sorted plan's", np.array_equal(bits(y), bits(first[gcol])))
                    first.setdefault(gcol, y)
                    two = None if half else drv.two_pass(x, w, nbmaps, nboffs, pos, gcol, transposed)
                    if two is not None:
                        one = ref.L[0] == 1
                        ck.true(stage, f"{what}: {int((bits(y)[one] != bits(two)[one]).sum())} elements of rows with one pair do not carry the bits of pair GEMM + pass 2",
                                np.array_equal(bits(y)[one], bits(two)[one]))


def run_case(ck, case, drv, **kw):
    name, (c_red, c_out) = case
    drv.ck = ck
    if table(name)[3] == "down":
        run_direct_case(ck, name, c_red, c_out, drv, **kw)
    else:
        run_pass2_case(ck, name, c_red, c_out, drv, **kw)


def listing_row(nbr, at_least=3, skip=(0,)):
    """an input row that at least three offsets list, not one of `skip`"""
    counts = np.bincount(nbr[nbr >= 0], minlength=nbr.shape[1]).astype(np.int64)
    counts[list(skip)] = 0
    row = int(np.argmax(counts))
    assert counts[row] >= at_least
    return row


def run_contracts(ck, name, c_red, c_out, drv, kinds=(False, True)):
    """on an edge table: the same launch twice and a freshly built plan give the same bits; NaN in input row 0 - the row a dead slot
    would read - and then in a row that three offsets list appears in exactly the Z' and result rows whose src lists the row"""
    nbr, n_in, groups, kind = table(name)
    assert kind == "sub"
    drv.ck = ck
    plan = drv.plan(nbr, groups, False)
    if not check_plan(ck, nbr, groups, plan, False, n_in):
        return
    pos = plan["pos"]
    again = drv.plan(nbr, groups, False)
    ck.true("plan", "a freshly built plan differs in src or pos", np.array_equal(plan["src"], again["src"]) and np.array_equal(pos, again["pos"]))
    if not check_plan(ck, nbr, groups, again, False, n_in):
        return
    for half in kinds:
        sfx = "_half" if half else "_f32"
        for transposed in (False, True):
            x, w = operands("dense", n_in, 27, c_red, c_out, transposed, half)
            ref = class_gemm64(f64(x), f64(w), nbr, groups, transposed, transposed)
            add = addend_for(ref, pos, half)
            what = "transposed, mirror" if transposed else "forward"
            z, y = drv.gemm(x, w, plan, transposed, 0), drv.conv(x, w, plan, transposed, add, 0)
            for p, tag in ((plan, "the same launch twice"), (again, "a freshly built plan")):
                z2, y2 = drv.gemm(x, w, p, transposed, 0), drv.conv(x, w, p, transposed, add, 0)
                live = pos >= 0
                ck.true("class" + sfx, f"{what}: {tag}: other bits", all(np.array_equal(bits(z)[pos[g][live[g]]], bits(z2)[pos[g][live[g]]]) for g in range(groups)))
                ck.true("finish" + sfx, f"{what}: {tag}: other bits", np.array_equal(bits(y), bits(y2)))
            for row in (0, listing_row(nbr)):
                xn = x.copy()
                xn[row, c_red // 2] = np.nan
                lists = (nbr.reshape(groups, -1, nbr.shape[1]) == row).any(1)          # [groups, n]: the slot rows whose src lists the row
                zn = drv.gemm(xn, w, plan, transposed, 0)
                with np.errstate(invalid="ignore"):
                    for g in range(groups):
                        live = pos[g] >= 0
                        hit = lists[g] & live
                        ck.true("class" + sfx, f"{what}, NaN in row {row}: a Z' row of group {g} that lists the row is finite",
                                bool(np.isnan(zn[pos[g][hit]]).all()))
                    check_slots(ck, "class" + sfx, f"{what}, NaN in row {row}", zn, plan, ref, where=~lists.any(0))
                    for g in range(groups):
                        live = pos[g] >= 0
                        rest = live & ~lists[g]
                        ck.true("class" + sfx, f"{what}, NaN in row {row}: NaN in a Z' row of group {g} that does not list the row",
                                not bool(np.isnan(zn[pos[g][rest]]).any()))
                    hit_y = lists.any(0)
                    for out, tag in ((drv.gather_sum(zn, plan), "pass2"), (drv.conv(xn, w, plan, transposed, None, 0), "finish"),
                                     (drv.conv(xn, w, plan, transposed, add, 0), "finish")):
                        ck.true(tag + sfx, f"{what}, NaN in row {row}: NaN is not in exactly the rows that list it",
                                bool(np.isnan(out[hit_y]).all()) and not bool(np.isnan(out[~hit_y]).any()))
