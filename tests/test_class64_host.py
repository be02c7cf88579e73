"""oracle/class64.py - the float64 reference, the expected plan and the bars tests/test_gpu_class_float64.py holds the class-sorted
implicit GEMM to - checked without a device: the helpers against brute force, a float32 emulation of both kernels inside every bar at
every element of every case of the device test (LONG apart), and twelve emulated wrong kernels each rejected by the stage named
for it.

The emulation walks the tile list of the expected plan as csrc/conv_class.hip does, numpy float32 throughout:
  fp32    per tile and offset of the tile's union mask: the 128 gathered rows (zeros where a slot lacks the offset) and the weight slice
          split into h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); per 32-slice the six products of CG_MMA in its order
          (al bh, ah bl, am bm, am bh, ah bm, ah bh), each one float32 matrix product added to acc; then tot = fl(tot + acc), acc = +0
  half    halves cast up; ONE accumulator across the offsets and the row chunks of a tile, a float32 matrix product per 32-slice; one
          rounding to half when the tile is flushed.  The persistent walk: workgroup `slot` of G runs tile round G + slot, the slot
          order reversed in odd rounds
  pass 2  acc = +0; groups ascending: acc = fl(acc + z); half rows cast up and down once
  finish  class64.finish32 on the emulation's own Z' (what the kernel adds, in its order)
Z' and the results are NaN (or 7.0) before a launch, so a tile that is never run, a row that is never written, shows."""
import numpy as np
import pytest

from oracle import class64 as K
from oracle import conv64 as C

F32 = np.float32
SPLIT_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # CG_MMA: (plane of A, plane of B)


def bf16(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split3(x):
    x = np.asarray(x, dtype=F32)
    h = bf16(x)
    m = bf16(x - h)
    return h, m, bf16(x - h - m)


def row_chunk(c):
    return 128 if c % 128 == 0 else 96 if c % 96 == 0 else 64 if c % 64 == 0 else 32


class Emu:
    """the driver class64.run_case takes, on the expected plan; mutant: the wrong kernel it emulates"""

    def __init__(self, mutant=None, workgroups=3):
        self.mutant, self.G, self.ck = mutant, workgroups, None

    # ------------------------------------------------------------------------------------------------------------- plans
    def plan(self, nbr, groups, direct):
        p = K.plan64(nbr, groups, direct)
        pop = K._popcount(p["tile_mask"][p["listed"]])
        order = p["listed"][np.argsort(-pop, kind="stable")]
        grp = order // (K.npad_of(nbr.shape[1]) // K.BM) if not direct else 0 * order
        p["tile_info"] = np.stack([grp + 4 * order, p["tile_mask"][order]], 1).astype(np.int32)
        p["n_tiles"] = np.array([len(order), int(pop.sum())], dtype=np.int32)
        p.update(K=nbr.shape[0], groups=groups, direct=direct, n=nbr.shape[1])
        if not direct:
            del p["rows"]
        return p

    def plan_pairs(self, nbmaps, nboffs, k, n_pairs):
        p = K.plan_pairs64(nbmaps, nboffs, k)
        pop = K._popcount(p["tile_mask"])
        order = np.argsort(-pop, kind="stable")
        p["tile_info"] = np.stack([4 * order, p["tile_mask"][order]], 1).astype(np.int32)
        p["n_tiles"] = np.array([len(order), int(pop.sum())], dtype=np.int32)
        p.update(K=k, groups=1, direct=True, n=int(n_pairs))
        return p

    def nbr_transposed(self, pos_in, nbmaps, k):
        return np.where(pos_in >= 0, nbmaps[np.maximum(pos_in, 0), 1], -1).astype(np.int32)

    # ----------------------------------------------------------------------------------------------------------- product
    def tiles_run(self, n_tiles, half):
        """list indices in the order they are run (a tile may come twice, or never)"""
        if not half:
            return list(range(n_tiles))
        G, out = min(self.G, max(n_tiles, 1)), []
        for slot in range(G):
            rnd = 0
            while True:
                rev = rnd & 1 and not (self.mutant == "round1_not_reversed" and rnd == 1 and slot == 0)
                t = rnd * G + (G - 1 - slot if rev else slot)
                if t >= n_tiles:
                    break
                out.append(t)
                rnd += 1
        return out

    def gemm(self, x, w, plan, transposed, fill=0, phase=0, out=None, addend=None):
        with np.errstate(over="ignore", invalid="ignore"):             # half_large: sums of 65520 or more are inf, as on the device
            return self._gemm(x, w, plan, transposed, fill, phase, out, addend)

    def _gemm(self, x, w, plan, transposed, fill, phase, out, addend):
        half = x.dtype == np.float16
        xf, wf = x.astype(F32), w.astype(F32)
        mut, kvol, groups, direct = self.mutant, plan["K"], plan["groups"], plan["direct"]
        gk = kvol // groups
        mirror = transposed and not direct
        c_red = x.shape[1]
        c = w.shape[1] if transposed else w.shape[2]
        src = plan["src"]
        z = np.full((plan["n"] if direct else plan["m_pad"], c), [np.nan, 7.0][fill], dtype=x.dtype) if out is None else out
        info = plan["tile_info"][:int(plan["n_tiles"][0])]
        tiles_per_group = plan["m_pad"] // groups // K.BM
        for ti in self.tiles_run(len(info), half):
            tile, grp, mask = int(info[ti, 0]) >> 2, int(info[ti, 0]) & 3, int(info[ti, 1])
            slots = np.arange(tile * K.BM, (tile + 1) * K.BM)
            if phase and (grp == 1) != (phase == 2):
                continue
            if mask == 0:                                                   # direct plans: destination rows without a pair
                dst = plan["rows"][slots]
                if mut != "dead_unwritten":
                    z[dst[dst >= 0]] = 0
                continue
            read = slots
            if mut == "second_tile_first_src" and tile % tiles_per_group == 1:
                read = slots - K.BM
            if mut == "first_row_mask":
                mask = int(sum(1 << kl for kl in range(gk) if src[kl][slots[0]] >= 0)) or mask
            tot = np.zeros((K.BM, c), dtype=F32)
            for kl in range(gk):
                if not (mask >> kl) & 1:
                    continue
                k = kl if mut == "no_group" else gk * grp + kl
                kw = k
                if (transposed and mirror and mut != "mirror_ignored") or (not transposed and mut == "mirror_forward"):
                    kw = kvol - 1 - k
                rows = src[kl][read]
                a = xf[np.maximum(rows, 0)]
                if mut != "dead_reads_row0":
                    a = np.where((rows >= 0)[:, None], a, F32(0))
                wk = wf[kw].T if transposed else wf[kw]
                red = c_red
                if mut == "drop_last_slice" and not half:
                    red = c_red - 32
                if mut == "drop_last_chunk" and half and c_red > row_chunk(c_red):
                    red = c_red - row_chunk(c_red)
                acc = np.zeros((K.BM, c), dtype=F32)
                if half:
                    for s0 in range(0, red, 32):
                        acc = acc + a[:, s0:s0 + 32] @ wk[s0:s0 + 32]
                    if mut == "round_per_offset":
                        acc = acc.astype(np.float16).astype(F32)
                else:
                    pa, pb = split3(a), split3(wk)
                    for s0 in range(0, red, 32):
                        for i, j in SPLIT_ORDER:
                            acc = acc + pa[i][:, s0:s0 + 32] @ pb[j][s0:s0 + 32]
                tot = tot + acc
            if phase == 2:                                                  # the centre group's tiles store the result rows
                r = src[4][slots]
                live = r >= 0
                v = np.zeros((K.BM, c), dtype=F32)
                pos, zf = plan["pos"], z.astype(F32)
                th = tot.astype(np.float16).astype(F32) if half else tot
                if mut == "addend_first" and addend is not None:
                    v[live] = v[live] + addend[r[live]].astype(F32)
                for g, own in ((0, None), (1, th), (2, None)):
                    if own is not None:
                        v = v + own
                    else:
                        p = np.where(live, pos[g][np.maximum(r, 0)], -1)
                        v = np.where((p >= 0)[:, None], v + zf[np.maximum(p, 0)], v)
                if mut != "addend_first" and addend is not None:
                    v[live] = v[live] + addend[r[live]].astype(F32)
                with np.errstate(over="ignore"):
                    out_rows = v.astype(x.dtype)
                self.result[r[live]] = out_rows[live]
                continue
            with np.errstate(over="ignore"):
                res = tot.astype(np.float16) if half else tot
            if direct:
                dst = plan["rows"][slots]
                z[dst[dst >= 0]] = res[dst >= 0]
            else:
                z[slots] = res
        return z

    def gather_sum(self, z, plan):
        return K.finish32(z, plan["pos"], None, z.dtype == np.float16)

    def conv(self, x, w, plan, transposed, addend, fill=0):
        c = w.shape[1] if transposed else w.shape[2]
        self.result = np.full((plan["n"], c), [np.nan, 7.0][fill], dtype=x.dtype)
        z = self.gemm(x, w, plan, transposed, fill, phase=1)
        self.gemm(x, w, plan, transposed, fill, phase=2, out=z, addend=addend)
        return self.result

    def two_pass(self, *args):
        return None


# ------------------------------------------------------------------------------------------------------------- emulation

@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_the_emulation_stays_inside_every_bar(case):
    ck = K.Checks(K.case_id(case), "class_float64 emulation")
    K.run_case(ck, case, Emu())
    ck.done()
    assert all(v <= 1.0 for v in ck.ratios.values())


@pytest.mark.parametrize("name", K.EDGE_TABLES)
def test_the_emulation_keeps_the_contracts(name):
    ck = K.Checks(f"contracts {name}", "class_float64 emulation")
    K.run_contracts(ck, name, 32, 32, Emu())
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- mutants

MUTANTS = [   # (wrong kernel, the stage whose check must miss, half, case, operand families, contracts instead of the stages)
    ("dead_reads_row0", "class_f32", False, ("SUB257", (32, 32)), ("dense",), False),
    ("dead_reads_row0", "class_half", True, ("FREE257", (32, 32)), ("dense",), False),
    ("dead_reads_row0", "class_f32", False, ("SUB257", (32, 32)), None, True),
    ("mirror_ignored", "class_f32", False, ("SUB129", (32, 32)), ("dense",), False),
    ("mirror_forward", "class_half", True, ("SUB129", (32, 32)), ("dense",), False),
    ("no_group", "class_f32", False, ("SUB257", (32, 32)), ("one_hot",), False),
    ("drop_last_slice", "class_f32", False, ("SUB257", (96, 96)), ("two_hot",), False),
    ("drop_last_chunk", "class_half", True, ("SUB257", (256, 128)), ("dense",), False),
    ("drop_last_chunk", "direct_half", True, ("D129", (256, 128)), ("one_hot",), False),
    ("second_tile_first_src", "class_f32", False, ("SUB257", (32, 32)), ("dense",), False),
    ("second_tile_first_src", "direct_half", True, ("D129", (32, 32)), ("dense",), False),
    ("first_row_mask", "class_f32", False, ("SUB257", (32, 32)), ("dense",), False),
    ("first_row_mask", "class_half", True, ("FREE257", (32, 32)), ("one_hot",), False),
    ("round1_not_reversed", "class_half", True, ("SUB257", (32, 32)), ("dense",), False),
    ("round_per_offset", "class_half", True, ("SUB127", (32, 32)), ("dense",), False),
    ("addend_first", "finish_half", True, ("SUB257", (32, 32)), ("dense",), False),
    ("dead_unwritten", "direct_f32", False, ("D129", (32, 32)), ("dense",), False),
    ("dead_unwritten", "direct_half", True, ("D129", (32, 32)), ("dense",), False),
]


def _run(ck, case, half, fams, contracts, mutant):
    if contracts:
        K.run_contracts(ck, case[0], case[1][0], case[1][1], Emu(mutant), kinds=(half,))
    else:
        K.run_case(ck, case, Emu(mutant), fams=fams, kinds=(half,))


@pytest.mark.parametrize("mutant,stage,half,case,fams,contracts", MUTANTS,
                         ids=[f"{m[0]}-{m[1]}-{K.case_id(m[3])}{'-contracts' if m[5] else ''}" for m in MUTANTS])
def test_a_wrong_kernel_is_rejected_by_its_stage(mutant, stage, half, case, fams, contracts):
    ck = K.Checks(f"{mutant} {K.case_id(case)}", "class_float64 mutant")
    _run(ck, case, half, fams, contracts, mutant)
    print("\n".join(ck.lines()) + f"\n  first: {ck.missed[0] if ck.missed else None}")
    assert ck.missed, f"{mutant} passed every check of {K.case_id(case)}"
    assert any(m.startswith(stage + " ") for m in ck.missed), f"{mutant}: no check of {stage} missed: {ck.missed[:5]}"
    sound = K.Checks("sound")
    _run(sound, case, half, fams, contracts, None)
    assert not sound.missed                              # the same case without the mutation passes


# ---------------------------------------------------------------------------------------------------------------- helpers

@pytest.mark.parametrize("name", K.SUBS + K.FREES + K.DOWNS)
def test_the_tables_are_the_ones_asked_for(name):
    nbr, n_in, groups, kind = K.table(name)
    k, n = nbr.shape
    for j in range(n):                                     # brute force: a row's entries are distinct rows of the gathered operand
        e = [int(v) for v in nbr[:, j] if v >= 0]
        assert len(set(e)) == len(e) and all(0 <= v < n_in for v in e)
    if kind == "sub":
        assert all(nbr[13, j] == j for j in range(n))
        for kk in range(27):
            for j in range(n):
                if nbr[kk, j] >= 0:
                    assert nbr[26 - kk, nbr[kk, j]] == j
    live = [len(r) for r in K.live_rows(nbr, groups)]
    msk = K.masks(nbr, groups)
    want = {"SUB1": [0, 1, 0], "SUB127": [0, 127, 0], "SUB128": [None, 128, None], "SUB129": [128, 129, None], "SUB257": [129, 257, None],
            "NONE129": [0, 0, 0], "FREE257": [0, 257, 129]}.get(name)
    if want:
        assert all(w is None or w == got for w, got in zip(want, live)), live
    if name == "SUB127":
        assert (msk[1] == 511).all()
    if name == "FREE257":
        assert (msk[2][msk[2] != 0] == 511).all() and all(bin(int(m)).count("1") == 1 for m in msk[1])
        tiles = np.sort(511 - msk[1], kind="stable").reshape(-1)
        assert len(set(tiles[:128].tolist())) == 3 and len(set(tiles[128:256].tolist())) == 2      # tiles that straddle three and two masks
    if name == "SUB257":
        assert all(bin(int(m)).count("1") <= 1 for m in msk[0])
        assert len(set(np.sort(511 - msk[0], kind="stable")[:128].tolist())) >= 3
    if name == "D8":                                        # the strided shape: 1 to 8 children per coarse row, every offset used
        children = (nbr >= 0).sum(0)
        assert sorted(set(children.tolist())) == list(range(1, 9)) and (children == 8).sum() == 8
        assert ((nbr >= 0).sum(1) > 0).all() and (K.masks(nbr, 1)[0] == 0xFF).sum() == 8
        assert children.tolist() == K.D8_CHILDREN and n_in == children.sum() == 205
    elif kind == "down":
        counts, n_coarse = K.DOWN[name]
        assert n == n_coarse and [int((nbr[kk] >= 0).sum()) for kk in range(8)] == counts and n_in == sum(counts)
        assert sum(counts) in (1, 128, 129)
        if name == "D129":
            assert ((nbr >= 0).sum(0) == 0).sum() > 128               # a whole tile of destination rows without a pair


def test_channel_pairs_reach_every_tile_width():
    col = lambda c: 128 if c % 128 == 0 else 96 if c % 96 == 0 else 64 if c % 64 == 0 else 32  # noqa: E731
    outs = {(col(c), c // col(c)) for _, c in K.CHANNELS}                         # the result has c_out columns in either direction
    assert {(128, 1), (96, 1), (64, 1), (32, 1), (96, 2), (128, 2)} <= outs
    chunks = {(row_chunk(c), c // row_chunk(c)) for c, _ in K.CHANNELS}             # and the reduction runs over c_red
    assert {(128, 1), (96, 1), (64, 1), (32, 1), (128, 2), (96, 2), (128, 3)} <= chunks


def _brute_masks(nbr, groups):
    k, n = nbr.shape
    gk = k // groups
    return [[sum(1 << kl for kl in range(gk) if nbr[gk * g + kl, j] >= 0) for j in range(n)] for g in range(groups)]


@pytest.mark.parametrize("name", K.DOWNS)
def test_plan_pairs64_against_brute_force(name):
    """slot p = pair p of the rulebook: its input row in rows, its destination row in src at its own offset alone, mask = 1 << offset"""
    nbr, n_fine, _, _ = K.table(name)
    nbmaps, nboffs, pos_in = K.rulebook_of(nbr, n_fine)
    pairs = [(kk, int(nbr[kk, j]), j) for kk in range(8) for j in range(nbr.shape[1]) if nbr[kk, j] >= 0]      # by offset, then destination row
    assert [(int(a), int(b)) for a, b in nbmaps] == [(i, j) for _, i, j in pairs]
    assert [int(v) for v in nboffs] == [sum(1 for kk, _, _ in pairs if kk < k) for k in range(9)]
    for kk, i, j in pairs:
        assert nbmaps[pos_in[kk, i]].tolist() == [i, j]
    p = K.plan_pairs64(nbmaps, nboffs, 8)
    m_pad = (len(pairs) + 127) // 128 * 128
    assert p["m_pad"] == m_pad and p["src"].shape == (8, m_pad) and p["rows"].shape == (m_pad,)
    for slot in range(m_pad):
        col = [int(v) for v in p["src"][:, slot]]
        if slot < len(pairs):
            kk, i, j = pairs[slot]
            assert p["rows"][slot] == i and col == [j if k == kk else -1 for k in range(8)]
        else:
            assert p["rows"][slot] == -1 and col == [-1] * 8
    for t in range(m_pad // 128):
        union = 0
        for kk, _, _ in pairs[t * 128:(t + 1) * 128]:
            union |= 1 << kk
        assert p["tile_mask"][t] == union and p["tile_rows"][t] == len(pairs[t * 128:(t + 1) * 128])
    assert p["listed"].tolist() == list(range(m_pad // 128))
    inv = K.inverse_table(nbr, n_fine)                      # the table the plan belongs to
    for kk, i, j in pairs:
        assert inv[kk, i] == j
    assert (inv >= 0).sum() == len(pairs)


@pytest.mark.parametrize("name", ["SUB129", "SUB257", "FREE257", "NONE129", "D128", "D129", "D8"])
def test_plan64_against_brute_force(name):
    nbr, n_in, groups, kind = K.table(name)
    direct = kind == "down"
    k, n = nbr.shape
    gk, npad = k // groups, K.npad_of(n)
    msk = _brute_masks(nbr, groups)
    assert np.array_equal(K.masks(nbr, groups), np.array(msk))
    p = K.plan64(nbr, groups, direct)
    for g in range(groups):
        order = sorted(range(n), key=lambda j: (511 - msk[g][j], j))
        for i, j in enumerate(order):
            slot = g * npad + i
            assert p["rows"][slot] == j
            if msk[g][j]:
                assert direct or p["pos"][g][j] == slot
                assert [int(v) for v in p["src"][:, slot]] == [int(nbr[gk * g + kl, j]) for kl in range(gk)]
            else:
                assert (direct or p["pos"][g][j] == -1) and (p["src"][:, slot] == -1).all()
        assert (p["rows"][g * npad + n:(g + 1) * npad] == -1).all() and (p["src"][:, g * npad + n:(g + 1) * npad] == -1).all()
    for t in range(groups * npad // 128):
        rows = [int(r) for r in p["rows"][t * 128:(t + 1) * 128] if r >= 0]
        g = t // (npad // 128)
        union = 0
        for j in rows:
            union |= msk[g][j]
        assert p["tile_mask"][t] == union and ((t in p["listed"]) == bool(union or (direct and rows)))


def test_check_plan_rejects_wrong_plans():
    nbr, n_in, groups, kind = K.table("SUB257")
    good = Emu().plan(nbr, 3, False)

    def missed(change):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        change(p)
        ck = K.Checks("bad plan")
        assert not K.check_plan(ck, nbr, 3, p, False, n_in)
        return ck.missed

    ck = K.Checks("good plan")
    assert K.check_plan(ck, nbr, 3, good, False, n_in) and not ck.missed

    def swap_equal_keys(p):                                # two rows of one key in descending row order: every older property holds
        msk = K.masks(nbr, 3)[1]
        order = np.argsort(511 - msk, kind="stable")
        i = next(i for i in range(len(order) - 1) if msk[order[i]] == msk[order[i + 1]])
        a, b = order[i], order[i + 1]
        sa, sb = p["pos"][1][a], p["pos"][1][b]
        p["pos"][1][a], p["pos"][1][b] = sb, sa
        p["src"][:, [sa, sb]] = p["src"][:, [sb, sa]]

    def out_of_range(p):
        p["src"][0, p["pos"][0][p["pos"][0] >= 0][0]] = n_in

    def swap_tiles(p):
        p["tile_info"][[0, -1]] = p["tile_info"][[-1, 0]]

    def lose_tile(p):
        p["n_tiles"][0] -= 1

    def wrong_mask(p):
        p["tile_info"][0, 1] ^= 1

    assert any("stable order" in m for m in missed(swap_equal_keys))
    assert any("outside [-1, n_in)" in m for m in missed(out_of_range))
    assert any("longest first" in m for m in missed(swap_tiles))
    assert missed(lose_tile) and any("union" in m for m in missed(wrong_mask))


def test_class_gemm64_against_loops():
    nbr, n_in, groups, _ = K.table("FREE257")
    rs = np.random.RandomState(3)
    x, w = rs.randn(n_in, 3), rs.randn(27, 3, 2)
    x[5] = 0
    for transposed, mirror in ((False, False), (True, False), (True, True)):
        ws = np.ascontiguousarray(w.transpose(0, 2, 1)) if transposed else w
        ref = K.class_gemm64(x, ws, nbr, 3, transposed, mirror)
        for g in range(3):
            for j in range(0, nbr.shape[1], 7):
                z, s, cnt, live = np.zeros(2), np.zeros(2), np.zeros(2), 0
                for kl in range(9):
                    k = 9 * g + kl
                    if nbr[k, j] >= 0:
                        wk = w[26 - k] if (transposed and mirror) else w[k]
                        live += 1
                        for o in range(2):
                            terms = [x[nbr[k, j], r] * wk[r, o] for r in range(3)]
                            z[o] += sum(terms)
                            s[o] += sum(abs(t) for t in terms)
                            cnt[o] += sum(1 for t in terms if t != 0)
                assert np.allclose(ref.z[g, j], z, atol=1e-13) and np.allclose(ref.S[g, j], s, atol=1e-13)
                assert np.array_equal(ref.N[g, j], cnt) and ref.L[g, j] == live
    sub = K.class_gemm64(x, w, nbr, 3, False, False, rows=np.array([3, 200, 9]), group=2)
    full = K.class_gemm64(x, w, nbr, 3, False, False)
    assert np.array_equal(sub.z[0], full.z[2][[3, 200, 9]]) and np.array_equal(sub.L[0], full.L[2][[3, 200, 9]])


def test_a_one_hot_row_with_one_offset_is_held_to_a_few_u():
    nbr, n_in, groups, _ = K.table("SUB257")
    x, w = K.operands("one_hot", n_in, 27, 32, 32, False, False)
    ref = K.class_gemm64(K.f64(x), K.f64(w), nbr, 3, False, False)
    one = ref.L[0] == 1
    assert one.sum() == 129
    bar, s = K.bar_class_f32(ref)[0][one], ref.S[0][one]
    assert (bar[s > 0] <= 13 * K.U * s[s > 0]).all()


def test_the_long_table():
    nbr, tiles = K.long_table(4)
    assert tiles == 65 and nbr.shape == (27, 128 * 22)
    assert (K.masks(nbr, 3) != 0).all()
    p = K.plan64(nbr, 3, False)
    assert len(p["listed"]) == 66 >= tiles
    for j in range(0, nbr.shape[1], 97):
        e = nbr[:, j][nbr[:, j] >= 0]
        assert len(set(e.tolist())) == len(e)
