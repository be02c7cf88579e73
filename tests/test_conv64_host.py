"""oracle/conv64.py - the float64 reference and the bars tests/test_gpu_conv_float64.py holds the two-pass convolution kernels to -
checked without a device: the bars are neither wrong (a float32 emulation of every stage stays inside them at every element of every
case of the device test) nor empty (ten emulated wrong kernels are each rejected by a check that names the right stage).

The emulation, numpy float32 throughout, every product and every sum rounded to float32 where it is made:
  pass 1, f32     acc = +0; for r ascending: acc = fl(acc + fl(x[r] w[r]))
  pass 1, split   bf16 by round-to-nearest-even on the bit pattern, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); per 32-slice
                  of the reduction the six terms in the order of TS_SPLIT_MMA (al bh, ah bl, am bm, am bh, ah bm, ah bh), each
                  sequential in r
  pass 1, half    halves cast up, the f32 chain, numpy's float16 cast (one rounding to nearest even, subnormals kept)
  pass 2          acc = +0; for k ascending over the live positions: acc = fl(acc + z); half rows: cast up, cast down once
  wgrad           chunks of 128 pairs of the flat list; inside a chunk one chain per offset, sequential in the pair index (split:
                  the six terms per 32 pairs); the partial tiles of an offset added in ascending chunk order onto +0
Each stage receives the emulation's own previous stage, as the device test hands each kernel the device's own."""
import functools

import numpy as np
import pytest

from oracle import conv64 as C

F32 = np.float32


# --------------------------------------------------------------------------------------------------------------- emulation

def bf16(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split3(x):
    x = np.asarray(x, dtype=F32)
    h = bf16(x)
    m = bf16(x - h)
    return h, m, bf16(x - h - m)


SPLIT_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # TS_SPLIT_MMA: (plane of A, plane of B)


def chain(acc, a, b, lo, hi):
    """acc [m, n] += sum_r a[:, r] b[r, :] for r = lo .. hi - 1, one float32 product and one float32 sum per step"""
    for r in range(lo, hi):
        col = a[:, r]
        if col.any():
            acc += col[:, None] * b[r][None, :]
    return acc


def product(a, b, split, drop=(), skip_slices=()):
    """float32 [m, n] = a [m, R] @ b [R, n] in the stated order; drop: terms of SPLIT_ORDER left out; skip_slices: 32-slices left out"""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=F32)
    red = a.shape[1]
    if not split:
        for s0 in range(0, red, 32):
            if s0 // 32 not in skip_slices:
                chain(acc, a, b, s0, min(s0 + 32, red))
        return acc
    pa, pb = split3(a), split3(b)
    for s0 in range(0, red, 32):
        if s0 // 32 in skip_slices:
            continue
        for i, j in SPLIT_ORDER:
            if (i, j) not in drop:
                chain(acc, pa[i], pb[j], s0, min(s0 + 32, red))
    return acc


def emu_pass1(x, w, nbmaps, nboffs, gather_col, transposed, split=False, half=False, mutant=None):
    """x, w float32 (half: the halves cast up).  Returns float32 [P, c_out], or float16 when half."""
    k_vol = len(nboffs) - 1
    c_out = w.shape[1] if transposed else w.shape[2]
    z = np.zeros((int(nboffs[-1]), c_out), dtype=F32)
    drop = {"no_am_bm": ((1, 1),), "no_cross": ((1, 0),)}.get(mutant, ())
    skip = (1,) if mutant == "skip_middle_slice" and x.shape[1] == 96 else ()
    for k in range(k_vol):
        lo, hi = int(nboffs[k]), int(nboffs[k + 1])
        if hi > lo:
            kw = min(k + 1, k_vol - 1) if mutant == "next_weight" else k
            wk = w[kw].T if transposed else w[kw]
            z[lo:hi] = product(x[nbmaps[lo:hi, gather_col]], wk, split, drop, skip)
            if mutant == "drop_row_128":
                z[lo + 127:hi:128] = 0
    if not half:
        return z
    if mutant == "round_twice":
        z = bf16(z)
    zh = z.astype(np.float16)
    if mutant == "flush_subnormals":
        zh[np.abs(zh.astype(F32)) < 2.0 ** -14] = 0
    return zh


def emu_pass2(z, pos, half=False, mutant=None):
    zf = z.astype(F32)
    k_vol, n = pos.shape
    acc = np.zeros((n, z.shape[1]), dtype=F32)
    last = np.full(n, -1)
    for k in range(k_vol):
        last = np.where(pos[k] >= 0, k, last)
    for k in range(k_vol):
        live = pos[k] >= 0
        if mutant == "skip_last_live":
            live = live & (last != k)
        acc[live] = acc[live] + zf[pos[k][live]]
    with np.errstate(over="ignore"):                      # half_large: a sum of 65520 or more is inf, as on the device
        return acc.astype(np.float16) if half else acc


def emu_wgrad(a, b, nbmaps, nboffs, col_a, split=False, mutant=None, prefill=7.0, chunk=128):
    k_vol, p = len(nboffs) - 1, int(nboffs[-1])
    dw = np.full((k_vol, a.shape[1], b.shape[1]), prefill, dtype=F32)
    for k in range(k_vol):
        if nboffs[k + 1] > nboffs[k] or mutant != "empty_unwritten":
            dw[k] = 0
    drop = {"no_am_bm": ((1, 1),), "no_cross": ((1, 0),)}.get(mutant, ())
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        carried = None
        for k in range(k_vol):
            lo, hi = max(int(nboffs[k]), c0), min(int(nboffs[k + 1]), c1)
            if hi <= lo:
                continue
            tile = product(np.ascontiguousarray(a[nbmaps[lo:hi, col_a]].T), b[nbmaps[lo:hi, 1 - col_a]], split, drop)
            if carried is not None:
                tile = tile + carried
                carried = None
            if mutant == "no_flush" and hi < c1 and hi == int(nboffs[k + 1]):
                carried = tile                      # the chunk goes on into the next offset with its accumulators as they are
                continue
            dw[k] = dw[k] + tile
        if carried is not None:
            dw[k_vol - 1] = dw[k_vol - 1] + carried
    return dw


# ------------------------------------------------------------------------------------------------------------------ a case

@functools.lru_cache(maxsize=None)
def book(name):
    return C.rulebook(name)


def f64(a):
    return np.asarray(a).astype(np.float64)


def run_case(ck, case, kinds=("f32", "split", "half"), mutant=None, fams=None, wgrad=True, dgrad=True):
    """every stage of the emulation against the reference, with the checks of the device test; mutant: the wrong kernel emulated in
    the stage it belongs to"""
    name, (c_red, c_out) = case
    nbmaps, nboffs, pos_out, pos_in, n = book(name)
    k_vol = len(nboffs) - 1
    for kind in kinds:
        half, split = kind == "half", kind == "split"
        if (half or split) and not C.is_half_shape(c_red, c_out):
            continue                                    # the guarded shapes reach the f32 kernels only
        for fam in fams or C.families(c_red, half):
            tag = f"{kind} {fam}"
            cast = (lambda t: C.to_half(t).astype(F32)) if half else (lambda t: t)
            for gcol, transposed, pos in ((0, False, pos_out), (1, True, pos_in)) if dgrad else ((0, False, pos_out),):
                x = cast(C.features(fam, n, c_red, "x", half))
                w = cast(C.weights(fam, k_vol, c_red, c_out, "w", transposed, half))
                z64, s, cnt = C.pair_gemm64(f64(x), f64(w), nbmaps, nboffs, gcol, transposed)
                z = emu_pass1(x, w, nbmaps, nboffs, gcol, transposed, split, half, mutant)
                what = f"{tag} gather_col={gcol}"
                if half:
                    assert np.abs(z64).max(initial=0.0) < C.HALF_MAX
                    C.check_half(ck, "pass1_half", what, z, z64, C.bar_pass1_half(z64, s, cnt))
                elif split:
                    C.check_close(ck, "pass1_split", what, z, z64, C.bar_pass1_split(s, cnt))
                else:
                    C.check_close(ck, "pass1_f32", what, z, z64, C.bar_pass1_f32(s, cnt))
                if split:
                    continue                            # pass 2 has no split form
                y = emu_pass2(z, pos, half, mutant)
                bits = (lambda t: t.view(np.int16)) if half else (lambda t: t.view(np.int32))
                C.check_pass2(ck, "pass2_half" if half else "pass2", what, bits(y), y, bits(z), f64(z), pos, half)
            if not wgrad:
                continue
            a, b = cast(C.features(fam, n, c_red, "a", half)), cast(C.second_operand(fam, n, c_out, "b", half))
            dw64, s, cnt, n_k = C.wgrad64(f64(a), f64(b), nbmaps, nboffs, 0)
            dw = emu_wgrad(a, b, nbmaps, nboffs, 0, split, mutant)
            stage = "wgrad_" + kind
            empty = n_k == 0
            ck.true(stage, f"{tag}: an empty offset is not +0 everywhere", bool((dw[empty].view(np.int32) == 0).all()))
            C.check_close(ck, stage, tag, dw[~empty], dw64[~empty], C.bar_wgrad(s, cnt, n_k, 6 if split else 1)[~empty])


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_the_emulation_stays_inside_every_bar(case):
    ck = C.Checks(C.case_id(case), "conv_float64 emulation")
    run_case(ck, case)
    ck.done()
    assert all(v <= 1.0 for v in ck.ratios.values())


# ----------------------------------------------------------------------------------------------------------------- mutants

MUTANTS = [   # (wrong kernel, the stage whose check must miss, kernel family, a case that shows it, operand families)
    ("no_am_bm", "pass1_split", "split", ("EDGE", (32, 32)), ("one_hot",)),
    ("no_am_bm", "wgrad_split", "split", ("TINY27", (32, 32)), ("one_hot",)),
    ("no_cross", "pass1_split", "split", ("EDGE", (96, 128)), ("dense",)),
    ("no_cross", "wgrad_split", "split", ("ONE", (32, 32)), ("one_hot",)),
    ("drop_row_128", "pass1_f32", "f32", ("EDGE", (32, 32)), ("dense",)),
    ("next_weight", "pass1_f32", "f32", ("K8", (48, 24)), ("dense",)),
    ("skip_middle_slice", "pass1_f32", "f32", ("EDGE", (96, 20)), ("one_hot",)),
    ("skip_middle_slice", "pass1_half", "half", ("CENTRE", (96, 128)), ("dense",)),
    ("round_twice", "pass1_half", "half", ("EDGE", (32, 32)), ("dense",)),
    ("flush_subnormals", "pass1_half", "half", ("EDGE", (32, 32)), ("half_small",)),
    ("skip_last_live", "pass2", "f32", ("EDGE", (32, 32)), ("dense",)),
    ("skip_last_live", "pass2_half", "half", ("K8", (32, 32)), ("dense",)),
    ("no_flush", "wgrad_f32", "f32", ("TINY27", (32, 32)), ("dense",)),
    ("no_flush", "wgrad_f32", "f32", ("EDGE", (48, 24)), ("one_hot",)),
    ("empty_unwritten", "wgrad_f32", "f32", ("EDGE", (32, 32)), ("dense",)),
    ("empty_unwritten", "wgrad_half", "half", ("ONE", (32, 32)), ("one_hot",)),
]


@pytest.mark.parametrize("mutant,stage,kind,case,fams", MUTANTS, ids=[f"{m[0]}-{m[1]}-{C.case_id(m[3])}" for m in MUTANTS])
def test_a_wrong_kernel_is_rejected_by_its_stage(mutant, stage, kind, case, fams):
    ck = C.Checks(f"{mutant} {C.case_id(case)}", "conv_float64 mutant")
    run_case(ck, case, kinds=(kind,), mutant=mutant, fams=fams)
    print("\n".join(ck.lines()) + f"\n  first: {ck.missed[0] if ck.missed else None}")
    assert ck.missed, f"{mutant} passed every check of {C.case_id(case)}"
    assert any(m.startswith(stage + " ") for m in ck.missed), f"{mutant}: no check of {stage} missed: {ck.missed[:5]}"
    sound = C.Checks("sound")
    run_case(sound, case, kinds=(kind,), fams=fams)
    assert not sound.missed                              # the same case without the mutation passes


def test_the_two_hot_family_sees_a_dropped_last_slice():
    """what two_hot is for: entries in the first and the last 32-slice of a 96-wide reduction"""
    x = C.features("two_hot", 64, 96, "x")
    assert ((x != 0).sum(1) == 2).all() and (x[:, :32] != 0).any(1).all() and (x[:, 64:] != 0).any(1).all() and not x[:, 32:64].any()


# ----------------------------------------------------------------------------------------------------------------- helpers

def test_round_half_is_numpys_float16():
    rs = np.random.RandomState(5)
    v = rs.randn(200000) * np.ldexp(1.0, rs.randint(-30, 18, size=200000))
    halves = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)          # every finite half, and the midpoints
    mid = (halves[1:] + halves[:-1]) / 2
    edge = np.array([0.0, -0.0, 65504.0, 65519.999, 65520.0, 65536.0, 1e9, np.inf, 2.0 ** -25, np.nextafter(2.0 ** -25, 1.0), 2.0 ** -26])
    for part in (v, halves, mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf), edge):
        for sign in (1.0, -1.0):
            with np.errstate(over="ignore"):
                want = (sign * part).astype(np.float16)
            got = C.round_half(sign * part)
            assert np.array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))
            assert np.array_equal(got, want.astype(np.float64))
    assert np.isnan(C.round_half(np.array([np.nan]))).all()


@pytest.mark.parametrize("name", list(C.COUNTS))
def test_make_rulebook_against_brute_force(name):
    counts, n = C.COUNTS[name]
    nbmaps, nboffs, pos_out, pos_in, _ = book(name)
    assert len(nboffs) == len(counts) + 1 and nbmaps.shape == (sum(counts), 2)
    p = 0
    want_out, want_in = np.full((len(counts), n), -1), np.full((len(counts), n), -1)
    for k, c in enumerate(counts):
        assert nboffs[k] == p
        seg = nbmaps[p:p + c]
        assert len(set(seg[:, 0].tolist())) == c and all(0 <= v < n for v in seg.reshape(-1).tolist())
        assert all(seg[i, 1] < seg[i + 1, 1] for i in range(c - 1)), "output rows ascending and distinct"
        for i in range(c):
            want_in[k, seg[i, 0]] = p + i
            want_out[k, seg[i, 1]] = p + i
        p += c
    assert nboffs[-1] == p and np.array_equal(pos_out, want_out) and np.array_equal(pos_in, want_in)
    with pytest.raises(AssertionError):
        C.make_rulebook([n + 1], n, n, 0)
    if p:
        bad = nbmaps.copy()
        bad[0, 0] = n
        with pytest.raises(AssertionError):
            C.check_rulebook(bad, nboffs, pos_out, pos_in, n, n)
        bad_pos = pos_out.copy()
        bad_pos[bad_pos >= 0] = p
        with pytest.raises(AssertionError):
            C.check_rulebook(nbmaps, nboffs, bad_pos, pos_in, n, n)


def test_the_count_vectors_are_the_ones_asked_for():
    tiny, _ = C.COUNTS["TINY27"]
    assert len(tiny) == 27 and max(tiny) <= 3 and sum(tiny) <= 60 and sum(1 for c in tiny if c) > 20
    assert C.EDGE[:5] == [0, 1, 127, 128, 129] and len(C.EDGE) == 27 and max(C.EDGE) == 385
    for name in ("EDGE", "TINY27"):                        # the NaN checks need a row that three offsets pair, on either side
        nbmaps = book(name)[0]
        assert np.bincount(nbmaps[:, 0]).max() >= 3 and np.bincount(nbmaps[:, 1]).max() >= 3


def test_stage_functions_against_loops():
    nbmaps, nboffs, pos_out, pos_in, n = book("TINY27")
    rs = np.random.RandomState(2)
    x, w = rs.randn(n, 5), rs.randn(27, 5, 3)
    x[3] = 0
    z, s, cnt = C.pair_gemm64(x, w, nbmaps, nboffs, 0, False)
    zt = C.pair_gemm64(x, np.ascontiguousarray(w.transpose(0, 2, 1)), nbmaps, nboffs, 0, True)[0]
    assert np.allclose(z, zt, rtol=0, atol=1e-13)
    k_of = np.repeat(np.arange(27), np.diff(nboffs))
    for p in range(len(nbmaps)):
        for o in range(3):
            terms = [x[nbmaps[p, 0], r] * w[k_of[p], r, o] for r in range(5)]
            assert abs(z[p, o] - sum(terms)) < 1e-13 and abs(s[p, o] - sum(abs(t) for t in terms)) < 1e-13
            assert cnt[p, o] == sum(1 for t in terms if t != 0)
    y, a, live = C.gather_sum64(z, pos_out)
    for j in range(n):
        ps = [pos_out[k, j] for k in range(27) if pos_out[k, j] >= 0]
        assert live[j] == len(ps) and np.allclose(y[j], sum((z[p] for p in ps), np.zeros(3)), atol=1e-13)
        assert np.allclose(a[j], sum((np.abs(z[p]) for p in ps), np.zeros(3)), atol=1e-13)
    b = rs.randn(n, 4)
    dw, s, cnt, n_k = C.wgrad64(x, b, nbmaps, nboffs, 0)
    want = np.zeros((27, 5, 4))
    for p in range(len(nbmaps)):
        want[k_of[p]] += np.outer(x[nbmaps[p, 0]], b[nbmaps[p, 1]])
    assert np.allclose(dw, want, atol=1e-12) and np.array_equal(n_k, np.diff(nboffs))
    assert np.array_equal(C.wgrad_additions(np.ones((2, 1, 1)), np.array([0, 129]), 6)[:, 0, 0], [7.0, 9.0])
