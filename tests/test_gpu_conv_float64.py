"""The two-pass sparse convolution - ts_conv_pair_gemm, ts_conv_gather_sum, ts_conv_wgrad[_det] and their half-storage and split-bf16
forms - against float64 (oracle/conv64.py) on hand-made rulebooks (-m gpu).

Every element is compared.  Every check of a case is evaluated; the case fails with the list of those that missed and prints one line
of worst error / bar per stage (profiles/conv_float64.txt keeps a run's lines).  Every bar is computed from the inputs and the
float64 reference, never from a kernel's output; oracle/conv64.py derives them, tests/test_conv64_host.py shows on the same cases
that a float32 emulation stays inside them and that ten wrong kernels do not.  Every stage receives the device's own previous stage,
cast up unchanged.

Which kernel a call reaches (csrc/conv_pairs.hip, launch_pair_gemm / launch_wgrad): channel pairs whose two widths are multiples of
32 take the full-tile kernels - split bf16 under conv_impl 0 and 6 (6: 64 x 64 tiles), f32 MFMA under 3 (one workgroup per tile),
4 (persistent), 5 (the default choice of the two) - and the guarded kernel under 2; the other pairs (4 -> 32, 48 -> 24, 32 -> 48,
96 -> 20) and operands off a 16-byte boundary take the guarded f32 kernel under every setting and are held to the f32 bar.
Pre-split weight planes behind ts_conv_planes_hint reach the direct-rows kernel on 128-column tiles under conv_impl 0 and on
96-column tiles under 11.  Pass 2 runs the list form (default) and the K-register form (conv_impl 1 keeps it).

No case hands a kernel an index outside its arrays: conv64.check_rulebook runs on every rulebook before its first launch, every
buffer has the size its entry point documents, n_pairs is nboffs[K]."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import conv64 as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND = 256                                     # guard rows behind Z
BAND_BITS = 0x4B1D4B1D                         # what they hold (a finite float; 0x4B1D is a finite half)
CONTRACT_CASES = [(n, c) for n in C.CONTRACT_COUNTS for c in C.FEW_CHANNELS]


def _L():
    from taseg_amd import _lib as L
    return L, L.load()


def _B():
    from taseg_amd import backend as B
    return B


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)                # a copy: the shared references are read-only


def H(t):
    return t.detach().cpu().numpy()


def f64(a):
    return np.asarray(a).astype(np.float64)


def bits(a):
    return a.view(np.int16) if a.dtype == np.float16 else a.view(np.int32)


@contextlib.contextmanager
def conv_impl(impl):
    L, lib = _L()
    _B().set_conv_impl(impl)
    try:
        yield
    finally:
        _B().set_conv_impl(0)
        lib.ts_conv_planes_hint(None, None, 0, 0, 0)


class Book:
    def __init__(self, name):
        self.nbmaps, self.nboffs, self.pos_out, self.pos_in, self.n = C.rulebook(name)
        assert C.check_rulebook(self.nbmaps, self.nboffs, self.pos_out, self.pos_in, self.n, self.n)      # before any launch
        self.k, self.p = len(self.nboffs) - 1, int(self.nboffs[-1])
        self.d_nbmaps, self.d_nboffs = T(self.nbmaps), T(self.nboffs)
        self.d_pos = {0: T(self.pos_out), 1: T(self.pos_in)}           # by gather_col: the forward product sums into output rows
        self.pos = {0: self.pos_out, 1: self.pos_in}
        self.n_k = np.diff(self.nboffs)


@functools.lru_cache(maxsize=None)
def book(name):
    return Book(name)


@functools.lru_cache(maxsize=16)
def pass1_ref(name, c_red, c_out, fam, gcol, half):
    """(x, w in its stored layout, z64, S, N) - computed once, shared by every variant, never written to"""
    bk = book(name)
    transposed = gcol == 1
    x, w = C.features(fam, bk.n, c_red, "x", half), C.weights(fam, bk.k, c_red, c_out, "w", transposed, half)
    if half:
        x, w = C.to_half(x), C.to_half(w)
    z64, s, cnt = C.pair_gemm64(f64(x), f64(w), bk.nbmaps, bk.nboffs, gcol, transposed)
    if half:
        assert np.abs(z64).max(initial=0.0) < C.HALF_MAX, "the reference of pass 1 stays a finite half"
    for a in (x, w, z64, s, cnt):
        a.setflags(write=False)
    return x, w, z64, s, cnt


@functools.lru_cache(maxsize=16)
def wgrad_ref(name, c_a, c_b, fam, half):
    bk = book(name)
    a, b = C.features(fam, bk.n, c_a, "a", half), C.second_operand(fam, bk.n, c_b, "b", half)
    if half:
        a, b = C.to_half(a), C.to_half(b)
    dw64, s, cnt, n_k = C.wgrad64(f64(a), f64(b), bk.nbmaps, bk.nboffs, 0)
    for t in (a, b, dw64, s, cnt):
        t.setflags(write=False)
    return a, b, dw64, s, cnt, n_k


# ------------------------------------------------------------------------------------------------------------ the launches

def k_pass1(bk, x, w, gcol, impl, planes=None, z=None):
    """ts_conv_pair_gemm; w stored [K, c_red, c_out] (gcol 0) or [K, c_out, c_red] (gcol 1, weight_transposed).  z: a buffer of the
    caller's (through the C ABI), else the wrapper allocates."""
    L, lib = _L()
    transposed = gcol == 1
    with conv_impl(impl):
        if planes is not None:
            lib.ts_conv_planes_hint(L.ptr(w), L.ptr(planes), bk.k, w.shape[1], w.shape[2])
        if z is None:
            return _B().conv_pair_gemm(x, w, bk.d_nbmaps, bk.d_nboffs, bk.p, gcol, weight_transposed=transposed)
        c_red, c_out = (w.shape[2], w.shape[1]) if transposed else (w.shape[1], w.shape[2])
        L.check(lib.ts_conv_pair_gemm(L.ptr(x), x.shape[0], c_red, L.ptr(w), bk.k, int(transposed), L.ptr(bk.d_nbmaps),
                                      L.ptr(bk.d_nboffs), bk.p, gcol, L.ptr(z), c_out, L.stream()), "ts_conv_pair_gemm")
        return z


def k_pass1_half(bk, x, w, gcol, natural, z=None):
    """natural: w [K, c_red, c_out] (ts_conv_pair_gemm_f16_nat), else one row per output column, [K, c_out, c_red]"""
    L, lib = _L()
    if z is None:
        return _B().conv_pair_gemm_f16(x, w, bk.d_nbmaps, bk.d_nboffs, bk.p, gcol, natural=natural)
    c_red, c_out = (w.shape[1], w.shape[2]) if natural else (w.shape[2], w.shape[1])
    fn = lib.ts_conv_pair_gemm_f16_nat if natural else lib.ts_conv_pair_gemm_f16
    L.check(fn(L.ptr(x), x.shape[0], c_red, L.ptr(w), bk.k, L.ptr(bk.d_nbmaps), L.ptr(bk.d_nboffs), bk.p, gcol, L.ptr(z), c_out,
               L.stream()), "ts_conv_pair_gemm_f16")
    return z


def k_pass2(bk, z, gcol, registers, out=None):
    """list form, or the K-register form that conv_impl 1 keeps; half rows by dtype"""
    L, lib = _L()
    B = _B()
    half = z.dtype == torch.float16
    with conv_impl(1 if registers else 0):
        if out is None:
            return (B.conv_gather_sum_f16 if half else B.conv_gather_sum)(z, bk.d_pos[gcol], bk.n)
        fn = lib.ts_conv_gather_sum_f16 if half else lib.ts_conv_gather_sum
        L.check(fn(L.ptr(z), z.shape[1], L.ptr(bk.d_pos[gcol]), bk.k, bk.n, bk.p, L.ptr(out), L.stream()), "ts_conv_gather_sum")
        return out


def k_wgrad(bk, a, b, form, impl=0, out=None):
    """form: "det" (ts_conv_wgrad_det), "atomic" (ts_conv_wgrad), "half" (ts_conv_wgrad_f16_det); col_a = 0"""
    L, lib = _L()
    B = _B()
    with conv_impl(impl):
        if out is None and form != "atomic":
            return (B.conv_wgrad_f16 if form == "half" else B.conv_wgrad)(a, b, bk.d_nbmaps, bk.d_nboffs, bk.k, 0, bk.p)
        if out is None:
            out = torch.empty((bk.k, a.shape[1], b.shape[1]), dtype=torch.float32, device=DEV)
        args = (L.ptr(a), a.shape[1], L.ptr(b), b.shape[1], L.ptr(bk.d_nbmaps), L.ptr(bk.d_nboffs), bk.k, 0, bk.p, L.ptr(out))
        if form == "atomic":
            L.check(lib.ts_conv_wgrad(*args, L.stream()), "ts_conv_wgrad")
        else:
            ws = L.workspace(lib.ts_conv_wgrad_workspace_bytes(bk.p, a.shape[1], b.shape[1], bk.k), a.device)
            fn = lib.ts_conv_wgrad_f16_det if form == "half" else lib.ts_conv_wgrad_det
            L.check(fn(*args, L.ptr(ws), ws.numel(), L.stream()), "ts_conv_wgrad_det")
        return out


# -------------------------------------------------------------------------------------------------------------- the checks

def pass1_kind(impl, c_red, c_out, aligned=True):
    """("pass1_split" | "pass1_f32", bar function) of the kernel the call reaches"""
    split = impl in C.SPLIT_IMPLS + (11,) and C.is_half_shape(c_red, c_out) and aligned
    return ("pass1_split", C.bar_pass1_split) if split else ("pass1_f32", C.bar_pass1_f32)


def check_wgrad(ck, stage, what, got, dw64, s, cnt, n_k, m, poisoned=None):
    """got [K, c_a, c_b] float32 on the host.  Empty offsets exactly +0, the others inside the bar; poisoned: a boolean [K, c_a] of
    the rows that a non-finite operand element reaches - exactly those are non-finite"""
    empty = n_k == 0
    ck.true(stage, f"{what}: an empty offset is not +0 everywhere", bool((bits(got)[empty] == 0).all()))
    bar = C.bar_wgrad(s, cnt, n_k, m)
    keep = np.broadcast_to((~empty)[:, None, None], got.shape).copy()
    if poisoned is not None:
        bad = np.broadcast_to(poisoned[:, :, None], got.shape)
        ck.true(stage, f"{what}: {int((np.isfinite(got) & bad).sum())} elements that the non-finite operand reaches are finite",
                not bool((np.isfinite(got) & bad).any()))
        keep &= ~bad
    C.check_close(ck, stage, what, got, dw64, bar, where=keep)


def wgrad_m(impl, c_a, c_b, aligned=True):
    split = impl in C.SPLIT_IMPLS and C.is_half_shape(c_a, c_b) and aligned
    return ("wgrad_split", 6) if split else ("wgrad_f32", 1)


def has_planes_kernel(c_out):
    """(conv_impl under which the hint is taken) for the 128- and 96-column tiles, else None"""
    bn = 32 if c_out <= 32 else 64 if c_out <= 64 else 96 if c_out % 96 == 0 else 128
    return {128: 0, 96: 11}.get(bn) if c_out % bn == 0 else None


# -------------------------------------------------------------------------------------------------------------- the stages

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_stages(case):
    """pass 1 under every conv_impl (forward product and input gradient), pass 2 in both forms, the weight gradient in its
    deterministic, atomic and half forms - every operand family of the case, each call made twice for its bits"""
    L, lib = _L()
    name, (c_red, c_out) = case
    bk = book(name)
    ck = C.Checks(C.case_id(case))
    for fam in C.families(c_red):
        for gcol in (0, 1):
            x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, gcol, False)
            xd, wd = T(x), T(w)
            tag = f"{fam} gather_col={gcol}"
            z_default = None
            for impl in C.SPLIT_IMPLS + C.F32_IMPLS:
                stage, bar = pass1_kind(impl, c_red, c_out)
                z = k_pass1(bk, xd, wd, gcol, impl)
                ck.true(stage, f"{tag} impl {impl}: shape", tuple(z.shape) == (bk.p, c_out))
                C.check_close(ck, stage, f"{tag} impl {impl}", H(z), z64, bar(s, cnt))
                ck.true(stage, f"{tag} impl {impl}: a second call gives other bits", torch.equal(bits_t(z), bits_t(k_pass1(bk, xd, wd, gcol, impl))))
                z_default = z if impl == 0 else z_default
            hint_impl = has_planes_kernel(c_out) if C.is_half_shape(c_red, c_out) else None
            if hint_impl is not None and bk.p:
                planes = torch.empty(3 * wd.numel(), dtype=torch.int16, device=DEV)
                L.check(lib.ts_conv_split_planes(L.ptr(wd), bk.k, wd.shape[1], wd.shape[2], L.ptr(planes), L.stream()), "ts_conv_split_planes")
                plain = k_pass1(bk, xd, wd, gcol, hint_impl)
                hinted = k_pass1(bk, xd, wd, gcol, hint_impl, planes=planes)
                ck.true("pass1_split", f"{tag}: planes behind the hint change the bits", torch.equal(bits_t(hinted), bits_t(plain)))
                C.check_close(ck, "pass1_split", f"{tag} planes", H(hinted), z64, C.bar_pass1_split(s, cnt))
                junk = torch.zeros_like(planes)                          # that the hinted call did read its planes
                ck.true("pass1_split", f"{tag}: the hinted call did not take the planes",
                        not torch.equal(k_pass1(bk, xd, wd, gcol, hint_impl, planes=junk), plain))
            # pass 2 on the device's own Z
            zh = H(z_default)
            ys = [k_pass2(bk, z_default, gcol, registers) for registers in (False, True)]
            ck.true("pass2", f"{tag}: the list form and the register form differ", torch.equal(bits_t(ys[0]), bits_t(ys[1])))
            for y, form in zip(ys, ("list", "registers")):
                yh = H(y)
                ck.true("pass2", f"{tag} {form}: shape", yh.shape == (bk.n, c_out))
                C.check_pass2(ck, "pass2", f"{tag} {form}", bits(yh), yh, bits(zh), f64(zh), bk.pos[gcol])
            ck.true("pass2", f"{tag}: a second call gives other bits", torch.equal(bits_t(ys[0]), bits_t(k_pass2(bk, z_default, gcol, False))))
        a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, False)
        ad, bd = T(a), T(b)
        for form, impl in (("det", 0), ("det", 2), ("det", 5), ("atomic", 0)):
            stage, m = wgrad_m(impl, c_red, c_out)
            dw = k_wgrad(bk, ad, bd, form, impl)
            check_wgrad(ck, stage, f"{fam} {form} impl {impl}", H(dw), dw64, s, cnt, n_k, m)
            if form == "det":
                ck.true(stage, f"{fam} det impl {impl}: a second call gives other bits", torch.equal(bits_t(dw), bits_t(k_wgrad(bk, ad, bd, form, impl))))
    if C.is_half_shape(c_red, c_out):
        half_stages(ck, name, c_red, c_out)
    ck.done()


def bits_t(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def half_stages(ck, name, c_red, c_out):
    bk = book(name)
    for fam in C.families(c_red, half=True):
        for gcol in (0, 1):
            x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, gcol, True)           # w natural for gather_col 0, rows for 1
            xd = T(x)
            for natural in (True, False):                # both weight layouts in both directions: the same W_k either way
                wd = T(w if natural == (gcol == 0) else w.transpose(0, 2, 1))
                tag = f"half {fam} gather_col={gcol} natural={natural}"
                z = k_pass1_half(bk, xd, wd, gcol, natural)
                zh = H(z)
                ck.true("pass1_half", f"{tag}: shape", zh.shape == (bk.p, c_out))
                C.check_half(ck, "pass1_half", tag, zh, z64, C.bar_pass1_half(z64, s, cnt))
                ck.true("pass1_half", f"{tag}: a second call gives other bits", torch.equal(bits_t(z), bits_t(k_pass1_half(bk, xd, wd, gcol, natural))))
            tag = f"half {fam} gather_col={gcol}"
            ys = [k_pass2(bk, z, gcol, registers) for registers in (False, True)]
            ck.true("pass2_half", f"{tag}: the list form and the register form differ", torch.equal(bits_t(ys[0]), bits_t(ys[1])))
            for y, form in zip(ys, ("list", "registers")):
                yh = H(y)
                C.check_pass2(ck, "pass2_half", f"{tag} {form}", bits(yh), yh, bits(zh), f64(zh), bk.pos[gcol], half=True)
        a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, True)
        ad, bd = T(a), T(b)
        dw = k_wgrad(bk, ad, bd, "half")
        check_wgrad(ck, "wgrad_half", f"half {fam}", H(dw), dw64, s, cnt, n_k, 1)
        ck.true("wgrad_half", f"half {fam}: a second call gives other bits", torch.equal(bits_t(dw), bits_t(k_wgrad(bk, ad, bd, "half"))))


# ----------------------------------------------------------------------------------------------------------- the contracts

def z_buffer(p, c, dtype):
    """[p + BAND, c]: NaN below p, the band pattern behind"""
    z = torch.full((p + BAND, c), float("nan"), dtype=dtype, device=DEV)
    bits_t(z)[p:] = BAND_BITS if dtype == torch.float32 else BAND_BITS & 0xFFFF
    return z


def band_kept(z, p):
    return bool((bits_t(z)[p:] == (BAND_BITS if z.dtype == torch.float32 else BAND_BITS & 0xFFFF)).all())


@pytest.mark.parametrize("case", CONTRACT_CASES, ids=C.case_id)
def test_guard_band_and_overwritten_buffers(case):
    """Z with 256 rows more than P: the band keeps its bits, the rows below P - NaN before the call - are all written; the output
    of pass 2 and dW - NaN and 7.0 before the call - are overwritten: rows without a pair and empty offsets read +0"""
    name, (c_red, c_out) = case
    bk = book(name)
    ck = C.Checks("band " + C.case_id(case))
    fam = "dense"
    for gcol in (0, 1):
        x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, gcol, False)
        xd, wd = T(x), T(w)
        for impl in C.SPLIT_IMPLS + C.F32_IMPLS:
            stage, bar = pass1_kind(impl, c_red, c_out)
            z = k_pass1(bk, xd, wd, gcol, impl, z=z_buffer(bk.p, c_out, torch.float32))
            ck.true(stage, f"gather_col={gcol} impl {impl}: the rows behind n_pairs were written", band_kept(z, bk.p))
            C.check_close(ck, stage, f"gather_col={gcol} impl {impl}", H(z[:bk.p]), z64, bar(s, cnt))
        hint_impl = has_planes_kernel(c_out) if C.is_half_shape(c_red, c_out) else None
        if hint_impl is not None:
            L, lib = _L()
            planes = torch.empty(3 * wd.numel(), dtype=torch.int16, device=DEV)
            L.check(lib.ts_conv_split_planes(L.ptr(wd), bk.k, wd.shape[1], wd.shape[2], L.ptr(planes), L.stream()), "ts_conv_split_planes")
            z = k_pass1(bk, xd, wd, gcol, hint_impl, planes=planes, z=z_buffer(bk.p, c_out, torch.float32))
            ck.true("pass1_split", f"gather_col={gcol} planes: the rows behind n_pairs were written", band_kept(z, bk.p))
            C.check_close(ck, "pass1_split", f"gather_col={gcol} planes", H(z[:bk.p]), z64, C.bar_pass1_split(s, cnt))
        zs = [z[:bk.p]]
        if C.is_half_shape(c_red, c_out):
            xh, wh, z64h, sh, cnth = pass1_ref(name, c_red, c_out, fam, gcol, True)
            z = k_pass1_half(bk, T(xh), T(wh), gcol, gcol == 0, z=z_buffer(bk.p, c_out, torch.float16))
            ck.true("pass1_half", f"gather_col={gcol}: the rows behind n_pairs were written", band_kept(z, bk.p))
            C.check_half(ck, "pass1_half", f"gather_col={gcol}", H(z[:bk.p]), z64h, C.bar_pass1_half(z64h, sh, cnth))
            zs.append(z[:bk.p])
        for z in zs:                                    # pass 2 into a buffer of NaN with a band of its own
            half = z.dtype == torch.float16
            stage = "pass2_half" if half else "pass2"
            for registers in (False, True):
                y = k_pass2(bk, z, gcol, registers, out=z_buffer(bk.n, c_out, z.dtype))
                ck.true(stage, f"gather_col={gcol} registers={registers}: rows behind n_rows were written", band_kept(y, bk.n))
                yh, zh = H(y[:bk.n]), H(z)
                C.check_pass2(ck, stage, f"gather_col={gcol} registers={registers}", bits(yh), yh, bits(zh), f64(zh), bk.pos[gcol], half)
    a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, False)
    ad, bd = T(a), T(b)
    seven = lambda: torch.full((bk.k, c_red, c_out), 7.0, dtype=torch.float32, device=DEV)          # noqa: E731
    for form, impl in (("det", 0), ("det", 2), ("det", 5), ("atomic", 0), ("atomic", 5)):
        stage, m = wgrad_m(impl, c_red, c_out)
        check_wgrad(ck, stage, f"{form} impl {impl} into 7.0", H(k_wgrad(bk, ad, bd, form, impl, out=seven())), dw64, s, cnt, n_k, m)
    if C.is_half_shape(c_red, c_out):
        a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, True)
        check_wgrad(ck, "wgrad_half", "half into 7.0", H(k_wgrad(bk, T(a), T(b), "half", out=seven())), dw64, s, cnt, n_k, 1)
    ck.done()


def shared_row(bk, col):
    """a row that at least three offsets pair on side `col` of the rulebook, and its pairs"""
    counts = np.bincount(bk.nbmaps[:, col], minlength=bk.n)
    row = int(np.argmax(counts))
    assert counts[row] >= 3
    return row, np.nonzero(bk.nbmaps[:, col] == row)[0]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", CONTRACT_CASES, ids=C.case_id)
def test_a_non_finite_element_reaches_exactly_its_outputs(case, value):
    """one element of one feature row that three offsets pair: exactly the Z rows of its pairs, then exactly the output rows they
    feed, are non-finite (the kind is not asserted: the split form turns inf into NaN); every other element is finite and inside
    its bar.  In the weight gradient A[row, ci0] reaches exactly dW[k, ci0, :] of the offsets k that pair the row."""
    name, (c_red, c_out) = case
    bk = book(name)
    ck = C.Checks(f"{'nan' if value != value else 'inf'} " + C.case_id(case))
    fam = "dense"
    ci0 = c_red // 2
    for gcol in (0, 1):
        row, pairs = shared_row(bk, gcol)
        hit_z = np.zeros(bk.p, dtype=bool)
        hit_z[pairs] = True
        hit_y = np.zeros(bk.n, dtype=bool)
        hit_y[bk.nbmaps[pairs, 1 - gcol]] = True
        variants = [(impl, False) for impl in C.SPLIT_IMPLS + C.F32_IMPLS] + ([(None, True)] if C.is_half_shape(c_red, c_out) else [])
        for impl, half in variants:
            x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, gcol, half)
            xd, wd = T(x), T(w)
            xd[row, ci0] = value
            if half:
                stage, z = "pass1_half", k_pass1_half(bk, xd, wd, gcol, gcol == 0)
            else:
                (stage, bar), z = pass1_kind(impl, c_red, c_out), k_pass1(bk, xd, wd, gcol, impl)
            zh = H(z)
            what = f"gather_col={gcol} {'half' if half else f'impl {impl}'}"
            ck.true(stage, f"{what}: {int(np.isfinite(zh[hit_z]).sum())} elements of the Z rows of the row's pairs are finite",
                    not bool(np.isfinite(zh[hit_z]).any()))
            if half:
                C.check_half(ck, stage, what, zh[~hit_z], z64[~hit_z], C.bar_pass1_half(z64, s, cnt)[~hit_z])
            else:
                C.check_close(ck, stage, what, zh[~hit_z], z64[~hit_z], bar(s, cnt)[~hit_z])
            if impl in (None, 0, 5):
                stage2 = "pass2_half" if half else "pass2"
                for registers in (False, True):
                    yh = H(k_pass2(bk, z, gcol, registers))
                    ck.true(stage2, f"{what} registers={registers}: {int(np.isfinite(yh[hit_y]).sum())} elements of the rows fed are finite",
                            not bool(np.isfinite(yh[hit_y]).any()))
                    with np.errstate(invalid="ignore"):
                        C.check_pass2(ck, stage2, f"{what} registers={registers}", bits(yh), yh, bits(zh), f64(zh), bk.pos[gcol], half, where=~hit_y)
    row, pairs = shared_row(bk, 0)
    k_of = np.repeat(np.arange(bk.k), bk.n_k)
    poisoned = np.zeros((bk.k, c_red), dtype=bool)
    poisoned[k_of[pairs], ci0] = True
    forms = [("det", 0, False), ("det", 2, False), ("det", 5, False), ("atomic", 0, False)] + ([("half", 0, True)] if C.is_half_shape(c_red, c_out) else [])
    for form, impl, half in forms:
        a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, half)
        ad, bd = T(a), T(b)
        ad[row, ci0] = value
        stage, m = ("wgrad_half", 1) if half else wgrad_m(impl, c_red, c_out)
        check_wgrad(ck, stage, f"{form} impl {impl}", H(k_wgrad(bk, ad, bd, form, impl)), dw64, s, cnt, n_k, m, poisoned=poisoned)
    ck.done()


def off_boundary(a, elements):
    """the same values, contiguous, starting `elements` elements into a flat buffer: 4 bytes off a 16-byte boundary"""
    flat = torch.zeros(a.size + 8, dtype=torch.float16 if a.dtype == np.float16 else torch.float32, device=DEV)
    view = flat[elements:elements + a.size].view(a.shape)
    view.copy_(T(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("case", CONTRACT_CASES, ids=C.case_id)
def test_operands_off_a_16_byte_boundary(case):
    """features that start 4 bytes off a 16-byte boundary: the fp32 entry points take their guarded kernels and meet the f32 bars,
    the half entry points refuse the call"""
    L, lib = _L()
    name, (c_red, c_out) = case
    bk = book(name)
    ck = C.Checks("misaligned " + C.case_id(case))
    fam = "dense"
    for gcol in (0, 1):
        x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, gcol, False)
        z = k_pass1(bk, off_boundary(x, 1), T(w), gcol, 0)
        C.check_close(ck, "pass1_f32", f"gather_col={gcol} x off the boundary", H(z), z64, C.bar_pass1_f32(s, cnt))
        zo = off_boundary(H(z), 1)
        yh, zh = H(k_pass2(bk, zo, gcol, False)), H(z)
        C.check_pass2(ck, "pass2", f"gather_col={gcol} z off the boundary", bits(yh), yh, bits(zh), f64(zh), bk.pos[gcol])
    a, b, dw64, s, cnt, n_k = wgrad_ref(name, c_red, c_out, fam, False)
    for form in ("det", "atomic"):
        check_wgrad(ck, "wgrad_f32", f"{form}, a off the boundary", H(k_wgrad(bk, off_boundary(a, 1), T(b), form)), dw64, s, cnt, n_k, 1)
        check_wgrad(ck, "wgrad_f32", f"{form}, b off the boundary", H(k_wgrad(bk, T(a), off_boundary(b, 1), form)), dw64, s, cnt, n_k, 1)
    if C.is_half_shape(c_red, c_out):
        x, w, z64, s, cnt = pass1_ref(name, c_red, c_out, fam, 0, True)
        for what, call in (("ts_conv_pair_gemm_f16_nat", lambda: k_pass1_half(bk, off_boundary(x, 2), T(w), 0, True)),
                           ("ts_conv_pair_gemm_f16", lambda: k_pass1_half(bk, off_boundary(x, 2), T(w.transpose(0, 2, 1)), 0, False)),
                           ("ts_conv_gather_sum_f16", lambda: k_pass2(bk, off_boundary(np.zeros((bk.p, c_out), np.float16), 2), 0, False)),
                           ("ts_conv_wgrad_f16_det", lambda: k_wgrad(bk, off_boundary(x, 2), T(C.to_half(C.second_operand(fam, bk.n, c_out, "b", True))), "half"))):
            with pytest.raises(L.BackendError, match="16-byte aligned"):
                call()
            ck.true("half", f"{what} refused the call", True)
    ck.done()
