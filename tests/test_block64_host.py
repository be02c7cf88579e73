"""oracle/block64.py - the float64 reference of the fused conv-block calls and the bars tests/test_gpu_block_float64.py holds them to -
checked without a device: the reference against autograd in double on every rulebook of the device test, a float32 / half emulation
of every call inside every bar of every case, and twelve emulated wrong calls each rejected by a bar or an exact check.

The emulation, numpy float32 throughout, follows the kernels' order:
  products   per offset (conv_pairs*.hip) or per group of a class plan (conv_class.hip): per 32-slice of the reduction one float32
             matrix product per term - fp32 split kernels: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) of both operands and the
             six products al bh, ah bl, am bm, am bh, ah bm, ah bh; half: the halves cast up, one product; Z (Z' per group) rounded to
             half where it is stored
  pass 2     acc = +0; offsets (groups) ascending: acc = fl(acc + z); then the addend; half rows cast down once.  The finish inside
             the product adds the same rows in the same order
  wgrad      partial tiles per chunk of 128 pairs of the flat list, flushed at offset boundaries into slot (chunk + offset); the
             ordered sum adds an offset's slots in ascending chunk onto +0
  BatchNorm  the slice layout oracle/bn64.py documents: slices of `rows` rows, a lane adds its rows of the slice in float32, the rpp
             lanes of a channel are added in float32, the slices in float64; the statistics converted to float32; the elementwise
             passes in float32, one rounding to the storage type; the mask bit from the STORED value
Every stage receives the emulation's own previous stage, as the device test hands each stage the device's own."""
import numpy as np
import pytest
import torch

from oracle import block64 as B
from oracle import class64 as K
from oracle import conv64 as C

F32 = np.float32
SPLIT_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # TS_SPLIT_MMA / CG_MMA: (plane of A, plane of B)
CHUNK = 128                                                           # ts_wgrad_plan's chunk at these pair counts (its minimum)


def bf16(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split3(x):
    x = np.asarray(x, dtype=F32)
    h = bf16(x)
    m = bf16(x - h)
    return h, m, bf16(x - h - m)


def product(a, b, split):
    """float32 [m, n] = a [m, R] @ b [R, n]: per 32-slice one float32 matrix product per term, added in the kernels' order"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=F32)
    if not a.shape[0]:
        return acc
    pa, pb = (split3(a), split3(b)) if split else ((a,), (b,))
    for s0 in range(0, a.shape[1], 32):
        for i, j in (SPLIT_ORDER if split else ((0, 0),)):
            acc = acc + pa[i][:, s0:s0 + 32] @ pb[j][s0:s0 + 32]
    return acc


def store(v, half):
    with np.errstate(over="ignore"):
        return v.astype(np.float16) if half else v.astype(F32)


# --------------------------------------------------------------------------------------------------------------- emulation

def emu_conv(x, w, bk, gather_col, pos, wt, half, split, addend=None, swap_col=False, rounded=True):
    """pair GEMM + pass 2 (and the natural form, whose one pair per row passes through pass 2 unchanged)"""
    xf, wf = x.astype(F32), w.astype(F32)
    c = w.shape[1] if wt else w.shape[2]
    z = np.zeros((bk.p, c), dtype=F32)
    col = 1 - gather_col if swap_col else gather_col
    for k in range(bk.k):
        lo, hi = int(bk.nboffs[k]), int(bk.nboffs[k + 1])
        z[lo:hi] = product(xf[bk.nbmaps[lo:hi, col]], wf[k].T if wt else wf[k], split)
    z = store(z, half).astype(F32)
    acc = np.zeros((pos.shape[1], c), dtype=F32)
    for k in range(pos.shape[0]):
        live = pos[k] >= 0
        acc[live] = acc[live] + z[pos[k][live]]
    if addend is not None:
        acc = acc + addend.astype(F32)
    return store(acc, half) if rounded else acc


def emu_class(x, w, nbr, groups, wt, mirror, half, addend=None, rounded=True):
    """the product on a class plan of the table nbr [K, n] (pass-2 plans: groups = 3, Z' stored per group, then pass 2 or the finish,
    the same additions; direct plans: groups = 1, the sums are the result)"""
    xf, wf = x.astype(F32), w.astype(F32)
    kvol, n = nbr.shape
    gk = kvol // groups
    c = w.shape[1] if wt else w.shape[2]
    zg = np.zeros((groups, n, c), dtype=F32)
    has = np.zeros((groups, n), dtype=bool)
    for g in range(groups):
        tot = np.zeros((n, c), dtype=F32)
        for kl in range(gk):
            k = gk * g + kl
            src = nbr[k]
            if not (src >= 0).any():
                continue
            kw = kvol - 1 - k if mirror else k
            a = np.where((src >= 0)[:, None], xf[np.maximum(src, 0)], F32(0))
            tot = tot + product(a, wf[kw].T if wt else wf[kw], not half)      # half: one accumulator set; fp32: tot += acc
            has[g] |= src >= 0
        zg[g] = tot
    if groups == 1:
        return store(zg[0], half)
    zg = store(zg, half).astype(F32)
    acc = np.zeros((n, c), dtype=F32)
    for g in range(groups):
        acc[has[g]] = acc[has[g]] + zg[g][has[g]]
    if addend is not None:
        acc = acc + addend.astype(F32)
    return store(acc, half) if rounded else acc


def emu_wgrad(a, b, bk, col_a, split, prefill, mutant=None):
    af, bf = a.astype(F32), b.astype(F32)
    part = {}
    for c0 in range(0, bk.p, CHUNK):
        c1, ci = min(bk.p, c0 + CHUNK), c0 // CHUNK
        first = None
        for k in range(bk.k):
            lo, hi = max(int(bk.nboffs[k]), c0), min(int(bk.nboffs[k + 1]), c1)
            if hi <= lo:
                continue
            tile = product(np.ascontiguousarray(af[bk.nbmaps[lo:hi, col_a]].T), bf[bk.nbmaps[lo:hi, 1 - col_a]], split)
            if mutant == "straddle_to_first" and first is not None:
                part[(ci, first)] = part[(ci, first)] + tile                 # no flush at the boundary: the first offset takes it all
                continue
            first = k if first is None else first
            part[(ci, k)] = tile
    dw = np.full((bk.k, a.shape[1], b.shape[1]), prefill, dtype=F32)
    for k in range(bk.k):
        lo, hi = int(bk.nboffs[k]), int(bk.nboffs[k + 1])
        if hi <= lo:
            if mutant != "empty_keeps_contents":
                dw[k] = 0
            continue
        acc = np.zeros(dw.shape[1:], dtype=F32)
        chunks = range(lo // CHUNK, (hi - 1) // CHUNK + 1)
        for ci in chunks:
            if mutant == "last_chunk_left_out" and len(chunks) > 1 and ci == chunks[-1]:
                continue
            acc = acc + part.get((ci, k), F32(0))
        dw[k] = acc
    return dw


def sliced_sums(v, half):
    """float64 [c]: the column sums of float32 v [n, c] in the slice layout of bn.hip"""
    n, c = v.shape
    rpp = 256 // (c // (8 if half else 4))
    rows = -(-max(-(-n // 512), 32) // rpp) * rpp
    total = np.zeros(c, dtype=np.float64)
    for s0 in range(0, n, rows):
        sl = v[s0:s0 + rows]
        sl = np.concatenate([sl, np.zeros((-len(sl) % rpp, c), dtype=F32)]).reshape(-1, rpp, c)
        lanes = np.zeros((rpp, c), dtype=F32)
        for i in range(sl.shape[0]):
            lanes = lanes + sl[i]
        acc = np.zeros(c, dtype=F32)
        for r in range(rpp):
            acc = acc + lanes[r]
        total += acc
    return total


def emu_bn_forward(x, res, w, b, rm0, rv0, relu, half, mutant=None):
    xf = x.astype(F32)
    n = len(xf)
    m64, e2 = sliced_sums(xf, half) / n, sliced_sums(xf * xf, half) / n
    var = np.maximum(e2 - m64 * m64, 0.0)
    mean, invstd = m64.astype(F32), (1.0 / np.sqrt(var + B.EPS)).astype(F32)
    if mutant == "residual_before_affine" and res is not None:
        v = (xf + res.astype(F32) - mean) * invstd * w + b
    else:
        v = (xf - mean) * invstd * w + b
        if res is not None:
            v = v + res.astype(F32)
    if relu:
        v = np.maximum(v, F32(0))
    out = store(v, half)
    mask = B.pack_mask(v if mutant == "mask_from_fp32" else out, half) if relu else None
    unbiased = 1.0 if (n == 1 or mutant == "biased_running_var") else n / (n - 1.0)
    mom = B.MOMENTUM
    rm = ((1.0 - mom) * rm0.astype(np.float64) + mom * m64).astype(F32)
    rv = ((1.0 - mom) * rv0.astype(np.float64) + mom * var * unbiased).astype(F32)
    return out, mean, invstd, mask, rm, rv


def unpack_mask(mask, n, c, half):
    ve = 8 if half else 4
    return ((mask.reshape(n, c // ve, 1) >> np.arange(ve)) & 1).reshape(n, c).astype(bool)


def emu_bn_backward(gy, mask, x, mean, invstd, w, half, want_res):
    g = gy.astype(F32)
    n, c = g.shape
    if mask is not None:
        g = np.where(unpack_mask(mask, n, c, half), g, F32(0))
    xc = x.astype(F32) - mean
    sg, sgx = sliced_sums(g, half), sliced_sums(g * xc, half)
    gb, gw = sg.astype(F32), (sgx * invstd.astype(np.float64)).astype(F32)
    c1 = (sg / n).astype(F32)
    c2 = (sgx / n * invstd.astype(np.float64) ** 2).astype(F32)
    gx = (g - c1 - xc * c2) * (invstd * w)
    return store(gx, half), (store(g, half) if want_res else None), gw, gb


class Emu:
    """the calls of a case in float32; mutant: the wrong call it emulates"""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def conv(self, cs, ops, w, x, direction, addend=None, rounded=True):
        bk = B.book(cs["book"])
        sd = bk.sides(cs["transposed"])
        half, mut = cs["half"], self.mutant
        fwd = direction == "forward"
        route = cs["route_f"] if fwd else cs["route_d"]
        c_red, c_out = (cs["c_in"], cs["c_out"]) if fwd else (cs["c_out"], cs["c_in"])
        split = B.split_kernel(route, c_red, c_out, half, cs["impl"])
        if mut == "addend_dropped":
            addend = None
        if mut == "addend_twice" and addend is not None:
            addend = store(addend.astype(F32) * F32(2), half)
        if route in ("pairs", "natural"):
            gcol, pos = (sd["gather_col"], sd["pos"]) if fwd else (sd["dgrad_gather_col"], sd["pos_dgrad"])
            return emu_conv(x, w, bk, gcol, pos, not fwd, half, split, addend, swap_col=(mut == "dgrad_col_swapped" and not fwd), rounded=rounded)
        if route == "direct":
            return emu_class(x, w, sd["nbr_f"] if fwd else sd["nbr_d"], 1, not fwd, False, half)
        # a submanifold map: ONE plan, of the table itself; the input gradient takes the mirrored slice
        return emu_class(x, w, bk.nbr, 3, not fwd, (not fwd) and mut != "mirror_ignored", half, addend, rounded)

    def train(self, cs, ops, prefill=np.nan):
        bk = B.book(cs["book"])
        sd = bk.sides(cs["transposed"])
        half, mut = cs["half"], self.mutant
        got = {}
        w = ops["w16"] if half else ops["kernel"]
        if half:
            got["w16"] = w
        got["conv_out"] = self.conv(cs, ops, w, ops["feat"], "forward")
        (got["out"], got["mean"], got["invstd"], got["mask"], got["running_mean"], got["running_var"]) = emu_bn_forward(
            got["conv_out"], ops["residual"], ops["bn_w"], ops["bn_b"], ops["rm0"], ops["rv0"], cs["relu"], half, mut)
        got["nbt"] = np.int64(1)
        got["grad_conv"], got["grad_residual"], got["grad_bn_weight"], got["grad_bn_bias"] = emu_bn_backward(
            ops["grad_out"], got["mask"], got["conv_out"], got["mean"], got["invstd"], ops["bn_w"], half, cs["residual"])
        if cs["addend"]:
            ops["addend"] = B.make_addend(cs, ops, got["grad_conv"])
        col_a = 1 - sd["wgrad_col_a"] if mut == "wgrad_col_a_swapped" else sd["wgrad_col_a"]
        split = not half and cs["impl"] == 0 and C.is_half_shape(cs["c_in"], cs["c_out"])
        got["grad_kernel"] = emu_wgrad(ops["feat"], got["grad_conv"], bk, col_a, split, prefill, mut)
        got["grad_feat"] = self.conv(cs, ops, w, got["grad_conv"], "backward", addend=ops["addend"]) if cs["grad_feat"] else None
        return got

    def eval(self, cs, ops):
        half = cs["half"]
        w = ops["w16"] if half else ops["kernel"]
        got = {"conv_out": self.conv(cs, ops, w, ops["feat"], "forward")}
        s = self.conv(cs, ops, w, ops["feat"], "forward", rounded=False) if cs["tail"] and cs["route_f"] != "direct" else got["conv_out"]
        if self.mutant == "tail_on_rounded_sum":
            s = got["conv_out"]
        with np.errstate(over="ignore", invalid="ignore"):
            v = (s.astype(F32) - ops["mean"]) * ops["invstd"] * ops["bn_w"] + ops["bn_b"]
            if ops["residual"] is not None:
                v = v + ops["residual"].astype(F32)
            got["out"] = store(np.maximum(v, F32(0)) if cs["relu"] else v, half)
        return got


def run_training(cs, mutant=None, prefill=np.nan):
    ck = C.Checks(B.case_id(cs), "block_float64 emulation" if mutant is None else f"block_float64 {mutant}")
    ops = B.operands(cs)
    B.check_training(ck, cs, ops, Emu(mutant).train(cs, ops, prefill))
    return ck


def run_eval(cs, mutant=None):
    ck = C.Checks(B.eval_id(cs), "block_float64 emulation" if mutant is None else f"block_float64 {mutant}")
    ops = B.operands(cs)
    ops["mean"], ops["invstd"] = B.eval_statistics(cs, ops)
    B.check_eval(ck, cs, ops, Emu(mutant).eval(cs, ops))
    return ck


TRAINING = B.TWO_PASS + B.ADDEND + B.PLANS + B.REFUSED_PLANS + B.NATURAL


@pytest.mark.parametrize("cs", TRAINING, ids=B.case_id)
def test_the_emulation_stays_inside_every_bar(cs):
    for prefill in (np.nan, 7.0):
        ck = run_training(cs, prefill=prefill)
        ck.done()
        assert all(v <= 1.0 for v in ck.ratios.values())


@pytest.mark.parametrize("cs", B.EVAL, ids=B.eval_id)
def test_the_evaluation_emulation_stays_inside_every_bar(cs):
    ck = run_eval(cs)
    ck.done()
    assert all(v <= 1.0 for v in ck.ratios.values())


# ----------------------------------------------------------------------------------------------------------------- mutants

def _find(cases, **kw):
    for cs in cases:
        if all(cs[k] == v for k, v in kw.items()):
            return cs
    raise KeyError(kw)


MUTANTS = [   # (the wrong call, the stage whose check must miss, a case of the device test that shows it)
    ("addend_dropped", "grad_feat", _find(B.ADDEND, book="EDGE", half=False)),
    ("addend_twice", "grad_feat", _find(B.ADDEND, book="SUB129", half=True, route_d="finish")),
    ("mirror_ignored", "grad_feat", _find(B.PLANS, book="SUB129", half=False, route_d="class")),
    ("wgrad_col_a_swapped", "grad_kernel", _find(B.TWO_PASS, book="EDGE", c_in=96, half=False, grad_feat=True)),
    ("dgrad_col_swapped", "grad_feat", _find(B.TWO_PASS, book="K8", c_in=96, half=True)),
    ("last_chunk_left_out", "grad_kernel", _find(B.TWO_PASS, book="EDGE", c_in=32, half=False, residual=True, gk_off=False)),
    ("straddle_to_first", "grad_kernel", _find(B.TWO_PASS, book="EDGE", c_in=48)),
    ("empty_keeps_contents", "grad_kernel", _find(B.TWO_PASS, book="EDGE", c_in=32, half=True, residual=True, gk_off=False)),
    ("mask_from_fp32", "forward", _find(B.TWO_PASS, book="TINY27", half=True)),
    ("biased_running_var", "forward", _find(B.TWO_PASS, book="EDGE", c_in=96, half=False, grad_feat=True)),
    ("residual_before_affine", "forward", _find(B.PLANS, book="D128", half=False, transposed=False)),
]


@pytest.mark.parametrize("mutant,stage,cs", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_wrong_call_is_rejected(mutant, stage, cs):
    ck = run_training(cs, mutant)
    print("\n".join(ck.lines()) + f"\n  first: {ck.missed[0] if ck.missed else None}")
    assert ck.missed, f"{mutant} passed every check of {B.case_id(cs)}"
    assert any(m.startswith(stage) for m in ck.missed), f"{mutant}: no check of {stage} missed: {ck.missed[:5]}"
    assert not run_training(cs).missed                    # the same case without the mutation passes


def test_a_tail_on_the_rounded_sum_is_rejected():
    """half storage, sums of 65520 and more (half_large): rounded to half before the tail they are infinities; the riding tail keeps
    the float32 sum and its result is finite"""
    cs = _find(B.EVAL, family="half_large")
    ck = run_eval(cs, "tail_on_rounded_sum")
    print("\n".join(ck.lines()) + f"\n  first: {ck.missed[0] if ck.missed else None}")
    assert any(m.startswith("eval_tail") for m in ck.missed)
    assert not run_eval(cs).missed
    ops = B.operands(cs)
    bk = B.book(cs["book"])
    sd = bk.sides(cs["transposed"])
    y = B.conv_ref(B.f64(ops["feat"]), B.f64(ops["w16"]), bk, sd["gather_col"], sd["pos"], False).y
    assert (np.abs(y) >= C.HALF_INF).any(), "the case holds a sum beyond the half range"


# ----------------------------------------------------------------------------------------------------------- the reference

def _books():
    names = []
    for cs in TRAINING + B.SECOND_STREAM + B.SPLIT + B.EVAL:
        if (cs["book"], cs["transposed"]) not in names:
            names.append((cs["book"], cs["transposed"]))
    return names


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("name,transposed", _books(), ids=[f"{n}{'-T' if t else ''}" for n, t in _books()])
def test_the_reference_against_autograd_in_double(name, transposed, addend):
    """reference_chain against torch in double under autograd: a dense index_add convolution built from the rulebook, BatchNorm1d,
    the residual, ReLU; the addend reaches the input along a second path"""
    cs = B.case(name, 8, 12, transposed=transposed, addend=addend)
    bk = B.book(name)
    sd = bk.sides(transposed)
    ops = B.operands(cs)
    if addend:
        ops["addend"] = C.second_operand("dense", sd["n_dgrad"], 8, "autograd addend")
    ref = B.reference_chain(cs, ops)
    x = torch.from_numpy(B.f64(ops["feat"])).requires_grad_()
    w = torch.from_numpy(B.f64(ops["kernel"])).requires_grad_()
    res = torch.from_numpy(B.f64(ops["residual"])).requires_grad_()
    bn = torch.nn.BatchNorm1d(12, eps=B.EPS, momentum=B.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(B.f64(ops["bn_w"])))
        bn.bias.copy_(torch.from_numpy(B.f64(ops["bn_b"])))
        bn.running_mean.copy_(torch.from_numpy(B.f64(ops["rm0"])))
        bn.running_var.copy_(torch.from_numpy(B.f64(ops["rv0"])))
    src, dst = (bk.nbmaps[:, 1], bk.nbmaps[:, 0]) if transposed else (bk.nbmaps[:, 0], bk.nbmaps[:, 1])
    conv = torch.zeros((sd["n_out"], 12), dtype=torch.float64)
    for k in range(bk.k):
        lo, hi = int(bk.nboffs[k]), int(bk.nboffs[k + 1])
        if hi > lo:
            conv = conv.index_add(0, torch.from_numpy(dst[lo:hi].astype(np.int64)), x[torch.from_numpy(src[lo:hi].astype(np.int64))] @ w[k])
    conv.retain_grad()
    if sd["n_out"] > 1:
        y = torch.relu(bn(conv) + res)
    else:                                                                # BatchNorm1d refuses one row: its formulas, spelled out
        y = torch.relu((conv - conv.mean(0)) * (conv.var(0, unbiased=False) + B.EPS).rsqrt() * bn.weight + bn.bias + res)
    gy = torch.from_numpy(B.f64(ops["grad_out"]))
    loss = (y * gy).sum()
    if addend:
        loss = loss + (x * torch.from_numpy(B.f64(ops["addend"]))).sum()
    loss.backward()
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-11, atol=1e-12)    # noqa: E731
    close(ref["conv_out"], conv)
    close(ref["out"], y)
    close(ref["grad_conv"], conv.grad)
    close(ref["grad_residual"], res.grad)
    close(ref["grad_bn_weight"], bn.weight.grad)
    close(ref["grad_bn_bias"], bn.bias.grad)
    close(ref["grad_kernel"], w.grad)
    close(ref["grad_feat"], x.grad)
    if sd["n_out"] > 1:
        close(ref["running_mean"], bn.running_mean)
        close(ref["running_var"], bn.running_var)


@pytest.mark.parametrize("name", ["SUB127", "SUB129", "SUB257", "D128", "D8", "D129"])
def test_the_plans_reach_the_rulebook_s_pairs(name):
    """the input gradient a class plan forms - the mirrored slice on a submanifold table, the inverse table of a strided one - is the
    rulebook's expression through W_k^T on dgrad_gather_col and pos_dgrad; without the mirror it is not"""
    bk = B.book(name)
    rs = np.random.RandomState(3)
    for transposed in (False,) if bk.kind == "sub" else (False, True):      # (the blocks on a submanifold map are never transposed)
        sd = bk.sides(transposed)
        g, w = rs.randn(sd["n_out"], 5), rs.randn(bk.k, 3, 5)
        want = B.conv_ref(g, w, bk, sd["dgrad_gather_col"], sd["pos_dgrad"], True).y
        if bk.kind == "sub":
            got = K.class_gemm64(g, w, bk.nbr, 3, True, True).z.sum(0)
            assert not np.allclose(K.class_gemm64(g, w, bk.nbr, 3, True, False).z.sum(0), want)
        else:
            got = K.class_gemm64(g, w, sd["nbr_d"], 1, True, False).z[0]
        assert np.allclose(got, want, rtol=0, atol=1e-12)
        x, wf = rs.randn(sd["n_feat"], 3), rs.randn(bk.k, 3, 5)
        fwd = K.class_gemm64(x, wf, sd["nbr_f"], bk.groups, False, False).z.sum(0)
        assert np.allclose(fwd, B.conv_ref(x, wf, bk, sd["gather_col"], sd["pos"], False).y, rtol=0, atol=1e-12)


def test_the_cases_are_the_ones_asked_for():
    nboffs = B.book("EDGE").nboffs
    chunks = -(-int(nboffs[-1]) // CHUNK)
    straddling = sum(1 for c in range(chunks) if len({int(np.searchsorted(nboffs, p, side="right")) for p in (c * CHUNK, min((c + 1) * CHUNK, int(nboffs[-1])) - 1)}) > 1)
    assert int(nboffs[-1]) == 1935 and chunks == 16 and straddling >= 2 and int((np.diff(nboffs) == 0).sum()) == 9
    for name, m_pad, pairs in (("SUB127", 384, 1143), ("SUB129", 768, 1521), ("SUB257", 1152, 1739)):
        bk = B.book(name)
        assert 3 * K.npad_of(bk.n_out) == m_pad and bk.p == pairs and m_pad <= pairs        # plan_fits accepts the plan
    assert B.book("SUB1").p == 1                                                            # ... and declines this one
    d = B.book("D129")
    assert (d.n_in, d.n_out) == (129, 300)
    assert B.pack_mask(np.array([[1, 0, -1, 2, 0, 0, 0, 3]], dtype=np.float32), False).tolist() == [0b1001, 0b1000]
    ids = [B.case_id(cs) for cs in TRAINING + B.KEPT + B.SECOND_STREAM + B.SPLIT] + [B.eval_id(cs) for cs in B.EVAL]
    assert len(set(ids)) == len(ids)
