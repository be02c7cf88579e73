"""Float64 reference of the fused conv-block calls of csrc/block.hip - ts_conv_block_forward, ts_conv_block_backward (with
ts_conv_block_wgrad_side) and ts_conv_block_eval - stage by stage, with the bars of every stage: test infrastructure, not product
code.  Plain numpy (the BatchNorm stages go through oracle/bn64.py, tensor ops in double); nothing of taseg_amd is imported.
tests/test_block64_host.py checks this file (the reference against autograd in double, a float32 / half emulation of every call
inside every bar, twelve emulated wrong calls rejected); tests/test_gpu_block_float64.py holds the calls against it.  The cases live
here so that both files run the same ones; both run the same walk (check_training, check_eval) on what a driver returns.

No bar of its own: every stage is held to the bar of the kernel family it reaches, composed from conv64, class64 and bn64.  u = 2^-24,
u16 = 2^-11, SLACK, TINY: conv64's.  Every stage receives the DEVICE'S OWN previous stage, cast up unchanged.

  1 conv_out    y[j] = sum over the rulebook pairs p of row j of feat[nbmaps[p][gather_col]] @ W_k(p), with per pair S_p = |x| |W_k| and
                N_p = the products that are not zero, L = the pairs of row j.
                fp32, either route (pair GEMM + pass 2, class plan):     sum_p bar_pass1(S_p, N_p) + SLACK (L - 1) u sum_p S_p
                  bar_pass1 = conv64.bar_pass1_split where the call reaches a split-bf16 kernel (the class kernels; the pair GEMM on
                  channel counts that are multiples of 32 under conv_impl 0), conv64.bar_pass1_f32 where it reaches the guarded or the
                  scalar kernel (every other channel pair; conv_impl 1).  Inside a group of a class plan and across its groups the
                  additions that round are L - 1 in all.
                half, pair route: Z is rounded to half per pair, b_p = conv64.bar_pass1_half(z64_p, S_p, N_p); pass 2 adds the rows in
                  float32 and rounds once.  With B = sum_p b_p, A = sum_p (|z64_p| + b_p) >= sum |Z row|:
                        (1 + u16) (B + SLACK (L - 1) u A) + u16 |y64| + 2^-25
                  (conv64.bar_pass2_half on a Z that is itself only known to b_p; the factor 1 + u16: the rounding acts on the float32
                  sum, not on y64).  The natural form (K = 1, the product's rows ARE the result): b_p alone.
                half, class route: a direct plan rounds the sum of a row once, class64.bar_class_half; a pass-2 plan rounds Z' per
                  group (class64.bar_class_half of the group) and pass 2 - or the finish inside the product, the same bits - once
                  more: the expression above over groups instead of pairs.
                L = 0: exactly +0.
  2 forward     out, mean, invstd, running_mean, running_var, num_batches_tracked from bn64.bn_ref64 / running_ref64 on the device's
                conv_out, bars LAMBDA(n, c) u S as in tests/test_gpu_bn_float64.py (var observed as 1 / invstd^2 - eps); the mask bits
                are exactly `stored out > 0`: the ReLU's derivative follows the STORED value (a positive fp32 value of at most 2^-25
                is a half zero and passes nothing).  Every operand set carries such an element: BatchNorm weight 0 and bias 2^-26 in
                channel 1, so that out = 2^-26 there in fp32 and +0 in half storage.
  3 backward    grad_bn_weight, grad_bn_bias, grad_residual (exactly grad_out where the stored out > 0) and the gradient w.r.t. the
                convolution output.  That one is no output of the call: the tests take its bits from ts_bn_act_train_backward[_f16] on
                the same operands (and, second stream, from the head of wgrad_ws, asserted equal) - held to bn_ref64 here.
  4 grad_kernel conv64.wgrad64(feat, grad_conv, col_a = wgrad_col_a) with conv64.bar_wgrad (m = 6 where the fp32 call reaches the split
                kernel, else 1); an offset without a pair is +0 in every bit whatever the buffer held.
  5 grad_feat   stage 1's expression on grad_conv through W_k^T, on dgrad_gather_col and pos_dgrad (on a submanifold map the class plan
                reaches the same pairs as W_{K-1-k}^T of the mirrored table: class64.weight_slice; the host file shows the two agree).
                The addend is one more term of the final sum: L + 1 terms, S + |addend| (class64.with_addend's fourth row).
  eval          stage 1, then act((s - mean) invstd w + b [+ residual]).  Where the tail rides on pass 2 the sum s is not rounded to
                storage in between: the bar of s (half: B + SLACK (L - 1) u A, no rounding of the sum) carried through |invstd w|, plus
                8 u S_e of the elementwise operations, S_e = (|s| + |mean|) |invstd w| + |b| + |residual| (the term
                tests/test_gpu_bn_float64.py uses for this tail), plus one half rounding of the result.  A sum of 65520 or more is
                therefore no infinity: the half_large cases of the evaluation block hold sums beyond the half range whose result is
                finite.  Where the separate pass runs, the stored conv_out bits of a training forward on the same operands are cast
                up and only the elementwise bar applies.
"""
import numpy as np
import torch

from oracle import bn64
from oracle import class64 as K
from oracle import conv64 as C
from oracle.conv64 import HALF_SUB, HALF_U, SLACK, U, rng

EPS = float(np.float32(1e-5))                 # the calls take eps and momentum as floats
MOMENTUM = float(np.float32(0.1))
TINY_CH = 1                                   # the channel whose pre-activation is exactly 2^-26 (module docstring, stage 2)


def f64(a):
    return np.asarray(a).astype(np.float64)


def bits(a):
    return a.view(np.int16) if a.dtype == np.float16 else a.view(np.int32)


def t64(a):
    return None if a is None else torch.from_numpy(f64(a))


# ---------------------------------------------------------------------------------------------------------------- rulebooks

class Book:
    """a kernel map as the block calls name it: nbmaps [P, 2] (input row, output row), nboffs [K + 1], pos_out [K, n_out],
    pos_in [K, n_in]; nbr [K, n_out] (the input row of (offset, output row) or -1) and kind "pairs" | "sub" | "down" | "identity" """

    def __init__(self, name):
        self.name = name
        if name == "ID257":                    # the identity rulebook of a 1x1x1 convolution: pair p = (p, p)
            n = 257
            self.nbmaps = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
            self.nboffs = np.array([0, n], dtype=np.int32)
            self.pos_out = self.pos_in = np.arange(n, dtype=np.int32)[None]
            self.n_in = self.n_out = n
            self.kind, self.groups = "identity", 1
        elif name in C.COUNTS:
            self.nbmaps, self.nboffs, self.pos_out, self.pos_in, n = C.rulebook(name)
            self.n_in = self.n_out = n
            self.kind, self.groups = "pairs", 0
        else:
            nbr, self.n_in, self.groups, self.kind = K.table(name)
            self.n_out = nbr.shape[1]
            self.nbmaps, self.nboffs, self.pos_in = K.rulebook_of(nbr, self.n_in)
            self.pos_out = np.full(nbr.shape, -1, dtype=np.int32)
            k_of = np.repeat(np.arange(nbr.shape[0]), np.diff(self.nboffs))
            self.pos_out[k_of, self.nbmaps[:, 1]] = np.arange(len(self.nbmaps))
        self.k, self.p = len(self.nboffs) - 1, int(self.nboffs[-1])
        C.check_rulebook(self.nbmaps, self.nboffs, self.pos_out, self.pos_in, self.n_in, self.n_out)
        self.nbr = np.where(self.pos_out >= 0, self.nbmaps[np.maximum(self.pos_out, 0), 0], -1).astype(np.int32)
        self.nbr_t = np.where(self.pos_in >= 0, self.nbmaps[np.maximum(self.pos_in, 0), 1], -1).astype(np.int32)

    def sides(self, transposed):
        """the rulebook arguments of a block on this map, as torchsparse's ConvolutionFunction picks them: the strided block gathers
        column 0 and sums into the output rows; the transposed block swaps the columns"""
        if not transposed:
            return dict(gather_col=0, pos=self.pos_out, n_feat=self.n_in, n_out=self.n_out, dgrad_gather_col=1, pos_dgrad=self.pos_in,
                        n_dgrad=self.n_in, wgrad_col_a=0, nbr_f=self.nbr, nbr_d=self.nbr_t)
        return dict(gather_col=1, pos=self.pos_in, n_feat=self.n_out, n_out=self.n_in, dgrad_gather_col=0, pos_dgrad=self.pos_out,
                    n_dgrad=self.n_out, wgrad_col_a=1, nbr_f=self.nbr_t, nbr_d=self.nbr)


_BOOKS = {}


def book(name):
    if name not in _BOOKS:
        _BOOKS[name] = Book(name)
    return _BOOKS[name]


# -------------------------------------------------------------------------------------------------------------------- cases
# A case is a dict; what it leaves out is the default below.  route_f / route_d: what the forward product and the input gradient must
# run on - "pairs" (pair GEMM + pass 2), "class" (class GEMM + pass 2), "finish" (the finish inside the product), "direct", "natural" -
# the launches of the device run are held to it (expected_kinds).  plan_f / plan_d: a plan is handed to the call; spoil: how the
# plan is made unfit ("map_id", "rows"), the call must then take the two passes.  family: conv64's operand families ("one_hot": one
# product per pair, the rows nearest their bars).  kept: the call receives what the caller keeps in step with the weight - the pre-split
# bf16 planes (fp32), the half copy with w16_current (half) - and must give the bits of the call without them.

DEFAULT = dict(half=False, transposed=False, relu=1, residual=True, grad_feat=True, addend=False, route_f="pairs", route_d="pairs",
               plan_f=False, plan_d=False, spoil=None, impl=0, gk_off=False, natural=False, stream=None, split=False, family="dense",
               kept=False)


def case(book_name, c_in, c_out, **kw):
    out = dict(DEFAULT, book=book_name, c_in=c_in, c_out=c_out)
    assert set(kw) <= set(DEFAULT), kw
    out.update(kw)
    if not out["grad_feat"]:
        out["route_d"] = None
    return out


def case_id(cs):
    flags = [cs["book"], f"{cs['c_in']}to{cs['c_out']}", "half" if cs["half"] else "fp32"]
    flags += ["T"] if cs["transposed"] else []
    flags += [] if cs["relu"] else ["norelu"]
    flags += [] if cs["residual"] else ["nores"]
    flags += [] if cs["grad_feat"] else ["nogf"]
    flags += ["addend"] if cs["addend"] else []
    flags += [f"f={cs['route_f']}"] if cs["plan_f"] or cs["natural"] else []
    flags += [f"d={cs['route_d']}"] if cs["plan_d"] else []
    flags += [f"spoil={cs['spoil']}"] if cs["spoil"] else []
    flags += [f"impl{cs['impl']}"] if cs["impl"] else []
    flags += ["gkoff"] if cs["gk_off"] else []
    flags += [cs["stream"]] if cs["stream"] else []
    flags += ["split"] if cs["split"] else []
    flags += [cs["family"]] if cs["family"] != "dense" else []
    flags += ["kept"] if cs["kept"] else []
    return "-".join(flags)


def _both(book_name, c_in, c_out, **kw):
    """the fp32 case, and the half one where both widths are multiples of 32"""
    out = [case(book_name, c_in, c_out, **kw)]
    if C.is_half_shape(c_in, c_out):
        out.append(case(book_name, c_in, c_out, half=True, **kw))
    return out


# group 1: training forward and backward on the two-pass route
TWO_PASS = (
    _both("EDGE", 32, 32) + _both("EDGE", 96, 128) + _both("EDGE", 48, 24) + _both("TINY27", 32, 32) + _both("K8", 96, 128, transposed=True)
    + _both("K1", 32, 32) + _both("K8", 32, 32, relu=0, residual=False) + _both("K8", 32, 32, relu=0) + _both("EDGE", 32, 32, residual=False)
    + _both("EDGE", 96, 128, grad_feat=False) + [case("K8", 4, 32, grad_feat=False, residual=False), case("EDGE", 96, 20), case("K8", 32, 16)]
    + _both("EDGE", 32, 32, gk_off=True) + [case("K8", 96, 128, gk_off=True, grad_feat=False), case("K8", 32, 32, impl=1)]
    + _both("EDGE", 32, 32, family="one_hot") + _both("K8", 96, 128, family="one_hot", transposed=True, residual=False))

# group 2: the addend
ADDEND = (
    _both("EDGE", 32, 32, addend=True) + _both("K8", 96, 128, addend=True, transposed=True)
    + _both("SUB129", 96, 128, addend=True, plan_d=True, route_d="class") + _both("SUB129", 96, 128, addend=True, plan_d=True, route_d="finish")
    + _both("SUB257", 32, 32, addend=True, plan_d=True, route_d="finish")
    + _both("D129", 32, 32, addend=True, plan_d=True, route_d="pairs") + _both("D129", 32, 32, addend=True, plan_d=True, route_d="pairs", transposed=True))

# group 3: class plans inside the block
PLANS = []
for _name, _ch in (("SUB127", (32, 32)), ("SUB129", (96, 128)), ("SUB257", (256, 128)), ("SUB257", (32, 32))):
    PLANS += _both(_name, *_ch, plan_f=True, plan_d=True, route_f="class", route_d="class")
PLANS += _both("SUB129", 32, 32, plan_f=True, plan_d=True, route_f="finish", route_d="finish")
for _name, _ch in (("D128", (32, 32)), ("D8", (96, 128)), ("D129", (256, 128)), ("D129", (32, 32))):
    for _t in (False, True):
        PLANS += _both(_name, *_ch, plan_f=True, plan_d=True, route_f="direct", route_d="direct", transposed=_t)
PLANS += _both("SUB129", 96, 128, plan_f=True, plan_d=True, route_f="class", route_d="class", family="one_hot")
PLANS += _both("D8", 96, 128, plan_f=True, plan_d=True, route_f="direct", route_d="direct", family="one_hot")
# ... with the caller's pre-split planes / kept half weights: each against the same case without them, bit for bit
KEPT = [dict(cs, kept=True) for cs in _both("EDGE", 96, 128) + _both("SUB257", 256, 128, plan_f=True, plan_d=True, route_f="class", route_d="class")
        + _both("D129", 256, 128, plan_f=True, plan_d=True, route_f="direct", route_d="direct")]
REFUSED_PLANS = (
    _both("SUB129", 32, 32, plan_f=True, plan_d=True, spoil="map_id") + _both("SUB129", 32, 32, plan_f=True, plan_d=True, spoil="rows")
    + _both("D128", 32, 32, plan_f=True, plan_d=True, spoil="map_id") + _both("SUB1", 32, 32, plan_f=True, plan_d=True)
    + [case("SUB129", ci, co, plan_f=True, plan_d=True) for ci, co in K.REFUSED_CHANNELS])

# group 4: the natural form
NATURAL = _both("ID257", 32, 32, natural=True, route_f="natural", route_d="natural") + _both("ID257", 96, 128, natural=True, route_f="natural",
                                                                                             route_d="natural", relu=0, residual=False)
# group 5: the weight gradient on a second stream (each against the riding form of the same case without `stream`)
SECOND_STREAM = [dict(cs, stream=s) for s in ("stream", "deferred")
                 for cs in _both("EDGE", 32, 32) + _both("EDGE", 96, 128, grad_feat=False) + [case("EDGE", 48, 24)]]
# group 6: the split call
SPLIT = [dict(cs, split=True) for cs in _both("EDGE", 32, 32) + _both("K8", 96, 128, transposed=True)]

# group 7: the evaluation block.  tail: the tail must ride on pass 2 (True) or run as the separate pass (False); option:
# eval_tail_in_pass2
def eval_case(book_name, c_in, c_out, tail, option=True, **kw):
    return dict(case(book_name, c_in, c_out, **kw), tail=tail, option=option)


EVAL = (
    [eval_case("EDGE", 32, 32, True), eval_case("EDGE", 32, 32, False, option=False), eval_case("EDGE", 32, 32, True, relu=0, residual=False),
     eval_case("K8", 32, 16, True), eval_case("EDGE", 96, 20, True), eval_case("K8", 32, 12, False),
     eval_case("K8", 96, 128, True, transposed=True, residual=False), eval_case("SUB129", 96, 128, True, plan_f=True, route_f="class"),
     eval_case("D129", 32, 32, False, plan_f=True, route_f="direct")]
    + [eval_case("EDGE", 96, 128, True, half=True), eval_case("EDGE", 96, 128, False, half=True, option=False),
       eval_case("EDGE", 32, 32, False, half=True), eval_case("K8", 64, 64, True, half=True, relu=0, residual=False),
       eval_case("K8", 96, 128, True, half=True, family="half_large"), eval_case("SUB129", 96, 128, True, half=True, plan_f=True, route_f="class")])


def eval_id(cs):
    return case_id(cs) + ("-tail" if cs["tail"] else "-separate") + ("" if cs["option"] else "-optoff")


def expected_kinds(cs, direction):
    """the record kinds (include/taseg_hip.h: 0 pair GEMM, 1 gather-sum, 2 weight gradient, 3 class GEMM, 4 class GEMM with finish, 5
    ordered sum as its own launch) a call of the case must leave, in order"""
    conv = {"pairs": [0, 1], "class": [3, 1], "finish": [4], "direct": [3], "natural": [0], None: []}
    if direction == "forward":
        return conv[cs["route_f"]]
    if cs["stream"] == "deferred":
        return conv[cs["route_d"]] + [2, 5]
    return [2] + conv[cs["route_d"]]


# ----------------------------------------------------------------------------------------------------------------- operands

def _rows(n, c, key, half, top):
    """float32 [n, c]: every row on its own power of two 2^-top .. 2^top; half storage: magnitudes 0.5 .. 1.5, no half subnormal"""
    rs = rng("block", key, n, c, half)
    return (C._normal(rs, (n, c), half) * np.ldexp(1.0, rs.randint(-top, top + 1, size=(n, 1)))).astype(np.float32)


def operands(cs):
    """every operand of the case's calls, in its storage type (float32, or the halves), deterministic in the case's shape"""
    bk = book(cs["book"])
    sd = bk.sides(cs["transposed"])
    half, c_in, c_out = cs["half"], cs["c_in"], cs["c_out"]
    key = (cs["book"], cs["transposed"])
    store = (lambda a: C.to_half(a)) if half else (lambda a: np.ascontiguousarray(a, dtype=np.float32))
    fam = cs["family"]
    if fam == "dense":
        feat = _rows(sd["n_feat"], c_in, key + ("feat",), half, 3 if half else 6)
        kernel = C.weights("dense", bk.k, c_in, c_out, key, False, half)
    else:                                       # conv64's families (half_large: sums beyond the half range)
        feat = C.features(fam, sd["n_feat"], c_in, key, half)
        kernel = C.weights(fam, bk.k, c_in, c_out, key, False, half)
    rs = rng("block", key, c_in, c_out, "bn")
    bn_w = ((rs.rand(c_out) + 0.5) * np.where(np.arange(c_out) % 3 == 0, -1.0, 1.0)).astype(np.float32)
    bn_b = rs.randn(c_out).astype(np.float32)
    residual = C._normal(rs, (sd["n_out"], c_out), half).astype(np.float32) if cs["residual"] else None
    if cs["relu"]:                              # the element the stored-value rule is about
        bn_w[TINY_CH], bn_b[TINY_CH] = 0.0, 2.0 ** -26
        if residual is not None:
            residual[:, TINY_CH] = 0.0
    ops = dict(feat=store(feat), kernel=np.ascontiguousarray(kernel, dtype=np.float32), bn_w=bn_w, bn_b=bn_b,
               residual=None if residual is None else store(residual), rm0=rs.randn(c_out).astype(np.float32),
               rv0=(rs.rand(c_out) + 0.5).astype(np.float32),
               grad_out=store(C.second_operand("dense", sd["n_out"], c_out, key + ("gy",), half) + np.float32(0.25)),
               addend=None, mean=None, invstd=None)
    if half:                                    # what the call's cast must write into w16 (round to nearest even)
        ops["w16"] = ops["kernel"].astype(np.float16)
    return ops


def make_addend(cs, ops, grad_conv):
    """[n_dgrad, c_in] in grad_feat's storage type: even rows cancel the input gradient itself (minus its float64 reference, rounded to
    the storage type) - what is left there is rounding, where an addend added twice or dropped shows at full size; odd rows dense"""
    bk = book(cs["book"])
    sd = bk.sides(cs["transposed"])
    w = f64(ops["w16"] if cs["half"] else ops["kernel"])
    ref = conv_ref(f64(grad_conv), w, bk, sd["dgrad_gather_col"], sd["pos_dgrad"], True)
    add = f64(_rows(sd["n_dgrad"], cs["c_in"], (cs["book"], "addend"), cs["half"], 3))
    add[::2] = -ref.y[::2]
    add = np.clip(add, -60000.0, 60000.0)
    return add.astype(np.float16) if cs["half"] else add.astype(np.float32)


def eval_statistics(cs, ops):
    """the caller's mean / invstd of an evaluation block: the running statistics, 1 / sqrt(running_var + eps) - for half_large an invstd
    that brings sums of 10^5 back into the half range"""
    mean = ops["rm0"].copy()
    invstd = (1.0 / np.sqrt(f64(ops["rv0"]) + EPS)).astype(np.float32)
    if cs["family"] == "half_large":
        mean, invstd = (mean * np.float32(1000.0)).astype(np.float32), (invstd * np.float32(2.0 ** -12)).astype(np.float32)
    return mean, invstd


# ------------------------------------------------------------------------------------------------------------------ stage 1

class Conv:
    """y, S, A = sum |z64_p|, L [rows]; z, s, n: the pairs' own (conv64.pair_gemm64); pos"""


def conv_ref(x, w, bk, gather_col, pos, wt):
    """the convolution over the rulebook: w [K, c_in, c_out] as stored; wt: through W_k^T (the input gradient)"""
    cv = Conv()
    cv.z, cv.s, cv.n = C.pair_gemm64(x, w, bk.nbmaps, bk.nboffs, gather_col, wt)
    cv.y, cv.A, cv.L = C.gather_sum64(cv.z, pos)
    cv.S = C.gather_sum64(cv.s, pos)[0]
    cv.pos = pos
    return cv


def split_kernel(route, c_red, c_out, half, impl):
    """does the fp32 product reach a split-bf16 kernel (else: the guarded or the scalar f32 kernel)"""
    if half:
        return False
    if route in ("class", "finish", "direct"):
        return True
    return impl == 0 and C.is_half_shape(c_red, c_out)


def _groups_of(cv, groups):
    """per group of offsets: (|z_g|, bar_class_half of the group) summed over the live groups, and the count of live groups"""
    k = cv.pos.shape[0]
    gk = k // groups
    bar, mag = np.zeros_like(cv.y), np.zeros_like(cv.y)
    live = np.zeros(cv.pos.shape[1], dtype=np.int64)
    for g in range(groups):
        pg = cv.pos[g * gk:(g + 1) * gk]
        zg, _, lg = C.gather_sum64(cv.z, pg)
        ref = K.Ref(zg, C.gather_sum64(cv.s, pg)[0], C.gather_sum64(cv.n, pg)[0], lg, None)
        on = (lg > 0)[:, None]
        bar += np.where(on, K.bar_class_half(ref), 0.0)
        mag += np.where(on, np.abs(zg), 0.0)
        live += lg > 0
    return bar, mag, live


def conv_bar(cv, route, half, split, groups=0, addend=None, rounded=True):
    """the bar of stage 1 / stage 5 (module docstring).  addend: one more term of the final sum.  rounded = False: the float32 sum
    before it is stored (the evaluation tail riding on pass 2)"""
    extra = 0 if addend is None else 1
    a_abs = 0.0 if addend is None else np.abs(f64(addend))
    if not half:
        b1 = (C.bar_pass1_split if split else C.bar_pass1_f32)(cv.s, cv.n)
        return C.gather_sum64(b1, cv.pos)[0] + SLACK * np.maximum(cv.L + extra - 1, 0)[:, None] * U * (cv.S + a_abs)
    if route == "natural":                      # the product's rows are the result rows: one rounding
        return C.gather_sum64(C.bar_pass1_half(cv.z, cv.s, cv.n), cv.pos)[0]
    if route == "direct":
        ref = K.Ref(cv.y, cv.S, C.gather_sum64(cv.n, cv.pos)[0], cv.L, None)
        return K.bar_class_half(ref)
    if route == "pairs":
        b = C.bar_pass1_half(cv.z, cv.s, cv.n)
        parts_bar, parts_abs, parts = C.gather_sum64(b, cv.pos)[0], cv.A, cv.L
    else:
        parts_bar, parts_abs, parts = _groups_of(cv, groups)
    acc = parts_bar + SLACK * np.maximum(parts + extra - 1, 0)[:, None] * U * (parts_abs + parts_bar + a_abs)
    if not rounded:
        return acc
    y = cv.y if addend is None else cv.y + f64(addend)
    return (1.0 + HALF_U) * acc + HALF_U * np.abs(y) + HALF_SUB


def check_rows(ck, stage, what, got, ref, bar, live):
    """rows without a term exactly +0, the others inside the bar (half: conv64.check_half's rule for references of 65520 or more)"""
    none = live == 0
    ck.true(stage, f"{what}: shape {got.shape}", got.shape == ref.shape)
    if got.shape != ref.shape:
        return
    ck.true(stage, f"{what}: {int((bits(got)[none] != 0).sum())} elements of rows without a pair are not +0", bool((bits(got)[none] == 0).all()))
    if (~none).any():
        if got.dtype == np.float16:
            C.check_half(ck, stage, what, got[~none], ref[~none], bar[~none])
        else:
            C.check_close(ck, stage, what, got[~none], ref[~none], bar[~none])


# ------------------------------------------------------------------------------------------------------------ BatchNorm stages

def check_bn(ck, stage, what, got, ref, s, lam, extra=0.0):
    """|got - ref| <= LAMBDA u S (+ extra), + u16 |ref| + 2^-25 for a half result: the check of tests/test_gpu_bn_float64.py"""
    ref, s = np.asarray(ref), np.asarray(s)
    bar = lam * U * s + extra
    if got.dtype == np.float16:
        bar = bar + HALF_U * np.abs(ref) + HALF_SUB
    ck.true(stage, f"{what}: shape {got.shape}", got.shape == ref.shape)
    if got.shape == ref.shape:
        C.check_close(ck, stage, what, got, ref, bar)


def pack_mask(out, half):
    """the mask the forward must write: one byte per 4 (half: 8) channels of a row, bit i = stored out of channel i > 0"""
    ve = 8 if half else 4
    on = (f64(out) > 0).reshape(out.shape[0], out.shape[1] // ve, ve)
    return (on * (1 << np.arange(ve))).sum(2).astype(np.uint8).reshape(-1)


def bn_stages(cs, ops, conv_out, out, relu_from=True):
    """bn_ref64 on the device's conv_out: ((y, gx, gres, gw, gb, mean, var), (their S)) as numpy"""
    res, val = bn64.bn_ref64(t64(conv_out), t64(ops["residual"]), t64(ops["bn_w"]), t64(ops["bn_b"]), bool(cs["relu"]), EPS,
                             t64(ops["grad_out"]), relu_from=t64(out) if (cs["relu"] and relu_from) else None)
    num = lambda tup: tuple(None if t is None else t.numpy() for t in tup)  # noqa: E731
    return num(res), num(val)


def reference_chain(cs, ops):
    """the whole training call in float64 from the exact values of the inputs, every stage fed the reference's own previous stage (what
    tests/test_block64_host.py holds against autograd in double): dict of numpy arrays"""
    bk = book(cs["book"])
    sd = bk.sides(cs["transposed"])
    w = f64(ops["kernel"])
    cv = conv_ref(f64(ops["feat"]), w, bk, sd["gather_col"], sd["pos"], False)
    (y, gx, gres, gw, gb, mean, var), (_, _, _, _, _, smean, svar) = bn_stages(cs, ops, cv.y, None, relu_from=False)
    rm, rv, _, _ = (t.numpy() for t in bn64.running_ref64(t64(ops["rm0"]), t64(ops["rv0"]), t64(mean), t64(var), t64(smean), t64(svar),
                                                          sd["n_out"], MOMENTUM))
    out = dict(conv_out=cv.y, out=y, mean=mean, var=var, running_mean=rm, running_var=rv, grad_conv=gx, grad_residual=gres,
               grad_bn_weight=gw, grad_bn_bias=gb, grad_kernel=C.wgrad64(f64(ops["feat"]), gx, bk.nbmaps, bk.nboffs, sd["wgrad_col_a"])[0])
    dv = conv_ref(gx, w, bk, sd["dgrad_gather_col"], sd["pos_dgrad"], True)
    out["grad_feat"] = dv.y if ops.get("addend") is None else dv.y + f64(ops["addend"])
    return out


# ------------------------------------------------------------------------------------------------------------------ the walks

def check_training(ck, cs, ops, got, sfx=None):
    """one training forward + backward of a case: `got` holds what the driver's calls returned, as numpy arrays in their storage type -
    conv_out, out, mean, invstd, mask, running_mean, running_var, nbt, w16 (half); grad_feat, grad_residual, grad_kernel,
    grad_bn_weight, grad_bn_bias; grad_conv: the bits of the stand-alone BatchNorm backward on the same operands"""
    bk = book(cs["book"])
    sd = bk.sides(cs["transposed"])
    half, c_in, c_out, n = cs["half"], cs["c_in"], cs["c_out"], sd["n_out"]
    sfx = sfx if sfx is not None else ("_half" if half else "_f32")
    # ---- stage 1
    if half:
        ck.true("cast" + sfx, "w16 is not the weight rounded to half", np.array_equal(bits(got["w16"]), bits(ops["w16"])))
    w = f64(got["w16"] if half else ops["kernel"])
    cv = conv_ref(f64(ops["feat"]), w, bk, sd["gather_col"], sd["pos"], False)
    if half:
        assert np.abs(cv.y).max(initial=0.0) < C.HALF_MAX and np.abs(cv.z).max(initial=0.0) < C.HALF_MAX, "the references stay finite halves"
    split = split_kernel(cs["route_f"], c_in, c_out, half, cs["impl"])
    check_rows(ck, "conv_out" + sfx, "conv_out", got["conv_out"], cv.y, conv_bar(cv, cs["route_f"], half, split, bk.groups), cv.L)
    # ---- stage 2
    lam = bn64.LAMBDA(n, c_out, half)
    (ry, rgx, rgres, rgw, rgb, rmean, rvar), (sy, sgx, _, sgw, sgb, smean, svar) = bn_stages(cs, ops, got["conv_out"], got["out"])
    st = "forward" + sfx
    check_bn(ck, st, "out", got["out"], ry, sy, lam)
    check_bn(ck, st, "mean", got["mean"], rmean, smean, lam)
    ok = bool(np.isfinite(got["invstd"]).all() and (got["invstd"] > 0).all())
    ck.true(st, "invstd is not finite and positive", ok)
    if ok:
        check_bn(ck, st, "var = 1 / invstd^2 - eps", 1.0 / f64(got["invstd"]) ** 2 - EPS, rvar, svar, lam, extra=2 * U * (rvar + EPS))
    rm, rv, srm, srv = (t.numpy() for t in bn64.running_ref64(t64(ops["rm0"]), t64(ops["rv0"]), t64(rmean), t64(rvar), t64(smean), t64(svar),
                                                              n, MOMENTUM))
    check_bn(ck, st, "running_mean", got["running_mean"], rm, srm, lam)
    check_bn(ck, st, "running_var", got["running_var"], rv, srv, lam)
    ck.true(st, f"num_batches_tracked = {int(got['nbt'])}", int(got["nbt"]) == 1)
    if cs["relu"]:
        want = pack_mask(got["out"], half)
        ck.true(st, f"mask: {int((got['mask'] != want).sum())} bytes are not `stored out > 0`", np.array_equal(got["mask"], want))
        tiny = got["out"][:, TINY_CH]
        ck.true(st, "the pre-activation of 2^-26 is not stored as 2^-26 (fp32) / +0 (half)",
                bool((bits(tiny) == 0).all()) if half else bool((tiny == np.float32(2.0 ** -26)).all()))
    # ---- stage 3
    st = "bn_backward" + sfx
    check_bn(ck, st, "grad_conv (stand-alone BatchNorm backward)", got["grad_conv"], rgx, sgx, lam)
    check_bn(ck, st, "grad_bn_weight", got["grad_bn_weight"], rgw, sgw, lam)
    check_bn(ck, st, "grad_bn_bias", got["grad_bn_bias"], rgb, sgb, lam)
    if cs["residual"]:
        gy = ops["grad_out"]
        want = np.where(f64(got["out"]) > 0, gy, np.zeros_like(gy)) if cs["relu"] else gy
        ck.true(st, "grad_residual is not grad_out where the stored out > 0", np.array_equal(bits(got["grad_residual"]), bits(np.ascontiguousarray(want))))
    # ---- stage 4
    gc = f64(got["grad_conv"])
    dw64, s, cnt, n_k = C.wgrad64(f64(ops["feat"]), gc, bk.nbmaps, bk.nboffs, sd["wgrad_col_a"])
    m = 6 if (not half and cs["impl"] == 0 and C.is_half_shape(c_in, c_out)) else 1
    st = "grad_kernel" + sfx
    gk = got["grad_kernel"]
    ck.true(st, f"shape {gk.shape}", gk.shape == dw64.shape)
    if gk.shape == dw64.shape:
        empty = n_k == 0
        ck.true(st, f"{int((bits(gk)[empty] != 0).sum())} elements of offsets without a pair are not +0", bool((bits(gk)[empty] == 0).all()))
        keep = np.broadcast_to((~empty)[:, None, None], gk.shape)
        C.check_close(ck, st, "grad_kernel", gk, dw64, C.bar_wgrad(s, cnt, n_k, m), where=keep)
    # ---- stage 5
    st = "grad_feat" + sfx
    if not cs["grad_feat"]:
        ck.true(st, "a call without grad_feat returned one", got.get("grad_feat") is None)
        return
    dv = conv_ref(gc, w, bk, sd["dgrad_gather_col"], sd["pos_dgrad"], True)
    add = ops["addend"] if cs["addend"] else None
    ref = dv.y if add is None else dv.y + f64(add)
    if half:
        assert np.abs(ref).max(initial=0.0) < C.HALF_MAX
    split = split_kernel(cs["route_d"], c_out, c_in, half, cs["impl"])
    bar = conv_bar(dv, cs["route_d"], half, split, bk.groups, addend=add)
    live = dv.L + (1 if add is not None else 0)
    check_rows(ck, st, "grad_feat", got["grad_feat"], ref, bar, live)
    if add is not None:                         # rows without a pair: 0 + addend, the addend's own bits (a -0 reads +0)
        none = dv.L == 0
        gb_, ab_ = bits(got["grad_feat"])[none], bits(add)[none]
        same = (gb_ == ab_) | ((f64(add)[none] == 0) & (gb_ == 0))
        ck.true(st, f"{int((~same).sum())} elements of rows without a pair are not the addend's bits", bool(same.all()))


def check_eval(ck, cs, ops, got, sfx=None):
    """one evaluation block: got["out"]; where the separate pass must have run, got["conv_out"] = the stored convolution output of a
    training forward on the same operands"""
    bk = book(cs["book"])
    sd = bk.sides(cs["transposed"])
    half, c_in, c_out = cs["half"], cs["c_in"], cs["c_out"]
    sfx = sfx if sfx is not None else ("_half" if half else "_f32")
    mean, invstd, w, b = f64(ops["mean"]), f64(ops["invstd"]), f64(ops["bn_w"]), f64(ops["bn_b"])
    res = 0.0 if ops["residual"] is None else f64(ops["residual"])
    scale = np.abs(invstd * w)

    def tail(s):
        v = (s - mean) * invstd * w + b + res
        se = (np.abs(s) + np.abs(mean)) * scale + np.abs(b) + np.abs(res)
        return (np.maximum(v, 0.0) if cs["relu"] else v), se

    st = ("eval_tail" if cs["tail"] else "eval_separate") + sfx
    out = got["out"]
    if cs["tail"]:
        kw = f64(ops["w16"] if half else ops["kernel"])
        cv = conv_ref(f64(ops["feat"]), kw, bk, sd["gather_col"], sd["pos"], False)
        split = split_kernel(cs["route_f"], c_in, c_out, half, cs["impl"])
        ref, se = tail(cv.y)
        bar = conv_bar(cv, cs["route_f"], half, split, bk.groups, rounded=False) * scale + 8 * U * se
    else:
        ref, se = tail(f64(got["conv_out"]))
        bar = 8 * U * se
    if half:
        bar = bar + HALF_U * np.abs(ref) + HALF_SUB
        assert np.abs(ref).max(initial=0.0) < C.HALF_MAX, "the result stays a finite half"
    ck.true(st, f"out: shape {out.shape}", out.shape == ref.shape)
    if out.shape == ref.shape:
        C.check_close(ck, st, "out", out, ref, bar)
