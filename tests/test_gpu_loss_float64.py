"""The CE and Lovasz loss kernels of csrc/loss.hip against float64 (oracle/loss64.py), stage by stage through the C ABI.

The Lovasz gradient is piecewise constant in the sort order of the errors: an independent float64 evaluation that sorts its own errors
legitimately orders two errors the other way round where they differ by less than the fp32 rounding of the softmax, and the two rows
trade their gradients.  So the gradient is never compared with an independently sorted reference.  `check_chain` runs the kernels the
way `pcseg.loss._CeLovasz` and `lovasz._LovaszPresent` call them and hands the float64 reference the permutation the device sort
produced:

  1  ts_softmax_ce_forward and ts_lovasz_errors against float64 - no ordering in this stage
  2  the permutation is a permutation, carries the device errors, and is a valid descending order of the FLOAT64 errors
  3  ts_lovasz_grad on the given (errors_sorted, perm) against loss64.lovasz_from_perm64 with the same perm, errors cast up unchanged:
     the loss scalar and every element of grad_probas, in both layouts
  4  ts_ce_lovasz_finish and ts_ce_lovasz_backward on the device's own probas / grad_probas / out4 cast up unchanged, every element,
     and their NULL forms (no Lovasz term)
  5  pcseg.loss.Losses and lovasz.lovasz_softmax give the BITS of this file's chain, value and gradient
  6  the value - continuous, independent of the order inside a tie - against the fully independent oracle on double inputs
     (oracle.model.lovasz_softmax_ref, torch's cross_entropy) with its own sort

2 and 3 together say: the gradient is a valid subgradient of the true loss; 5 carries that to what the models call.  No element is
left out of any comparison.  Every check of a case is evaluated; the case fails with the list of those that missed.

Bars (u = 2^-24; each is computed from the inputs and the float64 reference, never from a kernel's output).

ts_lovasz_errors: |fg - p| is one rounding of a value <= 1: u absolute; 0 exactly on the rows that do not count.

ts_softmax_ce_forward (probas, errors, the two partial sums): the error depends on the device's expf / logf and on |x - max x|, so it
is measured against an independent fp32 evaluation - torch on the CPU: softmax / log_softmax in fp32 on the same logits, the row sum
of logp in fp32, the block sums in float64.  With e_ref the largest error of that evaluation against loss64, the kernel may have
max(4 e_ref, 2^-22 scale), scale = 1 for probas and errors and the largest |partial| of the case for a partial sum: as good as
another fp32 evaluation, with room for another summation order (the rule of test_conv_split_bf16_kernels_are_fp32_grade).  The number
of rows of a block is exact.  Each case prints its e_ref and the kernel's error (profiles/loss_float64.txt keeps a run's lines).

Order (stage 2): the device errors are sorted exactly (non-increasing) and each lies within the error allowed in stage 1 of its
float64 value; an adjacent pair of the float64 errors in device order may be inverted by no more than that error.  For
ts_lovasz_errors that is all two roundings can do: p itself is exact (fg = 0), 1 - p is exact for p >= 1/2 and lands in [1/2, 1],
spacing u, below - an error of at most u / 2 each, u for the pair.

ts_lovasz_grad.  For the element at position i of class c, a = gts - cum_i and b = gts + rank_i - cum_i are exact integers < 2^24.
q = a / b is one correctly rounded division (|dq| <= u q), j = 1 - q one rounding (<= u (1 - q)): |dj| <= u.  j_(i-1) is evaluated
from the same operands in the element behind it, to the same bits.  g_i = j_i - j_(i-1): |dg_i| <= 2 u + u |g_i|.  The factor
present_c / #present = fl(1 / #present) and the product add 2 u |g_i|:
    |d grad_probas| <= (2 + 3 |g_i|) u / #present            (<= 5 u / #present), every element
Loss: sum_i e_i g_i = sum_i j_i (e_i - e_(i+1)) (Abel; e sorted, e_P = 0), so the errors of the j's contribute <= u e_0 <= u; the
subtraction, the product and a summation tree of depth D = 3 (a thread's elements) + 6 + 2 (wave, workgroup) + ceil(tiles / 32) + 32
(lovasz_finish_kernel) on non-negative terms contribute (D + 2) u per_class; the mean over the classes (C additions, one division)
(C + 1) u loss:          |d loss| <= u (1 + (D + C + 3) loss)
Neither may exceed the bars the suite already holds this code to: 1e-4 max|ref| + 1e-7 (gradient), 5e-6 max(1, |ref|) (value).

ts_ce_lovasz_finish: ce is summed in double and rounded once: u |ce|; out[0] = w_ce ce + w_lov lov, three roundings:
3 u (|w_ce ce| + |w_lov lov|); out[2] and out[3] exact.

ts_ce_lovasz_backward: go [ w_ce / n ((1 - eps)(p - onehot) + eps (p - 1 / C)) + w_lov p (dp - sum_c p_c dp_c) ].  First term: two
roundings in go w_ce / n, seven in the bracket (|bracket| <= 1), one product: 10 u |go| w_ce / n.  Second, with m = max|dp|:
the dot product C u m, the difference, the two products and go w_lov 4 u 2 m: (C / 2 + 4) u |go| w_lov 2 m.  Their sum: one more.
    |d grad_logits| <= (C / 2 + 11) u |go| (w_ce / n + 2 w_lov m)            (w_ce / n := 0 when no row counts)
and no more than the present 1e-4 max|ref| + 1e-9.

smoothing, w_ce and w_lov reach the kernels as floats; the reference takes those float values.
"""
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import loss64 as L64

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SLACK = 1.01                 # second-order terms of the first-order bounds above
LV_TILE, LV_BIG_TILE, LV_BYTE_LABELS_FROM = 1024, 512, 1 << 20       # csrc/loss.hip
GO = 3.0                     # the upstream gradient
f32 = lambda v: float(np.float32(v))


# ------------------------------------------------------------------------------------------ the kernels, as the wrappers call them

def _L():
    from taseg_amd import _lib as L
    return L, L.load()


def ign_of(ignore):
    from taseg_amd.pcseg.loss.lovasz import _NO_IGNORE
    return _NO_IGNORE if ignore is None else int(ignore)


def k_forward(x, lab, ignore):
    L, lib = _L()
    p, c = x.shape
    probas = torch.empty((p, c), dtype=torch.float32, device=x.device)
    err = torch.empty((c, p), dtype=torch.float32, device=x.device)
    partials = torch.empty(((p + 255) // 256, 3), dtype=torch.float64, device=x.device)
    L.check(lib.ts_softmax_ce_forward(L.ptr(x), L.ptr(lab), ign_of(ignore), p, c, L.ptr(probas), L.ptr(err), L.ptr(partials),
                                      L.stream()), "ts_softmax_ce_forward")
    return probas, err, partials


def k_errors(probas, lab, ignore):
    L, lib = _L()
    p, c = probas.shape
    err = torch.empty((c, p), dtype=torch.float32, device=probas.device)
    L.check(lib.ts_lovasz_errors(L.ptr(probas), L.ptr(lab), ign_of(ignore), p, c, L.ptr(err), L.stream()), "ts_lovasz_errors")
    return err


def k_lovasz(es, perm, lab, ignore, class_major):
    L, lib = _L()
    c, p = es.shape
    loss = torch.empty(1, dtype=torch.float32, device=es.device)
    dprob = torch.empty((c, p) if class_major else (p, c), dtype=torch.float32, device=es.device)
    ws = L.workspace(lib.ts_lovasz_workspace_bytes(p, c), es.device)
    L.check(lib.ts_lovasz_grad(L.ptr(es), L.ptr(perm), L.ptr(lab), ign_of(ignore), p, c, L.ptr(loss), L.ptr(dprob),
                               1 if class_major else 0, L.ptr(ws), ws.numel(), L.stream()), "ts_lovasz_grad")
    return loss, dprob


def k_finish(partials, p, c, smoothing, w_ce, w_lov, lov):
    L, lib = _L()
    out4 = torch.empty(4, dtype=torch.float32, device=partials.device)
    L.check(lib.ts_ce_lovasz_finish(L.ptr(partials), p, c, float(smoothing), float(w_ce), float(w_lov), L.ptr(lov), L.ptr(out4),
                                    L.stream()), "ts_ce_lovasz_finish")
    return out4


def k_backward(probas, lab, ignore, dprob_cm, out4, go, smoothing, w_ce, w_lov):
    L, lib = _L()
    p, c = probas.shape
    got = torch.empty_like(probas)
    L.check(lib.ts_ce_lovasz_backward(L.ptr(probas), L.ptr(lab), ign_of(ignore), L.ptr(dprob_cm), L.ptr(out4), L.ptr(go), p, c,
                                      float(smoothing), float(w_ce), float(w_lov), L.ptr(got), L.stream()), "ts_ce_lovasz_backward")
    return got


def k_sort(err):
    return torch.sort(err, dim=1, descending=True)


def w_losses(logits, lab, ignore, smoothing, w_ce, w_lov):
    """pcseg.loss.Losses: (value, gradient of GO * value w.r.t. the logits)"""
    import taseg_amd.pcseg.loss as LS
    assert LS._FUSED
    crit = LS.Losses(["CELoss", "LovLoss"], [w_ce, w_lov], ignore_index=ignore, label_smoothing=smoothing)
    a = logits.clone().requires_grad_()
    got = crit(a, lab)
    (got * GO).backward()
    return got.detach(), a.grad


def w_lovasz(probas, lab, ignore):
    """lovasz.lovasz_softmax: (value, gradient of GO * value w.r.t. the probabilities)"""
    from taseg_amd.pcseg.loss import lovasz as LV
    assert LV._FUSED
    a = probas.clone().requires_grad_()
    got = LV.lovasz_softmax(a, lab, ignore=ignore)
    (got * GO).backward()
    return got.detach(), a.grad


# ------------------------------------------------------------------------------------------------------------------------- cases

def case(p, c, ignore=0, logits="randn2", labels="absent", smoothing=0.1, w=(1.0, 0.7)):
    return pytest.param((p, c, ignore, logits, labels, smoothing, w),
                        id=f"P{p}-C{c}-ign{ignore}-{logits}-{labels}-s{smoothing:g}-w{w[0]:g}_{w[1]:g}")


def make_inputs(p, c, ignore, logits_kind, labels_kind):
    """(logits fp32 [P, C], labels int64 [P]) on the CPU, seeded by the case"""
    rs = np.random.RandomState(zlib.crc32(repr((p, c, ignore, logits_kind, labels_kind)).encode()))
    base = rs.randn(p, c).astype(np.float32)
    x = {"randn2": lambda: base * 2, "offset80": lambda: base * 2 + 80, "sat30": lambda: base * 30,
         "tiny": lambda: base * 1e-3, "dup": lambda: base * 2}[logits_kind]().astype(np.float32)
    lab = rs.randint(0, c, size=p).astype(np.int64)
    one = 1 if c > 1 else 0                                   # a class that counts under every `ignore` used here
    outside = ignore is not None and not 0 <= ignore < c      # -100 / 255: such labels are put in
    if labels_kind == "absent":
        if c > 2:
            lab[lab == c - 1] = 1                             # the last class never occurs
        if outside:
            lab[rs.rand(p) < 0.15] = ignore
    elif labels_kind == "one_class":
        lab[:] = one
        lab[rs.rand(p) < 0.2] = ignore
    elif labels_kind == "one_valid":
        lab[:] = ignore
        lab[p // 2] = one
    elif labels_kind == "block_ignored":
        if c > 2:
            lab[lab == c - 1] = 1
        lab[256:512] = ignore
    elif labels_kind == "all_ignored":
        lab[:] = ignore
    else:
        raise KeyError(labels_kind)
    if p == 1 and labels_kind != "all_ignored":
        lab[0] = one
    if logits_kind == "dup":                                  # the second half repeats the first: exact ties in every class
        h = p // 2
        x[h:2 * h] = x[:h]
        lab[h:2 * h] = lab[:h]
    return torch.from_numpy(x), torch.from_numpy(lab)


def block_sums(cols):
    p = cols.shape[0]
    pad = (-p) % L64.ROWS
    if pad:
        cols = torch.cat([cols, cols.new_zeros(pad, cols.shape[1])])
    return cols.view(-1, L64.ROWS, cols.shape[1]).sum(dim=1)


def fp32_evaluation(x, lab, ignore):
    """the independent fp32 evaluation of stage 1 (torch, CPU): probas, errors [C, P], partials [blocks, 2] (block sums in float64)"""
    p, c = x.shape
    pr = torch.softmax(x, dim=1)
    lp = torch.log_softmax(x, dim=1)
    valid = torch.ones(p, dtype=torch.bool) if ignore is None else lab != ignore
    fg = ((lab.view(1, -1) == torch.arange(c).view(-1, 1)) & valid.view(1, -1)).float()
    err = (fg - pr.t()).abs() * valid.view(1, -1).float()
    picked = lp.gather(1, lab.clamp(0, c - 1).view(-1, 1)).view(-1)
    w = valid.double()
    return pr, err, block_sums(torch.stack([-picked.double() * w, -lp.sum(dim=1).double() * w], dim=1))


def worst(got, ref):
    return float((got.double() - ref.double()).abs().max())


def lovasz_depth(p):
    tiles = -(-p // (LV_BIG_TILE if p >= LV_BYTE_LABELS_FROM else LV_TILE))
    return 3 + 6 + 2 + -(-tiles // 32) + 32


class Checks:
    def __init__(self, cid):
        self.cid, self.missed, self.n, self.ratios = cid, [], 0, []

    def le(self, what, value, bound):
        self.n += 1
        self.ratios.append((what, value / bound if bound > 0 else (0.0 if value <= bound else math.inf)))
        if not value <= bound:
            self.missed.append(f"{what}: {value:.3e} > {bound:.3e}")

    def true(self, what, ok):
        self.n += 1
        if not ok:
            self.missed.append(what)

    def worst_ratio(self, part):
        return max([r for what, r in self.ratios if part in what], default=0.0)

    def done(self):
        print(f"loss_float64 {self.cid:<62} error / bar:  " + "  ".join(f"{name} {self.worst_ratio(part):.3f}" for name, part in (
            ("ts_lovasz_errors", "ts_lovasz_errors vs"), ("inversion (fused)", "fused largest inversion"),
            ("inversion (lovasz_softmax)", "lovasz_softmax largest inversion"), ("lovasz loss", "loss vs float64"),
            ("grad_probas", "grad_probas vs"), ("finish", "finish:"), ("backward", "backward: grad_logits"), ("oracle value", "6 "))))
        assert not self.missed, f"{self.cid}: {len(self.missed)} of {self.n} checks missed\n  " + "\n  ".join(self.missed)


def check_lovasz_stage(ck, tag, es, perm, err_dev, err64, b_err, lab, ignore, outs):
    """stages 2 and 3 for one sort: es, perm (CPU copies of the device sort's results) order err_dev; err64 are the float64 errors
    that err_dev approximates within b_err; outs = [(class_major, loss, grad_probas), ...] from ts_lovasz_grad.
    Returns the float64 (loss, grad_probas [P, C])."""
    c, p = es.shape
    ck.true(f"{tag} perm is a permutation of the rows", bool((torch.sort(perm, dim=1).values == torch.arange(p).view(1, -1)).all()))
    perm = perm.clamp(0, p - 1)
    ck.true(f"{tag} errors_sorted = errors[perm]", torch.equal(torch.gather(err_dev, 1, perm), es))
    ck.true(f"{tag} errors_sorted is non-increasing", bool((es[:, 1:] <= es[:, :-1]).all()))
    e64p = torch.gather(err64, 1, perm)
    if p > 1:
        ck.le(f"{tag} largest inversion of the float64 errors in device order",
              float((e64p[:, 1:] - e64p[:, :-1]).clamp_min(0.0).max()), b_err)
    loss64, d64, n_present, _ = L64.lovasz_from_perm64(es, perm, lab, ignore)
    loss64 = float(loss64)
    depth = lovasz_depth(p)
    b_loss = min(SLACK * U * (1.0 + (depth + c + 3) * abs(loss64)), 5e-6 * max(1.0, abs(loss64)))
    g_abs = d64.abs() * max(n_present, 1.0)                                  # |g_i| at the element's place
    b_grad = torch.clamp(SLACK * U * (2.0 + 3.0 * g_abs) / max(n_present, 1.0), max=1e-4 * float(d64.abs().max()) + 1e-7)
    first = None
    for class_major, loss, dprob in outs:
        lay = f"{tag} class_major={class_major}"
        got = dprob.t() if class_major else dprob
        ck.true(f"{lay} loss and grad_probas are finite", bool(torch.isfinite(loss).all()) and bool(torch.isfinite(got).all()))
        ck.le(f"{lay} loss vs float64 with the device order", abs(float(loss) - loss64), b_loss)
        ck.le(f"{lay} grad_probas vs float64 with the device order, worst error / the element's bar (max |ref| "
              f"{float(d64.abs().max()):.3e})", float(((got.double() - d64).abs() / b_grad).max()), 1.0)
        if n_present == 0:
            ck.true(f"{lay} nothing counts: loss 0, zero gradient", float(loss) == 0.0 and float(got.abs().max()) == 0.0)
        if first is None:
            first = (loss, got)
        else:
            ck.true(f"{lay} the two layouts hold the same bits", torch.equal(loss, first[0]) and torch.equal(got, first[1]))
    return loss64, d64


def check_chain(params, half=False):
    """stages 1 - 6 on one case"""
    from oracle import model as OM
    p, c, ignore, logits_kind, labels_kind, smoothing, (w_ce, w_lov) = params
    cid = f"P{p}-C{c}-ign{ignore}-{logits_kind}-{labels_kind}-s{smoothing:g}-w{w_ce:g}_{w_lov:g}" + ("-half" if half else "")
    ck = Checks(cid)
    s32, wce32, wlov32 = f32(smoothing), f32(w_ce), f32(w_lov)
    x_in, lab = make_inputs(p, c, ignore, logits_kind, labels_kind)
    if half:
        x_in = x_in.half()
    x = x_in.float()                                         # half logits: the chain on .float(), its gradient .half()
    valid = torch.ones(p, dtype=torch.bool) if ignore is None else lab != ignore
    n_valid = int(valid.sum())

    # ---- 1: ts_softmax_ce_forward
    p64, e64, part64 = L64.softmax_ce_forward64(x, lab, ignore)
    p32, e32, part32 = fp32_evaluation(x, lab, ignore)
    if logits_kind == "sat30":
        assert bool((e32[:, valid] == 0).any()), "the saturated case holds no fp32 error that is exactly 0"
    if logits_kind == "dup":
        h = p // 2
        assert torch.equal(e32[:, :h], e32[:, h:2 * h]) and h > 0, "the duplicated case holds no exact ties"
    xd, labd = x.to(DEV), lab.to(DEV)
    probas_d, err_d, part_d = k_forward(xd, labd, ignore)
    probas, err, part = probas_d.cpu(), err_d.cpu(), part_d.cpu()
    scale_nll = max(float(part64[:, 0].abs().max()), 0.0)
    scale_sm = max(float(part64[:, 1].abs().max()), 0.0)
    e_ref = [worst(p32, p64), worst(e32, e64), worst(part32[:, 0], part64[:, 0]), worst(part32[:, 1], part64[:, 1])]
    e_ker = [worst(probas, p64), worst(err, e64), worst(part[:, 0], part64[:, 0]), worst(part[:, 1], part64[:, 1])]
    bars = [max(4 * e_ref[0], 2.0 ** -22), max(4 * e_ref[1], 2.0 ** -22), max(4 * e_ref[2], 2.0 ** -22 * scale_nll),
            max(4 * e_ref[3], 2.0 ** -22 * scale_sm)]
    print(f"loss_float64 {cid:<62} " + "  ".join(f"{n} e_ref {r:.2e} kernel {k:.2e} bar {b:.2e}" for n, r, k, b in
                                                 zip(("probas", "errors", "nll", "smooth"), e_ref, e_ker, bars)))
    for name, k, b in zip(("probas", "errors", "partial sum of -logp[y]", "partial sum of -sum_c logp_c"), e_ker, bars):
        ck.le(f"1 ts_softmax_ce_forward {name} vs float64", k, b)
    ck.true("1 ts_softmax_ce_forward rows per block exact", torch.equal(part[:, 2], part64[:, 2]))
    ck.true("1 ts_softmax_ce_forward errors exactly 0 on the rows that do not count", float(err[:, ~valid].abs().sum()) == 0.0)
    b_err = bars[1]
    #      ts_lovasz_errors on the device's probabilities
    err2_d = k_errors(probas_d, labd, ignore)
    err2 = err2_d.cpu()
    e64_2 = L64.errors64(probas, lab, ignore)
    ck.le("1 ts_lovasz_errors vs float64 of the same probabilities", worst(err2, e64_2), U)
    ck.true("1 ts_lovasz_errors exactly 0 on the rows that do not count", float(err2[:, ~valid].abs().sum()) == 0.0)

    # ---- 2, 3: the fused chain's sort (both layouts) and lovasz_softmax's sort
    es_d, perm_d = k_sort(err_d)
    lov_d, dp_cm_d = k_lovasz(es_d, perm_d, labd, ignore, 1)
    lov_rm_d, dp_rm_d = k_lovasz(es_d, perm_d, labd, ignore, 0)
    lov64, d64 = check_lovasz_stage(ck, "2/3 fused", es_d.cpu(), perm_d.cpu(), err, e64, b_err, lab, ignore,
                                    [(1, lov_d.cpu(), dp_cm_d.cpu()), (0, lov_rm_d.cpu(), dp_rm_d.cpu())])
    es2_d, perm2_d = k_sort(err2_d)
    lov2_d, dp2_d = k_lovasz(es2_d, perm2_d, labd, ignore, 0)
    check_lovasz_stage(ck, "2/3 lovasz_softmax", es2_d.cpu(), perm2_d.cpu(), err2, e64_2, U, lab, ignore,
                       [(0, lov2_d.cpu(), dp2_d.cpu())])

    # ---- 4: finish and backward on the device's own intermediate values, and the NULL forms
    go_d = torch.tensor([GO], dtype=torch.float32, device=DEV)
    out4_d = k_finish(part_d, p, c, smoothing, w_ce, w_lov, lov_d)
    dlogits_d = k_backward(probas_d, labd, ignore, dp_cm_d, out4_d, go_d, smoothing, w_ce, w_lov)
    out4n_d = k_finish(part_d, p, c, smoothing, w_ce, w_lov, None)
    dlogitsn_d = k_backward(probas_d, labd, ignore, None, out4n_d, go_d, smoothing, w_ce, w_lov)
    lov_dev = float(lov_d.cpu())
    m = float(dp_cm_d.abs().max().cpu())
    for tag, o4, dl, lov_in, dp_in in (("4", out4_d.cpu(), dlogits_d.cpu(), lov_dev, dp_cm_d.cpu().t()),
                                       ("4 NULL", out4n_d.cpu(), dlogitsn_d.cpu(), None, None)):
        ref4 = L64.finish64(part, c, s32, wce32, wlov32, lov_in)
        ck.true(f"{tag} finish: rows that count exact", float(o4[3]) == float(ref4[3]) == float(n_valid))
        ck.true(f"{tag} finish: out[2] is the Lovasz scalar it was given", float(o4[2]) == (lov_in or 0.0))
        if n_valid:
            ce64 = float(ref4[1])
            ck.le(f"{tag} finish: ce vs float64", abs(float(o4[1]) - ce64), SLACK * U * abs(ce64) + 1e-12)
            ck.le(f"{tag} finish: total vs float64", abs(float(o4[0]) - float(ref4[0])),
                  SLACK * 3 * U * (abs(wce32 * ce64) + abs(wlov32 * (lov_in or 0.0))) + 1e-12)
        else:
            ck.true(f"{tag} finish: no row counts, ce and total are NaN (the mean over nothing)",
                    math.isnan(float(o4[1])) and math.isnan(float(o4[0])))
        refb = L64.backward64(probas, lab, ignore, dp_in, n_valid, GO, s32, wce32, wlov32)
        mm = m if dp_in is not None else 0.0
        b_bwd = min(SLACK * (c / 2 + 11) * U * GO * ((wce32 / n_valid if n_valid else 0.0) + 2 * wlov32 * mm),
                    1e-4 * float(refb.abs().max()) + 1e-9)
        ck.true(f"{tag} backward: every element finite", bool(torch.isfinite(dl).all()))
        ck.le(f"{tag} backward: grad_logits vs float64 (max |ref| {float(refb.abs().max()):.3e})", worst(dl, refb), b_bwd)

    # ---- 5: the wrappers give the bits of this chain
    got, grad = w_losses(x_in.to(DEV), labd, ignore, smoothing, w_ce, w_lov)
    ck.true("5 Losses: the value is out4[0] of the chain, to the bit", torch.equal(got.cpu(), out4_d[0].cpu())
            or (not n_valid and bool(torch.isnan(got)) and bool(torch.isnan(out4_d[0]))))
    want = dlogits_d.half() if half else dlogits_d
    ck.true("5 Losses: the gradient is the chain's, to the bit", grad.dtype == x_in.dtype and torch.equal(grad, want))
    if not half:
        got, grad = w_lovasz(probas_d, labd, ignore)
        ck.true("5 lovasz_softmax: value, to the bit", torch.equal(got.reshape(1).cpu(), lov2_d.cpu()))
        ck.true("5 lovasz_softmax: gradient, to the bit", torch.equal(grad, dp2_d * GO))

    # ---- 6: the value against the independent oracle, its own sort, in double
    oi = -1 if ignore is None else ignore
    lov_o = float(OM.lovasz_softmax_ref(x.double().softmax(1), lab, ignore=oi))
    ck.le("6 Lovasz value vs the independent oracle in double", abs(lov_dev - lov_o), 5e-6 * max(1.0, abs(lov_o)))
    ck.le("6 Lovasz value of lovasz_softmax's chain vs the independent oracle", abs(float(lov2_d.cpu()) - lov_o),
          5e-6 * max(1.0, abs(lov_o)))
    if n_valid:
        ce_o = float(torch.nn.functional.cross_entropy(x.double(), lab, ignore_index=oi, label_smoothing=s32))
        tot_o = wce32 * ce_o + wlov32 * lov_o
        o4 = out4_d.cpu()
        ck.le("6 CE value vs torch's cross_entropy in double", abs(float(o4[1]) - ce_o), 5e-6 * max(1.0, abs(ce_o)))
        ck.le("6 total vs the independent oracle in double", abs(float(o4[0]) - tot_o), 5e-6 * max(1.0, abs(tot_o)))
    ck.done()


# ------------------------------------------------------------------------------------------------------------------------- tests

CE_CLASSES = [1, 2, 5, 16, 17, 19, 20, 31, 32]


@pytest.mark.parametrize("params", [case(p, c, None if c <= 2 else 0) for c in CE_CLASSES for p in (1, 257)])
def test_class_counts_of_the_ce_kernels(params):
    """the compile-time class counts 20, 19, 17, the run-time path below, between and above them, and its limit 32 (LDS pitch 33); one
    row, and a full workgroup plus one row"""
    check_chain(params)


def _lovasz_only(p, c, ignore):
    """ts_lovasz_errors -> sort -> ts_lovasz_grad on given probabilities (stages 1 - 3, 5, 6) for class counts the CE kernels do not
    take"""
    from oracle import model as OM
    ck = Checks(f"lovasz P{p}-C{c}-ign{ignore}")
    x, lab = make_inputs(p, c, ignore, "randn2", "absent")
    probas = torch.softmax(x, dim=1)                         # given fp32 probabilities
    valid = torch.ones(p, dtype=torch.bool) if ignore is None else lab != ignore
    pd, labd = probas.to(DEV), lab.to(DEV)
    err_d = k_errors(pd, labd, ignore)
    err = err_d.cpu()
    e64 = L64.errors64(probas, lab, ignore)
    ck.le("1 ts_lovasz_errors vs float64", worst(err, e64), U)
    ck.true("1 ts_lovasz_errors exactly 0 on the rows that do not count", float(err[:, ~valid].abs().sum()) == 0.0)
    es_d, perm_d = k_sort(err_d)
    outs = [(cm,) + k_lovasz(es_d, perm_d, labd, ignore, cm) for cm in (0, 1)]
    check_lovasz_stage(ck, "2/3 lovasz_softmax", es_d.cpu(), perm_d.cpu(), err, e64, U, lab, ignore,
                       [(cm, l.cpu(), d.cpu()) for cm, l, d in outs])
    _, loss_rm, dp_rm = outs[0]
    got, grad = w_lovasz(pd, labd, ignore)
    ck.true("5 lovasz_softmax: value, to the bit", torch.equal(got.reshape(1), loss_rm))
    ck.true("5 lovasz_softmax: gradient, to the bit", torch.equal(grad, dp_rm * GO))
    ref = float(OM.lovasz_softmax_ref(probas.double(), lab, ignore=-1 if ignore is None else ignore))
    ck.le("6 value vs the independent oracle in double", abs(float(loss_rm.cpu()) - ref), 5e-6 * max(1.0, abs(ref)))
    ck.done()


@pytest.mark.parametrize("p", [1, 257, 2049])
@pytest.mark.parametrize("c", [33, 64])
def test_class_counts_of_the_lovasz_kernels_above_32(p, c):
    """lovasz_finish_kernel's second pass of 32 classes; 2049 rows: more than one tile per class in that pass"""
    _lovasz_only(p, c, 0)


@pytest.mark.parametrize("params", [case(p, c) for c in (5, 20) for p in (1, 63, 255, 256, 257, 1023, 1024, 1025, 2049)])
def test_row_counts(params):
    """less than a wave, either side of the 256-row CE workgroup and of the 1024-element Lovasz tile, several tiles"""
    check_chain(params)


@pytest.mark.parametrize("params", [case(300001, 2, -100), case((1 << 20) - 1, 2, -100), case((1 << 20) - 1, 2, 255),
                                    case(1 << 20, 2, -100), case(1 << 20, 2, 255), case((1 << 20) + 513, 2, 255)])
def test_large_row_counts(params):
    """294 tiles on the int64 labels: a second trip of lovasz_tile_scan_kernel's carry loop; either side of the switch to the byte
    label table at 2^20 rows with ignore = -100 and 255 and such labels present; a ragged last 512-element tile"""
    check_chain(params)


@pytest.mark.parametrize("params", [
    case(1025, 20, 0, labels="absent"), case(1025, 20, None, labels="absent"), case(1025, 20, -100, labels="absent"),
    case(1025, 20, 255, labels="absent"), case(1025, 20, 0, labels="one_class"), case(1025, 20, 255, labels="one_class"),
    case(1025, 20, 0, labels="one_valid"), case(1025, 5, -100, labels="one_valid"), case(1025, 20, 0, labels="block_ignored"),
    case(1025, 5, 255, labels="block_ignored")])
def test_label_cases(params):
    """an absent class, nothing ignored, ignore values outside the classes (the byte table's 255 among them), one class, one row that
    counts, a whole aligned block of 256 rows that does not"""
    check_chain(params)


@pytest.mark.parametrize("params", [case(1025, 20, 0, logits=k) for k in ("randn2", "offset80", "sat30", "tiny")]
                         + [case(2049, 20, 0, logits="dup"), case(257, 5, None, logits="sat30"), case(515, 5, None, logits="dup")])
def test_logit_regimes(params):
    """a common offset of 80 (the max subtraction), saturated rows (errors exactly 0: the sign(0) = 0 rule), near-uniform rows, exact
    ties from a cloud whose second half repeats its first"""
    check_chain(params)


@pytest.mark.parametrize("params", [case(1025, 20, 0, smoothing=s, w=w) for w in ((1.0, 0.7), (1.0, 0.0), (0.0, 1.0))
                                    for s in (0.0, 0.1)] + [case(300, 19, 0, smoothing=0.1, w=(0.0, 1.0)),
                                                            case(300, 7, 0, smoothing=0.0, w=(1.0, 0.0))])
def test_weights_and_smoothing(params):
    check_chain(params)


def test_half_logits_through_losses():
    """half logits: Losses gives the chain on .float(), and its gradient rounded to half"""
    check_chain((1025, 20, 0, "randn2", "absent", 0.1, (1.0, 0.7)), half=True)


@pytest.mark.parametrize("p,c,ignore", [(1025, 20, 0), (257, 5, -100), (1 << 20, 2, 255)])
def test_all_rows_ignored(monkeypatch, p, c, ignore):
    """nothing counts: Lovasz 0 with a zero gradient, ts_ce_lovasz_backward writes no non-finite element (check_chain), and the
    value of Losses is NaN or finite exactly as its tensor form makes it"""
    import taseg_amd.pcseg.loss as LS
    check_chain((p, c, ignore, "randn2", "all_ignored", 0.1, (1.0, 0.7)))
    x, lab = make_inputs(p, c, ignore, "randn2", "all_ignored")
    fused, grad = w_losses(x.to(DEV), lab.to(DEV), ignore, 0.1, 1.0, 0.7)
    monkeypatch.setattr(LS, "_FUSED", False)
    crit = LS.Losses(["CELoss", "LovLoss"], [1.0, 0.7], ignore_index=ignore, label_smoothing=0.1)
    tensor_form = crit(x.to(DEV), lab.to(DEV))
    assert bool(torch.isnan(fused)) == bool(torch.isnan(tensor_form)) and bool(torch.isinf(fused)) == bool(torch.isinf(tensor_form))
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) == 0.0


def test_entry_points_refuse_class_counts_above_their_limit():
    """33 classes at the CE entry points, 65 at ts_lovasz_grad: the documented error code, and nothing is launched (the outputs keep
    what they held)"""
    L, lib = _L()
    p = 300
    for c, which in ((33, "ce"), (65, "lovasz")):
        x, lab = make_inputs(p, c, 0, "randn2", "absent")
        xd, labd = x.to(DEV), lab.to(DEV)
        if which == "ce":
            probas = torch.full((p, c), 7.0, device=DEV)
            err = torch.full((c, p), 7.0, device=DEV)
            part = torch.full(((p + 255) // 256, 3), 7.0, dtype=torch.float64, device=DEV)
            rc = lib.ts_softmax_ce_forward(L.ptr(xd), L.ptr(labd), 0, p, c, L.ptr(probas), L.ptr(err), L.ptr(part), L.stream())
            assert rc == -1 and b"1 .. 32 classes" in lib.ts_last_error()               # TS_ERR_INVALID_ARGUMENT
            out4 = torch.tensor([1.0, 1.0, 0.0, 100.0], device=DEV)
            go = torch.ones(1, device=DEV)
            dl = torch.full((p, c), 7.0, device=DEV)
            pr = torch.softmax(xd, 1)
            rc = lib.ts_ce_lovasz_backward(L.ptr(pr), L.ptr(labd), 0, None, L.ptr(out4), L.ptr(go), p, c, 0.0, 1.0, 1.0, L.ptr(dl),
                                           L.stream())
            assert rc == -1 and b"1 .. 32 classes" in lib.ts_last_error()
            torch.cuda.synchronize()
            assert all(bool((t == 7.0).all()) for t in (probas, err, part, dl))
        else:
            err = k_errors(torch.softmax(xd, 1), labd, 0)
            es, perm = k_sort(err)
            loss = torch.full((1,), 7.0, device=DEV)
            dprob = torch.full((p, c), 7.0, device=DEV)
            ws = L.workspace(lib.ts_lovasz_workspace_bytes(p, c), xd.device)
            rc = lib.ts_lovasz_grad(L.ptr(es), L.ptr(perm), L.ptr(labd), 0, p, c, L.ptr(loss), L.ptr(dprob), 0, L.ptr(ws), ws.numel(),
                                    L.stream())
            assert rc == -1 and b"1 .. 64 classes" in lib.ts_last_error()
            torch.cuda.synchronize()
            assert bool((loss == 7.0).all()) and bool((dprob == 7.0).all())


@pytest.mark.parametrize("c", [33, 65])
def test_wrappers_take_the_tensor_form_above_the_kernels_limits(monkeypatch, c):
    """Losses with 33 classes does not reach the fused CE kernels, lovasz_softmax with 65 does not reach the Lovasz kernels; both
    still give the oracle's value"""
    from oracle import model as OM
    import taseg_amd.pcseg.loss as LS
    from taseg_amd.pcseg.loss import lovasz as LV

    def refuse(*a, **k):
        raise AssertionError("the fused form was taken above its class limit")
    monkeypatch.setattr(LS._CeLovasz, "apply", refuse)
    if c > 64:
        monkeypatch.setattr(LV._LovaszPresent, "apply", refuse)
    p = 1025
    x, lab = make_inputs(p, c, 0, "randn2", "absent")
    crit = LS.Losses(["CELoss", "LovLoss"], [1.0, 1.0], ignore_index=0, label_smoothing=0.1)
    a = x.to(DEV).requires_grad_()
    got = crit(a, lab.to(DEV))
    got.backward()
    ref = float(OM.loss_ce_lovasz(x.double(), lab, ignore=0, label_smoothing=f32(0.1)))
    assert abs(float(got) - ref) <= 5e-6 * max(1.0, abs(ref))
    assert bool(torch.isfinite(a.grad).all())
    lov = LV.lovasz_softmax(torch.softmax(x, 1).to(DEV), lab.to(DEV), ignore=0)
    ref = float(OM.lovasz_softmax_ref(torch.softmax(x, 1).double(), lab, ignore=0))
    assert abs(float(lov) - ref) <= 5e-6 * max(1.0, abs(ref))
