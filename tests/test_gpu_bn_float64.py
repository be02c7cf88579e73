"""The sparse BatchNorm (+ residual) (+ ReLU) kernels of csrc/bn.hip against float64, at the edges of their layout.

Every output of the training entry points - y, grad x, grad residual, grad weight, grad bias, the saved mean / invstd, the running
statistics and the batch counter - is compared with `bn_ref64`, a float64 reference spelled out with tensor ops (no
functional.batch_norm, no autograd; itself checked against nn.BatchNorm1d in double under autograd on the CPU, the one test of this
file that needs no device).  fp32 and half storage, through `batch_norm_act_train` (one process) and through the SyncBatchNorm halves
run as two simulated ranks with unequal row counts: their double packs added on the device, which is all the all-reduce does.

Bars.  u32 = 2^-24, u16 = 2^-11.  A sum of k float additions of terms t_i is within k u32 sum |t_i| of the exact sum.  bn.hip
documents the layout of the reductions: a launch is cut into <= 512 slices of at least 32 rows, a slice's length is a whole number of
passes; one thread holds 4 (half: 8) channels of a row, so a pass of a 256-thread workgroup covers rpp = 256 // (c / 4) rows
(256 // (c / 8)); a lane adds its rows of the slice in float, the rpp lanes of a channel are added in float, the slices in double.
The longest chain of float additions is therefore

    rows = ceil(max(ceil(n / 512), 32) / rpp) * rpp          rows per slice
    LAMBDA(n, c) = rows / rpp  +  rpp  +  8                  rows a lane adds + lanes added per workgroup + elementwise operations

(8: the product inside the sum, x - mean, * invstd, * weight, + bias, + residual, the two conversions of a statistic to float).  It
is evaluated from n and c alone.  With S the same expression evaluated on absolute values

    an fp32 result (elementwise or a sum)    |got - ref| <= LAMBDA u32 S
    a half result                            |got - ref| <= u16 |ref| + LAMBDA u32 S + 2^-25      (2^-25: below half's normal range)

S of the statistics: mean -> E|x|;  var -> E[x^2] + mean^2 (the kernels form E[x^2] - mean^2; var is recovered from the saved float
invstd as 1 / invstd^2 - eps, whose own rounding, 2 u32 (var + eps), is added to the bar: it is the observation's, not the
kernel's).  invstd = (var + eps)^-1/2 inherits var's error through its derivative: S_invstd = invstd^3 S_var / 2 - the conditioning
of the one-pass variance, (1 + 2 kappa^2) / 2 relative to invstd with kappa = |mean| / std.  Every later expression carries that
term: S_y = (|x| + E|x|) invstd |w| + |x - mean| S_invstd |w| + |b| + |res|, and likewise for grad weight and grad x (bn_ref64
spells them out).  At kappa = 1/4 the term is half the first one; at kappa = 32 it is most of the bar of y and grad x, which is
what a one-pass variance costs, while the bars of mean, var, grad bias and the running statistics stay at LAMBDA u32 of their sums
- and those are what a lost row moves.  A correct kernel sits one to two orders of magnitude below these worst-case bars (rounding
errors add like a random walk).  On a channel that holds one value the linearisation has no force (var = 0: S_invstd / invstd ~ S_var
/ eps): there invstd is held by the bar of var and, for the value 3.0 whose sums are exact in any order, y must equal bias (+
residual) to the bit.

Regimes (explicit seeds): benign randn * 2 + 0.5; offset, channel means +-8 (sign alternating) with std 1/4 (kappa = 32) and
gradients with a mean of half their spread - every sum is coherent, a row lost from a reduction moves mean / grad bias by 1/n of the
sum, far over LAMBDA u32 at the small shapes; constant channels (3.0 and 0.1 in every row); n = 1 and n = 2, where the finish kernels
clamp the variance at 0 from below and keep the biased variance for running_var when the total is 1 (one row: the one-pass variance
is fl(x^2) - x^2, not 0 - invstd may sit below eps^-1/2 by the bar of var, never above it).

The ReLU's derivative in the reference is taken from the kernel's own output (`relu_from`): the forward check certifies that output
and torch's ReLU backward is defined on the output too, so no element is left out of any comparison.  For half storage that is the
sign of the STORED value: a positive fp32 value of at most 2^-25 is stored as a half zero and passes no gradient.  (The kernel once
took the bit from the fp32 value; two of the 134 M elements of the 131 200 x 1 024 case, residual and all, fell into that gap and
moved grad bias / n, so every row of their channels left the bar.  `test_half_relu_mask_follows_the_stored_value` builds such an
element on purpose.)  Every case runs twice and must produce the same bits.

The module carries no `pytestmark`: the reference's own test runs without a device.  Every other test is marked gpu by name, and
`test_every_device_test_of_this_module_is_marked_gpu` fails in the CPU suite if one is added without the mark.
"""
import math

import pytest
import torch

from oracle.bn64 import LAMBDA as _lam, bn_ref64, running_ref64

gpu = pytest.mark.gpu

DEV = "cuda"
U32, U16, SUB = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the kernels take eps and momentum as floats
GRID_CAP = (1 << 16) * 256                                  # vectors one trip of the elementwise kernels covers (bn.hip's launches)
CONST3, CONST01 = (1, 5), (2, -1)                           # channels of the constant regime: 3.0 and 0.1 in every row


# ------------------------------------------------------------------------------------------------------------------ reference

@pytest.mark.parametrize("n,c", [(257, 8), (40, 20)])
@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, True), (True, False)])
def test_bn_ref64_matches_double_batchnorm1d_autograd(n, c, with_res, relu):
    """the reference itself (on the CPU): bn_ref64 and running_ref64 against nn.BatchNorm1d in double + add + relu under autograd"""
    g = torch.Generator().manual_seed(100 + n + c)
    x = (torch.randn(n, c, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_()
    res = torch.randn(n, c, generator=g, dtype=torch.float64).requires_grad_() if with_res else None
    gy = torch.randn(n, c, generator=g, dtype=torch.float64) + 0.5
    bn = torch.nn.BatchNorm1d(c, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y = bn(x)
    if with_res:
        y = y + res
    if relu:
        y = torch.relu(y)
    leaves = (x, res, bn.weight, bn.bias) if with_res else (x, bn.weight, bn.bias)
    grads = list(torch.autograd.grad(y, leaves, gy))
    if not with_res:
        grads.insert(1, None)
    (ry, rgx, rgres, rgw, rgb, mean, var), (_, _, _, _, _, smean, svar) = bn_ref64(
        x.detach(), None if res is None else res.detach(), bn.weight.detach(), bn.bias.detach(), relu, 1e-5, gy)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)       # noqa: E731
    close(ry, y.detach())
    close(rgx, grads[0])
    assert (rgres is None) == (not with_res)
    if with_res:
        close(rgres, grads[1])
    close(rgw, grads[2])
    close(rgb, grads[3])
    rm, rv, _, _ = running_ref64(rm0, rv0, mean, var, smean, svar, n, 0.1)
    close(rm, bn.running_mean)
    close(rv, bn.running_var)
    assert int(bn.num_batches_tracked) == 1
    bn(x)                                                       # a second pass over the same batch
    rm, rv, _, _ = running_ref64(rm0, rv0, mean, var, smean, svar, n, 0.1, passes=2)
    close(rm, bn.running_mean)
    close(rv, bn.running_var)


# ------------------------------------------------------------------------------------------------------------------ helpers

def _randn(shape, seed, scale=1.0, shift=0.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


def _rand(shape, seed, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV) + shift


def _check(name, got, ref, s, lam, extra=0.0):
    """|got - ref| <= lam u32 S (+ extra) elementwise, + u16 |ref| + 2^-25 for a half result; prints and returns the worst err / bar"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bar = lam * U32 * s + extra
    if got.dtype == torch.float16:
        bar = bar + U16 * ref.abs() + SUB
    ok = err <= bar                                            # (a NaN or an infinity in `got` compares false)
    worst = float((err / bar.clamp_min(1e-300)).max())
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:4].tolist()
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bar, worst err/bar {worst:.3g}, "
                             f"e.g. at {bad}")
    print(f"{name}: worst err/bar {worst:.3g}")
    return worst


def _twice(fn):
    """run a case twice: same bits (every kernel of the family is run-to-run deterministic)"""
    a, b = fn(), fn()
    for i, (p, q) in enumerate(zip(a, b)):
        assert p is None and q is None or torch.equal(p, q), f"output {i} differs between two runs"
    return a


def _poison(like, count):
    """fill and release `count` buffers of `like`'s size with NaN: the allocator hands these blocks to the outputs allocated next, so an
    element a kernel does not write reads as NaN instead of what an earlier run left there"""
    for t in [torch.full_like(like, float("nan")) for _ in range(count)]:
        del t


def _inputs(n, c, regime, dtype, seed, residual):
    """x, gy, residual, weight, bias, running_mean, running_var of a regime"""
    if regime == "offset":
        sign = torch.where(torch.arange(c, device=DEV) % 2 == 0, 8.0, -8.0)
        x = (_randn((n, c), seed, scale=0.25) + sign).to(dtype)
        gy = _randn((n, c), seed + 1, shift=0.5, dtype=dtype)
    else:
        x = _randn((n, c), seed, scale=2.0, shift=0.5, dtype=dtype)
        gy = _randn((n, c), seed + 1, dtype=dtype)
    if regime == "const":
        for ch in CONST3:
            x[:, ch] = 3.0
        for ch in CONST01:
            x[:, ch] = 0.1
    res = _randn((n, c), seed + 2, dtype=dtype) if residual else None
    weight = _rand((c,), seed + 3, shift=0.5) * torch.where(torch.arange(c, device=DEV) % 3 == 0, -1.0, 1.0)
    bias = _randn((c,), seed + 4)
    return x, gy, res, weight, bias, _randn((c,), seed + 5), _rand((c,), seed + 6, shift=0.5)


def _relu_fp32(bias, res, relu, dtype):
    """what the kernels give where x - mean is exactly 0: bias (+ residual) in fp32, the ReLU, one rounding to the storage type"""
    v = bias if res is None else bias + res.float()
    return (v.clamp_min(0.0) if relu else v).to(dtype)


# ------------------------------------------------------------------------------------------------------------------ one process

_FLAGS = {"relu": (True, False), "res+relu": (True, True), "res": (False, True), "plain": (False, False)}


def _cases(half):
    w = {4: 8, 20: 24}.get if half else (lambda c, d: c)           # the two narrow widths of each storage type
    c4, c20 = w(4, 4), w(20, 20)
    cases = [
        # every row count at c = 32 and c = 96
        (1, 32, "benign", "res+relu"), (2, 32, "benign", "relu"), (31, 32, "offset", "res+relu"), (33, 32, "offset", "relu"),
        (33, 32, "const", "res+relu"), (16384, 32, "offset", "res+relu"), (16385, 32, "benign", "relu"),
        (16385, 32, "offset", "res+relu"), (16385, 32, "offset", "res"), (16385, 32, "const", "relu"),
        (16385, 32, "offset", "plain"), (180001, 32, "offset", "res+relu"),
        (1, 96, "benign", "relu"), (2, 96, "benign", "res+relu"), (31, 96, "offset", "relu"), (33, 96, "offset", "res+relu"),
        (16384, 96, "offset", "relu"), (16384, 96, "benign", "res+relu"), (16384, 96, "offset", "res"),
        (16384, 96, "const", "res+relu"), (16385, 96, "benign", "res+relu"), (180001, 96, "benign", "res+relu"),
        # every other width at a small and a mid row count
        (33, c4, "offset", "res+relu"), (16385, c4, "benign", "relu"), (2, c4, "benign", "res"),
        (31, c20, "offset", "relu"), (16384, c20, "offset", "res+relu"),
        (33, 256, "offset", "res+relu"), (16384, 256, "benign", "res+relu"),
        (33, 1024, "offset", "relu"), (33, 1024, "offset", "res+relu"), (33, 1024, "benign", "res"), (1, 1024, "benign", "res+relu"),
        (16384, 1024, "offset", "res+relu"),
        # more vectors than one trip of the elementwise kernels' grid covers
        (GRID_CAP * (8 if half else 4) // 1024 + (128 if half else 64), 1024, "benign", "res+relu"),
    ]
    return [pytest.param(n, c, regime, flags, id=f"{n}x{c}-{regime}-{flags}") for n, c, regime, flags in cases]


def _single(dtype, n, c, regime, flags):
    from taseg_amd.torchsparse.nn.batchnorm import batch_norm_act_train, batch_norm_train
    half = dtype == torch.float16
    relu, residual = _FLAGS[flags]
    # momentum 0.02 at the bench-scale c = 32 case, two consecutive passes at (33, 96)
    momentum = float(torch.tensor(0.02 if (n, c) == (180001, 32) else 0.1, dtype=torch.float32))
    passes = 2 if (n, c, regime) == (33, 96, "offset") else 1
    x, gy, res, weight, bias, rm0, rv0 = _inputs(n, c, regime, dtype, 1000 * (c % 97) + n % 1000 + (7 if half else 0), residual)
    tag = f"{'half' if half else 'fp32'} {n}x{c} {regime} {flags}"
    if n * c // (8 if half else 4) > GRID_CAP // 2:
        assert n * c // (8 if half else 4) > GRID_CAP, "the large case must take a second trip of the grid-stride loop"

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        xr, wr, br = x.detach().requires_grad_(), weight.detach().requires_grad_(), bias.detach().requires_grad_()
        rr = res.detach().requires_grad_() if residual else None
        _poison(x, 1)
        for _ in range(passes):
            if flags == "plain":
                y = batch_norm_train(xr, wr, br, rm, rv, momentum, EPS, num_batches_tracked=nbt)
            else:
                y = batch_norm_act_train(xr, wr, br, rm, rv, momentum, EPS, relu=relu, residual=rr, num_batches_tracked=nbt)
        saved = y.grad_fn.saved_tensors                                      # x, weight, mean, invstd, mask
        mean, invstd = saved[2].clone(), saved[3].clone()
        _poison(x, 2)
        if residual:
            gx, gres, gw, gb = torch.autograd.grad(y, (xr, rr, wr, br), gy)
        else:
            (gx, gw, gb), gres = torch.autograd.grad(y, (xr, wr, br), gy), None
        return y.detach(), gx, gres, gw, gb, mean, invstd, rm, rv, nbt
    y, gx, gres, gw, gb, mean, invstd, rm, rv, nbt = _twice(run)
    assert y.dtype == gx.dtype == dtype and gw.dtype == gb.dtype == mean.dtype == invstd.dtype == torch.float32
    assert int(nbt) == passes
    assert bool(torch.isfinite(invstd).all()) and bool((invstd > 0).all())
    lam = _lam(n, c, half)
    (ry, rgx, rgres, rgw, rgb, rmean, rvar), (sy, sgx, sgres, sgw, sgb, smean, svar) = bn_ref64(
        x, res, weight, bias, relu, EPS, gy, relu_from=y if relu else None)
    _check(f"{tag}: y", y, ry, sy, lam)
    del ry, sy
    _check(f"{tag}: grad x", gx, rgx, sgx, lam)
    if regime == "const":
        # on a channel of 3.0 every sum is exact in any order, so var = 0 and invstd = (float)(1 / sqrt(eps)) to the bit: grad x is
        # held WITHOUT the conditioning term |inner| S_invstd |w| = |grad x| S_var / (2 (var + eps)), which would swallow it there
        ch = list(CONST3)
        tight = sgx[:, ch] - rgx[:, ch].abs() * (0.5 * svar[ch] / (rvar[ch] + EPS))
        _check(f"{tag}: grad x, channels of 3.0", gx[:, ch], rgx[:, ch], tight, lam)
    del rgx, sgx
    if residual:
        _check(f"{tag}: grad residual", gres, rgres, sgres, lam)
        assert torch.equal(gres, gy * (y > 0) if relu else gy)               # a masked copy: exact
        del rgres, sgres
    _check(f"{tag}: grad weight", gw, rgw, sgw, lam)
    _check(f"{tag}: grad bias", gb, rgb, sgb, lam)
    _check(f"{tag}: mean", mean, rmean, smean, lam)
    _check(f"{tag}: var = 1 / invstd^2 - eps", 1.0 / invstd.double().square() - EPS, rvar, svar, lam, extra=2 * U32 * (rvar + EPS))
    erm, erv, srm, srv = running_ref64(rm0, rv0, rmean, rvar, smean, svar, n, momentum, passes)
    _check(f"{tag}: running_mean", rm, erm, srm, lam)
    _check(f"{tag}: running_var", rv, erv, srv, lam)
    if regime == "const":
        # a channel of 3.0: every sum is exact in any order, so mean = 3, var = 0, invstd = (float)(1 / sqrt(eps)), x - mean = 0 and
        # y = bias (+ residual), all to the bit (the bar of var, LAMBDA u32 * 18 > eps, would let invstd be off by a factor there);
        # the channels of 0.1, whose sums round, are held by the bars above
        for ch in CONST3:
            assert float(mean[ch]) == 3.0
            assert float(invstd[ch]) == float(torch.tensor(1.0 / math.sqrt(EPS), dtype=torch.float32)), (ch, float(invstd[ch]))
            assert torch.equal(y[:, ch], _relu_fp32(bias[ch].expand(n), None if res is None else res[:, ch], relu, dtype)), ch
    if n == 1:
        # one row (nn.BatchNorm1d refuses it): mean = the row and y = bias (+ residual) to the bit; the variance, fl(x^2) - x^2 in the
        # one-pass form, is clamped at 0 from below - invstd never exceeds (float)(1 / sqrt(eps)) and sits within the bar of var
        # checked above - and running_var takes var itself, not var * n / (n - 1): finite, within its bar of (1 - momentum) rv0
        assert torch.equal(mean, x[0].float())
        assert bool((invstd <= torch.full_like(invstd, 1.0 / math.sqrt(EPS))).all())
        assert torch.equal(y[0], _relu_fp32(bias, None if res is None else res[0], relu, dtype))
        assert bool(torch.isfinite(rv).all())


@gpu
@pytest.mark.parametrize("n,c,regime,flags", _cases(False))
def test_bn_act_train_fp32_vs_float64(n, c, regime, flags):
    """batch_norm_act_train / batch_norm_train on fp32 rows: every output against bn_ref64 within LAMBDA u32 S"""
    _single(torch.float32, n, c, regime, flags)


@gpu
@pytest.mark.parametrize("n,c,regime,flags", _cases(True))
def test_bn_act_train_half_vs_float64(n, c, regime, flags):
    """the same on half rows: the reference reads the exact half values; y, grad x and grad residual carry one half rounding"""
    _single(torch.float16, n, c, regime, flags)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
def test_half_relu_mask_follows_the_stored_value(dtype):
    """a pre-activation of exactly 2^-26 (a channel of 3.0, so x - mean = 0, bias 2^-26, a zero residual): positive in fp32, a zero
    once stored as half.  Half storage: y = 0 there and NO gradient passes - grad residual, grad bias and grad weight of the channel
    are 0, grad x is the float64 value without that row's dy.  fp32 storage: y = 2^-26 and dy passes whole.  One more channel with
    bias 2^-24, half's smallest subnormal, keeps its gradient in both."""
    from taseg_amd.torchsparse.nn.batchnorm import batch_norm_act_train
    n, c, tiny, small = 33, 32, 1, 5
    half = dtype == torch.float16
    x, gy, _, weight, bias, rm0, rv0 = _inputs(n, c, "const", dtype, 4242, False)
    res = torch.zeros_like(x)
    bias[tiny], bias[small] = 2.0 ** -26, 2.0 ** -24

    def run():
        xr, rr = x.detach().requires_grad_(), res.detach().requires_grad_()
        wr, br = weight.detach().requires_grad_(), bias.detach().requires_grad_()
        y = batch_norm_act_train(xr, wr, br, rm0.clone(), rv0.clone(), 0.1, EPS, relu=True, residual=rr)
        return (y.detach(),) + torch.autograd.grad(y, (xr, rr, wr, br), gy)
    y, gx, gres, gw, gb = _twice(run)
    assert torch.equal(y[:, small], torch.full_like(y[:, small], 2.0 ** -24)) and torch.equal(gres[:, small], gy[:, small])
    if half:
        assert not bool(y[:, tiny].any()) and not bool(gres[:, tiny].any()) and float(gb[tiny]) == 0.0 and float(gw[tiny]) == 0.0
    else:
        assert torch.equal(y[:, tiny], torch.full_like(y[:, tiny], 2.0 ** -26)) and torch.equal(gres[:, tiny], gy[:, tiny])
    (_, rgx, rgres, _, rgb, _, rvar), (_, sgx, _, _, sgb, _, svar) = bn_ref64(x, res, weight, bias, True, EPS, gy, relu_from=y)
    assert torch.equal(gres, gy * (y > 0))
    lam = _lam(n, c, half)
    _check(f"mask {'half' if half else 'fp32'}: grad bias", gb, rgb, sgb, lam)
    ch = [tiny, small]
    tight = sgx[:, ch] - rgx[:, ch].abs() * (0.5 * svar[ch] / (rvar[ch] + EPS))
    _check(f"mask {'half' if half else 'fp32'}: grad x of the two channels", gx[:, ch], rgx[:, ch], tight, lam)


def test_every_device_test_of_this_module_is_marked_gpu():
    """this module has no module-level mark (its reference test runs on the CPU): a test added without @gpu would run, and fail,
    in the CPU suite - this one fails first and says why"""
    import sys
    cpu = {"test_bn_ref64_matches_double_batchnorm1d_autograd", "test_every_device_test_of_this_module_is_marked_gpu"}
    for name, fn in vars(sys.modules[__name__]).items():
        if name.startswith("test_") and callable(fn) and name not in cpu:
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not marked gpu"


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
def test_bn_act_train_refuses_more_than_1024_channels(dtype):
    """c = 1028 is past the documented maximum of the fp32 kernels (and no multiple of 8 for the half ones): the library's error, and
    nothing launched - the counter and the running buffers are the ones the finish kernel would have written"""
    from taseg_amd._lib import BackendError
    from taseg_amd.torchsparse.nn.batchnorm import batch_norm_act_train
    c = 1028
    x = _randn((8, c), 1, dtype=dtype).requires_grad_()
    weight, bias, rm, rv = _rand((c,), 2, shift=0.5), _randn((c,), 3), _randn((c,), 4), _rand((c,), 5, shift=0.5)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    with pytest.raises(BackendError, match=r"need N > 0 and C a multiple of (4, <= 1024|8, <= 2048)"):
        batch_norm_act_train(x, weight, bias, rm, rv, 0.1, EPS, relu=True, num_batches_tracked=nbt)
    torch.cuda.synchronize()
    assert int(nbt) == 0 and torch.equal(rm, rm0) and torch.equal(rv, rv0)


@gpu
def test_bn_invstd_error_at_kappa_128_is_printed():
    """not asserted: the worst relative error of invstd with channel means 128 x the standard deviation (32 +- 1/4), the figure the
    next change to the reductions is compared with (the one-pass variance loses kappa^2 u32 there)"""
    from taseg_amd.torchsparse.nn.batchnorm import batch_norm_train
    worst = {}
    for dtype in (torch.float32, torch.float16):
        for n, c in ((33, 32), (16385, 32), (16384, 96), (180001, 32)):
            x = (_randn((n, c), 128 + n % 100 + c, scale=0.25) + 32.0).to(dtype)
            weight, bias = torch.ones(c, device=DEV).requires_grad_(), torch.zeros(c, device=DEV)
            y = batch_norm_train(x, weight, bias, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), 0.1, EPS)
            invstd = y.grad_fn.saved_tensors[3].double()
            ref = (x.double().var(0, unbiased=False) + EPS).rsqrt()
            worst[(str(dtype).split(".")[1], n, c)] = float(((invstd - ref).abs() / ref).max())
    for key, value in worst.items():
        print(f"kappa = 128, {key}: invstd relative error {value:.3g}")
    print(f"kappa = 128: worst invstd relative error {max(worst.values()):.3g}")


# ------------------------------------------------------------------------------------------------------------------ SyncBatchNorm halves

def _sync(dtype, xs, ress, gys, weight, bias, rm0, rv0, momentum, relu):
    """the SyncBatchNorm recipe of torchsparse/nn/batchnorm.py over simulated ranks: per-rank statistics -> the [2C + 1] double packs
    added -> ts_bn_finalize per rank with total_dev = the summed count and total_host = the rank's own -> apply; backward the same with
    the [2C] sums.  Returns per-rank lists."""
    from taseg_amd import _lib as L
    lib = L.load()
    half = dtype == torch.float16
    sfx = "_f16" if half else ""
    c = xs[0].shape[1]
    per = 8 if half else 4
    ws = L.workspace(lib.ts_bn_train_workspace_bytes(c), xs[0].device)
    packs = []
    for x in xs:
        pack = torch.empty(2 * c + 1, dtype=torch.float64, device=DEV)
        L.check(getattr(lib, "ts_bn_sync_stats" + sfx)(L.ptr(x), x.shape[0], c, L.ptr(pack), L.ptr(ws), ws.numel(), L.stream()),
                "ts_bn_sync_stats" + sfx)
        packs.append(pack)
    assert [float(p[2 * c]) for p in packs] == [float(x.shape[0]) for x in xs]
    total = sum(packs[1:], packs[0].clone())                                       # the all-reduce
    total_dev = total[2 * c:]
    out = {k: [] for k in ("y", "gx", "gres", "gw", "gb", "mean", "invstd", "rm", "rv")}
    masks, sums = [], []
    for x, res in zip(xs, ress):
        n = x.shape[0]
        stats = torch.empty((2, c), dtype=torch.float32, device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        L.check(lib.ts_bn_finalize(L.ptr(total), L.ptr(total_dev), float(n), c, EPS, momentum, L.ptr(rm), L.ptr(rv), L.ptr(stats[0]),
                                   L.ptr(stats[1]), L.stream()), "ts_bn_finalize")
        _poison(x, 1)
        y = torch.empty_like(x)
        mask = torch.empty(n * (c // per), dtype=torch.uint8, device=DEV) if relu else None
        L.check(getattr(lib, "ts_bn_act_forward" + sfx)(L.ptr(x), L.ptr(res), L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(weight),
                                                        L.ptr(bias), n, c, 1 if relu else 0, L.ptr(y), L.ptr(mask), L.stream()),
                "ts_bn_act_forward" + sfx)
        masks.append(mask)
        for k, v in (("y", y), ("mean", stats[0]), ("invstd", stats[1]), ("rm", rm), ("rv", rv)):
            out[k].append(v)
    for i, (x, gy) in enumerate(zip(xs, gys)):
        s = torch.empty((2, c), dtype=torch.float64, device=DEV)
        gwb = torch.empty((2, c), dtype=torch.float32, device=DEV)
        L.check(getattr(lib, "ts_bn_sync_backward_reduce" + sfx)(
            L.ptr(gy), L.ptr(masks[i]), L.ptr(x), L.ptr(out["mean"][i]), L.ptr(out["invstd"][i]), x.shape[0], c, L.ptr(s),
            L.ptr(gwb[0]), L.ptr(gwb[1]), L.ptr(ws), ws.numel(), L.stream()), "ts_bn_sync_backward_reduce" + sfx)
        sums.append(s)
        out["gw"].append(gwb[0])
        out["gb"].append(gwb[1])
    allsum = sum(sums[1:], sums[0].clone())                                        # the all-reduce
    for i, (x, gy, res) in enumerate(zip(xs, gys, ress)):
        n = x.shape[0]
        _poison(x, 2)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if res is not None else None
        args = (L.ptr(gy), L.ptr(masks[i]), L.ptr(x), L.ptr(out["mean"][i]), L.ptr(out["invstd"][i]), L.ptr(weight), L.ptr(allsum),
                L.ptr(total_dev), float(n), n, c, L.ptr(gx), L.ptr(gres))
        if half:
            L.check(lib.ts_bn_act_backward_f16(*args, L.ptr(ws), ws.numel(), L.stream()), "ts_bn_act_backward_f16")
        else:
            L.check(lib.ts_bn_act_backward(*args, L.stream()), "ts_bn_act_backward")
        out["gx"].append(gx)
        out["gres"].append(gres)
    torch.cuda.synchronize()
    return out


_BIG = GRID_CAP * 4 // 1024 + 64                            # fp32 rows of 1024 channels past one trip of the elementwise grid
_SYNC_CASES = [pytest.param(dt, n, c, split, regime, id=f"{'half' if dt == torch.float16 else 'fp32'}-{split}+{n - split}x{c}-{regime}")
               for dt in (torch.float32, torch.float16)
               for n, c, split, regime in ((20011, 96, 13007, "benign"), (20011, 96, 13007, "offset"), (33, 32, 32, "benign"),
                                           (33, 32, 32, "offset"))]
# (the half elementwise kernels of this path are the single-process ones, which take their second trip above; the fp32 backward,
# bn_act_bwd_kernel, has no other caller)
_SYNC_CASES.append(pytest.param(torch.float32, _BIG, 1024, _BIG - 10, "benign", id="fp32-grid-cap"))


@gpu
@pytest.mark.parametrize("dtype,n,c,split,regime", _SYNC_CASES)
def test_syncbn_halves_as_two_unequal_ranks_vs_float64(dtype, n, c, split, regime):
    """two simulated ranks holding `split` and n - split rows (13007 + 7004, 32 + 1; one rank past the grid cap of the elementwise
    kernels): concatenated, every output meets the bars of bn_ref64 over the WHOLE matrix - only with total_dev, the summed count, does
    the mean come out - the per-rank grad weight / grad bias sum to the reference's, and both ranks hold the same statistics"""
    half = dtype == torch.float16
    momentum = float(torch.tensor(0.1, dtype=torch.float32))
    x, gy, res, weight, bias, rm0, rv0 = _inputs(n, c, regime, dtype, 5000 + n % 1000 + c + (7 if half else 0), True)
    cut = lambda t: [t[:split], t[split:]]                                          # noqa: E731  (row blocks: contiguous, 16-byte aligned)
    tag = f"sync {'half' if half else 'fp32'} {split}+{n - split} x {c} {regime}"

    def run():
        o = _sync(dtype, cut(x), cut(res), cut(gy), weight, bias, rm0, rv0, momentum, True)
        assert all(torch.equal(o[k][0], o[k][1]) for k in ("mean", "invstd", "rm", "rv")), "the ranks disagree on the statistics"
        return (torch.cat(o["y"]), torch.cat(o["gx"]), torch.cat(o["gres"]), o["gw"][0], o["gw"][1], o["gb"][0], o["gb"][1],
                o["mean"][0], o["invstd"][0], o["rm"][0], o["rv"][0])
    y, gx, gres, gw0, gw1, gb0, gb1, mean, invstd, rm, rv = _twice(run)
    lam = max(_lam(split, c, half), _lam(n - split, c, half))                        # each rank's own chains; doubles across ranks
    assert bool(torch.isfinite(invstd).all())
    (ry, rgx, rgres, rgw, rgb, rmean, rvar), (sy, sgx, sgres, sgw, sgb, smean, svar) = bn_ref64(
        x, res, weight, bias, True, EPS, gy, relu_from=y)
    _check(f"{tag}: y", y, ry, sy, lam)
    del ry, sy
    _check(f"{tag}: grad x", gx, rgx, sgx, lam)
    del rgx, sgx
    _check(f"{tag}: grad residual", gres, rgres, sgres, lam)
    assert torch.equal(gres, gy * (y > 0))
    del rgres, sgres
    _check(f"{tag}: grad weight (ranks summed)", (gw0.double() + gw1.double()).float(), rgw, sgw, lam)
    _check(f"{tag}: grad bias (ranks summed)", (gb0.double() + gb1.double()).float(), rgb, sgb, lam)
    _check(f"{tag}: mean", mean, rmean, smean, lam)
    _check(f"{tag}: var = 1 / invstd^2 - eps", 1.0 / invstd.double().square() - EPS, rvar, svar, lam, extra=2 * U32 * (rvar + EPS))
    erm, erv, srm, srv = running_ref64(rm0, rv0, rmean, rvar, smean, svar, n, momentum)
    _check(f"{tag}: running_mean", rm, erm, srm, lam)
    _check(f"{tag}: running_var", rv, erv, srv, lam)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
@pytest.mark.parametrize("total_on_device", [True, False])
def test_syncbn_finalize_with_a_total_of_one(dtype, total_on_device):
    """bn_finalize_kernel on a single row in all, the total read from the pack or handed over by the host: mean = the row, the
    variance (fl(x^2) - x^2 here) clamped at 0 from below so invstd <= (float)(1 / sqrt(eps)), within the bar of var; running_var
    keeps var itself where var * n / (n - 1) has no value"""
    from taseg_amd import _lib as L
    lib = L.load()
    c = 32
    momentum = float(torch.tensor(0.1, dtype=torch.float32))
    x = _randn((1, c), 77, scale=2.0, shift=0.5, dtype=dtype)
    rm0, rv0 = _randn((c,), 78), _rand((c,), 79, shift=0.5)
    rm, rv = rm0.clone(), rv0.clone()
    ws = L.workspace(lib.ts_bn_train_workspace_bytes(c), x.device)
    pack = torch.empty(2 * c + 1, dtype=torch.float64, device=DEV)
    sfx = "_f16" if dtype == torch.float16 else ""
    L.check(getattr(lib, "ts_bn_sync_stats" + sfx)(L.ptr(x), 1, c, L.ptr(pack), L.ptr(ws), ws.numel(), L.stream()), "ts_bn_sync_stats")
    stats = torch.empty((2, c), dtype=torch.float32, device=DEV)
    total_dev = pack[2 * c:] if total_on_device else None
    L.check(lib.ts_bn_finalize(L.ptr(pack), L.ptr(total_dev), 1.0, c, EPS, momentum, L.ptr(rm), L.ptr(rv), L.ptr(stats[0]),
                               L.ptr(stats[1]), L.stream()), "ts_bn_finalize")
    assert torch.equal(pack[:c], x[0].double()) and torch.equal(pack[c:2 * c], x[0].float().square().double()) and float(pack[2 * c]) == 1.0
    assert torch.equal(stats[0], x[0].float())
    assert bool((stats[1] <= torch.full_like(stats[1], 1.0 / math.sqrt(EPS))).all()) and bool((stats[1] > 0).all())
    lam = _lam(1, c, dtype == torch.float16)
    zero, svar = torch.zeros(c, dtype=torch.float64, device=DEV), 2 * x[0].double().square()
    _check("finalize, total 1: var = 1 / invstd^2 - eps", 1.0 / stats[1].double().square() - EPS, zero, svar, lam, extra=2 * U32 * EPS)
    erm, erv, srm, srv = running_ref64(rm0, rv0, x[0].double(), zero, x[0].double().abs(), svar, 1, momentum)
    _check("finalize, total 1: running_mean", rm, erm, srm, lam)
    _check("finalize, total 1: running_var", rv, erv, srv, lam)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
@pytest.mark.parametrize("n,c,residual", [(33, 96, False), (16385, 32, True)])
def test_bn_act_forward_eval_style_vs_float64(dtype, n, c, residual):
    """ts_bn_act_forward with mask = NULL and relu = 1 on given statistics (running_mean and 1 / sqrt(running_var + eps)), the call
    ts_conv_block_eval issues: relu((x - mean) invstd w + b [+ residual]) within 8 u32 S (elementwise operations only)"""
    from taseg_amd import _lib as L
    lib = L.load()
    half = dtype == torch.float16
    x, _, res, weight, bias, rm, rv = _inputs(n, c, "offset", dtype, 9000 + n % 1000 + c, residual)
    invstd = (rv + EPS).rsqrt()
    mean = rm + torch.where(torch.arange(c, device=DEV) % 2 == 0, 8.0, -8.0)

    def run():
        _poison(x, 1)
        y = torch.empty_like(x)
        L.check(getattr(lib, "ts_bn_act_forward" + ("_f16" if half else ""))(
            L.ptr(x), L.ptr(res), L.ptr(mean), L.ptr(invstd), L.ptr(weight), L.ptr(bias), n, c, 1, L.ptr(y), None, L.stream()),
            "ts_bn_act_forward")
        return (y,)
    (y,) = _twice(run)
    m64, i64, w64, b64 = mean.double(), invstd.double(), weight.double(), bias.double()
    ref = (x.double() - m64) * i64 * w64 + b64
    s = (x.double().abs() + m64.abs()) * i64 * w64.abs() + b64.abs()
    if residual:
        ref, s = ref + res.double(), s + res.double().abs()
    _check(f"eval {'half' if half else 'fp32'} {n}x{c}: y", y, ref.clamp_min(0.0), s, 8)
