"""csrc/fid.hip (the interpolation decoder and its adjoint) and the BatchNorm -> residual -> LeakyReLU calls of csrc/bn.hip on the GPU,
against tests/fid_ref.py.

Decoder, at four shapes (a level of one row; odd sizes with non-dyadic scales; `out == 1` rows with a one-pixel level; the model's 16 x
64) and three widths, float and half: the forward equals the numpy restatement of the header's rule bit for bit (half: after the one
rounding) and lies within the derived bar of the float64 evaluation; the level maps, when asked for, equal their slices of cat; the
backward equals the restatement's ordered sum bit for bit with and without the three extra gradients, lies within its bar of float64,
and gives the same bits on a second call.  A width the kernel must refuse (Cl = 12 in half) is refused with TS_ERR_UNSUPPORTED.

BatchNorm: N in {2, 3, 257, 5000} x C in {4, 8, 128, 1024}, with and without a residual, slopes 0.01 and 0.2, float and half, one channel
constant (3.0 in every row, with a zero bias: outputs that are exactly 0, which must take the slope branch) - forward, mask, running
buffers, num_batches_tracked and the four gradients against float64 within LAMBDA u32 S (oracle/bn64.py's chain length plus 2 for the
slope's products; half results + u16 |ref| + 2^-25); grad_residual equals the masked gradient bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import fid_ref as FR
from oracle.bn64 import LAMBDA, running_ref64

pytestmark = pytest.mark.gpu

SHAPES = [((2, 8, 16), ((4, 8), (2, 4), (1, 2))), ((1, 9, 13), ((5, 7), (3, 4), (2, 2))), ((1, 1, 7), ((1, 4), (1, 2), (1, 1))),
          ((1, 16, 64), ((8, 32), (4, 16), (2, 8)))]
WIDTHS = [(8, 8, 8), (512, 128, 128), (128, 128, 128)]
U32, U16, SUB = FR.U32, FR.U16, FR.SUB


def _dev(a):
    """rows [T, H, W, C] on the host -> the channels-last map [T, C, H, W] on the device (the same memory)"""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().permute(0, 3, 1, 2)


def _host(t):
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _maps(shape, sizes, channels, half, seed):
    (T, H, W), (ca, cb, cl) = shape, channels
    rs = np.random.RandomState(seed)
    dt = np.float16 if half else np.float32
    x, x1 = rs.randn(T, H, W, ca).astype(dt), rs.randn(T, H, W, cb).astype(dt)
    coarse = [(rs.randn(T, h, w, cl) * 2 + 0.5).astype(dt) for h, w in sizes]
    g = rs.randn(T, H, W, ca + cb + 3 * cl).astype(dt)
    gres = [rs.randn(T, H, W, cl).astype(dt) for _ in range(3)]
    return x, x1, coarse, g, gres


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("channels", WIDTHS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("shape,sizes", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "levels")
def test_decoder_forward_and_adjoint(shape, sizes, channels, half):
    from taseg_amd import backend as B
    x, x1, coarse, g, gres = _maps(shape, sizes, channels, half, 11)
    ca, cb, cl = channels
    lanes = 8 if half else 4
    dx, dx1, dco = _dev(x), _dev(x1), [_dev(v) for v in coarse]
    assert B.fid_upcat_rows_takes(dx, dx1, dco)
    # ---- forward
    cat, res, tables = B.fid_upcat_rows_forward(dx, dx1, dco, levels=True)
    plain, none, _ = B.fid_upcat_rows_forward(dx, dx1, dco)
    assert none is None and torch.equal(plain, cat)
    want32, _ = FR.upcat(x, x1, coarse, np.float32)
    want = FR.store(want32, x)
    got = _host(cat)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), int((got != want).sum())
    for k, r in enumerate(res):
        assert torch.equal(r, cat[:, ca + cb + k * cl: ca + cb + (k + 1) * cl])
    want64, _ = FR.upcat(x, x1, coarse, np.float64)
    for k, bar in enumerate(FR.forward_bar(coarse, shape[1], shape[2])):
        sl = slice(ca + cb + k * cl, ca + cb + (k + 1) * cl)
        err = np.abs(got[..., sl].astype(np.float64) - want64[..., sl])
        allowed = bar + ((U16 * np.abs(want64[..., sl]) + SUB) if half else 0.0)
        assert (err <= allowed).all()
        print(f"level {sizes[k]}: worst |got - float64| {err.max():.2e}, bar {bar:.2e}")
    # ---- backward: with and without the level maps' gradients, twice
    dg, dgres = _dev(g), [_dev(a) for a in gres]
    for extra, dextra in ((None, None), (gres, dgres)):
        gx, gx1, gk = B.fid_upcat_rows_backward(dg, channels, sizes, tables, dextra)
        again = B.fid_upcat_rows_backward(dg, channels, sizes, tables, dextra)
        assert torch.equal(gx, again[0]) and torch.equal(gx1, again[1]) and all(torch.equal(a, b) for a, b in zip(gk, again[2]))
        assert torch.equal(gx, dg[:, :ca]) and torch.equal(gx1, dg[:, ca:ca + cb])
        _, _, want_k = FR.upcat_adjoint(g, channels, sizes, extra, np.float32, lanes)
        _, _, want_k64 = FR.upcat_adjoint(g, channels, sizes, extra, np.float64, lanes)
        bars = FR.adjoint_bar(g, channels, sizes, extra, lanes)
        for k in range(3):
            got_k, w = _host(gk[k]), FR.store(want_k[k], g)
            assert got_k.shape == w.shape and got_k.tobytes() == w.tobytes(), (k, extra is not None, int((got_k != w).sum()))
            err = np.abs(got_k.astype(np.float64) - want_k64[k])
            allowed = bars[k] + ((U16 * np.abs(want_k64[k]) + SUB) if half else 0.0)
            assert (err <= allowed).all()
            print(f"adjoint level {sizes[k]} (extra gradients: {extra is not None}): worst err / bar {float((err / allowed).max()):.3g}")


def test_decoder_refuses_a_width_that_is_no_multiple_of_the_piece():
    from taseg_amd import _lib as L
    from taseg_amd import backend as B
    (T, H, W), sizes = SHAPES[0]
    x, x1, coarse, _, _ = _maps((T, H, W), sizes, (8, 8, 12), True, 3)
    dx, dx1, dco = _dev(x), _dev(x1), [_dev(v) for v in coarse]
    assert not B.fid_upcat_rows_takes(dx, dx1, dco)
    with pytest.raises(ValueError):
        B.fid_upcat_rows_forward(dx, dx1, dco)
    # ... and by the library itself
    tables = B.fid_upcat_tables(H, W, sizes, dx.device)
    arr = ctypes.c_int32 * 3
    hk, wk = arr(*(h for h, _ in sizes)), arr(*(w for _, w in sizes))
    cat = torch.empty((T, H, W, 8 + 8 + 36), dtype=torch.float16, device="cuda")
    rc = L.load().ts_fid_upcat_rows_forward(L.ptr(dx), L.ptr(dx1), L.ptr(dco[0]), L.ptr(dco[1]), L.ptr(dco[2]), L.ptr(tables), T, H, W, hk, wk,
                                            8, 8, 12, 1, L.ptr(cat), None, None, None, L.stream())
    assert rc != 0 and "multiple of 8" in L.load().ts_last_error().decode()
    with pytest.raises(L.BackendError):          # float rows take 12 channels; 6 they do not
        L.check(L.load().ts_fid_upcat_rows_forward(L.ptr(dx), L.ptr(dx1), L.ptr(dco[0]), L.ptr(dco[1]), L.ptr(dco[2]), L.ptr(tables), T, H, W,
                                                   hk, wk, 8, 8, 6, 0, L.ptr(cat), None, None, None, L.stream()))


def test_fid_upcat_node_matches_the_aten_chain_under_autograd():
    """the autograd node (functional.fid_upcat) against F.interpolate + torch.cat on the device: values to the forward's bar (ATen's own
    kernel contracts its products and sums, so equal bits are not asked of it), gradients to the adjoint's"""
    from taseg_amd.options import options
    from taseg_amd.pcseg.model.segmentor.range.functional import fid_upcat
    (shape, sizes), channels = SHAPES[3], (128, 128, 128)
    x, x1, coarse, g, gres = _maps(shape, sizes, channels, False, 21)
    outs = {}
    for on in (True, False):
        leaves = [_dev(a).requires_grad_() for a in (x, x1, *coarse)]
        with options.override(image_fid_upcat=on):
            cat, res = fid_upcat(*leaves, levels=True)
        assert (type(cat.grad_fn).__name__ == "_FidUpCatRowsBackward") == on          # the node itself, not a quiet fall-back
        loss = (cat * _dev(g)).sum() + sum((r * _dev(a)).sum() for r, a in zip(res, gres))
        loss.backward()
        outs[on] = (cat.detach(), [leaf.grad for leaf in leaves])
    bars = FR.forward_bar(coarse, shape[1], shape[2])
    assert float((outs[True][0] - outs[False][0]).abs().max()) <= 2 * max(bars)
    differ = int((outs[True][0] != outs[False][0]).sum())
    print(f"{differ} of {outs[True][0].numel()} elements differ in bits between the kernel and ATen's device kernel")
    abars = FR.adjoint_bar(g, channels, sizes, gres, 4)
    for k in range(5):
        a, b = outs[True][1][k], outs[False][1][k]
        assert a.shape == b.shape
        if k < 2:
            assert torch.equal(a, b)
        else:
            assert (np.abs(_host(a).astype(np.float64) - _host(b)) <= 2 * abars[k - 2]).all()


# ------------------------------------------------------------------------------------------------------------------ BatchNorm

def _check(name, got, ref, s, lam, extra=0.0):
    err = (got.double() - ref).abs()
    bar = lam * U32 * s + extra
    if got.dtype == torch.float16:
        bar = bar + U16 * ref.abs() + SUB
    worst = float((err / bar.clamp_min(1e-300)).max())
    assert bool((err <= bar).all()), f"{name}: worst err/bar {worst:.3g}"
    return worst


def _bits(mask, n, c, half):
    """the mask's bits as a bool [n, c]"""
    ve = 8 if half else 4
    m = mask.view(n, c // ve, 1).to(torch.int32)
    return ((m >> torch.arange(ve, device=mask.device, dtype=torch.int32)) & 1).bool().reshape(n, c)


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("c", [4, 8, 128, 1024])
@pytest.mark.parametrize("n", [2, 3, 257, 5000])
def test_bn_leaky_act_train_against_float64(n, c, half):
    from taseg_amd import _lib as L
    from taseg_amd import backend as B
    dt = torch.float16 if half else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + c)
    rnd = lambda *s: torch.randn(*s, generator=gen, device="cuda")  # noqa: E731
    x = (rnd(n, c) * 2 + 0.5).to(dt)
    const = 1                                                       # a channel that holds one value; with a zero bias its output is 0
    x[:, const] = 3.0
    res = rnd(n, c).to(dt)
    res[::2, const] = 0.0                                           # (with a residual: exact zeros in every other row)
    gy = (rnd(n, c) + 0.5).to(dt)
    weight, bias = torch.rand(c, generator=gen, device="cuda") + 0.5, rnd(c)
    bias[const] = 0.0
    eps, momentum = float(np.float32(1e-5)), float(np.float32(0.1))
    if half and c % 8:
        with pytest.raises(L.BackendError, match="multiple of 8"):
            B.bn_leaky_act_train_forward(x, weight, bias, None, None, None, eps, momentum, 0.01)
        return
    lam = LAMBDA(n, c, half) + 2
    for with_res in (False, True):
        for slope in (float(np.float32(0.01)), float(np.float32(0.2))):
            rm0, rv0 = rnd(c), torch.rand(c, generator=gen, device="cuda") + 0.5
            rm, rv, nbt = rm0.clone(), rv0.clone(), torch.tensor(7, device="cuda")
            r = res if with_res else None
            out, mask, stats = B.bn_leaky_act_train_forward(x, weight, bias, rm, rv, nbt, eps, momentum, slope, r)
            out2, mask2, stats2 = B.bn_leaky_act_train_forward(x, weight, bias, rm0.clone(), rv0.clone(), None, eps, momentum, slope, r)
            assert torch.equal(out, out2) and torch.equal(mask, mask2) and torch.equal(stats, stats2) and int(nbt) == 8
            (y, gx, gres, gw, gb, mean, var), (sy, sgx, sgres, sgw, sgb, smean, svar), g = FR.bn_leaky_ref64(x, r, weight, bias, slope, eps, gy,
                                                                                                         out)
            tag = f"n {n} c {c} {'half' if half else 'float'} res {with_res} slope {slope:.2f}"
            worst = [_check(tag + " y", out, y, sy, lam), _check(tag + " mean", stats[0], mean, smean, lam)]
            got_var = 1.0 / stats[1].double().square() - eps
            worst.append(_check(tag + " var", got_var.float(), var, svar, lam, extra=2 * U32 * (var + eps)))
            assert torch.equal(_bits(mask, n, c, half), out > 0)
            zero = out[:, const] == 0
            assert bool(zero.all()) if not with_res else bool(zero[::2].all())          # exact zeros, all on the slope branch
            want_rm, want_rv, srm, srv = running_ref64(rm0, rv0, mean, var, smean, svar, n, momentum)
            worst += [_check(tag + " running_mean", rm, want_rm, srm, lam), _check(tag + " running_var", rv, want_rv, srv, lam)]
            ggx, ggres, ggw, ggb = B.bn_leaky_act_train_backward(gy, mask, x, stats, weight, slope, with_res)
            again = B.bn_leaky_act_train_backward(gy, mask, x, stats, weight, slope, with_res)
            assert all(a is b or torch.equal(a, b) for a, b in zip((ggx, ggres, ggw, ggb), again))
            worst += [_check(tag + " grad_x", ggx, gx, sgx, lam), _check(tag + " grad_weight", ggw, gw, sgw, lam),
                      _check(tag + " grad_bias", ggb, gb, sgb, lam)]
            assert (ggres is None) == (not with_res)
            if with_res:
                masked = torch.where(out > 0, gy, (gy.float() * slope).to(dt))
                assert torch.equal(ggres, masked)
                worst.append(_check(tag + " grad_residual", ggres, gres, sgres, lam))
            print(f"{tag}: worst err / bar {max(worst):.3g}")


def test_bn_leaky_node_matches_the_modules_under_autograd():
    """`_bn_act` on a channels-last device map (one node) against the modules themselves, values and gradients"""
    from taseg_amd.options import options
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _bn_act
    torch.manual_seed(5)
    outs = {}
    for fused in (True, False):
        bn, act = torch.nn.BatchNorm2d(128).cuda().train(), torch.nn.LeakyReLU()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, 128))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, 128))
        gen = torch.Generator(device="cuda").manual_seed(9)
        x = torch.randn(2, 128, 9, 13, generator=gen, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_()
        res = torch.randn(2, 128, 9, 13, generator=gen, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_()
        with options.override(image_fused_bn=fused):
            y = _bn_act(bn, act, x, res)
        assert (type(y.grad_fn).__name__ == "_BatchNormLeakyRowsBackward") == fused
        (y * torch.randn(y.shape, generator=gen, device="cuda")).sum().backward()
        outs[fused] = (y.detach(), x.grad, res.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(),
                       int(bn.num_batches_tracked))
    for a, b in zip(outs[True][:-1], outs[False][:-1]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    assert outs[True][-1] == outs[False][-1] == 1
