"""The kernels of csrc/rpvnet.hip on the GPU, and the entry points of torchsparse/nn/functional.py that sit on them.

ts_range_plan equals tests/rpvnet_ref.py's float32 restatement BIT FOR BIT (pixels, corners, weights, the flag word) - at the three
resolutions of the range branch on every column and ring the dataset can produce, and on small maps with hand-placed rows.
`point_to_range` equals the restated summation rule of ts_voxelize_mean_forward (tests/spvcnn_ref.py) bit for bit over B h w "voxels".
`range_to_point`, its adjoint under both inverse forms, and ts_range_point_tail_forward meet float64 within bars built from the
number of live terms and the sum of their magnitudes (oracle/points64.py; tests/rpvnet_ref.py states the tail's).  The tail's mask
must equal the sign of the float64 BatchNorm term wherever that term exceeds its own bar.  Every kernel gives the same bits twice.

Shapes: n = 1, 2, 63, 65 (one row, below / above the 64 rows one block holds at c = 4); c = 4, 8, 1024 (narrowest of either storage,
one row per block); maps 1 x 1 (three of four corners outside), 2 x 2, 4 x 128; B = 3 with the middle sample empty."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rpvnet_ref as R  # noqa: E402
import spvcnn_ref as RS  # noqa: E402
from oracle import points64 as P64  # noqa: E402
from test_gpu_bn_float64 import EPS, U32, _check, _lam, bn_ref64  # noqa: E402

MAPS = [(1, 1), (2, 2), (4, 128)]
TAIL_CASES = [(torch.float32, 4), (torch.float32, 8), (torch.float32, 1024), (torch.float16, 8), (torch.float16, 1024)]
_ids = lambda case: f"{'half' if case[0] == torch.float16 else 'fp32'}-{case[1]}"  # noqa: E731
FLAGGED = np.array([[3, 0, 0], [-1, 0, 0], [0.5, 0, 0], [0, np.nan, 0], [1, 0, np.inf], [0, np.float32(1.0000001), 0], [2, 0, -1.5]],
                   dtype=np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_plan(pxpy, b, h, w):
    from taseg_amd import backend as B
    pix, bidx, bw, err = B.range_plan(_dev(pxpy), b, h, w)
    pix2, bidx2, bw2, _ = B.range_plan(_dev(pxpy), b, h, w)
    assert torch.equal(pix, pix2) and torch.equal(bidx, bidx2) and torch.equal(bw, bw2)
    rp, ri, rw, re = R.plan32(pxpy, b, h, w)
    assert np.array_equal(pix.cpu().numpy(), rp)
    assert np.array_equal(bidx.cpu().numpy(), ri)
    assert np.array_equal(_bits(bw.cpu().numpy()), _bits(rw))
    assert int(err) == re
    return rp, ri, rw, re


# ---------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("hw", [(64, 2048), (16, 512), (4, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_on_every_dataset_column_and_ring(hw):
    pxpy, xs, ys = R.kitti_pxpy()
    pix, bidx, bw, err = _same_plan(pxpy, 1, *hw)
    assert err == 0 and (pix >= 0).all() and (pix < hw[0] * hw[1]).all()
    if hw == (64, 2048):
        below = (pix[:2048] % 2048) < xs                      # the truncating rule: columns that land under their own index
        assert below.any() and ((pix[:2048] % 2048)[below] == xs[below] - 1).all()


@pytest.mark.parametrize("n", [1, 2, 63, 65])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_equals_the_restatement(hw, n):
    b = 3
    pxpy = np.concatenate([R.random_pxpy(n, b, 10 * n + hw[1]), FLAGGED])          # sample 1 has no row; flagged rows behind
    pix, bidx, bw, err = _same_plan(pxpy, b, *hw)
    assert err == (R.ERR_BATCH | R.ERR_NONFINITE | R.ERR_OUTSIDE)
    assert (pix[n:] == -1).all() and (bidx[n:] == -1).all() and (bw[n:] == 0).all()
    assert (pix[:n] >= 0).all() and ((pix[:n] // (hw[0] * hw[1])) == pxpy[:n, 0]).all()   # every row inside its own sample's map
    live = (bidx[:n, :4] >= 0)
    assert ((bidx[:n, :4] // (hw[0] * hw[1]))[live] == np.repeat(pxpy[:n, :1], 4, 1)[live]).all()
    if hw == (1, 1):
        assert (live.sum(1) == 1).all()                       # three of four corners outside
    assert _same_plan(pxpy[:n], b, *hw)[3] == 0               # no flagged row: a clean word
    _same_plan(pxpy[:0], b, *hw)                              # no rows at all


def test_plan_refuses_bad_sizes():
    from taseg_amd import backend as B
    with pytest.raises(B.BackendError):
        B.range_plan(torch.zeros((4, 3), device="cuda"), 0, 4, 4)
    with pytest.raises(B.BackendError):
        B.range_plan(torch.zeros((4, 3), device="cuda"), 1 << 10, 1 << 11, 1 << 11)


# --------------------------------------------------------------------------------------------------------------- point_to_range
def _crowded_pxpy(n, b, seed, crowd):
    """random rows plus `crowd` rows at one spot of the last sample: one pixel of more than P rows, one interpolation cell of more than
    one segment of the cells form"""
    spot = np.tile(np.array([[b - 1, 0.3, -0.2]], dtype=np.float32), (crowd, 1))
    out = np.concatenate([R.random_pxpy(n, b, seed), spot])
    return np.ascontiguousarray(out[np.argsort(out[:, 0], kind="stable")])


@pytest.mark.parametrize("case", [(torch.float32, 4), (torch.float32, 1024), (torch.float16, 8)], ids=_ids)
def test_point_to_range_equals_the_mean_rule(case):
    from taseg_amd import backend as B
    from taseg_amd.torchsparse.nn import functional as F
    dtype, c = case
    half = dtype == torch.float16
    b, h, w = 3, 4, 128
    piece = B.voxelize_mean_piece_rows()
    pxpy = np.concatenate([_crowded_pxpy(65, b, 3, 2 * piece + 7), FLAGGED])
    n = len(pxpy)
    feat = (np.random.RandomState(5).randn(n, c) * 2 + 0.25).astype(np.float16 if half else np.float32)
    plan = F.range_plan(_dev(pxpy), b, h, w)
    pix = plan["pix"].cpu().numpy()
    assert np.bincount(pix[pix >= 0]).max() > 2 * piece
    x = _dev(feat).requires_grad_()
    fmap = F.point_to_range(x, plan, b, h, w)
    assert fmap.shape == (b, c, h, w) and fmap.dtype == dtype and fmap.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(fmap, F.point_to_range(x, plan, b, h, w))
    want = RS.mean32(feat, pix, b * h * w, piece)
    want = want.astype(np.float16) if half else want
    got = fmap.detach().permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    empty = np.bincount(pix[pix >= 0], minlength=b * h * w) == 0
    assert empty[h * w:2 * h * w].all() and (got[empty] == 0).all()                # the sample without rows: a zero map
    g = np.random.RandomState(6).randn(b, c, h, w).astype(feat.dtype)
    fmap.backward(_dev(g))
    grows = np.ascontiguousarray(g.transpose(0, 2, 3, 1)).reshape(-1, c)
    want_back = RS.mean_backward(grows, pix, b * h * w)
    want_back = want_back.astype(np.float16) if half else want_back
    assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(want_back))
    assert (x.grad.cpu().numpy()[pix < 0] == 0).all()                               # flagged rows take no part


# --------------------------------------------------------------------------------------------------------------- range_to_point
@pytest.mark.parametrize("cells", [False, True], ids=["csr", "cells"])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", [(torch.float32, 4), (torch.float32, 1024), (torch.float16, 8)], ids=_ids)
def test_range_to_point_and_its_adjoint_vs_float64(case, hw, cells):
    from taseg_amd.torchsparse.nn import functional as F
    dtype, c = case
    half = dtype == torch.float16
    b, (h, w) = 3, hw
    pxpy = np.concatenate([_crowded_pxpy(63, b, 11, 150), FLAGGED])
    n, rows = len(pxpy), b * h * w
    rs = np.random.RandomState(12)
    fm = rs.randn(b, c, h, w).astype(np.float16 if half else np.float32)
    plan = F.range_plan(_dev(pxpy), b, h, w, cells=cells)
    if cells:
        assert plan["order"][0] == "cells" and plan["order"][2].shape[0] - 1 > len(np.unique(plan["bidx"].cpu().numpy(), axis=0))
    t = _dev(fm).contiguous(memory_format=torch.channels_last).requires_grad_()
    out = F.range_to_point(t, plan)
    assert out.shape == (n, c) and out.dtype == dtype and torch.equal(out, F.range_to_point(t, plan))
    bidx, bw = plan["bidx"].cpu().numpy(), plan["bw"].cpu().numpy()
    frows = np.ascontiguousarray(fm.transpose(0, 2, 3, 1)).reshape(rows, c)
    ref, tl, s = P64.devoxelize_forward64(frows, bidx, bw)
    bar = P64.bar_sum(tl, s)
    bar = P64.bar_half(bar, ref) if half else bar
    err = np.abs(out.detach().double().cpu().numpy() - ref)
    print(f"range_to_point {_ids(case)} {h}x{w}: worst err / bar {float((err / np.maximum(bar, 1e-300)).max()):.3g}")
    assert (err <= bar).all() and (out.detach().cpu().numpy()[-len(FLAGGED):] == 0).all()
    # a row of another layout (plain NCHW) reads the same values
    assert torch.equal(F.range_to_point(_dev(fm), plan), out.detach())
    g = rs.randn(n, c).astype(fm.dtype)
    out.backward(_dev(g))
    a64, ta, sa = P64.adjoint64(g, bidx, bw, rows)
    abar = P64.bar_sum(ta, sa)
    abar = P64.bar_half(abar, a64) if half else abar
    got = t.grad.permute(0, 2, 3, 1).reshape(rows, c)
    aerr = np.abs(got.double().cpu().numpy() - a64)
    print(f"  adjoint ({'cells' if cells else 'csr'}): worst err / bar {float((aerr / np.maximum(abar, 1e-300)).max()):.3g}")
    assert (aerr <= abar).all()
    assert (got.cpu().numpy()[ta == 0] == 0).all() and (ta[h * w:2 * h * w] == 0).all()       # pixels nobody reads: zero gradient


# ---------------------------------------------------------------------------------------------------------------------- the tail
def _unpack(mask, n, c, half):
    per = 8 if half else 4
    bits = (mask.cpu().numpy().reshape(n, c // per, 1) >> np.arange(per).reshape(1, 1, per)) & 1
    return bits.reshape(n, c).astype(bool)


@pytest.mark.parametrize("n", [1, 2, 63, 65])
@pytest.mark.parametrize("case", TAIL_CASES, ids=_ids)
def test_range_point_tail_forward_vs_float64(case, n):
    from taseg_amd import backend as B
    dtype, c = case
    half = dtype == torch.float16
    b, h, w = 2, 4, 128
    idx, tw, m, pxpy, y, vox, rows, mean, invstd, gamma, beta = R.tail_inputs(n, c, half, 500 + n + c, b, h, w)
    _, bidx, bw, _ = R.plan32(pxpy, b, h, w)
    args = [_dev(a) for a in (y, vox, idx, tw, rows, bidx, bw, mean, invstd, gamma, beta)]
    out, mask = B.range_point_tail_forward(*args, want_mask=True)
    out2, mask2 = B.range_point_tail_forward(*args, want_mask=True)
    plain, none = B.range_point_tail_forward(*args)
    assert torch.equal(out, out2) and torch.equal(mask, mask2) and torch.equal(out, plain) and none is None
    ref, bar, bn, bn_bar, t_d, t_r = R.tail64(y, vox, idx, tw, rows, bidx, bw, mean, invstd, gamma, beta)
    if half:
        bar = P64.bar_half(bar, ref)
    err = np.abs(out.double().cpu().numpy() - ref)
    print(f"range tail {_ids(case)} n={n}: worst err / bar {float((err / bar).max()):.3g}")
    assert (err <= bar).all()
    assert (t_r > 0).all() and (n < 6 or ((t_d == 0).any() and (t_d > 0).any()))
    if n >= 6:
        assert (pxpy[:, 0] == 1).any() and (bidx[pxpy[:, 0] == 1, :4].max(1) >= h * w).all()     # sample 1 reads the second map
    sure = np.abs(bn) > bn_bar
    assert (~sure).mean() <= 0.01
    assert np.array_equal(_unpack(mask, n, c, half)[sure], (bn > 0)[sure])
    # with an empty map operand (all corners -1) the kernel is ts_point_tail_forward, bit for bit
    none_idx, none_w = torch.full_like(args[5], -1), torch.zeros_like(args[6])
    alone, _ = B.range_point_tail_forward(*args[:5], none_idx, none_w, *args[7:])
    spv, _ = B.point_tail_forward(args[0], args[1], args[2], args[3], *args[7:])
    assert torch.equal(alone, spv)


def test_range_point_tail_refuses_widths_off_the_16_byte_rule():
    from taseg_amd import backend as B
    for dtype, c in ((torch.float32, 6), (torch.float16, 12), (torch.float32, 1028)):
        idx, tw, m, pxpy, y, vox, rows, mean, invstd, gamma, beta = R.tail_inputs(3, c, dtype == torch.float16, 5)
        _, bidx, bw, _ = R.plan32(pxpy, 2, 4, 128)
        with pytest.raises(B.BackendError):
            B.range_point_tail_forward(*[_dev(a) for a in (y, vox, idx, tw, rows, bidx, bw, mean, invstd, gamma, beta)])


@pytest.mark.parametrize("cells", [False, True], ids=["csr", "cells"])
@pytest.mark.parametrize("case", [(torch.float32, 32), (torch.float32, 48), (torch.float16, 32)], ids=_ids)
def test_range_point_tail_function_vs_float64_autograd(case, cells):
    """functional.range_point_tail on a training-mode BatchNorm1d: value, grad_y, grad_gamma, grad_beta, the voxel gradient and the
    map's gradient against float64 (bn_ref64 for the BatchNorm half; points64 for the two gathered halves; the ReLU's derivative
    taken where the float64 BatchNorm term is positive - no element sits inside that term's bar, asserted)."""
    from taseg_amd import backend as B
    from taseg_amd.torchsparse.nn import functional as F
    dtype, c = case
    half = dtype == torch.float16
    n, b, h, w = 257, 2, 4, 128
    idx, tw, m, pxpy, y, vox, rows, _, _, gamma, beta = R.tail_inputs(n, c, half, 900 + c, b, h, w)
    fm = np.ascontiguousarray(rows.reshape(b, h, w, c).transpose(0, 3, 1, 2))
    bn = torch.nn.BatchNorm1d(c).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
    yt, vt = _dev(y).requires_grad_(), _dev(vox).requires_grad_()
    ft = _dev(fm).contiguous(memory_format=torch.channels_last).requires_grad_()
    it, wt = _dev(idx), _dev(tw)
    plan = F.range_plan(_dev(pxpy), b, h, w, cells=cells)
    g = _dev(np.random.RandomState(11).randn(n, c).astype(y.dtype))
    out = F.range_point_tail(yt, bn, vt, it, wt, B.devox_csr(it, wt, m), ft, plan)
    assert out.dtype == dtype and int(bn.num_batches_tracked) == 1
    out.backward(g)
    lam = _lam(n, c, half)
    (bn64, _, _, _, _, _, _), (sy, _, _, _, _, _, _) = bn_ref64(yt.detach(), None, bn.weight.detach(), bn.bias.detach(), False, EPS, g,
                                                              None)
    assert bool((bn64.abs() > lam * U32 * sy).all())
    (_, gx, _, gw, gb, _, _), (_, sgx, _, sgw, sgb, _, _) = bn_ref64(yt.detach(), None, bn.weight.detach(), bn.bias.detach(), True,
                                                                   EPS, g, relu_from=bn64)
    bidx, bw = plan["bidx"].cpu().numpy(), plan["bw"].cpu().numpy()
    d64, t_d, s_d = P64.devoxelize_forward64(vox, idx, tw)
    r64, t_r, s_r = P64.devoxelize_forward64(rows, bidx, bw)
    gather_bar = P64.bar_sum(t_d, s_d) + P64.bar_sum(t_r, s_r)
    d64, r64, gather_bar = (torch.from_numpy(a).cuda() for a in (d64, r64, gather_bar))
    ref = (d64 + r64) + bn64.clamp_min(0.0)
    extra = gather_bar + P64.SLACK * P64.U * (2 * (d64 + r64).abs() + bn64.clamp_min(0.0)) + P64.TINY * 12
    _check("range tail value", out.detach(), ref, sy, lam, extra=extra)
    _check("grad y", yt.grad, gx, sgx, lam)
    _check("grad gamma", bn.weight.grad, gw, sgw, lam)
    _check("grad beta", bn.bias.grad, gb, sgb, lam)
    for name, got, (a64, ta, sa) in (("voxels", vt.grad, P64.adjoint64(g.cpu().numpy(), idx, tw, m)),
                                     ("map", ft.grad.permute(0, 2, 3, 1).reshape(b * h * w, c),
                                      P64.adjoint64(g.cpu().numpy(), bidx, bw, b * h * w))):
        abar = P64.bar_sum(ta, sa)
        abar = P64.bar_half(abar, a64) if half else abar
        aerr = np.abs(got.double().cpu().numpy() - a64)
        print(f"  grad {name}: worst err / bar {float((aerr / np.maximum(abar, 1e-300)).max()):.3g}")
        assert (aerr <= abar).all()
    # two runs from one state: the same bits everywhere
    bn2 = torch.nn.BatchNorm1d(c).cuda().train()
    with torch.no_grad():
        bn2.weight.copy_(torch.from_numpy(gamma))
        bn2.bias.copy_(torch.from_numpy(beta))
    y2, v2 = _dev(y).requires_grad_(), _dev(vox).requires_grad_()
    f2 = _dev(fm).contiguous(memory_format=torch.channels_last).requires_grad_()
    out2 = F.range_point_tail(y2, bn2, v2, it, wt, B.devox_csr(it, wt, m), f2, plan)
    out2.backward(g)
    for p, q in ((out, out2), (yt.grad, y2.grad), (vt.grad, v2.grad), (ft.grad, f2.grad), (bn.weight.grad, bn2.weight.grad),
                 (bn.running_var, bn2.running_var)):
        assert torch.equal(p, q)


def test_range_point_tail_falls_back_to_the_chain_where_it_must(monkeypatch):
    """evaluation mode without a graph is the kernel's evaluation form; with a graph, or with the private switch off, the chain
    spdevoxelize + range_to_point + relu(bn(y)) - two float32 evaluations of one expression, each within the value's bar"""
    from taseg_amd.torchsparse.nn import functional as F
    n, c, b, h, w = 255, 32, 2, 4, 128
    idx, tw, m, pxpy, y, vox, rows, mean, invstd, gamma, beta = R.tail_inputs(n, c, False, 77, b, h, w)
    fm = np.ascontiguousarray(rows.reshape(b, h, w, c).transpose(0, 3, 1, 2))
    bn = torch.nn.BatchNorm1d(c).cuda().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(mean))
    yt, vt, it, wt, ft = (_dev(a) for a in (y, vox, idx, tw, fm))
    plan = F.range_plan(_dev(pxpy), b, h, w)
    with torch.no_grad():
        kernel = F.range_point_tail(yt, bn, vt, it, wt, None, ft, plan)
    chain = F.range_point_tail(yt.clone().requires_grad_(), bn, vt, it, wt, None, ft, plan)
    assert chain.requires_grad and not kernel.requires_grad
    monkeypatch.setattr(F, "_RANGE_TAIL_KERNEL", False)
    with torch.no_grad():
        off = F.range_point_tail(yt, bn, vt, it, wt, None, ft, plan)
    assert torch.equal(off, chain.detach())
    is64 = np.full(c, 1.0 / np.sqrt(1.0 + float(bn.eps)))
    ref, bar, *_ = R.tail64(y, vox, idx, tw, rows, plan["bidx"].cpu().numpy(), plan["bw"].cpu().numpy(), mean, is64, gamma, beta)
    for got in (kernel, off):
        assert (np.abs(got.double().cpu().numpy() - ref) <= bar + R.U * np.abs(ref)).all()       # (+ invstd's own rounding)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_range_hand_over_without_a_map_term_is_point_tail_bit_for_bit(half):
    """Through the functional layer, in training mode: with every corner of the plan -1 and a map of zeros `range_point_tail` is
    `point_tail` - the result, the gradient of y, the gradient of the voxel rows, and what the BatchNorm module takes home."""
    from taseg_amd import backend as B
    from taseg_amd.torchsparse.nn import functional as F
    n, c, b, h, w = 65, 32, 2, 4, 128
    idx, tw, m, pxpy, y, vox, _, _, _, gamma, beta = R.tail_inputs(n, c, half, 41, b, h, w)
    it, wt = _dev(idx), _dev(tw)
    order = B.devox_csr(it, wt, m)
    plan = F.range_plan(_dev(pxpy), b, h, w, backward=False)
    plan["bidx"], plan["bw"] = torch.full_like(plan["bidx"], -1), torch.zeros_like(plan["bw"])
    fmap = torch.zeros((b, c, h, w), dtype=_dev(y).dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    g = _dev(np.random.RandomState(12).randn(n, c).astype(y.dtype))
    got = []
    for ranged in (False, True):
        bn = torch.nn.BatchNorm1d(c).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(gamma))
            bn.bias.copy_(torch.from_numpy(beta))
        yt, vt = _dev(y).requires_grad_(), _dev(vox).requires_grad_()
        out = F.range_point_tail(yt, bn, vt, it, wt, order, fmap, plan) if ranged else F.point_tail(yt, bn, vt, it, wt, order)
        assert out.dtype == yt.dtype and out.grad_fn is not None and "_PointTail" in type(out.grad_fn).__name__
        out.backward(g)
        got.append((out.detach(), yt.grad, vt.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    for name, p, q in zip(("out", "grad y", "grad vox", "grad gamma", "grad beta", "running mean", "running var"), *got):
        assert torch.equal(p, q), name
    assert bool(got[0][2].abs().sum() > 0)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_range_point_tail_in_evaluation_mode_is_the_kernel_on_the_running_statistics(half):
    """no graph, module in evaluation mode: the bits of the kernel the training node launches, fed the running buffers"""
    from taseg_amd import backend as B
    from taseg_amd.torchsparse.nn import functional as F
    n, c, b, h, w = 2, 32, 2, 4, 128
    idx, tw, m, pxpy, y, vox, rows, mean, invstd, gamma, beta = R.tail_inputs(n, c, half, 43, b, h, w)
    bn = torch.nn.BatchNorm1d(c).cuda().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(mean))
        bn.running_var.copy_(torch.from_numpy(1.0 / (invstd * invstd)))
    yt, vt, it, wt, rt = (_dev(a) for a in (y, vox, idx, tw, rows))
    ft = rt.view(b, h, w, c).permute(0, 3, 1, 2)
    plan = F.range_plan(_dev(pxpy), b, h, w, backward=False)
    with torch.no_grad():
        out = F.range_point_tail(yt, bn, vt, it, wt, None, ft, plan)
        want, _ = B.range_point_tail_forward(yt, vt, it, wt, rt, plan["bidx"], plan["bw"], bn.running_mean,
                                             torch.rsqrt(bn.running_var + bn.eps), bn.weight, bn.bias, want_mask=True)
    assert out.dtype == yt.dtype and torch.equal(out, want)
    assert int(bn.num_batches_tracked) == 0 and np.array_equal(bn.running_mean.cpu().numpy(), mean)
