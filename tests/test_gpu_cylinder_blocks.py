"""The block-level pieces of Cylinder_TS against float64: the sigmoid gate of ReconBlock (ts_sigmoid3_gate_*), `spnn.leaky_bn` on sparse
rows (ts_leaky_bn_train_*), and the deterministic row gather of the point refinement (`functional.gather_rows`).

Gate.  Reference: x * (sigmoid(u) + sigmoid(v) + sigmoid(w)) and its four gradients in float64 from the SAME fp32 inputs.  Bar, per
output tensor: 4 x the largest error the ATen fp32 expression (torch.sigmoid, autograd) has against those float64 values on the same
inputs - the kernel may round `exp` differently, it may not be a different function.  Both errors are printed (run with -s;
profiles/cylinder_float64.txt keeps a run's figures).  Half storage rounds each result once more: the bar there is half's unit
roundoff of the float64 value plus the fp32 bar of the same shape.

leaky_bn.  Reference: nn.BatchNorm1d(LeakyReLU(x)) + r in double, spelled out by `bn_ref64` / `running_ref64` of
tests/test_gpu_bn_float64.py on a = LeakyReLU(x), with that module's bars - LAMBDA(n, c) u32 S, S the same expression on absolute
values - for the same kernel family; LAMBDA + 2 here: the activation's product and the slope, which the kernel takes as a float.
grad x = grad a * (1 or slope).  Running statistics and `num_batches_tracked` included.

Row gather.  out = feats[idx] exactly; its gradient against `index_add_` in double within k u32 sum |g| (k = the most rows one
source row feeds: a float sum of k terms), identical bits in two runs, zero for rows nothing reads."""
import numpy as np
import pytest
import torch

from test_gpu_bn_float64 import EPS, U16, U32, _check, _lam, bn_ref64, running_ref64

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.01


def _gate64(x, u, v, w, g):
    x, u, v, w, g = (t.double().cpu() for t in (x, u, v, w, g))
    su, sv, sw = torch.sigmoid(u), torch.sigmoid(v), torch.sigmoid(w)
    return [x * (su + sv + sw), g * (su + sv + sw), g * x * su * (1 - su), g * x * sv * (1 - sv), g * x * sw * (1 - sw)]


def _gate_inputs(n, c, dtype=torch.float32):
    gen = torch.Generator().manual_seed(1000 * c + n)
    scale = (1.0, 3.0, 0.5, 6.0, 1.0)                              # u wide enough for saturated sigmoids, w for exp overflow at -6 * 4
    return [(torch.randn(n, c, generator=gen) * s).to(dtype).to(DEV) for s in scale]


NAMES = ("out", "grad_x", "grad_u", "grad_v", "grad_w")
_ATEN_ERR = {}


def _aten_errors(n, c):
    """largest |ATen fp32 - float64| per output on the fp32 inputs of this shape (computed once per shape)"""
    if (n, c) not in _ATEN_ERR:
        x, u, v, w, g = _gate_inputs(n, c)
        leaves = [t.clone().requires_grad_() for t in (x, u, v, w)]
        out = (torch.sigmoid(leaves[1]) + torch.sigmoid(leaves[2]) + torch.sigmoid(leaves[3])) * leaves[0]
        got = [out.detach()] + list(torch.autograd.grad(out, leaves, g))
        _ATEN_ERR[(n, c)] = [float((a.double().cpu() - r).abs().max()) for a, r in zip(got, _gate64(x, u, v, w, g))]
    return _ATEN_ERR[(n, c)]


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_gate_vs_float64(n, c):
    from taseg_amd.torchsparse.nn import functional as F
    x, u, v, w, g = _gate_inputs(n, c)
    ref = _gate64(x, u, v, w, g)
    aten = _aten_errors(n, c)
    leaves = [t.clone().requires_grad_() for t in (x, u, v, w)]
    out = F.sigmoid3_gate(*leaves)
    assert type(out.grad_fn).__name__ == "_Sigmoid3GateBackward"        # the kernel ran, not the tensor ops
    got = [out.detach()] + list(torch.autograd.grad(out, leaves, g))
    errs = [float((a.double().cpu() - r).abs().max()) for a, r in zip(got, ref)]
    for name, e, a in zip(NAMES, errs, aten):
        print(f"gate n={n} c={c} {name}: kernel {e:.3e}  ATen fp32 {a:.3e}  ratio {e / a if a else float('inf'):.2f}")
    for name, e, a in zip(NAMES, errs, aten):
        assert e <= 4.0 * a, (name, e, a)
    out2 = F.sigmoid3_gate(x, u, v, w)
    assert torch.equal(out2, got[0])


@pytest.mark.parametrize("n,c", [(257, 32), (4099, 64)])
def test_gate_half_storage(n, c):
    from taseg_amd.torchsparse.nn import functional as F
    x, u, v, w, g = _gate_inputs(n, c, torch.float16)
    ref = _gate64(x, u, v, w, g)
    aten = _aten_errors(n, c)
    leaves = [t.clone().requires_grad_() for t in (x, u, v, w)]
    out = F.sigmoid3_gate(*leaves)
    got = [out.detach()] + list(torch.autograd.grad(out, leaves, g))
    for name, a, r, fp32_bar in zip(NAMES, got, ref, aten):
        assert a.dtype == torch.float16
        err = (a.double().cpu() - r).abs()
        bar = U16 * r.abs() + 4.0 * fp32_bar + 2.0 ** -25
        print(f"gate half n={n} c={c} {name}: worst err/bar {float((err / bar).max()):.3g}")
        assert bool((err <= bar).all()), name


def test_gate_falls_back_where_the_kernel_refuses():
    from taseg_amd.torchsparse.nn import functional as F
    x, u, v, w = (torch.randn(10, 9, device=DEV) for _ in range(4))
    out = F.sigmoid3_gate(x, u, v, w)                                # 9 channels: the tensor ops
    assert torch.equal(out, (torch.sigmoid(u) + torch.sigmoid(v) + torch.sigmoid(w)) * x)


# ------------------------------------------------------------------------------------------------------------------ leaky_bn
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("n,c", [(1, 16), (257, 16), (1000, 32), (4099, 64)])
def test_leaky_bn_vs_float64(n, c, residual):
    import taseg_amd.torchsparse.nn as spnn
    from taseg_amd.torchsparse import SparseTensor
    gen = torch.Generator().manual_seed(77 * c + n)
    x = (torch.randn(n, c, generator=gen) * 2 + 0.5).to(DEV)
    gy = torch.randn(n, c, generator=gen).to(DEV)
    r = torch.randn(n, c, generator=gen).to(DEV) if residual else None
    coords = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    bn = spnn.BatchNorm(c, eps=EPS, momentum=0.1).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=gen))
        bn.running_mean.copy_(torch.randn(c, generator=gen))
        bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    def once():
        with torch.no_grad():
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
            bn.num_batches_tracked.zero_()
        xi = x.clone().requires_grad_()
        ri = r.clone().requires_grad_() if residual else None
        y = spnn.leaky_bn(bn, SparseTensor(xi, coords), residual=SparseTensor(ri, coords) if residual else None)
        assert type(y.F.grad_fn).__name__ == "_LeakyBatchNormTrainBackward"
        leaves = [xi, bn.weight, bn.bias] + ([ri] if residual else [])
        grads = torch.autograd.grad(y.F, leaves, gy)
        return [y.F.detach(), *grads, bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]

    a, b = once(), once()
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two runs gave different bits"
    y, gx, gw, gb = a[:4]
    gres = a[4] if residual else None
    rm, rv, nbt = a[-3:]
    x64 = x.double()
    pos = x64 > 0
    act = torch.where(pos, x64, x64 * SLOPE)
    (ry, rga, rgres, rgw, rgb, mean, var), (sy, sga, _, sgw, sgb, smean, svar) = bn_ref64(act, r, bn.weight.detach(), bn.bias.detach(),
                                                                                        False, EPS, gy)
    lam = _lam(n, c, False) + 2
    d = torch.where(pos, torch.ones_like(x64), torch.full_like(x64, SLOPE))
    _check("leaky_bn y", y, ry, sy, lam)
    _check("leaky_bn grad x", gx, rga * d, sga * d, lam)
    _check("leaky_bn grad weight", gw, rgw, sgw, lam)
    _check("leaky_bn grad bias", gb, rgb, sgb, lam)
    if residual:
        assert torch.equal(gres, gy)                                # the residual's gradient is the incoming gradient
    rrm, rrv, srm, srv = running_ref64(rm0, rv0, mean, var, smean, svar, n, 0.1)
    _check("leaky_bn running_mean", rm, rrm, srm, lam)
    _check("leaky_bn running_var", rv, rrv, srv, lam)
    assert int(nbt) == 1


def test_leaky_bn_in_evaluation_mode_is_the_module_chain():
    import taseg_amd.torchsparse.nn as spnn
    from taseg_amd.torchsparse import SparseTensor
    x = torch.randn(300, 32, device=DEV)
    coords = torch.zeros((300, 4), dtype=torch.int32, device=DEV)
    bn = spnn.BatchNorm(32).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 1.5)
    y = spnn.leaky_bn(bn, SparseTensor(x, coords), residual=SparseTensor(x, coords))
    want = torch.nn.functional.batch_norm(torch.nn.functional.leaky_relu(x, SLOPE), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                          False, 0.1, bn.eps) + x
    assert torch.equal(y.F, want) and int(bn.num_batches_tracked) == 0


# ------------------------------------------------------------------------------------------------------------------ row gather
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
@pytest.mark.parametrize("m,n,c", [(1, 5, 4), (300, 2000, 64), (1437, 4099, 128)])
def test_row_gather_has_index_adds_gradient(m, n, c, dtype):
    from taseg_amd.torchsparse.nn import functional as F
    rs = np.random.RandomState(m + n)
    idx_np = rs.randint(0, m, size=n)
    if m > 10:
        idx_np[idx_np == 7] = 8                                     # a row nothing reads
        idx_np[:200] = 3                                            # ... and one that feeds 200 rows
        idx_np[-1] = -1                                             # tensor indexing's "last row"
    idx = torch.from_numpy(idx_np).to(DEV)
    feats = torch.from_numpy(rs.randn(m, c).astype(np.float32)).to(dtype).to(DEV)
    g = torch.from_numpy(rs.randn(n, c).astype(np.float32)).to(dtype).to(DEV)

    def once():
        f = feats.clone().requires_grad_()
        out = F.gather_rows(f, idx)
        (gf,) = torch.autograd.grad(out, f, g)
        return out.detach(), gf

    out, gf = once()
    assert out.dtype == dtype and gf.dtype == dtype
    assert torch.equal(out, feats[idx])
    out2, gf2 = once()
    assert torch.equal(out2, out) and torch.equal(gf2, gf), "two runs gave different bits"
    pos = torch.from_numpy(np.where(idx_np < 0, idx_np + m, idx_np)).to(DEV)
    ref = torch.zeros((m, c), dtype=torch.float64, device=DEV).index_add_(0, pos, g.double())
    s = torch.zeros((m, c), dtype=torch.float64, device=DEV).index_add_(0, pos, g.double().abs())
    k = int(np.bincount(np.where(idx_np < 0, idx_np + m, idx_np), minlength=m).max())
    err = (gf.double() - ref).abs()
    bar = k * U32 * s + (U16 * ref.abs() + 2.0 ** -25 if dtype == torch.float16 else 0.0)
    print(f"gather m={m} n={n} c={c} {dtype}: worst err/bar {float((err / bar.clamp_min(1e-300)).max()):.3g}, longest sum {k}")
    assert bool((err <= bar).all())
    if m > 10:
        assert bool((gf[7] == 0).all())
