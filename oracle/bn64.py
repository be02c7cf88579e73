"""Float64 reference of the sparse BatchNorm (+ residual) (+ ReLU) kernels of csrc/bn.hip and the length of their longest chain of
float additions - test infrastructure, not product code.  Tensor ops of torch in double, on whatever device the operands live on (no
functional.batch_norm, no autograd; tests/test_gpu_bn_float64.py checks it against nn.BatchNorm1d in double under autograd on the CPU).
Nothing of taseg_amd is imported.  tests/test_gpu_bn_float64.py holds the kernels against it and derives the bars in its docstring;
oracle/block64.py composes the fused conv-block reference from it.

The layout of the reductions (bn.hip): a launch is cut into <= 512 slices of at least 32 rows, a slice's length is a whole number of
passes; one thread holds 4 (half: 8) channels of a row, so a pass of a 256-thread workgroup covers rpp = 256 // (c / 4) rows
(256 // (c / 8)); a lane adds its rows of the slice in float, the rpp lanes of a channel are added in float, the slices in double.
The longest chain of float additions is therefore

    rows = ceil(max(ceil(n / 512), 32) / rpp) * rpp          rows per slice
    LAMBDA(n, c) = rows / rpp  +  rpp  +  8                  rows a lane adds + lanes added per workgroup + elementwise operations

(8: the product inside the sum, x - mean, * invstd, * weight, + bias, + residual, the two conversions of a statistic to float).  It
is evaluated from n and c alone."""


def bn_ref64(x, residual, weight, bias, relu, eps, gy, relu_from=None):
    """act(BatchNorm_train(x) [+ residual]) and its backward in float64 from the exact values of the inputs:
    (y, gx, gres, gw, gb, mean, var) and the same expressions on absolute values (sy, sgx, sgres, sgw, sgb, smean, svar).
    var is the biased variance; gres is None without a residual.  relu_from: the tensor whose sign decides the ReLU's derivative
    (default: the reference's own y)."""
    x, g = x.double(), gy.double()
    w, b = weight.double(), bias.double()
    n = x.shape[0]
    mean, smean = x.mean(0), x.abs().mean(0)
    xc = x - mean
    var = xc.square().mean(0)
    svar = x.square().mean(0) + mean.square()
    invstd = (var + eps).rsqrt()
    sis = 0.5 * invstd ** 3 * svar                                     # var's error seen through invstd
    xa = x.abs() + smean                                               # |x| + E|x|: x - mean on absolute values
    del x
    y = xc * invstd * w + b
    sy = xa * invstd * w.abs() + xc.abs() * sis * w.abs() + b.abs()
    if residual is not None:
        y += residual.double()
        sy += residual.double().abs()
    if relu:
        y = y.clamp_min(0.0)
        g = g * ((y if relu_from is None else relu_from) > 0)
    gres, sgres = (g, g.abs()) if residual is not None else (None, None)
    gb, sgb = g.sum(0), g.abs().sum(0)
    gac, sgac = (g * xc).sum(0), (g.abs() * xa).sum(0)
    gw, sgw = gac * invstd, sgac * invstd + gac.abs() * sis
    k = gac / n * invstd.square()
    sk = sgac / n * invstd.square() + gac.abs() / n * 2.0 * invstd * sis
    inner = g - gb / n - xc * k
    sinner = g.abs() + sgb / n + xa * k.abs() + xc.abs() * sk
    del xa, xc
    gx = inner * invstd * w
    sgx = sinner * invstd * w.abs() + inner.abs() * sis * w.abs()
    del inner, sinner
    return (y, gx, gres, gw, gb, mean, var), (sy, sgx, sgres, sgw, sgb, smean, svar)


def running_ref64(rm0, rv0, mean, var, smean, svar, n, momentum, passes=1):
    """nn.BatchNorm1d's running statistics after `passes` training passes over the same batch, each applied to the result of the one
    before (running_var takes the unbiased variance; the biased one when n = 1, as the kernels document), and their S"""
    unbiased = n / (n - 1.0) if n > 1 else 1.0
    rm, rv, srm, srv = rm0.double(), rv0.double(), rm0.double().abs(), rv0.double().abs()
    for _ in range(passes):
        rm, srm = (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * srm + momentum * smean
        rv, srv = (1.0 - momentum) * rv + momentum * var * unbiased, (1.0 - momentum) * srv + momentum * svar * unbiased
    return rm, rv, srm, srv


def LAMBDA(n, c, half):
    """LAMBDA(n, c) of the module docstring (half: 8 channels per thread)"""
    rpp = 256 // (c // (8 if half else 4))
    rows = -(-max(-(-n // 512), 32) // rpp) * rpp
    return rows // rpp + rpp + 8
