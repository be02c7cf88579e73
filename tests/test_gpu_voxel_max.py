"""ts_voxelize_max_forward / _backward (csrc/cylinder.hip) against a reference on the CPU - EXACT equality: a maximum and a copy round
nothing.  out[v, ch] = max of feat[i, ch] over the rows with idx[i] == v, arg[v, ch] = the SMALLEST such row that attains it,
0 / -1 for a voxel without rows; grad_feat[i, ch] = grad_out[idx[i], ch] where arg[idx[i], ch] == i, else 0.

Row counts 1, 63, 64, 65, 257, 5000 and channel counts 4, 16, 256 (one lane, a quarter wave and a whole wave per voxel; several
voxels per workgroup and one).  Populations, spread over the row counts (`population`): voxels of one row, a voxel of 65 rows, a
voxel of more than 256 rows, an empty voxel, skipped rows (idx -1).  Column 0 is negative in every row and column 1 in every row of
the first voxel (a maximum that starts from zero fails there); inside a voxel some rows are copies of an earlier one (ties in every
channel: the smaller index wins and alone receives the gradient).  The rows of a voxel are scattered over the matrix.  Outputs are
allocated over NaN-filled blocks, so an element the kernels leave out shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257, 5000)
CHANNELS = (4, 16, 256)


def population(n, seed):
    """idx [n] (voxel of every row, -1 = skipped) and the voxel count m, with the populations of the module docstring"""
    rs = np.random.RandomState(seed)
    if n == 1:
        return np.array([0], np.int32), 2                          # one voxel of one row, one empty voxel
    if n in (65, 257):
        return np.full(n, 1, np.int32), 3                          # ONE voxel of 65 / of more than 256 rows between two empty ones
    big = [300, 65] if n >= 5000 else [n // 2]
    skipped = max(3, n // 50)
    idx = []
    for v, size in enumerate(big):
        idx += [v] * size
    idx += [-1] * skipped
    v = len(big) + 1                                               # voxel len(big) stays empty
    rest = n - len(idx)
    pairs = rest // 6
    for _ in range(pairs):                                         # voxels of two rows
        idx += [v, v]
        v += 1
    while len(idx) < n:                                            # voxels of one row
        idx.append(v)
        v += 1
    idx = np.array(idx, np.int32)
    rs.shuffle(idx)
    return idx, v + 1                                              # ... and the last voxel is empty too


def features(n, c, idx, seed, dtype):
    rs = np.random.RandomState(seed)
    f = rs.randn(n, c).astype(np.float32)
    f[:, 0] = -np.abs(f[:, 0]) - 0.5                               # all-negative column
    first = idx == idx[idx >= 0][0]
    f[first, 1] = -np.abs(f[first, 1]) - 0.25                      # ... and one that is negative in one voxel only
    for v in np.unique(idx[idx >= 0])[:40]:                        # copies inside a voxel: ties in every channel
        rows = np.nonzero(idx == v)[0]
        if len(rows) >= 2:
            a, b = rs.choice(rows, 2, replace=False)
            f[b] = f[a]
    t = torch.from_numpy(f).to(dtype)
    return t


def reference(feat, idx, m):
    """(out, arg) on the CPU; numpy's argmax returns the first maximum, the rows are walked in ascending order"""
    f = feat.float().numpy()
    out = np.zeros((m, f.shape[1]), np.float32)
    arg = np.full((m, f.shape[1]), -1, np.int32)
    for v in range(m):
        rows = np.nonzero(idx == v)[0]
        if len(rows):
            out[v] = f[rows].max(0)
            arg[v] = rows[f[rows].argmax(0)]
    return out, arg


def reference_grad(gout, arg, n):
    go = gout.float().numpy()
    g = np.zeros((n, go.shape[1]), np.float32)
    v, ch = np.nonzero(arg >= 0)
    g[arg[v, ch], ch] = go[v, ch]
    return g


def poison(*shapes_dtypes):
    for shape, dtype in shapes_dtypes:
        t = torch.full(shape, float("nan") if dtype.is_floating_point else -77, dtype=dtype, device="cuda")
        del t


def run(feat, idx, m, gout):
    from taseg_amd import backend as B
    f, i, g = feat.cuda(), torch.from_numpy(idx).cuda(), gout.cuda()
    poison(((m, f.shape[1]), f.dtype), ((m, f.shape[1]), torch.int32))
    out, arg = B.voxelize_max_forward(f, i, m)
    poison((tuple(f.shape), f.dtype))
    gf = B.voxelize_max_backward(g, i, arg, f.shape[0])
    torch.cuda.synchronize()
    return out.cpu(), arg.cpu(), gf.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("n", ROWS)
def test_max_arg_and_gradient_are_exact(n, c, dtype):
    from taseg_amd import backend as B
    idx, m = population(n, 7 * n + c)
    feat = features(n, c, idx, n + c, dtype)
    gout = torch.from_numpy(np.random.RandomState(3).randn(m, c).astype(np.float32)).to(dtype)
    if dtype == torch.float16 and c % 8:
        with pytest.raises(B.BackendError, match="multiple of 8"):
            B.voxelize_max_forward(feat.cuda(), torch.from_numpy(idx).cuda(), m)
        return
    want_out, want_arg = reference(feat, idx, m)
    want_grad = reference_grad(gout, want_arg, n)
    out, arg, gf = run(feat, idx, m, gout)
    assert out.dtype == dtype and gf.dtype == dtype and arg.dtype == torch.int32
    assert np.array_equal(out.float().numpy(), want_out)
    assert np.array_equal(arg.numpy(), want_arg)
    assert np.array_equal(gf.float().numpy(), want_grad)
    # what the populations promise
    empty = np.setdiff1d(np.arange(m), idx)
    assert len(empty) >= 1 and (want_out[empty] == 0).all() and (want_arg[empty] == -1).all()
    assert (want_grad[idx < 0] == 0).all() and (want_out[np.unique(idx[idx >= 0]), 0] < 0).all()
    again = run(feat, idx, m, gout)
    assert all(torch.equal(a, b) for a, b in zip((out, arg, gf), again)), "two calls gave different bits"


def test_populations_cover_what_the_issue_lists():
    sizes = {n: np.bincount(population(n, 7 * n + 4)[0][population(n, 7 * n + 4)[0] >= 0]) for n in ROWS}
    assert any((s == 1).any() for s in sizes.values()) and any((s == 65).any() for s in sizes.values())
    assert any((s > 256).any() for s in sizes.values()) and all((population(n, 1)[0] == -1).any() for n in (63, 64, 5000))


def test_nine_channels_are_refused_not_wrong():
    from taseg_amd import backend as B
    feat = torch.randn(10, 9, device="cuda")
    idx = torch.zeros(10, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BackendError, match="multiple of 4"):
        B.voxelize_max_forward(feat, idx, 1)
    with pytest.raises(B.BackendError, match="multiple of 4"):
        B.voxelize_max_backward(torch.randn(1, 9, device="cuda"), idx, torch.zeros((1, 9), dtype=torch.int32, device="cuda"), 10)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
def test_autograd_node_equals_the_tensor_ops(dtype):
    """functional.spvoxelize_max under autograd against scatter_reduce('amax') - the form the private switch puts in its place - on rows
    without ties (torch splits a tied gradient); out-of-range voxel ids take no part"""
    from taseg_amd.torchsparse.nn import functional as F
    rs = np.random.RandomState(11)
    n, c, m = 3000, 32, 700
    idx = torch.from_numpy(rs.randint(-1, m + 2, size=n).astype(np.int32)).cuda()          # -1 and m, m + 1: no voxel
    base = torch.from_numpy(rs.permutation(n * c).reshape(n, c).astype(np.float32) / 64.0 - 700.0).to(dtype)
    if dtype != torch.float32:                                      # distinct values half holds exactly (steps of 1/4 below 512)
        base = torch.from_numpy(rs.permutation(n)[:, None].astype(np.float32) / 4.0 - 300.0).to(dtype).expand(n, c).contiguous()
    gout = torch.from_numpy(rs.randn(m, c).astype(np.float32)).to(dtype).cuda()
    x1 = base.cuda().requires_grad_()
    y1 = F.spvoxelize_max(x1, idx, m)
    (g1,) = torch.autograd.grad(y1, x1, gout)
    inside = (idx >= 0) & (idx < m)
    x2 = base.cuda().requires_grad_()
    y2 = x2.new_zeros((m, c)).scatter_reduce(0, idx[inside].long().unsqueeze(1).expand(-1, c), x2[inside], "amax", include_self=False)
    (g2,) = torch.autograd.grad(y2, x2, gout)
    assert y1.dtype == dtype and g1.dtype == dtype
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
