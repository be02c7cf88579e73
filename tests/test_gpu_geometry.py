"""The overlapping-window `spdownsample` (ts_downsample_windows) and the convolutions over its maps - kernel 3 / stride 2,
anisotropic strides, anisotropic kernels - on the device, against tests/golden/ops_geometry.npz (the real reference) and the
numpy restatement of tests/test_geometry_host.py.

Bars: coordinates and kernel maps bit for bit; fp32 convolutions 1e-5 of the tensor's scale (test_gpu_ops.py's `close`, the bar
of test_conv_golden); half storage 4e-3 against a float64 evaluation on the half-rounded inputs (the bar of the half products in
test_gpu_ops.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ts_oracle as O  # noqa: E402
from test_geometry_host import PLAIN, STRIDED, cap, g, ntuple, windows_ref, windows_ref_candidates  # noqa: E402,F401  (g: the fixture)
from test_gpu_ops import T, close, same  # noqa: E402

ONES = (1, 1, 1)


@pytest.fixture(scope="module")
def F():
    from taseg_amd.torchsparse.nn import functional
    return functional


def sparse(feats, coords, stride=1):
    from taseg_amd.torchsparse import SparseTensor
    st = SparseTensor(feats, coords, stride)
    st.cmaps[st.stride] = st.coords
    return st


def cloud(n, seed, lo=-7, side=24):
    """n distinct voxels of two scenes in [lo, lo + side)^3: a negative batch-wide minimum"""
    rs = np.random.RandomState(seed)
    cells = rs.choice(2 * side ** 3, n, replace=False)
    b, cells = cells // side ** 3, cells % side ** 3
    xyz = np.stack(np.unravel_index(cells, (side, side, side)), 1) + lo
    return np.concatenate([xyz, b[:, None]], 1).astype(np.int32)


# --------------------------------------------------------------------------- coordinates
@pytest.mark.parametrize("tag", sorted(STRIDED))
def test_coordinates_equal_the_reference(F, g, tag):
    kernel, stride, ts = STRIDED[tag]
    got = F.spdownsample(T(g[f"{tag}_coords_in"]), stride, kernel, ts)
    assert got.dtype == torch.int32 and got.is_cuda
    same(got, g[f"{tag}_coords"])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("kernel,stride", [(3, 2), (3, (2, 2, 1))])
def test_coordinates_at_the_block_edges(F, n, kernel, stride):
    c = cloud(257, 3)[:n]
    got = F.spdownsample(T(c).view(-1, 4), stride, kernel, 1)
    assert got.shape[1] == 4 and got.dtype == torch.int32
    same(got, windows_ref(c, stride, kernel, 1))


@pytest.mark.parametrize("kernel,stride,ts", [(5, 2, 1), (1, 2, 1), ((3, 1, 3), (2, 1, 2), (2, 2, 1)), (3, (2, 2, 1), (2, 2, 1)),
                                              (3, 2, 2), (4, 3, 1), ((2, 5, 1), (3, 3, 2), 1)])
def test_coordinates_of_other_geometries(F, kernel, stride, ts):
    """kernel 5 (27 candidates per row), kernel 1 / stride 2 (the overlapping branch with one offset), input tensor strides 2 and
    (2, 2, 1), an even kernel; the cloud's minimum is negative and the result may be larger than the input"""
    c = cloud(700, 11).astype(np.int64)
    c[:, :3] *= np.array(ntuple(ts))
    c = c.astype(np.int32)
    want = windows_ref(c, stride, kernel, ts)
    assert c[:, :3].min() < 0 and len(want) <= cap(kernel, stride) * len(c)
    same(F.spdownsample(T(c), stride, kernel, ts), want)


def test_coordinates_of_a_cloud_larger_than_one_grid(F):
    """more rows than the minimum pass has threads (1024 x 256) and more slots than the key pass has (2048 x 256): both walk
    their grid-stride loops"""
    c = cloud(270000, 5, lo=-9, side=64)
    assert len(c) > 1024 * 256
    got = F.spdownsample(T(c), 2, 3, 1)
    same(got, windows_ref_candidates(c, 2, 3, 1))


def test_coordinate_outside_the_pack_range_is_refused(F):
    c = cloud(300, 2)
    c[17, 0] = (1 << 17) - 1                        # its candidate x + 1 = 2^17 is on the stride-2 grid and outside ts_pack's range
    with pytest.raises(ValueError):
        F.spdownsample(T(c), 2, 3, 1)
    c[17, 0] = (1 << 17) - 2                        # x itself is kept and the last coordinate inside the range; x + 2 is no candidate
    same(F.spdownsample(T(c), 2, 3, 1), windows_ref(c, 2, 3, 1))
    for bad in (dict(kernel_size=6), dict(kernel_size=(3, 0, 3)), dict(stride=(2, 0, 2))):
        with pytest.raises(ValueError):
            F.spdownsample(T(c), **{"stride": 2, "kernel_size": 3, **bad})


# --------------------------------------------------------------------------- kernel maps and fp32 convolutions
def run_golden(F, g, tag):
    strided = tag in STRIDED
    kernel, stride, ts = STRIDED[tag] if strided else (PLAIN[tag], ONES, ONES)
    src = g[f"{tag}_coords_in"] if strided else g["coords"]
    x = T(g["c_x"] if tag == "c" else g["x"]).requires_grad_()
    w = T(g[f"{tag}_w"]).requires_grad_()
    st = sparse(x, T(src), ts)
    y = F.conv3d(st, w, kernel, stride=stride)
    return st, x, w, y, st.kmaps[(ntuple(ts), ntuple(kernel), ntuple(stride), ONES)]


@pytest.mark.parametrize("tag", sorted(STRIDED) + sorted(PLAIN))
def test_kernel_map_equals_the_reference(F, g, tag):
    st, _, _, y, km = run_golden(F, g, tag)
    want = g[f"{tag}_nbmaps"]
    assert km.total == len(want) and km.cls is None and km.direct is None
    same(km.nbmaps_buf[:km.total], want)
    same(km.nbsizes_dev, g[f"{tag}_nbsizes"])
    same(km.nbmaps, want.astype(np.int64))
    if tag in STRIDED:
        same(y.C, g[f"{tag}_coords"])
        assert km.sizes == (len(g[f"{tag}_coords_in"]), len(g[f"{tag}_coords"]))
    else:
        assert y.C is st.C


@pytest.mark.parametrize("tag", sorted(STRIDED) + sorted(PLAIN))
def test_fp32_convolution_equals_the_reference(F, g, tag):
    st, x, w, y, _ = run_golden(F, g, tag)
    assert y.F.dtype == torch.float32
    close(y.F, g[f"{tag}_y"])
    gy = T(g[f"{tag}_gy"] if tag in STRIDED else g["e_gy"])
    gx, gw = torch.autograd.grad(y.F, (x, w), gy, retain_graph=True)
    close(gx, g[f"{tag}_gx"])
    close(gw, g[f"{tag}_gw"])
    if tag not in STRIDED:
        return
    kernel, stride, _ = STRIDED[tag]
    wu = T(g[f"{tag}_wu"]).requires_grad_()
    yu = F.conv3d(y, wu, kernel, stride=stride, transposed=True)          # through the cached map (conv.py:184-192)
    assert yu.C is st.C and yu.stride == st.stride
    close(yu.F, g[f"{tag}_yu"])
    ugx, ugw, ugwu = torch.autograd.grad(yu.F, (x, w, wu), T(g["c_gyu"] if tag == "c" else g["gyu"]))
    close(ugx, g[f"{tag}_ugx"])
    close(ugw, g[f"{tag}_ugw"])
    close(ugwu, g[f"{tag}_ugwu"])


GEOMETRIES = [((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (2, 2, 1)), ((3, 1, 3), (2, 1, 2)), ((1, 3, 3), ONES), ((3, 1, 3), ONES),
              ((1, 1, 3), ONES), ((1, 3, 1), ONES), ((3, 1, 1), ONES)]


@pytest.mark.parametrize("ts", [ONES, (2, 2, 2), (2, 2, 1)])
@pytest.mark.parametrize("kernel,stride", GEOMETRIES)
def test_every_geometry_at_every_input_stride(F, g, kernel, stride, ts):
    """coordinates against the restatement, the map and y / gx / gw (and the transposed convolution back up) against the oracle
    in float64, on the fixture's cloud scaled to the input tensor stride"""
    c = g["coords"].astype(np.int64)
    c[:, :3] *= np.array(ts)
    c = c.astype(np.int32)
    rs = np.random.RandomState(sum(kernel) * 7 + sum(stride) * 3 + sum(ts))
    k = int(np.prod(kernel))
    xn, wn, wun = rs.randn(len(c), 8).astype(np.float32), (rs.randn(k, 8, 16) * 0.2).astype(np.float32), \
        (rs.randn(k, 16, 8) * 0.2).astype(np.float32)
    x, w, wu = T(xn).requires_grad_(), T(wn).requires_grad_(), T(wun).requires_grad_()
    st = sparse(x, T(c), ts)
    y = F.conv3d(st, w, kernel, stride=stride)
    dst = c if stride == ONES else windows_ref(c, stride, kernel, ts)
    same(y.C, dst)
    _, nbmaps, nbsizes = O.build_kmap(c, dst, O.get_kernel_offsets(kernel, ts))
    km = st.kmaps[(ts, kernel, stride, ONES)]
    same(km.nbmaps, nbmaps)
    same(km.nbsizes, nbsizes)
    sizes = (len(c), len(dst))
    y64 = O.conv_forward(xn.astype(np.float64), wn, nbmaps, nbsizes, sizes)
    close(y.F, y64)
    gyn = rs.randn(*y64.shape).astype(np.float32)
    gx, gw = torch.autograd.grad(y.F, (x, w), T(gyn), retain_graph=True)
    gx64, gw64 = O.conv_backward(xn.astype(np.float64), wn, gyn, nbmaps, nbsizes)
    close(gx, gx64)
    close(gw, gw64)
    if stride == ONES:
        return
    yu = F.conv3d(y, wu, kernel, stride=stride, transposed=True)
    assert yu.C is st.C
    yn = y.F.detach().cpu().numpy().astype(np.float64)
    close(yu.F, O.conv_forward(yn, wun, nbmaps, nbsizes, sizes, transposed=True))
    gun = rs.randn(len(c), 8).astype(np.float32)
    gyd, gwu = torch.autograd.grad(yu.F, (y.F, wu), T(gun))
    gyd64, gwu64 = O.conv_backward(yn, wun, gun, nbmaps, nbsizes, transposed=True)
    close(gyd, gyd64)
    close(gwu, gwu64)


# --------------------------------------------------------------------------- modules
def test_module_chain_of_cylinder3d_shape(g):
    """down (kernel 3 / stride 2) -> anisotropic kernel at the coarse stride -> transposed up through the cached map"""
    import taseg_amd.torchsparse.nn as spnn
    torch.manual_seed(3)
    down, mid, up = spnn.Conv3d(16, 32, 3, stride=2).cuda(), spnn.Conv3d(32, 32, (1, 3, 3)).cuda(), \
        spnn.Conv3d(32, 16, 3, stride=2, transposed=True).cuda()
    c = T(g["coords"])
    x = sparse(torch.randn(len(c), 16, device="cuda"), c)
    h = mid(down(x))
    assert h.stride == (2, 2, 2) and h.F.shape == (len(g["a_coords"]), 32)
    same(h.C, g["a_coords"])
    out = up(h)
    assert out.C is x.C and out.stride == ONES and out.F.shape == (len(c), 16) and out.cmaps is x.cmaps
    out.F.square().sum().backward()
    for m in (down, mid, up):
        gk = m.kernel.grad
        assert gk.shape == m.kernel.shape and bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0
    assert set(x.kmaps) == {(ONES, (3, 3, 3), (2, 2, 2), ONES), ((2, 2, 2), (1, 3, 3), ONES, ONES)}


# --------------------------------------------------------------------------- half storage
@pytest.mark.parametrize("tag", ["a", "e133", "e313", "e113"])
def test_half_storage_against_float64(F, g, tag):
    """32 -> 64 channels under autocast: half features and results, fp32 accumulation; against the oracle in float64 on the
    half-rounded x, w and gy"""
    strided = tag in STRIDED
    kernel, stride, _ = STRIDED[tag] if strided else (PLAIN[tag], ONES, ONES)
    src = g["coords"]
    dst = g[f"{tag}_coords"] if strided else src
    rs = np.random.RandomState(len(tag) + kernel[0])
    k = int(np.prod(kernel))
    x = T(rs.randn(len(src), 32).astype(np.float32)).requires_grad_()
    w = T((rs.randn(k, 32, 64) / np.sqrt(32 * k)).astype(np.float32)).requires_grad_()
    gy = T(rs.randn(len(dst), 64).astype(np.float32)).half()
    with torch.autocast("cuda", dtype=torch.float16):
        y = F.conv3d(sparse(x, T(src)), w, kernel, stride=stride)
    assert y.F.dtype == torch.float16 and y.F.shape == (len(dst), 64)
    gx, gw = torch.autograd.grad(y.F, (x, w), gy)
    assert gx.dtype == torch.float32 and gw.dtype == torch.float32
    x64, w64, g64 = (t.detach().half().double().cpu().numpy() for t in (x, w, gy))
    nbmaps, nbsizes = g[f"{tag}_nbmaps"].astype(np.int64), g[f"{tag}_nbsizes"]
    close(y.F.float(), O.conv_forward(x64, w64, nbmaps, nbsizes, (len(src), len(dst))), 4e-3)
    gx64, gw64 = O.conv_backward(x64, w64, g64, nbmaps, nbsizes)
    close(gx, gx64, 4e-3)
    close(gw, gw64, 4e-3)


# --------------------------------------------------------------------------- the existing path, determinism
def test_which_entry_point_each_geometry_calls(F, g, monkeypatch):
    from taseg_amd import _lib as L
    lib = L.load()
    calls = []
    for name in ("ts_downsample", "ts_downsample_windows"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    c = T(g["coords"])
    x = torch.randn(len(c), 8, device="cuda")
    w = {k: torch.randn(k, 8, 16, device="cuda") for k in (8, 27)}
    F.conv3d(sparse(x, c), w[8], 2, stride=2)
    assert calls == ["ts_downsample"]
    F.spdownsample(c, 2, 2, 1)
    F.spdownsample(c, 1, 3, 1)
    F.spdownsample(c, (2, 1, 2), (2, 3, 2), 1)
    assert calls == ["ts_downsample"] * 4
    del calls[:]
    F.conv3d(sparse(x, c), w[27], 3)
    assert calls == []
    F.conv3d(sparse(x, c), w[27], 3, stride=2)
    assert calls == ["ts_downsample_windows"]


def test_same_bits_every_run(F, g):
    c, x, w = T(g["coords"]), T(g["x"]), T(g["a_w"])
    runs = []
    for _ in range(2):
        y = F.conv3d(sparse(x, c), w, 3, stride=2)
        runs.append((y.C.clone(), y.F.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    big = T(cloud(20000, 9, side=40))
    assert torch.equal(F.spdownsample(big, (2, 2, 1), 3, 1), F.spdownsample(big, (2, 2, 1), 3, 1))
