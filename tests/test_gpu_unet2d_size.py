"""UNet2D - TIAF's camera branch - at the size the TIAF training step runs it, against float64.

* Training: MinkUNetMsMm under FlatSGD, step for step against torch.optim.SGD + clip_grad_norm_ (+ GradScaler): every parameter with a
  gradient moves - the camera branch's convolution weights included - and stays a view of its flat bucket.
* Each of the library's 2-D nodes (unet2d._Conv3x3C32Rows, _Conv1x1C32Act, _Conv3x3Rows, _LeakyBatchNormRows, _AvgPool3s2Rows,
  _ShuffleCatRows) at the shapes of the TIAF step - T = 10 frames (batch 2 x 5 cameras) of 384 x 1280, half, channels-last - through
  the autograd Functions the model uses.  References are float64 on the device; bars are elementwise and come from error analysis:
  with S the same operation evaluated on absolute values, a half result is within 2^-11 |ref| + 2^-14 S, an fp32 one within 2^-14 S
  (fp32 sums of exact half products: 2^-14 leaves the sums of a few million terms their statistical error and nothing else).  The
  convolutions' inputs and gradients have a mean of half their spread: their weight-gradient sums are coherent, S ~ 2.6 |ref|, so a
  lost border row of a frame (1/384 of the sum) is ~ 5 bars off (the half weight gradient's own rounding, 2^-11 |ref|, is most of the
  bar: the kernels measure 0.61 of it) - with zero-mean data the lost row would be a random walk smaller than the bar.  The
  convolutions' forward and data gradient are evaluated on sampled output rows (image borders, the middle, 8 random rows per frame:
  every 4- / 8-row tile seam class and all columns, so every 32-pixel segment seam), their weight gradient in full.
* The whole branch (encoder, both decoders, classifier) at a small size with every family routed, gradients included: no further
  from float64 than the vendor's half path is.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from taseg_amd.data.synthetic import TIAF_CFG, fill_parameters, make_model_cfg  # noqa: E402

T, H, W = 10, 384, 1280
REL, ABS = 2.0 ** -11, 2.0 ** -14
SUB = 2.0 ** -25                # half rounding below the smallest normal (6.1e-5): an absolute error of up to half its spacing 2^-24
SLOPE = 0.01                    # nn.LeakyReLU()'s
GS = 2.0 ** -8                  # scale of the convolutions' output gradients: coherent sums over 4.9 M pixels stay in half's range


# ------------------------------------------------------------------------------------------------------------------ helpers

def _randn(shape, seed, scale=1.0, shift=0.0, dtype=torch.float16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, generator=g, device="cuda") * scale + shift
    return x.to(dtype).contiguous(memory_format=torch.channels_last) if len(shape) == 4 else x.to(dtype)


def _check(name, got, ref, s, rel=REL, mask=None):
    """|got - ref| <= rel |ref| + 2^-14 S elementwise (where `mask`), + 2^-25 for a half result; returns the worst err / bar"""
    err = (got.double() - ref).abs()
    bar = rel * ref.abs() + ABS * s + (SUB if got.dtype == torch.float16 else 0.0)
    ok = err <= bar
    if mask is not None:
        ok = ok | ~mask
        err = err * mask
    worst = float((err / bar.clamp_min(1e-300)).max())
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:4].tolist()
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bar, worst err/bar {worst:.3g}, "
                             f"e.g. at {bad}")
    print(f"{name}: worst err/bar {worst:.3g}")
    return worst


def _rows(h, t, seed):
    """output rows checked per frame: borders, the middle, 8 random ones"""
    fixed = {0, 1, 2, 3, 4, h // 2, h - 3, h - 2, h - 1}
    g = torch.Generator().manual_seed(seed)
    return [sorted(fixed | set(torch.randint(0, h, (8,), generator=g).tolist())) for _ in range(t)]


def _conv_rows64(x, w64, b64, dilation, rows):
    """float64 Conv2d(x, w64, b64, stride 1, padding = dilation * (k // 2), dilation) at the given output rows of every frame, and the
    same of |x|, |w|, |b| (S): two lists of [R, C_out, W], one per frame - each from the 1 + 2d input rows around the row (zero rows
    past the image's edge)"""
    t, c, h, w = x.shape
    k = w64.shape[2] // 2
    offs = dilation * torch.arange(-k, k + 1, device=x.device)
    outs, sums = [], []
    for f in range(t):
        taps = torch.tensor(rows[f], device=x.device)[:, None] + offs              # [R, 2k + 1]
        ok = ((taps >= 0) & (taps < h)).double()
        xr = (x[f][:, taps.clamp(0, h - 1), :].double() * ok[None, :, :, None]).permute(1, 0, 2, 3)   # [R, C, 2k + 1, W]
        pad, dil = (0, dilation * k), (1, dilation)          # (the rows are gathered tap by tap: no dilation across them)
        outs.append(F.conv2d(xr, w64, b64, padding=pad, dilation=dil)[:, :, 0])
        sums.append(F.conv2d(xr.abs(), w64.abs(), None if b64 is None else b64.abs(), padding=pad, dilation=dil)[:, :, 0])
    return outs, sums


def _at_rows(y, rows):
    """[R, C, W] per frame of a [T, C, H, W] map"""
    return [y[f][:, torch.tensor(rows[f], device=y.device), :].permute(1, 0, 2) for f in range(y.shape[0])]


def _wgrad64(x, gy, k, dilation, chunk=2):
    """float64 weight and bias gradient of Conv2d(k x k, stride 1, padding = dilation * (k // 2)) from x [T, Ci, H, W] and gy
    [T, Co, H, W] as (2k + 1)^2 GEMMs of shifted x against gy, frames in chunks; with their sums of absolute terms"""
    t, ci, h, w = x.shape
    co = gy.shape[1]
    kk, p = 2 * k + 1, dilation * k
    gw = torch.zeros(co, ci, kk, kk, dtype=torch.float64, device=x.device)
    sw, gb, sb = torch.zeros_like(gw), torch.zeros(co, dtype=torch.float64, device=x.device), torch.zeros(co, dtype=torch.float64, device=x.device)
    for f0 in range(0, t, chunk):
        xp = F.pad(x[f0:f0 + chunk].permute(0, 2, 3, 1).double(), (0, 0, p, p, p, p))         # [tc, H + 2p, W + 2p, Ci]
        g = gy[f0:f0 + chunk].permute(0, 2, 3, 1).reshape(-1, co).double()
        ga = g.abs()
        for ky in range(kk):
            for kx in range(kk):
                xt = xp[:, ky * dilation:ky * dilation + h, kx * dilation:kx * dilation + w, :].reshape(-1, ci)
                gw[:, :, ky, kx] += g.T @ xt
                sw[:, :, ky, kx] += ga.T @ xt.abs()
        gb += g.sum(0)
        sb += ga.sum(0)
        del xp, g, ga
    return gw, sw, gb, sb


def _twice(fn):
    """run a node's forward + backward twice: same bits (every node of the library is run-to-run deterministic)"""
    a, b = fn(), fn()
    for i, (p, q) in enumerate(zip(a, b)):
        assert p is None and q is None or torch.equal(p, q), f"output {i} differs between two runs"
    return a


# ------------------------------------------------------------------------------------------------------------------ training

def _tiaf_batch(g):
    from taseg_amd.torchsparse import SparseTensor
    dev = "cuda"
    coords = torch.from_numpy(g["coords"]).to(dev)
    fov_coords = torch.from_numpy(g["fov_coords"]).to(dev)
    return {
        "lidar_ms": SparseTensor(torch.from_numpy(g["feats"]).to(dev), coords),
        "targets_ms": SparseTensor(torch.from_numpy(g["labels"]).to(dev), coords),
        "lidar_fov_ms": SparseTensor(torch.from_numpy(g["fov_feats"]).to(dev), fov_coords),
        "image_ms": torch.from_numpy(g["images"]).to(dev),
        "semantic_map_ms": torch.from_numpy(g["semantic"]).to(dev),
        "offset_img": torch.from_numpy(g["offset_img"]).to(dev),
        "offset_ms": torch.tensor([0], device=dev),
    }


def _build_mm():
    from taseg_amd.pcseg.model import build_network
    cfg = make_model_cfg("MinkUNetMsMm", in_dim=5, cr=1.0, num_layer=[1] * 8, **TIAF_CFG)
    model = fill_parameters(build_network(cfg, 20), seed=3).cuda()
    model.train()
    for m in model.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
            m.eval()
    return model


@pytest.mark.parametrize("amp", [False, True])
def test_flat_sgd_trains_every_tiaf_parameter_like_torch_sgd(g_minkunet_ms_mm, amp):
    """MinkUNetMsMm twice from one seed on the golden batch: twin A under torch.optim.SGD(momentum 0.9, weight decay 1e-4) +
    clip_grad_norm_(10) (+ GradScaler), twin B under FlatSGD(max_norm 10, amp).  Three steps; after each, every parameter that had a
    gradient - the camera branch's convolution weights among them - moved from where it was, by twin A's update (elementwise, the bars
    of test_flat_sgd_matches_torch_sgd_clip_and_gradscaler), is still a view of its slice of the flat bucket with its own strides, and
    state_dict() returns the updated values.  Both twins run forward and backward; twin A's optimizer is handed twin B's gradients
    (where it has a gradient itself): the optimizers are what is compared - the vendor's half convolutions are not bit-reproducible
    from one call to the next."""
    from taseg_amd.optim import FlatSGD
    lr, steps = 0.05, 3
    a, b = _build_mm(), _build_mm()
    names = [n for n, _ in b.named_parameters()]
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    ref_opt = torch.optim.SGD(a.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=amp, init_scale=1024.0)
    ours = FlatSGD(b, lr=lr, momentum=0.9, weight_decay=1e-4, max_norm=10.0, amp=amp, init_scale=1024.0)
    slot = {}
    for bk in ours.reducer.buckets:
        for p, off in zip(bk["params"], bk["offsets"]):
            slot[id(p)] = (bk, off)
    image_convs = [n for n in names if n.startswith("image_backbone.") and pb[n].dim() == 4]
    assert len(image_convs) == 24
    applied = 0
    for step in range(steps):
        before_a = {n: p.detach().clone() for n, p in pa.items()}
        before_b = {n: p.detach().clone() for n, p in pb.items()}
        ref_opt.zero_grad(set_to_none=True)
        ours.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            ret_a, _, _ = a(_tiaf_batch(g_minkunet_ms_mm))
            ret_b, _, _ = b(_tiaf_batch(g_minkunet_ms_mm))
        scaler.scale(ret_a["loss"].float()).backward()
        (ret_b["loss"].float() * ours.loss_scale()).backward()
        used = [n for n in names if pa[n].grad is not None]
        assert sorted(used) == sorted(n for n in names if pb[n].grad is not None) and set(image_convs) <= set(used)
        with torch.no_grad():
            for n in used:
                pa[n].grad.copy_(pb[n].grad)
        nonzero = {n for n in used if bool(pb[n].grad.ne(0).any())}
        scale = float(scaler.get_scale()) if amp else 1.0
        scaler.unscale_(ref_opt)
        torch.nn.utils.clip_grad_norm_(a.parameters(), 10.0)
        scaler.step(ref_opt)
        scaler.update()
        ours.step()
        if amp:
            assert float(ours.state[0]) == float(scaler.get_scale()), step
        if amp and float(scaler.get_scale()) < scale:         # non-finite gradients: both skipped the step
            assert all(torch.equal(pb[n].detach(), before_b[n]) and torch.equal(pa[n].detach(), before_a[n]) for n in names)
            continue
        applied += 1
        frozen = [n for n in sorted(nonzero) if torch.equal(pb[n].detach(), before_b[n])]
        assert not frozen, f"step {step + 1}: parameters with a gradient that did not move under FlatSGD: {frozen}"
        for n in used:
            da, db = pa[n].detach() - before_a[n], pb[n].detach() - before_b[n]
            # the update elementwise (2^-21 |p|: the rounding of the parameter itself), and the parameters as in the small test
            bar = 1e-5 * da.abs() + 2.0 ** -21 * before_a[n].abs() + 1e-9
            assert bool(((db - da).abs() <= bar).all()), (step, n, float((db - da).abs().max()))
            assert torch.allclose(pa[n], pb[n], rtol=1e-5, atol=1e-6), (step, n)
        sd = b.state_dict()
        for n in names:
            p = pb[n]
            bk, off = slot[id(p)]
            # the parameter IS its slice (dense strides of its own layout) and state_dict() saves what the update wrote there
            assert p.data_ptr() == bk["pflat"].data_ptr() + 4 * off, f"step {step + 1}: {n} is not a view of its bucket slice"
            assert p.stride() == torch.empty_like(p, device="meta").stride(), n
            assert torch.equal(sd[n], bk["pflat"][off:off + p.numel()].as_strided(p.shape, p.stride())), n
    assert applied >= 2 and len(nonzero) > 200
    # (the camera branch's weights kept the layout UNet2D gave them at construction: channels-last)
    assert all(pb[n].is_contiguous(memory_format=torch.channels_last) for n in image_convs)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_unet2d_weights_take_the_layout_when_they_move_to_the_device(layout):
    """UNet2D's convolution weights take options.image_layout's memory format in the .cuda() that moves them (on the host they keep the
    contiguous format); conversions after that (.cuda(), .float(), .to(device)) and a forward leave every parameter where it is, so
    FlatSGD built on the moved module keeps its views"""
    from taseg_amd.optim import FlatSGD
    from taseg_amd.options import options
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import UNet2D
    fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
    with options.override(image_layout=layout):
        torch.manual_seed(4)
        net = UNet2D(3, 20)
        assert all(p.is_contiguous() for p in net.parameters())
        net = net.cuda().train()
        convs = [p for p in net.parameters() if p.dim() == 4]
        assert len(convs) == 24 and all(p.is_contiguous(memory_format=fmt) for p in convs)
        opt = FlatSGD(net, lr=0.1, momentum=0.9)
        ptrs = [p.data_ptr() for p in net.parameters()]
        net.cuda().float().to("cuda")
        x = torch.randn(2, 3, 32, 64, device="cuda").contiguous(memory_format=fmt)
        x5, skips = net._encode(x)
        net.classifier(net._decode_u4(net._decode_u2(x5, skips), skips)).square().mean().backward()
        assert [p.data_ptr() for p in net.parameters()] == ptrs
        before = [p.detach().clone() for p in convs]
        opt.step()
        assert all(not torch.equal(p, q) for p, q in zip(convs, before))


def test_flat_sgd_refuses_a_rebound_parameter():
    """a parameter whose .data is rebound after FlatSGD was built (what Module.to(memory_format=...) does to 4-D weights) holds a
    tensor the flat update would never reach: the next step() raises and names the parameter"""
    from taseg_amd.optim import FlatSGD
    torch.manual_seed(2)
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 2, 1)).cuda()
    net.to(memory_format=torch.channels_last)
    opt = FlatSGD(net, lr=0.1, momentum=0.9)
    x = torch.randn(2, 4, 6, 10, device="cuda").contiguous(memory_format=torch.channels_last)
    net(x).square().sum().backward()
    opt.step()                                           # (the layout the parameters had: kept)
    opt.zero_grad()
    net[0].weight.data = net[0].weight.data.contiguous()
    net(x).square().sum().backward()
    with pytest.raises(RuntimeError, match=r"'0\.weight'"):
        opt.step()


# ------------------------------------------------------------------------------------------------------------------ convolutions

@pytest.mark.parametrize("dilation", [1, 2])
def test_conv3x3_c32_at_the_tiaf_shape_vs_float64(dilation):
    """the seven full-resolution 32 -> 32 layers of the stem and stage 1 (unet2d._Conv3x3C32Rows): y, grad x, grad w, grad b"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _Conv3x3C32Rows
    x = _randn((T, 32, H, W), 1, shift=0.5)
    gy = _randn((T, 32, H, W), 2, scale=GS, shift=0.5 * GS)
    w16 = (_randn((32, 32, 3, 3), 3, scale=0.06)).contiguous(memory_format=torch.channels_last)
    bias = _randn((32,), 4, scale=0.1, dtype=torch.float32)

    def run():
        xr, wr, br = x.detach().requires_grad_(), w16.detach().requires_grad_(), bias.detach().requires_grad_()
        y = _Conv3x3C32Rows.apply(xr, wr, br, dilation)
        return (y,) + torch.autograd.grad(y, (xr, wr, br), gy)
    y, gx, gw, gb = _twice(run)
    assert gw.dtype == torch.float16 and gb.dtype == torch.float32
    _check_conv(f"c32 d{dilation}", x, gy, w16, bias, dilation, y, gx, gw, gb, seed=10 + dilation)


def _check_conv(name, x, gy, w16, bias, dilation, y, gx, gw, gb, seed):
    rows = _rows(x.shape[2], x.shape[0], seed)
    w64, b64 = w16.double(), bias.double()
    ref, s = _conv_rows64(x, w64, b64, dilation, rows)
    _check(f"{name} y", torch.cat(_at_rows(y, rows)), torch.cat(ref), torch.cat(s))
    wt = w64.flip(2, 3).transpose(0, 1)                     # data gradient: the flipped, transposed weight over gy
    ref, s = _conv_rows64(gy, wt, None, dilation, rows)
    _check(f"{name} grad x", torch.cat(_at_rows(gx, rows)), torch.cat(ref), torch.cat(s))
    del ref, s
    rgw, sgw, rgb, sgb = _wgrad64(x, gy, w16.shape[2] // 2, dilation)
    _check(f"{name} grad w", gw, rgw, sgw)
    _check(f"{name} grad b", gb, rgb, sgb, rel=0.0)


@pytest.mark.parametrize("c_in,c_out,scale", [(32, 64, 2), (96, 96, 2), (56, 96, 1)], ids=["stage2", "up3", "up4"])
def test_conv3x3_general_at_the_tiaf_shapes_vs_float64(c_in, c_out, scale):
    """the general 3 x 3 kernel (unet2d._Conv3x3Rows) at the layers it carries in the TIAF step: stage2.conv2 32 -> 64 and up3.conv1
    96 -> 96 (two weight-gradient passes) at 192 x 640, up4.conv1 56 -> 96 at 384 x 1280: y, grad x, grad w, grad b"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _Conv3x3Rows
    h, w = H // scale, W // scale
    x = _randn((T, c_in, h, w), 21, shift=0.5)
    gy = _randn((T, c_out, h, w), 22, scale=GS, shift=0.5 * GS)
    w16 = _randn((c_out, c_in, 3, 3), 23, scale=(1.0 / (9 * c_in)) ** 0.5).contiguous(memory_format=torch.channels_last)
    bias = _randn((c_out,), 24, scale=0.1, dtype=torch.float32)

    def run():
        xr, wr, br = x.detach().requires_grad_(), w16.detach().requires_grad_(), bias.detach().requires_grad_()
        y = _Conv3x3Rows.apply(xr, wr, br)
        return (y,) + torch.autograd.grad(y, (xr, wr, br), gy)
    y, gx, gw, gb = _twice(run)
    assert y.shape == (T, c_out, h, w) and gw.dtype == torch.float16 and gb.dtype == torch.float32
    _check_conv(f"general {c_in}->{c_out} at {h}x{w}", x, gy, w16, bias, 1, y, gx, gw, gb, seed=20 + c_in)


def test_conv1x1_c32_leaky_at_the_tiaf_shape_vs_float64():
    """the 1 x 1, 32 -> 32 layers with their LeakyReLU (unet2d._Conv1x1C32Act): y, grad x, grad w, grad b.  Grad x leaves out the
    pixels where a float64 pre-activation lies within the bar of zero: there the slope legitimately follows the rounded output's sign"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _Conv1x1C32Act
    x = _randn((T, 32, H, W), 31, shift=0.5)
    gy = _randn((T, 32, H, W), 32, scale=GS, shift=0.5 * GS)
    w16 = _randn((32, 32, 1, 1), 33, scale=0.18).contiguous(memory_format=torch.channels_last)
    bias = _randn((32,), 34, scale=0.1, dtype=torch.float32)

    def run():
        xr, wr, br = x.detach().requires_grad_(), w16.detach().requires_grad_(), bias.detach().requires_grad_()
        y = _Conv1x1C32Act.apply(xr, wr, br, SLOPE)
        return (y,) + torch.autograd.grad(y, (xr, wr, br), gy)
    y, gx, gw, gb = _twice(run)
    rows = _rows(H, T, 35)
    w64, b64 = w16.double(), bias.double()
    pre, s = _conv_rows64(x, w64, b64, 1, rows)
    pre, s = torch.cat(pre), torch.cat(s)
    slope = torch.where(pre > 0, 1.0, SLOPE).double()
    # (an output within the bar of zero may take the other slope: left out of y, and its pixel out of grad x.  A negative output is
    # rounded twice by design - the activation acts on the half value, as the module pair does: 2^-10 |ref| there)
    _check("c1x1 y", torch.cat(_at_rows(y, rows)), pre * slope, s * slope, rel=torch.where(pre > 0, REL, 2 * REL),
           mask=pre.abs() > ABS * s)
    g64 = torch.cat(_at_rows(gy, rows)).double() * slope                          # [R, 32, W]: the gradient at the layer's output
    ref = torch.einsum("oi,row->riw", w64[:, :, 0, 0], g64)
    sref = torch.einsum("oi,row->riw", w64[:, :, 0, 0].abs(), g64.abs())
    clear = ((pre.abs() > ABS * s).all(dim=1, keepdim=True)).expand_as(ref)
    assert float(clear.double().mean()) > 0.99
    _check("c1x1 grad x", torch.cat(_at_rows(gx, rows)), ref, sref, mask=clear)
    del pre, s, slope, g64, ref, sref, clear
    # weight and bias gradient: the full sums, with the slope of the float64 pre-activation
    gw64, sw64 = torch.zeros(32, 32, dtype=torch.float64, device="cuda"), torch.zeros(32, 32, dtype=torch.float64, device="cuda")
    gb64, sb64 = torch.zeros(32, dtype=torch.float64, device="cuda"), torch.zeros(32, dtype=torch.float64, device="cuda")
    for f0 in range(0, T, 2):
        xf = x[f0:f0 + 2].permute(0, 2, 3, 1).reshape(-1, 32).double()
        p = xf @ w64[:, :, 0, 0].T + b64
        g = gy[f0:f0 + 2].permute(0, 2, 3, 1).reshape(-1, 32).double() * torch.where(p > 0, 1.0, SLOPE).double()
        gw64 += g.T @ xf
        sw64 += g.abs().T @ xf.abs()
        gb64 += g.sum(0)
        sb64 += g.abs().sum(0)
        del xf, p, g
    _check("c1x1 grad w", gw[:, :, 0, 0], gw64, sw64)
    _check("c1x1 grad b", gb, gb64, sb64, rel=0.0)


# ------------------------------------------------------------------------------------------------------------------ LeakyReLU + BatchNorm2d

@pytest.mark.parametrize("c,h,w,residual,offset", [(32, H, W, False, False), (32, H, W, True, False), (64, H // 2, W // 2, False, False),
                                                   (96, H, W, False, False), (256, H // 16, W // 16, False, False),
                                                   (32, H, W, False, True)],
                         ids=["c32", "c32-residual", "c64", "c96", "c256", "c32-offset"])
def test_leaky_batch_norm_at_the_tiaf_shapes_vs_float64(c, h, w, residual, offset):
    """bn(LeakyReLU(x)) (+ the block's residual) as one node (unet2d._LeakyBatchNormRows): y, grad x, grad weight, grad bias, the running
    statistics, the saved mean / invstd and the batch counter.  `offset`: channel means ~ 32 x the standard deviation (8 + 0.25 randn),
    where fp32 sums of a and a^2 lose the variance to cancellation"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _LeakyBatchNormRows
    x = _randn((T, c, h, w), 41, scale=0.25 if offset else 1.5, shift=8.0 if offset else 0.3)
    gy = _randn((T, c, h, w), 42)
    res = _randn((T, c, h, w), 43) if residual else None
    weight = _randn((c,), 44, dtype=torch.float32).abs() * 0.5 + 0.5
    bias = _randn((c,), 45, dtype=torch.float32)
    eps, momentum = 1e-5, 0.1
    stats = []

    def run():
        rm, rv = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")     # from zero: running = momentum x the batch's
        nbt = torch.zeros((), dtype=torch.long, device="cuda")
        xr, wr, br = x.detach().requires_grad_(), weight.detach().requires_grad_(), bias.detach().requires_grad_()
        y = _LeakyBatchNormRows.apply(xr, wr, br, rm, rv, nbt, eps, momentum, SLOPE, res)
        saved = y.grad_fn.saved_tensors[2]                                         # [mean, invstd]
        stats.append((rm, rv, nbt, saved.clone()))
        return (y,) + torch.autograd.grad(y, (xr, wr, br), gy) + (rm, rv, saved)
    y, gx, gw, gb, _, _, _ = _twice(run)
    rm, rv, nbt, saved = stats[0]
    assert int(nbt) == 1 and y.is_contiguous(memory_format=torch.channels_last) and gx.is_contiguous(memory_format=torch.channels_last)
    n = T * h * w
    x64 = x.double()
    a = torch.where(x64 > 0, x64, SLOPE * x64)
    del x64
    mu = a.mean((0, 2, 3), keepdim=True)
    ac = a - mu
    var = ac.square().mean((0, 2, 3), keepdim=True)
    invstd = (var + eps).rsqrt()
    w64, b64 = weight.double().view(1, c, 1, 1), bias.double().view(1, c, 1, 1)
    yb = ac * invstd * w64 + b64
    sy = (a.abs() + mu.abs()) * invstd * w64.abs() + b64.abs()
    del a
    if residual:
        # the residual is added to the ROUNDED normalised value, as the module pair does: one more half rounding, of |yb|
        r64 = res.double()
        _check("lbn y", y, yb + r64, sy + r64.abs() + 2 ** 3 * yb.abs())
        del r64
    else:
        _check("lbn y", y, yb, sy)
    del yb, sy
    # statistics: the saved mean / invstd, the running mean / unbiased variance (momentum x the batch's, from zero), rtol 1e-3
    torch.testing.assert_close(saved[0].double(), mu.flatten(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(saved[1].double(), invstd.flatten(), rtol=1e-3, atol=0.0)
    torch.testing.assert_close(rm.double(), momentum * mu.flatten(), rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(rv.double(), momentum * var.flatten() * n / (n - 1), rtol=1e-3, atol=0.0)
    # backward
    g = gy.double()
    gb64 = g.sum((0, 2, 3), keepdim=True)
    gac = (g * ac).sum((0, 2, 3), keepdim=True)
    _check("lbn grad bias", gb, gb64.flatten(), g.abs().sum((0, 2, 3)), rel=0.0)
    _check("lbn grad weight", gw, (gac * invstd).flatten(), (g * ac).abs().sum((0, 2, 3)) * invstd.flatten(), rel=0.0)
    k1 = gac / n * invstd.square()
    ga = (g - gb64 / n - ac * k1) * invstd * w64
    sa = (g.abs() + g.abs().mean((0, 2, 3), keepdim=True) + ac.abs() * (g * ac).abs().mean((0, 2, 3), keepdim=True) * invstd.square()) \
        * invstd * w64.abs()
    d = torch.where(x > 0, 1.0, SLOPE).double()
    _check("lbn grad x", gx, ga * d, sa * d)


# ------------------------------------------------------------------------------------------------------------------ pool, shuffle + concat

@pytest.mark.parametrize("c,h,w", [(32, H, W), (64, H // 2, W // 2), (256, H // 8, W // 8)])
def test_avgpool3s2_at_the_tiaf_shapes_vs_float64(c, h, w):
    """AvgPool2d(3, stride 2, padding 1) of the encoder's stages (unet2d._AvgPool3s2Rows): y and grad x against the contiguous
    float64 pool"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _AvgPool3s2Rows
    x = _randn((T, c, h, w), 51)
    gy = _randn((T, c, h // 2, w // 2), 52)

    def run():
        xr = x.detach().requires_grad_()
        y = _AvgPool3s2Rows.apply(xr)
        return (y,) + torch.autograd.grad(y, (xr,), gy)
    y, gx = _twice(run)
    assert y.shape == gy.shape and y.is_contiguous(memory_format=torch.channels_last)
    pool = lambda v: F.avg_pool2d(v, 3, stride=2, padding=1)            # noqa: E731
    x64 = x.double().contiguous().requires_grad_()
    _check("pool y", y, pool(x64).detach(), pool(x64.detach().abs()))
    (ref,) = torch.autograd.grad(pool(x64), x64, gy.double().contiguous())
    (s,) = torch.autograd.grad(pool(x64), x64, gy.double().abs().contiguous())
    _check("pool grad x", gx, ref, s)


@pytest.mark.parametrize("cx,hx,wx,cs", [(96, H // 2, W // 2, 32), (128, H // 4, W // 4, 64)], ids=["up4", "up3"])
def test_shuffle_cat_at_the_tiaf_shapes(cx, hx, wx, cs):
    """UpBlock's entry (unet2d._ShuffleCatRows) at up4 and up3: without dropout factors bit-equal to pixel_shuffle + cat and so is its
    adjoint; with them bit-equal to the float64 product rounded once (the factors 0, 1.25, 1.5625 times a half value are exact in
    fp32)"""
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import _ShuffleCatRows
    x = _randn((T, cx, hx, wx), 61)
    skip = _randn((T, cs, 2 * hx, 2 * wx), 62)
    gy = _randn((T, cx // 4 + cs, 2 * hx, 2 * wx), 63)
    g = torch.Generator().manual_seed(64)
    m = torch.tensor([0.0, 1.25, 1.5625], device="cuda")[torch.randint(0, 3, (T, cx // 4 + cs), generator=g).cuda()]
    for scale in (None, m):
        def run():
            xr, sr = x.detach().requires_grad_(), skip.detach().requires_grad_()
            y = _ShuffleCatRows.apply(xr, sr, scale)
            return (y,) + torch.autograd.grad(y, (xr, sr), gy)
        y, gx, gs = _twice(run)
        xr, sr = x.detach().requires_grad_(), skip.detach().requires_grad_()
        want = torch.cat((F.pixel_shuffle(xr, 2), sr), dim=1)
        if scale is None:
            wx_, ws_ = torch.autograd.grad(want, (xr, sr), gy)
            assert torch.equal(y, want) and torch.equal(gx, wx_) and torch.equal(gs, ws_)
        else:
            f = scale[:, :, None, None].double()
            assert torch.equal(y, (want.detach().double() * f).half())
            gcat = gy.double() * f
            assert torch.equal(gx, F.pixel_unshuffle(gcat[:, :cx // 4], 2).half())
            assert torch.equal(gs, gcat[:, cx // 4:].half())


# ------------------------------------------------------------------------------------------------------------------ the whole branch

_NODES = ("_Conv3x3C32Rows", "_Conv1x1C32Act", "_Conv3x3Rows", "_LeakyBatchNormRows", "_AvgPool3s2Rows", "_ShuffleCatRows")


def test_unet2d_branch_under_autocast_is_no_further_from_float64_than_the_vendor_half_path(monkeypatch):
    """UNet2D._encode -> _decode_u2 -> _decode_u4 -> classifier on T = 2 frames of 96 x 320 with every family of the library routed
    (the pixel gate monkeypatched away), under autocast, Dropout2d in evaluation and BatchNorm in training mode, backward with a fixed
    gradient: the logits and EVERY parameter gradient are at most 2 x as far from float64 (a contiguous-format copy with the half
    weights autocast uses) as the same run on the vendor's half path is, plus 1e-6 of the tensor's norm.  (The pools run on the
    library's kernels in both runs: _pool has no switch.)"""
    from taseg_amd.options import options
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet import unet2d
    monkeypatch.setattr(unet2d, "_CONV_ROWS_MIN_PIXELS", 1)
    torch.manual_seed(0)
    net = fill_parameters(unet2d.UNet2D(3, 20), seed=5).cuda()
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    x = _randn((2, 3, 96, 320), 71, dtype=torch.float32)
    gout = _randn((2, 20, 96, 320), 72, dtype=torch.float32)

    def branch(model, inp):
        x5, skips = model._encode(inp)
        return model.classifier(model._decode_u4(model._decode_u2(x5, skips), skips))

    def run(**switches):
        model = copy.deepcopy(net)
        with options.override(**switches), torch.autocast("cuda", dtype=torch.float16):
            y = branch(model, x)
        seen, stack = set(), [y.grad_fn]
        while stack:
            node = stack.pop()
            if node is None or id(node) in seen:
                continue
            seen.add(id(node))
            seen.add(type(node).__name__)
            stack.extend(fn for fn, _ in node.next_functions)
        y.float().backward(gout)
        return y.detach().double(), {n: p.grad.double() for n, p in model.named_parameters()}, seen

    ours, g_ours, seen = run()
    for name in _NODES:
        assert any(isinstance(t, str) and t.startswith(name) for t in seen), f"{name} is not in the graph"
    vendor, g_vendor, seen_v = run(image_conv_rows=False, image_fused_bn=False, image_shuffle_cat=False)
    assert not any(isinstance(t, str) and t.startswith(n) for t in seen_v for n in _NODES if n != "_AvgPool3s2Rows")
    with options.override(image_layout="nchw"):
        ref = unet2d.UNet2D(3, 20).cuda().double()
    sd = net.state_dict()
    with torch.no_grad():
        for name, mod in net.named_modules():
            if isinstance(mod, torch.nn.Conv2d):                 # the half weights (and biases) autocast hands the convolutions
                for pn in ("weight", "bias"):
                    sd[f"{name}.{pn}"] = sd[f"{name}.{pn}"].half()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    ref.train()
    for m in ref.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    assert all(p.is_contiguous() for p in ref.parameters())
    y64 = branch(ref, x.double().contiguous())
    y64.backward(gout.double().contiguous())
    g64 = {n: p.grad for n, p in ref.named_parameters()}
    assert sorted(g64) == sorted(g_ours) == sorted(g_vendor) and len(g64) == 78
    worst = []
    for name, a, v, r in [("logits", ours, vendor, y64.detach())] + [(n, g_ours[n], g_vendor[n], g64[n]) for n in sorted(g64)]:
        d_ours, d_vendor, norm = float((a - r).norm()), float((v - r).norm()), float(r.norm())
        worst.append((d_ours / (2 * d_vendor + 1e-6 * norm), name, d_ours, d_vendor))
        assert d_ours <= 2 * d_vendor + 1e-6 * norm, (name, d_ours, d_vendor, norm)
    print("branch: worst distance / bar %.3g (%s: ours %.3g, vendor %.3g)" % max(worst))
