"""Operators the range-view segmentors share beyond the blocks of minkunet/unet2d.py.

`fid_upcat` is the "fully interpolation decoding" step of FIDNet and CENet (reference fidnet.py:300-311, cenet.py:233-243):

    res_k = F.interpolate(x_k, size=(H, W), mode='bilinear', align_corners=True)      for the 1/2, 1/4, 1/8 maps
    out   = torch.cat([x, x_1, res_2, res_3, res_4], dim=1)

On channels-last device maps it is ONE autograd node on csrc/fid.hip (`options.image_fid_upcat`): one pass over the result forward, and
a gather in a fixed order backward - where ATen's `upsample_bilinear2d_backward` adds with float atomics and is marked
non-deterministic.  With the option off, or on maps the kernel does not take (the CPU, "nchw", other dtypes or channel counts), it is
that chain of ATen calls itself.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from taseg_amd import backend as B
from taseg_amd.options import options

__all__ = ["fid_upcat"]


class _FidUpCatRows(Function):
    """(cat[, res_2, res_3, res_4]) of five channels-last maps; the tables the forward built are the ones the backward reads"""

    @staticmethod
    def forward(ctx, x, x1, x2, x3, x4, levels):
        cat, res, tables = B.fid_upcat_rows_forward(x, x1, (x2, x3, x4), levels=levels)
        ctx.tables, ctx.channels, ctx.levels, ctx.dtype = tables, (x.shape[1], x1.shape[1], x2.shape[1]), levels, x.dtype
        ctx.sizes = [tuple(m.shape[2:]) for m in (x2, x3, x4)]
        return (cat, *res) if levels else cat

    @staticmethod
    def backward(ctx, grad_cat, *grad_res):
        # (autograd materialises the gradient of an output nobody used as zeros: every argument is a tensor)
        rows = lambda g: g.to(ctx.dtype).contiguous(memory_format=torch.channels_last)  # noqa: E731
        extra = [rows(g) for g in grad_res] if ctx.levels else None
        gx, gx1, gk = B.fid_upcat_rows_backward(rows(grad_cat), ctx.channels, ctx.sizes, ctx.tables, extra)
        return gx, gx1, gk[0], gk[1], gk[2], None


def fid_upcat(x, x1, x2, x3, x4, levels=False):
    """torch.cat([x, x1, up(x2), up(x3), up(x4)], dim=1) with up = bilinear interpolation to x's size, align_corners=True.
    levels=True: (cat, (res_2, res_3, res_4)) - the three interpolated maps as tensors of their own (CENet's auxiliary heads)."""
    if options.image_fid_upcat and x.is_cuda and not x.is_contiguous() and B.fid_upcat_rows_takes(x, x1, (x2, x3, x4)):
        if levels:
            cat, r2, r3, r4 = _FidUpCatRows.apply(x, x1, x2, x3, x4, True)
            return cat, (r2, r3, r4)
        return _FidUpCatRows.apply(x, x1, x2, x3, x4, False)
    res = [F.interpolate(m, size=x.size()[2:], mode='bilinear', align_corners=True) for m in (x2, x3, x4)]
    cat = torch.cat([x, x1, *res], dim=1)
    return (cat, tuple(res)) if levels else cat
