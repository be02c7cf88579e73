"""SalsaNext, the range-view segmentor (reference pcseg/model/segmentor/range/salsanext/model/semantic/salsanext.py).

Module tree and attribute names are the reference's - `downCntx.conv1.weight` .. `resBlock1.bn4.num_batches_tracked` ..
`upBlock4.bn4.*`, `logits.bias`, and `WCE.weight` with LOSS 'wce' - so every state_dict key, their order and shapes are the reference's
and its checkpoints load here and vice versa.  The blocks are the FULL ones (conv3 .. conv5 and bn2 .. bn4; RPVNet's range branch runs
the reduced blocks of minkunet/unet2d.py), built on that file's helpers: the 32-channel full-resolution 3 x 3 and 1 x 1 layers take the
channels-last row kernels under autocast (`_conv`, `_conv_act`), every LeakyReLU + training-mode BatchNorm2d is one node on the row
kernels with the block's residual sum in its pass (`_act_bn`), the pooling is `_pool`, an UpBlock's entry `_ShuffleCatRows`; the 2 x 2
dilated convolutions and the 1 x 1 layers behind the concatenations are nn.Conv2d.  The memory layout is `options.image_layout`'s, as
in UNet2D.

Losses as the reference combines them (salsanext.py:249-277): `1.0 ce + 3.0 ls + 1.0 bd`, the cross entropy over the
TOP_K_PERCENT_PIXELS hardest pixels; all in float32.  The Lovasz term runs on the library's kernels over the channels-last rows
(range/utils.py here).  The scalars of tb_dict / disp_dict are lazy (no host read in forward; the reference calls `.item()` twice).
The evaluation branch returns {'point_predict': logits, 'point_labels': label_rv} as the reference does.
"""
import torch
import torch.nn.functional as F
from torch import nn

from taseg_amd.options import options
from taseg_amd.pcseg.model.segmentor.base_segmentors import BaseSegmentor
from taseg_amd.pcseg.model.segmentor.range.utils import BoundaryLoss, ClassWeightSemikitti, CrossEntropyDiceLoss, Lovasz_softmax
from taseg_amd.pcseg.model.segmentor.voxel.minkunet import unet2d as U
from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import LazyScalar
from taseg_amd.pcseg.model.segmentor.voxel.minkunet.unet2d import ResContextBlock, _act_bn, _conv, _conv_act, _leaky, _pool

__all__ = ["SalsaNext", "ResContextBlock", "ResBlock", "UpBlock"]


class ResBlock(U.ResBlock):
    """salsanext.py:40-114: 1 x 1 shortcut; 3 x 3, 3 x 3 dilated 2 and 2 x 2 dilated 2 in a chain, each LeakyReLU + BatchNorm; their
    three outputs concatenated into a 1 x 1; the sum with the shortcut; Dropout2d and the 3 x 3 / stride-2 average pool.  The base
    class registers conv1, conv2, bn1 (and the parameter-free dropout and pool), this one conv3 .. bn4 behind them: the reference's
    parameter order."""

    def __init__(self, in_filters, out_filters, dropout_rate, kernel_size=(3, 3), stride=1, pooling=True, drop_out=True):
        super().__init__(in_filters, out_filters, dropout_rate, kernel_size, stride, pooling, drop_out)
        self.conv3 = nn.Conv2d(out_filters, out_filters, kernel_size=(3, 3), dilation=2, padding=2)
        self.act3 = _leaky()
        self.bn2 = nn.BatchNorm2d(out_filters)
        self.conv4 = nn.Conv2d(out_filters, out_filters, kernel_size=(2, 2), dilation=2, padding=1)
        self.act4 = _leaky()
        self.bn3 = nn.BatchNorm2d(out_filters)
        self.conv5 = nn.Conv2d(out_filters * 3, out_filters, kernel_size=(1, 1))
        self.act5 = _leaky()
        self.bn4 = nn.BatchNorm2d(out_filters)

    def forward(self, x):
        shortcut = _conv_act(self.conv1, self.act1, x)
        a1 = _act_bn(self.act2, self.bn1, _conv(self.conv2, x))
        a2 = _act_bn(self.act3, self.bn2, _conv(self.conv3, a1))
        a3 = _act_bn(self.act4, self.bn3, self.conv4(a2))
        res = _act_bn(self.act5, self.bn4, self.conv5(torch.cat((a1, a2, a3), dim=1)), residual=shortcut)
        out = self.dropout(res) if self.drop_out else res
        if not self.pooling:
            return out
        return _pool(self.pool, out), res


class UpBlock(U.UpBlock):
    """salsanext.py:117-174: PixelShuffle(2) + skip concat with Dropout2d around them (the base class's entry), then the same chain of
    three convolutions, the concatenation and the 1 x 1 as ResBlock, without a shortcut"""

    def __init__(self, in_filters, out_filters, dropout_rate, drop_out=True):
        super().__init__(in_filters, out_filters, dropout_rate, drop_out)
        self.conv2 = nn.Conv2d(out_filters, out_filters, (3, 3), dilation=2, padding=2)
        self.act2 = _leaky()
        self.bn2 = nn.BatchNorm2d(out_filters)
        self.conv3 = nn.Conv2d(out_filters, out_filters, (2, 2), dilation=2, padding=1)
        self.act3 = _leaky()
        self.bn3 = nn.BatchNorm2d(out_filters)
        self.conv4 = nn.Conv2d(out_filters * 3, out_filters, kernel_size=(1, 1))
        self.act4 = _leaky()
        self.bn4 = nn.BatchNorm2d(out_filters)

    def forward(self, x, skip):
        cat = self._entry(x, skip)
        e1 = _act_bn(self.act1, self.bn1, _conv(self.conv1, cat))
        e2 = _act_bn(self.act2, self.bn2, _conv(self.conv2, e1))
        e3 = _act_bn(self.act3, self.bn3, self.conv3(e2))
        out = _act_bn(self.act4, self.bn4, self.conv4(torch.cat((e1, e2, e3), dim=1)))
        return self.dropout3(out) if self.drop_out else out


class SalsaNext(BaseSegmentor):
    def __init__(self, model_cfgs, num_class: int):
        super().__init__(model_cfgs, num_class)
        self.num_class = num_class
        self.if_ls_loss = model_cfgs.IF_LS_LOSS
        self.if_bd_loss = model_cfgs.IF_BD_LOSS

        self.downCntx = ResContextBlock(6, 32)
        self.downCntx2 = ResContextBlock(32, 32)
        self.downCntx3 = ResContextBlock(32, 32)

        self.resBlock1 = ResBlock(32, 2 * 32, 0.2, pooling=True, drop_out=False)
        self.resBlock2 = ResBlock(2 * 32, 2 * 2 * 32, 0.2, pooling=True)
        self.resBlock3 = ResBlock(2 * 2 * 32, 2 * 4 * 32, 0.2, pooling=True)
        self.resBlock4 = ResBlock(2 * 4 * 32, 2 * 4 * 32, 0.2, pooling=True)
        self.resBlock5 = ResBlock(2 * 4 * 32, 2 * 4 * 32, 0.2, pooling=False)

        self.upBlock1 = UpBlock(2 * 4 * 32, 4 * 32, 0.2)
        self.upBlock2 = UpBlock(4 * 32, 4 * 32, 0.2)
        self.upBlock3 = UpBlock(4 * 32, 2 * 32, 0.2)
        self.upBlock4 = UpBlock(2 * 32, 32, 0.2, drop_out=False)

        self.logits = nn.Conv2d(32, num_class, kernel_size=(1, 1))
        self.build_loss_funs(model_cfgs)

    def build_loss_funs(self, model_cfgs):
        self.top_k_percent_pixels = model_cfgs.TOP_K_PERCENT_PIXELS
        if model_cfgs.LOSS == 'wce':
            self.WCE = nn.CrossEntropyLoss(reduction='none', weight=torch.tensor(ClassWeightSemikitti.get_weight()))
        elif model_cfgs.LOSS == 'dice':
            self.WCE = CrossEntropyDiceLoss(reduction='none')
        if self.if_ls_loss:
            self.LS = Lovasz_softmax(ignore=0)
        if self.if_bd_loss:
            self.BD = BoundaryLoss()

    def _apply(self, fn, *args, **kwargs):
        """as UNet2D._apply: the convolution weights of a module on the device take `options.image_layout`'s memory format in the pass
        that moves them, so nothing after that reallocates a parameter"""
        out = super()._apply(fn, *args, **kwargs)
        if any(p.is_cuda for p in self.parameters()):
            want = self._set_layout()
            super()._apply(lambda t: t.contiguous(memory_format=want) if t.dim() == 4 else t)
        return out

    def _set_layout(self):
        return torch.channels_last if options.image_layout == "nhwc" else torch.contiguous_format

    def forward_logits(self, scan_rv):
        x = scan_rv.contiguous(memory_format=self._set_layout())
        x = self.downCntx3(self.downCntx2(self.downCntx(x)))
        down0c, down0b = self.resBlock1(x)
        down1c, down1b = self.resBlock2(down0c)
        down2c, down2b = self.resBlock3(down1c)
        down3c, down3b = self.resBlock4(down2c)
        down5c = self.resBlock5(down3c)
        up4e = self.upBlock1(down5c, down3b)
        up3e = self.upBlock2(up4e, down2b)
        up2e = self.upBlock3(up3e, down1b)
        up1e = self.upBlock4(up2e, down0b)
        return self.logits(up1e)

    def forward(self, batch):
        label_rv = batch['label_rv']
        if label_rv.dim() != 3:
            label_rv = label_rv.squeeze(dim=1)
        logits = self.forward_logits(batch['scan_rv'])
        if not self.training:
            return {'point_predict': logits, 'point_labels': label_rv}

        logits = logits.float()
        label_rv = label_rv.to(logits.device, non_blocking=True)
        pixel_losses = self.WCE(logits, label_rv).contiguous().view(-1)
        if self.top_k_percent_pixels != 1.0:
            pixel_losses, _ = torch.topk(pixel_losses, int(self.top_k_percent_pixels * pixel_losses.numel()))
        loss_ce = pixel_losses.mean()
        probs = F.softmax(logits, dim=1) if (self.if_ls_loss or self.if_bd_loss) else None
        loss_ls = self.LS(probs, label_rv).mean() if self.if_ls_loss else 0.
        loss_bd = self.BD(probs, label_rv) if self.if_bd_loss else 0.
        loss = 1.0 * loss_ce + 3.0 * loss_ls + 1.0 * loss_bd
        lazy = LazyScalar(loss)
        return {'loss': loss}, {'loss': lazy}, {'loss': lazy}
