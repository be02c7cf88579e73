"""MinkUNet segmentor (reference pcseg/model/segmentor/voxel/minkunet/minkunet.py:186-458).

Module tree, attribute names and therefore every state_dict key / shape are identical to
the reference (`stem.0.kernel`, `stage1.0.net.0.kernel`, `stage2.1.downsample.0.kernel`,
`up1.1.0.net.0.kernel`, `classifier.0.weight`, BN `weight/bias/running_*` ...), so reference
checkpoints load here and vice versa.  The sparse ops run on the HIP backend through
`taseg_amd.torchsparse`.
"""
import torch
from torch import nn

from taseg_amd import torchsparse
from taseg_amd.torchsparse import PointTensor, SparseTensor
from taseg_amd.torchsparse import nn as spnn
from taseg_amd.torchsparse.nn import functional as spF
from taseg_amd.pcseg.loss import Losses
from ...base_segmentors import BaseSegmentor
from taseg_amd import backend as B
from taseg_amd import _fast
from taseg_amd.options import options
from .utils import voxel_to_point, voxelize_index
from . import stage_program as _SP

__all__ = ["MinkUNet", "unvoxelise_predictions", "DeviceEvalTail"]

import contextlib
import os as _os
_DEVOX_ATOMIC = options.devox_atomic
_DEVOX_CELLS = options.devox_cells     # stride-16 devoxelize backward: cell-reduced two-stage sum


def _coarse_devox_plan(idx, w, n_vox):
    """How the stride-16 devoxelize backward walks its map (~700 contributions per voxel, ~4 voxels per point): by default
    the cell-reduced two-stage sum (every gradient row read once, backend.devox_cells); TASEG_DEVOX_CELLS=0: the plain
    gather along the inverse map (every row read once per live corner)."""
    return B.devox_cells(idx, w, n_vox) if _DEVOX_CELLS else B.devox_csr(idx, w, n_vox)


class SyncBatchNorm(spnn.SyncBatchNorm):
    """nn.SyncBatchNorm applied to SparseTensor features (minkunet.py:23-25); training-mode reductions on HIP."""


class BatchNorm(spnn.BatchNorm):
    """nn.BatchNorm1d applied to SparseTensor features (minkunet.py:27-29); training-mode reductions on HIP."""


def _norm(channels: int, if_dist: bool) -> nn.Module:
    return SyncBatchNorm(channels) if if_dist else BatchNorm(channels)


class BasicConvolutionBlock(nn.Module):
    """conv -> BN -> ReLU (minkunet.py:31-54)."""

    def __init__(self, inc, outc, ks=3, stride=1, dilation=1, if_dist=False):
        super().__init__()
        self.net = nn.Sequential(
            spnn.Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride),
            _norm(outc, if_dist),
            spnn.ReLU(True),
        )

    def forward(self, x):
        # (children straight from the module dictionaries: `self.net[0]` is nn.Module.__getattr__ + nn.Sequential.__getitem__,
        # ~2 us each and five of them per residual block)
        net = self._modules["net"]._modules
        return spnn.conv_bn_act(net["0"], net["1"], x, relu=True)      # conv -> BN -> ReLU, one node


class BasicDeconvolutionBlock(nn.Module):
    """transposed conv -> BN -> ReLU (minkunet.py:57-80)."""

    def __init__(self, inc, outc, ks=3, stride=1, if_dist=False):
        super().__init__()
        self.net = nn.Sequential(
            spnn.Conv3d(inc, outc, kernel_size=ks, stride=stride, transposed=True),
            _norm(outc, if_dist),
            spnn.ReLU(True),
        )

    def forward(self, x):
        net = self._modules["net"]._modules
        return spnn.conv_bn_act(net["0"], net["1"], x, relu=True)


def _shortcut(inc, outc, stride, if_dist):
    if inc == outc and stride == 1:
        return nn.Identity()
    return nn.Sequential(spnn.Conv3d(inc, outc, kernel_size=1, dilation=1, stride=stride), _norm(outc, if_dist))


class ResidualBlock(nn.Module):
    """two 3x3x3 convs + identity / 1x1x1 shortcut (minkunet.py:83-129)."""
    expansion = 1

    def __init__(self, inc, outc, ks=3, stride=1, dilation=1, if_dist=False):
        super().__init__()
        self.net = nn.Sequential(
            spnn.Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride),
            _norm(outc, if_dist),
            spnn.ReLU(True),
            spnn.Conv3d(outc, outc, kernel_size=ks, dilation=dilation, stride=1),
            _norm(outc, if_dist),
        )
        self.downsample = _shortcut(inc, outc * self.expansion, stride, if_dist)
        self.relu = spnn.ReLU(True)

    def forward(self, x):
        # relu(net(x) + downsample(x)) with the BN / add / ReLU tails fused (same module parameters / buffers)
        # (the first block hands x through: the shortcut's gradient then lands in the store of conv1's input gradient)
        mods = self._modules
        net, down = mods["net"]._modules, mods["downsample"]
        h, x = spnn.conv_bn_act(net["0"], net["1"], x, relu=True, passthrough=True)
        # (the 1x1x1 shortcut + its BatchNorm: one block call on the identity rulebook, spnn.conv_bn_act)
        if isinstance(down, nn.Identity):
            shortcut = x
        else:
            dm = down._modules
            shortcut = spnn.conv_bn_act(dm["0"], dm["1"], x, relu=False)
        return spnn.conv_bn_act(net["3"], net["4"], h, relu=True, residual=shortcut)


class Bottleneck(nn.Module):
    """1x1x1 -> 3x3x3 -> 1x1x1 (x4) with shortcut (minkunet.py:132-183)."""
    expansion = 4

    def __init__(self, inc, outc, ks=3, stride=1, dilation=1, if_dist=False):
        super().__init__()
        wide = outc * self.expansion
        self.net = nn.Sequential(
            spnn.Conv3d(inc, outc, kernel_size=1, bias=False),
            _norm(outc, if_dist),
            spnn.Conv3d(outc, outc, kernel_size=ks, stride=stride, bias=False, dilation=dilation),
            _norm(outc, if_dist),
            spnn.Conv3d(outc, wide, kernel_size=1, bias=False),
            _norm(wide, if_dist),
        )
        self.downsample = _shortcut(inc, wide, stride, if_dist)
        self.relu = spnn.ReLU(True)

    def forward(self, x):
        return self.relu(self.net(x) + self.downsample(x))


class LazyScalar:
    """float-like view of a device scalar: the host sync happens only if somebody formats or
    converts it (the reference calls `loss.item()` inside forward, stalling the launch queue
    before backward; TASeg's trainer only logs the value)."""

    def __init__(self, t):
        self._t = t.detach()
        self._v = None

    def item(self):
        if self._v is None:
            self._v = float(self._t.item())
        return self._v

    __float__ = item

    def __format__(self, spec):
        return format(self.item(), spec)

    def __repr__(self):
        return repr(self.item())

    def _num(self, other):
        return float(other)

    def __add__(self, o):
        return self.item() + self._num(o)

    __radd__ = __add__

    def __mul__(self, o):
        return self.item() * self._num(o)

    __rmul__ = __mul__

    def __truediv__(self, o):
        return self.item() / self._num(o)


class MinkUNetBackbone(BaseSegmentor):
    """Everything MinkUNet and MinkUNetMs share: construction (minkunet.py:187-356 ==
    minkunet_ms.py:187-356) and the encoder / decoder / point-head pass (minkunet.py:393-422)."""

    def __init__(self, model_cfgs, num_class: int):
        super().__init__(model_cfgs, num_class)
        self.in_feature_dim = model_cfgs.IN_FEATURE_DIM
        self.num_layer = model_cfgs.get("NUM_LAYER", [2, 3, 4, 6, 2, 2, 2, 2])
        self.block = {"ResBlock": ResidualBlock, "Bottleneck": Bottleneck}[model_cfgs.get("BLOCK", "Bottleneck")]
        cr = model_cfgs.get("cr", 1.0)
        cs = [int(cr * x) for x in model_cfgs.get("PLANES", [32, 32, 64, 128, 256, 256, 128, 96, 96])]
        self.pres = model_cfgs.get("pres", 0.05)
        self.vres = model_cfgs.get("vres", 0.05)
        if_dist = model_cfgs.IF_DIST
        exp = self.block.expansion

        self.stem = nn.Sequential(
            spnn.Conv3d(self.in_feature_dim, cs[0], kernel_size=3, stride=1), _norm(cs[0], if_dist), spnn.ReLU(True),
            spnn.Conv3d(cs[0], cs[0], kernel_size=3, stride=1), _norm(cs[0], if_dist), spnn.ReLU(True),
        )
        self.in_channels = cs[0]

        def encoder_stage(width, depth):
            return nn.Sequential(
                BasicConvolutionBlock(self.in_channels, self.in_channels, ks=2, stride=2, dilation=1, if_dist=if_dist),
                *self._make_layer(self.block, width, depth, if_dist=if_dist))

        self.stage1 = encoder_stage(cs[1], self.num_layer[0])
        self.stage2 = encoder_stage(cs[2], self.num_layer[1])
        self.stage3 = encoder_stage(cs[3], self.num_layer[2])
        self.stage4 = encoder_stage(cs[4], self.num_layer[3])

        def decoder_stage(width, skip_channels, depth):
            up = BasicDeconvolutionBlock(self.in_channels, width, ks=2, stride=2, if_dist=if_dist)
            self.in_channels = width + skip_channels
            body = nn.Sequential(*self._make_layer(self.block, width, depth, if_dist=if_dist))
            return nn.ModuleList([up, body])

        self.up1 = decoder_stage(cs[5], cs[3] * exp, self.num_layer[4])
        self.up2 = decoder_stage(cs[6], cs[2] * exp, self.num_layer[5])
        self.up3 = decoder_stage(cs[7], cs[1] * exp, self.num_layer[6])
        self.up4 = decoder_stage(cs[8], cs[0], self.num_layer[7])

        self.classifier = nn.Sequential(spnn.PointLinear((cs[4] + cs[6] + cs[8]) * exp, self.num_class))
        self.weight_initialization()
        self.dropout = nn.Dropout(model_cfgs.get("DROPOUT_P", 0.3), True)

        default_loss = {"LOSS_TYPES": ["CELoss", "LovLoss"], "LOSS_WEIGHTS": [1.0, 1.0], "KNN": 10}
        loss_cfg = self.model_cfgs.get("LOSS_CONFIG", default_loss)
        loss_types = loss_cfg.get("LOSS_TYPES", default_loss["LOSS_TYPES"])
        loss_weights = loss_cfg.get("LOSS_WEIGHTS", default_loss["LOSS_WEIGHTS"])
        assert len(loss_types) == len(loss_weights)
        self.criterion_losses = Losses(
            loss_types=loss_types, loss_weights=loss_weights, ignore_index=model_cfgs.IGNORE_LABEL,
            knn=loss_cfg.get("KNN", default_loss["KNN"]), label_smoothing=model_cfgs.get("LABEL_SMOOTHING", 0.0))

    def _make_layer(self, block, out_channels, num_block, stride=1, if_dist=False):
        layers = [block(self.in_channels, out_channels, stride=stride, if_dist=if_dist)]
        self.in_channels = out_channels * block.expansion
        layers += [block(self.in_channels, out_channels, if_dist=if_dist) for _ in range(1, num_block)]
        return layers

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.SyncBatchNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    @staticmethod
    def _index_plan(coords: torch.Tensor, point_coords: torch.Tensor, backward: bool = True, **extra):
        """Everything of a pass that depends on coordinates only - no features, no parameters: the
        coordinate set and kernel map of every stride (same `cmaps` / `kmaps` entries conv3d would create
        lazily, conv.py:144-177) and the trilinear point<->voxel maps `voxel_to_point` caches per stride
        (utils.py:72-82; the U-Net devoxelises at strides 1, 16 and 4).  Built before the first convolution
        so the host reads (voxel counts, pair totals) do not stall the launch stream mid-network; a data stage
        may build it for the NEXT batch on another stream (`taseg_amd.data.stage.DevicePrefetcher`).  backward=False (an
        evaluation pass): without the walk orders of the devoxelize BACKWARD (three plans, one host read, ~25 launches)."""
        fast = _fast.module()
        if fast is not None and coords.is_cuda and coords.dtype == torch.int32 and point_coords.dtype == torch.float32:
            # native, interpreter-lock-free form of the block below (csrc/fastpath: same backend calls, same results)
            pc = point_coords.contiguous()
            cm, sub_t, down_t, totals, t_idx, t_w, orders = fast.index_plan(coords.contiguous(), pc, 4, B.L.stream())
            names = ("nbr", "nbmaps", "nbsizes", "nboffs", "pos_out", "pos_in")
            cmaps, kmaps = {}, {}
            for lvl, c in enumerate(cm):
                s = 1 << lvl
                cmaps[(s, s, s)] = c
            for lvl in range(5):
                s = 1 << lvl
                km = spF.KernelMap(dict(zip(names, sub_t[lvl])), (cm[lvl].shape[0], cm[lvl].shape[0]))
                t = int(totals[2 * lvl])
                # (a negative entry: the level's coordinates hold a duplicate - the map was built by the full probe, -(pairs + 1))
                km._total, km._dup = (-t - 1, True) if t < 0 else (t, False)
                km.build_class_plan(defer=True)       # large maps: plan of the class-sorted implicit GEMM (csrc/conv_class.hip)
                kmaps[((s, s, s), (3, 3, 3), (1, 1, 1), (1, 1, 1))] = km
                if lvl < 4:
                    km = spF.KernelMap(dict(zip(names, down_t[lvl])), (cm[lvl].shape[0], cm[lvl + 1].shape[0]))
                    km._total = int(totals[2 * lvl + 1])
                    km.build_direct_plans()               # 2x2x2 strided map: one-pass plans of its two directions
                    kmaps[((s, s, s), (2, 2, 2), (2, 2, 2), (1, 1, 1))] = km
            spF.accept_class_plans(list(kmaps.values()))       # ONE host read for the class plans of all levels
            keys = ((1, 1, 1), (16, 16, 16), (4, 4, 4))
            tri_idx, tri_w = dict(zip(keys, t_idx)), dict(zip(keys, t_w))
            tri_order = {keys[1]: orders[0]} if (_DEVOX_ATOMIC and backward) else {}
            for key in ((keys if not _DEVOX_ATOMIC else (keys[0], keys[2])) if backward else ()):
                plan = _coarse_devox_plan if key == keys[1] else B.devox_csr
                tri_order[key] = plan(tri_idx[key], tri_w[key], cmaps[key].shape[0])
            return dict(coords=coords, point_coords=pc, cmaps=cmaps, kmaps=kmaps, tri_idx=tri_idx, tri_w=tri_w,
                        tri_order=tri_order, **extra)
        with torch.no_grad():
            probe = SparseTensor(None, coords, 1)
            spF.build_pyramid(probe, num_levels=4)
            for key, km in probe.kmaps.items():
                if key[1] == (3, 3, 3) and key[2] == (1, 1, 1):
                    km.build_class_plan()
                elif key[1] == key[2] == (2, 2, 2):
                    km.build_direct_plans()
            tri_idx, tri_w, tri_order = {}, {}, {}
            pc = point_coords.contiguous()
            for s in (1, 16, 4):
                key = (s, s, s)
                tri_idx[key], tri_w[key] = B.trilinear_map(pc, probe.cmaps[key], s)
                if not backward:
                    continue
                # how the devoxelize backward walks this map: a gather along the inverse map, no atomics, fixed summation
                # order (the whole training step is run-to-run deterministic).  TASEG_DEVOX_ATOMIC=1: stride 16 (~4 live
                # corners, ~60 points per voxel) adds runs of points of one interpolation cell with float atomics instead,
                # every gradient row read once (147 vs 235 us per step, last-bit noise in the stage-4 gradients)
                if s == 16 and _DEVOX_ATOMIC:
                    tri_order[key] = B.devox_order(tri_idx[key], probe.cmaps[key].shape[0])
                elif s == 16:
                    tri_order[key] = _coarse_devox_plan(tri_idx[key], tri_w[key], probe.cmaps[key].shape[0])
                else:
                    tri_order[key] = B.devox_csr(tri_idx[key], tri_w[key], probe.cmaps[key].shape[0])
        return dict(coords=coords, point_coords=pc, cmaps=probe.cmaps, kmaps=probe.kmaps, tri_idx=tri_idx,
                    tri_w=tri_w, tri_order=tri_order, **extra)

    def prepare(self, batch_dict):
        """Build the index plan of `batch_dict` and leave it under batch_dict['_plan'] (forward() does this
        itself when it is absent)."""
        raise NotImplementedError

    def _unet(self, feats: torch.Tensor, point_feats: torch.Tensor, plan) -> torch.Tensor:
        """stem .. classifier on the stride-1 voxel features and their point view; returns logits [N, num_class]."""
        return self.classifier(self._unet_point_features(feats, point_feats, plan, concat=True))

    def _unet_point_features(self, feats: torch.Tensor, point_feats: torch.Tensor, plan, concat: bool = False):
        """The encoder / decoder pass; returns the three per-point feature blocks the classifier concatenates:
        stride-16 encoder output, stride-4 and stride-1 decoder outputs, each devoxelised onto the points.
        concat=True returns them as ONE [N, C1 + C2 + C3] tensor, interpolated straight into its column blocks
        (`spF.spdevoxelize_cat`: no torch.cat, no copies of the gradient slices in the backward pass)."""
        x0 = SparseTensor(feats, plan["coords"], 1)
        x0.cmaps, x0.kmaps = plan["cmaps"], plan["kmaps"]
        z = PointTensor(point_feats, plan["point_coords"], idx_query=plan["tri_idx"], weights=plan["tri_w"])
        z.additional_features["devox_order"] = plan["tri_order"]
        if "vox_idx" in plan:
            z.additional_features["idx_query"][1] = plan["vox_idx"]
            z.additional_features["counts"][1] = plan["vox_counts"]
        x0 = spnn.conv_bn_act(self.stem[0], self.stem[1], x0, relu=True)          # stem = 2 x (conv, BN, ReLU)
        x0 = spnn.conv_bn_act(self.stem[3], self.stem[4], x0, relu=True)
        progs = self._stage_programs(x0.F, plan)
        if progs is not None:
            return self._unet_stages(progs, x0.F, plan, concat)
        z0 = voxel_to_point(x0, z, nearest=False, features=False)      # z0.F is never read (cache carrier only)

        x1 = self.stage1(x0)
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        concat = concat and all(k in plan["tri_idx"] for k in (x4.s, x2.s, x0.s))
        sources = []                                   # (voxel features before dropout, stride) of z1, z2, z3
        if concat:
            sources.append((x4.F, x4.s))
        else:
            z1 = voxel_to_point(x4, z0)

        # out of place: `sources` (and the ReLU node that produced x4.F) still hold the features BEFORE dropout - the
        # reference devoxelises z1 / z2 before its in-place dropout (minkunet.py:400-412)
        x4.F = torch.nn.functional.dropout(x4.F, self.dropout.p, self.training, False)
        y1 = self.up1[1](torchsparse.cat([self.up1[0](x4), x3]))
        y2 = self.up2[1](torchsparse.cat([self.up2[0](y1), x2]))
        if concat:
            sources.append((y2.F, y2.s))
        else:
            z2 = voxel_to_point(y2, z1)

        y2.F = torch.nn.functional.dropout(y2.F, self.dropout.p, self.training, False)
        y3 = self.up3[1](torchsparse.cat([self.up3[0](y2), x1]))
        y4 = self.up4[1](torchsparse.cat([self.up4[0](y3), x0]))
        if concat:
            sources.append((y4.F, y4.s))
            orders = plan["tri_order"]
            return spF.spdevoxelize_cat([f for f, _ in sources],
                                        [(plan["tri_idx"][k], plan["tri_w"][k], orders.get(k)) for _, k in sources])
        z3 = voxel_to_point(y4, z2)
        return z1.F, z2.F, z3.F

    def _stage_programs(self, feats, plan):
        """the compiled stage programs of this model (stage_program.StagePrograms) if they can serve this pass on this index plan,
        else None: the module-by-module path then runs (TASEG_STAGE_PROGRAM=0, no native binding, Bottleneck blocks, hooks on
        the conv modules, widths off the full-tile paths, an index plan without the U-Net's kernel maps ...)"""
        if not _SP.enabled():
            return None
        progs = _SP.programs_of(self)
        if progs is None:
            return None
        if not progs.usable(feats, self.training, torch.is_grad_enabled()):
            if progs.stale:                          # parameter / buffer objects were replaced: compile again at the next pass
                _SP.forget(self)
            return None
        if not all(k in plan["tri_idx"] for k in ((16, 16, 16), (4, 4, 4), (1, 1, 1))):
            return None
        half = spF._amp_half(feats)
        progs.half = half                            # (prepare() resolves the NEXT batch's geometry for this storage mode)
        try:
            progs.prepare(plan, half)                # cached in the plan: a no-op when the data stage has done it
        except _SP._Unsupported:
            return None
        return progs

    def _stage_prepare(self, plan):
        """resolve the stage programs' geometry (kernel maps + class plans per op) with the index plan - on the thread that stages
        the batch, not on the one that issues the step; a no-op until the first pass has compiled the programs"""
        progs = _SP.programs_of(self, compile=False)
        if progs is not None:
            try:
                progs.prepare(plan, progs.half)
            except _SP._Unsupported:
                pass
        return plan

    def _unet_stages(self, progs, f0, plan, concat):
        """stage1 .. up4 of `_unet_point_features` on the stage programs: one call (and one autograd node) per stage"""
        # (the eight stages and the two out-of-place dropouts between them - the point head devoxelises the features BEFORE
        # dropout, minkunet.py:400-412 - in one native call, issued without the interpreter lock)
        f4, y2, y4 = progs.run_unet(f0, plan, self.training, self.dropout.p)
        keys = ((16, 16, 16), (4, 4, 4), (1, 1, 1))
        tri_idx, tri_w, orders = plan["tri_idx"], plan["tri_w"], plan["tri_order"]
        maps = [(tri_idx[k], tri_w[k], orders.get(k)) for k in keys]
        if concat:
            return spF.spdevoxelize_cat([f4, y2, y4], maps)
        return tuple(spF.spdevoxelize(f, i, w, o) for f, (i, w, o) in zip((f4, y2, y4), maps))

    def _train_outputs(self, logits, target, coords_xyz, offset):
        loss = self.criterion_losses(logits, target, xyz=coords_xyz, offset=offset)
        lazy = LazyScalar(loss)
        return {"loss": loss}, {"loss": lazy}, {"loss": lazy}

    @staticmethod
    def _eval_outputs(out, x, batch_dict, want_probs, defer, device_tail, ms=False):
        """The evaluation ending of every forward of this family: the logits `out` of the voxels of `x` leave through `device_tail`
        (DeviceEvalTail: nothing is un-voxelised to the host) or through `unvoxelise_predictions`.  ms: the keys of a fused
        multi-scan cloud - its own inverse map, and `point_mask` / `num_points_ms` to keep the current frame's points and trim to
        the scan's own point count (minkunet_ms.py:433-458)."""
        args = (out, x.C[:, -1], batch_dict["inverse_map_ms" if ms else "inverse_map"], batch_dict["targets_mapped"],
                batch_dict["num_points"])
        kw = {"point_mask": batch_dict["point_mask"], "num_points_ms": batch_dict["num_points_ms"]} if ms else {}
        if device_tail is not None:
            return device_tail.run(*args, names=batch_dict["name"], **kw)
        return unvoxelise_predictions(*args, want_probs, names=batch_dict["name"], defer=defer, **kw)


class _PinnedRing:
    """host buffers for the evaluation tail's device -> host copies: page-locked (the copies are asynchronous), grown on demand,
    four generations deep - a deferred result stays valid until three further deferred tails have been issued"""
    DEPTH = 4

    def __init__(self):
        self.bufs, self.at = {}, 0

    def next_generation(self):
        self.at = (self.at + 1) % self.DEPTH

    def take(self, key, like, numel):
        k = (key, self.at)
        b = self.bufs.get(k)
        if b is None or b.dtype != like.dtype or b.numel() < numel:
            b = self.bufs[k] = torch.empty(max(int(numel * 1.25), 1024), dtype=like.dtype, pin_memory=True)
        return b[:numel]


_pinned = _PinnedRing()
# TASEG_EVAL_COPY_STREAM=0: the deferred tail's device -> host copies on the launch stream
_COPY_STREAM = options.eval_copy_stream
_copy_streams = {}


def _copy_stream(device):
    s = _copy_streams.get(device)
    if s is None:
        s = _copy_streams[device] = torch.cuda.Stream(device=device)
    return s


class PendingPredictions:
    """The evaluation tail in flight (`model(batch, defer=True)`): every device -> host copy has been enqueued into page-locked
    buffers behind the forward pass, one event marks their end.  `result()` waits for the event, checks what the reference's
    indexing would have raised on, and slices the dictionary of numpy arrays `model(batch)` returns.  The arrays are views of a
    ring of host buffers: valid until three further deferred tails have been issued (copy them to keep them longer)."""

    def __init__(self, event, meta_h, result_h, mapped_h, labels_h, shapes, names, n_scenes, has_ms, fused=False, fallback=None):
        self.event, self.meta_h, self.result_h, self.mapped_h, self.labels_h = event, meta_h, result_h, mapped_h, labels_h
        self.shapes, self.names, self.n_scenes, self.has_ms = shapes, names, n_scenes, has_ms
        self.fused, self.fallback = fused, fallback
        self._out = None

    def result(self):
        if self._out is not None:
            return self._out
        self.event.synchronize()
        n = self.n_scenes
        meta = self.meta_h.numpy()
        if self.fused:
            # the fused tail (csrc/evaltail.hip): [flags, voxels per scene, points per scene, labels per scene, ...]; flags bit 0:
            # a scene index outside the batch, bit 1: an index array not grouped by scene (the sorted form then serves the batch),
            # bit 2: inverse map outside its scene
            flags = int(meta[0])
            if flags & 2:
                self._out = self.fallback()
                return self._out
            bad = (1 if flags & 4 else 0) | (2 if flags & 1 else 0)
            cnt_p_h = cnt_k_h = meta[1 + n:1 + 2 * n].tolist()
        else:
            bad, cnt_p_h, cnt_k_h = int(meta[0]), meta[1:1 + n].tolist(), meta[1 + n:1 + 2 * n].tolist()
        cnt_l_h = meta[1 + 2 * n:1 + 3 * n].tolist()
        n_cur_h = meta[1 + 3 * n:1 + 4 * n].tolist()
        if bad & 2:
            raise IndexError(f"batch indices beyond the {n} scenes of the batch")
        if bad & 1:
            raise IndexError("inverse_map names a voxel outside its scene")
        if self.has_ms:
            n_ms_h = meta[1 + 4 * n:1 + 5 * n].tolist()
            if n_ms_h != cnt_p_h:
                raise IndexError(f"num_points_ms {n_ms_h} does not match the inverse map's points per scene {cnt_p_h}")
        result_h = self.result_h.numpy().reshape(self.shapes[0])
        mapped_h = None if self.mapped_h is None else self.mapped_h.numpy().reshape(self.shapes[1])
        labels_h = self.labels_h.numpy().reshape(self.shapes[2])
        point_predict, point_labels, point_predict_logits = [], [], []
        at_k = at_l = 0
        for b in range(n):
            n_cur = int(n_cur_h[b])
            seg = slice(at_k, at_k + min(int(cnt_k_h[b]), n_cur))
            point_predict.append(result_h[seg])                 # (views of the batch's arrays: no second host copy)
            if mapped_h is not None:
                point_predict_logits.append(mapped_h[seg])
            point_labels.append(labels_h[at_l: at_l + min(int(cnt_l_h[b]), n_cur)])
            at_k += int(cnt_k_h[b])
            at_l += int(cnt_l_h[b])
        self._out = {"point_predict": point_predict, "point_labels": point_labels, "name": self.names,
                     "point_predict_logits": point_predict_logits}
        return self._out


_FUSED_TAIL = options.fused_eval_tail


def _fused_tail(out, vox_batch, invs, all_labels, num_points, want_probs, num_points_ms, names, defer, n_scenes):
    """unvoxelise_predictions for index arrays grouped by scene (what sparse_collate builds) in two launches of csrc/evaltail.hip -
    rows per scene, then gather + arg-max - instead of three stable sorts and ~45 tensor ops; None where it does not apply.  A batch
    that is not grouped is detected on the device and served by the sorted form when the arrays are collected."""
    bv, bp, bl = vox_batch, invs.C[:, -1], all_labels.C[:, -1]
    if not (out.is_cuda and out.dim() == 2 and out.dtype in (torch.float32, torch.float16) and n_scenes <= 64
            and all(t.dtype == torch.int32 and t.is_cuda and t.dim() == 1 for t in (bv, bp, bl))):
        return None
    L = B.L
    lib = L.load()
    dev = out.device
    inv = invs.F if invs.F.dtype == torch.int64 else invs.F.long()
    inv = inv.contiguous()
    n = n_scenes
    has_ms = num_points_ms is not None
    meta = torch.zeros(1 + (5 if has_ms else 4) * n, dtype=torch.int64, device=dev)      # [flags | counts 3 x n | num_points (| _ms)]
    st = L.stream()
    stride = lambda t: int(t.stride(0)) if t.shape[0] > 1 else 1  # noqa: E731
    L.check(lib.ts_scene_counts(L.ptr(bv), stride(bv), bv.shape[0], L.ptr(bp), stride(bp), bp.shape[0], L.ptr(bl), stride(bl),
                                bl.shape[0], n, meta.data_ptr() + 8, meta.data_ptr(), st), "ts_scene_counts")
    logits = out.contiguous()
    pts, c = inv.shape[0], logits.shape[1]
    mapped = torch.empty((pts, c), dtype=logits.dtype, device=dev)
    pred = None if want_probs else torch.empty(pts, dtype=torch.int64, device=dev)
    L.check(lib.ts_unvoxelise(L.ptr(logits), 1 if logits.dtype == torch.float16 else 0, c, meta.data_ptr() + 8, n, L.ptr(bp), stride(bp),
                              L.ptr(inv), pts, L.ptr(mapped), L.ptr(pred), meta.data_ptr(), st), "ts_unvoxelise")
    meta[1 + 3 * n:1 + 4 * n].copy_(torch.as_tensor(num_points).reshape(-1)[:n], non_blocking=True)
    if has_ms:
        meta[1 + 4 * n:1 + 5 * n].copy_(torch.as_tensor(num_points_ms).reshape(-1)[:n], non_blocking=True)
    result = mapped.softmax(1) if want_probs else pred
    return meta, result, mapped, all_labels.F


def unvoxelise_predictions(out, vox_batch, invs, all_labels, num_points, want_probs, point_mask=None, num_points_ms=None,
                           names=None, defer=False, _fused=True):
    """The evaluation tail of the segmentors (minkunet.py:435-455, minkunet_ms.py:433-458) for the WHOLE batch at once: per scene
    `out[scene][inverse_map of the scene]` (Ms: `[point_mask of the scene]`), trimmed to the scan's own point count; arg-max and
    logits (or the soft-max under return_logit / return_tta) and the mapped labels as numpy arrays, scene by scene - what the
    reference's per-scene loop of boolean masks returns, with three stable sorts, one gather and a handful of device -> host
    copies instead of ~12 launches and 6 host reads per scene.  defer: return a PendingPredictions instead of waiting for the
    copies - the caller issues the next batch's forward pass first and collects `result()` afterwards (pcseg/eval.py, bench.py
    --eval): the host never waits for the device between two batches."""
    dev = out.device
    n_scenes = len(names) if names is not None else int(torch.as_tensor(num_points).numel())
    fused = _fused_tail(out, vox_batch, invs, all_labels, num_points, want_probs, num_points_ms, names, defer, n_scenes) \
        if (_fused and _FUSED_TAIL and point_mask is None) else None
    if fused is not None:
        meta, result, mapped, labels_sorted = fused
        return _tail_to_host(meta, result, mapped, labels_sorted, want_probs, defer, names, n_scenes, num_points_ms is not None, True,
                             lambda: unvoxelise_predictions(out, vox_batch, invs, all_labels, num_points, want_probs, point_mask,
                                                            num_points_ms, names, False, _fused=False))
    b_vox, b_pts, b_lab = vox_batch.long(), invs.C[:, -1].long(), all_labels.C[:, -1].long()
    # stable sorts by scene: 8-bit keys where the batch allows it (one radix pass instead of the eight of a 64-bit key; an index
    # outside 0 .. 254 wraps to a value that is still >= n_scenes or lands in the wrong scene's count - both are reported below)
    narrow = (lambda t: t.clamp(-1, 255).to(torch.uint8)) if n_scenes < 255 else (lambda t: t)
    bv_sorted, order_v = torch.sort(narrow(b_vox), stable=True)   # out[scene] = out[order_v[start : start + count]] (original order kept)
    bp_sorted, order_p = torch.sort(narrow(b_pts), stable=True)
    bl_sorted, order_l = torch.sort(narrow(b_lab), stable=True)
    # rows per scene from the SORTED keys (torch.bincount reads the largest index on the host: with four of them the "deferred" tail
    # waited for the forward pass four times per batch - the host issue time of bench.py --eval was 2.3 ms of bincount)
    edges = torch.arange(n_scenes + 1, device=dev)

    def counts(sorted_keys):
        at = torch.searchsorted(sorted_keys.long(), edges)
        # (second value: rows whose scene index is outside 0 .. n_scenes - 1 - the reference's boolean masks would drop them
        # silently and fail on the shapes later; reported when the arrays are collected)
        return at[1:] - at[:-1], (at[0] != 0) | (at[-1] != sorted_keys.shape[0])
    cnt_v, out_v = counts(bv_sorted)
    cnt_p, out_p = counts(bp_sorted)
    cnt_l, out_l = counts(bl_sorted)
    bp_sorted = bp_sorted.long()
    start_v = torch.cumsum(cnt_v, 0) - cnt_v
    local = invs.F[order_p].long()
    scene_p = bp_sorted.clamp(0, n_scenes - 1)
    bad = ((local < 0) | (local >= cnt_v[scene_p])).any()           # read with the counts (the reference's indexing raises)
    rows = order_v[(start_v[scene_p] + local).clamp_(0, max(int(order_v.shape[0]) - 1, 0))]
    mapped = out[rows]                                      # [points, classes], scene-major, the scene's own point order
    cnt_k = cnt_p
    if point_mask is not None:
        keep = point_mask.to(dev).bool()
        mapped, kept_scene = mapped[keep], bp_sorted[keep]          # (boolean indexing: one host read, Ms models only)
        cnt_k, _ = counts(kept_scene)
    result = mapped.softmax(1) if want_probs else mapped.argmax(1)
    labels_sorted = all_labels.F[order_l]
    # one small tensor with everything the per-scene slicing needs, then the arrays themselves: asynchronous copies into page-locked
    # buffers, one event behind them
    code = bad.long() + 2 * (out_v | out_p | out_l).long()      # bit 0: inverse map outside its scene; bit 1: scene index outside the batch
    parts = [code.reshape(1), cnt_p.long(), cnt_k.long(), cnt_l.long(),
             torch.as_tensor(num_points).reshape(-1)[:n_scenes].to(dev, non_blocking=True).long()]
    if num_points_ms is not None:
        parts.append(torch.as_tensor(num_points_ms).reshape(-1)[:n_scenes].to(dev, non_blocking=True).long())
    meta = torch.cat(parts)
    return _tail_to_host(meta, result, mapped, labels_sorted, want_probs, defer, names, n_scenes, num_points_ms is not None, False, None)


def _tail_to_host(meta, result, mapped, labels_sorted, want_probs, defer, names, n_scenes, has_ms, fused, fallback):
    """one small tensor with everything the per-scene slicing needs, then the arrays themselves: asynchronous copies into page-locked
    buffers, one event behind them"""
    if defer:
        _pinned.next_generation()
    meta, result, labels_sorted = meta.contiguous(), result.contiguous(), labels_sorted.contiguous()
    mapped = mapped if want_probs else mapped.contiguous()

    def to_host(key, t):
        if not defer:
            return t.reshape(-1).cpu()           # fresh arrays, as `model(batch)` has always returned them
        h = _pinned.take(key, t, t.numel())
        h.copy_(t.reshape(-1), non_blocking=True)
        return h

    # deferred: the copies (the logits of every point among them: 19 MB per bench batch) run on a stream of their own behind an
    # event of the launch stream - there they are blit kernels that would hold the next pass's forward up (0.3 ms per pass)
    side = _copy_stream(meta.device) if (defer and _COPY_STREAM) else None
    if side is not None:
        ready = torch.cuda.Event()
        ready.record()
        side.wait_event(ready)
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        meta_h = to_host("meta", meta)
        result_h = to_host("result", result)
        mapped_h = None if want_probs else to_host("mapped", mapped)
        labels_h = to_host("labels", labels_sorted)
        event = torch.cuda.Event()
        event.record()
    pending = PendingPredictions(event, meta_h, result_h, mapped_h, labels_h, (tuple(result.shape), tuple(mapped.shape), tuple(labels_sorted.shape)),
                                 names, n_scenes, has_ms, fused, fallback)
    # (the device tensors stay alive until the copies have run: the event's owner keeps them)
    pending._keep = (meta, result, mapped, labels_sorted)
    return pending if defer else pending.result()


class PendingVotes:
    """One TTA batch of the device tail in flight: the label payload (and the chosen scores) of the scan are on their way into
    page-locked buffers behind one event.  `result()` waits for it, raises what the host path would have raised, and returns
    {"payload": [n, 1] uint32 / uint8, "scores": [n, C] / [n, 3] float32 or None, "name"} as arrays of their own."""

    def __init__(self, event, meta_h, label_h, scores_h, width, names, nuscenes, keep, remapped=False):
        self.event, self.meta_h, self.label_h, self.scores_h, self.width = event, meta_h, label_h, scores_h, width
        self.names, self.nuscenes, self._keep, self._out, self.remapped = names, nuscenes, keep, None, remapped

    def result(self):
        if self._out is None:
            self.event.synchronize()
            flags, zero, n = (int(v) for v in self.meta_h.numpy())
            DeviceEvalTail.raise_flags(flags, len(self.names))
            import numpy as np
            label = np.array(self.label_h.numpy()[:n]).reshape(n, 1)
            if self.nuscenes:
                # (a remapped payload no longer shows the class: the tail looked before the table and sent `zero` along)
                if zero if self.remapped else (label == 0).any():
                    raise ValueError("nuScenes submission must not contain the ignored class 0 (R/train.py:523)")
            else:
                label = label.view(np.uint32)
            scores = None if self.scores_h is None else np.array(self.scores_h.numpy()[:n * self.width]).reshape(n, self.width)
            self._out, self._keep = {"payload": label, "scores": scores, "name": self.names}, None
        return self._out


class PendingLabels:
    """One validation batch of the device tail with predictions=True in flight: the arg-max class of every kept point of every scan
    (through the remap table, narrowed to the payload type) and the per-scan counts m_s are on their way into page-locked buffers
    behind one event.  `result()` waits for it, raises what the host path would have raised, and returns {"payload": one [m_s, 1]
    uint32 / uint8 array of its own per scan, "name"}."""

    def __init__(self, event, meta_h, label_h, names, nuscenes, keep, remapped):
        self.event, self.meta_h, self.label_h, self.names, self.nuscenes = event, meta_h, label_h, names, nuscenes
        self._keep, self._out, self.remapped = keep, None, remapped

    def result(self):
        if self._out is None:
            self.event.synchronize()
            import numpy as np
            meta = self.meta_h.numpy()
            flags, zero, counts = int(meta[0]), int(meta[1]), meta[2:].tolist()
            DeviceEvalTail.raise_flags(flags, len(counts))
            labels, payloads, at = self.label_h.numpy(), [], 0
            for m in counts:
                label = np.array(labels[at:at + m]).reshape(m, 1)
                at += m
                if self.nuscenes:
                    if zero if self.remapped else (label == 0).any():
                        raise ValueError("nuScenes submission must not contain the ignored class 0 (R/train.py:523)")
                else:
                    label = label.view(np.uint32)
                payloads.append(label)
            self._out, self._keep = {"payload": payloads, "name": self.names}, None
        return self._out


class DeviceEvalTail:
    """Where `model(batch, device_tail=tail)` leaves an evaluation batch instead of un-voxelising it to the host - all six
    segmentors take it: MinkUNet, MinkUNetMs, MinkUNetMsMm, MinkUNetMsMmNus, MinkUNetMsKd through `run` (logits rows grouped by scene, a
    per-scene inverse map; csrc/evaltail.hip: ts_scene_counts + one launch, three more where a point_mask has to be compacted) and
    Cylinder_TS through `run_points` (rows in ascending-hash order over the batch, found by one batch-wide hash lookup of the points'
    cells; ts_scene_counts + one launch):

    votes == 0 (validation)  every scene is a scan: additions to `hist`, the resident [num_class, num_class] int64 confusion matrix
                             (R/train.py:35-52 fast_hist before its crop).  Nothing leaves the device until `read()` - unless
                             predictions=True: the launch also writes the arg-max of every kept point, and the call returns a
                             PendingLabels (label payload of every scan and the per-scan counts, behind one event).
    votes == V  (TTA)        the V scenes are the votes of one scan: float32 sum in vote order, arg-max, label payload (uint32, or
                             uint8 for nuScenes) and optionally scores ("all": the sums, "top3": the three largest) - the call
                             returns a PendingVotes; only payload and scores cross to the host.
    remap: a {class: raw id} dictionary or a table as pcseg.eval.remap_lut builds - the payloads go through it on the device (one
    gather) before they are narrowed to the payload type.
    `flags` collects what the host path raises on (include/taseg_hip.h ts_eval_*); it is read with the matrix / every payload."""

    def __init__(self, num_class, device, votes=0, dataset="semantickitti", scores=None, predictions=False, remap=None):
        if scores not in (None, "all", "top3"):
            raise ValueError(f"scores must be None, 'all' or 'top3' (got {scores!r})")
        if predictions and votes:
            raise ValueError("predictions=True is for validation batches (votes == 0): a TTA batch returns its payload anyway")
        self.num_class, self.votes, self.scores, self.predictions = int(num_class), int(votes), scores, bool(predictions)
        self.nuscenes = dataset.startswith("nuscenes")
        self.hist = torch.zeros((self.num_class, self.num_class), dtype=torch.int64, device=device)
        self.n_scenes = 0
        self.flags = torch.zeros(1, dtype=torch.int32, device=device)
        self.lut = None
        if remap is not None:
            from taseg_amd.pcseg.eval import _remap_table
            self.lut = torch.from_numpy(_remap_table(remap, self.num_class)).to(device)

    @staticmethod
    def raise_flags(flags, n_scenes):
        """the host path's exceptions (PendingPredictions.result, accumulate_votes, numpy) for the bits of `flags`"""
        if flags & 1:
            raise IndexError(f"batch indices beyond the {n_scenes} scenes of the batch")
        if flags & 2:
            raise ValueError("a batch is not grouped by scene in ascending order (sparse_collate builds it so): the device tail "
                             "does not sort - evaluate it with on_device=False")
        if flags & 4:
            raise IndexError("inverse_map names a voxel outside its scene")
        if flags & 32:
            raise IndexError("num_points_ms does not match the inverse map's points per scene")
        if flags & 8:
            raise IndexError("predictions and labels of a scan differ in length (labels per scene / num_points / kept points)")
        if flags & 16:
            raise ValueError("votes must cover the same points (one scan per TTA batch)")
        if flags & 64:
            raise IndexError("a point's cell has no voxel row (the hash lookup of its coordinates found none)")

    def _payload(self, classes, written):
        """classes (int32 / uint8, the first `written` rows - a device scalar - are valid) as the label payload: through the remap
        table, narrowed to the payload type.  Returns (payload, zero): zero [1] int64 counts the valid rows of class 0 where the
        table hides them from the host's nuScenes check, else 0."""
        zero = torch.zeros(1, dtype=torch.int64, device=classes.device)
        if self.lut is not None:
            if self.nuscenes:
                valid = torch.arange(classes.shape[0], device=classes.device) < written
                zero = ((classes == 0) & valid).sum().reshape(1)
            # (rows behind the written ones hold whatever the allocation held: clamped, so that the gather stays inside the table)
            classes = self.lut[classes.long().clamp_(0, self.num_class - 1)]
        return (classes.to(torch.uint8) if self.nuscenes else classes.to(torch.int32)), zero

    @staticmethod
    def _to_host(device, tensors):
        """asynchronous copies of `tensors` ({key: tensor}) into page-locked buffers on the copy stream, one event behind them"""
        _pinned.next_generation()
        side = _copy_stream(device) if _COPY_STREAM else None
        if side is not None:
            ready = torch.cuda.Event()
            ready.record()
            side.wait_event(ready)
        out = {}
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            for key, t in tensors.items():
                if t is None:
                    out[key] = None
                    continue
                h = out[key] = _pinned.take(key, t, t.numel())
                h.copy_(t.reshape(-1), non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        return event, out

    def run(self, out, vox_batch, invs, all_labels, num_points, point_mask=None, num_points_ms=None, names=None):
        if out.shape[1] != self.num_class:
            raise ValueError(f"the model has {out.shape[1]} classes, the evaluation {self.num_class}")
        pts_batch = invs.C[:, -1]
        self.n_scenes = n_scenes = len(names) if names is not None else int(torch.as_tensor(num_points).numel())
        mask = None if point_mask is None else point_mask.to(out.device)
        if not self.votes:
            got = B.eval_confusion(out, vox_batch, pts_batch, invs.F, all_labels.F.reshape(-1), all_labels.C[:, -1], num_points, self.hist,
                                   self.flags, point_mask=mask, num_points_ms=num_points_ms, want_pred=self.predictions,
                                   want_counts=self.predictions)
            return self._labels_to_host(out.device, got, names) if self.predictions else self
        if n_scenes != self.votes:
            raise ValueError(f"TTA batch holds {n_scenes} votes, {self.votes} expected (one scan per batch, collate_batch_tta)")
        got = B.eval_votes(out, vox_batch, pts_batch, invs.F, num_points, self.flags, point_mask=mask, num_points_ms=num_points_ms,
                           label_bytes=1 if self.nuscenes else 4, want_sums=self.scores == "all", want_top3=self.scores == "top3")
        return self._votes_to_host(out.device, got, names)

    def run_points(self, logits, voxel_coords, point_coord, point_label, num_points, names):
        """`run` for a model whose logits rows are in no per-scene order and whose points find their row through the hash of their
        cell (Cylinder_TS, cylinder_ts.py:244-260): logits [n_vox, C] with their int32 coordinates voxel_coords [n_vox, 4], point_coord
        [n_pts, 4] (x, y, z, batch; grouped by scene), point_label [n_pts] aligned with the points, num_points per scene.  ONE
        batch-wide lookup - a hash of the points' cells, a hash of the voxels', one query - names every point's logits row (the hash
        covers the batch column, so it is the row the reference's per-scene query finds), then ts_scene_counts + one launch
        (ts_eval_confusion_rows / ts_eval_votes_rows).  Returns what `run` returns.  One stated difference from the host path: a cell
        without a voxel row (the query's -1, with which the reference silently reads the scene's LAST row) raises IndexError at the
        read - batches of data.cylinder.build_cylinder_batch cannot produce one."""
        B.L.require_device(logits, voxel_coords, point_coord, point_label)
        if logits.shape[1] != self.num_class:
            raise ValueError(f"the model has {logits.shape[1]} classes, the evaluation {self.num_class}")
        self.n_scenes = n_scenes = len(names) if names is not None else int(torch.as_tensor(num_points).numel())
        cells = point_coord.to(voxel_coords)
        rows = spF.sphashquery(spF.sphash(cells), spF.sphash(voxel_coords))
        pts_batch = cells[:, -1]
        if not self.votes:
            labels = point_label.reshape(-1)
            labels = labels if labels.dtype in (torch.uint8, torch.int32, torch.int64) else labels.long()
            got = B.eval_confusion_rows(logits, rows, pts_batch, labels, num_points, self.hist, self.flags, want_pred=self.predictions,
                                        want_counts=self.predictions)
            return self._labels_to_host(logits.device, got, names) if self.predictions else self
        if n_scenes != self.votes:
            raise ValueError(f"TTA batch holds {n_scenes} votes, {self.votes} expected (one scan per batch, collate_batch_tta)")
        got = B.eval_votes_rows(logits, rows, pts_batch, num_points, self.flags, label_bytes=1 if self.nuscenes else 4,
                                want_sums=self.scores == "all", want_top3=self.scores == "top3")
        return self._votes_to_host(logits.device, got, names)

    def _labels_to_host(self, device, got, names):
        """validation with predictions=True: (pred, m) of the confusion call on their way to the host as a PendingLabels"""
        pred, m = got
        label, zero = self._payload(pred, m.sum())
        meta = torch.cat([self.flags.long(), zero, m])
        event, h = self._to_host(device, {"pred_meta": meta, "pred_label": label})
        return PendingLabels(event, h["pred_meta"], h["pred_label"], names, self.nuscenes, (meta, label), self.lut is not None)

    def _votes_to_host(self, device, got, names):
        """TTA: the dictionary of the votes call on its way to the host as a PendingVotes"""
        scores = got["sums"] if self.scores == "all" else got["top3"]
        label, zero = self._payload(got["label"], got["n"]) if self.lut is not None else (got["label"], got["n"].new_zeros(1))
        meta = torch.cat([self.flags.long(), zero, got["n"]])
        event, h = self._to_host(device, {"vote_meta": meta, "vote_label": label, "vote_scores": scores})
        return PendingVotes(event, h["vote_meta"], h["vote_label"], h["vote_scores"], 0 if scores is None else scores.shape[1], names,
                            self.nuscenes, (meta, got, label, scores), self.lut is not None)

    def read(self):
        """validation: the matrix summed over the ranks (parallel.reduce_confusion) and the flags in ONE host read"""
        from taseg_amd.parallel import reduce_confusion
        hist = reduce_confusion(self.hist.clone())       # (the all-reduce is in place: the resident matrix stays this rank's)
        both = torch.cat([hist.reshape(-1), self.flags.long()]).cpu().numpy()
        self.raise_flags(int(both[-1]), self.n_scenes)
        return both[:-1].reshape(self.num_class, self.num_class)


class MinkUNet(MinkUNetBackbone):
    """Single-frame model: re-voxelises `batch_dict['lidar']` on device, then the U-Net
    (minkunet.py:385-455)."""

    def prepare(self, batch_dict):
        with torch.no_grad():
            z = PointTensor(None, batch_dict["lidar"].C.float())
            coords, vox_idx, vox_counts = voxelize_index(z, self.pres, self.vres)      # minkunet.py:388-390
        plan = self._stage_prepare(self._index_plan(coords, z.C, backward=self.training, vox_idx=vox_idx, vox_counts=vox_counts))
        batch_dict["_plan"] = plan
        return plan

    def forward(self, batch_dict, return_logit=False, return_tta=False, defer=False, device_tail=None):
        x = batch_dict["lidar"]
        x.F = x.F[:, :self.in_feature_dim]
        plan = batch_dict.get("_plan") or self.prepare(batch_dict)
        feats = spF.spvoxelize(x.F, plan["vox_idx"], plan["vox_counts"])      # feature half of initial_voxelize
        out = self._unet(feats, x.F, plan)

        if self.training:
            target = batch_dict["targets"].F.long().cuda(non_blocking=True)
            return self._train_outputs(out, target, batch_dict["lidar"].C[:, :3].float(), batch_dict["offset"])

        return self._eval_outputs(out, x, batch_dict, return_logit or return_tta, defer, device_tail)

    def forward_ensemble(self, batch_dict):
        return self.forward(batch_dict, return_tta=True)
