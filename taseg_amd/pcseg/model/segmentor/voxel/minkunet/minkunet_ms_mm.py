"""MinkUNetMsMm - TASeg's TIAF segmentor: temporal image aggregation and fusion
(reference pcseg/model/segmentor/voxel/minkunet/minkunet_ms_mm.py:186-571).

Three branches, five losses:
  * `image_backbone` (UNet2D, dense, PyTorch-ROCm) on the stack of temporal camera frames; its logits and two decoder
    feature maps are gathered at the pixels the FOV points project to (HIP `ts_image_gather_*`);
  * `lidar_backbone` (UNet3D, sparse, HIP backend) on the FOV cloud with [LiDAR attributes | image features];
  * the MinkUNet of `MinkUNetMs` on the whole fused cloud; the FOV encoder's stride-16 / 4 / 1 voxel features are
    trilinearly devoxelised onto ALL points (`voxel_to_point_fov`), concatenated with the main branch's point
    features and classified by `classifier_fusion` on the points that overlap the FOV cloud.
Module names / state_dict follow the reference, so its checkpoints (and its `fix_part_param` fine-tuning recipe) load.
"""
import torch
from torch import nn

from taseg_amd.torchsparse import PointTensor
from .minkunet import LazyScalar, MinkUNetBackbone
from .unet2d import UNet2D
from .unet3d import UNet3D
from .utils import voxel_to_point_fov

__all__ = ["MinkUNetMsMm", "MinkUNetMsMmNus"]


class _RowsBatchNorm1d(nn.BatchNorm1d):
    """nn.BatchNorm1d of the fusion head (minkunet_ms_mm.py:372-377), same parameters and state_dict keys.  In training mode a device
    row matrix goes through the library's row kernels (taseg_amd/torchsparse/nn/batchnorm.py: sliced sums, double finish, one
    elementwise pass per direction): torch's native kernels take 0.8 ms for the backward reduction of the ~120k x 480 half matrix
    of a TIAF step, 1.9 ms per step in all.  Everything else is the module itself."""

    def forward(self, x):
        if (self.training and x.is_cuda and x.dim() == 2 and x.shape[0] > 1 and x.dtype in (torch.float32, torch.float16)
                and x.shape[1] % (8 if x.dtype == torch.float16 else 4) == 0 and x.shape[1] <= 1024 and self.affine
                and self.track_running_stats and self.momentum is not None and self.weight.dtype == torch.float32
                and not (self._forward_hooks or self._forward_pre_hooks or self._backward_hooks)):
            from taseg_amd.torchsparse.nn.batchnorm import batch_norm_train
            return batch_norm_train(x.contiguous(), self.weight, self.bias, self.running_mean, self.running_var, self.momentum,
                                    self.eps, num_batches_tracked=self.num_batches_tracked)
        return super().forward(x)


class MinkUNetMsMm(MinkUNetBackbone):
    def __init__(self, model_cfgs, num_class: int):
        super().__init__(model_cfgs, num_class)
        exp = self.block.expansion
        cr = model_cfgs.get("cr", 1.0)
        cs = [int(cr * x) for x in model_cfgs.get("PLANES", [32, 32, 64, 128, 256, 256, 128, 96, 96])]
        self.input_feat = model_cfgs.get("INPUT_FEAT")
        self.input_feat_lidar = model_cfgs.get("INPUT_FEAT_LIDAR")
        self.image_channel_in = 3 * ("rgb" in self.input_feat) + 1 * ("depth" in self.input_feat) \
            + 4 * ("lidar" in self.input_feat)
        self.image_backbone_type = model_cfgs.get("IMAGE_BACKBONE_TYPE")
        if self.image_backbone_type != "UNet2D":
            raise NotImplementedError(f"IMAGE_BACKBONE_TYPE '{self.image_backbone_type}'")
        self.image_backbone = UNet2D(self.image_channel_in, self.num_class)
        self.image_channel_out = 96 + 128
        self.lidar_channel_in = (self.in_feature_dim - 1) * ("lidar" in self.input_feat_lidar) \
            + self.image_channel_out * ("image" in self.input_feat_lidar) \
            + self.num_class * ("logit" in self.input_feat_lidar)
        self.lidar_backbone_type = model_cfgs.get("LIDAR_BACKBONE_TYPE")
        if self.lidar_backbone_type != "UNet3D":
            raise NotImplementedError(f"LIDAR_BACKBONE_TYPE '{self.lidar_backbone_type}'")
        # the reference's UNet3D hard-wires SyncBatchNorm (unet3d.py:200); it degrades to local statistics when
        # no process group is up, which is also what our SyncBatchNorm does
        self.lidar_backbone = UNet3D(self.lidar_channel_in, self.num_class, if_dist=True)

        (self.lidar_weight, self.fusion_weight, self.image_weight_s, self.image_weight_d,
         self.image_lidar_weight) = model_cfgs.get("LOSS_WEIGHT")
        self.fusion_type = model_cfgs.get("FUSION_TYPE")
        self.ensemble_type = model_cfgs.get("ENSEMBLE_TYPE")
        if self.fusion_type != "cat":
            raise NotImplementedError("only FUSION_TYPE 'cat' exists in the reference (minkunet_ms_mm.py:380,489)")
        point_channels = (cs[4] + cs[6] + cs[8]) * exp
        self.fusion_channel = 2 * point_channels
        self.classifier_fusion = nn.Sequential(
            nn.Linear(self.fusion_channel, point_channels), _RowsBatchNorm1d(point_channels), nn.ReLU(inplace=True),
            nn.Linear(point_channels, self.num_class))
        self.weight_initialization()

    def _fov_targets(self, batch_dict):
        """labels of the FOV points: the camera label map at their pixels (minkunet_ms_mm.py:457)"""
        return batch_dict["image_targets_fov"]

    def prepare(self, batch_dict):
        x_ms = batch_dict["lidar_ms"]
        plan = self._index_plan(x_ms.C, x_ms.C.float())
        batch_dict["_plan"] = plan
        return plan

    def forward(self, batch_dict, return_logit=False, return_tta=False, defer=False, device_tail=None):
        maps = []
        if "rgb" in self.input_feat:
            maps.append(batch_dict["image_ms"])
        if "depth" in self.input_feat:
            maps.append(batch_dict["depth_map_ms"])
        if "lidar" in self.input_feat:
            maps.append(batch_dict["lidar_map_ms"])
        batch_dict["image_input"] = torch.cat(maps, dim=1)
        batch_dict = self.image_backbone(batch_dict)

        # FOV cloud: [LiDAR attributes | gathered image features | gathered image logits]
        x_fov = batch_dict["lidar_fov_ms"]
        cols = []
        if "lidar" in self.input_feat_lidar:
            cols.append(x_fov.F[:, :self.in_feature_dim - 1])
        if "image" in self.input_feat_lidar:
            cols.append(batch_dict["image_features_fov"])
        if "logit" in self.input_feat_lidar:
            cols.append(batch_dict["image_logits_fov"])
        x_fov.F = torch.cat(cols, dim=-1)
        fov_logits, x4_fov, y2_fov, y4_fov = self.lidar_backbone(batch_dict)

        # main branch on the fused cloud
        x_ms = batch_dict["lidar_ms"]
        x_ms.F = x_ms.F[:, :self.in_feature_dim]
        plan = batch_dict.get("_plan") or self.prepare(batch_dict)
        z1, z2, z3 = self._unet_point_features(x_ms.F, x_ms.F, plan)
        out_ms = self.classifier(torch.cat([z1, z2, z3], dim=1))

        # FOV encoder features onto every point of the fused cloud (minkunet_ms_mm.py:483,494,505)
        pts = PointTensor(x_ms.F, plan["point_coords"])
        z1_fov = voxel_to_point_fov(x4_fov, pts).F
        z2_fov = voxel_to_point_fov(y2_fov, pts).F
        z3_fov = voxel_to_point_fov(y4_fov, pts).F
        overlap = z1_fov.sum(-1) != 0
        fusion_features = torch.cat([z1, z2, z3, z1_fov, z2_fov, z3_fov], dim=1)

        if self.training:
            out_fusion = self.classifier_fusion(fusion_features[overlap])
            target = batch_dict["targets_ms"].F.long().cuda(non_blocking=True)
            img_logits = batch_dict["image_logits"].permute(0, 2, 3, 1).reshape(-1, self.num_class)
            img_targets = batch_dict["semantic_map_ms"].permute(0, 2, 3, 1).reshape(-1).to(target.dtype)
            fov_targets = self._fov_targets(batch_dict).to(target.dtype)
            crit = self.criterion_losses
            parts = {
                "loss_lidar": crit(out_ms, target, xyz=x_ms.C[:, :3].float(), offset=batch_dict["offset_ms"])
                * self.lidar_weight,
                "loss_fusion": crit(out_fusion, target[overlap]) * self.fusion_weight,
                "loss_image_s": crit(batch_dict["image_logits_fov"], fov_targets) * self.image_weight_s,
                "loss_image_d": crit(img_logits, img_targets) * self.image_weight_d,
                "loss_image_lidar": crit(fov_logits, fov_targets) * self.image_lidar_weight,
            }
            loss = sum(parts.values())
            disp = {"loss": LazyScalar(loss), **{k: LazyScalar(v) for k, v in parts.items()}}
            return {"loss": loss}, disp, dict(disp)

        # the rows of `overlap` as an integer index, taken ONCE: the boolean gather and the boolean assignment of the replace ensemble
        # each ran a `nonzero` with a host wait of its own.  Same rows in the same order - the bits of the boolean forms.
        overlap_rows = overlap.nonzero().reshape(-1)
        out_fusion = self.classifier_fusion(fusion_features.index_select(0, overlap_rows))
        if self.ensemble_type == "replace":
            # (out of place: `out_ms` is the classifier's own output - a hook or a caller that holds it keeps its rows)
            out_ms = out_ms.index_copy(0, overlap_rows, out_fusion.to(out_ms.dtype))
        return self._eval_outputs(out_ms, x_ms, batch_dict, return_logit or return_tta, defer, device_tail, ms=True)

    def forward_ensemble(self, batch_dict):
        return self.forward(batch_dict, return_tta=True)

    def fix_part_param(self):
        """Freeze the fused-cloud MinkUNet; train the image branch, the FOV encoder and the fusion head
        (minkunet_ms_mm.py:566-571: the TIAF stage starts from a trained MinkUNetMs checkpoint)."""
        for name, p in self.named_parameters():
            if not any(tag in name for tag in ("image_backbone", "classifier_fusion", "lidar_backbone")):
                p.requires_grad = False


class MinkUNetMsMmNus(MinkUNetMsMm):
    """nuScenes twin (minkunet_ms_mm_nus.py): identical network; the FOV points carry their own LiDAR labels
    (`targets_fov_ms`), used for both the sparse image loss and the FOV-encoder loss (:454-455, :526)."""

    def _fov_targets(self, batch_dict):
        return batch_dict["targets_fov_ms"].F.reshape(-1)
