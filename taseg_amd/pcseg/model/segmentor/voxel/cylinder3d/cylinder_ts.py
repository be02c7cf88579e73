"""Cylinder_TS - the Cylinder3D segmentor on the torchsparse API (reference pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py;
recipes tools/cfgs/voxel/semantic_kitti/cylinder_cy480_cr{10,5}.yaml and the Waymo one).

Same modules, attribute names and `state_dict` (keys, order, shapes) as the reference, same `forward(batch_dict)` contract.  What
differs is where the work runs:

* `voxelize` (seg_utils.py:385-401) - ts_hash, ts_unique_i64 (voxel order = ascending hash, its inverse = `idx_query`), ts_count,
  the coordinates of one point per voxel, and the max kernel (ts_voxelize_max_*) in place of `torch_scatter.scatter_max`;
* conv -> LeakyReLU -> BatchNorm (-> + shortcut) of every block - `spnn.leaky_bn`: one node per direction on ts_leaky_bn_train_*;
* ReconBlock - three BatchNorms without activation (`spnn.bn_act(relu=False)`) and the gate x * (s(u) + s(v) + s(w)) as one kernel
  per direction (ts_sigmoid3_gate_*);
* the row gather of the point refinement (:542) - `functional.gather_rows`: a one-neighbour, weight-1 devoxelisation whose adjoint
  is a gather along the inverse map, so that the training step stays run-to-run bit-identical.

Reproduced as the reference has them (README "Cylinder_TS"):

* :539-542 looks every point up in `batch_dict['voxel_coord']` - rows in the data stage's `sparse_quantize` order - and indexes
  `up0e.F` with the result, whose rows are in ascending-hash order: a point receives the features of its own voxel only where the
  two orders agree;
* `DROPOUT_P` and the blocks' `drop_out` flag are read and never used;
* `self.name` is "RPV_Cylinder";
* `forward_ensemble` (ensemble=True) fails in the evaluation branch at the first scene (`out_batch_i_logits` is only bound on the
  other branch, :576-586).

`forward(batch_dict, device_tail=tail)` (evaluation mode; pcseg.eval.evaluate(on_device=True)) hands the evaluation branch to
minkunet.DeviceEvalTail.run_points: one batch-wide hash lookup in place of the per-scene queries, the confusion matrix / the vote
sums on the device.  Without a tail the branch is the reference's, host dictionary and all; in training mode a tail is ignored.
"""
import torch
from torch import nn

from taseg_amd import backend as B
from taseg_amd.pcseg.loss import Losses
from taseg_amd.torchsparse import PointTensor, SparseTensor
from taseg_amd.torchsparse import nn as spnn
from taseg_amd.torchsparse.nn import functional as F
from ...base_segmentors import BaseSegmentor

__all__ = ["Cylinder_TS"]

K133, K313, K333 = (1, 3, 3), (3, 1, 3), (3, 3, 3)


def voxelize(z: PointTensor) -> SparseTensor:
    """Max-voxelisation of a PointTensor whose coordinates are whole numbers stored as floats (seg_utils.py:385-401,
    voxel_type 'max'): one voxel per distinct coordinate, in ascending order of the coordinate hash."""
    coords = z.C.int()
    pc_hash = F.sphash(coords)
    sparse_hash, idx_query = B.unique_i64(pc_hash)
    m = sparse_hash.shape[0]
    counts = F.spcount(idx_query, m)
    # (the reference takes whichever point of a voxel a scatter_ leaves behind, seg_utils.py:22-26; all of them share the coordinate)
    inds = F.sphashquery(sparse_hash, pc_hash)
    out = SparseTensor(F.spvoxelize_max(z.F, idx_query, m), coords[inds], 1)
    out.cmaps.setdefault(out.stride, out.coords)
    z.additional_features["idx_query"][1] = idx_query.long()
    z.additional_features["counts"][1] = counts
    return out


def _norm(channels, if_dist, sparse=True):
    if sparse:
        return spnn.SyncBatchNorm(channels) if if_dist else spnn.BatchNorm(channels)
    return nn.SyncBatchNorm(channels) if if_dist else nn.BatchNorm1d(channels)


def _conv(c_in, c_out, kernel):
    return spnn.Conv3d(c_in, c_out, kernel_size=kernel, stride=1, bias=False)


class _Block(nn.Module):
    """conv / activation / BatchNorm triples registered under the reference's attribute names, in its order"""

    def _units(self, if_dist, spec, act=nn.LeakyReLU):
        for conv, act_name, bn, kernel, c_in, c_out in spec:
            setattr(self, conv, _conv(c_in, c_out, kernel))
            setattr(self, act_name, act())
            setattr(self, bn, _norm(c_out, if_dist))

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.SyncBatchNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _unit(self, conv, act, bn, x, residual=None):
        return spnn.leaky_bn(getattr(self, bn), getattr(self, conv)(x), residual=residual,
                             negative_slope=getattr(self, act).negative_slope)

    def _two_branches(self, x):
        """shortcut = the (conv1, conv1_2) branch; result = the (conv2, conv3) branch + shortcut (cylinder_ts.py:137-155, 227-244)"""
        shortcut = self._unit("conv1_2", "act1_2", "bn0_2", self._unit("conv1", "act1", "bn0", x))
        return self._unit("conv3", "act3", "bn2", self._unit("conv2", "act2", "bn1", x), residual=shortcut)


class ResContextBlock(_Block):
    def __init__(self, in_filters, out_filters, kernel_size=K333, stride=1, indice_key=None, if_dist=False):
        super().__init__()
        self._units(if_dist, [("conv1", "act1", "bn0", K133, in_filters, out_filters),
                              ("conv1_2", "act1_2", "bn0_2", K313, out_filters, out_filters),
                              ("conv2", "act2", "bn1", K313, in_filters, out_filters),
                              ("conv3", "act3", "bn2", K133, out_filters, out_filters)])
        self.weight_initialization()

    def forward(self, x):
        return self._two_branches(x)


class ResBlock(_Block):
    def __init__(self, in_filters, out_filters, dropout_rate, kernel_size=K333, stride=1, pooling=True, drop_out=True,
                 height_pooling=False, indice_key=None, if_dist=False):
        super().__init__()
        self.pooling = pooling
        self.drop_out = drop_out                  # (read, never used: cylinder_ts.py:174)
        self._units(if_dist, [("conv1", "act1", "bn0", K313, in_filters, out_filters),
                              ("conv1_2", "act1_2", "bn0_2", K133, out_filters, out_filters),
                              ("conv2", "act2", "bn1", K133, in_filters, out_filters),
                              ("conv3", "act3", "bn2", K313, out_filters, out_filters)])
        if pooling:
            self.pool = spnn.Conv3d(out_filters, out_filters, kernel_size=3, stride=2 if height_pooling else (2, 2, 1), bias=False)
        self.weight_initialization()

    def forward(self, x):
        res = self._two_branches(x)
        return (self.pool(res), res) if self.pooling else res


class UpBlock(_Block):
    def __init__(self, in_filters, out_filters, kernel_size=K333, indice_key=None, up_key=None, height_pooling=False,
                 if_dist=False):
        super().__init__()
        self._units(if_dist, [("trans_dilao", "trans_act", "trans_bn", K333, in_filters, out_filters),
                              ("conv1", "act1", "bn1", K133, out_filters, out_filters),
                              ("conv2", "act2", "bn2", K313, out_filters, out_filters),
                              ("conv3", "act3", "bn3", K333, out_filters, out_filters)])
        self.up_subm = spnn.Conv3d(out_filters, out_filters, kernel_size=3, stride=2 if height_pooling else (2, 2, 1), bias=False,
                                   transposed=True)
        self.weight_initialization()

    def forward(self, x, skip):
        up = self.up_subm(self._unit("trans_dilao", "trans_act", "trans_bn", x))
        up.F = up.F + skip.F
        for conv, act, bn in (("conv1", "act1", "bn1"), ("conv2", "act2", "bn2"), ("conv3", "act3", "bn3")):
            up = self._unit(conv, act, bn, up)
        return up


class ReconBlock(_Block):
    def __init__(self, in_filters, out_filters, kernel_size=K333, stride=1, indice_key=None, if_dist=False):
        super().__init__()
        self._units(if_dist, [("conv1", "act1", "bn0", (3, 1, 1), in_filters, out_filters),
                              ("conv1_2", "act1_2", "bn0_2", (1, 3, 1), in_filters, out_filters),
                              ("conv1_3", "act1_3", "bn0_3", (1, 1, 3), in_filters, out_filters)], act=nn.Sigmoid)

    def forward(self, x):
        u, v, w = (spnn.bn_act(getattr(self, bn), getattr(self, conv)(x), relu=False).F
                   for conv, bn in (("conv1", "bn0"), ("conv1_2", "bn0_2"), ("conv1_3", "bn0_3")))
        out = SparseTensor(F.sigmoid3_gate(x.F, u, v, w), x.C, x.s)
        out.cmaps, out.kmaps = x.cmaps, x.kmaps
        return out


class Cylinder_TS(BaseSegmentor):
    def __init__(self, model_cfgs, num_class: int = 20):
        super().__init__(model_cfgs, num_class)
        self.name = "RPV_Cylinder"
        self.in_feature_dim = model_cfgs.IN_FEATURE_DIM
        self.ignore_label = model_cfgs.IGNORE_LABEL
        self.init_size = init = model_cfgs.get("INIT_SIZE", 32)
        if_dist = model_cfgs.IF_DIST

        widths = (self.in_feature_dim, 64, 128, 256)
        pp = [_norm(widths[0], if_dist, sparse=False)]
        for c_in, c_out in zip(widths, widths[1:]):
            pp += [nn.Linear(c_in, c_out), _norm(c_out, if_dist, sparse=False), nn.ReLU()]
        self.PPmodel = nn.Sequential(*pp, nn.Linear(256, 256))
        self.fea_compression = nn.Sequential(nn.Linear(256, 16), nn.ReLU())

        self.downCntx = ResContextBlock(16, init, indice_key="pre", if_dist=if_dist)
        self.resBlock2 = ResBlock(init, 2 * init, 0.2, height_pooling=True, indice_key="down2", if_dist=if_dist)
        self.resBlock3 = ResBlock(2 * init, 4 * init, 0.2, height_pooling=True, indice_key="down3", if_dist=if_dist)
        self.resBlock4 = ResBlock(4 * init, 8 * init, 0.2, pooling=True, height_pooling=False, indice_key="down4", if_dist=if_dist)
        self.resBlock5 = ResBlock(8 * init, 16 * init, 0.2, pooling=True, height_pooling=False, indice_key="down5", if_dist=if_dist)
        self.upBlock0 = UpBlock(16 * init, 16 * init, indice_key="up0", up_key="down5", height_pooling=False, if_dist=if_dist)
        self.upBlock1 = UpBlock(16 * init, 8 * init, indice_key="up1", up_key="down4", height_pooling=False, if_dist=if_dist)
        self.upBlock2 = UpBlock(8 * init, 4 * init, indice_key="up2", up_key="down3", height_pooling=True, if_dist=if_dist)
        self.upBlock3 = UpBlock(4 * init, 2 * init, indice_key="up3", up_key="down2", height_pooling=True, if_dist=if_dist)
        self.ReconNet = ReconBlock(2 * init, 2 * init, indice_key="recon", if_dist=if_dist)
        self.logits = spnn.Conv3d(4 * init, self.num_class, kernel_size=3, stride=1, bias=True)

        label_smoothing = model_cfgs.get("LABEL_SMOOTHING", 0)
        self.in_channel_num = int(init * 64 / 16)
        self.point_refinement = model_cfgs.get("POINT_REFINEMENT", True)
        if self.point_refinement:
            self.change_dim = nn.Sequential(nn.Linear(self.in_channel_num, 256), _norm(256, if_dist, sparse=False), nn.LeakyReLU())
            self.point_logits = nn.Linear(256, self.num_class)

        default_loss_cfgs = {"LOSS_TYPES": ["CELoss", "LovLoss"], "LOSS_WEIGHTS": [1.0, 1.0], "KNN": 10}
        self.loss_cfgs = self.model_cfgs.get("LOSS_CONFIG", default_loss_cfgs)
        self.criterion_losses = Losses(loss_types=self.loss_cfgs.get("LOSS_TYPES", default_loss_cfgs["LOSS_TYPES"]),
                                       loss_weights=self.loss_cfgs.get("LOSS_WEIGHTS", default_loss_cfgs["LOSS_WEIGHTS"]),
                                       ignore_index=model_cfgs.IGNORE_LABEL, knn=self.loss_cfgs.get("KNN", default_loss_cfgs["KNN"]),
                                       label_smoothing=label_smoothing)
        self.loss_funs = nn.CrossEntropyLoss(ignore_index=self.ignore_label, label_smoothing=label_smoothing)

    weight_initialization = _Block.weight_initialization

    def get_training_loss(self, outputs, voxel_label, batch_dict):
        return self.criterion_losses(outputs, voxel_label, xyz=batch_dict["voxel_coord"][:, :3].float(), offset=batch_dict["offset"])

    def forward(self, batch_dict, ensemble=False, device_tail=None):
        point_feature = self.PPmodel(batch_dict["point_feature"])
        ret = voxelize(PointTensor(point_feature, batch_dict["point_coord"].float()))
        ret.F = self.fea_compression(ret.F)
        ret = self.downCntx(ret)
        down1c, down1b = self.resBlock2(ret)
        down2c, down2b = self.resBlock3(down1c)
        down3c, down3b = self.resBlock4(down2c)
        down4c, down4b = self.resBlock5(down3c)
        up4e = self.upBlock0(down4c, down4b)
        up3e = self.upBlock1(up4e, down3b)
        up2e = self.upBlock2(up3e, down2b)
        up1e = self.upBlock3(up2e, down1b)
        up0e = self.ReconNet(up1e)
        up0e.F = torch.cat((up0e.F, up1e.F), 1)
        logits = self.logits(up0e).F

        if self.point_refinement:
            # rows of `voxel_coord` (the data stage's order) index up0e.F (ascending-hash order): as the reference does, :539-542
            voxel_hash = F.sphash(batch_dict["voxel_coord"].int())
            idx_query = F.sphashquery(F.sphash(batch_dict["point_coord"].int()), voxel_hash)
            point_feature_cat = point_feature + self.change_dim(F.gather_rows(up0e.F, idx_query))
            point_logits = self.point_logits(point_feature_cat)
            loss_point = self.loss_funs(point_logits, batch_dict["point_label"])

        if self.training:
            voxel_hash = F.sphash(batch_dict["voxel_coord"].to(up0e.C))
            target = batch_dict["voxel_label"][F.sphashquery(F.sphash(up0e.C), voxel_hash)]
            loss = self.get_training_loss(logits, target, batch_dict)
            if self.point_refinement:
                ret_dict = {"loss": loss + loss_point}
                disp_dict = {"loss": loss.item(), "loss_point": loss_point.item()}
                tb_dict = {"loss": loss.item(), "loss_point": loss_point.item()}
            else:
                ret_dict, disp_dict, tb_dict = {"loss": loss}, {"loss": loss.item()}, {"loss": loss.item()}
            return ret_dict, tb_dict, disp_dict

        if device_tail is not None:       # evaluation on the device (minkunet.DeviceEvalTail.run_points): no logits cross to the host
            return device_tail.run_points(logits, up0e.C, batch_dict["point_coord"], batch_dict["point_label"], batch_dict["num_points"],
                                          batch_dict["name"])
        all_labels = batch_dict["point_label"]
        point_predict, point_labels, point_predict_logits = [], [], []
        for idx in range(int(batch_dict["point_coord"][:, -1].max() + 1)):
            mask_point = batch_dict["point_coord"][:, -1] == idx
            mask_logits = up0e.C[:, -1] == idx
            if ensemble:
                out_batch_i = logits[mask_logits]
            else:
                out_batch_i = logits[mask_logits].argmax(1)
                out_batch_i_logits = logits[mask_logits]
            idx_query = F.sphashquery(F.sphash(batch_dict["point_coord"][mask_point].to(up0e.C)), F.sphash(up0e.C[mask_logits]))
            n = batch_dict["num_points"][idx]
            point_predict.append(out_batch_i[idx_query][:n].cpu().numpy())
            point_labels.append(all_labels[mask_point][:n].cpu().numpy())
            point_predict_logits.append(out_batch_i_logits[idx_query][:n].cpu().numpy())     # (ensemble: unbound, as in the reference)
        return {"point_predict": point_predict, "point_labels": point_labels, "name": batch_dict["name"],
                "point_predict_logits": point_predict_logits}

    def forward_ensemble(self, batch_dict):
        return self.forward(batch_dict, ensemble=True)
