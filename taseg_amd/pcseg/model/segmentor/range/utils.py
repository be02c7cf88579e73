"""The range-view family's kNN post-processing (reference pcseg/model/segmentor/range/utils.py:291-341): per-pixel classes back to
per-point labels.  The reference runs it one scan at a time and materialises two [1, S S, n] unfold gathers, a topk, two gathers and
a scatter_add_ into a [1, nclasses + 1, n] one-hot; here one scan or a whole batch is ONE launch of ts_rv_knn (csrc/range_view.hip),
one lane per point, no temporaries.  The rules are restated in include/taseg_hip.h; the one this library adds is the tie rule - the
K smallest by ascending (distance, slot) - where the reference's `topk(sorted=False)` states none."""
import torch
import torch.nn.functional as F
from torch import nn

from taseg_amd import backend as B
from taseg_amd.data.range_view import knn_weight
from taseg_amd.pcseg.loss.lovasz import lovasz_softmax

__all__ = ["KNN", "ClassWeightSemikitti", "DiceLoss", "CrossEntropyDiceLoss", "Lovasz_softmax", "BoundaryLoss"]

# SemanticKITTI's class frequencies as the reference lists them (range/utils.py:347-367): per training class the shares of the raw
# classes mapped onto it; the weight of a class is 1 / (their sum, left to right, + 0.001), class 0 (unlabelled) weighs 0
_SEMKITTI_FREQUENCIES = (
    (0.040818519255974316, 0.001789309418528068), (0.00016609538710764618,), (0.00039838616015114444,),
    (0.0020633612104619787, 0.00010157861367183268),
    (2.7879693665067774e-05, 0.0016218197275284021, 0.00011351574470342043, 4.3840131989471124e-05),
    (0.00017698551338515307, 0.00016059776092534436), (1.1065903904919655e-08, 0.00012709999297008662),
    (5.532951952459828e-09, 3.745553104802113e-05), (0.1987493871255525, 4.7084144280367186e-05), (0.014717169549888214,),
    (0.14392298360372,), (0.0039048553037472045,), (0.1326861944777486,), (0.0723592229456223,), (0.26681502148037506,),
    (0.006035012012626033,), (0.07814222006271769,), (0.002855498193863172,), (0.0006155958086189918,))


class ClassWeightSemikitti:
    @staticmethod
    def get_weight():
        out = [0.0]
        for shares in _SEMKITTI_FREQUENCIES:
            total = shares[0]
            for s in shares[1:]:
                total = total + s
            out.append(1.0 / (total + 0.001))
        return out


class DiceLoss(nn.Module):
    """the multi-channel Dice loss of range/utils.py:520-637 on softmax(predictions): one scalar; tensor ops in float32.  Where the
    reference reads `denominator.sum() == 0` on the host, the same choice is a torch.where here - no host read."""

    def __init__(self, weight=None, ignore_index=255, binary=False, reduction='mean'):
        super().__init__()
        if binary:
            raise NotImplementedError("the binary Dice loss is not used by the range-view segmentors")
        self.register_buffer("weight", weight)
        self.ignore_index, self.reduction = ignore_index, reduction

    def forward(self, predictions, targets):
        probs = F.softmax(predictions.float(), dim=1)
        c = probs.shape[1]
        void = targets == self.ignore_index
        keep = (~void).unsqueeze(1).to(probs.dtype)
        encoded = F.one_hot(targets.masked_fill(void, 0), c).permute(0, 3, 1, 2).to(probs.dtype) * keep
        numerator = 2 * (probs * encoded).sum(dim=(0, 2, 3))
        denominator = ((probs + encoded) * keep).sum(dim=(0, 2, 3))
        total = denominator.sum()
        weight = 1 if self.weight is None else self.weight / self.weight.mean()
        loss = (weight * (1 - numerator / (denominator + 0.0001))).sum() / c
        return torch.where(total == 0, total, loss)


class CrossEntropyDiceLoss(nn.Module):
    """cross entropy + Dice (range/utils.py:640-662); with reduction='none' - how SalsaNext builds it - the per-pixel cross entropy
    plus the Dice scalar on every pixel"""

    def __init__(self, reduction='mean', ignore_index=-100, weight=None):
        super().__init__()
        self.dice = DiceLoss(ignore_index=ignore_index, reduction=reduction, weight=weight)
        self.cross_entropy = nn.CrossEntropyLoss(weight=weight, reduction=reduction, ignore_index=ignore_index)

    def forward(self, predictions, targets):
        return self.cross_entropy(predictions.float(), targets) + self.dice(predictions, targets)


class Lovasz_softmax(nn.Module):
    """range/utils.py:509-517 on [B, C, H, W] probabilities and [B, H, W] labels: the rows of the channels-last map are the [P, C]
    matrix the library's Lovasz kernels (csrc/loss.hip behind pcseg.loss.lovasz) take - no per-class sort loop, no host read.
    Stated difference: a batch whose every pixel is `ignore` gives 0 here; the reference's `.mean()` of an empty tensor is NaN."""

    def __init__(self, classes='present', per_image=False, ignore=None):
        super().__init__()
        self.classes, self.per_image, self.ignore = classes, per_image, ignore

    def forward(self, probas, labels):
        if probas.dim() == 3:
            probas = probas.unsqueeze(1)
        rows = probas.permute(0, 2, 3, 1).reshape(-1, probas.shape[1])
        return lovasz_softmax(rows, labels.reshape(-1), classes=self.classes, per_image=self.per_image, ignore=self.ignore)


class BoundaryLoss(nn.Module):
    """Boundary loss (Bokhovkin et al., arXiv:1905.07852) as range/utils.py:665-714 computes it on probabilities: boundaries by a
    theta0 max-pool of the complement, precision / recall per sample and class, 1 - BF1 averaged; tensor ops in float32"""

    def __init__(self, theta0=3, theta=5):
        super().__init__()
        self.theta0, self.theta = theta0, theta

    def forward(self, pred, gt):
        pred = pred.float().contiguous()        # (plain NCHW for the pooling: csrc/image.hip says why channels-last pools are avoided)
        n, c = pred.shape[:2]
        pad = (self.theta0 - 1) // 2
        inv_gt = 1 - F.one_hot(gt, c).permute(0, 3, 1, 2).to(pred.dtype)
        gt_b = F.max_pool2d(inv_gt, kernel_size=self.theta0, stride=1, padding=pad) - inv_gt
        inv_pred = 1 - pred
        pred_b = F.max_pool2d(inv_pred, kernel_size=self.theta0, stride=1, padding=pad) - inv_pred
        gt_b, pred_b = gt_b.reshape(n, c, -1), pred_b.reshape(n, c, -1)
        hit = torch.sum(pred_b * gt_b, dim=2)
        precision = hit / (torch.sum(pred_b, dim=2) + 1e-7)
        recall = hit / (torch.sum(gt_b, dim=2) + 1e-7)
        bf1 = 2 * precision * recall / (precision + recall + 1e-7)
        return torch.mean(1 - bf1)


class KNN(torch.nn.Module):
    def __init__(self, params={'knn': 5, 'search': 5, 'sigma': 1.0, 'cutoff': 1.0}, nclasses=20):
        super().__init__()
        self.knn = params["knn"]
        self.search = params["search"]
        self.sigma = params["sigma"]
        self.cutoff = params["cutoff"]
        self.nclasses = nclasses
        self._weight = {}

    def weight(self, device):
        """1 - gaussian [search * search] float32: the reference's torch expression on the CPU, once, then uploaded"""
        key = (str(device), self.search, self.sigma)
        if key not in self._weight:
            self._weight[key] = knn_weight(self.search, self.sigma).to(device)
        return self._weight[key]

    def forward_batch(self, proj_range, unproj_range, proj_argmax, px, py, batch, err=None):
        """(label [n] int64, err [1] int32) for a batch: proj_range / proj_argmax [B, H, W], unproj_range / px / py / batch [n]"""
        if self.search % 2 == 0:
            raise ValueError("Nearest neighbor kernel must be odd number")
        label, err = B.rv_knn(proj_range.float(), proj_argmax.int(), unproj_range.float(), px.int(), py.int(), batch.int(),
                              self.weight(proj_range.device), self.knn, self.search, self.cutoff, self.nclasses, err=err)
        return label.long(), err

    def forward(self, proj_range, unproj_range, proj_argmax, px, py):
        """one scan, as the reference: proj_range / proj_argmax [H, W], unproj_range / px / py [n]; label [n] int64"""
        batch = torch.zeros(unproj_range.shape[0], dtype=torch.int32, device=proj_range.device)
        return self.forward_batch(proj_range[None], unproj_range, proj_argmax[None], px, py, batch)[0]
