"""Evaluation of a range-view segmentor (SalsaNext; the reference's loop is validate_semkitti, pcseg/model/segmentor/range/utils.py:28-
150): the per-pixel confusion matrix of what the model returns, or - with the kNN post-processing - per-point labels, their confusion
matrix and the `.label` payloads.  `pcseg.eval.evaluate` is the voxel family's loop and is not touched; this one shares its metric,
payload and remap functions.

The reference post-processes one scan at a time (KNN.forward: a dozen launches and ~30 MB of temporaries per 120k-point scan); here a
batch is ONE ts_rv_knn launch, the confusion matrix is added on the device (a bincount per batch) and read ONCE at the end, together
with the flag word.  With predictions=True the labels of each batch follow to the host, one copy per batch."""
from typing import Dict, Iterable

import numpy as np
import torch

from .eval import _class_payload, _prediction_path, _remap_table, _remapped, per_class_iu, write_prediction

__all__ = ["evaluate_range_view"]


def evaluate_range_view(model, batches: Iterable[Dict], num_class: int, knn=None, predictions: bool = False, remap=None,
                        save_dir: str = None) -> Dict:
    """Validation over collated range-view batches (taseg_amd.data.range_view.build_range_view_batch).  Returns {"iou", "miou",
    "hist", "err"}: mIoU over the classes 1 .. num_class - 1 (`hist` is the cropped matrix, as pcseg.eval.evaluate's), `err` the OR of
    the kNN step's flag words.

    knn=None: the per-pixel matrix of the model's `point_predict` (arg-max over the classes) against its `point_labels`.
    knn=dict(knn=5, search=5, sigma=1.0, cutoff=1.0): per-point labels from one ts_rv_knn call per batch (the batch's `proj_range`,
    `unproj_range`, `proj_x`, `proj_y`, `batch`) against the batch's `point_labels` [n]; with predictions=True the result also holds
    "predictions", one [n, 1] uint32 payload per scan in the order of the scans, through `remap` (a {class: raw id} dictionary or a
    remap_lut table) when given, and with `save_dir` every scan is written to its prediction file (the batch's `scan_name`)."""
    if (predictions or remap is not None or save_dir is not None) and knn is None:
        raise ValueError("label payloads are per point: give the kNN parameters (knn=dict(knn=5, search=5, sigma=1.0, cutoff=1.0))")
    if remap is not None and not predictions:
        raise ValueError("remap applies to label payloads: predictions=True")
    lut = None if remap is None else _remap_table(remap, num_class)
    post = None
    if knn is not None:
        from .model.segmentor.range.utils import KNN
        post = KNN(dict(knn), num_class)
    device = next(model.parameters()).device
    hist = torch.zeros(num_class * num_class, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    preds = []
    was_training = model.training
    model.eval()
    try:
        for batch in batches:
            with torch.no_grad():
                ret = model(batch)
                classes = ret["point_predict"].argmax(dim=1)                                  # [B, H, W]
                if post is None:
                    got, want = classes.reshape(-1), ret["point_labels"].reshape(-1).to(device)
                else:
                    got, _ = post.forward_batch(batch["proj_range"], batch["unproj_range"], classes, batch["proj_x"], batch["proj_y"],
                                                batch["batch"], err=err)
                    want = batch["point_labels"].reshape(-1).to(device).long()
                keep = (want >= 0) & (want < num_class)
                hist += torch.bincount(num_class * want[keep] + got[keep], minlength=num_class * num_class)[:num_class * num_class]
            if predictions:
                labels = got.cpu().numpy()
                offset = np.asarray(batch["offset"]).astype(np.int64)
                for k, name in enumerate(batch["scan_name"]):
                    payload = _remapped(_class_payload(labels[offset[k]:offset[k + 1]], "semantickitti"), lut)
                    preds.append(payload)
                    if save_dir is not None:
                        write_prediction(_prediction_path(save_dir, name, "semantickitti"), payload)
        full = torch.cat([hist, err.long()]).cpu().numpy()                                    # the ONE host read of the matrix
    finally:
        model.train(was_training)
    matrix = np.ascontiguousarray(full[:-1].reshape(num_class, num_class)[1:, 1:])            # fast_hist_crop: classes 1 .. num_class - 1
    iou = per_class_iu(matrix)
    out = {"iou": iou, "miou": float(np.nanmean(iou) * 100), "hist": matrix, "err": int(full[-1])}
    if predictions:
        out["predictions"] = preds
    return out
