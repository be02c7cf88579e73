"""Evaluation / test-time-augmentation side of the path: what the reference's trainer does
with the dictionary a segmentor's eval branch returns (R/train.py:452-611) and the label remap of the saved predictions
(R/tta_remap.py:95-155), as plain functions around the model - no trainer, logger or file-system layout of its own.

    ret = model(batch)                                  # eval mode: point_predict / point_labels / point_predict_logits
    hist += scan_confusions(ret, unique_label)          # validation: R/train.py:535-540 -> per_class_iu
    logits = accumulate_votes(ret, votes)               # TTA: one batch entry per vote (collate_batch_tta), summed
    write_prediction(path, vote_payload(logits, "semantickitti"))
"""
import os
from typing import Dict, Iterable, List, Sequence

import numpy as np
from taseg_amd.options import options

__all__ = ["accumulate_votes", "vote_payload", "write_prediction", "remap_lut", "remap_labels", "fast_hist",
           "fast_hist_crop", "per_class_iu", "scan_confusions", "evaluate"]


def accumulate_votes(ret_dict: Dict, votes: int) -> np.ndarray:
    """Sum of the per-vote point logits of ONE scan (R/train.py:474-477, 505-508): under TTA the dataset returns
    `votes` augmented copies of a scan as one batch (semantickitti_voxel_ms.py:66-72, collate_batch_tta), the eval
    branch un-voxelises each copy onto the scan's points, and the trainer adds the raw logits."""
    logits = ret_dict["point_predict_logits"]
    if len(logits) < votes:
        raise ValueError(f"eval dictionary holds {len(logits)} votes, {votes} expected")
    total = np.array(logits[0], copy=True)
    for count in range(1, votes):
        if logits[count].shape != total.shape:
            raise ValueError("votes must cover the same points (one scan per TTA batch)")
        total += logits[count]
    return total


def vote_payload(point_logits: np.ndarray, dataset: str = "semantickitti") -> np.ndarray:
    """What the trainer writes per scan: arg-max class as [n, 1] uint32 (.label, SemanticKITTI; R/train.py:499-503) or
    uint8 (nuScenes lidarseg .bin; :519-523, where class 0 must not occur)."""
    return _class_payload(np.argmax(point_logits, axis=1), dataset)


def _class_payload(classes: np.ndarray, dataset: str) -> np.ndarray:
    """vote_payload behind its arg-max: the classes of one scan as the [n, 1] array of the dataset's label file"""
    pred = np.expand_dims(np.asarray(classes).reshape(-1), axis=1)
    if dataset.startswith("nuscenes"):
        out = pred.astype(np.uint8)
        if (out == 0).any():
            raise ValueError("nuScenes submission must not contain the ignored class 0 (R/train.py:523)")
        return out
    return pred.astype(np.uint32)


def _remap_table(remap, num_class: int) -> np.ndarray:
    """evaluate(remap=...): a {class: raw id} dictionary (remap_lut builds its table) or such a table, as a 1-d int32 array with an
    entry for every class the model can predict"""
    if isinstance(remap, dict):
        if not remap:
            raise ValueError("remap: an empty dictionary")
        remap = remap_lut(remap)
    elif not isinstance(remap, np.ndarray):
        raise TypeError(f"remap must be a {{class: raw id}} dictionary or a lookup array as remap_lut builds (got {type(remap).__name__})")
    if remap.ndim != 1 or remap.dtype.kind not in "iu":
        raise TypeError(f"remap: the lookup array must be 1-d and integer (got {remap.dtype}, {remap.shape})")
    if remap.shape[0] < num_class:
        raise ValueError(f"remap: the table has {remap.shape[0]} entries, the model {num_class} classes")
    return np.ascontiguousarray(remap.astype(np.int32))


def _remapped(payload: np.ndarray, lut) -> np.ndarray:
    """a payload through the table (remap_labels: a class has no instance bits, so all of it goes through), shape and type kept"""
    return payload if lut is None else remap_labels(payload, lut).reshape(-1, 1).astype(payload.dtype)


def write_prediction(path: str, payload: np.ndarray) -> str:
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    payload.tofile(path)
    return path


def remap_lut(remapdict: Dict[int, int]) -> np.ndarray:
    """Lookup table of R/tta_remap.py:103-108 (size max key + 100, unknown labels map to 0)."""
    lut = np.zeros(max(remapdict.keys()) + 100, dtype=np.int32)
    lut[list(remapdict.keys())] = list(remapdict.values())
    return lut


def remap_labels(label: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """R/tta_remap.py:147-154: the lower 16 bits (semantics) go through the table, the upper 16 (instance) stay."""
    label = np.asarray(label, dtype=np.uint32).reshape(-1)
    upper, lower = label >> 16, label & 0xFFFF
    return ((upper << 16) + lut[lower].astype(np.uint32)).astype(np.uint32)


def fast_hist(pred, label, n):
    """R/train.py:35-40."""
    pred, label = np.asarray(pred), np.asarray(label)
    k = (label >= 0) & (label < n)
    return np.bincount(n * label[k].astype(int) + pred[k], minlength=n ** 2)[:n ** 2].reshape(n, n)


def per_class_iu(hist):
    """R/train.py:43-44."""
    hist = np.asarray(hist)
    return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist) + 1e-9)


def fast_hist_crop(output, target, unique_label):
    """R/train.py:47-52: confusion matrix over `unique_label` (the learning classes without the ignored one)."""
    unique_label = np.asarray(unique_label)
    hist = fast_hist(np.asarray(output).flatten(), np.asarray(target).flatten(), np.max(unique_label) + 2)
    hist = hist[unique_label + 1, :]
    return hist[:, unique_label + 1]


def scan_confusions(ret_dict: Dict, unique_label: Sequence[int]) -> np.ndarray:
    """Sum over the scans of a batch of the cropped confusion matrices (R/train.py:535-540).  Note the reference's
    index shift: `unique_label` holds class ids - 1 (np.arange(num_class - 1), :148-150) and predictions / labels are
    compared as they are, so row r of the result is class r + 1."""
    total = None
    for pred, label in zip(ret_dict["point_predict"], ret_dict["point_labels"]):
        h = fast_hist_crop(pred, label, unique_label)
        total = h if total is None else total + h
    return total


def _staged(model, batches: Iterable[Dict], prefetch: bool):
    """the batches with their index plan (coordinates only: coordinate pyramid, kernel maps, class plans, trilinear maps) built one
    batch AHEAD on a second stream / worker thread (data.stage.DevicePrefetcher) - the role of the reference's DataLoader workers;
    an evaluation pass then is forward + un-voxelisation only (bench.py --eval: 5.2 + 1.2 ms instead of 2.9 + 5.2 + 1.2 per batch)"""
    prepare = getattr(model, "prepare", None)
    if not prefetch or prepare is None:
        yield from batches
        return
    from ..data.stage import DevicePrefetcher
    it = iter(batches)
    done = object()
    import os
    # two batches staged ahead (each on a stream and thread of its own; the batches are taken from `batches` one after the other, in
    # order): beside a forward pass one index plan takes longer than the pass (bench.py --eval: 5.9-6.3 -> 5.4 ms fp32, 4.2-5.1 -> 3.5-3.8
    # ms under autocast).  TASEG_EVAL_STAGE_DEPTH=1: one.
    pf = DevicePrefetcher(lambda: next(it, done), lambda b: b if b is done else prepare(b), threaded=True,
                          depth=options.eval_stage_depth)
    try:
        while True:
            batch = pf.next()
            if batch is done:
                return
            pf.prefetch_early()
            yield batch
    finally:
        pf.close()


def _prediction_path(save_dir, name, dataset):
    if dataset.startswith("nuscenes"):
        return os.path.join(save_dir, name.split("/")[-1])
    # .../sequences/<seq>/velodyne/<frame>.bin -> sequences/<seq>/predictions/<frame>.label
    seq_id, frame_id = name.split("/")[-3], name.split("/")[-1]
    return os.path.join(save_dir, "sequences", seq_id, "predictions", frame_id.replace("bin", "label"))


def _evaluate_on_device(model, batches, num_class, tta_votes, dataset, save_dir, prefetch, scores, predictions, remap):
    """evaluate(on_device=True): see there"""
    import inspect
    import torch
    from .model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    if "device_tail" not in inspect.signature(model.forward).parameters:
        raise ValueError(f"{type(model).__name__}.forward takes no `device_tail`: evaluate it with on_device=False")
    tail = DeviceEvalTail(num_class, next(model.parameters()).device, votes=tta_votes, dataset=dataset, scores=scores,
                          predictions=predictions, remap=remap)
    preds, kept_scores = [], []
    was_training = model.training
    model.eval()
    try:
        pending = None

        def collect(p):
            out = p.result()
            if not tta_votes:                                    # validation with predictions=True: one payload per scan
                preds.extend(out["payload"])
                if save_dir is not None:
                    for name, payload in zip(out["name"], out["payload"]):
                        write_prediction(_prediction_path(save_dir, name, dataset), payload)
                return
            preds.append(out["payload"])
            if scores is not None:
                kept_scores.append(out["scores"])
            if save_dir is not None:
                write_prediction(_prediction_path(save_dir, out["name"][0], dataset), out["payload"])

        for batch in _staged(model, batches, prefetch):
            with torch.no_grad():
                cur = model(batch, device_tail=tail)
            # one batch in flight - the next forward pass is issued before the host waits for this payload
            if pending is not None:
                collect(pending)
            pending = cur if (tta_votes or predictions) else None
        if pending is not None:
            collect(pending)
        if not tta_votes:
            full = tail.read()                                   # the ONE host read of a validation run's matrix
    finally:
        model.train(was_training)
    if tta_votes:
        return {"predictions": preds, "scores": kept_scores} if scores is not None else {"predictions": preds}
    hist = np.ascontiguousarray(full[1:, 1:])                    # fast_hist_crop: rows and columns 1 .. num_class - 1
    iou = per_class_iu(hist)
    out = {"iou": iou, "miou": float(np.nanmean(iou) * 100), "hist": hist}
    if predictions:
        out["predictions"] = preds
    return out


def evaluate(model, batches: Iterable[Dict], num_class: int, tta_votes: int = 0, dataset: str = "semantickitti",
             save_dir: str = None, prefetch: bool = True, on_device: bool = False, scores: str = None, predictions: bool = False,
             remap=None) -> Dict:
    """The loop body of Trainer.evaluate (R/train.py:465-540) over already collated, device-resident batches: validation
    (mIoU over the classes 1 .. num_class - 1) or, with tta_votes > 0, vote accumulation and optional writing of one
    prediction file per scan.  Returns {"iou", "miou", "hist"} or {"predictions": [...]}.  prefetch: stage the index plan of the
    next batch while this one runs (same results).
    predictions=True (validation only): the result also holds "predictions", one [n, 1] label payload per scan in the order of the
    scans (uint32, or uint8 for nuScenes: vote_payload of the scan's single-vote logits), and with `save_dir` every scan is written
    to its prediction file - the recipe's "history predictions" (R/docs/TASeg_Sem.md) from validation batches of any size.
    Without it `save_dir` is ignored in a validation run.
    remap: a {class: raw id} dictionary (data.semantickitti.LEARNING_MAP_INV) or a table as remap_lut builds; the payloads of a
    TTA run or of predictions=True go through it (remap_labels: R/tta_remap.py --inverse) before they are returned or written.
    on_device=True (all eight segmentors: MinkUNet, MinkUNetMs, MinkUNetMsMm, MinkUNetMsMmNus, MinkUNetMsKd, Cylinder_TS, SPVCNN, RPVNet - every
    forward that takes `device_tail`): the tail of every batch stays on the device (csrc/evaltail.hip).  Validation adds into a resident
    confusion matrix - no device -> host copy per batch, ONE host read at the end (after parallel.reduce_confusion); with
    predictions=True the label bytes and the per-scan counts of each batch follow it to the host, one batch in flight.  TTA sums
    the votes, takes the arg-max and sends only the label payload to the host - with scores="all" / "top3" also the summed
    logits / their three largest (R/train.py:487-501), returned as "scores".  `remap` is a table gather on the device.  Same
    results as the host path; what the host path raises per batch surfaces at the read."""
    import torch
    if scores is not None and not (on_device and tta_votes):
        raise ValueError("scores are kept by the device tail of a TTA run: on_device=True and tta_votes > 0")
    if predictions and tta_votes:
        raise ValueError("predictions=True is for validation batches (tta_votes == 0): a TTA run returns its predictions anyway")
    if remap is not None and not (predictions or tta_votes):
        raise ValueError("remap applies to label payloads: predictions=True or tta_votes > 0")
    lut = None if remap is None else _remap_table(remap, num_class)
    if on_device:
        return _evaluate_on_device(model, batches, num_class, tta_votes, dataset, save_dir, prefetch, scores, predictions, lut)
    unique_label = np.arange(num_class - 1)
    hist, preds = np.zeros((num_class - 1, num_class - 1), dtype=np.int64), []
    was_training = model.training
    model.eval()
    try:
        # one batch in flight: the forward pass of batch i + 1 is issued before the host waits for the arrays of batch i (models
        # whose forward takes `defer`; see minkunet.PendingPredictions)
        import inspect
        can_defer = "defer" in inspect.signature(model.forward).parameters

        def results():
            pending = None
            for batch in _staged(model, batches, prefetch):
                with torch.no_grad():
                    cur = model(batch, defer=True) if can_defer else model(batch)
                if pending is not None:
                    yield pending.result()
                if can_defer:
                    pending = cur
                else:
                    yield cur
            if pending is not None:
                yield pending.result()

        for ret in results():
            if tta_votes:
                payload = _remapped(vote_payload(accumulate_votes(ret, tta_votes), dataset), lut)
                preds.append(payload)
                if save_dir is not None:
                    write_prediction(_prediction_path(save_dir, ret["name"][0], dataset), payload)
            else:
                hist += scan_confusions(ret, unique_label)
                if predictions:
                    for name, classes in zip(ret["name"], ret["point_predict"]):
                        payload = _remapped(_class_payload(classes, dataset), lut)
                        preds.append(payload)
                        if save_dir is not None:
                            write_prediction(_prediction_path(save_dir, name, dataset), payload)
    finally:
        model.train(was_training)
    if tta_votes:
        return {"predictions": preds}
    iou = per_class_iu(hist)
    out = {"iou": iou, "miou": float(np.nanmean(iou) * 100), "hist": hist}
    if predictions:
        out["predictions"] = preds
    return out
