"""Timings behind profiles/range_view_aug.txt (run on the GPU; fails without one):

    python tools/time_range_view_aug.py [--reps 20] [--points 120000]

build_range_view_train_batch on B = 2 and B = 30 recipe samples (salsanext_res34.yaml: every switch on) of `--points`-row synthetic
scans at 64 x 512, against
  (a) the same stage in numpy on the host, as a data loader computes it (np.delete, the four steps, the projection of
      tools/time_salsanext_step.py, np.roll / np.where for the image steps), plus the upload of its arrays;
  (b) for the image-level steps alone: ATen ops on the device (torch.roll, torch.where, bincount) on the output of two
      build_range_view_batch calls, against ts_rv_label_counts + ts_rv_compose on the same images (the upload of the records included).
Every pair is timed in alternation, `--reps` repetitions of a window around whole calls that ends in a device synchronise; medians and
quartiles are printed.  A path is called faster only where the gap between the medians exceeds the wider interquartile range of the
pair.  The compose kernel alone is timed between device events; the bytes it must move are computed from the shapes."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_salsanext_step import alternate, cloud, project_numpy, report  # noqa: E402

from taseg_amd import backend as B  # noqa: E402
from taseg_amd.data.range_view import (RangeViewAug, build_range_view_batch, build_range_view_train_batch, compose_record,  # noqa: E402
                                       draw_range_view_params, mix_bounds)

PASTE = (2, 3, 4, 5, 6, 7, 8, 12, 16, 18, 19)


def augment_numpy(points, labels, d):
    """LaserScan.open_scan's augmentation as the reference writes it (plain numpy, no fused multiply-add emulation)"""
    pts, lab = points.copy(), labels
    if d["drop"] is not None:
        pts, lab = np.delete(pts, d["drop"], axis=0), np.delete(lab, d["drop"])
    if d["flip"] in (1, 3):
        pts[:, 0] = -pts[:, 0]
    if d["flip"] in (2, 3):
        pts[:, 1] = -pts[:, 1]
    if d["scale"] is not None:
        pts[:, 0] *= d["scale"]
        pts[:, 1] *= d["scale"]
    if d["rotate"] is not None:
        c, s = d["rotate"]
        pts[:, :2] = np.dot(pts[:, :2], np.array([[c, s], [-s, c]]))
    if d["jitter"] is not None:
        pts[:, :3] += d["jitter"]
    return pts, lab


def checker(strategy, mixture, h, w):
    """[h, w] bool: where the mixed image holds the partner"""
    rows, cols = mix_bounds(strategy, h, w)
    cr, cc = np.zeros(h, dtype=np.int64), np.zeros(w, dtype=np.int64)
    for bound in rows:
        cr += np.arange(h) >= bound
    for bound in cols:
        cc += np.arange(w) >= bound
    even = (cr[:, None] + cc[None, :]) % 2 == 0
    return ~even if mixture == 1 else even


def image_numpy(points, labels, d, shift, h, w):
    pts, lab = augment_numpy(points, labels, d)
    scan, _, px, py, depth = project_numpy(pts, h, w)
    order = np.argsort(depth)[::-1]
    limg = np.zeros((h, w), dtype=np.int64)
    limg[py[order], px[order]] = lab[order]
    return np.roll(scan, -shift, axis=2), np.roll(limg, -shift, axis=1)


def host_stage(clouds, labels, params, h, w, dev):
    scans, labs = [], []
    for p in params:
        a, la = image_numpy(clouds[p["index"]], labels[p["index"]], p["scan"], p["shift"], h, w)
        b, lb = image_numpy(clouds[p["partner"]], labels[p["partner"]], p["partner_scan"], p["partner_shift"], h, w)
        take = checker(p["strategy"], p["mixture"], h, w) if p["mixture"] else np.zeros((h, w), dtype=bool)
        if p["paste"]:
            counts = np.bincount(lb.reshape(-1), minlength=32)
            take = take | (np.isin(lb, [c for c in PASTE if counts[c] > 20]))
        if p["union"]:
            take = take | (np.where(take, b[5], a[5]) == 0)
        scans.append(np.where(take[None], b, a))
        labs.append(np.where(take, lb, la)[None])
    return torch.from_numpy(np.stack(scans)).to(dev), torch.from_numpy(np.stack(labs)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=120000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_range_view_aug.py measures on the GPU: no device found")
    dev = torch.device("cuda")
    n, h, w = args.points, 64, 512
    print(f"device {torch.cuda.get_device_name(0)}; {args.reps} alternating repetitions; {n} points per scan; images {h} x {w}")
    clouds = [cloud(s, n) for s in (1, 2, 3, 4)]
    labels = [np.random.RandomState(10 + i).randint(0, 20, n).astype(np.int32) for i in range(4)]
    resident = [{"points": torch.from_numpy(c).to(dev), "labels": torch.from_numpy(l).to(dev), "name": str(i)}
                for i, (c, l) in enumerate(zip(clouds, labels))]
    for nb in (2, 30):
        rs, pyr = np.random.RandomState(nb), random.Random(nb)
        params = [draw_range_view_params(RangeViewAug.recipe(), i % 4, 4, lambda k: n, rs, pyr, (h, w)) for i in range(nb)]
        scans, partners = [resident[p["index"]] for p in params], [resident[p["partner"]] for p in params]
        kept = sum(p["scan"]["n"] - len(p["scan"]["drop"]) + p["partner_scan"]["n"] - len(p["partner_scan"]["drop"]) for p in params)

        def stage():
            return build_range_view_train_batch(scans, partners, params, (h, w))

        def host():
            return host_stage(clouds, labels, params, h, w, dev)

        got, ref = stage(), host()
        same = float((got["label_rv"] == ref[1]).float().mean())
        report(f"training batch, B = {nb} recipe samples ({2 * nb} clouds, {kept} surviving rows) at {h} x {w}",
               alternate({"build_range_view_train_batch (device)": stage, "numpy on the host + upload": host}, args.reps, 2 if nb == 2 else 1),
               f"labels equal at {same * 100:.3f} % of the pixels (numpy's float32 arctan2 / arcsin; no fma emulation on the host)")

        # ---- the image-level steps alone
        a, b = build_range_view_batch(scans, (h, w)), build_range_view_batch(partners, (h, w))
        recs = np.stack([compose_record(p, h, w) for p in params])
        masks = torch.from_numpy(np.stack([checker(p["strategy"], p["mixture"], h, w) if p["mixture"] else np.zeros((h, w), dtype=bool)
                                           for p in params])).to(dev)
        paste_set = torch.zeros(32, dtype=torch.bool, device=dev)
        paste_set[list(PASTE)] = True
        paste_on = torch.tensor([bool(p["paste"]) for p in params], device=dev).view(nb, 1, 1)
        union_on = torch.tensor([bool(p["union"]) for p in params], device=dev).view(nb, 1, 1)

        def kernels():
            rec = torch.from_numpy(recs).to(dev, non_blocking=True)
            return B.rv_compose(a["scan_rv"], a["label_rv"], rec, b["scan_rv"], b["label_rv"], B.rv_label_counts(b["label_rv"]))

        def aten():
            sa = torch.stack([torch.roll(a["scan_rv"][i], -p["shift"], 2) for i, p in enumerate(params)])
            la = torch.stack([torch.roll(a["label_rv"][i], -p["shift"], 2) for i, p in enumerate(params)])
            sb = torch.stack([torch.roll(b["scan_rv"][i], -p["partner_shift"], 2) for i, p in enumerate(params)])
            lb = torch.stack([torch.roll(b["label_rv"][i], -p["partner_shift"], 2) for i, p in enumerate(params)])
            counts = torch.stack([torch.bincount(lb[i].reshape(-1), minlength=32)[:32] for i in range(nb)])
            pasted = (paste_set.view(1, 32) & (counts > 20))[torch.arange(nb, device=dev).view(nb, 1, 1), lb[:, 0]] & paste_on
            take = masks | pasted
            take = take | (union_on & (torch.where(take, sb[:, 5], sa[:, 5]) == 0))
            return torch.where(take[:, None], sb, sa), torch.where(take[:, None], lb, la)

        k, t = kernels(), aten()
        assert torch.equal(k[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(k[1], t[1])
        report(f"image-level steps alone (shift, mix, paste, union), B = {nb} at {h} x {w}",
               alternate({"ts_rv_label_counts + ts_rv_compose": kernels, "ATen ops (roll, where, bincount)": aten}, args.reps, 10),
               "outputs equal bit for bit")
        rec = torch.from_numpy(recs).to(dev)
        counts = B.rv_label_counts(b["label_rv"])
        times = []
        for _ in range(args.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            B.rv_compose(a["scan_rv"], a["label_rv"], rec, b["scan_rv"], b["label_rv"], counts)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        q1, med, q3 = np.percentile(times[2:], [25, 50, 75])
        # per pixel: the chosen source's six values and label in (32 B), the partner's label (8 B) for the paste rule, six values and
        # the label out (32 B); the primary's mask (4 B) only with union
        must = nb * h * w * (32 + 8 + 32)
        print(f"    ts_rv_compose alone (device events, allocation of its outputs included): median {med * 1e3:.1f} us, quartiles "
              f"{q1 * 1e3:.1f} .. {q3 * 1e3:.1f}; bytes it must move {must / 1e6:.2f} MB -> {must / (med * 1e-3) / 1e9:.1f} GB/s")


if __name__ == "__main__":
    main()
