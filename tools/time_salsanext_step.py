"""Timings behind profiles/salsanext.txt (run on the GPU; fails without one):

    python tools/time_salsanext_step.py [--reps 20] [--points 120000]

  1. ts_rv_knn on one and on two `--points` scans at 64 x 2048 against the reference's formulation of the kNN step as ATen ops on the
     device (unfold, gather, topk, gather, scatter_add into a one-hot), one scan at a time as the reference runs it;
  2. build_range_view_batch (two scans, 64 x 2048) against the projection in numpy on the host plus the upload of its images;
  3. one SalsaNext training step (forward, backward; B = 2 at 64 x 512, LOSS 'dice' with the Lovasz and boundary terms) in fp32 and under
     autocast, and each loss term alone (forward + backward from the logits) - the share a fused Dice / boundary kernel could win.

Every pair is timed in alternation, `--reps` repetitions of a window that ends in a device synchronise; medians and quartiles are
printed.  A path is called faster only where the gap between the medians exceeds the wider interquartile range of the pair.  The bytes
each kernel must move are computed from the shapes."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from taseg_amd.data.range_view import build_range_view_batch, knn_weight  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg  # noqa: E402


def cloud(seed, n):
    rng = np.random.RandomState(seed)
    yaw, pitch, depth = rng.uniform(-np.pi, np.pi, n), np.deg2rad(rng.uniform(-25.0, 3.0, n)), rng.uniform(2.0, 60.0, n)
    return np.stack([depth * np.cos(pitch) * np.cos(yaw), depth * np.cos(pitch) * np.sin(yaw), depth * np.sin(pitch),
                     rng.uniform(0, 1, n)], 1).astype(np.float32)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(pairs, reps, iters):
    """{name: [ms per call] * reps}, the candidates timed one after the other within every repetition"""
    for fn in pairs.values():
        window(fn, 2)                                             # warm-up of every shape
    out = {k: [] for k in pairs}
    for _ in range(reps):
        for k, fn in pairs.items():
            out[k].append(window(fn, iters))
    return out


def report(title, times, note=""):
    print(title)
    stats = {}
    for k, v in times.items():
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        stats[k] = (med, q3 - q1)
        print(f"    {k:<44s} median {med:9.4f} ms   quartiles {q1:9.4f} .. {q3:9.4f}")
    names = list(stats)
    if len(names) == 2:
        (a, ia), (b, ib) = stats[names[0]], stats[names[1]]
        gap, spread = abs(a - b), max(ia, ib)
        verdict = (f"{names[0] if a < b else names[1]} is faster ({max(a, b) / min(a, b):.2f} x): gap {gap:.4f} ms > wider IQR {spread:.4f} ms"
                   if gap > spread else f"no difference shown: gap {gap:.4f} ms <= wider IQR {spread:.4f} ms")
        print("    -> " + verdict)
    if note:
        print("    " + note)


def knn_aten(proj_range, unproj_range, proj_argmax, px, py, weight, k, search, cutoff, nclasses):
    """the reference's formulation of the kNN step for ONE scan, as ATen ops on the device"""
    h, w = proj_range.shape
    n = unproj_range.shape[0]
    pad = (search - 1) // 2
    F = torch.nn.functional
    idx = py.long() * w + px.long()
    ranges = F.unfold(proj_range[None, None], kernel_size=(search, search), padding=(pad, pad))[:, :, idx]
    ranges[ranges < 0] = float("inf")
    ranges[:, (search * search - 1) // 2, :] = unproj_range
    dist = torch.abs(ranges - unproj_range) * weight.view(1, -1, 1)
    _, nearest = dist.topk(k, dim=1, largest=False, sorted=False)
    classes = F.unfold(proj_argmax[None, None].float(), kernel_size=(search, search), padding=(pad, pad)).long()[:, :, idx]
    votes = torch.gather(classes, 1, nearest)
    if cutoff > 0:
        votes[torch.gather(dist, 1, nearest) > cutoff] = nclasses
    onehot = torch.zeros((1, nclasses + 1, n), device=proj_range.device, dtype=proj_range.dtype)
    onehot.scatter_add_(1, votes, torch.ones_like(votes, dtype=proj_range.dtype))
    return (onehot[:, 1:-1].argmax(dim=1) + 1).view(n)


def project_numpy(points, h, w, fov_up=3.0, fov_down=-25.0):
    """the projection of one scan in numpy on the host, as a data loader computes it: norm, two inverse trigonometric functions, an
    argsort by depth, fancy assignments; returns the [6, h, w] input and the range image"""
    down, up = fov_down / 180.0 * np.pi, fov_up / 180.0 * np.pi
    fov = abs(down) + abs(up)
    xyz, rem = points[:, :3], points[:, 3]
    depth = np.linalg.norm(xyz, 2, axis=1)
    yaw, pitch = -np.arctan2(xyz[:, 1], xyz[:, 0]), np.arcsin(xyz[:, 2] / depth)
    px = np.maximum(0, np.minimum(w - 1, np.floor(0.5 * (yaw / np.pi + 1.0) * w))).astype(np.int32)
    py = np.maximum(0, np.minimum(h - 1, np.floor((1.0 - (pitch + abs(down)) / fov) * h))).astype(np.int32)
    order = np.argsort(depth)[::-1]
    rng = np.full((h, w), -1, dtype=np.float32)
    img = np.full((h, w, 5), -1, dtype=np.float32)
    index = np.full((h, w), -1, dtype=np.int32)
    rng[py[order], px[order]] = depth[order]
    img[py[order], px[order], :3] = xyz[order]
    img[py[order], px[order], 3] = rem[order]
    index[py[order], px[order]] = order
    img[..., 4] = rng
    scan = np.concatenate([img / np.array([50, 50, 3, 1, 80], dtype=np.float32), (index > 0).astype(np.float32)[..., None]], -1)
    return np.ascontiguousarray(scan.transpose(2, 0, 1)), rng, px, py, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=120000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_salsanext_step.py measures on the GPU: no device found")
    from taseg_amd.pcseg.model.segmentor.range.salsanext.model.semantic.salsanext import SalsaNext
    from taseg_amd.pcseg.model.segmentor.range.utils import KNN
    dev = torch.device("cuda")
    n, h, w = args.points, 64, 2048
    print(f"device {torch.cuda.get_device_name(0)}; {args.reps} alternating repetitions; {n} points per scan")

    # ---- 1. kNN
    clouds = [cloud(s, n) for s in (1, 2)]
    scans = [{"points": torch.from_numpy(c).to(dev), "labels": torch.from_numpy(np.random.RandomState(i).randint(0, 20, n).astype(np.int32)).to(dev),
              "name": str(i)} for i, c in enumerate(clouds)]
    post = KNN(nclasses=20)
    weight = knn_weight(5, 1.0).to(dev)
    for count in (1, 2):
        b = build_range_view_batch(scans[:count], (h, w))
        cls = b["label_rv"][:, 0].int().contiguous()
        off = b["offset"].tolist()

        def ours():
            return post.forward_batch(b["proj_range"], b["unproj_range"], cls, b["proj_x"], b["proj_y"], b["batch"])[0]

        def aten():
            return [knn_aten(b["proj_range"][i], b["unproj_range"][off[i]:off[i + 1]], cls[i], b["proj_x"][off[i]:off[i + 1]],
                             b["proj_y"][off[i]:off[i + 1]], weight, 5, 5, 1.0, 20) for i in range(count)]

        same = torch.cat(aten()) == ours()
        must = count * (h * w * 8 + n * 20)             # the two images once; per point range, px, py, batch in and the label out
        temp = count * n * (25 * 4 * 3 + 25 * 8 + 5 * 8 * 2 + 21 * 4)
        report(f"kNN step, {count} scan(s) of {n} points at {h} x {w} (K 5, S 5, cutoff 1.0, 20 classes)",
               alternate({"ts_rv_knn (one launch)": ours, "ATen formulation, one scan at a time": aten}, args.reps, 10),
               f"labels equal at {float(same.float().mean()) * 100:.3f} % of the points (ties: topk states no rule); bytes the step must "
               f"move {must / 1e6:.2f} MB; temporaries of the ATen formulation ~{temp / 1e6:.1f} MB")

    # ---- 2. projection
    def stage():
        return build_range_view_batch(scans, (h, w))

    def host():
        parts = [project_numpy(c, h, w) for c in clouds]
        return (torch.from_numpy(np.stack([p[0] for p in parts])).to(dev), torch.from_numpy(np.stack([p[1] for p in parts])).to(dev),
                [torch.from_numpy(np.concatenate([p[k] for p in parts])).to(dev) for k in (2, 3, 4)])

    must = 2 * (n * (16 + 4 + 4 + 12) + h * w * (8 + 8 + 6 * 4 + 4 + 4 + 8) + n * 4)
    report(f"range-view batch, 2 scans of {n} points at {h} x {w}",
           alternate({"build_range_view_batch (device)": stage, "numpy on the host + upload": host}, args.reps, 3),
           f"bytes the two kernels must move {must / 1e6:.2f} MB (rows in, three per-row outputs, the winner table written and read, "
           f"the winners' rows and labels, six planes + range + index + label out)")

    # ---- 3. training step
    hh, ww = 64, 512
    batch = build_range_view_batch(scans, (hh, ww))
    cfg = make_model_cfg("SalsaNext", LOSS="dice", IF_LS_LOSS=True, IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=1.0)
    model = fill_parameters(SalsaNext(cfg, 20), seed=1).to(dev).train()

    def step(amp):
        def run():
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                ret, _, _ = model(batch)
            model.zero_grad(set_to_none=True)
            ret["loss"].float().backward()
        return run

    report(f"SalsaNext training step (forward + backward), B = 2 at {hh} x {ww}, LOSS 'dice' + Lovasz + boundary",
           alternate({"fp32": step(False), "autocast (float16)": step(True)}, args.reps, 3))
    logits = torch.randn((2, 20, hh, ww), device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    label = batch["label_rv"][:, 0]

    def term(fn):
        def run():
            logits.grad = None
            fn().backward()
        return run

    soft = lambda: torch.softmax(logits, dim=1)                                     # noqa: E731
    report("the loss terms alone, forward + backward from the logits (each includes its own softmax)",
           alternate({"cross entropy + Dice (tensor ops)": term(lambda: model.WCE(logits, label).mean()),
                      "Lovasz (library kernels)": term(lambda: model.LS(soft(), label)),
                      "boundary (tensor ops)": term(lambda: model.BD(soft(), label))}, args.reps, 3))


if __name__ == "__main__":
    main()
