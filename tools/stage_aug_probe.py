"""Diagnostic: what `aug=` costs the batched SemanticKITTI data stage at the bench shape (4-scan TFA, bs 2, 2 x 5 x 120 000
points, voxel 0.05 m).  One fresh process; after warm-up the two forms - build_multiscan_batch(aug=None), which is the stage as
it was, and build_multiscan_batch(aug=<drawn per batch>) - alternate, each rep timed with a host clock around work that ends in a
device synchronise; medians and quartiles are printed.  ts_stage_augment alone is timed with device events over the same rows
(the stage calls it in place; same traffic): 24 B per point of xyz traffic plus 4 B of index, 32 B + 4 B on the 16-byte path that carries
the fourth column along.
     timeout 300 python tools/stage_aug_probe.py [--reps 60]
     rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stage_aug_probe.py --trace aug|none --reps 20
(--trace runs ONE form only, reps batches after 3 of warm-up: the difference of the two kernel counts over reps + 3 is the number
of extra launches per batch)"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd.data import augment as A
from taseg_amd.data import stage as S
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--trace", default="", choices=["", "aug", "none"])
args = ap.parse_args()

scans, npts = bench.make_multiscans(0, 2, 120000)
rng = np.random.RandomState(0)


def plain():
    return S.build_multiscan_batch(scans, 0.05, FLEXIBLE_STEPS_KITTI)


def augmented():
    return S.build_multiscan_batch(scans, 0.05, FLEXIBLE_STEPS_KITTI, aug=[A.draw_train_params(rng) for _ in scans])


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def quart(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):6.3f} ms (quartiles {q[0]:6.3f} .. {q[2]:6.3f}, min {min(v):6.3f})"


if args.trace:
    fn = augmented if args.trace == "aug" else plain
    for _ in range(3 + args.reps):
        fn()
    torch.cuda.synchronize()
    print(f"traced form: aug={args.trace}, {3 + args.reps} batches", flush=True)
    sys.exit(0)

for _ in range(5):
    plain(), augmented()
t_plain, t_aug = [], []
for _ in range(args.reps):                      # alternating: both forms see the same machine
    t_plain.append(once(plain))
    t_aug.append(once(augmented))
print(f"batched KITTI stage, bs 2, {npts} raw points, {args.reps} reps each, alternating", flush=True)
print(f"  aug=None : {quart(t_plain)}")
print(f"  aug=drawn: {quart(t_aug)}")
d = statistics.median(t_aug) - statistics.median(t_plain)
print(f"  difference of the medians: {1e3 * d:+.1f} us = {100 * d / statistics.median(t_plain):+.2f} %")

# the kernel alone, on the rows the stage hands it: all current + all history points, [n, 4], in place, one record per scan
n = sum(int(p.shape[0]) for s in scans for p in s["points"])
pts = torch.cat([p for s in scans for p in s["points"]], 0).contiguous()
idx = S.rows_index32([int(p.shape[0]) for s in scans for p in s["points"]], pts.device)
rec = torch.from_numpy(A.pack_params([A.draw_train_params(rng) for s in scans for _ in s["points"]])).to(pts.device)
dst = torch.empty_like(pts)           # (out of place here: 1 200 passes in place would walk the values off)
for _ in range(10):
    A.augment_points(pts, rec, idx, out=dst)
times = []
for _ in range(args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        A.augment_points(pts, rec, idx, out=dst)
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) / 20)
us = 1e3 * statistics.median(times)
print(f"ts_stage_augment alone, {n} rows of 4 floats (device events, 20 back-to-back launches per sample, L2/MALL-warm: "
      f"the rows are {16 * n / 2 ** 20:.1f} MiB): median {us:.1f} us per launch")
print(f"  algorithmic traffic 24 B xyz + 4 B index per point = {28 * n / 1e6:.1f} MB -> {28 * n / us / 1e3:.0f} GB/s ; "
      f"moved on the 16-byte path 36 B per point -> {36 * n / us / 1e3:.0f} GB/s")
