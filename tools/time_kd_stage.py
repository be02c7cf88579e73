"""Measurement: the mask-distillation recipe's data stage, `build_kd_batch` (taseg_amd/data/kd.py), against the construction of
`bench.py --workload kd`, and ts_stage_layout_pair against the sequence it replaces - at the KD line's stage shape (bs 6, 120k-point
synthetic scans, history 16, `bench.make_multiscans(..., pseudo_flip=0.1)`, voxel 0.05 m).  One fresh process, device events, one
warm-up pass of every form, then the forms ALTERNATE rep by rep so that all see the same machine; medians, quartiles and the full
range are written to profiles/kd_stage.txt:

  a  bench.py's construction: build_multiscan_batch twice (with and without the pseudo labels), `lidar_ms` of the second call kept
  b  build_kd_batch with ts_stage_layout_pair: one walk, one pose fuse, the pair kernel, three voxelisations
  c  (b) with ts_stage_layout_pair swapped for kd._layout_sequence: ts_stage_keep_flags -> nonzero -> searchsorted ->
     ts_stage_layout once per cloud on the four-column rows, the time flag appended to the kept rows only, the teacher's count
     before the clamp from one more ts_stage_keep_flags launch without a minimum and a running sum
  (kd._PAIR_KERNEL chooses between (b) and (c); the file records which of them build_kd_batch runs by default)
  d  a mixed + augmented batch (PolarMix with swap and paste for every sample, partner = the next sample of the batch, all four
     augmentations), for the record

(a), (b) and (c) build the same three clouds - checked once.  A stage call holds host reads, so its device-event time includes the
host's share between the launches - it is the time of the call, which is what a training step waits for when the stage is not
overlapped.
     timeout 900 python tools/time_kd_stage.py [--reps 20] [--out profiles/kd_stage.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd.data import augment as A
from taseg_amd.data import kd as KD
from taseg_amd.data import mix as M
from taseg_amd.data import stage as S
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI as STEPS

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=6)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--history", type=int, default=16)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kd_stage.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"

scans, npts = bench.make_multiscans(0, args.batch, args.points, history=args.history, pseudo_flip=0.1)
scans_gt = [{k: v for k, v in s.items() if k != "pseudo"} for s in scans]
partners = [scans[(b + 1) % len(scans)] for b in range(len(scans))]
rng = np.random.RandomState(0)
omega = M.draw_omega(rng)
mix = [M.MixParams(kind=M.POLAR, alpha=float(a), beta=float(a + np.pi), swap=True, paste=True, omega=omega)
       for a in (rng.random_sample(len(scans)) - 1) * np.pi]
aug = [A.draw_train_params(rng) for _ in scans]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def form_a():
    bd = S.build_multiscan_batch(scans, 0.05, STEPS)
    bd["lidar_ms_gt"] = S.build_multiscan_batch(scans_gt, 0.05, STEPS)["lidar_ms"]
    return bd


def with_switch(pair_kernel):
    was, KD._PAIR_KERNEL = KD._PAIR_KERNEL, pair_kernel
    try:
        return KD.build_kd_batch(scans, 0.05, STEPS)
    finally:
        KD._PAIR_KERNEL = was


def form_b():
    return with_switch(True)


def form_c():
    return with_switch(False)


def form_d():
    return KD.build_kd_batch(scans, 0.05, STEPS, aug=aug, mix=mix, partners=partners)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def quart(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):7.3f} ms  quartiles {q[0]:7.3f} .. {q[2]:7.3f}  range {min(v):7.3f} .. {max(v):7.3f}"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def same(x, y):
    return x.C.shape == y.C.shape and torch.equal(x.C, y.C) and torch.equal(x.F.view(torch.int32), y.F.view(torch.int32))


# the warm-up: code objects, caches of the layouts, allocator - and the one comparison of what the forms build
a, b, c, d = form_a(), form_b(), form_c(), form_d()
n_hist = sum(int(p.shape[0]) for s in scans for p in s["points"][:-1])
rows = {k: int(b[k].reshape(-1).sum()) for k in ("num_points", "num_points_ms", "num_points_ms_gt")}
# (the teacher's cloud of (a) is shifted by its own minimum, (b)'s by the student's: the same voxels where the two minima agree,
#  which the clamp to the current scan's minimum makes them do)
assert all(same(a[k], b[k]) and same(b[k], c[k]) for k in ("lidar", "lidar_ms", "lidar_ms_gt")), "the forms build different clouds"
assert torch.equal(b["offset_ms_gt"], c["offset_ms_gt"]) and torch.equal(b["num_points_ms_gt"], c["num_points_ms_gt"])
del a, c
say(f"mask-distillation data stage, bs {len(scans)}, {args.points} points per scan, history {args.history}, {npts} raw points, "
    f"{n_hist} history rows; {args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
say(f"  rows: current {rows['num_points']}, student {rows['num_points_ms']}, teacher {rows['num_points_ms_gt']} before its clamp; "
    f"voxels: {b['lidar'].C.shape[0]} / {b['lidar_ms'].C.shape[0]} / {b['lidar_ms_gt'].C.shape[0]}; (a), (b), (c): the same three "
    f"clouds (checked)")
t = {k: [] for k in "abcd"}
for _ in range(args.reps):
    for k, fn in (("a", form_a), ("b", form_b), ("c", form_c), ("d", form_d)):
        t[k].append(once(fn)[0])
say(f"  a  two build_multiscan_batch calls (bench.py)         : {quart(t['a'])}")
say(f"  b  build_kd_batch, ts_stage_layout_pair               : {quart(t['b'])}")
say(f"  c  build_kd_batch, _layout_sequence                   : {quart(t['c'])}")
say(f"  d  build_kd_batch, PolarMix x {len(scans)} + augmentation      : {quart(t['d'])}   ({d['lidar_ms'].C.shape[0]} / "
    f"{d['lidar_ms_gt'].C.shape[0]} voxels)")
med = {k: statistics.median(v) for k, v in t.items()}
say(f"     b - a = {med['b'] - med['a']:+.3f} ms at the medians = {100 * (med['b'] - med['a']) / med['a']:+.1f} %")
spread = max(iqr(t["b"]), iqr(t["c"]))
say(f"     b - c = {med['b'] - med['c']:+.3f} ms at the medians; the wider interquartile range of the two {spread:.3f} ms")
say("     verdict: " + ("the kernel is faster than the sequence it replaces by more than that spread"
                        if med["c"] - med["b"] > spread else
                        "the kernel is NOT faster than the sequence it replaces by more than that spread"))
say(f"     build_kd_batch runs form ({'b' if KD._PAIR_KERNEL else 'c'}) by default")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
