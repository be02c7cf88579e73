"""Measurement: F.spdownsample(coords, 2, 3, 1) - the overlapping-window branch on ts_downsample_windows (minimum pass, padded
key pass, radix sort, unique, unpack; one count read) - against the reference's own formulation (downsample.py:32-51) run as ATen
ops on the device: `repeat`, add, `cat`, the two masks, `torch.unique(dim=0)`.  Input: the voxels (0.05 m) of one 120k-point
synthetic scan.  Both forms end with a host read of the row count, so a repetition is timed on the host clock between two device
synchronisations.  One warm-up pass of each form (and the one comparison of their results, which must be the same rows), then the
forms ALTERNATE rep by rep so that both see the same machine; medians, quartiles and ranges go to profiles/downsample_windows.txt.
The rule for the word "faster": the gap between the medians must exceed the wider interquartile range of the two.
     timeout 600 python tools/time_downsample_windows.py [--reps 20] [--out profiles/downsample_windows.txt]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from oracle import ts_oracle as O
from taseg_amd.data.synthetic import synth_scan
from taseg_amd.torchsparse.nn import functional as F
from taseg_amd.torchsparse.nn.utils import get_kernel_offsets

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "downsample_windows.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"

STRIDE, KERNEL, TENSOR_STRIDE = 2, 3, 1
pts, _ = synth_scan(5)
pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
pc -= pc.min(0)
idx, _ = O.sparse_quantize(pc)
coords = torch.from_numpy(np.concatenate([pc[idx], np.zeros((len(idx), 1), np.int32)], 1)).cuda()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def ours():
    return F.spdownsample(coords, STRIDE, KERNEL, TENSOR_STRIDE)


def aten():
    """the formulation of downsample.py:32-51 on torch ops (what the reference library runs on a CUDA device)"""
    xyz, batch = coords[:, :3], coords[:, 3:]
    grid = torch.full((1, 3), STRIDE * TENSOR_STRIDE, dtype=torch.int, device=coords.device)
    offs = get_kernel_offsets(KERNEL, TENSOR_STRIDE, device=coords.device)
    lowest = xyz.min(dim=0, keepdim=True).values
    cand = (xyz[:, None, :].repeat(1, len(offs), 1) + offs).view(-1, 3)             # all K candidates of every row
    rows = torch.cat([batch.repeat(1, len(offs)).view(-1, 1), cand], dim=1)         # (b, x, y, z): the order unique sorts by
    on_grid, not_below = cand % grid == 0, cand >= lowest
    rows = torch.unique(rows[(on_grid & not_below).all(dim=1)], dim=0)
    return rows[:, [1, 2, 3, 0]]


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def quart(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):7.4f} ms  quartiles {q[0]:7.4f} .. {q[2]:7.4f}  range {min(v):7.4f} .. {max(v):7.4f}"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


a, b = ours(), aten()                                # the warm-up (code objects, workspaces) and the one comparison
assert a.shape == b.shape and torch.equal(a, b.to(a.dtype)), "the two forms give different rows"
say(f"spdownsample(stride {STRIDE}, kernel {KERNEL}, tensor stride {TENSOR_STRIDE}) on the {coords.shape[0]} voxels of one "
    f"{len(pts)}-point synthetic scan -> {a.shape[0]} rows (the same rows from both forms, checked); {args.reps} reps of each form, "
    f"alternating, host clock between two synchronisations; {torch.cuda.get_device_name(0)}")
t = {"ours": [], "aten": []}
for _ in range(args.reps):
    for k, fn in (("ours", ours), ("aten", aten)):
        t[k].append(once(fn))
say(f"  ours  ts_downsample_windows                        : {quart(t['ours'])}")
say(f"  aten  repeat / add / cat / masks / unique(dim=0)   : {quart(t['aten'])}")
med = {k: statistics.median(v) for k, v in t.items()}
spread = max(iqr(t["ours"]), iqr(t["aten"]))
gap = med["aten"] - med["ours"]
say(f"     aten - ours = {gap:+.4f} ms at the medians ({med['aten'] / med['ours']:.2f} x); the wider interquartile range of the two "
    f"{spread:.4f} ms")
say("     by the rule (a gap beyond that range): ours is " + ("faster" if gap > spread else "slower" if -gap > spread else "not distinguishable"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
