"""Measurement: the apply launch of FlatSGD.step() - ts_sgd_apply_segments (per-slot groups and skips, 16-byte accesses) against
ts_sgd_apply (one float per lane, one hyper-parameter set) - on the flat buckets of the benchmarked model (mk34, cr 1.0, 37.9 M
parameters, FlatSGD's default 32 MB buckets) in one process.  Device events around the per-bucket launches of one form, one warm-up
pass of every form, then the forms ALTERNATE rep by rep so that all see the same machine; medians, quartiles, ranges and GB/s at 20
bytes per element (p, g, m read; p, m written) go to profiles/flat_step.txt:

  a  ts_sgd_apply, one launch per bucket
  b  ts_sgd_apply_segments, one group (values as kernel arguments), nothing skipped - what bench.py's step runs
  c  ts_sgd_apply_segments, every slot a group of its own (the `sgd_fc` shape: values from the device array), for the record

(a) and (b) are first run once from the same buckets and must leave the same bits.  The criterion was set before the measurement: (b)
may not be slower than (a) by more than the wider interquartile range of the two.
     timeout 600 python tools/time_flat_step.py [--reps 20] [--out profiles/flat_step.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from taseg_amd import _lib as L
from taseg_amd.data.synthetic import make_model_cfg
from taseg_amd.optim import _GROUP, FlatSGD
from taseg_amd.pcseg.model import build_network

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flat_step.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"

model = build_network(make_model_cfg("MinkUNet", in_dim=4, cr=1.0), 20).cuda()
opt = FlatSGD(model, lr=1e-3, momentum=0.9, weight_decay=1e-4, max_norm=10.0)
buckets = opt.reducer.buckets
torch.manual_seed(0)
for b in buckets:                                   # gradients and momentum inside the slots, the padding stays zero
    for p, v in zip(b["params"], b["views"]):
        v.normal_(std=1e-2)
        opt._momentum_of[id(p)].normal_(std=1e-2)
opt.state[2], opt.state[3] = 1.0, 0.0
lib, HYPER = L.load(), (1e-3, 0.9, 1e-4)
n_total = sum(b["flat"].numel() for b in buckets)
n_slots = sum(len(b["params"]) for b in buckets)
own_group, base = [], 0                              # form (c): slot i of the model in group i
for b in buckets:
    rec = b["slot_host"].copy()
    rec["group"] = base + np.arange(len(rec))
    base += len(rec)
    own_group.append(torch.from_numpy(rec.view(np.uint8)).cuda())
groups_dev = torch.from_numpy(np.array([HYPER + (0,)] * n_slots, dtype=_GROUP).view(np.uint8)).cuda()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def form_a():
    for b in buckets:
        L.check(lib.ts_sgd_apply(L.ptr(b["pflat"]), L.ptr(b["flat"]), L.ptr(b["mflat"]), b["flat"].numel(), L.ptr(opt.state), *HYPER, 0,
                                 L.stream()), "ts_sgd_apply")


def segments(slots_of, groups, n_groups):
    for i, b in enumerate(buckets):
        L.check(lib.ts_sgd_apply_segments(L.ptr(b["pflat"]), L.ptr(b["flat"]), L.ptr(b["mflat"]), b["flat"].numel(), L.ptr(opt.state),
                                          L.ptr(slots_of(i, b)), len(b["params"]), L.ptr(b["tile_first"]), b["tile_first"].numel(),
                                          None, L.ptr(groups), n_groups, *HYPER, 0, 0, L.stream()), "ts_sgd_apply_segments")


def form_b():
    segments(lambda i, b: b["slots"], None, 1)


def form_c():
    segments(lambda i, b: own_group[i], groups_dev, n_slots)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def quart(v):
    q = statistics.quantiles(v, n=4)
    med = statistics.median(v)
    return (f"median {med:7.4f} ms  quartiles {q[0]:7.4f} .. {q[2]:7.4f}  range {min(v):7.4f} .. {max(v):7.4f}  "
            f"{20 * n_total / med / 1e6:7.1f} GB/s")


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


# the warm-up (code objects) - and the one comparison of what (a), (b) and (c) leave behind, from the same buckets
start = [(b["pflat"].clone(), b["mflat"].clone()) for b in buckets]
left = []
for fn in (form_a, form_b, form_c):
    for b, (p0, m0) in zip(buckets, start):
        b["pflat"].copy_(p0)
        b["mflat"].copy_(m0)
    fn()
    left.append([(b["pflat"].clone(), b["mflat"].clone()) for b in buckets])
for other in left[1:]:
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) and torch.equal(m.view(torch.int32), k.view(torch.int32))
               for (p, m), (q, k) in zip(left[0], other)), "the forms leave different bits"
del start, left
say(f"FlatSGD apply launch, mk34 cr 1.0: {sum(p.numel() for p in model.parameters())} parameters in {n_slots} slots, {len(buckets)} "
    f"buckets of {n_total} elements with the padding ({20 * n_total / 1e6:.0f} MB moved per step); {args.reps} reps of each form, "
    f"alternating, device events around the {len(buckets)} launches; {torch.cuda.get_device_name(0)}")
say("  (a), (b), (c) leave the same bits in the parameter and momentum buckets (checked)")
t = {k: [] for k in "abc"}
for _ in range(args.reps):
    for k, fn in (("a", form_a), ("b", form_b), ("c", form_c)):
        t[k].append(once(fn))
say(f"  a  ts_sgd_apply                                   : {quart(t['a'])}")
say(f"  b  ts_sgd_apply_segments, one group               : {quart(t['b'])}")
say(f"  c  ts_sgd_apply_segments, {n_slots} groups (device array) : {quart(t['c'])}")
med = {k: statistics.median(v) for k, v in t.items()}
spread = max(iqr(t["a"]), iqr(t["b"]))
say(f"     b - a = {med['b'] - med['a']:+.4f} ms at the medians = {100 * (med['b'] - med['a']) / med['a']:+.1f} %; the wider "
    f"interquartile range of the two {spread:.4f} ms")
say("     criterion (b may not be slower than a by more than that range): " + ("met" if med["b"] - med["a"] <= spread else "NOT met"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
