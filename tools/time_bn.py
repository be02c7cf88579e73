"""Measurement: ts_bn_act_train_forward / _backward and their _f16 forms (residual + ReLU, the mask in the backward) at three layer
shapes of the headline step - the stride-1 level at 32 channels, the stride-2 level at 96 and the stride-16 level at 256, the row
counts those of bench.py's default batch (2 x 120k points).  One fresh process, device events, one warm-up pass of every form, then
the forms ALTERNATE rep by rep so that all see the same machine; ms: median (lower .. upper quartile).  One library per process:
run it once more with TASEG_HIP_LIB=<other .so> to compare two builds.
     timeout 300 python tools/time_bn.py [--reps 200] [--out FILE]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from taseg_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
lib = L.load()
DEV = "cuda"
coords = bench.make_scans(0, 2, 120000, "minkunet")[0]


def rows(stride):
    c = coords.clone()
    c[:, :3] = torch.div(c[:, :3], stride, rounding_mode="floor")
    return int(torch.unique(c, dim=0).shape[0])


forms = []
for stride, c in ((1, 32), (2, 96), (16, 256)):
    n = rows(stride)
    for half in (False, True):
        dt, sfx, per = (torch.float16, "_f16", 8) if half else (torch.float32, "", 4)
        g = torch.Generator(device="cpu").manual_seed(c + int(half))
        x, res, gy = ((torch.randn(n, c, generator=g)).to(dt).to(DEV) for _ in range(3))
        w, b = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
        rm, rv, nbt = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
        mean, invstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        y, gx, gres = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        gw, gb = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        mask = torch.zeros(n * (c // per), dtype=torch.uint8, device=DEV)
        ws = torch.empty(lib.ts_bn_train_workspace_bytes(c), dtype=torch.uint8, device=DEV)
        keep = (x, res, gy, w, b, rm, rv, nbt, mean, invstd, y, gx, gres, gw, gb, mask, ws)

        def fwd(sfx=sfx, n=n, c=c, t=keep):
            x, res, gy, w, b, rm, rv, nbt, mean, invstd, y, gx, gres, gw, gb, mask, ws = t
            L.check(getattr(lib, "ts_bn_act_train_forward" + sfx)(
                L.ptr(x), L.ptr(res), L.ptr(w), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(nbt), n, c, 1e-5, 0.1, 1, L.ptr(mean), L.ptr(invstd),
                L.ptr(y), L.ptr(mask), L.ptr(ws), ws.numel(), L.stream()), "ts_bn_act_train_forward" + sfx)

        def bwd(sfx=sfx, n=n, c=c, t=keep):
            x, res, gy, w, b, rm, rv, nbt, mean, invstd, y, gx, gres, gw, gb, mask, ws = t
            L.check(getattr(lib, "ts_bn_act_train_backward" + sfx)(
                L.ptr(gy), L.ptr(mask), L.ptr(x), L.ptr(mean), L.ptr(invstd), L.ptr(w), n, c, L.ptr(gx), L.ptr(gres), L.ptr(gw), L.ptr(gb),
                L.ptr(ws), ws.numel(), L.stream()), "ts_bn_act_train_backward" + sfx)

        forms.append((f"ts_bn_act_train_forward{sfx:4s}  {n:6d} x {c:<3d}", fwd))
        forms.append((f"ts_bn_act_train_backward{sfx:4s} {n:6d} x {c:<3d}", bwd))

for _, fn in forms:
    fn()
torch.cuda.synchronize()
times = [[] for _ in forms]
for _ in range(args.reps):
    for i, (_, fn) in enumerate(forms):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times[i].append(e0.elapsed_time(e1))
lines = [f"library: {'TASEG_HIP_LIB' if os.environ.get('TASEG_HIP_LIB') else 'in-tree'}   reps {args.reps}"]
for (name, _), t in zip(forms, times):
    q = statistics.quantiles(t, n=4)
    lines.append(f"  {name}  {q[1]:.4f} ({q[0]:.4f} .. {q[2]:.4f})")
print("\n".join(lines), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
