"""Measurement: what `mix=` costs the batched nuScenes data stage, and ts_stage_clamp_compact against the ATen sequence it replaces,
at the stage shape of `bench.py --workload nuscenes_ms` (bs 4, 32-beam 34.7k-point synthetic sweeps, the sweeps the distance rule
selects over 15 m, voxel 0.1 m).  One fresh process, device events, one warm-up pass of every form, then the forms ALTERNATE rep by
rep so that both see the same machine; medians, quartiles and the full range are written to profiles/nuscenes_mix_stage.txt:

  1  the stage with mix=None
  2  the stage with a PolarMix record (swap and paste on) for every sample, partner = the next sample of the batch
  3  the clamp + compaction alone on the rows the mixed stage hands it: backend.stage_clamp_compact (three launches, one host read
     of the counts) against the ATen sequence it replaced in both mixed stages, restated in aten() below (compare, all, nonzero, four
     gathers, searchsorted; two host reads; the per-sample clamp of stage.voxelize_sample_ms is its one-sample form), results
     compared once

--dataset semantickitti: forms 1 and 2 alone on the SemanticKITTI stage at the shape of `bench.py --workload minkunet_ms` (bs 2,
120k-point synthetic scans, history 4, voxel 0.05 m), through public functions only - the same file measures any commit that has
`mix=`.  --parent FILE: the file this command wrote on the parent commit, same machine, same session; its mixed-stage line and the
verdict (this tree's median may exceed the parent's by no more than the wider interquartile range of the two) are appended.

A stage call holds host reads, so its device-event time includes the host's share between the launches - it is the time of the
call, which is what a training step waits for when the stage is not overlapped.
     timeout 600 python tools/time_nuscenes_mix.py [--reps 40] [--out profiles/nuscenes_mix_stage.txt]
     timeout 600 python tools/time_nuscenes_mix.py --dataset semantickitti [--parent FILE] [--out profiles/kitti_mix_stage.txt]"""
import argparse, os, re, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd import backend as B
from taseg_amd.data import mix as M
from taseg_amd.data import nuscenes as N
from taseg_amd.data import stage as S
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI, FLEXIBLE_STEPS_NUSC

ap = argparse.ArgumentParser()
ap.add_argument("--dataset", default="nuscenes", choices=["nuscenes", "semantickitti"])
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--batch", type=int, default=None, help="default: the bench line's, 4 (nuscenes) / 2 (semantickitti)")
ap.add_argument("--points", type=int, default=None, help="default: the bench line's, 34700 / 120000")
ap.add_argument("--parent", default=None, help="semantickitti: the file this command wrote on the parent commit")
ap.add_argument("--out", default=None, help="default: profiles/nuscenes_mix_stage.txt / profiles/kitti_mix_stage.txt")
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
kitti = args.dataset == "semantickitti"
args.batch = args.batch or (2 if kitti else 4)
args.points = args.points or (120000 if kitti else 34700)
args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "kitti_mix_stage.txt" if kitti else "nuscenes_mix_stage.txt")

if kitti:
    samples, npts = bench.make_multiscans(0, args.batch, args.points, history=4)
    kind = {}
else:
    samples, npts, n_sweeps = bench.make_nusc_samples(0, args.batch, args.points)
    kind = dict(tail_all=False, instance_classes=M.INSTANCE_CLASSES["nuscenes"], dataset="nuscenes")
partners = [samples[(b + 1) % len(samples)] for b in range(len(samples))]
rng = np.random.RandomState(0)
omega = M.draw_omega(rng)
mix = [M.MixParams(kind=M.POLAR, alpha=float(a), beta=float(a + np.pi), swap=True, paste=True, omega=omega, **kind)
       for a in (rng.random_sample(len(samples)) - 1) * np.pi]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def plain():
    if kitti:
        return S.build_multiscan_batch(samples, 0.05, FLEXIBLE_STEPS_KITTI)
    return N.build_nuscenes_batch(samples, 0.1, FLEXIBLE_STEPS_NUSC)


def mixed():
    if kitti:
        return S.build_multiscan_batch(samples, 0.05, FLEXIBLE_STEPS_KITTI, mix=mix, partners=partners)
    return N.build_nuscenes_batch(samples, 0.1, FLEXIBLE_STEPS_NUSC, mix=mix, partners=partners)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(a, b, reps):
    a(), b()                                   # the warm-up: code objects, caches of the layouts, allocator
    ta, tb = [], []
    for _ in range(reps):
        ta.append(once(a)[0])
        tb.append(once(b)[0])
    return ta, tb


def quart(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):7.3f} ms  quartiles {q[0]:7.3f} .. {q[2]:7.3f}  range {min(v):7.3f} .. {max(v):7.3f}"


def finish():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", args.out)


if kitti:
    say(f"SemanticKITTI data stage, bs {len(samples)}, {args.points} points per scan, history 4, {npts} raw points; "
        f"{args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
else:
    say(f"nuScenes data stage, bs {len(samples)}, {args.points} points per sweep, {n_sweeps} sweeps per sample, {npts} raw points; "
        f"{args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
t_plain, t_mix = alternate(plain, mixed, args.reps)
say(f"  1  stage, mix=None                      : {quart(t_plain)}")
say(f"  2  stage, PolarMix (swap + paste) x {len(samples)}     : {quart(t_mix)}")
d = statistics.median(t_mix) - statistics.median(t_plain)
say(f"     difference of the medians {d:+.3f} ms = {100 * d / statistics.median(t_plain):+.1f} % "
    f"(twice the {'scans' if kitti else 'sweeps'} are fused: every partner's too)")
if kitti:
    if args.parent:
        def figures(ln):
            return map(float, re.search(r"median\s+([\d.]+) ms\s+quartiles\s+([\d.]+) \.\.\s+([\d.]+)", ln).groups())
        was_plain, was = [[ln for ln in open(args.parent).read().splitlines() if ln.startswith(tag)][0] for tag in ("  1  ", "  2  ")]
        m0, q0, q1 = figures(was)
        q = statistics.quantiles(t_mix, n=4)
        spread, dm = max(q[2] - q[0], q1 - q0), statistics.median(t_mix) - m0
        say("  the parent commit, same machine and session, its own file:")
        say(was_plain)
        say(was)
        say(f"     mix=None, the same code in both, this tree - parent = {statistics.median(t_plain) - next(figures(was_plain)):+.3f} ms at the "
            f"medians: what two processes differ by on their own")
        say(f"     mixed stage, this tree - parent = {dm:+.3f} ms at the medians; the wider interquartile range of the two runs {spread:.3f} ms")
        say("     verdict: " + ("not slower than the parent by more than that spread" if dm <= spread
                                else "SLOWER than the parent by more than that spread"))
    finish()
    sys.exit(0)

# the rows the mixed stage hands the clamp: one stage call with the wrapper recording its arguments
seen = {}
real = B.stage_clamp_compact


def record(*a):
    seen["args"] = a
    return real(*a)


B.stage_clamp_compact = record
try:
    mixed()
finally:
    B.stage_clamp_compact = real
ms, ms_lab, ms_b32, lo = seen["args"]
nb, dev = lo.shape[0], ms.device


def kernel():
    out, lab, b, b32, counts = B.stage_clamp_compact(ms, ms_lab, ms_b32, lo)
    n_ms = counts.tolist()                                              # the host read
    kept = sum(n_ms)
    return out[:kept], lab[:kept], b[:kept], b32[:kept], n_ms


def aten():
    ms_b = ms_b32.long()
    idx = (ms[:, :3] >= lo[ms_b]).all(1).nonzero().squeeze(1)           # host read 1 (the compaction's size)
    out, lab, b, b32 = ms[idx].contiguous(), ms_lab[idx], ms_b[idx], ms_b32[idx]
    start = torch.searchsorted(b, torch.arange(nb + 1, device=dev))
    n_ms = (start[1:] - start[:-1]).tolist()                            # host read 2 (fused rows per sample)
    return out, lab, b, b32, n_ms


got, want = kernel(), aten()
assert got[4] == want[4] and all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                             y.view(torch.int32) if y.dtype == torch.float32 else y)
                                 for x, y in zip(got[:4], want[:4])), "the kernel and the ATen sequence disagree"
t_k, t_a = alternate(kernel, aten, 3 * args.reps)
say(f"  3  clamp + compaction alone, {ms.shape[0]} fused rows of {ms.shape[1]} floats, {sum(got[4])} survive; "
    f"{3 * args.reps} reps each, alternating; same rows, labels, sample columns and counts (checked)")
say(f"     stage_clamp_compact (3 launches, 1 read) : {quart(t_k)}")
say(f"     ATen sequence (aten() here, 2 reads)     : {quart(t_a)}")
qk, qa = statistics.quantiles(t_k, n=4), statistics.quantiles(t_a, n=4)
spread = max(qk[2] - qk[0], qa[2] - qa[0])
dk = statistics.median(t_k) - statistics.median(t_a)
say(f"     kernel - ATen = {dk:+.3f} ms at the medians; spread of the repetitions (the wider interquartile range) {spread:.3f} ms")
say("     verdict: " + ("the kernel is not slower than the ATen sequence by more than the spread: it stays"
                        if dk <= spread else "the kernel is SLOWER than the ATen sequence by more than the spread"))
finish()
