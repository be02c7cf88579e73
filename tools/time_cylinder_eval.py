"""Measurement: Cylinder_TS evaluation, the host tail against the device tail (pcseg.eval.evaluate(on_device=False / True)) at the
recipe's shape - bs 2, 120k-point synthetic scans through data.cylinder.build_cylinder_batch, cylinder grid 480 x 360 x 32 over
(0..50 m, -180..180 deg, -4..2 m), INIT_SIZE 32 - in fp32 and under autocast:

  a  validation: whole evaluate() calls over `--batches` batches, wall clock around a call that starts and ends synchronised (the host
     path's work IS on the host: per scene two masks, two hashes, a query with its table and three copies of the scene's logits)
  b  one 10-vote TTA batch of build_cylinder_tta_batch: evaluate(tta_votes=10) host against device
  c  the two launches of the device tail alone (backend.eval_confusion_rows / eval_votes_rows on the tensors of a batch of (a) / (b),
     device events), beside the bytes they must move from the shapes: per point 8 B row + C logits + label + payload

One process, warm-up calls of every form, then the two forms ALTERNATE rep by rep; medians and quartiles PER BATCH go to
profiles/cylinder_eval.txt.  The project's rule decides: the device path is "the way to run these loops" where the gain at the medians
exceeds the wider interquartile range of the pair; otherwise it is not shown to be faster.
     timeout 900 python tools/time_cylinder_eval.py [--reps 20] [--commit <hash>] [--out profiles/cylinder_eval.txt]"""
import argparse, datetime, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from taseg_amd import backend as B
from taseg_amd.data import CylinderGrid, build_cylinder_batch, build_cylinder_tta_batch
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, synth_scan
from taseg_amd.pcseg import eval as E
from taseg_amd.pcseg.model import build_network
from taseg_amd.torchsparse.nn import functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--batches", type=int, default=3)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--votes", type=int, default=10)
ap.add_argument("--init-size", type=int, default=32)
ap.add_argument("--commit", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cylinder_eval.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def scan(seed):
    pts, lab = synth_scan(seed, n_points=args.points)
    return {"points": torch.from_numpy(pts).cuda(), "labels": torch.from_numpy(lab.astype(np.int64)).cuda(),
            "name": "synthetic/sequences/08/velodyne/%06d.bin" % seed}


grid = CylinderGrid([0, -180, -4], [50, 180, 2], [480, 360, 32])
val = [build_cylinder_batch([scan(100 + args.batch * i + b) for b in range(args.batch)], grid) for i in range(args.batches)]
tta = build_cylinder_tta_batch(scan(500), 0, args.votes, np.random.RandomState(1), grid)
model = fill_parameters(build_network(make_model_cfg("Cylinder_TS", in_dim=9, INIT_SIZE=args.init_size, LABEL_SMOOTHING=0.0), 20), seed=1).cuda().eval()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(t):
    q = statistics.quantiles(t, n=4)
    return statistics.median(t), q[0], q[2]


def compare(what, run, per):
    """run(on_device) is one evaluate() call over `per` batches; both forms warmed, then alternating"""
    for _ in range(2):
        for on_device in (False, True):
            run(on_device)
    times = {False: [], True: []}
    for _ in range(args.reps):
        for on_device in (False, True):
            times[on_device].append(wall(lambda: run(on_device)) / per)
    res = {k: stats(v) for k, v in times.items()}
    for on_device in (False, True):
        med, q1, q3 = res[on_device]
        say(f"  {what} {'on_device=True ' if on_device else 'on_device=False'}: median {med:8.3f} ms per batch  quartiles {q1:8.3f} .. {q3:8.3f}")
    gain = res[False][0] - res[True][0]
    spread = max(res[True][2] - res[True][1], res[False][2] - res[False][1])
    say(f"     host - device = {gain:+.3f} ms per batch at the medians = {100 * gain / res[False][0]:+.1f} %; the wider interquartile range of "
        f"the two {spread:.3f} ms")
    say("     verdict: " + ("the device tail is faster by more than that spread: it is the way to run this loop" if gain > spread
                            else "the device tail is not shown to be faster"))


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


n_pts, n_tta = int(val[0]["point_coord"].shape[0]), int(tta["point_coord"].shape[0])
say(f"Cylinder_TS evaluation, {datetime.date.today().isoformat()}, commit {commit()}, {torch.cuda.get_device_name(0)}: bs {args.batch} x {args.points} "
    f"points, grid [480, 360, 32], INIT_SIZE {args.init_size}; {args.batches} batches per evaluate() call, {args.reps} reps of each form, "
    f"alternating, wall clock between synchronisations")
same = None
for amp in (False, True):
    tag = "autocast" if amp else "fp32    "
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        host, dev = (E.evaluate(model, [dict(b) for b in val], 20, on_device=d) for d in (False, True))
        same = bool(np.array_equal(host["hist"], dev["hist"]))
        say(f"{tag}: validation, {n_pts} points and {int(val[0]['voxel_coord'].shape[0])} voxels in the first batch; the two matrices are "
            f"{'equal' if same else 'NOT EQUAL'} ({int(host['hist'].sum())} points counted)")
        compare(f"validation {tag}", lambda d: E.evaluate(model, [dict(b) for b in val], 20, on_device=d), args.batches)
        host, dev = (E.evaluate(model, [dict(tta)], 20, tta_votes=args.votes, on_device=d) for d in (False, True))
        same = bool(np.array_equal(host["predictions"][0], dev["predictions"][0]))
        say(f"{tag}: TTA, one batch of {args.votes} votes of {args.points} points ({n_tta} rows); the payloads are "
            f"{'equal' if same else 'NOT EQUAL' + (' (half votes: the host path rounds the running sum to half after every vote)' if amp else '')}")
        compare(f"TTA x{args.votes}  {tag}", lambda d: E.evaluate(model, [dict(tta)], 20, tta_votes=args.votes, on_device=d), 1)

# ---- the two launches alone, bytes from the shapes
say("the device tail's calls alone (median of 20, device events; ts_scene_counts + one launch each), bytes they must move from the shapes:")
C = 20
for name, bd, votes in (("validation", val[0], 0), ("TTA", tta, args.votes)):
    cells = bd["point_coord"].int()
    pts_batch = cells[:, -1]
    n = int(cells.shape[0])
    vox = torch.unique(cells, dim=0)
    rows = F.sphashquery(F.sphash(cells), F.sphash(vox))
    t_rows = timed(lambda: F.sphashquery(F.sphash(cells), F.sphash(vox)))
    say(f"  {name}: the batch-wide row lookup (two hashes, one query with its table) of {n} points in {int(vox.shape[0])} voxels: {t_rows:8.1f} us")
    for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
        logits = torch.randn(vox.shape[0], C, device="cuda").to(dtype)
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        if not votes:
            hist = torch.zeros((C, C), dtype=torch.int64, device="cuda")
            t = timed(lambda: B.eval_confusion_rows(logits, rows, pts_batch, bd["point_label"], bd["num_points"], hist, flags))
            t_p = timed(lambda: B.eval_confusion_rows(logits, rows, pts_batch, bd["point_label"], bd["num_points"], hist, flags, want_pred=True))
            nb, nb_p = n * (8 + C * e + 8), n * (8 + C * e + 8 + 4)
            say(f"  eval_confusion_rows {str(dtype)[6:]:8s} [{n} points, C {C}]: {t:8.1f} us; {nb / 1e6:.1f} MB (8 B row + {C * e} B logits + 8 B label per "
                f"point) = {nb / t / 1e6:.2f} TB/s;  with the int32 predictions {t_p:8.1f} us; {nb_p / 1e6:.1f} MB = {nb_p / t_p / 1e6:.2f} TB/s")
        else:
            t = timed(lambda: B.eval_votes_rows(logits, rows, pts_batch, bd["num_points"], flags))
            t_s = timed(lambda: B.eval_votes_rows(logits, rows, pts_batch, bd["num_points"], flags, want_sums=True))
            nb = n * (8 + C * e) + (n // votes) * 4
            nb_s = nb + (n // votes) * 4 * C
            say(f"  eval_votes_rows     {str(dtype)[6:]:8s} [{votes} votes x {n // votes} points, C {C}]: {t:8.1f} us; {nb / 1e6:.1f} MB (8 B row + {C * e} B "
                f"logits per vote and point, 4 B payload per point) = {nb / t / 1e6:.2f} TB/s;  with the float32 sums {t_s:8.1f} us; {nb_s / 1e6:.1f} MB = "
                f"{nb_s / t_s / 1e6:.2f} TB/s")
        assert int(flags) == 0
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
