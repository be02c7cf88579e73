"""Measurement: the cylinder data stage of one Cylinder_TS batch at the recipe's shape - bs 2, 120k-point synthetic scans, cylinder grid
480 x 360 x 32 over (0..50 m, -180..180 deg, -4..2 m) - on the device (taseg_amd.data.build_cylinder_batch: ts_cylinder_cells, one
ts_cylinder_voxels chain, one host read) against the two forms a user has without it:

  device    build_cylinder_batch on the resident scans                                                          (this stage)
  host      what tools/time_cylinder_step.py does: the stage restated on numpy on the host (np.unique for the voxels, np.add.at for the
            vote - far quicker than the reference's Python loop over every point) plus the upload of its arrays
  aten      the closest device formulation in tensor ops: float32 torch.atan2, torch.unique (sorted, no first-occurrence index: the
            representative is the minimum row index per voxel through scatter_reduce), an [M, C] vote table through index_put_
            (accumulate) and argmax.  For orientation only: it is NOT equal to the reference (ATen's float32 atan2 has no stated
            rounding), and it reads the host twice (the unique's size, the per-sample counts).

One fresh process, warm-up calls of every form, then the forms ALTERNATE rep by rep; device events around whole calls, each of which
ends in its host read (the host form's time is host time: the device waits between the two events); medians, quartiles and the range go
to profiles/cylinder_stage.txt.  The project's rule decides: the stage is faster than a form if the gain at the medians exceeds the wider
interquartile range of the two; the stage ships on the kernels either way - equality with the reference is what they are for.  The two
entry points' own call times follow, with the bytes they must move computed from the shapes, against the 8 TB/s peak.
     timeout 600 python tools/time_cylinder_stage.py [--reps 20] [--out profiles/cylinder_stage.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from taseg_amd import backend as B
from taseg_amd.data import CylinderGrid, build_cylinder_batch
from taseg_amd.data.synthetic import synth_scan
from taseg_amd.torchsparse.utils.quantize import sparse_quantize

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cylinder_stage.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
GRID, HI, LO = np.array([480, 360, 32]), np.array([50.0, 180.0, 2.0]), np.array([0.0, -180.0, -4.0])
PEAK = 8e12
grid = CylinderGrid([0, -180, -4], [50, 180, 2], [480, 360, 32])
dev = "cuda"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


host_scans = [synth_scan(100 + b, n_points=args.points) for b in range(args.batch)]
host_scans = [(p, l.astype(np.int64)) for p, l in host_scans]
scans = [{"points": torch.from_numpy(p).to(dev), "labels": torch.from_numpy(l).to(dev), "name": "scan%d" % b}
         for b, (p, l) in enumerate(host_scans)]


# ---- the host form: tools/time_cylinder_step.py's cylinder_sample / make_batch
def cylinder_sample(pts, lab):
    pol = np.stack([np.hypot(pts[:, 0], pts[:, 1]), np.degrees(np.arctan2(pts[:, 1], pts[:, 0])), pts[:, 2]], 1)
    step = (HI - LO) / (GRID - 1)
    cell = np.floor((np.clip(pol, LO, HI) - LO) / step).astype(np.int32)
    _, inds, inverse = sparse_quantize(cell, return_index=True, return_inverse=True)
    votes = np.zeros((len(inds), 20), np.int32)
    np.add.at(votes, (inverse, lab), 1)
    feat = np.concatenate([(cell.astype(np.float32) + 0.5) * step + LO, pol, pts[:, :2], pts[:, 3:]], 1).astype(np.float32)
    return cell, cell[inds], votes.argmax(1), lab, feat, inverse


def host_form():
    parts = [cylinder_sample(p, l) for p, l in host_scans]
    pad = lambda a, b: np.concatenate([a, np.full((len(a), 1), b, a.dtype)], 1)  # noqa: E731
    out = {"point_coord": torch.from_numpy(np.concatenate([pad(p[0], b) for b, p in enumerate(parts)])).long().to(dev),
           "voxel_coord": torch.from_numpy(np.concatenate([pad(p[1], b) for b, p in enumerate(parts)])).long().to(dev),
           "voxel_label": torch.from_numpy(np.concatenate([p[2] for p in parts])).long().to(dev),
           "point_label": torch.from_numpy(np.concatenate([p[3] for p in parts])).long().to(dev),
           "point_feature": torch.from_numpy(np.concatenate([p[4] for p in parts])).to(dev),
           "inverse_map": torch.from_numpy(np.concatenate([p[5] for p in parts])).long().to(dev),
           "num_points": torch.tensor([len(p[0]) for p in parts]),
           "offset": torch.tensor(np.cumsum([len(p[1]) for p in parts])).int().to(dev), "name": [s["name"] for s in scans]}
    torch.cuda.synchronize()
    return out


# ---- the tensor-op form
lo_t, hi_t = torch.tensor(LO, device=dev), torch.tensor(HI, device=dev)
step_t = torch.tensor((HI - LO) / (GRID - 1), device=dev)
span = [int(g) for g in GRID]


def aten_form():
    pts = torch.cat([s["points"] for s in scans], 0)
    lab = torch.cat([s["labels"] for s in scans], 0)
    b = torch.repeat_interleave(torch.arange(len(scans), device=dev), torch.tensor([len(s["points"]) for s in scans], device=dev))
    x, y = pts[:, 0], pts[:, 1]
    pol = torch.stack([torch.sqrt(x * x + y * y), torch.atan2(y, x) / np.float32(np.pi) * 180.0, pts[:, 2]], 1)
    cell = torch.floor((torch.minimum(torch.maximum(pol.double(), lo_t), hi_t) - lo_t) / step_t).long()
    key = ((b * span[0] + cell[:, 0]) * span[1] + cell[:, 1]) * span[2] + cell[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)                                        # host read: the number of voxels
    m = uniq.shape[0]
    rows = torch.arange(len(key), device=dev)
    inds = torch.full((m,), len(key), dtype=torch.int64, device=dev).scatter_reduce(0, inverse, rows, "amin", include_self=True)
    votes = torch.zeros((m, 20), dtype=torch.int32, device=dev)
    keep = lab != 67
    votes.index_put_((inverse[keep], lab[keep]), torch.ones((), dtype=torch.int32, device=dev), accumulate=True)
    voxel_label = votes.argmax(1)
    centre = ((cell.float() + 0.5).double() * step_t + lo_t).float()
    feat = torch.cat([centre, pol, pts[:, :2], pts[:, 3:]], 1)
    coord = torch.cat([cell, b.unsqueeze(1)], 1)
    vb = coord[inds, 3]
    start = torch.searchsorted(vb, torch.arange(len(scans) + 1, device=dev))
    offset = start[1:].int()
    out = {"point_coord": coord, "voxel_coord": coord[inds], "voxel_label": voxel_label, "point_label": lab, "point_feature": feat,
           "voxel_feature": feat[inds], "inverse_map": inverse - start[b], "num_points": torch.tensor([len(s["points"]) for s in scans]),
           "offset": offset, "name": [s["name"] for s in scans]}
    offset.cpu()                                                                                  # host read: the per-sample counts
    return out


def device_form():
    return build_cylinder_batch(scans, grid)


def stats(t):
    q = statistics.quantiles(t, n=4)
    return statistics.median(t), q[0], q[2], min(t), max(t)


def one(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    return statistics.median(one(fn) * 1e3 for _ in range(reps))


forms = {"device": device_form, "host  ": host_form, "aten  ": aten_form}
ref = device_form()
n_pts, n_vox = len(ref["point_coord"]), len(ref["voxel_coord"])
say(f"cylinder data stage, bs {args.batch}, {args.points} points per scan, grid {GRID.tolist()}: {n_pts} points, {n_vox} voxels; {args.reps} reps of "
    f"each form, alternating, device events around whole calls (each ends in its host read); {torch.cuda.get_device_name(0)}")
for name, fn in (("host", host_form), ("aten", aten_form)):
    other = fn()
    moved = int((ref["point_coord"] != other["point_coord"]).any(1).sum())
    say(f"  rows whose cell differs between the device stage and the {name} form (float32 arc tangents of other roundings): {moved} of {n_pts}; "
        f"voxels {len(other['voxel_coord'])}")
for fn in forms.values():
    for _ in range(3):
        fn()
times = {k: [] for k in forms}
for _ in range(args.reps):
    for k, fn in forms.items():
        times[k].append(one(fn))
res = {k: stats(t) for k, t in times.items()}
for k, (med, q1, q3, lo, hi) in res.items():
    say(f"  {k}: median {med:8.3f} ms  quartiles {q1:8.3f} .. {q3:8.3f}  range {lo:8.3f} .. {hi:8.3f}")
for k in ("host  ", "aten  "):
    gain = res[k][0] - res["device"][0]
    spread = max(res[k][2] - res[k][1], res["device"][2] - res["device"][1])
    say(f"     {k.strip()} - device = {gain:+.3f} ms at the medians = {100 * gain / res[k][0]:+.1f} % ({res[k][0] / res['device'][0]:.1f} x); the wider "
        f"interquartile range of the two {spread:.3f} ms")
    say("     verdict: " + (f"the device stage is faster than the {k.strip()} form by more than that spread" if gain > spread
                            else f"the device stage is NOT shown to be faster than the {k.strip()} form"))

# ---- the two entry points alone, bytes from the shapes
say("entry points alone (median of 20 calls, device events, no host read), bytes the algorithm must move from the shapes, against 8 TB/s:")
pts = torch.cat([s["points"] for s in scans], 0)
lab = torch.cat([s["labels"] for s in scans], 0)
f = pts.shape[1]
sample = torch.repeat_interleave(torch.arange(len(scans), device=dev), torch.tensor([len(s["points"]) for s in scans], device=dev)).int()
flags = torch.zeros(B.CYL_FLAG_WORDS, dtype=torch.int32, device=dev)
space = grid.space()
cells = B.cylinder_cells(pts, space, sample, flags)[0]
t_c = timed(lambda: B.cylinder_cells(pts, space, sample, flags))
b_c = n_pts * (4 * f + 4) + n_pts * (16 + 32 + 4 * (5 + f))
say(f"  ts_cylinder_cells  [{n_pts}, {f}] -> cells, point_coord, point_feature [{n_pts}, {5 + f}]: {t_c:8.1f} us; {b_c / 1e6:.1f} MB "
    f"({4 * f + 4} B in, {16 + 32 + 4 * (5 + f)} B out per point) = {b_c / t_c / 1e6:.2f} TB/s = {100 * b_c / t_c / 1e-6 / PEAK:.0f} % of peak; "
    f"at peak {b_c / PEAK * 1e6:.1f} us")
t_v = timed(lambda: B.cylinder_voxels(cells, lab, len(scans)))
b_v = n_pts * (16 + 8) + n_pts * 8 + n_vox * (4 + 8)
say(f"  ts_cylinder_voxels {n_pts} cells -> {n_vox} voxels: {t_v:8.1f} us for the chain (pack, 64-bit radix sort of {n_pts} pairs, head flags, scan, "
    f"starts, scatter, vote); {b_v / 1e6:.1f} MB in and out (cells and labels read, inverse map, representatives and labels written; the "
    f"sort's own passes not counted) = {b_v / t_v / 1e6:.2f} TB/s over the whole chain; at peak {b_v / PEAK * 1e6:.1f} us")
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
