"""Measurement: the TIAF recipe's data stage with its camera side on csrc/tiaf_stage.hip (`build_tiaf_batch_from_frames`,
taseg_amd/data/tiaf.py) against the construction of `bench.py --workload tiaf`, and the two kernels alone against the ATen sequences
they replace - at the TIAF line's stage shape (`bench.make_tiaf_frames`: bs 2, 120k-point synthetic scans, 16 history scans, 5 camera
frames of 376 x 1241 per sample against the 384 x 1280 crop, voxel 0.05 m).  One fresh process, device events around whole calls,
one warm-up pass of every form, then the forms ALTERNATE rep by rep so that all see the same machine; medians, quartiles and the full
range are written to profiles/tiaf_stage.txt:

  a  bench.py's construction: build_tiaf_sample per sample + build_tiaf_batch
  b  build_tiaf_batch_from_frames, aug=None, flips=None
  c  (b) with an AugParams per sample and a flip for every frame, for the record
  d  the kernels alone: ts_tiaf_image_stack on the ten frames against crop_image + _pad per frame, stack, cat, permute +
     contiguous; ts_tiaf_fov_cloud (cat of the rows, frame table, three launches, the read of the counts) against project_fov,
     boolean index, fuse_scan, cat per frame and the per-sample clamp.  The image kernel's bytes - 3 h w + 4 h w read and 16 H W
     written per frame, from the shapes - over its time, as a share of the 8 TB/s HBM peak of the data sheet.

(a) and (b) build the same batch - checked once.  A stage call holds host reads, so its device-event time includes the host's share
between the launches - it is the time of the call, which is what a training step waits for when the stage is not overlapped.
     timeout 900 python tools/time_tiaf_stage.py [--reps 20] [--out profiles/tiaf_stage.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd import backend as B
from taseg_amd.data import augment as A
from taseg_amd.data import tiaf as TF
from taseg_amd.data.stage import rows_index32
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI as STEPS

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tiaf_stage.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
HBM_PEAK = 8.0e12                          # bytes / s, the data sheet's

frames_list, proj, npts = bench.make_tiaf_frames(0, args.batch, args.points)
MS, STEP, CROP, VOXEL = bench.TIAF_MULTISCAN, bench.TIAF_STEP_IMAGE, (bench.TIAF_HEIGHT, bench.TIAF_WIDTH), 0.05
dev = proj.device
rng = np.random.RandomState(0)
aug = [A.draw_train_params(rng) for _ in frames_list]
flips = [{d: True for d in TF._camera_deltas(f)} for f in frames_list]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def form_a():
    return TF.build_tiaf_batch([TF.build_tiaf_sample(f, STEPS, MS, STEP, proj, CROP, VOXEL, name=str(b)) for b, f in enumerate(frames_list)])


def form_b():
    return TF.build_tiaf_batch_from_frames(frames_list, STEPS, MS, STEP, proj, CROP, VOXEL, names=[str(b) for b in range(len(frames_list))])


def form_c():
    return TF.build_tiaf_batch_from_frames(frames_list, STEPS, MS, STEP, proj, CROP, VOXEL, aug=aug, flips=flips)


cams = [(b, d, f[d]) for b, f in enumerate(frames_list) for d in TF._camera_deltas(f)]
table = TF._unit_table(dev)
# the clamp's minima, as the stage has them when the camera side starts
los = [f[0]["points"][:, :3].t().contiguous().min(1).values for f in frames_list]


def image_kernel():
    return B.tiaf_image_stack([f["image"] for _, _, f in cams], [f["semantic"] for _, _, f in cams], None, table, CROP)


def image_aten():
    img, sem = [[] for _ in frames_list], [[] for _ in frames_list]
    for b, _, f in cams:
        img[b].append(TF.crop_image(f["image"], CROP))
        sem[b].append(TF._pad(f["semantic"].float(), CROP))
    img, sem = [torch.stack(x, 0) for x in img], [torch.stack(x, 0) for x in sem]         # build_tiaf_sample's stacks
    return torch.cat(img, 0).permute(0, 3, 1, 2).contiguous(), torch.cat(sem, 0).permute(0, 3, 1, 2).contiguous()


def fov_kernel():
    entries, first, lengths = [], 0, []
    for b, d, f in cams:
        n = int(f["points"].shape[0])
        entries.append((proj, frames_list[b][0]["pose"], f["pose"], {
            "row_offset": float(CROP[0] * (abs(d) // STEP)), "fov_dist": -1.0, "sample": b, "img_w": int(f["image"].shape[1]),
            "img_h": int(f["image"].shape[0]), "flags": TF.FUSE * (d != 0), "first": first, "src": first}))
        first += n
        lengths.append(n)
    out, _, _, counts = B.tiaf_fov_cloud(torch.cat([f["points"][:, :4] for _, _, f in cams], 0), rows_index32(lengths, dev),
                                         TF._frame_records(entries, dev), len(frames_list), CROP, lo=torch.stack(los, 0))
    counts = counts.tolist()
    return [c for c in torch.split(out[:sum(counts)], counts)]


def fov_aten():
    clouds = [[] for _ in frames_list]
    for b, d, f in cams:
        pts = TF.fov_points(f["points"], proj, (f["image"].shape[1], f["image"].shape[0]), CROP, abs(d) // STEP)
        if d != 0:
            pts = torch.cat([B.fuse_scan(pts[:, :4].contiguous(), frames_list[b][0]["pose"], f["pose"]), pts[:, 4:]], 1)
        clouds[b].append(pts)
    out = []
    for b, cl in enumerate(clouds):
        fov = torch.cat(cl, 0)
        out.append(fov[(fov[:, :3] >= los[b]).all(1)].contiguous())
    return out


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


forms = (("a", form_a), ("b", form_b), ("c", form_c), ("ik", image_kernel), ("ia", image_aten), ("fk", fov_kernel), ("fa", fov_aten))
# the warm-up: code objects, caches of the layouts, allocator - and the one comparison of what the forms build
warm = {k: fn() for k, fn in forms}
a, b = warm["a"], warm["b"]
assert all(same(a[k], b[k]) for k in ("lidar", "lidar_ms", "lidar_fov_ms")), "the forms build different clouds"
assert all(torch.equal(a[k], b[k]) for k in ("image_ms", "semantic_map_ms", "offset_img", "point_mask")), "the forms build different images"
assert all(torch.equal(x, y) for x, y in zip(warm["ik"], warm["ia"])) and all(torch.equal(x, y) for x, y in zip(warm["fk"], warm["fa"]))
n_rows = sum(int(f["points"].shape[0]) for _, _, f in cams)
img_bytes = sum(7 * int(f["image"].shape[0]) * int(f["image"].shape[1]) + 16 * CROP[0] * CROP[1] for _, _, f in cams)
say(f"TIAF data stage, bs {len(frames_list)}, {args.points} points per scan, history {MS}, {len(cams)} camera frames of "
    f"{tuple(cams[0][2]['image'].shape[:2])} against {CROP}, {npts} raw points, {n_rows} camera rows; {args.reps} reps of each form, "
    f"alternating, device events; {torch.cuda.get_device_name(0)}")
say(f"  voxels: {b['lidar'].C.shape[0]} / {b['lidar_ms'].C.shape[0]} / {b['lidar_fov_ms'].C.shape[0]} (FOV); (a) and (b): the same batch, "
    f"the kernels and their ATen sequences: the same tensors (checked)")
del warm, a
t = {k: [] for k, _ in forms}
for _ in range(args.reps):
    for k, fn in forms:
        t[k].append(once(fn)[0])
med = {k: statistics.median(v) for k, v in t.items()}
say(f"  a  build_tiaf_sample per sample + build_tiaf_batch (bench.py) : {quart(t['a'])}")
say(f"  b  build_tiaf_batch_from_frames                               : {quart(t['b'])}")
say(f"  c  (b) + augmentation and a flip for every frame              : {quart(t['c'])}")
spread = max(iqr(t["a"]), iqr(t["b"]))
say(f"     b - a = {med['b'] - med['a']:+.3f} ms at the medians = {100 * (med['b'] - med['a']) / med['a']:+.1f} %; the wider interquartile "
    f"range of the two {spread:.3f} ms")
say("     verdict: " + ("the batched builder is faster than bench.py's construction by more than that spread"
                        if med["a"] - med["b"] > spread else
                        "the batched builder is NOT faster than bench.py's construction by more than that spread"))
say(f"     c - b = {med['c'] - med['b']:+.3f} ms at the medians: what the augmentation and the flips cost")
say(f"  d  images, {len(cams)} frames: ts_tiaf_image_stack                  : {quart(t['ik'])}")
say(f"     images, the ATen sequence                                  : {quart(t['ia'])}")
say(f"     the kernel moves {img_bytes / 1e6:.1f} MB: {img_bytes / (med['ik'] * 1e-3) / 1e12:.2f} TB/s over the call's time = "
    f"{100 * img_bytes / (med['ik'] * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak (the call includes the wrapper's host time)")
say(f"     FOV cloud, {n_rows} rows: ts_tiaf_fov_cloud                  : {quart(t['fk'])}")
say(f"     FOV cloud, project / index / fuse / cat per frame + clamp  : {quart(t['fa'])}")
say("     bench.py's TIAF line keeps building per sample (form a): its number does not move with this file")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
