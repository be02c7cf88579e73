"""Measurement: the nuScenes TIAF recipe's data stage with its camera side on csrc/nusc_tiaf_stage.hip
(`build_nusc_tiaf_batch_from_keyframes`, taseg_amd/data/nuscenes_tiaf.py) against the per-sample path, and the kernels alone against
the ATen sequences they replace - at the recipe's shape (nuscenes/minkunet_mk34_cr10_fsa_tiaf.yaml: bs 2, MULTISCAN_IMAGE 0,
MULTISCAN_INTERVAL 1, USED_VIEW of six cameras, PAINT_DIST -1; synthetic 34 720-point keyframes of `synth_nusc_sequence`, 900 x 1600
images, so 448 x 800 planes; voxel 0.1 m).  One fresh process, device events around whole calls, one warm-up pass of every form, then
the forms ALTERNATE rep by rep so that all see the same machine; medians, quartiles and the full range are written to
profiles/nusc_tiaf_stage.txt:

  a   build_nusc_tiaf_sample per sample + build_nusc_tiaf_batch      (zero_maps off: the 345 MB of zero fills would drown the rest)
  b   build_nusc_tiaf_batch_from_keyframes                           (zero_maps off)
  a+, b+   the same with an AugParams per sample
  d   the pieces alone: the FOV chain (one ts_fuse_sweeps, the record table, ts_nusc_fov_cloud, the read of the counts) against
      frame_cloud + ts_project_cam / index / cat / ts_fuse_sweeps / cat per view and the per-sample clamp; ts_tiaf_image_stack on the
      twelve frames against half_image per frame, stack, cat, permute + contiguous; ts_nusc_fov_cloud alone (its wrapper's call on
      prepared inputs) with the bytes it moves - per virtual row 21 read in each of its two passes, per survivor 8 read and 44
      written, from the shapes - over its time, as a share of the 8 TB/s HBM peak of the data sheet.

(a) and (b) build the same batch - checked once.  A stage call holds host reads, so its device-event time includes the host's share
between the launches - it is the time of the call, which is what a training step waits for when the stage is not overlapped.
     timeout 900 python tools/time_nusc_tiaf_stage.py [--reps 20] [--out profiles/nusc_tiaf_stage.txt]"""
import argparse, os, random, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd import backend as B
from taseg_amd.data import augment as A
from taseg_amd.data import nuscenes_tiaf as T
from taseg_amd.data.stage import rows_index32
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_NUSC as STEPS, KITTI_TO_NUSC, synth_nusc_sequence, synth_scan
from taseg_amd.data.tiaf import _unit_table

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=34720)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nusc_tiaf_stage.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
HBM_PEAK = 8.0e12                          # bytes / s, the data sheet's
W_FULL, H_FULL, CROP_TOP, VOXEL, INTERVAL = 1600, 900, 2, 0.1, 1
VIEWS, VIEW_YAW = [0, 1, 2, 3, 4, 5], [0.0, -55.0, -110.0, 180.0, 110.0, 55.0]       # degrees, ego frame (x forward, y left)
dev = torch.device("cuda")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def quat(m):
    """unit quaternion (w, x, y, z) of a rotation matrix"""
    t = np.trace(m)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s])
    i = int(np.argmax(np.diag(m)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k]) * 2
    q = np.zeros(4)
    q[0], q[1 + i], q[1 + j], q[1 + k] = (m[k, j] - m[j, k]) / s, 0.25 * s, (m[j, i] + m[i, j]) / s, (m[k, i] + m[i, k]) / s
    return q


def camera_rotation(yaw_deg):
    """camera -> ego rotation of a camera looking along the ego-frame direction `yaw` (camera: z forward, x right, y down)"""
    a = np.deg2rad(yaw_deg)
    return np.stack([[np.sin(a), -np.cos(a), 0.0], [0.0, 0.0, -1.0], [np.cos(a), np.sin(a), 0.0]], axis=1)


# the recipe's inputs: the FSA side as bench.py builds it, the keyframe and its interval predecessor, six cameras per keyframe
fsa_samples, _, _ = bench.make_nusc_samples(0, args.batch, args.points)
seq, world = synth_nusc_sequence()
index = len(seq.global_indexes) - 1
remap = np.asarray(KITTI_TO_NUSC, dtype=np.int64)
rs = np.random.RandomState(0)
view_cs = {v: (quat(camera_rotation(VIEW_YAW[v])), np.array([1.5 - 0.2 * v, 0.1 * (v - 2), 1.5]),
               np.array([[1260.0 + v, 0.0, W_FULL / 2 - 1.3 * v], [0.0, 1260.0 + v, H_FULL / 2 + 0.7 * v], [0.0, 0.0, 1.0]])) for v in VIEWS}
inputs = []
for b, fsa in enumerate(fsa_samples):
    seed = 100 * b
    key_points, key_labels = {index: fsa["points"]}, {index: fsa["labels"]}
    for i in range(index - INTERVAL, index):
        g = int(seq.global_indexes[i])
        p, l = synth_scan(seed + g, n_points=args.points, n_beams=32, n_az=1090, pose=world[g].astype(np.float32), scene_seed=seed)
        key_points[i] = torch.from_numpy(np.concatenate([p, np.zeros((len(p), 1), np.float32)], 1)).to(dev)
        key_labels[i] = torch.from_numpy(remap[l]).to(dev)
    cam_frames = {}
    for v in VIEWS:              # the camera fires a few ms away from the lidar sweep: its own ego pose
        q = seq.e2g_q[index] + np.array([0.0, 0.0, 0.0, 2e-4 * (v + 1)])
        cam_frames[(index, v)] = dict(pose_q=q / np.linalg.norm(q), pose_t=seq.e2g_t[index] + np.array([0.011 * (v + 1), -0.004 * v, 0.0]),
                                      image=torch.from_numpy(rs.randint(0, 256, size=(H_FULL // 2, W_FULL // 2, 3)).astype(np.uint8)).to(dev),
                                      semantic=torch.from_numpy(rs.randint(0, 17, size=(H_FULL // 2, W_FULL // 2, 1)).astype(np.float32)).to(dev))
    inputs.append(dict(fsa=fsa, seq=seq, index=index, key_points=key_points, key_labels=key_labels, lidar_cs=(seq.l2e_q[index], seq.l2e_t[index]),
                       view_cs=view_cs, cam_frames=cam_frames, steps=STEPS, multiscan_image=0, step_image=1.0, interval=INTERVAL,
                       used_view=VIEWS, paint_dist=-1.0, full_image_size=(W_FULL, H_FULL), voxel_size=VOXEL, rng=random.Random(0),
                       crop_top=CROP_TOP, name=str(b)))
nb = len(inputs)
aug = [A.draw_train_params(np.random.RandomState(0)) for _ in inputs]
HEIGHT = H_FULL // 2 - CROP_TOP


def form_a(aug=None):
    return T.build_nusc_tiaf_batch([T.build_nusc_tiaf_sample(**inp, zero_maps=False, aug=None if aug is None else aug[b])
                                    for b, inp in enumerate(inputs)])


def form_b(aug=None):
    return T.build_nusc_tiaf_batch_from_keyframes(inputs, aug=aug)


los = [T._current_keyframe(inp["fsa"]["points"], 4)[:, :3].t().contiguous().min(1).values for inp in inputs]
frames_of = [[0]] * nb


def fov_prepared():
    points5, labels, sweep, params, table, virt, _ = T._camera_records(inputs, frames_of, list(range(nb)), dev)
    moved, no_ego = B.fuse_sweeps(points5.contiguous(), sweep, params)
    records = torch.from_numpy(table.view(np.uint8).reshape(len(table), T.CAM_FRAME_DTYPE.itemsize)).to(dev, non_blocking=True)
    return moved[:, :4].contiguous(), labels, rows_index32(virt, dev), records, no_ego


def fov_kernel():
    pts, labels, frame, records, no_ego = fov_prepared()
    out, lab, _, _, counts = B.nusc_fov_cloud(pts, labels, frame, records, nb, pre_keep=no_ego, lo=torch.stack(los, 0))
    counts = counts.tolist()
    return [c for c in torch.split(out[:sum(counts)], counts)]


prepared = fov_prepared()
lo_all = torch.stack(los, 0)


def fov_kernel_alone():
    pts, labels, frame, records, no_ego = prepared
    return B.nusc_fov_cloud(pts, labels, frame, records, nb, pre_keep=no_ego, lo=lo_all)


def fov_aten():
    out = []
    for b, inp in enumerate(inputs):
        cloud, lab = T.frame_cloud(seq, index, 0, None, INTERVAL, inp["key_points"], inp["key_labels"], -1.0)
        fov = []
        for view_idx, v in enumerate(VIEWS):
            rec = inp["cam_frames"][(index, v)]
            chain = T.camera_chain(inp["lidar_cs"][0], inp["lidar_cs"][1], seq.e2g_q[index], seq.e2g_t[index], rec["pose_q"], rec["pose_t"],
                                   view_cs[v][0], view_cs[v][1], view_cs[v][2])
            pts, _ = T.fov_points(cloud, lab, torch.from_numpy(chain).to(dev), (W_FULL, H_FULL), CROP_TOP, HEIGHT, view_idx)
            rot, trans = T.relative_transform(seq, index, index)
            params = np.zeros((1, 28), dtype=np.float64)
            params[0, 13:22], params[0, 22:25], params[0, 25] = rot.reshape(-1), trans, 1.0
            five = torch.cat([pts[:, :4], torch.zeros((pts.shape[0], 1), dtype=torch.float32, device=dev)], 1).contiguous()
            moved, _ = B.fuse_sweeps(five, torch.zeros(pts.shape[0], dtype=torch.int32, device=dev), torch.from_numpy(params).to(dev))
            fov.append(torch.cat([moved[:, :4], pts[:, 4:]], 1))
        fov = torch.cat(fov, 0)
        out.append(fov[(fov[:, :3] >= los[b]).all(1)].contiguous())
    return out


pictures = [inp["cam_frames"][(index, v)] for inp in inputs for v in VIEWS]
table = _unit_table(dev)


def image_kernel():
    return B.tiaf_image_stack([f["image"][CROP_TOP:] for f in pictures], [f["semantic"][CROP_TOP:] for f in pictures], None, table,
                              (HEIGHT, W_FULL // 2))


def image_aten():
    img = [torch.stack([T.half_image(inp["cam_frames"][(index, v)]["image"], CROP_TOP) for v in VIEWS], 0) for inp in inputs]
    sem = [torch.stack([inp["cam_frames"][(index, v)]["semantic"].float()[CROP_TOP:].contiguous() for v in VIEWS], 0) for inp in inputs]
    return torch.cat(img, 0).permute(0, 3, 1, 2).contiguous(), torch.cat(sem, 0).permute(0, 3, 1, 2).contiguous()


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
    return x.C.shape == y.C.shape and torch.equal(x.C, y.C) and x.F.dtype == y.F.dtype and \
        torch.equal(x.F.view(torch.int32) if x.F.dtype == torch.float32 else x.F, y.F.view(torch.int32) if y.F.dtype == torch.float32 else y.F)


forms = (("a", form_a), ("b", form_b), ("a+", lambda: form_a(aug)), ("b+", lambda: form_b(aug)), ("fk", fov_kernel), ("fa", fov_aten),
         ("f1", fov_kernel_alone), ("ik", image_kernel), ("ia", image_aten))
# the warm-up: code objects, caches of the layouts, allocator - and the one comparison of what the forms build
warm = {k: fn() for k, fn in forms}
for x, y in (("a", "b"), ("a+", "b+")):
    assert all(same(warm[x][k], warm[y][k]) for k in ("lidar", "lidar_ms", "lidar_fov_ms", "targets_fov_ms")), "the forms build different clouds"
    assert all(torch.equal(warm[x][k], warm[y][k]) for k in ("image_ms", "semantic_map_ms", "offset_img", "point_mask")), "the forms build different images"
assert all(torch.equal(x, y) for x, y in zip(warm["ik"], warm["ia"])) and all(torch.equal(x, y) for x, y in zip(warm["fk"], warm["fa"]))
n_rows, survivors = int(prepared[2].shape[0]), int(warm["f1"][4].sum())
b = warm["b"]
say(f"nuScenes TIAF data stage, bs {nb}, {args.points} points per keyframe, MULTISCAN_IMAGE 0, MULTISCAN_INTERVAL {INTERVAL}, {len(VIEWS)} views of "
    f"{H_FULL} x {W_FULL} ({HEIGHT} x {W_FULL // 2} planes), {int(prepared[0].shape[0])} camera-side point rows, {n_rows} virtual rows, "
    f"{survivors} survivors; {args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
say(f"  voxels: {b['lidar'].C.shape[0]} / {b['lidar_ms'].C.shape[0]} / {b['lidar_fov_ms'].C.shape[0]} (FOV); (a) and (b), (a+) and (b+): the same "
    f"batch, the kernels and their ATen sequences: the same tensors (checked)")
del warm, b
t = {k: [] for k, _ in forms}
for _ in range(args.reps):
    for k, fn in forms:
        t[k].append(once(fn)[0])
med = {k: statistics.median(v) for k, v in t.items()}
say(f"  a   build_nusc_tiaf_sample per sample + build_nusc_tiaf_batch : {quart(t['a'])}")
say(f"  b   build_nusc_tiaf_batch_from_keyframes                      : {quart(t['b'])}")
for x, y, what in (("a", "b", "without augmentation"), ("a+", "b+", "with an AugParams per sample")):
    if x == "a+":
        say(f"  a+  (a) with an AugParams per sample                          : {quart(t['a+'])}")
        say(f"  b+  (b) with an AugParams per sample                          : {quart(t['b+'])}")
    spread = max(iqr(t[x]), iqr(t[y]))
    say(f"      {y} - {x} = {med[y] - med[x]:+.3f} ms at the medians = {100 * (med[y] - med[x]) / med[x]:+.1f} %; the wider interquartile "
        f"range of the two {spread:.3f} ms")
    say(f"      verdict, {what}: " + ("the batched builder is faster than the per-sample path by more than that spread"
                                     if med[x] - med[y] > spread else
                                     "the batched builder is NOT faster than the per-sample path by more than that spread"))
say(f"  d   FOV cloud, {n_rows} virtual rows: fuse + records + ts_nusc_fov_cloud + counts : {quart(t['fk'])}")
say(f"      FOV cloud, frame_cloud + project / index / cat / fuse / cat per view + clamp   : {quart(t['fa'])}")
fov_bytes = 2 * 21 * n_rows + 52 * survivors
say(f"      ts_nusc_fov_cloud alone (the wrapper's call, three launches)                   : {quart(t['f1'])}")
say(f"      it moves {fov_bytes / 1e6:.1f} MB: {fov_bytes / (med['f1'] * 1e-3) / 1e12:.3f} TB/s over the call's time = "
    f"{100 * fov_bytes / (med['f1'] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak (the call includes the wrapper's host time and five "
    f"allocations; the kernels' own device time was not measured)")
img_bytes = len(pictures) * (7 * HEIGHT * (W_FULL // 2) + 16 * HEIGHT * (W_FULL // 2))
say(f"      images, {len(pictures)} frames: ts_tiaf_image_stack                                    : {quart(t['ik'])}")
say(f"      images, the ATen sequence                                                      : {quart(t['ia'])}")
say(f"      the image kernel moves {img_bytes / 1e6:.1f} MB: {img_bytes / (med['ik'] * 1e-3) / 1e12:.2f} TB/s over the call's time = "
    f"{100 * img_bytes / (med['ik'] * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak (the call includes the wrapper's host time)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
