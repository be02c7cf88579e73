"""Measurement: pcseg.eval.evaluate with the tail on the host (on_device=False: every batch's logits, predictions and labels cross
to the host, numpy sums / bincounts there) against the tail on the device (on_device=True: csrc/evaltail.hip, one host read per
validation run, the label payload per TTA batch) - same tree, same process, same batches.

  a  the validation loop body at `bench.py --eval`'s shape: MinkUNet mk34 cr 1.0, bs 2, 120k-point scans, fp32 and autocast;
     one call = evaluate() over `--batches` batches, reported per batch
  b  one 10-vote TTA batch of a 120k-point scan (data.stage.build_tta_batch, history 4): MinkUNet and MinkUNetMs; one call =
     evaluate(tta_votes=10) over `--batches` such batches, reported per batch
  c  the launches of the device tail alone (backend.eval_votes / eval_confusion on the tensors of one batch of (b) / (a), enqueued
     behind a long matrix product so that the events bracket device time, not the host's issue time), with the
     bytes they move stated from the shapes: V n (C s + 8) read (s = bytes per logit; 8: the int64 inverse map entry) plus the
     outputs, and that as a fraction of the 8 TB/s HBM peak

  d  the TIAF model (MinkUNetMsMm mk34 cr 1.0) at `bench.py --workload tiaf`'s shape under autocast, as the recipe runs it:
     validation at bs 2 and one 10-vote TTA batch (data.tiaf.build_tiaf_tta_batch)
  e  the KD student (MinkUNetMsKd, the teacher runs too) at `bench.py --workload kd`'s evaluation shape: validation at bs 6,
     history 16
  f  label export from validation batches: evaluate(predictions=True, remap=LEARNING_MAP_INV) on MinkUNet at bs 2 and bs 12, host
     path against device path, and beside them what the same scans took before: tta_votes=1, one scan per batch, on the device,
     then remap_labels over the payloads on the host; times per scan

One warm-up call of every form, then the forms ALTERNATE rep by rep; device events around whole calls (a call holds host waits: it
is the time of the loop, which is what a validation epoch or a pseudo-label run takes); medians, quartiles and the full range go
to profiles/eval_device.txt.
     timeout 900 python tools/time_eval_device.py [--reps 20] [--sections abcdef] [--append] [--out profiles/eval_device.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from taseg_amd import backend as B
from taseg_amd.data import stage as S
from taseg_amd.data.synthetic import FLEXIBLE_STEPS_KITTI as STEPS
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg
from taseg_amd.pcseg import eval as E
from taseg_amd.pcseg.model import build_network
from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
from taseg_amd.torchsparse import SparseTensor

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batches", type=int, default=4)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--votes", type=int, default=10)
ap.add_argument("--history", type=int, default=4)
ap.add_argument("--sections", default="abcdef", help="which of the sections a .. f to run ((c) runs with (a) and (b))")
ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_device.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
torch.cuda.set_device(0)
lines = []
HBM_PEAK = 8e12


def say(text):
    print(text, flush=True)
    lines.append(text)


def fresh(bd):
    """the batch as a data stage hands it over: new SparseTensor objects, no index plan"""
    return {k: SparseTensor(v.F, v.C) if isinstance(v, SparseTensor) else v for k, v in bd.items() if k != "_plan"}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


_busy = torch.randn(8192, 8192, device="cuda")


def once_queued(fn):
    """device time of launches that hold no host read: they are enqueued behind a matrix product that keeps the device busy while
    the host issues them, so the events bracket the launches and not the host's issue time"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.mm(_busy, _busy)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def quart(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):8.3f} ms  quartiles {q[0]:8.3f} .. {q[2]:8.3f}  range {min(v):8.3f} .. {max(v):8.3f}"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def compare(title, host_fn, dev_fn, same, per):
    """alternating reps of the two paths; times per batch"""
    h, d = host_fn(), dev_fn()                    # warm-up, and the one comparison of what the two paths return
    assert same(h, d), f"{title}: the two paths disagree"
    t = {"host": [], "device": []}
    for _ in range(args.reps):
        t["host"].append(once(host_fn)[0] / per)
        t["device"].append(once(dev_fn)[0] / per)
    say(f"  {title}")
    say(f"      on_device=False : {quart(t['host'])}")
    say(f"      on_device=True  : {quart(t['device'])}")
    mh, md = statistics.median(t["host"]), statistics.median(t["device"])
    spread = max(iqr(t["host"]), iqr(t["device"]))
    say(f"      device - host = {md - mh:+.3f} ms per batch at the medians ({100 * (md - mh) / mh:+.1f} %); the wider interquartile range "
        f"of the two {spread:.3f} ms; verdict: the device path is " + ("faster" if mh - md > spread else "NOT faster") +
        " than the host path by more than that spread")


class _Capture(DeviceEvalTail):
    """keeps the tensors the segmentor hands to the tail"""

    def run(self, *a, **kw):
        self.args, self.kwargs = a, kw
        return super().run(*a, **kw)


def tail_alone(title, model, bd, votes, amp):
    tail = _Capture(20, "cuda", votes=votes)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        model(fresh(bd), device_tail=tail)
    out, vox_batch, invs, labels, num_points = tail.args
    mask, n_ms = tail.kwargs.get("point_mask"), tail.kwargs.get("num_points_ms")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.zeros((20, 20), dtype=torch.int64, device="cuda")
    if votes:
        fn = lambda: B.eval_votes(out, vox_batch, invs.C[:, -1], invs.F, num_points, flags, point_mask=mask, num_points_ms=n_ms)  # noqa: E731
    else:
        fn = lambda: B.eval_confusion(out, vox_batch, invs.C[:, -1], invs.F, labels.F.reshape(-1), labels.C[:, -1], num_points, hist, flags,  # noqa: E731
                                      point_mask=mask, num_points_ms=n_ms)
    fn()
    t = [once_queued(fn) for _ in range(args.reps)]
    assert int(flags) == 0
    n_scenes = int(torch.as_tensor(num_points).numel())
    rows = int(torch.as_tensor(num_points).sum())                       # V n: the logits rows the reduce launch reads
    c, s = out.shape[1], out.element_size()
    read = rows * (c * s + 8)
    written = rows // n_scenes * 4 if votes else 0
    extra = invs.F.shape[0] * (1 + 4 + 8 + 4 + 12) if mask is not None else 0      # compaction: mask, scene, inv read; table + samples written
    med = statistics.median(t) * 1e-3
    say(f"  {title}: {quart(t)}")
    say(f"      {n_scenes} scenes, {rows} rows of {c} x {s} B: reduce launch reads {read / 1e6:.1f} MB, writes {written / 1e6:.2f} MB"
        + (f"; mask compaction moves {extra / 1e6:.1f} MB more" if extra else "") +
        f"; all launches of the tail at the median: {(read + written + extra) / med / 1e9:.0f} GB/s = "
        f"{100 * (read + written + extra) / med / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")


say(f"evaluation tail on the host against on the device; {args.reps} reps of each path, alternating, device events around whole "
    f"evaluate() calls of {args.batches} batches, times per batch; sections {args.sections}; {torch.cuda.get_device_name(0)}")


def validation_batch(n_scans):
    """`bench.py --eval`'s batch of single scans, with what the evaluation tail reads"""
    coords, feats, labels, _ = bench.make_scans(0, n_scans, args.points, "minkunet")
    counts = torch.bincount(coords[:, 3].long())
    inv = torch.cat([torch.arange(int(c), device="cuda") for c in counts])
    return {"lidar": SparseTensor(feats, coords), "targets": SparseTensor(labels, coords),
            "offset": torch.tensor([len(coords)], device="cuda", dtype=torch.int32), "targets_mapped": SparseTensor(labels, coords),
            "inverse_map": SparseTensor(inv, coords), "num_points": counts, "name": [f"scan{b}" for b in range(n_scans)]}


def same_lists(h, d):
    return len(h["predictions"]) == len(d["predictions"]) and all(np.array_equal(x, y) for x, y in zip(h["predictions"], d["predictions"]))


model = None
if set("abf") & set(args.sections):
    model = fill_parameters(build_network(make_model_cfg("MinkUNet", in_dim=4, cr=1.0), 20), seed=1).cuda().eval()

# ---- (a) validation at bench.py --eval's shape
if "a" in args.sections:
    val = validation_batch(2)
    say(f"(a) validation, MinkUNet mk34 cr 1.0, bs 2, {args.points} points per scan ({val['lidar'].C.shape[0]} voxels)")
    for amp in (False, True):
        def run(on_device, amp=amp):
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                return E.evaluate(model, (fresh(val) for _ in range(args.batches)), 20, on_device=on_device)
        compare("autocast fp16" if amp else "fp32", lambda: run(False), lambda: run(True),
                lambda h, d: np.array_equal(h["hist"], d["hist"]), args.batches)
    tail_alone("(c) validation tail alone, fp32", model, val, 0, False)

# ---- (b) one 10-vote TTA batch of a scan
if "b" in args.sections:
    scan = bench.make_multiscans(0, 1, args.points, history=args.history)[0][0]
    tta = S.build_tta_batch(scan, 0, args.votes, np.random.RandomState(0), 0.05, STEPS)
    say(f"(b) TTA, {args.votes} votes of one {args.points}-point scan, history {args.history}: {tta['lidar'].C.shape[0]} voxels (current), "
        f"{tta['lidar_ms'].C.shape[0]} (fused), {tta['inverse_map_ms'].F.shape[0]} fused points")
    model_ms = fill_parameters(build_network(make_model_cfg("MinkUNetMs", in_dim=5, cr=1.0), 20), seed=1).cuda().eval()
    for name, m in (("MinkUNet", model), ("MinkUNetMs", model_ms)):
        def run(on_device, m=m):
            return E.evaluate(m, (fresh(tta) for _ in range(args.batches)), 20, tta_votes=args.votes, on_device=on_device)
        compare(f"{name} mk34 cr 1.0, fp32", lambda: run(False), lambda: run(True), same_lists, args.batches)
        tail_alone(f"(c) {name} vote tail alone, fp32", m, tta, args.votes, False)
    del model_ms, tta, scan

# ---- (d) the TIAF model at bench.py --workload tiaf's shape, under autocast
if "d" in args.sections:
    from taseg_amd.data import tiaf as TF
    from taseg_amd.data.synthetic import TIAF_CFG
    bench.miopen_find_db()
    frames, proj, _ = bench.make_tiaf_frames(0, 2, args.points)
    crop = (bench.TIAF_HEIGHT, bench.TIAF_WIDTH)
    val_mm = TF.build_tiaf_batch_from_frames(frames, STEPS, bench.TIAF_MULTISCAN, bench.TIAF_STEP_IMAGE, proj, crop, 0.05, names=["0/0", "0/1"])
    tta_mm = TF.build_tiaf_tta_batch(frames[0], 0, args.votes, np.random.RandomState(0), STEPS, bench.TIAF_MULTISCAN, bench.TIAF_STEP_IMAGE,
                                     proj, crop, 0.05, name="0/0")
    model_mm = fill_parameters(build_network(make_model_cfg("MinkUNetMsMm", in_dim=5, cr=1.0, **TIAF_CFG), 20), seed=1).cuda().eval()
    say(f"(d) TIAF, MinkUNetMsMm mk34 cr 1.0, autocast fp16, {args.points} points per scan, history {bench.TIAF_MULTISCAN}, image stack "
        f"{tuple(val_mm['image_ms'].shape)} at bs 2: {val_mm['lidar_ms'].C.shape[0]} fused voxels, {val_mm['lidar_fov_ms'].C.shape[0]} FOV voxels")
    # (the image branch's half convolutions are not bit-reproducible from call to call - tests/test_gpu_tiaf.py - and under
    # autocast the host path adds the half votes in half precision, the device path in float32: near-ties fall on either side, so
    # the warm-up comparison of the two paths counts the differing cells / labels and accepts up to 1 %)

    def run_val(on_device):
        with torch.autocast("cuda", dtype=torch.float16):
            return E.evaluate(model_mm, (fresh(val_mm) for _ in range(args.batches)), 20, on_device=on_device)

    def run_tta(on_device):
        with torch.autocast("cuda", dtype=torch.float16):
            return E.evaluate(model_mm, (fresh(tta_mm) for _ in range(args.batches)), 20, tta_votes=args.votes, on_device=on_device)

    def close_hist(h, d):
        moved = int(np.abs(h["hist"] - d["hist"]).sum())
        say(f"      (confusion matrices of the two paths: {int(h['hist'].sum())} points, {moved} matrix-cell moves apart)")
        return moved <= 1e-2 * h["hist"].sum()

    def close_labels(h, d):
        differ = sum(int((x != y).sum()) for x, y in zip(h["predictions"], d["predictions"]))
        total = sum(len(x) for x in h["predictions"])
        say(f"      (payloads of the two paths: {differ} of {total} labels differ)")
        return differ <= 1e-2 * total
    compare("validation, bs 2", lambda: run_val(False), lambda: run_val(True), close_hist, args.batches)
    say(f"    TTA, {args.votes} votes of one scan: {tta_mm['lidar_ms'].C.shape[0]} fused voxels, {tta_mm['inverse_map_ms'].F.shape[0]} fused points, "
        f"image stack {tuple(tta_mm['image_ms'].shape)}")
    compare(f"{args.votes}-vote TTA batch", lambda: run_tta(False), lambda: run_tta(True), close_labels, args.batches)
    tail_alone("(c) TIAF vote tail alone, autocast fp16", model_mm, tta_mm, args.votes, True)
    del model_mm, val_mm, tta_mm, frames
    torch.cuda.empty_cache()

# ---- (e) the KD student at bench.py --workload kd's evaluation shape
if "e" in args.sections:
    from taseg_amd.data.kd import build_kd_batch
    scans, _ = bench.make_multiscans(0, 6, args.points, history=16, pseudo_flip=0.1)
    val_kd = build_kd_batch(scans, 0.05, STEPS)
    model_kd = fill_parameters(build_network(make_model_cfg("MinkUNetMsKd", in_dim=5, cr=1.0, SAMPLING_TYPE="random", MAX_VOXEL=3000,
                                                            FEAT_KD="mse", FEAT_KD_WEIGHT=10.0), 20), seed=1).cuda().eval()
    say(f"(e) KD, MinkUNetMsKd mk34 cr 1.0 (student and teacher), bs 6, {args.points} points per scan, history 16: "
        f"{val_kd['lidar_ms'].C.shape[0]} student voxels, {val_kd['lidar_ms_gt'].C.shape[0]} teacher voxels")
    for amp in (False, True):
        def run(on_device, amp=amp):
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                return E.evaluate(model_kd, (fresh(val_kd) for _ in range(args.batches)), 20, on_device=on_device)
        compare("validation, " + ("autocast fp16" if amp else "fp32"), lambda: run(False), lambda: run(True),
                lambda h, d: np.array_equal(h["hist"], d["hist"]), args.batches)
    del model_kd, val_kd, scans
    torch.cuda.empty_cache()

# ---- (f) label export from validation batches
if "f" in args.sections:
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    lut = E.remap_lut(LEARNING_MAP_INV)
    say(f"(f) label export, MinkUNet mk34 cr 1.0, fp32, {args.points} points per scan, remap to raw ids; times per SCAN")
    for bs in (2, 12):
        val = validation_batch(bs)
        singles = []                       # the same scans, one per batch: the only way to labels before (tta_votes=1)
        at_v = 0
        for b in range(bs):
            n = int(val["num_points"][b])
            c = val["lidar"].C[at_v:at_v + n].clone()
            c[:, 3] = 0
            f, l, i = val["lidar"].F[at_v:at_v + n], val["targets"].F[at_v:at_v + n], val["inverse_map"].F[at_v:at_v + n]
            singles.append({"lidar": SparseTensor(f, c), "targets": SparseTensor(l, c), "offset": torch.tensor([n], device="cuda", dtype=torch.int32),
                            "targets_mapped": SparseTensor(l, c), "inverse_map": SparseTensor(i, c), "num_points": val["num_points"][b:b + 1],
                            "name": [val["name"][b]]})
            at_v += n
        n_batches = max(args.batches * 2 // bs, 1)
        forms = {
            "predictions=True, host  ": lambda: E.evaluate(model, (fresh(val) for _ in range(n_batches)), 20, predictions=True, remap=lut),
            "predictions=True, device": lambda: E.evaluate(model, (fresh(val) for _ in range(n_batches)), 20, predictions=True, remap=lut,
                                                           on_device=True),
            "tta_votes=1 per scan    ": lambda: {"predictions": [E.remap_labels(p, lut).reshape(-1, 1) for p in E.evaluate(
                model, (fresh(s) for _ in range(n_batches) for s in singles), 20, tta_votes=1, on_device=True)["predictions"]]},
        }
        first = {k: fn() for k, fn in forms.items()}                       # warm-up, and the comparison of what the forms return
        keys = list(forms)
        assert same_lists(first[keys[0]], first[keys[1]]) and same_lists(first[keys[0]], first[keys[2]]), "the forms disagree"
        t = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                t[k].append(once(fn)[0] / (n_batches * bs))
        say(f"  bs {bs}: {n_batches} batches = {n_batches * bs} scans per call ({val['lidar'].C.shape[0]} voxels per batch)")
        for k in forms:
            say(f"      {k}: {quart(t[k])}")
        med = {k: statistics.median(v) for k, v in t.items()}
        for other in (keys[0], keys[2]):
            spread = max(iqr(t[keys[1]]), iqr(t[other]))
            say(f"      device export - [{other.strip()}] = {med[keys[1]] - med[other]:+.3f} ms per scan ({100 * (med[keys[1]] - med[other]) / med[other]:+.1f} %); "
                f"the wider interquartile range of the two {spread:.3f} ms; verdict: the device export is "
                + ("faster" if med[other] - med[keys[1]] > spread else "NOT faster") + " by more than that spread")
        del val, singles

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
print("written:", args.out)
