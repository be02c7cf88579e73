"""Measurement: one RPVNet training step (forward, CE + Lovasz, backward, FlatSGD step) at the shape of the reference's
tools/cfgs/fusion/semantic_kitti/rpvnet_mk18_cr10.yaml - NUM_LAYER [2] * 8, cr 1.0, ResBlock, IF_DIST True - at bs 2 x 120k-point
synthetic scans voxelised at 0.05 with 64 x 2048 range images, in fp32 and under autocast, with the hand-over kernel against the chain:

  kernel   ts_range_point_tail_forward behind functional.range_point_tail                                            (the default)
  chain    functional._RANGE_TAIL_KERNEL = False: spdevoxelize, range_to_point (a second spdevoxelize over the pixel rows), the
           BatchNorm module, ReLU and two adds as separate passes

One fresh process, device events around a step that ends in a synchronise, warm-up steps of every form, then the forms ALTERNATE rep
by rep; medians, quartiles and the range go to profiles/rpvnet_step.txt.  The project's rule decides: the kernel is the default if the
gain at the medians exceeds the wider interquartile range of the pair.  Then: the hand-over call alone at its three resolutions
against the chain with the bytes it must move, computed from the shapes; `build_range_inputs` against the numpy stage (the
restatement of tests/rpvnet_ref.py) plus the upload of its results; registers and scratch of the new kernels from the compiler.
     timeout 900 python tools/time_rpvnet_step.py [--reps 20] [--out profiles/rpvnet_step.txt]"""
import argparse, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from taseg_amd import backend as B
from taseg_amd.data.range import build_range_inputs, draw_range_cut
from taseg_amd.data.synthetic import make_model_cfg, ring_column, synth_scan
from taseg_amd.optim import FlatSGD
from taseg_amd.pcseg.model.segmentor.fusion.rpvnet import RPVNet
from taseg_amd.torchsparse import SparseTensor
from taseg_amd.torchsparse.nn import functional as F
from taseg_amd.torchsparse.utils.collate import sparse_collate
from taseg_amd.torchsparse.utils.quantize import sparse_quantize

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpvnet_step.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
lines = []
HW = (64, 2048)


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_batch():
    lidar, targets = [], []
    for b in range(args.batch):
        pts, lab = synth_scan(100 + b, n_points=args.points)
        pts = np.concatenate([pts[:, :4], ring_column(pts, 64, HW[0])[:, None]], 1).astype(np.float32)
        pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
        pc -= pc.min(0, keepdims=1)
        _, inds, _ = sparse_quantize(pc, return_index=True, return_inverse=True)
        lidar.append(SparseTensor(torch.from_numpy(pts[inds]), torch.from_numpy(pc[inds])))
        targets.append(SparseTensor(torch.from_numpy(lab[inds].astype(np.int64)), torch.from_numpy(pc[inds])))
    x, t = sparse_collate(lidar), sparse_collate(targets)
    rng = np.random.RandomState(0)
    out = {"lidar": SparseTensor(x.F.float().cuda(), x.C.int().cuda()), "targets": SparseTensor(t.F.cuda(), t.C.int().cuda()),
           "offset": torch.tensor([0], device="cuda"), "cuts": [draw_range_cut(rng) for _ in range(args.batch)]}
    build_range_inputs(out["lidar"], out["cuts"], HW, batch_dict=out)
    return out


batch = make_batch()
n_rows = batch["lidar"].C.shape[0]
SWITCHES = {"kernel": True, "chain": False}


class Form:
    def __init__(self, name, amp):
        self.name, self.amp = name, amp
        torch.manual_seed(0)
        cfg = make_model_cfg("RPVNet", in_dim=4, cr=1.0, num_layer=[2] * 8, IF_DIST=True, LABEL_SMOOTHING=0.0, DROPOUT_P=0.0)
        self.model = RPVNet(cfg, 20).cuda().train()
        self.opt = FlatSGD(self.model, lr=1e-4, momentum=0.9, weight_decay=1e-4, max_norm=10.0, amp=amp)
        self.times, self.loss = [], None

    def step(self):
        was = F._RANGE_TAIL_KERNEL
        F._RANGE_TAIL_KERNEL = SWITCHES[self.name]
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.opt.zero_grad(set_to_none=True)
            bd = {"lidar": SparseTensor(batch["lidar"].F, batch["lidar"].C), "targets": batch["targets"], "offset": batch["offset"],
                  "range_image": batch["range_image"], "range_pxpy": batch["range_pxpy"]}
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.amp):
                ret, _, _ = self.model(bd)
            (ret["loss"].float().mean() * self.opt.loss_scale()).backward()
            self.opt.step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            F._RANGE_TAIL_KERNEL = was
        self.loss = float(ret["loss"].detach())
        return e0.elapsed_time(e1)


def stats(t):
    q = statistics.quantiles(t, n=4)
    return statistics.median(t), q[0], q[2], min(t), max(t)


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


say(f"RPVNet training step (mk18, cr 1.0, IF_DIST True in one process), bs {args.batch}, {args.points} points per scan: {n_rows} rows after "
    f"voxelisation at 0.05, range images {HW[0]} x {HW[1]}; {args.reps} reps of each form, alternating, device events; "
    f"{torch.cuda.get_device_name(0)}")
forms = {(k, a): Form(k, a) for a in (False, True) for k in SWITCHES}
for f in forms.values():
    for _ in range(3):
        f.step()
for _ in range(args.reps):
    for f in forms.values():
        f.times.append(f.step())
for amp in (False, True):
    res = {}
    for name in SWITCHES:
        f = forms[(name, amp)]
        res[name] = stats(f.times)
        med, q1, q3, lo, hi = res[name]
        say(f"  {'autocast' if amp else 'fp32    '} {name:6s}: median {med:8.3f} ms  quartiles {q1:8.3f} .. {q3:8.3f}  range {lo:8.3f} .. {hi:8.3f}   "
            f"(loss after the last step {f.loss:.4f})")
    gain = res["chain"][0] - res["kernel"][0]
    spread = max(res["kernel"][2] - res["kernel"][1], res["chain"][2] - res["chain"][1])
    say(f"     chain - kernel = {gain:+.3f} ms at the medians = {100 * gain / res['chain'][0]:+.1f} %; the wider interquartile range of the pair "
        f"{spread:.3f} ms: " + ("the hand-over kernel is faster than the chain by more than that spread" if gain > spread
                                else "the hand-over kernel is NOT shown to be faster than the chain"))

# ---- the hand-over alone where the three branches meet (cr 1.0): stride 1 / 32 channels / full image (z0), 16 / 256 / 1/16 (z1),
# 4 / 128 / 1/4 (z2), 1 / 96 / full image (z3)
model = forms[("kernel", False)].model
plan = model.prepare({"lidar": SparseTensor(batch["lidar"].F, batch["lidar"].C), "range_image": batch["range_image"],
                      "range_pxpy": batch["range_pxpy"]})
say("the hand-over alone (median of 20, device events, statistics given, no graph), bytes the algorithm must move from the shapes:")
for s, c, (h, w) in ((1, 32, HW), (16, 256, (4, 128)), (4, 128, (16, 512)), (1, 96, HW)):
    key = (s, s, s)
    tri_idx, tri_w, m = plan["tri_idx"][key], plan["tri_w"][key], plan["cmaps"][key].shape[0]
    rp = plan["range"][(h, w)]
    mp = args.batch * h * w
    for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
        y, vox = torch.randn(n_rows, c, device="cuda").to(dtype), torch.randn(m, c, device="cuda").to(dtype)
        rows = torch.randn(mp, c, device="cuda").to(dtype)
        fmap = rows.view(args.batch, h, w, c).permute(0, 3, 1, 2)
        st = [torch.randn(c, device="cuda") for _ in range(4)]
        st[1] = st[1].abs() + 0.5
        t_tail = timed(lambda: B.range_point_tail_forward(y, vox, tri_idx, tri_w, rows, rp["bidx"], rp["bw"], *st, want_mask=True))
        bn = torch.nn.BatchNorm1d(c).cuda().train()

        def chain():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):
                return F.spdevoxelize(vox, tri_idx, tri_w) + F.range_to_point(fmap, rp) + torch.relu(bn(y))
        t_chain = timed(chain)
        b_t = 2 * n_rows * c * e + n_rows * (128 + c // (16 // e)) + (m + mp) * c * e
        say(f"  ts_range_point_tail_forward {str(dtype)[6:]:8s} stride {s:2d}, c = {c:3d}, map {h:2d} x {w:4d}: {t_tail:7.1f} us; {b_t / 1e6:.1f} MB (y, out, "
            f"both maps, the mask, every voxel and pixel row once) = {b_t / t_tail / 1e6:.2f} TB/s   (the chain with its statistics pass: "
            f"{t_chain:.1f} us)")

# ---- the inputs: the device stage against the numpy stage plus the upload of what it made
import rpvnet_ref as R  # noqa: E402
t_dev = timed(lambda: build_range_inputs(batch["lidar"], batch["cuts"], HW))
feats, bcol = batch["lidar"].F.cpu().numpy(), batch["lidar"].C[:, -1].cpu().numpy()
host = []
for _ in range(3):
    t0 = time.perf_counter()
    got = R.range_stage32(feats, bcol, batch["cuts"], *HW)
    up = torch.from_numpy(got["image"]).cuda(), torch.from_numpy(got["pxpy"]).cuda()
    torch.cuda.synchronize()
    host.append((time.perf_counter() - t0) * 1e6)
say(f"range inputs of the batch ({n_rows} rows -> [{args.batch}, 5, {HW[0]}, {HW[1]}] + [{n_rows}, 3]): build_range_inputs on the device "
    f"{t_dev:.1f} us (6 launches); the numpy stage + upload {statistics.median(host):.0f} us (median of 3, wall clock)")

# ---- registers and scratch, from the compiler
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
say("registers and scratch of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
for src in ("rpvnet.hip", "range_stage.hip"):
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "taseg_amd", "csrc", src), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    cur = {}
    for line in r.stderr.splitlines():
        mm = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]):\s*(\S+)", line)
        if not mm:
            continue
        if mm.group(1) == "Function Name":
            cur = {"name": mm.group(2)}
        else:
            cur[mm.group(1).split(" ")[0]] = mm.group(2)
        if "Occupancy" in cur:
            demangled = subprocess.run(["c++filt", cur["name"]], capture_output=True, text=True).stdout.strip() or cur["name"]
            short = re.sub(r"\(anonymous namespace\)::|\(.*", "", demangled).replace("void ", "")
            if short.startswith("_Z"):                      # (c++filt does not know the _Float16 mangling)
                half_row = re.search(r"\d+([a-z_]+_kernel)IDF16_Lb([01])E", short)
                short = f"{half_row.group(1)}<_Float16, {'true' if half_row.group(2) == '1' else 'false'}>" if half_row else short
            say(f"  {src}: {short}: VGPRs {cur.get('VGPRs')}, AGPRs {cur.get('AGPRs')}, scratch {cur.get('ScratchSize')} bytes/lane, occupancy "
                f"{cur.get('Occupancy')} waves/SIMD")
            cur = {}
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
