"""Measurement: one Cylinder_TS training step (forward, CE + Lovasz and point loss, backward, FlatSGD step) at the recipe's shape -
bs 2, 120k-point synthetic scans, cylinder grid 480 x 360 x 32 over (0..50 m, -180..180 deg, -4..2 m), INIT_SIZE 32
(tools/cfgs/voxel/semantic_kitti/cylinder_cy480_cr10.yaml of the reference) - in fp32 and under autocast, with the kernels of
csrc/cylinder.hip and `spnn.leaky_bn`'s fused node against the same model with them switched off:

  kernels   ts_voxelize_max_*, ts_leaky_bn_train_* behind spnn.leaky_bn, ts_sigmoid3_gate_*                       (the default)
  baseline  scatter_reduce('amax'), LeakyReLU as a tensor op in front of the BatchNorm kernels + a separate residual add, the gate as
            tensor ops (functional._MAX_KERNEL / _GATE_KERNEL, batchnorm._LEAKY_KERNEL = False)

One fresh process, device events around a step that ends in a synchronise, warm-up steps of every form, then the forms ALTERNATE rep
by rep; medians, quartiles and the range go to profiles/cylinder_step.txt.  The project's rule decides: a kernel is the default if the
gain at the medians exceeds the wider interquartile range of the two forms; otherwise it is not shown to be faster.  The two kernels'
own call times follow, with the bytes they must move computed from the shapes (the grouping sort of the maximum is timed with it and
listed apart).  The cylinder data stage (polar transform, clipping, majority-vote voxel labels) is restated on numpy here: it is not
part of the step and not on the device.
     timeout 900 python tools/time_cylinder_step.py [--reps 20] [--out profiles/cylinder_step.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from taseg_amd import backend as B
from taseg_amd.data.synthetic import make_model_cfg, synth_scan
from taseg_amd.optim import FlatSGD
from taseg_amd.pcseg.model import build_network
from taseg_amd.torchsparse.nn import batchnorm as BN
from taseg_amd.torchsparse.nn import functional as F
from taseg_amd.torchsparse.utils.quantize import sparse_quantize

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--init-size", type=int, default=32)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cylinder_step.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
GRID, HI, LO = np.array([480, 360, 32]), np.array([50.0, 180.0, 2.0]), np.array([0.0, -180.0, -4.0])
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def cylinder_sample(seed):
    pts, lab = synth_scan(seed, n_points=args.points)
    pol = np.stack([np.hypot(pts[:, 0], pts[:, 1]), np.degrees(np.arctan2(pts[:, 1], pts[:, 0])), pts[:, 2]], 1)
    step = (HI - LO) / (GRID - 1)
    cell = np.floor((np.clip(pol, LO, HI) - LO) / step).astype(np.int32)
    _, inds, inverse = sparse_quantize(cell, return_index=True, return_inverse=True)
    votes = np.zeros((len(inds), 20), np.int32)
    np.add.at(votes, (inverse, lab.astype(np.int64)), 1)
    feat = np.concatenate([(cell.astype(np.float32) + 0.5) * step + LO, pol, pts[:, :2], pts[:, 3:]], 1).astype(np.float32)
    return cell, cell[inds], votes.argmax(1), lab.astype(np.int64), feat, inverse


def make_batch():
    parts = [cylinder_sample(100 + b) for b in range(args.batch)]
    pad = lambda a, b: np.concatenate([a, np.full((len(a), 1), b, a.dtype)], 1)  # noqa: E731
    dev = "cuda"
    return {"point_coord": torch.from_numpy(np.concatenate([pad(p[0], b) for b, p in enumerate(parts)])).long().to(dev),
            "voxel_coord": torch.from_numpy(np.concatenate([pad(p[1], b) for b, p in enumerate(parts)])).long().to(dev),
            "voxel_label": torch.from_numpy(np.concatenate([p[2] for p in parts])).long().to(dev),
            "point_label": torch.from_numpy(np.concatenate([p[3] for p in parts])).long().to(dev),
            "point_feature": torch.from_numpy(np.concatenate([p[4] for p in parts])).to(dev),
            "inverse_map": torch.from_numpy(np.concatenate([p[5] for p in parts])).long().to(dev),
            "num_points": torch.tensor([len(p[0]) for p in parts]),
            "offset": torch.tensor(np.cumsum([len(p[1]) for p in parts])).int().to(dev), "name": ["scan%d" % b for b in range(args.batch)]}


batch = make_batch()
n_pts, n_vox = len(batch["point_coord"]), len(batch["voxel_coord"])


class Form:
    def __init__(self, kernels, amp):
        self.kernels, self.amp = kernels, amp
        torch.manual_seed(0)
        cfg = make_model_cfg("Cylinder_TS", in_dim=9, INIT_SIZE=args.init_size, LABEL_SMOOTHING=0.0)
        self.model = build_network(cfg, 20).cuda().train()
        self.opt = FlatSGD(self.model, lr=1e-4, momentum=0.9, weight_decay=1e-4, max_norm=10.0, amp=amp)
        self.times, self.loss = [], None

    def step(self):
        was = F._MAX_KERNEL, F._GATE_KERNEL, BN._LEAKY_KERNEL
        F._MAX_KERNEL = F._GATE_KERNEL = BN._LEAKY_KERNEL = self.kernels
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.amp):
                ret, _, _ = self.model(dict(batch))
            (ret["loss"].float().mean() * self.opt.loss_scale()).backward()
            self.opt.step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            F._MAX_KERNEL, F._GATE_KERNEL, BN._LEAKY_KERNEL = was
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


say(f"Cylinder_TS training step, bs {args.batch}, {args.points} points per scan, grid {GRID.tolist()}, INIT_SIZE {args.init_size}: {n_pts} points, "
    f"{n_vox} voxels; {args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
forms = {(k, a): Form(k, a) for a in (False, True) for k in (True, False)}
for f in forms.values():
    for _ in range(3):
        f.step()
for _ in range(args.reps):
    for f in forms.values():
        f.times.append(f.step())
for amp in (False, True):
    res = {}
    for kernels in (True, False):
        f = forms[(kernels, amp)]
        res[kernels] = stats(f.times)
        med, q1, q3, lo, hi = res[kernels]
        say(f"  {'autocast' if amp else 'fp32    '} {'kernels ' if kernels else 'baseline'}: median {med:8.3f} ms  quartiles {q1:8.3f} .. {q3:8.3f}  "
            f"range {lo:8.3f} .. {hi:8.3f}   (loss after the last step {f.loss:.4f})")
    gain = res[False][0] - res[True][0]
    spread = max(res[True][2] - res[True][1], res[False][2] - res[False][1])
    say(f"     baseline - kernels = {gain:+.3f} ms at the medians = {100 * gain / res[False][0]:+.1f} %; the wider interquartile range of the two "
        f"{spread:.3f} ms")
    say("     verdict: " + ("the kernels are faster than the forms they replace by more than that spread: they are the default" if gain > spread
                            else "the kernels are NOT shown to be faster than the forms they replace"))

# ---- the two kernels alone, bytes from the shapes
say("kernel calls alone (median of 20, device events), bytes the algorithm must move from the shapes:")
c = 256
idx = B.unique_i64(F.sphash(batch["point_coord"].int()))[1]
for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
    feat = torch.randn(n_pts, c, device="cuda").to(dtype)
    out, arg = B.voxelize_max_forward(feat, idx, n_vox)
    gout = torch.randn(n_vox, c, device="cuda").to(dtype)
    t_f = timed(lambda: B.voxelize_max_forward(feat, idx, n_vox))
    t_b = timed(lambda: B.voxelize_max_backward(gout, idx, arg, n_pts))
    t_ref = timed(lambda: feat.new_zeros((n_vox, c)).scatter_reduce(0, idx.long().unsqueeze(1).expand(-1, c), feat, "amax", include_self=False))
    b_f = n_pts * c * e + n_vox * c * (e + 4) + 4 * (n_pts + n_vox + 1)
    b_b = n_vox * c * (e + 4) + n_pts * c * e + 4 * n_pts           # every arg / grad_out row once (its points share it), grad_feat written
    say(f"  ts_voxelize_max_forward  {str(dtype)[6:]:8s} [{n_pts}, {c}] -> [{n_vox}, {c}]: {t_f:8.1f} us incl. the grouping sort of {n_pts} keys; "
        f"{b_f / 1e6:.1f} MB for the maximum itself = {b_f / t_f / 1e6:.2f} TB/s over the whole call   (scatter_reduce amax: {t_ref:.1f} us)")
    say(f"  ts_voxelize_max_backward {str(dtype)[6:]:8s}: {t_b:8.1f} us; {b_b / 1e6:.1f} MB (arg and grad_out once per voxel, grad_feat written once) = "
        f"{b_b / t_b / 1e6:.2f} TB/s")
cg = 2 * args.init_size
for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
    x, u, v, w, g = (torch.randn(n_vox, cg, device="cuda").to(dtype) for _ in range(5))
    t_f = timed(lambda: B.sigmoid3_gate_forward(x, u, v, w))
    t_b = timed(lambda: B.sigmoid3_gate_backward(g, x, u, v, w))
    t_ref = timed(lambda: (torch.sigmoid(u) + torch.sigmoid(v) + torch.sigmoid(w)) * x)
    say(f"  ts_sigmoid3_gate_forward  {str(dtype)[6:]:8s} [{n_vox}, {cg}]: {t_f:8.1f} us; {5 * n_vox * cg * e / 1e6:.1f} MB = "
        f"{5 * n_vox * cg * e / t_f / 1e6:.2f} TB/s   (tensor ops, forward: {t_ref:.1f} us)")
    say(f"  ts_sigmoid3_gate_backward {str(dtype)[6:]:8s}: {t_b:8.1f} us; {9 * n_vox * cg * e / 1e6:.1f} MB = {9 * n_vox * cg * e / t_b / 1e6:.2f} TB/s")
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
