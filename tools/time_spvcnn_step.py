"""Measurement: one SPVCNN training step (forward, CE + Lovasz, backward, FlatSGD step) at the shape of the reference's
tools/cfgs/fusion/semantic_kitti/spvcnn_mk34_cr10.yaml - NUM_LAYER [2, 3, 4, 6, 2, 2, 2, 2], cr 1.0, ResBlock - at bs 2 x 120k-point
synthetic scans voxelised at 0.05, in fp32 and under autocast, with the kernels of csrc/spvcnn.hip against the same model with one of
them switched off:

  kernels   ts_voxelize_mean_* behind functional.spvoxelize_mean, ts_point_tail_forward behind functional.point_tail   (the default)
  no mean   functional._MEAN_KERNEL = False: ts_voxelize_forward's float atomics on spcount's counts
  no tail   functional._POINT_TAIL_KERNEL = False: BatchNorm1d (ts_bn_act_train_* through nn.BatchNorm1d's own forward), ReLU,
            spdevoxelize and the add as separate passes

One fresh process, device events around a step that ends in a synchronise, warm-up steps of every form, then the forms ALTERNATE rep
by rep; medians, quartiles and the range go to profiles/spvcnn_step.txt.  The project's rule decides: a kernel is the default if the
gain at the medians exceeds the wider interquartile range of the pair; the mean kernel stays the default either way (it is what makes
the step deterministic) and its cost is reported.  Then: each kernel's own call time with the bytes it must move, computed from the
shapes; the piece length P of the mean rule at 16 / 32 / 64; `torch.nn.functional.linear` against `_PointwiseConv`'s GEMM plus a bias
add for the three point transforms.
     timeout 900 python tools/time_spvcnn_step.py [--reps 20] [--out profiles/spvcnn_step.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from taseg_amd import backend as B
from taseg_amd.data.synthetic import make_model_cfg, synth_scan
from taseg_amd.optim import FlatSGD
from taseg_amd.pcseg.model.segmentor.fusion.spvcnn import SPVCNN
from taseg_amd.torchsparse import SparseTensor
from taseg_amd.torchsparse.nn import functional as F
from taseg_amd.torchsparse.utils.collate import sparse_collate
from taseg_amd.torchsparse.utils.quantize import sparse_quantize

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spvcnn_step.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_batch():
    lidar, targets = [], []
    for b in range(args.batch):
        pts, lab = synth_scan(100 + b, n_points=args.points)
        pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
        pc -= pc.min(0, keepdims=1)
        _, inds, _ = sparse_quantize(pc, return_index=True, return_inverse=True)
        lidar.append(SparseTensor(torch.from_numpy(pts[inds]), torch.from_numpy(pc[inds])))
        targets.append(SparseTensor(torch.from_numpy(lab[inds].astype(np.int64)), torch.from_numpy(pc[inds])))
    x, t = sparse_collate(lidar), sparse_collate(targets)
    return {"lidar": SparseTensor(x.F.float().cuda(), x.C.int().cuda()), "targets": SparseTensor(t.F.cuda(), t.C.int().cuda()),
            "offset": torch.tensor([0], device="cuda")}


batch = make_batch()
n_rows = batch["lidar"].C.shape[0]
SWITCHES = {"kernels": (True, True), "no mean": (False, True), "no tail": (True, False)}


class Form:
    def __init__(self, name, amp):
        self.name, self.amp = name, amp
        torch.manual_seed(0)
        self.model = SPVCNN(make_model_cfg("SPVCNN", in_dim=4, cr=1.0), 20).cuda().train()
        self.opt = FlatSGD(self.model, lr=1e-4, momentum=0.9, weight_decay=1e-4, max_norm=10.0, amp=amp)
        self.times, self.loss = [], None

    def step(self):
        was = F._MEAN_KERNEL, F._POINT_TAIL_KERNEL
        F._MEAN_KERNEL, F._POINT_TAIL_KERNEL = SWITCHES[self.name]
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.opt.zero_grad(set_to_none=True)
            bd = {"lidar": SparseTensor(batch["lidar"].F, batch["lidar"].C), "targets": batch["targets"], "offset": batch["offset"]}
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.amp):
                ret, _, _ = self.model(bd)
            (ret["loss"].float().mean() * self.opt.loss_scale()).backward()
            self.opt.step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            F._MEAN_KERNEL, F._POINT_TAIL_KERNEL = was
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


piece = B.voxelize_mean_piece_rows()
say(f"SPVCNN training step (mk34, cr 1.0), bs {args.batch}, {args.points} points per scan: {n_rows} rows after voxelisation at 0.05; P = {piece}; "
    f"{args.reps} reps of each form, alternating, device events; {torch.cuda.get_device_name(0)}")
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
        say(f"  {'autocast' if amp else 'fp32    '} {name:8s}: median {med:8.3f} ms  quartiles {q1:8.3f} .. {q3:8.3f}  range {lo:8.3f} .. {hi:8.3f}   "
            f"(loss after the last step {f.loss:.4f})")
    for name, what in (("no mean", "the mean kernel"), ("no tail", "the tail kernel")):
        gain = res[name][0] - res["kernels"][0]
        spread = max(res["kernels"][2] - res["kernels"][1], res[name][2] - res[name][1])
        say(f"     {name} - kernels = {gain:+.3f} ms at the medians = {100 * gain / res[name][0]:+.1f} %; the wider interquartile range of the "
            f"pair {spread:.3f} ms: " + (f"{what} is faster than the form it replaces by more than that spread" if gain > spread
                                         else f"{what} is NOT shown to be faster than the form it replaces"))

# ---- the kernels alone at the three places the point branch meets the U-Net (cr 1.0: stride 1 / 32 channels in, 16 / 256, 4 / 128)
plan = forms[("kernels", False)].model.prepare({"lidar": SparseTensor(batch["lidar"].F, batch["lidar"].C)})
lib = B.L.load()
say("kernel calls alone (median of 20, device events), bytes the algorithm must move from the shapes:")
for s, c in ((1, 32), (16, 256), (4, 128)):
    key = (s, s, s)
    idx, counts, groups = plan["p2v"][key]
    m = counts.shape[0]
    t_group = timed(lambda: B.point_groups(idx, m))
    say(f"  stride {s:2d}: {n_rows} rows -> {m} voxels, most rows in a voxel {int(counts.max())}; the grouping (once per batch and stride) {t_group:.1f} us")
    for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
        feat = torch.randn(n_rows, c, device="cuda").to(dtype)
        gout = torch.randn(m, c, device="cuda").to(dtype)
        per_p = {}
        for p in (16, 32, 64):
            B.L.check(lib.ts_voxelize_mean_set_piece_rows(p), "ts_voxelize_mean_set_piece_rows")
            per_p[p] = timed(lambda: B.voxelize_mean_forward(feat, idx, groups))
        B.L.check(lib.ts_voxelize_mean_set_piece_rows(piece), "ts_voxelize_mean_set_piece_rows")
        t_b = timed(lambda: B.voxelize_mean_backward(gout, idx, groups))
        f32, cnt32 = feat.float(), counts.int()
        t_atomic = timed(lambda: B.voxelize_forward_cuda(f32, idx, cnt32))
        b_f = n_rows * c * e + m * c * e + 4 * (2 * n_rows + m)
        b_b = m * c * e + n_rows * c * e + 4 * (n_rows + m)
        say(f"    ts_voxelize_mean_forward  {str(dtype)[6:]:8s} c = {c:3d}: P = 16 / 32 / 64: {per_p[16]:7.1f} / {per_p[32]:7.1f} / {per_p[64]:7.1f} us; "
            f"{b_f / 1e6:.1f} MB = {b_f / per_p[piece] / 1e6:.2f} TB/s at P = {piece}   (ts_voxelize_forward, float atomics, fp32 rows: {t_atomic:.1f} us)")
        say(f"    ts_voxelize_mean_backward {str(dtype)[6:]:8s} c = {c:3d}: {t_b:7.1f} us; {b_b / 1e6:.1f} MB = {b_b / t_b / 1e6:.2f} TB/s")
for (s, c), c_in in zip(((16, 256), (4, 128), (1, 96)), (32, 256, 128)):
    key = (s, s, s)
    tri_idx, tri_w, m = plan["tri_idx"][key], plan["tri_w"][key], plan["cmaps"][key].shape[0]
    live = float(((tri_idx >= 0) & (tri_w != 0)).float().sum(1).mean())
    for dtype, e in ((torch.float32, 4), (torch.float16, 2)):
        y, vox = torch.randn(n_rows, c, device="cuda").to(dtype), torch.randn(m, c, device="cuda").to(dtype)
        st = [torch.randn(c, device="cuda") for _ in range(4)]
        st[1] = st[1].abs() + 0.5
        t_tail = timed(lambda: B.point_tail_forward(y, vox, tri_idx, tri_w, *st, want_mask=True))
        bn = torch.nn.BatchNorm1d(c).cuda().train()

        def chain():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):
                return F.spdevoxelize(vox, tri_idx, tri_w) + torch.relu(bn(y))
        t_chain = timed(chain)
        b_t = 2 * n_rows * c * e + n_rows * (64 + c // (16 // e)) + m * c * e
        say(f"  ts_point_tail_forward {str(dtype)[6:]:8s} stride {s:2d}, c = {c:3d} ({live:.1f} live corners per row): {t_tail:7.1f} us; {b_t / 1e6:.1f} MB (y, out, "
            f"the maps, the mask, every voxel row once) = {b_t / t_tail / 1e6:.2f} TB/s   (statistics given; the chain BatchNorm1d -> ReLU -> spdevoxelize -> add "
            f"with its statistics pass, no graph: {t_chain:.1f} us)")
    # the Linear in front: torch.nn.functional.linear against _PointwiseConv's pair GEMM + a bias add (forward + backward)
    lin = torch.nn.Linear(c_in, c).cuda()
    for amp in (False, True):
        x = torch.randn(n_rows, c_in, device="cuda", requires_grad=True)
        g = torch.randn(n_rows, c, device="cuda")
        ident = F._identity_rows(n_rows, x.device)
        wt = lin.weight.detach().t().contiguous().requires_grad_()               # [c_in, c_out], the layout of a 1x1x1 kernel

        def torch_linear():
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                out = torch.nn.functional.linear(x, lin.weight, lin.bias)
            out.backward(g.to(out.dtype))

        def pair_gemm():
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                out = F._PointwiseConv.apply(x, wt, ident)
                out = out + lin.bias.to(out.dtype)
            out.backward(g.to(out.dtype))
        t_lin = timed(torch_linear)
        t_gemm = timed(pair_gemm) if F._dense_ok(c_in, c) else float("nan")
        say(f"  Linear {c_in:3d} -> {c:3d} over {n_rows} rows, forward + backward, {'autocast' if amp else 'fp32    '}: torch.nn.functional.linear {t_lin:7.1f} us, "
            f"_PointwiseConv GEMM + bias add {t_gemm:7.1f} us")
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
