"""Check: a digest of every output buffer of the BatchNorm entry points of csrc/bn.hip (the twelve ts_bn_* ones and the two
ts_leaky_bn_* ones) on fixed seeded inputs - fp32 and half rows, n in {1, 33, 16385}, c in {4 / 8, 20 / 24, 96, 1024}, plain / relu /
residual + relu, the backward with and without the mask.  Run it once per build of the library (TASEG_HIP_LIB=<other .so>, one
library per process) and compare the two files line by line: equal lines are equal bits.
     timeout 300 python tools/bn_digest.py [--out FILE]"""
import argparse, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from taseg_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "the kernels need the GPU"
lib = L.load()
DEV, EPS, MOM, SLOPE = "cuda", 1e-5, 0.1, 0.01
lines = []


def digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:12]


def call(name, *a):
    L.check(getattr(lib, name)(*a), name)


for half in (False, True):
    dt, sfx, per = (torch.float16, "_f16", 8) if half else (torch.float32, "", 4)
    for n in (1, 33, 16385):
        for c in (per, 24 if half else 20, 96, 1024):
            g = torch.Generator(device="cpu").manual_seed(1000 * c + n + (7 if half else 0))
            rnd = lambda *shape: torch.randn(*shape, generator=g)
            x = (rnd(n, c) * 1.5 + 0.25).to(dt).to(DEV)
            res, gy = rnd(n, c).to(dt).to(DEV), rnd(n, c).to(dt).to(DEV)
            w, b = (rnd(c) * 0.5 + 1.0).to(DEV), (rnd(c) * 0.2).to(DEV)
            ws = L.workspace(lib.ts_bn_train_workspace_bytes(c), x.device)
            for flags, relu, residual in (("plain", 0, None), ("relu", 1, None), ("residual+relu", 1, res)):
                out = []
                rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
                nbt = torch.zeros((), dtype=torch.long, device=DEV)
                mean, invstd, y = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty_like(x)
                mask = torch.zeros(n * (c // per), dtype=torch.uint8, device=DEV) if relu else None
                call("ts_bn_act_train_forward" + sfx, L.ptr(x), L.ptr(residual), L.ptr(w), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(nbt), n, c,
                     EPS, MOM, relu, L.ptr(mean), L.ptr(invstd), L.ptr(y), L.ptr(mask), L.ptr(ws), ws.numel(), L.stream())
                out.append(("train_fwd", digest(y, mask, mean, invstd, rm, rv, nbt)))
                pack = torch.empty(2 * c + 1, dtype=torch.float64, device=DEV)
                call("ts_bn_sync_stats" + sfx, L.ptr(x), n, c, L.ptr(pack), L.ptr(ws), ws.numel(), L.stream())
                out.append(("sync_stats", digest(pack)))
                y2 = torch.empty_like(x)
                mask2 = torch.zeros_like(mask) if relu else None
                call("ts_bn_act_forward" + sfx, L.ptr(x), L.ptr(residual), L.ptr(mean), L.ptr(invstd), L.ptr(w), L.ptr(b), n, c, relu,
                     L.ptr(y2), L.ptr(mask2), L.stream())
                out.append(("act_fwd", digest(y2, mask2)))
                for tag, mk in (("", None), ("+mask", mask)) if relu else (("", None),):
                    gx, gw, gb = torch.empty_like(x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
                    gres = torch.empty_like(x) if residual is not None else None
                    call("ts_bn_act_train_backward" + sfx, L.ptr(gy), L.ptr(mk), L.ptr(x), L.ptr(mean), L.ptr(invstd), L.ptr(w), n, c,
                         L.ptr(gx), L.ptr(gres), L.ptr(gw), L.ptr(gb), L.ptr(ws), ws.numel(), L.stream())
                    out.append(("train_bwd" + tag, digest(gx, gres, gw, gb)))
                    sums = torch.empty(2 * c, dtype=torch.float64, device=DEV)
                    call("ts_bn_sync_backward_reduce" + sfx, L.ptr(gy), L.ptr(mk), L.ptr(x), L.ptr(mean), L.ptr(invstd), n, c, L.ptr(sums),
                         L.ptr(gw), L.ptr(gb), L.ptr(ws), ws.numel(), L.stream())
                    out.append(("sync_bwd_reduce" + tag, digest(sums, gw, gb)))
                    a = (L.ptr(gy), L.ptr(mk), L.ptr(x), L.ptr(mean), L.ptr(invstd), L.ptr(w), L.ptr(sums), None, float(n), n, c, L.ptr(gx),
                         L.ptr(gres))
                    if half:
                        call("ts_bn_act_backward_f16", *a, L.ptr(ws), ws.numel(), L.stream())
                    else:
                        call("ts_bn_act_backward", *a, L.stream())
                    out.append(("act_bwd" + tag, digest(gx, gres)))
                rm.zero_(), rv.fill_(1.0), nbt.zero_()
                call("ts_leaky_bn_train_forward", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(nbt), n, c, EPS, MOM, SLOPE,
                     int(half), L.ptr(mean), L.ptr(invstd), L.ptr(residual), L.ptr(y), L.ptr(ws), ws.numel(), L.stream())
                out.append(("leaky_fwd", digest(y, mean, invstd, rm, rv, nbt)))
                gx, gw, gb = torch.empty_like(x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
                call("ts_leaky_bn_train_backward", L.ptr(gy), L.ptr(x), L.ptr(mean), L.ptr(invstd), L.ptr(w), n, c, SLOPE, int(half),
                     L.ptr(gx), L.ptr(gw), L.ptr(gb), L.ptr(ws), ws.numel(), L.stream())
                out.append(("leaky_bwd", digest(gx, gw, gb)))
                lines.append(f"{'half' if half else 'fp32'} n={n:<5d} c={c:<4d} {flags:13s} " + " ".join(f"{k}={v}" for k, v in out))
                print(lines[-1], flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
