"""Timings behind profiles/adamw_step.txt (run on the GPU; fails without one):

    python tools/time_adamw_step.py [--reps 20] [--out profiles/adamw_step.txt]

The optimizer step of the range-view recipes (OPTIMIZER adamw, GRAD_NORM_CLIP 10, AMP) at the parameter sets of FIDNet and SalsaNext:
real modules with every gradient filled (scaled by the loss scale), no forward pass.  Three candidates over three twins of the model,
each a whole step that leaves the gradients in place for the next one:

  flat      FlatAdamW(amp=True, max_norm=10).step(): grad_stats + decide + prepare + apply, no host read
  foreach   GradScaler.unscale_ + clip_grad_norm_ + scaler.step(torch.optim.AdamW) + scaler.update(), torch's default form
  fused     the same over torch.optim.AdamW(fused=True)

One warm-up of each, then `--reps` repetitions in ALTERNATION so that all see the same machine; a repetition is the host time of
ITERS steps that ends in a device synchronisation, divided by ITERS.  Medians and quartiles are reported, and the project's rule is
applied: one is faster only where the gap exceeds the wider interquartile range of the pair.  torch's unscale_ divides the gradients
in place, so its twins get their gradients back before every step (a multi-tensor copy inside the window, stated in the output and
timed alone); the flat step does not change its gradients.

The apply kernel alone (ts_adamw_apply_segments over the buckets, device events around the launches) with the bytes from the shapes -
28 per element: p, g, m, v read; p, m, v written - and the share of the HBM peak (8 TB/s) they imply.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from taseg_amd import _lib as L  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg  # noqa: E402
from taseg_amd.optim import FlatAdamW  # noqa: E402

HBM_PEAK = 8.0e12
HYPER = dict(lr=0.0025, betas=(0.9, 0.999), eps=5e-6, weight_decay=0.01)        # the recipes' values
SCALE = 1024.0
ITERS = 5
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def build(name):
    if name == "FIDNet":
        from taseg_amd.pcseg.model.segmentor.range.fidnet.model.semantic.fidnet import FIDNet as cls
        kw = dict(IF_BN=True, IF_INTENSITY=True, IF_RANGE=True, WITH_NORM=False, LOSS="dice", IF_LS_LOSS=True, IF_BD_LOSS=True,
                  TOP_K_PERCENT_PIXELS=1.0)
    else:
        from taseg_amd.pcseg.model.segmentor.range.salsanext.model.semantic.salsanext import SalsaNext as cls
        kw = dict(LOSS="dice", IF_LS_LOSS=True, IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=1.0)
    return fill_parameters(cls(make_model_cfg(name, **kw), 20), seed=1).cuda().train()


def gradients(model, seed=5):
    """one scaled gradient per parameter, total norm of the unscaled set above 10 so that the clip is live"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty_like(p).copy_(torch.randn(p.shape, generator=gen, device="cuda") * (0.05 * SCALE))      # p's own layout
            for p in model.parameters()]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def quartiles(v):
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return med, q1, q3


def verdict(name_a, a, name_b, b):
    (ma, qa1, qa3), (mb, qb1, qb3) = quartiles(a), quartiles(b)
    gap, spread = abs(ma - mb), max(qa3 - qa1, qb3 - qb1)
    if gap > spread:
        fast, slow = (name_a, name_b) if ma < mb else (name_b, name_a)
        return f"{fast} is faster than {slow} ({max(ma, mb) / min(ma, mb):.2f} x): gap {gap:.4f} ms > wider IQR {spread:.4f} ms"
    return f"no difference shown between {name_a} and {name_b}: gap {gap:.4f} ms <= wider IQR {spread:.4f} ms"


def one_model(name, reps):
    twins = {k: build(name) for k in ("flat", "foreach", "fused")}
    grads = gradients(twins["flat"])
    n_param = sum(p.numel() for p in twins["flat"].parameters())
    flat = FlatAdamW(twins["flat"], amp=True, max_norm=10.0, init_scale=SCALE, **HYPER)
    for p, g in zip(twins["flat"].parameters(), grads):
        p.grad = g.clone()
    flat.reducer.finish()                       # the gradients now sit in the buckets (p.grad are their views) and stay there
    buckets = flat.reducer.buckets
    n_total = sum(b["flat"].numel() for b in buckets)

    def flat_step():
        flat.step()

    torch_steps, restores = {}, {}
    for key in ("foreach", "fused"):
        model = twins[key]
        params = list(model.parameters())
        opt = torch.optim.AdamW(params, fused=(key == "fused"), **HYPER)
        scaler = torch.amp.GradScaler("cuda", init_scale=SCALE)
        scaler.scale(torch.zeros(1, device="cuda"))           # (the scale tensor is made by the first scale() call)
        for p, g in zip(params, grads):
            p.grad = g.clone()
        held = [p.grad for p in params]

        def restore(held=held):
            torch._foreach_copy_(held, grads)

        def step(opt=opt, scaler=scaler, params=params, restore=restore):
            restore()                           # unscale_ divided the gradients in place
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, 10.0)
            scaler.step(opt)
            scaler.update()

        torch_steps[key], restores[key] = step, restore
    cands = {"flat": flat_step, "foreach": torch_steps["foreach"], "fused": torch_steps["fused"], "restore": restores["foreach"]}
    for fn in cands.values():
        window(fn, 2)
    times = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            times[k].append(window(fn, ITERS))
    say(f"{name}: {n_param} parameters in {sum(len(b['params']) for b in buckets)} tensors, {len(buckets)} bucket(s) of {n_total} "
        f"elements with the padding; {reps} repetitions of {ITERS} steps each, alternating; host time to the end of the device work")
    label = {"flat": "flat     FlatAdamW.step() (amp, max_norm 10)", "foreach": "foreach  unscale_ + clip + scaler.step(AdamW) + update",
             "fused": "fused    the same, AdamW(fused=True)", "restore": "         (the gradient restore inside both torch windows)"}
    for k in cands:
        med, q1, q3 = quartiles(times[k])
        say(f"    {label[k]:<58s} median {med:8.4f} ms   quartiles {q1:8.4f} .. {q3:8.4f}")
    say("    -> " + verdict("flat", times["flat"], "foreach", times["foreach"]))
    say("    -> " + verdict("flat", times["flat"], "fused", times["fused"]))
    restore_med = quartiles(times["restore"])[0]
    for k in ("foreach", "fused"):
        less = [t - restore_med for t in times[k]]
        say(f"    -> with the restore's median taken off {k}: " + verdict("flat", times["flat"], k, less))
    # the apply kernel alone
    lib = L.load()

    def apply_only():
        for b in buckets:
            L.check(lib.ts_adamw_apply_segments(L.ptr(b["pflat"]), L.ptr(b["flat"]), L.ptr(b["mflat"]), L.ptr(b["vflat"]),
                                                b["flat"].numel(), L.ptr(flat.state), L.ptr(b["slots"]), len(b["params"]),
                                                L.ptr(b["tile_first"]), b["tile_first"].numel(), None, L.ptr(b["coef"]), L.stream()),
                    "ts_adamw_apply_segments")

    flat.state[3] = 0.0
    apply_only()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        apply_only()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    med, q1, q3 = quartiles(ev)
    moved = 28 * n_total
    rate = moved / (med * 1e-3)
    say(f"    ts_adamw_apply_segments alone ({len(buckets)} launch(es), device events): median {med:.4f} ms   quartiles {q1:.4f} .. {q3:.4f};"
        f" {moved / 1e6:.1f} MB from the shapes (28 B per element) -> {rate / 1e9:.0f} GB/s = {100 * rate / HBM_PEAK:.1f} % of the "
        f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    if rate < 0.25 * HBM_PEAK:
        say(f"    at this size the kernel is launch-bound, not bandwidth-bound: {moved / 1e6:.1f} MB would take "
            f"{moved / HBM_PEAK * 1e6:.1f} us at the peak, the launch(es) took {med * 1e3:.1f} us")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "adamw_step.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_adamw_step.py measures on the GPU: no device found")
    say(f"AdamW optimizer step, flat against torch's own; {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say("No multi-GPU AdamW step was run or timed.")
    say()
    for name in ("FIDNet", "SalsaNext"):
        one_model(name, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", args.out)


if __name__ == "__main__":
    main()
