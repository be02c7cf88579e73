"""Float64 reference of the flat SGD step kernels (csrc/optim.hip), stage by stage - test infrastructure, not product code.

Written from the formulas of torch.optim.SGD (momentum, weight decay, dampening 0, Nesterov), torch.nn.utils.clip_grad_norm_
(coefficient min(1, max_norm / (norm + 1e-6))) and torch.amp.GradScaler.update(), and from the comments of csrc/optim.hip for what
torch leaves open (max_norm <= 0: coefficient 1; amp = 0: the loss scale counts as 1 and the schedule stands still).  The float
hyper-parameters (lr, momentum, weight_decay, gs, max_norm, growth, backoff) enter as the float32 values the kernels receive, cast
up; `f32` gives that value.  tests/test_optim64_host.py checks this file against torch's own code in float64;
tests/test_gpu_optim_float64.py checks the kernels against this file.
"""
import math

import numpy as np
import torch

EPS = 1e-6          # clip_grad_norm_'s


def f32(v):
    """the float32 value a kernel receives for the Python float v, as a Python float"""
    return float(np.float32(v))


def _np64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(np.float64).reshape(-1)


def _t64(t):
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.asarray(t))
    return t.detach().cpu().double().reshape(-1)


def grad_stats64(g):
    """(sumsq, nonfinite) of one gradient bucket.  The square of a float is exact in double, so math.fsum of the squares is the
    correctly rounded sum.  A non-finite element gives nonfinite = 1; sumsq is then inf or NaN as IEEE makes it."""
    x = _np64(g)
    if not np.isfinite(x).all():
        with np.errstate(all="ignore"):
            return float(np.sum(x * x)), 1
    return math.fsum(x * x), 0


def decide64(sumsq, nonfinite, state, max_norm, growth, backoff, interval, amp):
    """The new state[0..4] after ts_sgd_decide: [loss scale, growth tracker, clip coefficient / scale, skip flag, norm of the unscaled
    gradients].  state[2] and state[4] in double; state[0] and state[1] as numpy float32, each ONE rounding of a product or a sum
    (scale x growth, scale x backoff, tracker + 1), which is what GradScaler's float32 tensors hold.

    GradScaler.update(): found_inf -> scale x backoff, tracker 0; else tracker + 1, and at growth_interval tracker 0 and scale x growth,
    unless that product is not finite: then the scale stays.
    A step is bad when a gradient was non-finite or the sum of squares is (an overflow of the sum)."""
    scale32 = np.float32(state[0]) if amp else np.float32(1.0)
    scale = float(scale32)
    bad = int(nonfinite) != 0 or not math.isfinite(sumsq)
    norm = math.nan if math.isnan(sumsq) else math.sqrt(sumsq) / scale
    if max_norm > 0:
        ratio = max_norm / (norm + EPS)
        coef = 1.0 if math.isnan(ratio) else min(1.0, ratio)
    else:
        coef = 1.0
    new_scale, tracker = np.float32(state[0]), np.float32(state[1])
    if amp:
        with np.errstate(over="ignore"):
            if bad:
                new_scale, tracker = scale32 * np.float32(backoff), np.float32(0.0)
            else:
                tracker = tracker + np.float32(1.0)
                if int(tracker) >= int(interval):
                    grown, tracker = scale32 * np.float32(growth), np.float32(0.0)
                    if np.isfinite(grown):                   # "Do not grow the scale past fp32 bounds to inf" (ATen, AmpKernels.cu)
                        new_scale = grown
    return [np.float32(new_scale), np.float32(tracker), coef / scale, 1.0 if bad else 0.0, norm]


def apply64(p, g, m, gs, lr, momentum, wd, nesterov=0, first=0):
    """One SGD step on flat tensors, elementwise in double: (p', m', (|a|, |b|, |c|)) with a = g gs, b = wd p, c = momentum m.
        d = a + b;  m' = d when first (no buffer yet: m is not read), else c + d;  p' = p - lr (d + momentum m') with Nesterov,
        p - lr m' without.
    The magnitudes are what the rounding bars of the device tests are made of; c = 0 when first."""
    p, g, m = _t64(p), _t64(g), _t64(m)
    a, b = g * gs, wd * p
    d = a + b
    if first:
        c = torch.zeros_like(d)
        buf = d.clone()
    else:
        c = momentum * m
        buf = c + d
    step = d + momentum * buf if nesterov else buf
    return p - lr * step, buf, (a.abs(), b.abs(), c.abs())


def slot_skipped(unused, flags, flag_index):
    """the rule of ts_sgd_apply_segments: no gradient here this step, and (several ranks) none on any other rank either"""
    return unused != 0 and (flags is None or float(flags[flag_index]) == 0.0)


def apply_segments64(p, g, m, offsets, sizes, gs, group_of, group_values, unused=(), flags=None, first=0):
    """apply64 per parameter slot with that slot's group.  offsets[i], sizes[i]: the slot's place in the bucket; group_of[i] its
    index into group_values = [(lr, momentum, wd, nesterov), ...] (float32 values cast up); unused: the slots without a gradient;
    flags: None or one float per slot (flag_index = slot).  Skipped slots and the padding between slots are returned unchanged.
    Returns (p', m', mags): mags = per-element |a|, |b|, |c|, lr, momentum, nesterov (0 / 1) and `active` (0 where nothing was
    applied), all float64 [n]."""
    p, g, m = _t64(p), _t64(g), _t64(m)
    p2, m2 = p.clone(), m.clone()
    mags = {k: torch.zeros_like(p) for k in ("a", "b", "c", "lr", "momentum", "nesterov", "active")}
    unused = set(int(i) for i in unused)
    for i, (o, s) in enumerate(zip(offsets, sizes)):
        if slot_skipped(1 if i in unused else 0, flags, i):
            continue
        lr, mom, wd, nest = group_values[int(group_of[i])]
        sl = slice(int(o), int(o) + int(s))
        p2[sl], m2[sl], (a, b, c) = apply64(p[sl], g[sl], m[sl], gs, lr, mom, wd, nest, first)
        mags["a"][sl], mags["b"][sl], mags["c"][sl] = a, b, c
        mags["lr"][sl], mags["momentum"][sl], mags["nesterov"][sl], mags["active"][sl] = lr, mom, float(bool(nest)), 1.0
    return p2, m2, mags
