"""The four kernels of csrc/optim.hip against float64 (oracle/optim64.py), stage by stage through the C ABI (-m gpu).

Every element is compared.  Every check of a case is evaluated; the case fails with the list of those that missed, and prints one
line of error / bar per stage (profiles/optim_float64.txt keeps a run's lines).  Every bar is computed from the inputs and the
float64 reference, never from a kernel's output.  u = 2^-24 (the relative error of one float rounding), TINY = 2^-149 (what one
float product may lose to underflow); first-order bounds carry the factor SLACK = 1.01 for their second-order terms.  A contracted
multiply-add only removes a rounding, so the counts hold with and without contraction.

ts_sgd_grad_stats.  The launch rule, restated here from ts_sgd_grad_stats: W = min(ceil(n / 16384), 512) workgroups of 256 threads,
thread t starts at float4 t and strides T = 256 W float4; four float4 per trip while the fourth lies inside, then one per trip, and
thread 0 of workgroup 0 adds the n % 4 last elements.  The squares are exact in double.  One thread makes
k = 4 ceil((n / 4) / T) + n % 4 additions (three inside a float4 and one onto the accumulator), the workgroup's tree 8 (allowance 16),
and the W atomic additions form a chain: every term passes at most k + 16 + W additions of non-negative numbers.  The cell holds
s0 before the call, and each atomic addition rounds a value of at most s0 + sumsq:
    |cell - (s0 + sumsq64)| <= (k + 16 + W) 2^-53 sumsq64 + W 2^-53 s0
(the second term is what the preset adds to the bar sumsq is given alone; the difference is evaluated exactly, with math.fsum).
The flag is exactly the reference's, OR-ed into what the cell held.  In the one-element family the gradient is zero but for one
element 3.0 (cell exactly s0 + 9) or inf / -inf / NaN (flag 1) at the places where the three loops and the workgroups meet, computed
from the launch rule: a dropped or doubled element fails by a whole number.

ts_sgd_decide.  scale = state[0] with amp, 1 without; r = 0 when scale is a power of two (1 / scale exact), else 1.
  state[4] = fl(fl32(sqrt(sumsq)) x fl(1 / scale)): one cast, one product, r for the reciprocal (the double square root's 2^-53 is
  inside SLACK):                                   |state[4] - norm64| <= SLACK (2 + r) u norm64 + TINY
  state[2] = fl(min(1, fl(max_norm / fl(norm + 1e-6f))) x fl(1 / scale)): the norm's (2 + r) u, the addition u, the constant 1e-6f
  against 1e-6 u / 2, the division u, min is 1-Lipschitz, the product u and its reciprocal r u:
                                                   |state[2] - ref| <= SLACK (5.5 + 2 r) u ref + TINY
  and exactly 1 / scale where the coefficient is 1 by rule (max_norm <= 0, a zero norm) and on the near side of the clip boundary.
  state[0], state[1], state[3] exact (decide64 rounds each product once, as the kernel does); state[5..7] keep their bits; sumsq and
  nonfinite read 0 afterwards.

ts_sgd_apply, a = g gs, b = wd p, c = momentum m (float values cast up), A = |a| + |b| + |c|:
  d = fl(fl(a) + fl(b)):                           E_d = 2 u (|a| + |b|)
  m' = fl(fl(c) + d) (first step: m' = d):         E_m = E_d + u |c| + u A <= 3 u (|a| + |b|) + 2 u |c|     (first: E_m = E_d)
  p' = fl(p - fl(lr m')):                          E_p = lr E_m + u lr A + u (|p| + lr A)
      |m' - m'64| <= SLACK E_m + 3 TINY            (three products may underflow)
      |p' - p'64| <= SLACK E_p + 4 TINY            (those three times lr < 1, and lr m')
ts_sgd_apply_segments with Nesterov, step = fl(d + fl(momentum m')), S = |a| + |b| + momentum A:
  E_s = E_d + momentum E_m + u momentum A + u S = E_d + momentum E_m + u (2 momentum A + |a| + |b|)
      |p' - p'64| <= SLACK (lr E_s + u (2 lr S + |p|)) + 5 TINY
Skipped slots and a skipped step keep every bit; the padding between slots is zero before and after.

The chain runs the three stages as FlatSGD.step() issues them, five steps with a loss scale; the reference receives the device's own
values from before each stage, cast up unchanged, and each stage is held to its single-step bar above.
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import optim64 as O64
from test_gpu_flat_optim import LAYOUTS, Bucket, apply_segments, make_state, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
D = 2.0 ** -53
TINY = 2.0 ** -149
SLACK = 1.01
INVALID = -1                                   # include/taseg_hip.h TS_ERR_INVALID_ARGUMENT
GS_PER_WG, GS_CAP, GS_THREADS = 16384, 512, 256          # ts_sgd_grad_stats' launch rule
AP_CAP = 8192 * 256                            # ts_sgd_apply: elements of one grid-stride pass at the grid cap
SEG_CAP = 2048 * 4096                          # ts_sgd_apply_segments: the same, 2048 tiles of TS_SGD_TILE
S0 = 0.75                                      # what the sumsq cell holds before a call
f32 = O64.f32


def _L():
    from taseg_amd import _lib as L
    return L, L.load()


class Checks:
    def __init__(self, cid):
        self.cid, self.missed, self.n, self.ratios = cid, [], 0, {}

    def le(self, stage, what, value, bound):
        self.n += 1
        ratio = value / bound if bound > 0 else (0.0 if value <= bound else math.inf)
        self.ratios[stage] = max(self.ratios.get(stage, 0.0), ratio)
        if not value <= bound:
            self.missed.append(f"{stage} {what}: {value:.3e} > {bound:.3e}")

    def true(self, what, ok):
        self.n += 1
        if not ok:
            self.missed.append(what)

    def done(self):
        print(f"optim_float64 {self.cid:<58} error / bar:  " + "  ".join(f"{k} {v:.3f}" for k, v in self.ratios.items())
              + f"  ({self.n} checks)")
        assert not self.missed, f"{self.cid}: {len(self.missed)} of {self.n} checks missed\n  " + "\n  ".join(self.missed[:40])


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------- ts_sgd_grad_stats

def gs_launch(n):
    """(workgroups, float4 stride of a thread, additions of one thread) by ts_sgd_grad_stats' launch rule"""
    w = min(-(-n // GS_PER_WG), GS_CAP)
    t = w * GS_THREADS
    return w, t, 4 * -(-(n // 4) // t) + n % 4


def gs_places(n):
    """element indexes where the loops and the workgroups of sgd_grad_stats_kernel meet, from the launch rule"""
    w, t, _ = gs_launch(n)
    q = n // 4                                                     # whole float4: the vector loops cover float4 0 .. q - 1
    f = np.arange(q, dtype=np.int64)
    thread, trip = f % t, f // t                                   # float4 f is the trip-th one of its thread
    unrolled_trips = 4 * np.clip(-(-(q - thread - 3 * t) // (4 * t)), 0, None)      # 4 per pass while thread + (4 j + 3) t < q
    in_unrolled = trip < unrolled_trips
    places = {"first": 0, "last": n - 1}
    if n & ~3:
        places["last of the float4 part"] = (n & ~3) - 1
    if n & 3:
        places["first of the tail"] = n & ~3
    for name, mask in (("unrolled loop", in_unrolled), ("single loop", ~in_unrolled)):
        if mask.any():
            places[f"first of the {name}"] = int(4 * f[mask].min())
            places[f"last of the {name}"] = int(4 * f[mask].max() + 3)
    if w > 1:
        places["first of workgroup 1"] = 4 * GS_THREADS
    assert all(0 <= v < n for v in places.values())
    return places, bool(in_unrolled.any())


def k_grad_stats(g, sumsq, flag, n=None):
    L, lib = _L()
    return lib.ts_sgd_grad_stats(L.ptr(g), g.numel() if n is None else n, L.ptr(sumsq), L.ptr(flag), L.stream())


def cells(s0=S0, flag=0):
    return torch.tensor([s0], dtype=torch.float64, device=DEV), torch.tensor([flag], dtype=torch.int32, device=DEV)


def gs_bar(n, ref, s0):
    w, _, k = gs_launch(n)
    return (k + 16 + w) * D * ref + w * D * s0


S_CAP = GS_CAP * GS_THREADS * 4                # elements of one grid-stride step at the cap
GS_SMALL = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 3075, 3076, 3079, 3080, 16384, 16385, 16387]
# 3 s + 3, 3 s + 4 and 8 s + 4 x 257 + 3 with s = S_CAP launch 97, 97 and 257 workgroups - ceil(n / 16384) reaches the cap of 512 only
# above 511 x 16384 elements - so the cap itself is met by two more sizes: 16 s = 8 388 608, exactly 512 workgroups x 16 384 elements
# (the benchmarked model's 32 MB bucket: four passes of the 4x loop, nothing else), and 4 x 257 + 3 elements more (a 17th float4 for
# 257 threads in the single loop, and a three-element tail)
GS_AT_CAP = [3 * S_CAP + 3, 3 * S_CAP + 4, 8 * S_CAP + 4 * 257 + 3, 16 * S_CAP, 16 * S_CAP + 4 * 257 + 3]
assert [min(-(-n // GS_PER_WG), GS_CAP) for n in GS_AT_CAP] == [97, 97, 257, 512, 512]


@pytest.mark.parametrize("n", GS_SMALL + [2097152 + 3] + GS_AT_CAP)
def test_grad_stats_random_gradients(n):
    """tail only; either side of a float4, of a workgroup's first trip, of the 4x loop of a one-workgroup launch (n > 3075), of the
    second workgroup; 129 workgroups; the sizes of GS_AT_CAP"""
    ck = Checks(f"grad_stats n={n}")
    g = (rng("gs", n).randn(n) * 1.5).astype(np.float32)
    ref, bad = O64.grad_stats64(g)
    assert bad == 0
    unrolled = gs_places(n)[1]
    assert unrolled == (n > 3 * gs_launch(n)[1] * 4 + 3)
    gd = torch.from_numpy(g).to(DEV)
    sumsq, flag = cells()
    ck.true("TS_OK", k_grad_stats(gd, sumsq, flag) == 0)
    ck.le("sumsq", "cell - (s0 + float64)", abs(math.fsum([float(sumsq.item()), -S0, -ref])), gs_bar(n, ref, S0))
    ck.true("flag 0 on finite gradients", int(flag.item()) == 0)
    sumsq, flag = cells(flag=1)
    k_grad_stats(gd, sumsq, flag)
    ck.true("a preset flag stays", int(flag.item()) == 1)
    ck.le("sumsq", "second call", abs(math.fsum([float(sumsq.item()), -S0, -ref])), gs_bar(n, ref, S0))
    ck.done()


@pytest.mark.parametrize("n", GS_SMALL + GS_AT_CAP)
def test_grad_stats_one_element(n):
    ck = Checks(f"grad_stats one element n={n}")
    places, _ = gs_places(n)
    gd = torch.zeros(n, dtype=torch.float32, device=DEV)
    sumsq, flag = cells()
    for name, at in places.items():
        for value in (3.0, math.inf, -math.inf, math.nan):
            gd[at] = value
            sumsq.fill_(S0)
            flag.zero_()
            rc = k_grad_stats(gd, sumsq, flag)
            got, got_flag = float(sumsq.item()), int(flag.item())
            gd[at] = 0.0
            if value == 3.0:
                ck.true(f"3.0 at {at} ({name}): cell {got!r} is not exactly {S0 + 9.0}, flag {got_flag}",
                        rc == 0 and got == S0 + 9.0 and got_flag == 0)
            else:
                ck.true(f"{value} at {at} ({name}): flag {got_flag}", rc == 0 and got_flag == 1)
    ck.done()


def test_grad_stats_two_buckets_into_one_cell():
    ck = Checks("grad_stats two buckets")
    na, nb = 16385, 1025
    a, b = (rng("two", n).randn(n).astype(np.float32) for n in (na, nb))
    ra, rb = O64.grad_stats64(a)[0], O64.grad_stats64(b)[0]
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sumsq, flag = cells()
    k_grad_stats(ad, sumsq, flag)
    k_grad_stats(bd, sumsq, flag)
    # the second call's chain adds onto s0 + ra
    ck.le("sumsq", "the sum of both", abs(math.fsum([float(sumsq.item()), -S0, -ra, -rb])), gs_bar(na, ra, S0) + gs_bar(nb, rb, S0 + ra))
    ck.true("flag 0", int(flag.item()) == 0)
    bd[nb - 1] = math.nan
    k_grad_stats(bd, sumsq, flag)
    ck.true("flag 1 after a bucket with a NaN", int(flag.item()) == 1)
    k_grad_stats(ad, sumsq, flag)
    ck.true("and stays 1 after a clean bucket", int(flag.item()) == 1)
    ck.done()


def test_grad_stats_refuses_a_misaligned_pointer_and_takes_nothing():
    """both are decided by the entry point before any launch"""
    L, lib = _L()
    g = torch.ones(64, dtype=torch.float32, device=DEV)
    sumsq, flag = cells()
    assert k_grad_stats(g[1:33], sumsq, flag) == INVALID and b"16-byte aligned" in lib.ts_last_error()
    assert lib.ts_sgd_grad_stats(None, 0, L.ptr(sumsq), L.ptr(flag), L.stream()) == 0
    torch.cuda.synchronize()
    assert float(sumsq.item()) == S0 and int(flag.item()) == 0


# -------------------------------------------------------------------------------------------------------------- ts_sgd_decide

MAX_NORM, GROWTH, BACKOFF = 10.0, 2.0, 0.5
KEEP = [5.5, -0.0, 1e-40]                      # state[5..7]: a value, a sign bit alone, a denormal


def k_decide(sumsq, nonfinite, state, max_norm, growth, backoff, interval, amp):
    """one launch on cells written by the test; returns (state [8] float32 on the CPU, sumsq after, nonfinite after)"""
    L, lib = _L()
    sd, fd = cells(sumsq, nonfinite)
    st = torch.tensor(state, dtype=torch.float32, device=DEV)
    L.check(lib.ts_sgd_decide(L.ptr(sd), L.ptr(fd), L.ptr(st), max_norm, growth, backoff, interval, amp, L.stream()), "ts_sgd_decide")
    return st.cpu(), float(sd.item()), int(fd.item())


def clip_boundary(max_norm, scale):
    """the two neighbouring doubles sumsq around which the float64 coefficient max_norm / (sqrt(sumsq) / scale + 1e-6), rounded to
    float32, turns from exactly 1.0f into the float32 just below 1: found by bisection over the doubles' bit patterns (the
    coefficient falls monotonically), downwards from (max_norm scale)^2, where it is below 1"""
    mx = f32(max_norm)
    one = lambda s: np.float32(mx / (math.sqrt(s) / scale + O64.EPS)) >= np.float32(1.0)
    as_int = lambda x: int(np.float64(x).view(np.int64))
    as_float = lambda i: float(np.int64(i).view(np.float64))
    hi = as_int((mx * scale) ** 2)
    lo = as_int((mx * scale) ** 2 * 0.5)
    assert one(as_float(lo)) and not one(as_float(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if one(as_float(mid)) else (lo, mid)
    near, far = as_float(lo), as_float(hi)
    assert np.float32(mx / (math.sqrt(near) / scale + O64.EPS)) == np.float32(1.0)
    assert np.float32(mx / (math.sqrt(far) / scale + O64.EPS)) == np.nextafter(np.float32(1.0), np.float32(0.0))
    return near, far


def check_decide(ck, tag, sumsq, nonfinite, state01, max_norm, growth, interval, amp, coefficient_one=False, at_most_one=False):
    state = [state01[0], state01[1], 7.0, 7.0, 7.0] + KEEP
    state_in = torch.tensor(state, dtype=torch.float32)
    got, sumsq_after, flag_after = k_decide(sumsq, nonfinite, state, max_norm, growth, BACKOFF, interval, amp)
    want = O64.decide64(sumsq, nonfinite, state_in.numpy(), f32(max_norm), f32(growth), f32(BACKOFF), interval, amp)
    scale = float(state_in[0]) if amp else 1.0
    r = 0 if math.frexp(scale)[0] == 0.5 else 1
    inv32 = np.float32(1.0) / np.float32(scale)
    ck.true(f"{tag}: skip flag {float(got[3])} != {want[3]}", float(got[3]) == want[3])
    ck.true(f"{tag}: scale {float(got[0])!r} != {float(want[0])!r}", got[0].numpy().view(np.int32) == want[0].view(np.int32))
    ck.true(f"{tag}: tracker {float(got[1])} != {float(want[1])}", float(got[1]) == float(want[1]))
    ck.true(f"{tag}: state[5..7] keep their bits", torch.equal(bits(got[5:]), bits(state_in[5:])))
    ck.true(f"{tag}: sumsq and nonfinite are re-armed", sumsq_after == 0.0 and flag_after == 0)
    if math.isfinite(sumsq):
        ck.le("state[4]", f"{tag}: norm", abs(float(got[4]) - want[4]), SLACK * (2 + r) * U * want[4] + TINY)
        ck.le("state[2]", f"{tag}: coefficient / scale", abs(float(got[2]) - want[2]), SLACK * (5.5 + 2 * r) * U * want[2] + TINY)
        if coefficient_one:
            ck.true(f"{tag}: state[2] = {float(got[2])!r} is not exactly 1 / scale = {float(inv32)!r}", got[2].numpy() == inv32)
        if at_most_one:
            ck.true(f"{tag}: state[2] = {float(got[2])!r} exceeds 1 / scale", got[2].numpy() <= inv32)
    elif math.isnan(sumsq):
        ck.true(f"{tag}: the norm of a NaN sum is NaN", math.isnan(float(got[4])))
    else:
        ck.true(f"{tag}: the norm of an infinite sum is infinite, the coefficient 0", float(got[4]) == math.inf and float(got[2]) == 0.0)
    return got


@pytest.mark.parametrize("scale", [1.0, 65536.0, 2.0 ** -3, 1000.0])
@pytest.mark.parametrize("amp", [0, 1])
def test_decide(amp, scale):
    ck = Checks(f"decide amp={amp} scale={scale:g}")
    eff = scale if amp else 1.0                # without amp the scale counts as 1 whatever state[0] holds
    clean = (3.0 * eff) ** 2                   # a sum of squares of scaled gradients whose unscaled norm is 3
    kw = dict(max_norm=MAX_NORM, growth=GROWTH, interval=2000, amp=amp)
    check_decide(ck, "sumsq 0", 0.0, 0, (scale, 0.0), coefficient_one=True, **kw)
    got = check_decide(ck, "sumsq 0: the norm is 0", 0.0, 0, (scale, 0.0), **kw)
    ck.true("sumsq 0: norm exactly 0", float(got[4]) == 0.0)
    near, far = clip_boundary(MAX_NORM, eff)
    check_decide(ck, "clip boundary, near side", near, 0, (scale, 0.0), coefficient_one=True, **kw)
    check_decide(ck, "clip boundary, far side", far, 0, (scale, 0.0), at_most_one=True, **kw)
    check_decide(ck, "norm 1000 max_norm", (1e3 * MAX_NORM * eff) ** 2, 0, (scale, 0.0), at_most_one=True, **kw)
    for mx in (0.0, -1.0):
        check_decide(ck, f"max_norm {mx}", (1e3 * MAX_NORM * eff) ** 2, 0, (scale, 0.0), coefficient_one=True, **{**kw, "max_norm": mx})
    for tag, s, flag in (("nonfinite 1, finite sumsq", clean, 1), ("sumsq inf", math.inf, 0), ("sumsq nan", math.nan, 0)):
        got = check_decide(ck, tag, s, flag, (scale, 5.0), **kw)
        ck.true(f"{tag}: skip", float(got[3]) == 1.0)
        if amp:
            ck.true(f"{tag}: scale x backoff, tracker 0", float(got[0]) == float(np.float32(scale) * np.float32(BACKOFF)) and float(got[1]) == 0.0)
        else:
            ck.true(f"{tag}: no amp, scale and tracker untouched", float(got[0]) == f32(scale) and float(got[1]) == 5.0)
    for interval in (1, 3, 2000):
        for tracker in (interval - 2, interval - 1):
            if tracker < 0:
                continue
            got = check_decide(ck, f"interval {interval}, tracker {tracker}", clean, 0, (scale, float(tracker)), **{**kw, "interval": interval})
            if not amp:
                ck.true("no amp: a clean step leaves scale and tracker alone", float(got[0]) == f32(scale) and float(got[1]) == tracker)
            elif tracker == interval - 1:
                ck.true(f"interval {interval}: grown, tracker 0", float(got[0]) == f32(scale) * 2.0 and float(got[1]) == 0.0)
            else:
                ck.true(f"interval {interval}: tracker {interval - 1}", float(got[0]) == f32(scale) and float(got[1]) == interval - 1)
    ck.done()


def test_decide_at_the_largest_scale():
    """2^127 x 2 is not a float: torch.amp.GradScaler keeps the scale ("Do not grow the scale past fp32 bounds to inf") and resets the
    tracker, and so does decide64; 1 / scale is a denormal"""
    ck = Checks("decide scale=2^127")
    big = 2.0 ** 127
    got = check_decide(ck, "growth at 2^127", 1.21 * 2.0 ** 252, 0, (big, 2.0), MAX_NORM, GROWTH, 3, 1, coefficient_one=True)
    ck.true(f"the scale stays 2^127 (is {float(got[0])!r}), tracker 0", float(got[0]) == big and float(got[1]) == 0.0)
    got = check_decide(ck, "backoff at 2^127", 1.21 * 2.0 ** 252, 1, (big, 2.0), MAX_NORM, GROWTH, 3, 1)
    ck.true("backoff: 2^126", float(got[0]) == 2.0 ** 126)
    ck.done()


# --------------------------------------------------------------------------------------------------------------- ts_sgd_apply

HYPER = [(0.1, 0.9, 1e-2), (0.24, 0.9, 1e-4), (0.05, 0.0, 0.0)]


def k_apply(p, g, m, state, hyper, first):
    L, lib = _L()
    p, m = p.clone(), m.clone()
    L.check(lib.ts_sgd_apply(L.ptr(p), L.ptr(g), L.ptr(m), p.numel(), L.ptr(state), *hyper, first, L.stream()), "ts_sgd_apply")
    return p, m


def apply_bars(p64, mags, lr, momentum, nesterov, first):
    """(bar of m', bar of p') per element, from the magnitudes of the float64 reference; lr, momentum, nesterov: numbers or tensors"""
    a, b, c = mags
    big_a = a + b + c
    e_d = 2 * U * (a + b)
    e_m = e_d if first else 3 * U * (a + b) + 2 * U * c
    plain = SLACK * (lr * e_m + U * (2 * lr * big_a + p64.abs())) + 4 * TINY
    s = a + b + momentum * big_a
    e_s = e_d + momentum * e_m + U * (2 * momentum * big_a + a + b)
    nest = SLACK * (lr * e_s + U * (2 * lr * s + p64.abs())) + 5 * TINY
    return SLACK * e_m + 3 * TINY, nest * nesterov + plain * (1 - nesterov)


def check_apply(ck, tag, p, g, m, gs, hyper, first):
    """p, g, m: float32 CPU tensors; one ts_sgd_apply launch against apply64, every element"""
    state = make_state(gs)
    gs32 = float(state[2].cpu())
    h32 = tuple(f32(v) for v in hyper)
    pd, gd, md = p.to(DEV), g.to(DEV), m.to(DEV)
    got_p, got_m = (t.cpu() for t in k_apply(pd, gd, md, state, hyper, first))
    want_p, want_m, mags = O64.apply64(p, g, m, gs32, *h32, 0, first)
    bar_m, bar_p = apply_bars(p.double(), mags, h32[0], h32[1], 0, first)
    ck.true(f"{tag}: every element finite", bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(got_m).all()))
    ck.le("m'", f"{tag}: worst error / the element's bar", float(((got_m.double() - want_m).abs() / bar_m).max()), 1.0)
    ck.le("p'", f"{tag}: worst error / the element's bar", float(((got_p.double() - want_p).abs() / bar_p).max()), 1.0)
    ck.true(f"{tag}: the step moved the parameters", not torch.equal(got_p, p) or float(g.abs().max()) < 1e-20)
    return pd, gd, md


@pytest.mark.parametrize("hyper", HYPER, ids=lambda h: "lr%g-mom%g-wd%g" % h)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, AP_CAP, AP_CAP + 257])
def test_apply(n, hyper):
    """one element, either side of a workgroup, several workgroups with a ragged end, exactly the grid cap of 8192 x 256 elements and
    one grid-stride pass more; gs 1, 0.37 and 2^-16 on gradients scaled by 2^16 (an AMP step); with first = 1 the momentum bucket
    holds NaN (it is not read)"""
    ck = Checks(f"apply n={n} lr={hyper[0]:g} momentum={hyper[1]:g} wd={hyper[2]:g}")
    rs = rng("apply", n)
    p, g, m = (torch.from_numpy(rs.randn(n).astype(np.float32)) for _ in range(3))
    nan = torch.full((n,), math.nan)
    for gs in (1.0, 0.37, 2.0 ** -16):
        for first in (0, 1):
            gg = g * 65536.0 if gs == 2.0 ** -16 else g
            pd, gd, md = check_apply(ck, f"gs={gs:g} first={first}", p, gg, nan if first else m, gs, hyper, first)
    got_p, got_m = k_apply(pd, gd, md, make_state(0.37, skip=1.0), hyper, 1)
    ck.true("state[3] = 1: no bit of p or m changes", same_bits(got_p, pd) and torch.equal(bits(got_m), bits(md)))
    ck.done()


@pytest.mark.parametrize("hyper", HYPER, ids=lambda h: "lr%g-mom%g-wd%g" % h)
def test_apply_underflow(hyper):
    """gradients of 1e-30 with gs = 1; and p, g, m all around 2^-120, where wd p and lr m' are denormals: a kernel that flushed them
    to zero would miss the bars by 2^-126"""
    ck = Checks(f"apply underflow lr={hyper[0]:g} momentum={hyper[1]:g} wd={hyper[2]:g}")
    n = 4099
    rs = rng("underflow", n)
    p, g, m = (torch.from_numpy(rs.randn(n).astype(np.float32)) for _ in range(3))
    for first in (0, 1):
        check_apply(ck, f"g 1e-30 first={first}", p, g * 1e-30, m, 1.0, hyper, first)
        tiny = 2.0 ** -120
        check_apply(ck, f"all 2^-120 first={first}", p * tiny, g * tiny, m * tiny, 0.37, hyper, first)
    ck.done()


# ------------------------------------------------------------------------------------------------------ ts_sgd_apply_segments

SEG_LAYOUTS = dict(LAYOUTS)
SEG_LAYOUTS.update({"cap_exact": [SEG_CAP - 16, 5],                       # ends at 2048 tiles, a slot boundary in the last one
                    "cap_crossed": [4200000, 5, 4188603, 4099],           # a boundary tile beyond the cap and a last partial tile
                    "cap_whole_tile": [SEG_CAP, 4096, 100]})              # a whole tile inside one slot beyond the cap
SEG_UNUSED = {"one": (0,), "small": (0, 2), "tiles": (1, 2), "mixed40": (4, 9, 19, 20, 39), "cap_exact": (1,), "cap_crossed": (1, 3),
              "cap_whole_tile": (1,)}
SEG_VARIANTS = ["one_group", "one_group_nesterov", "group_per_slot", "unused_slots", "unused_slots_flags", "skipped_step"]
SEG_GS = 0.37


@functools.lru_cache(maxsize=None)
def seg_bucket(layout):
    bk = Bucket(SEG_LAYOUTS[layout], seed=len(layout))
    bk.cpu = tuple(t.cpu() for t in (bk.p, bk.g, bk.m))
    bk.inside_cpu = bk.inside.cpu()
    return bk


def check_segments(ck, tag, bk, before, got_p, got_m, gs32, group_of, values, unused=(), flags=None, skipped_step=False):
    """one ts_sgd_apply_segments launch against apply_segments64, every element; before = (p, g, m) on the CPU, got_* on the CPU"""
    p, g, m = before
    values32 = [(f32(a), f32(b), f32(c), int(d)) for a, b, c, d in values]
    outside = ~bk.inside_cpu
    ck.true(f"{tag}: the padding is zero before", float(p[outside].abs().sum()) == 0 and float(m[outside].abs().sum()) == 0
            and float(g[outside].abs().sum()) == 0)
    ck.true(f"{tag}: the padding is exactly zero after", float(got_p[outside].abs().sum()) == 0 and float(got_m[outside].abs().sum()) == 0)
    if skipped_step:
        ck.true(f"{tag}: state[3] = 1, no bit of p or m changes", same_bits(got_p, p) and same_bits(got_m, m))
        return
    want_p, want_m, mags = O64.apply_segments64(p, g, m, bk.offsets[:-1], bk.sizes, gs32, group_of, values32, unused=unused,
                                                flags=None if flags is None else flags.cpu())
    active = mags["active"] > 0
    bar_m, bar_p = apply_bars(p.double(), (mags["a"], mags["b"], mags["c"]), mags["lr"], mags["momentum"], mags["nesterov"], 0)
    ck.true(f"{tag}: every element finite", bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(got_m).all()))
    kept = bk.inside_cpu & ~active               # (the padding is held to zero above: its zeros carry either sign)
    ck.true(f"{tag}: slots that are skipped keep their bits", torch.equal(bits(got_p)[kept], bits(p)[kept])
            and torch.equal(bits(got_m)[kept], bits(m)[kept]))
    if bool(active.any()):
        ck.le("m'", f"{tag}: worst error / the element's bar", float(((got_m.double() - want_m).abs() / bar_m)[active].max()), 1.0)
        ck.le("p'", f"{tag}: worst error / the element's bar", float(((got_p.double() - want_p).abs() / bar_p)[active].max()), 1.0)
    for i, (o, s) in enumerate(zip(bk.offsets[:-1], bk.sizes)):         # beyond the grid cap: every slot that is applied changed
        lo, hi = max(int(o), SEG_CAP), int(o) + int(s)
        if lo < hi and bool(active[lo]):
            ck.true(f"{tag}: slot {i} beyond element {SEG_CAP} did not change",
                    not torch.equal(bits(got_p)[lo:hi], bits(p)[lo:hi]) and not torch.equal(bits(got_m)[lo:hi], bits(m)[lo:hi]))


@pytest.mark.parametrize("variant", SEG_VARIANTS)
@pytest.mark.parametrize("layout", list(SEG_LAYOUTS))
def test_apply_segments(layout, variant):
    bk = seg_bucket(layout)
    k = len(bk.sizes)
    ck = Checks(f"apply_segments {layout} {variant}")
    state = make_state(SEG_GS, skip=1.0 if variant == "skipped_step" else 0.0)
    gs32 = float(state[2].cpu())
    one = (0.1, 0.9, 1e-2, 1 if variant == "one_group_nesterov" else 0)
    kw, ref = {}, dict(group_of=[0] * k, values=[one])
    if variant == "group_per_slot":            # the values of test_segments_kernel_per_slot_groups_equal_ts_sgd_apply_per_slot
        values = [(0.01 * (1 + i % 7), 0.5 + 0.05 * (i % 9), 1e-3 * (i % 4), i % 2) for i in range(k)]
        kw, ref = dict(group_of=np.arange(k), group_values=values), dict(group_of=list(range(k)), values=values)
    elif variant.startswith("unused_slots"):
        unused = SEG_UNUSED[layout]
        kw, ref["unused"] = dict(unused=unused), unused
        if variant == "unused_slots_flags":    # applied where some rank had a gradient (flag > 0), skipped where none had (flag 0)
            flags = torch.ones(k, device=DEV)
            flags[unused[0]] = 0.5
            for i in unused[1:]:
                flags[i] = 0.0
            kw["flags"] = ref["flags"] = flags
    got_p, got_m = apply_segments(bk, state, one, 0, **kw)
    check_segments(ck, variant, bk, bk.cpu, got_p.cpu(), got_m.cpu(), gs32, skipped_step=variant == "skipped_step", **ref)
    ck.done()


# --------------------------------------------------------------------------------------------- the chain of FlatSGD.step()

def test_the_chain_of_a_step():
    """ts_sgd_grad_stats on two buckets, ts_sgd_decide, ts_sgd_apply_segments on both - five steps (0 .. 4) with amp, scale 1024,
    interval 3, max_norm 0.5, gradients of unscaled norm 3 (clipped); step 3 carries one inf in the second bucket's last element:
    it changes no bit of p and m and halves the scale, which has grown in step 2"""
    L, lib = _L()
    ck = Checks("chain")
    bks = [Bucket(LAYOUTS["mixed40"], seed=11), Bucket(LAYOUTS["tiles"], seed=12)]
    for bk in bks:
        bk.inside_cpu = bk.inside.cpu()
        bk.slot_table = bk.slots()
    hyper = (0.24, 0.9, 1e-4, 1)
    max_norm, interval = 0.5, 3
    state = torch.tensor([1024.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV)
    sumsq, flag = cells(0.0, 0)
    count = sum(sum(bk.sizes) for bk in bks)
    rs = rng("chain")
    scales = []
    for step in range(5):
        before_state = state.cpu()
        scale = float(before_state[0])
        refs = []
        for bk in bks:
            g = rs.randn(bk.n).astype(np.float32) * bk.inside_cpu.numpy() * np.float32(3.0 / math.sqrt(count) * scale)
            bk.g = torch.from_numpy(g).to(DEV)
        if step == 3:
            bks[1].g[int(bks[1].offsets[-2]) + bks[1].sizes[-1] - 1] = math.inf
        total, bar, bad = 0.0, 0.0, 0
        for bk in bks:
            s, b = O64.grad_stats64(bk.g.cpu())
            bar += gs_bar(bk.n, s, total) if b == 0 else 0.0
            total, bad = total + s, bad | b
            ck.true(f"step {step}: ts_sgd_grad_stats", k_grad_stats(bk.g, sumsq, flag) == 0)
        dev_sumsq, dev_flag = float(sumsq.item()), int(flag.item())
        ck.true(f"step {step}: nonfinite {dev_flag} != {bad}", dev_flag == bad and bad == int(step == 3))
        if not bad:
            ck.le("sumsq", f"step {step}", abs(dev_sumsq - total), bar + D * total)
        L.check(lib.ts_sgd_decide(L.ptr(sumsq), L.ptr(flag), L.ptr(state), max_norm, GROWTH, BACKOFF, interval, 1, L.stream()), "decide")
        got = state.cpu()
        want = O64.decide64(dev_sumsq, dev_flag, before_state.numpy(), f32(max_norm), GROWTH, BACKOFF, interval, 1)
        ck.true(f"step {step}: scale, tracker and skip flag are decide64's", float(got[0]) == float(want[0])
                and float(got[1]) == float(want[1]) and float(got[3]) == want[3] == float(step == 3))
        if not bad:
            ck.le("state[4]", f"step {step}", abs(float(got[4]) - want[4]), SLACK * 2 * U * want[4] + TINY)
            ck.le("state[2]", f"step {step}", abs(float(got[2]) - want[2]), SLACK * 5.5 * U * want[2] + TINY)
            ck.true(f"step {step}: the norm is about 3 and clipped", 2.9 < float(got[4]) < 3.1 and float(got[2]) * scale < 0.2)
        ck.true(f"step {step}: the cells are re-armed", float(sumsq.item()) == 0.0 and int(flag.item()) == 0)
        for i, bk in enumerate(bks):
            before = (bk.p.cpu(), bk.g.cpu(), bk.m.cpu())
            L.check(lib.ts_sgd_apply_segments(L.ptr(bk.p), L.ptr(bk.g), L.ptr(bk.m), bk.n, L.ptr(state), L.ptr(bk.slot_table),
                                              len(bk.sizes), L.ptr(bk.tile_first), bk.tile_first.numel(), None, None, 1, *hyper, 0,
                                              L.stream()), "ts_sgd_apply_segments")
            check_segments(ck, f"step {step} bucket {i}", bk, before, bk.p.cpu(), bk.m.cpu(), float(got[2]), [0] * len(bk.sizes),
                           [hyper], skipped_step=step == 3)
            if step != 3:
                ck.true(f"step {step} bucket {i}: the step moved p and m", not same_bits(bk.p.cpu(), before[0])
                        and not same_bits(bk.m.cpu(), before[2]))
        scales.append(float(got[0]))
    ck.true(f"the scale grows in step 2 and is halved in step 3: {scales}", scales == [1024.0, 1024.0, 2048.0, 1024.0, 1024.0])
    ck.done()
