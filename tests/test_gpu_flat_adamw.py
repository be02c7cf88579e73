"""ts_adamw_prepare / ts_adamw_apply_segments and what FlatAdamW / taseg_amd.pcseg.optim build on them (-m gpu).

* ts_adamw_prepare: every coefficient inside adamw_ref.coefficient_bars of Python's double arithmetic (one rounding to float plus
  the device pow's stated error) at steps 1, 2, 1000 and 100000; counters + 1 on live slots, untouched on skipped slots and on a
  skipped step (then the coefficient table is untouched too);
* ts_adamw_apply_segments: given the coefficient table the kernel read, the bits of adamw_ref.step32 on every layout of LAYOUTS,
  two groups per bucket (one with weight_decay 0 and the other lerp branch), unused slots with and without a set flag, gs 1 and a
  clip; padding zero, guard words around all four buckets intact, a skipped step keeps every bit, refused arguments write nothing;
* FlatAdamW against torch.optim.AdamW step for step.  The bar is not a constant: three twins run the same problem - torch in
  float32, torch in float64, the flat optimizer - and per tensor and step
      max |flat - float64| <= 4 max |torch32 - float64|
  (the project's margin for "the float32 reference's own distance from float64").  Every line "adamw_float64 ..." printed here
  holds distance and error; profiles/adamw_float64.txt keeps a run's lines;
* the AMP route (a skipped step keeps every bit and halves the scale, no host read inside step()), clipping on both sides of
  max_norm, checkpoints in torch.optim.AdamW's format both ways through a file, the reference's loop unchanged, determinism, and two
  steps of SalsaNext under build_optimizer('adamw', max_norm=10, amp=True) + build_scheduler('onecycle').
"""
import io
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as R  # noqa: E402
from taseg_amd import _lib as L  # noqa: E402
from taseg_amd.optim import _ADAMW_COEF, _ADAMW_GROUP, FlatAdamW  # noqa: E402
from taseg_amd.pcseg import optim as PO  # noqa: E402
from test_gpu_flat_optim import LAYOUTS, Bucket, Cfg, batches, make_state, same_bits, seq_net  # noqa: E402

INVALID = -1                                   # include/taseg_hip.h TS_ERR_INVALID_ARGUMENT
GUARD, PAD = 12345.5, 16                       # guard words: PAD floats on either side of a bucket (64 bytes: alignment is kept)
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 1e-2), (3e-3, 0.3, 0.99, 5e-6, 0.0)]       # (lr, beta1, beta2, eps, wd); the second: w1 = 0.7, no decay
MARGIN = 4.0


def _groups_dev(values):
    return torch.from_numpy(np.array(values, dtype=_ADAMW_GROUP).view(np.uint8)).cuda()


def prepare(bk, state, values, group_of=None, unused=(), flags=None, steps=None):
    """(rc, step array, coefficient records) after ts_adamw_prepare; the table starts as 0x5A bytes"""
    k = len(bk.sizes)
    slots = bk.slots(unused, group_of)
    step = torch.tensor(list(steps) if steps is not None else [0] * k, dtype=torch.int32).cuda()
    coef = torch.full((k * _ADAMW_COEF.itemsize,), 0x5A, dtype=torch.uint8).cuda()
    rc = L.load().ts_adamw_prepare(L.ptr(slots), k, L.ptr(flags), L.ptr(state), L.ptr(_groups_dev(values)), len(values), L.ptr(step),
                                   L.ptr(coef), L.stream())
    return rc, step, coef, slots


def guarded(t):
    big = torch.full((t.numel() + 2 * PAD,), GUARD, device="cuda")
    big[PAD:PAD + t.numel()] = t
    return big, big[PAD:PAD + t.numel()]


def guards_intact(big):
    return bool((big[:PAD] == GUARD).all()) and bool((big[-PAD:] == GUARD).all())


def apply(bk, v, state, slots, coef, flags=None, n=None, n_tiles=None, shift=0):
    """(rc, p, m, v, the four guarded buffers) after ts_adamw_apply_segments on copies"""
    bufs = [guarded(t) for t in (bk.p, bk.g, bk.m, v)]
    ptrs = [L.ptr(view) + 4 * shift for _, view in bufs]
    rc = L.load().ts_adamw_apply_segments(*ptrs, bk.n if n is None else n, L.ptr(state), L.ptr(slots), len(bk.sizes),
                                          L.ptr(bk.tile_first), bk.tile_first.numel() if n_tiles is None else n_tiles, L.ptr(flags),
                                          L.ptr(coef), L.stream())
    return rc, bufs[0][1], bufs[2][1], bufs[3][1], [b for b, _ in bufs]


def second_moment(bk, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(bk.n, generator=gen) * 10.0 ** torch.empty(bk.n).uniform_(-8, 1, generator=gen)).cuda() * bk.inside


def records(coef):
    return coef.cpu().numpy().view(_ADAMW_COEF)


# ---- ts_adamw_prepare ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
def test_prepare_coefficients_against_double(t):
    bk = Bucket(LAYOUTS["small"], seed=1)
    k = len(bk.sizes)
    group_of = np.arange(k) % 2
    rc, step, coef, _ = prepare(bk, make_state(), GROUPS, group_of, unused=(2,), steps=[t - 1] * k)
    assert rc == 0
    rec, step = records(coef), step.cpu().numpy()
    for i in range(k):
        if i == 2:                                               # skipped slot: counter and record untouched
            assert step[i] == t - 1 and rec[i].tobytes() == b"\x5a" * _ADAMW_COEF.itemsize
            continue
        assert step[i] == t
        want, bars = R.coefficients64(*GROUPS[group_of[i]], t), R.coefficient_bars(*GROUPS[group_of[i]], t)
        for key in R.KEYS:
            err = abs(float(rec[i][key]) - want[key])
            print(f"adamw_prepare t={t} slot {i} {key}: error {err:.3e} bar {bars[key]:.3e}")
            assert err <= bars[key], (i, key, err, bars[key])
        assert rec[i]["live"] == (1 | (2 if want["has_decay"] else 0))
    if t == 100000:                                              # beta2^t has underflowed the correction to 1
        assert all(rec[i]["bc2_sqrt"] == 1.0 for i in range(k) if i != 2)


def test_prepare_counters_on_skipped_slots_and_a_skipped_step():
    bk = Bucket(LAYOUTS["mixed40"], seed=2)
    k = len(bk.sizes)
    start = list(np.arange(k) % 5)
    rc, step, coef, _ = prepare(bk, make_state(skip=1.0), GROUPS, np.arange(k) % 2, steps=start)       # skipped step: nothing written
    assert rc == 0 and step.cpu().tolist() == start and bool((coef == 0x5A).all())
    flags = torch.ones(k, device="cuda")
    flags[4], flags[9] = 0.5, 0.0
    rc, step, coef, _ = prepare(bk, make_state(), GROUPS, np.arange(k) % 2, unused=(4, 9), flags=flags, steps=start)
    want = [s + (0 if i == 9 else 1) for i, s in enumerate(start)]                                      # 4: some rank had a gradient
    assert rc == 0 and step.cpu().tolist() == want
    rc, step, coef, _ = prepare(bk, make_state(), GROUPS, np.arange(k) % 2, unused=(4, 9), steps=start)
    assert step.cpu().tolist() == [s + (0 if i in (4, 9) else 1) for i, s in enumerate(start)]


# ---- ts_adamw_apply_segments --------------------------------------------------------------------------------------------------
def expected(bk, v, gs, rec, skipped):
    p, g, m, v = (t.cpu().numpy().copy() for t in (bk.p, bk.g, bk.m, v))
    for i, (o, s) in enumerate(zip(bk.offsets[:-1], bk.sizes)):
        if i in skipped:
            continue
        c = {key: rec[i][key] for key in R.KEYS}
        c["has_decay"] = bool(rec[i]["live"] & 2)
        sl = slice(int(o), int(bk.offsets[i + 1]))               # the slot and its padding (zeros of either sign, which the rule keeps zero)
        p[sl], m[sl], v[sl] = R.step32(p[sl], g[sl], m[sl], v[sl], gs, c)
    return p, m, v


def bits_equal(t, want):
    return np.array_equal(t.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("gs", [1.0, 0.37])
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_apply_gives_the_bits_of_the_numpy_rule(layout, swap, gs):
    bk = Bucket(LAYOUTS[layout], seed=len(layout) + swap)
    k = len(bk.sizes)
    v = second_moment(bk, 7)
    group_of = (np.arange(k) + swap) % 2
    state = make_state(gs)
    unused = (1,) if k >= 3 else ()
    rc, _, coef, slots = prepare(bk, state, GROUPS, group_of, unused=unused, steps=np.arange(k) % 5)
    assert rc == 0
    rc, p, m, v2, bufs = apply(bk, v, state, slots, coef)
    assert rc == 0
    rec = records(coef)
    want = expected(bk, v, gs, rec, set(unused))
    assert not same_bits(p, bk.p) and not same_bits(m, bk.m) and not same_bits(v2, v)                  # (the step did something)
    assert bits_equal(p, want[0]) and bits_equal(m, want[1]) and bits_equal(v2, want[2])
    assert {int(r["live"]) for i, r in enumerate(rec) if i not in unused} <= {1, 3}
    for t in (p, m, v2):
        assert float(t[~bk.inside].abs().sum()) == 0                                                   # padding still zero
    assert all(guards_intact(b) for b in bufs)
    if k >= 3:        # several ranks: slot 0 unused here but some rank had a gradient (applied), slot 1 unused everywhere (skipped)
        flags = torch.ones(k, device="cuda")
        flags[0], flags[1] = 0.5, 0.0
        rc, _, coef, slots = prepare(bk, state, GROUPS, group_of, unused=(0, 1), flags=flags, steps=np.arange(k) % 5)
        rc2, p, m, v2, bufs = apply(bk, v, state, slots, coef, flags=flags)
        want = expected(bk, v, gs, records(coef), {1})
        assert rc == 0 and rc2 == 0 and bits_equal(p, want[0]) and bits_equal(m, want[1]) and bits_equal(v2, want[2])
        assert all(guards_intact(b) for b in bufs)
    # a skipped step (non-finite gradients) keeps every bit; so does a bucket whose slots are all unused
    rc, p, m, v2, bufs = apply(bk, v, make_state(gs, skip=1.0), slots, coef)
    assert rc == 0 and same_bits(p, bk.p) and same_bits(m, bk.m) and same_bits(v2, v) and all(guards_intact(b) for b in bufs)
    rc, p, m, v2, bufs = apply(bk, v, state, bk.slots(range(k), group_of), coef)
    assert rc == 0 and same_bits(p, bk.p) and same_bits(m, bk.m) and same_bits(v2, v)


def test_apply_refuses_bad_arguments_and_writes_nothing():
    bk = Bucket(LAYOUTS["tiles"], seed=3)
    v = second_moment(bk, 8)
    state = make_state()
    _, _, coef, slots = prepare(bk, state, GROUPS[:1])
    for kw in ({"shift": 1, "n": bk.n - 4}, {"n": bk.n - 1}, {"n_tiles": bk.tile_first.numel() + 1}, {"n_tiles": bk.tile_first.numel() - 1}):
        rc, p, m, v2, bufs = apply(bk, v, state, slots, coef, **kw)
        assert rc == INVALID, kw
        assert same_bits(p, bk.p) and same_bits(m, bk.m) and same_bits(v2, v) and all(guards_intact(b) for b in bufs), kw
    assert L.load().ts_adamw_prepare(L.ptr(slots), len(bk.sizes), None, L.ptr(state), L.ptr(_groups_dev(GROUPS)), 0, L.ptr(coef),
                                     L.ptr(coef), L.stream()) == INVALID


# ---- FlatAdamW against torch.optim.AdamW, the bar from torch's own distance to float64 ------------------------------------------
HYPER = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)


class LateNet(torch.nn.Module):
    """seq_net() and a head that joins the loss from the third step on: its parameters' first gradient arrives late"""

    def __init__(self):
        super().__init__()
        self.body = seq_net()
        torch.manual_seed(2)
        self.late = torch.nn.Linear(24, 7)

    def forward(self, x, use_late=False):
        out = self.body(x)
        return out + self.late(x) if use_late else out


def loss_of(net, x, y, use_late=None):
    x = x.to(next(net.parameters()).dtype)
    out = net(x) if use_late is None else net(x, use_late)
    return torch.nn.functional.cross_entropy(out, y)


def torch_step(net, opt, x, y, max_norm=0.0, mult=1.0, use_late=None):
    opt.zero_grad(set_to_none=True)
    (loss_of(net, x, y, use_late) * mult).backward()
    if max_norm:
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm)
    opt.step()


def flat_step(net, opt, x, y, mult=1.0, use_late=None):
    opt.zero_grad()
    flat = getattr(opt, "flat", opt)
    (loss_of(net, x, y, use_late) * mult * flat.loss_scale()).backward()
    opt.step()


def within_margin(a32, a64, b, tag, lines, states=None):
    """per tensor: |flat - float64| <= MARGIN |torch32 - float64|; `states` = (opt32, opt64, moments of the flat one) adds the moments"""
    rows = [(f"p{i}", p32.detach(), p64.detach(), pb.detach())
            for i, (p32, p64, pb) in enumerate(zip(a32.parameters(), a64.parameters(), b.parameters()))]
    if states is not None:
        o32, o64, flat = states
        for i, (p32, p64, pb) in enumerate(zip(a32.parameters(), a64.parameters(), b.parameters())):
            if p32 in o32.state and "exp_avg" in o32.state[p32]:
                mb, vb, _ = flat._moments_of[id(pb)]
                rows.append((f"m{i}", o32.state[p32]["exp_avg"], o64.state[p64]["exp_avg"], mb))
                rows.append((f"v{i}", o32.state[p32]["exp_avg_sq"], o64.state[p64]["exp_avg_sq"], vb))
    missed = []
    for name, t32, t64, tb in rows:
        dist = float((t32.double() - t64).abs().max())
        err = float((tb.double() - t64).abs().max())
        lines.append(f"adamw_float64 {tag:<34} {name:<3} distance {dist:.3e}  error {err:.3e}  error / (4 distance) "
                     f"{err / (MARGIN * dist) if dist > 0 else float('inf') if err > 0 else 0.0:.3f}")
        if not err <= MARGIN * dist:
            missed.append(lines[-1])
    return missed


def finish(lines, missed):
    print("\n".join(lines))
    assert not missed, f"{len(missed)} tensors outside 4 x torch's own distance from float64\n  " + "\n  ".join(missed[:20])


def twins(make=seq_net):
    a32, a64, b = make(), make().double(), make()
    return a32, a64, b


def group_list(net, case):
    if case == "two_groups":
        return [{"params": list(net[0].parameters())},
                {"params": list(net[2].parameters()), "lr": 6e-3, "weight_decay": 0.0, "betas": (0.4, 0.95), "eps": 5e-6}]
    return [{"params": list(net.parameters())}]


@pytest.mark.parametrize("case", ["one_group", "two_groups", "lambda_lr", "onecycle", "late_gradient"])
def test_flat_adamw_follows_torch_adamw(case):
    cfg = Cfg(OPTIMIZER="adamw", LR=HYPER["lr"], WEIGHT_DECAY=HYPER["weight_decay"], BETA1=0.9, BETA2=0.99, EPS=1e-8,
              LEARNING_RATE=HYPER["lr"], SCHEDULER="onecycle" if case == "onecycle" else "linear_warmup_with_cosdecay", WARMUP_EPOCH=1)
    late = case == "late_gradient"
    a32, a64, b = twins(lambda: LateNet().cuda()) if late else twins()
    o32 = torch.optim.AdamW(group_list(a32, case), **HYPER)
    o64 = torch.optim.AdamW(group_list(a64, case), **HYPER)
    if case in ("one_group", "two_groups"):
        ours = PO.FlatOptimizer(b, group_list(b, case), kind="adamw", bucket_mb=0.002, **HYPER)
    else:
        ours = PO.build_optimizer(b, cfg, bucket_mb=0.002)
    assert isinstance(ours, PO.FlatOptimizer) and isinstance(ours.flat, FlatAdamW) and ours.defaults["betas"] == (0.9, 0.99)
    scheds = [PO.build_scheduler(o, 4, 2, cfg) for o in (o32, o64, ours)] if case in ("lambda_lr", "onecycle") else []
    lines, missed, seen = [], [], []
    for it, (x, y) in enumerate(batches()):
        use = (it >= 2) if late else None
        torch_step(a32, o32, x, y, use_late=use)
        torch_step(a64, o64, x, y, use_late=use)
        flat_step(b, ours, x, y, use_late=use)
        for s in scheds:
            s.step()
        missed += within_margin(a32, a64, b, f"{case} step {it + 1}", lines, (o32, o64, ours.flat))
        assert [g["lr"] for g in ours.param_groups] == [g["lr"] for g in o32.param_groups]
        assert [g["betas"] for g in ours.param_groups] == [g["betas"] for g in o32.param_groups]
        seen.append((ours.param_groups[0]["lr"], ours.param_groups[0]["betas"][0]))
    if scheds:
        assert len({s[0] for s in seen}) > 4                     # the schedule moved the rate ...
    if case == "onecycle":
        assert len({s[1] for s in seen}) > 4                     # ... and OneCycleLR beta1
    sd, theirs = ours.state_dict(), o32.state_dict()
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in theirs["param_groups"]]
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    steps = {i: float(s["step"]) for i, s in sd["state"].items()}
    assert steps == {i: float(s["step"]) for i, s in theirs["state"].items()}
    assert all(s["step"].dtype == torch.float32 and s["step"].dim() == 0 and s["step"].device.type == "cpu" for s in sd["state"].values())
    if late:                                                     # the late head's counters lag by the two steps it sat out
        assert sorted(set(steps.values())) == [6.0, 8.0] and [steps[i] for i in (4, 5)] == [6.0, 6.0]
        assert [int(ours.state[p]["step"]) for p in b.late.parameters()] == [6, 6]
    finish(lines, missed)


@pytest.mark.parametrize("mult", [1.0, 4000.0])
def test_clipping_on_both_sides_of_max_norm(mult):
    a32, a64, b = twins()
    o32, o64 = torch.optim.AdamW(a32.parameters(), **HYPER), torch.optim.AdamW(a64.parameters(), **HYPER)
    ours = FlatAdamW(b, max_norm=10.0, bucket_mb=0.002, **HYPER)
    lines, missed, norms = [], [], []
    for it, (x, y) in enumerate(batches(4)):
        torch_step(a32, o32, x, y, max_norm=10.0, mult=mult)
        torch_step(a64, o64, x, y, max_norm=10.0, mult=mult)
        flat_step(b, ours, x, y, mult=mult)
        norms.append(float(ours.state[4]))
        missed += within_margin(a32, a64, b, f"clip x{mult:g} step {it + 1}", lines, (o32, o64, ours))
    assert all(n > 10.0 for n in norms) if mult > 1 else all(0 < n < 10.0 for n in norms), norms
    finish(lines, missed)


def _no_host_read(*a, **k):
    raise AssertionError("a host read inside step()")


def test_amp_route_skips_on_the_device_and_reads_nothing(monkeypatch):
    a32, a64, b = twins()
    o32, o64 = torch.optim.AdamW(a32.parameters(), **HYPER), torch.optim.AdamW(a64.parameters(), **HYPER)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3)
    ours = FlatAdamW(b, amp=True, max_norm=10.0, init_scale=1024.0, growth_interval=3, bucket_mb=0.002, **HYPER)
    lines, missed = [], []
    for it, (x, y) in enumerate(batches(6)):
        poison = float("inf") if it == 2 else 1.0
        o32.zero_grad(set_to_none=True)
        scaler.scale(loss_of(a32, x, y) * poison).backward()
        scaler.unscale_(o32)
        torch.nn.utils.clip_grad_norm_(a32.parameters(), 10.0)
        scaler.step(o32)
        scaler.update()
        if it != 2:
            torch_step(a64, o64, x, y, max_norm=10.0)
        before = [t.clone() for bk in ours.reducer.buckets for t in (bk["pflat"], bk["mflat"], bk["vflat"], bk["step"])]
        ours.zero_grad()
        (loss_of(b, x, y) * poison * ours.loss_scale()).backward()
        with monkeypatch.context() as mp, warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # (the mode announces itself as a prototype)
            for name in ("item", "tolist", "cpu", "numpy", "__bool__", "__float__", "__int__"):     # the ways of reading a tensor ...
                mp.setattr(torch.Tensor, name, _no_host_read)
            torch.cuda.set_sync_debug_mode("error")              # ... and whatever else makes the host wait for the device
            try:
                ours.step()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        after = [t for bk in ours.reducer.buckets for t in (bk["pflat"], bk["mflat"], bk["vflat"], bk["step"])]
        if it == 2:                                              # parameters, both moments and the counters keep every bit
            assert all(torch.equal(x0.view(torch.int32), x1.view(torch.int32)) for x0, x1 in zip(before, after))
            assert float(ours.state[0]) == 512.0
        else:
            assert not any(torch.equal(x0.view(torch.int32), x1.view(torch.int32)) for x0, x1 in zip(before, after))
        assert float(ours.state[0]) == scaler.get_scale(), it
        missed += within_margin(a32, a64, b, f"amp step {it + 1}{' (skipped)' if it == 2 else ''}", lines, (o32, o64, ours))
    assert [float(s["step"]) for s in ours.state_dict()["state"].values()] == [5.0] * 4
    assert ours.scaler_state_dict() == scaler.state_dict()
    finish(lines, missed)


@pytest.mark.parametrize("direction", ["flat_to_torch", "torch_to_flat"])
def test_checkpoints_through_a_file(direction):
    a32, a64, b = twins()
    o32, o64 = torch.optim.AdamW(a32.parameters(), **HYPER), torch.optim.AdamW(a64.parameters(), **HYPER)
    data = batches(6)
    first = FlatAdamW(b, bucket_mb=0.002, **HYPER) if direction == "flat_to_torch" else torch.optim.AdamW(b.parameters(), **HYPER)
    for x, y in data[:3]:
        torch_step(a32, o32, x, y)
        torch_step(a64, o64, x, y)
        (flat_step if direction == "flat_to_torch" else torch_step)(b, first, x, y)
    sd = first.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [3.0] * 4
    if direction == "flat_to_torch":
        bucket = first.reducer.buckets[first.reducer._slot_of[id(b[0].weight)][0]]
        i = first.reducer._slot_of[id(b[0].weight)][1]
        assert sd["state"][0]["exp_avg"].data_ptr() == bucket["mflat"].data_ptr() + 4 * bucket["offsets"][i]        # views of the buckets
        assert sd["state"][0]["exp_avg_sq"].data_ptr() == bucket["vflat"].data_ptr() + 4 * bucket["offsets"][i]
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    c = seq_net()
    c.load_state_dict(b.state_dict())
    if direction == "flat_to_torch":
        second = torch.optim.AdamW(c.parameters(), lr=1.0)       # every hyper-parameter comes from the dictionary
        step = torch_step
    else:
        second = PO.build_optimizer(c, Cfg(OPTIMIZER="adamw", LR=1.0, WEIGHT_DECAY=0.0), bucket_mb=0.002)
        step = flat_step
    second.load_state_dict(sd)
    g = second.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"])
    lines, missed = [], []
    for it, (x, y) in enumerate(data[3:], start=3):
        torch_step(a32, o32, x, y)
        torch_step(a64, o64, x, y)
        step(c, second, x, y)
        missed += within_margin(a32, a64, c, f"{direction} step {it + 1}", lines)
    assert [float(s["step"]) for s in second.state_dict()["state"].values()] == [6.0] * 4
    if direction == "torch_to_flat":
        for key, value in (("amsgrad", True), ("maximize", True), ("decoupled_weight_decay", False)):
            bad = o32.state_dict()
            bad["param_groups"][0][key] = value
            with pytest.raises(ValueError, match=key):
                second.load_state_dict(bad)
    finish(lines, missed)


def test_the_reference_loop_runs_unchanged_over_build_optimizer_adamw():
    """R/train.py:400-415 as written - zero_grad, scaler.scale(loss).backward(), scaler.unscale_, clip_grad_norm_, scaler.step,
    scaler.update, scheduler.step - over build_optimizer(model, cfg) with the recipes' keys, against the same lines over
    torch.optim.AdamW; an overflowing step at iteration 4"""
    cfg = Cfg(OPTIMIZER="adamw", LR=2e-3, WEIGHT_DECAY=1e-2, BETA1=0.9, BETA2=0.999, EPS=5e-6, LEARNING_RATE=2e-3, SCHEDULER="onecycle",
              WARMUP_EPOCH=1, GRAD_NORM_CLIP=10)
    a32, a64, b = twins()
    kw = dict(lr=cfg.LR, betas=(cfg.BETA1, cfg.BETA2), eps=cfg.EPS, weight_decay=cfg.WEIGHT_DECAY)
    opts = [torch.optim.AdamW(a32.parameters(), **kw), torch.optim.AdamW(a64.parameters(), **kw), PO.build_optimizer(b, cfg, bucket_mb=0.002)]
    g = opts[2].param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (2e-3, (0.9, 0.999), 5e-6, 1e-2)
    scalers = [torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3) for _ in range(2)]
    scheds = [PO.build_scheduler(o, 4, 2, cfg) for o in opts]
    lines, missed = [], []
    for it, (x, y) in enumerate(batches()):
        poison = float("inf") if it == 4 else 1.0
        if it != 4:                                              # the float64 twin: the same step without a loss scale
            torch_step(a64, opts[1], x, y, max_norm=cfg.GRAD_NORM_CLIP)
        scheds[1].step()
        for net, optimizer, scaler, scheduler in zip((a32, b), opts[::2], scalers, scheds[::2]):
            optimizer.zero_grad()
            loss = loss_of(net, x, y) * poison
            scaler.scale(loss).backward()
            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(net.parameters(), cfg.GRAD_NORM_CLIP)
            scaler.step(optimizer)
            scaler.update()
            scheduler.step()
        missed += within_margin(a32, a64, b, f"reference loop step {it + 1}", lines)
        assert scalers[0].get_scale() == scalers[1].get_scale(), it
        assert opts[0].param_groups[0]["betas"] == opts[2].param_groups[0]["betas"] and opts[0].param_groups[0]["lr"] == opts[2].param_groups[0]["lr"]
    assert scalers[1].get_scale() != 1024.0
    assert [float(s["step"]) for s in opts[2].state_dict()["state"].values()] == [7.0] * 4
    finish(lines, missed)


def test_three_steps_twice_give_the_same_bits():
    runs = []
    for _ in range(2):
        net = seq_net()
        opt = FlatAdamW(net, max_norm=10.0, amp=True, init_scale=1024.0, bucket_mb=0.002, **HYPER)
        for x, y in batches(3):
            flat_step(net, opt, x, y)
        runs.append([t.clone() for bk in opt.reducer.buckets for t in (bk["pflat"], bk["mflat"], bk["vflat"], bk["step"])])
    assert all(torch.equal(x0.view(torch.int32), x1.view(torch.int32)) for x0, x1 in zip(*runs))
    assert int(runs[0][3].min()) == 3


def test_two_salsanext_steps_under_the_recipe(monkeypatch):
    """SalsaNext at the shape of tests/test_gpu_salsanext_model.py: build_optimizer('adamw', max_norm=10, amp=True) and
    build_scheduler('onecycle'), two steps under autocast: finite, every parameter moved, the same bits in a second run"""
    import os
    import test_gpu_salsanext_model as S
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    g = dict(np.load(os.path.join(S.ROOT, "tests", "golden", "model_salsanext.npz"), allow_pickle=False))
    cfg = Cfg(OPTIMIZER="adamw", LR=0.0025, WEIGHT_DECAY=0.01, BETA1=0.9, BETA2=0.999, EPS=0.000005, LEARNING_RATE=0.0025,
              SCHEDULER="onecycle", WARMUP_EPOCH=1)
    runs = []
    for _ in range(2):
        model = S._modes(S._model(g))
        start = [p.detach().clone() for p in model.parameters()]
        optimizer = PO.build_optimizer(model, cfg, max_norm=10.0, amp=True, init_scale=1024.0)
        scheduler = PO.build_scheduler(optimizer, 2, 1, cfg)
        for _step in range(2):
            optimizer.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                ret, _, _ = model(S._batch(g))
            (ret["loss"].float() * optimizer.flat.loss_scale()).backward()
            optimizer.step()
            scheduler.step()
            assert float(optimizer.flat.state[3]) == 0.0 and np.isfinite(float(optimizer.flat.state[4]))
        now = [p.detach().clone() for p in model.parameters()]
        assert all(bool(torch.isfinite(p).all()) for p in now)
        stuck = [n for (n, _), p0, p1 in zip(model.named_parameters(), start, now) if torch.equal(p0, p1)]
        assert not stuck, stuck
        assert {float(s["step"]) for s in optimizer.state_dict()["state"].values()} == {2.0}
        runs.append(now + [t.clone() for bk in optimizer.flat.reducer.buckets for t in (bk["mflat"], bk["vflat"])])
    assert all(torch.equal(x0, x1) for x0, x1 in zip(*runs))
