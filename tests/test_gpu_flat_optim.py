"""ts_sgd_apply_segments and what FlatSGD / taseg_amd.pcseg.optim build on it (-m gpu).

* the kernel against ts_sgd_apply bit for bit (one group, nothing skipped), per slot with several groups, skipped slots, the flag array;
* FlatOptimizer against torch.optim.SGD step for step: Nesterov, groups, the `sgd_fc` grouping, LambdaLR and OneCycleLR - net, data, eight
  steps and bar (rtol 1e-5, atol 1e-6 after every step) of tests/test_gpu_amp.py::test_flat_sgd_matches_torch_sgd_clip_and_gradscaler;
* the reference's loop (GradScaler.scale / unscale_ / clip_grad_norm_ / step / update) over build_optimizer(..., 'sgd') unchanged;
* checkpoints in torch.optim.SGD's and GradScaler's formats, both directions, and the reference trainer's own checkpoint;
* a parameter that never receives a gradient.
"""
import copy
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from taseg_amd import _lib as L  # noqa: E402
from taseg_amd.optim import _GROUP, _SLOT, FlatSGD  # noqa: E402
from taseg_amd.pcseg import optim as PO  # noqa: E402

RTOL, ATOL = 1e-5, 1e-6
MIXED_40 = [1, 3, 5, 17, 33, 255, 257, 1023, 4097, 5001, 7, 16, 15, 31, 4095, 4096, 9001, 2, 129, 12289,
            11, 13, 64, 65, 63, 1000, 3000, 8193, 19, 23, 29, 37, 41, 43, 47, 53, 20000, 59, 61, 67]
LAYOUTS = {"one": [1], "small": [7, 1, 16, 17], "tiles": [4099, 3, 4096], "mixed40": MIXED_40}


class Cfg(dict):
    __getattr__ = dict.__getitem__


class Bucket:
    """parameter, gradient and momentum buckets laid out as GradBucketReducer lays them out (slots on 16-element boundaries, zero
    padding), random inside the slots, with the tables ts_sgd_apply_segments reads"""

    def __init__(self, sizes, seed=0):
        self.sizes = sizes
        self.offsets = np.concatenate([[0], np.cumsum([-(-s // 16) * 16 for s in sizes])]).astype(np.int64)
        self.n = int(self.offsets[-1])
        g = torch.Generator().manual_seed(seed)
        inside = torch.zeros(self.n, dtype=torch.bool)
        for o, s in zip(self.offsets, sizes):
            inside[o:o + s] = True
        self.inside = inside.cuda()
        self.p, self.g, self.m = ((torch.randn(self.n, generator=g) * inside).cuda() for _ in range(3))
        starts = np.arange(-(-self.n // L.SGD_TILE), dtype=np.int64) * L.SGD_TILE
        self.tile_first = torch.from_numpy((np.searchsorted(self.offsets[:-1], starts, side="right") - 1).astype(np.int32)).cuda()

    def slots(self, unused=(), groups=None):
        rec = np.zeros(len(self.sizes), dtype=_SLOT)
        rec["offset"], rec["count"], rec["flag_index"] = self.offsets[:-1], self.sizes, np.arange(len(self.sizes))
        rec["group"] = 0 if groups is None else groups
        rec["unused"][list(unused)] = 1
        return torch.from_numpy(rec.view(np.uint8)).cuda()

    def slice(self, t, i):
        return t[int(self.offsets[i]):int(self.offsets[i]) + self.sizes[i]]


def make_state(gs=1.0, skip=0.0):
    return torch.tensor([1.0, 0.0, gs, skip, 0.0, 0.0, 0.0, 0.0], device="cuda")


def apply_whole(bk, state, hyper, first):
    p, m = bk.p.clone(), bk.m.clone()
    L.check(L.load().ts_sgd_apply(L.ptr(p), L.ptr(bk.g), L.ptr(m), bk.n, L.ptr(state), *hyper, first, L.stream()), "ts_sgd_apply")
    return p, m


def apply_segments(bk, state, hyper=(0.1, 0.9, 1e-2, 0), first=0, unused=(), flags=None, group_of=None, group_values=None):
    p, m = bk.p.clone(), bk.m.clone()
    slots = bk.slots(unused, group_of)
    groups, n_groups = None, 1
    if group_values is not None:
        groups = torch.from_numpy(np.array(group_values, dtype=_GROUP).view(np.uint8)).cuda()
        n_groups = len(group_values)
    L.check(L.load().ts_sgd_apply_segments(L.ptr(p), L.ptr(bk.g), L.ptr(m), bk.n, L.ptr(state), L.ptr(slots), len(bk.sizes),
                                           L.ptr(bk.tile_first), bk.tile_first.numel(), L.ptr(flags), L.ptr(groups), n_groups,
                                           *hyper, first, L.stream()), "ts_sgd_apply_segments")
    return p, m


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("gs", [1.0, 0.37])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_segments_kernel_gives_the_bits_of_ts_sgd_apply(layout, first, gs):
    bk = Bucket(LAYOUTS[layout], seed=len(layout))
    state = make_state(gs)
    want_p, want_m = apply_whole(bk, state, (0.1, 0.9, 1e-2), first)
    got_p, got_m = apply_segments(bk, state, (0.1, 0.9, 1e-2, 0), first)
    assert not same_bits(want_p, bk.p) and not same_bits(want_m, bk.m)            # (the step did something)
    assert same_bits(got_p, want_p) and same_bits(got_m, want_m)
    assert float(got_p[~bk.inside].abs().sum()) == 0 and float(got_m[~bk.inside].abs().sum()) == 0     # padding still zero
    # non-finite gradients (state[3]): nothing is written
    got_p, got_m = apply_segments(bk, make_state(gs, skip=1.0), (0.1, 0.9, 1e-2, 0), first)
    assert same_bits(got_p, bk.p) and same_bits(got_m, bk.m)


@pytest.mark.parametrize("layout", ["small", "tiles", "mixed40"])
def test_segments_kernel_per_slot_groups_equal_ts_sgd_apply_per_slot(layout):
    """every slot a group of its own (the `sgd_fc` recipe): the bits ts_sgd_apply gives on that slot alone with that group's values;
    with Nesterov, torch's formula on the same tensors"""
    bk = Bucket(LAYOUTS[layout], seed=3)
    k = len(bk.sizes)
    state = make_state(0.37)
    values = [(0.01 * (1 + i % 7), 0.5 + 0.05 * (i % 9), 1e-3 * (i % 4), 0) for i in range(k)]
    got_p, got_m = apply_segments(bk, state, group_of=np.arange(k), group_values=values)
    lib = L.load()
    for i in range(k):
        p, m = bk.slice(bk.p, i).clone(), bk.slice(bk.m, i).clone()
        L.check(lib.ts_sgd_apply(L.ptr(p), L.ptr(bk.slice(bk.g, i).clone()), L.ptr(m), p.numel(), L.ptr(state), *values[i][:3], 0,
                                 L.stream()), "ts_sgd_apply")
        assert same_bits(bk.slice(got_p, i), p) and same_bits(bk.slice(got_m, i), m), i
    assert float(got_p[~bk.inside].abs().sum()) == 0 and float(got_m[~bk.inside].abs().sum()) == 0
    nest_p, nest_m = apply_segments(bk, state, group_of=np.arange(k), group_values=[v[:3] + (1,) for v in values])
    assert same_bits(nest_m, got_m)                                   # the buffer does not depend on the flag
    for i in (0, k // 2, k - 1):
        lr, mom, wd, _ = values[i]
        p, g, buf = bk.slice(bk.p, i).double(), bk.slice(bk.g, i).double(), bk.slice(got_m, i).double()
        want = p - lr * ((g * float(state[2]) + wd * p) + mom * buf)
        assert torch.allclose(bk.slice(nest_p, i).double(), want, rtol=1e-6, atol=1e-7), i


@pytest.mark.parametrize("layout,unused", [("small", (0, 2)), ("tiles", (0,)), ("tiles", (1, 2)), ("mixed40", (4, 9, 19, 20, 39))])
def test_segments_kernel_leaves_skipped_slots_alone(layout, unused):
    bk = Bucket(LAYOUTS[layout], seed=5)
    state = make_state(0.37)
    full_p, full_m = apply_segments(bk, state)
    got_p, got_m = apply_segments(bk, state, unused=unused)
    for i in range(len(bk.sizes)):
        want_p, want_m = (bk.p, bk.m) if i in unused else (full_p, full_m)
        assert same_bits(bk.slice(got_p, i), bk.slice(want_p, i)) and same_bits(bk.slice(got_m, i), bk.slice(want_m, i)), i
    assert float(got_p[~bk.inside].abs().sum()) == 0 and float(got_m[~bk.inside].abs().sum()) == 0
    # everything unused: no change
    got_p, got_m = apply_segments(bk, state, unused=range(len(bk.sizes)))
    assert same_bits(got_p, bk.p) and same_bits(got_m, bk.m)
    # several ranks: a locally unused slot is applied when some rank had a gradient (flag > 0) and skipped when none had (flag 0);
    # the flag of a slot with a local gradient is not asked
    flags = torch.ones(len(bk.sizes), device="cuda")
    flags[unused[0]] = 0.5
    for i in unused[1:]:
        flags[i] = 0.0
    got_p, got_m = apply_segments(bk, state, unused=unused, flags=flags)
    for i in range(len(bk.sizes)):
        want_p, want_m = (bk.p, bk.m) if i in unused[1:] else (full_p, full_m)
        assert same_bits(bk.slice(got_p, i), bk.slice(want_p, i)) and same_bits(bk.slice(got_m, i), bk.slice(want_m, i)), i


# ---- against torch.optim.SGD ----------------------------------------------------------------------------------------------
def seq_net():
    torch.manual_seed(1)
    return torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.ReLU(), torch.nn.Linear(40, 7)).cuda()


class HeadNet(torch.nn.Module):
    """seq_net()'s layers under the names the `sgd_fc` recipe looks for"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.body = torch.nn.Linear(24, 40)
        self.classifier = torch.nn.Linear(40, 7)

    def forward(self, x):
        return self.classifier(torch.relu(self.body(x)))


def batches(n=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(16, 24, generator=g).cuda(), torch.randint(0, 7, (16,), generator=g).cuda()) for _ in range(n)]


def close(a, b, where):
    for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
        assert torch.allclose(pa, pb, rtol=RTOL, atol=ATOL), (where, i, float((pa - pb).abs().max()))


def torch_step(net, opt, x, y, max_norm=0.5):
    opt.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(net(x), y).backward()
    torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm)
    opt.step()


def flat_step(net, opt, x, y):
    opt.zero_grad()
    torch.nn.functional.cross_entropy(net(x), y).backward()
    opt.step()


def _groups(net, kind):
    if kind == "two_groups":          # ten times the learning rate and another weight decay on the last layer
        return [{"params": list(net[0].parameters())}, {"params": list(net[2].parameters()), "lr": 0.5, "weight_decay": 5e-3}]
    return [{"params": list(net.parameters())}]


@pytest.mark.parametrize("case", ["nesterov", "two_groups", "sgd_fc", "lambda_lr", "onecycle"])
def test_flat_optimizer_matches_torch_sgd(case):
    cfg = Cfg(OPTIMIZER="sgd_fc" if case == "sgd_fc" else "sgd", LR=0.05, MOMENTUM=0.9, WEIGHT_DECAY=1e-3, LEARNING_RATE=0.05,
              SCHEDULER="onecycle" if case == "onecycle" else "linear_warmup_with_cosdecay", WARMUP_EPOCH=1)
    if case == "sgd_fc":
        a, b = HeadNet().cuda(), HeadNet().cuda()
        ref_groups = [{"params": [p]} for n, p in a.named_parameters() if "classifier" not in n]
        ref_groups.append({"params": list(a.classifier.parameters()), "lr": cfg.LR * 10})
        ref = torch.optim.SGD(ref_groups, lr=cfg.LR, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY)
        ours = PO.build_optimizer(b, cfg, max_norm=0.5, bucket_mb=0.002)
        assert [g["lr"] for g in ours.param_groups] == [0.05, 0.05, 0.5] and [len(g["params"]) for g in ours.param_groups] == [1, 1, 2]
    else:
        a, b = seq_net(), seq_net()
        nesterov = case == "nesterov"
        ref = torch.optim.SGD(_groups(a, case), lr=cfg.LR, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY, nesterov=nesterov)
        ours = PO.FlatOptimizer(b, _groups(b, case), lr=cfg.LR, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY, nesterov=nesterov,
                                max_norm=0.5, bucket_mb=0.002)
    scheds = []
    if case in ("lambda_lr", "onecycle"):
        scheds = [PO.build_scheduler(ref, 4, 2, cfg), PO.build_scheduler(ours, 4, 2, cfg)]         # stepped every iteration
    seen = []
    for it, (x, y) in enumerate(batches()):
        torch_step(a, ref, x, y)
        flat_step(b, ours, x, y)
        for s in scheds:
            s.step()
        close(a, b, (case, it))
        assert [g["lr"] for g in ours.param_groups] == [g["lr"] for g in ref.param_groups]
        assert [g["momentum"] for g in ours.param_groups] == [g["momentum"] for g in ref.param_groups]
        seen.append((ours.param_groups[0]["lr"], ours.param_groups[0]["momentum"]))
    if scheds:
        assert len({s[0] for s in seen}) > 4                     # the schedule moved the rate ...
    if case == "onecycle":
        assert len({s[1] for s in seen}) > 4                     # ... and OneCycleLR the momentum
    for pa, pb in zip(a.parameters(), b.parameters()):           # state[p]['momentum_buffer'] are the live bucket views
        assert torch.allclose(ref.state[pa]["momentum_buffer"], ours.state[pb]["momentum_buffer"], rtol=1e-4, atol=1e-6)


def test_build_optimizer_lr_sequence_equals_the_reference():
    """build_optimizer + build_scheduler on nn.Linear(2, 3): the learning rates the reference's pair produced (optim_sched.npz)"""
    want = np.load(os.path.join(GOLDEN, "optim_sched.npz"))["lr_sequence"]
    net = torch.nn.Linear(2, 3).cuda()
    cfg = Cfg(OPTIMIZER="sgd", LR=0.24, WEIGHT_DECAY=1e-4, MOMENTUM=0.9, NESTEROV=True, SCHEDULER="linear_warmup_with_cosdecay",
              WARMUP_EPOCH=1)
    opt = PO.build_optimizer(net, cfg)
    assert isinstance(opt, torch.optim.Optimizer) and opt.param_groups[0]["nesterov"] is False       # NESTEROV ignored, as there
    sched = PO.build_scheduler(opt, 4, 3, cfg)
    lrs = [opt.param_groups[0]["lr"]]
    for _ in range(12):
        opt.zero_grad()
        net(torch.ones(1, 2, device="cuda")).sum().backward()
        opt.step()
        sched.step()
        lrs.append(opt.param_groups[0]["lr"])
    assert np.array_equal(np.array(lrs, dtype=np.float64), want)


def test_the_reference_loop_runs_unchanged_over_build_optimizer():
    """R/train.py:400-415 as written: zero_grad, scaler.scale(loss).backward(), scaler.unscale_, clip_grad_norm_, scaler.step,
    scaler.update - over build_optimizer(model, cfg) with its defaults, against the same lines over torch.optim.SGD; an overflowing
    step at iteration 4 (skipped by GradScaler.step, scale halved), same scale after every step"""
    a, b = seq_net(), seq_net()
    cfg = Cfg(OPTIMIZER="sgd", LR=0.05, MOMENTUM=0.9, WEIGHT_DECAY=1e-3)
    opts = [torch.optim.SGD(a.parameters(), lr=cfg.LR, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY),
            PO.build_optimizer(b, cfg, bucket_mb=0.002)]
    scalers = [torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3) for _ in range(2)]
    for it, (x, y) in enumerate(batches()):
        poison = float("inf") if it == 4 else 1.0
        for net, optimizer, scaler in zip((a, b), opts, scalers):
            optimizer.zero_grad()
            loss = torch.nn.functional.cross_entropy(net(x), y) * poison
            scaler.scale(loss).backward()
            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            scaler.step(optimizer)
            scaler.update()
        close(a, b, it)
        assert scalers[0].get_scale() == scalers[1].get_scale(), it
    assert scalers[1].get_scale() != 1024.0


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
def _three_steps(a, ref, b, ours, data, where):
    for it, (x, y) in enumerate(data):
        torch_step(a, ref, x, y)
        flat_step(b, ours, x, y)
        close(a, b, (where, it))


@pytest.mark.parametrize("through_file", [False, True])
def test_checkpoint_from_flat_into_torch_sgd(through_file):
    """three steps on FlatSGD, its state_dict() (as it is, and through torch.save / torch.load) into a fresh torch.optim.SGD, three more
    steps on both"""
    a, b = seq_net(), seq_net()
    ours = FlatSGD(b, lr=0.05, momentum=0.9, weight_decay=1e-3, max_norm=0.5, nesterov=True, bucket_mb=0.002)
    data = batches()
    for x, y in data[:3]:
        flat_step(b, ours, x, y)
    sd = ours.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1, 2, 3]
    assert {k: v for k, v in sd["param_groups"][0].items()} == {"lr": 0.05, "momentum": 0.9, "dampening": 0, "weight_decay": 1e-3,
                                                                "nesterov": True, "maximize": False, "params": [0, 1, 2, 3]}
    bi, i = ours.reducer._slot_of[id(b[0].weight)]
    bucket = ours.reducer.buckets[bi]
    assert sd["state"][0]["momentum_buffer"].data_ptr() == bucket["mflat"].data_ptr() + 4 * bucket["offsets"][i]     # a view of the bucket
    if through_file:
        buf = io.BytesIO()
        torch.save(sd, buf)
        buf.seek(0)
        sd = torch.load(buf, weights_only=True)
    else:
        sd = copy.deepcopy(sd)                                   # (torch's load_state_dict keeps the tensors it is handed)
    a.load_state_dict(b.state_dict())
    ref = torch.optim.SGD(a.parameters(), lr=1.0)                # every hyper-parameter comes from the dictionary
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 0.05 and ref.param_groups[0]["nesterov"] is True
    _three_steps(a, ref, b, ours, data[3:6], "flat->torch")


def test_checkpoint_from_torch_sgd_into_flat_optimizer():
    a, b = seq_net(), seq_net()
    ref = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.8, weight_decay=1e-3, nesterov=True)
    data = batches()
    for x, y in data[:3]:
        torch_step(a, ref, x, y)
    b.load_state_dict(a.state_dict())
    ours = PO.build_optimizer(b, Cfg(OPTIMIZER="sgd", LR=1.0, MOMENTUM=0.0, WEIGHT_DECAY=0.0), max_norm=0.5, bucket_mb=0.002)
    ours.load_state_dict(ref.state_dict())
    g = ours.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.05, 0.8, 1e-3, True)
    _three_steps(a, ref, b, ours, data[3:6], "torch->flat")
    for key, value in (("dampening", 0.1), ("maximize", True)):
        bad = ref.state_dict()
        bad["param_groups"][0][key] = value
        with pytest.raises(ValueError, match=key):
            ours.load_state_dict(bad)


def test_scaler_state_round_trip():
    """scaler_state_dict() after a backoff and a growth equals GradScaler.state_dict() of the twin run; loaded into a fresh optimizer it
    continues the scale schedule identically"""
    a, b = seq_net(), seq_net()
    ref = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3)
    kw = dict(lr=0.05, momentum=0.9, max_norm=0.5, amp=True, init_scale=1024.0, growth_interval=3, bucket_mb=0.002)
    ours = FlatSGD(b, **kw)
    data = batches(10)

    def both(it, x, y, flat):
        poison = float("inf") if it == 1 else 1.0
        ref.zero_grad(set_to_none=True)
        scaler.scale(torch.nn.functional.cross_entropy(a(x), y) * poison).backward()
        scaler.unscale_(ref)
        torch.nn.utils.clip_grad_norm_(a.parameters(), 0.5)
        scaler.step(ref)
        scaler.update()
        flat.zero_grad()
        (torch.nn.functional.cross_entropy(b(x), y) * poison * flat.loss_scale()).backward()
        flat.step()

    for it, (x, y) in enumerate(data[:6]):                       # backoff at 1, growth after 2, 3, 4; tracker 1 after 5
        both(it, x, y, ours)
    mine, theirs = ours.scaler_state_dict(), scaler.state_dict()
    assert mine == theirs and mine["scale"] == 1024.0 and mine["_growth_tracker"] == 1, (mine, theirs)
    # an empty dictionary is a disabled scaler's: everything stays as constructed
    other = FlatSGD(seq_net(), **kw)
    other.load_scaler_state_dict({})
    assert other.scaler_state_dict()["scale"] == 1024.0
    assert FlatSGD(seq_net(), lr=0.1, bucket_mb=0.002).scaler_state_dict() == {}
    # the loaded optimizer continues the schedule on b's twin: same scale as the GradScaler after every further step
    c = seq_net()
    c.load_state_dict(b.state_dict())
    cont = FlatSGD(c, **{**kw, "init_scale": 4.0, "growth_interval": 1000})
    cont.load_scaler_state_dict(mine)
    cont.load_state_dict(ours.state_dict())
    assert cont.scaler_state_dict() == theirs
    for it, (x, y) in enumerate(data[6:], start=6):
        ref.zero_grad(set_to_none=True)
        scaler.scale(torch.nn.functional.cross_entropy(a(x), y)).backward()
        scaler.unscale_(ref)
        torch.nn.utils.clip_grad_norm_(a.parameters(), 0.5)
        scaler.step(ref)
        scaler.update()
        cont.zero_grad()
        (torch.nn.functional.cross_entropy(c(x), y) * cont.loss_scale()).backward()
        cont.step()
        assert float(cont.state[0]) == scaler.get_scale(), it
        close(a, c, ("continued", it))
    assert cont.scaler_state_dict() == scaler.state_dict()


def test_the_reference_trainers_checkpoint_loads():
    """optimizer_state / scaler_state of tests/golden/ckpt_minkunet_ms_ref.pth (written by the reference's trainer code over its own
    MinkUNetMs): hyper-parameters adopted - nesterov True among them -, momentum buckets zero, one step on synthetic gradients equal to
    torch.optim.SGD loaded from the same dictionary"""
    from taseg_amd.data.synthetic import fill_parameters, make_model_cfg
    from taseg_amd.pcseg.model import build_network
    ck = torch.load(os.path.join(GOLDEN, "ckpt_minkunet_ms_ref.pth"), map_location="cpu", weights_only=False)
    cfg = make_model_cfg("MinkUNetMs", in_dim=5, cr=0.125, num_layer=[1] * 8)
    a = fill_parameters(build_network(cfg, 20), seed=11).cuda()
    b = fill_parameters(build_network(cfg, 20), seed=11).cuda()
    ours = PO.build_optimizer(b, Cfg(OPTIMIZER="sgd", LR=1.0, MOMENTUM=0.5, WEIGHT_DECAY=0.0))
    ours.load_state_dict(ck["optimizer_state"])
    ours.flat.load_scaler_state_dict(ck["scaler_state"])
    assert len(ours.param_groups) == 1
    g = ours.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.24, 0.9, 1e-4, True)
    assert g["initial_lr"] == 0.24                              # what the reference's scheduler had added travels along
    assert all(float(bk["mflat"].abs().sum()) == 0 for bk in ours.flat.reducer.buckets)
    assert float(ours.flat.loss_scale()) == 1.0
    ref = torch.optim.SGD(a.parameters(), lr=1.0)
    ref.load_state_dict(ck["optimizer_state"])
    gen = torch.Generator().manual_seed(4)
    ours.zero_grad()
    for pa, pb in zip(a.parameters(), b.parameters()):
        grad = (torch.randn(pa.shape, generator=gen) * 0.01).cuda()
        pa.grad, pb.grad = grad.clone(), grad.clone()
    ref.step()
    ours.step()
    moved = 0
    for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
        assert torch.allclose(pa, pb, rtol=RTOL, atol=ATOL), (i, float((pa - pb).abs().max()))
        assert torch.allclose(ref.state[pa]["momentum_buffer"], ours.state[pb]["momentum_buffer"], rtol=RTOL, atol=ATOL), i
        moved += int(float(ours.state[pb]["momentum_buffer"].abs().sum()) > 0)
    assert moved == len(list(b.parameters()))


def test_a_parameter_without_gradient_keeps_its_bits():
    """a head no loss reaches: over three steps its parameters AND its momentum (made non-zero first) keep their bits, every other
    parameter follows the torch twin"""
    class WithHead(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(1)
            self.body = torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.ReLU(), torch.nn.Linear(40, 7))
            self.unused_head = torch.nn.Linear(40, 5000)          # more than a tile: the kernel's whole-tile skip too

        def forward(self, x):
            return self.body(x)

    a, b = WithHead().cuda(), WithHead().cuda()
    ref = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2)
    ours = FlatSGD(b, lr=0.05, momentum=0.9, weight_decay=1e-2, max_norm=0.5, bucket_mb=0.002)
    head = list(b.unused_head.parameters())
    for p in head:
        ours._momentum_of[id(p)].normal_()
    before = [(p.detach().clone(), ours._momentum_of[id(p)].clone()) for p in head]
    for it, (x, y) in enumerate(batches(3)):
        torch_step(a, ref, x, y)
        flat_step(b, ours, x, y)
        close(a.body, b.body, it)
        for p, (p0, m0) in zip(head, before):
            assert same_bits(p.detach(), p0) and same_bits(ours._momentum_of[id(p)], m0), it
