"""oracle/optim64.py - the float64 reference tests/test_gpu_optim_float64.py holds the SGD step kernels against - checked without a
device against torch's own code in float64: torch.optim.SGD (first step without a buffer, second with one), clip_grad_norm_ behind a
multiplication by 1 / scale, and torch.amp.GradScaler's state_dict() after scripted sequences of found-inf and clean steps.  Bar:
1e-12 relative to the largest magnitude."""
import math

import numpy as np
import pytest
import torch

from oracle import optim64 as O64

TOL = 1e-12


def _close(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("lr,momentum,wd,nesterov", [(0.1, 0.9, 1e-2, False), (0.1, 0.9, 1e-2, True), (0.24, 0.9, 1e-4, False),
                                                     (0.24, 0.9, 1e-4, True), (0.05, 0.0, 0.0, False), (0.05, 0.5, 0.0, True)])
@pytest.mark.parametrize("n", [1, 37, 300])
def test_apply64_is_torch_sgd_in_double(n, lr, momentum, wd, nesterov):
    rs = np.random.RandomState(n)
    p0 = torch.from_numpy(rs.randn(n))
    grads = [torch.from_numpy(rs.randn(n)) for _ in range(2)]
    gs = 0.37
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([param], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    p, m = p0.clone(), torch.full((n,), float("nan"), dtype=torch.float64)          # no buffer yet: m must not be read
    for it, g in enumerate(grads):
        param.grad = g * gs                                  # the clip coefficient, applied by torch in front of the step
        opt.step()
        p, m, (a, b, c) = O64.apply64(p, g, m, gs, lr, momentum, wd, int(nesterov), first=int(it == 0))
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all())
        assert _close(p, param.data), it
        if momentum:
            assert _close(m, opt.state[param]["momentum_buffer"]), it
        assert float(c.abs().max()) == 0.0 or it == 1        # first step: nothing of the buffer enters
    # a buffer of zeros behaves as no buffer (what FlatSGD relies on)
    q, mq, _ = O64.apply64(p0, grads[0], torch.zeros(n, dtype=torch.float64), gs, lr, momentum, wd, int(nesterov), first=0)
    q1, mq1, _ = O64.apply64(p0, grads[0], torch.zeros(n, dtype=torch.float64), gs, lr, momentum, wd, int(nesterov), first=1)
    assert torch.equal(q, q1) and torch.equal(mq, mq1)


def test_apply64_magnitudes():
    p, g, m = torch.tensor([2.0, -3.0]), torch.tensor([0.5, 4.0]), torch.tensor([-1.0, 8.0])
    _, _, (a, b, c) = O64.apply64(p, g, m, 0.5, 0.1, 0.25, 0.125)
    assert a.tolist() == [0.25, 2.0] and b.tolist() == [0.25, 0.375] and c.tolist() == [0.25, 2.0]


def test_apply_segments64_is_torch_sgd_with_groups_and_parameters_without_gradient():
    """three parameters in two groups (one Nesterov), the middle one without a gradient in the second step: torch.optim.SGD leaves it
    alone, weight decay and momentum included"""
    rs = np.random.RandomState(3)
    sizes, offsets = [5, 17, 33], [0, 16, 48]
    n = 96
    values = [(0.1, 0.9, 1e-2, 0), (0.03, 0.5, 1e-3, 1)]
    group_of = [0, 1, 1]
    inside = np.zeros(n, dtype=bool)
    for o, s in zip(offsets, sizes):
        inside[o:o + s] = True
    p = torch.from_numpy(rs.randn(n) * inside)
    m = torch.zeros(n, dtype=torch.float64)
    params = [torch.nn.Parameter(p[o:o + s].clone()) for o, s in zip(offsets, sizes)]
    opt = torch.optim.SGD([{"params": params[:1]},
                           {"params": params[1:], "lr": 0.03, "momentum": 0.5, "weight_decay": 1e-3, "nesterov": True}],
                          lr=0.1, momentum=0.9, weight_decay=1e-2)
    for it, unused in enumerate([(), (1,), ()]):
        g = torch.from_numpy(rs.randn(n) * inside)
        for i, q in enumerate(params):
            q.grad = None if i in unused else g[offsets[i]:offsets[i] + sizes[i]].clone() * 0.37
        opt.step()
        p_before = p.clone()
        p, m, mags = O64.apply_segments64(p, g, m, offsets, sizes, 0.37, group_of, values, unused=unused)
        for i, q in enumerate(params):
            sl = slice(offsets[i], offsets[i] + sizes[i])
            assert _close(p[sl], q.data), (it, i)
            if i in unused:
                assert torch.equal(p[sl], p_before[sl]) and float(mags["active"][sl].sum()) == 0
            else:
                assert _close(m[sl], opt.state[q]["momentum_buffer"]), (it, i)
                assert float(mags["active"][sl].min()) == 1.0 and float(mags["nesterov"][sl].min()) == float(group_of[i])
        assert float(p[~torch.from_numpy(inside)].abs().sum()) == 0 and float(m[~torch.from_numpy(inside)].abs().sum()) == 0


def test_apply_segments64_skip_rule():
    """unused != 0 and (flags is None or flags[flag_index] == 0)"""
    p, g, m = torch.ones(48), torch.ones(48), torch.zeros(48)
    kw = dict(offsets=[0, 16, 32], sizes=[16, 16, 16], gs=1.0, group_of=[0, 0, 0], group_values=[(0.5, 0.0, 0.0, 0)])
    moved = lambda q: [bool((q[i * 16:(i + 1) * 16] != 1).all()) for i in range(3)]
    assert moved(O64.apply_segments64(p, g, m, **kw)[0]) == [True, True, True]
    assert moved(O64.apply_segments64(p, g, m, unused=(0, 2), **kw)[0]) == [False, True, False]
    flags = torch.tensor([0.5, 0.0, 0.0])          # slot 0: another rank had a gradient; slot 1 has one here, its flag is not asked
    assert moved(O64.apply_segments64(p, g, m, unused=(0, 2), flags=flags, **kw)[0]) == [True, True, False]


@pytest.mark.parametrize("scale", [1.0, 65536.0, 0.125, 1000.0])
@pytest.mark.parametrize("max_norm,target", [(0.5, 3.0), (10.0, 3.0), (10.0, 1e4), (0.0, 3.0), (-1.0, 3.0)])
def test_grad_stats64_and_decide64_are_clip_grad_norm_behind_the_unscaling(scale, max_norm, target):
    rs = np.random.RandomState(7)
    shapes = [(5,), (17, 3), (301,)]
    raw = [rs.randn(*s) for s in shapes]
    k = target / math.sqrt(sum(float((r * r).sum()) for r in raw))
    grads = [torch.from_numpy(r * k * scale) for r in raw]            # the scaled gradients the kernels see
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
    inv = 1.0 / scale
    for q, g in zip(params, grads):
        q.grad = g * inv                                     # GradScaler.unscale_
    if max_norm > 0:
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    else:                                                    # the kernel's documented rule: no clipping
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(q.grad) for q in params]))
    sumsq, bad = 0.0, 0
    for g in grads:
        s, b = O64.grad_stats64(g)
        sumsq, bad = sumsq + s, bad | b
    state = [np.float32(scale), np.float32(0), 0, 0, 0, 0, 0, 0]
    new = O64.decide64(sumsq, bad, state, max_norm, 2.0, 0.5, 2000, 1)
    assert bad == 0 and new[3] == 0.0
    assert abs(new[4] - float(total)) <= TOL * float(total)
    for q, g in zip(params, grads):
        assert _close(g * new[2], q.grad)                    # state[2] multiplies the stored gradient
    if max_norm <= 0 or target < max_norm:
        assert new[2] == inv


def test_grad_stats64_edges():
    assert O64.grad_stats64(np.zeros(0, dtype=np.float32)) == (0.0, 0)
    assert O64.grad_stats64(np.array([3.0], dtype=np.float32)) == (9.0, 0)
    x = np.array([1e20, 1.0, -1e20, 1e-20], dtype=np.float32)
    want = 2 * float(np.float32(1e20)) ** 2 + 1.0 + float(np.float32(1e-20)) ** 2
    assert O64.grad_stats64(x) == (want, 0)
    for bad in (np.inf, -np.inf, np.nan):
        s, flag = O64.grad_stats64(np.array([1.0, bad, 2.0], dtype=np.float32))
        assert flag == 1 and not math.isfinite(s)
    assert O64.grad_stats64(torch.tensor([3e38, 3e38]))[1] == 0          # the squares do not overflow a double


def _scaler_run(script, init_scale, growth, backoff, interval):
    """torch.amp.GradScaler on the CPU through unscale_ / step / update with gradients that are finite or not"""
    q = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.SGD([q], lr=0.0)
    scaler = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    out = []
    for found_inf in script:
        scaler.scale(torch.zeros(()))                        # (creates the scale tensor)
        q.grad = torch.full((3,), float("inf") if found_inf else 1.0)
        scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        out.append(scaler.state_dict())
    return out


@pytest.mark.parametrize("interval", [1, 3, 2000])
@pytest.mark.parametrize("init_scale,growth,backoff", [(1024.0, 2.0, 0.5), (1000.0, 1.75, 0.375), (2.0 ** 127, 2.0, 0.5)])
def test_decide64_follows_gradscaler_update(interval, init_scale, growth, backoff):
    """factors that a float holds exactly, as the defaults 2 and 0.5 are: the kernels take growth and backoff as floats (and decide64
    their float values), torch multiplies the float scale by the Python double - for 0.3 the two differ in the last bit of the scale"""
    script = [0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    want = _scaler_run(script, init_scale, growth, backoff, interval)
    state = [np.float32(init_scale), np.float32(0), 0, 0, 0, 0, 0, 0]
    for it, found_inf in enumerate(script):
        new = O64.decide64(4.0, found_inf, state, 10.0, growth, backoff, interval, 1)
        state[:5] = new
        assert new[3] == float(found_inf)
        assert float(new[0]) == want[it]["scale"] and int(new[1]) == want[it]["_growth_tracker"], (it, new, want[it])
        assert new[0].dtype == np.float32 and new[1].dtype == np.float32
    # a non-finite sum of squares is a bad step too; without amp the schedule stands still and the scale counts as 1
    for s in (math.inf, math.nan):
        new = O64.decide64(s, 0, [np.float32(8.0), np.float32(1.0), 0, 0, 0, 0, 0, 0], 10.0, 2.0, 0.5, interval, 1)
        assert new[3] == 1.0 and float(new[0]) == 4.0 and float(new[1]) == 0.0
    new = O64.decide64(4.0, 0, [np.float32(8.0), np.float32(1.0), 0, 0, 0, 0, 0, 0], 10.0, 2.0, 0.5, interval, 0)
    assert float(new[0]) == 8.0 and float(new[1]) == 1.0 and new[4] == 2.0 and new[2] == 1.0
    new = O64.decide64(4.0, 1, [np.float32(8.0), np.float32(1.0), 0, 0, 0, 0, 0, 0], 10.0, 2.0, 0.5, interval, 0)
    assert float(new[0]) == 8.0 and float(new[1]) == 1.0 and new[3] == 1.0
