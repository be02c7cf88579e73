"""tests/adamw_ref.py against torch.optim.AdamW and against itself, and the host side of the `adamw` route (no GPU).

float64 restatement against torch.optim.AdamW on float64 parameters, 8 steps, lr and beta1 changed before every step.  Both compute
the same real function with the same double coefficients; they differ in rounding only (torch's addcdiv multiplies the quotient, the
rule divides the product; torch's lerp may contract).  Per step the path to p' has 12 rounded operations, each 2^-53 relative to a
quantity no larger than |p| or the update |delta| = |p_j - p_{j-1}|; the moments carry at most 6 roundings per step into the next
step's update, so step j's update is off by at most (8 + 6 j) 2^-53 |delta_j|, and the two additions onto p by 2 x 2^-53 |p_j|:
    |p_k - p_k(torch)| <= SLACK sum_{j <= k} 2^-53 (2 |p_j| + (8 + 6 j) |delta_j|)
with p_j and delta_j taken from torch's run.  The moments are held to 6 j roundings of the running maxima of |g|, |m| and g^2, v.
"""
import numpy as np
import pytest
import torch

import adamw_ref as R


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _problem(seed=0, shapes=((5, 3), (7,), (1,))):
    rs = np.random.RandomState(seed)
    params = [rs.randn(*s) for s in shapes]
    grads = [[rs.randn(*s) * 10.0 ** rs.uniform(-4, 1) for s in shapes] for _ in range(8)]
    return params, grads


@pytest.mark.parametrize("wd", [1e-2, 0.0])
def test_float64_rule_equals_torch_adamw_in_float64(wd):
    params, grads = _problem()
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = torch.optim.AdamW(tp, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, foreach=False)
    mine = [p.copy() for p in params]
    state = [{"step": 0, "exp_avg": np.zeros_like(p), "exp_avg_sq": np.zeros_like(p)} for p in params]
    bar = [np.zeros_like(p) for p in params]
    gmax = [np.zeros_like(p) for p in params]
    worst = 0.0
    for j in range(1, 9):
        lr, beta1 = 1e-3 * (1 + 0.37 * j), (0.95 - 0.06 * j if j < 8 else 0.3)        # beta1 0.3: the other lerp branch (w1 = 0.7)
        opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr, (beta1, 0.99)
        before = [p.detach().numpy().copy() for p in tp]
        for p, g in zip(tp, grads[j - 1]):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        R.adamw64(mine, grads[j - 1], state, lr, beta1, 0.99, 1e-8, wd)
        for i, p in enumerate(tp):
            now = p.detach().numpy()
            bar[i] += R.D * (2 * np.abs(now) + (8 + 6 * j) * np.abs(now - before[i]))
            gmax[i] = np.maximum(gmax[i], np.abs(grads[j - 1][i]))
            err = np.abs(mine[i] - now)
            worst = max(worst, float((err / (R.SLACK * bar[i])).max()))
            assert (err <= R.SLACK * bar[i]).all(), (j, i, float((err / bar[i]).max()))
            st = opt.state[p]
            assert float(st["step"]) == state[i]["step"] == j
            assert (np.abs(state[i]["exp_avg"] - st["exp_avg"].numpy()) <= R.SLACK * 6 * j * R.D * gmax[i]).all(), (j, i)
            assert (np.abs(state[i]["exp_avg_sq"] - st["exp_avg_sq"].numpy()) <= R.SLACK * 6 * j * R.D * gmax[i] ** 2).all(), (j, i)
    print(f"adamw float64 rule against torch: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("beta1", [0.9, 0.3])
@pytest.mark.parametrize("wd", [1e-2, 0.0])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_float32_rule_inside_its_bars_of_the_float64_rule(beta1, wd, t):
    rs = np.random.RandomState(t)
    n = 4000
    p = (rs.randn(n) * 10.0 ** rs.uniform(-3, 1, n)).astype(np.float32)
    g = (rs.randn(n) * 10.0 ** rs.uniform(-12, 2, n)).astype(np.float32)
    m = (rs.randn(n) * 10.0 ** rs.uniform(-12, 2, n)).astype(np.float32)
    v = (rs.rand(n) * 10.0 ** rs.uniform(-24, 4, n)).astype(np.float32)
    p[:8], g[:8], m[:8], v[:8] = 0, 0, 0, 0                                    # the padding's values
    g[8:16], v[8:16] = 1e-25, 0                                                # squares that underflow
    c = R.coefficients32(3e-3, beta1, 0.999, 1e-8, wd, t)
    for gs in (1.0, 0.37):
        p32, m32, v32 = R.step32(p, g, m, v, gs, c)
        p64, m64, v64, bars = R.step64(p, g, m, v, gs, c)
        for name, a, b in (("p", p32, p64), ("m", m32, m64), ("v", v32, v64)):
            err = np.abs(a.astype(np.float64) - b)
            assert (err <= bars[name]).all(), (name, gs, float((err / bars[name]).max()))
        assert not p32[:8].any() and not m32[:8].any() and not v32[:8].any()   # 0 / eps: the padding stays zero
        assert (p32[16:] != p[16:]).mean() > 0.5                                   # (the step did something)


def test_both_lerp_branches_and_the_decay_product():
    p, g, m, v = (np.array([x], np.float32) for x in (0.7, 0.3, -0.2, 0.04))
    low = R.coefficients32(1e-3, 0.9, 0.999, 1e-8, 1e-2, 3)                    # w1 = 0.1 < 0.5
    high = R.coefficients32(1e-3, 0.3, 0.999, 1e-8, 1e-2, 3)                   # w1 = 0.7
    f = np.float32
    d = g - m
    assert R.step32(p, g, m, v, 1.0, low)[1] == m + low["w1"] * d
    assert R.step32(p, g, m, v, 1.0, high)[1] == g - d * (f(1) - high["w1"])
    assert low["w1"] < f(0.5) <= high["w1"]
    # weight_decay 0: the product is left out (and a decay of exactly 1 would give the same bits)
    none = R.coefficients32(1e-3, 0.9, 0.999, 1e-8, 0.0, 3)
    assert none["has_decay"] is False and none["decay"] == f(1)
    with_decay = R.step32(p, g, m, v, 1.0, low)[0]
    without = R.step32(p, g, m, v, 1.0, none)[0]
    assert without > with_decay
    assert R.isclose_bits(without, R.step32(p, g, m, v, 1.0, {**none, "has_decay": True})[0])
    p64 = R.step64(p, g, m, v, 1.0, none)[0]
    _, m1, v1 = R.step32(p, g, m, v, 1.0, none)
    assert abs(float(p64[0]) - (0.7 + float(none["neg_step_size"]) * float(m1[0]) / (np.sqrt(float(v1[0])) / float(none["bc2_sqrt"]) + 1e-8))) < 1e-7


def test_zero_state_continues_as_an_empty_state():
    """step 0 and zero moments (what FlatAdamW.state_dict() gives a parameter never stepped) loaded into torch.optim.AdamW continue
    with the bits of an optimizer that has no state for it"""
    torch.manual_seed(0)
    a, b = torch.nn.Linear(5, 3), torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    fresh, loaded = torch.optim.AdamW(a.parameters(), lr=1e-2), torch.optim.AdamW(b.parameters(), lr=1e-2)
    sd = loaded.state_dict()
    sd["state"] = {i: {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                   for i, p in enumerate(b.parameters())}
    loaded.load_state_dict(sd)
    for _ in range(3):
        x = torch.randn(4, 5)
        for net, opt in ((a, fresh), (b, loaded)):
            opt.zero_grad()
            net(x).square().sum().backward()
            opt.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb) and torch.equal(fresh.state[pa]["exp_avg_sq"], loaded.state[pb]["exp_avg_sq"])
        assert float(fresh.state[pa]["step"]) == float(loaded.state[pb]["step"]) == 3


def test_build_optimizer_adamw_refuses_a_host_module():
    from taseg_amd.pcseg import optim as PO
    cfg = Cfg(OPTIMIZER="adamw", LR=1e-3, WEIGHT_DECAY=1e-2, BETA1=0.9, BETA2=0.999, EPS=1e-8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PO.build_optimizer(torch.nn.Linear(3, 2), cfg)


def test_adamW_and_adam_are_still_torchs_and_adam_onecycle_raises():
    from taseg_amd.pcseg import optim as PO
    net = torch.nn.Linear(3, 2)
    assert type(PO.build_optimizer(net, Cfg(OPTIMIZER="adamW", LR=1e-3, WEIGHT_DECAY=1e-2))) is torch.optim.AdamW
    assert type(PO.build_optimizer(net, Cfg(OPTIMIZER="adam", LR=1e-3, WEIGHT_DECAY=1e-2))) is torch.optim.Adam
    with pytest.raises(NotImplementedError):
        PO.build_optimizer(net, Cfg(OPTIMIZER="adam_onecycle", LR=1e-3, WEIGHT_DECAY=1e-2))


def test_group_keys_and_checks_equal_torchs():
    """the key set of a FlatAdamW group is torch.optim.AdamW's for the installed version; _check_adamw_group refuses what torch
    refuses and what the kernels do not do"""
    from taseg_amd.optim import FlatAdamW, _check_adamw_group
    import inspect
    p = torch.nn.Parameter(torch.zeros(2))
    ref = torch.optim.AdamW([p], lr=1e-3)
    theirs = ref.state_dict()["param_groups"][0]
    sig = inspect.signature(FlatAdamW.__init__).parameters
    assert (sig["betas"].default, sig["eps"].default, sig["weight_decay"].default) == (theirs["betas"], theirs["eps"], theirs["weight_decay"])
    src = inspect.getsource(FlatAdamW.__init__)
    for key in theirs:
        assert key == "params" or f'"{key}"' in src, key
    p.grad = torch.ones(2)
    ref.step()
    assert sorted(ref.state_dict()["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    st = ref.state_dict()["state"][0]["step"]
    assert st.dtype == torch.float32 and st.dim() == 0 and st.device.type == "cpu"
    good = {k: v for k, v in theirs.items() if k != "params"}
    _check_adamw_group(good)
    for key, value, torch_too in (("lr", -1.0, True), ("eps", -1e-8, True), ("weight_decay", -0.1, True), ("betas", (1.0, 0.9), True),
                                  ("betas", (0.9, -0.1), True), ("eps", 0.0, False), ("amsgrad", True, False),
                                  ("maximize", True, False), ("decoupled_weight_decay", False, False)):
        with pytest.raises(ValueError):
            _check_adamw_group({**good, key: value})
        if torch_too:
            with pytest.raises(ValueError):
                torch.optim.AdamW([p], **{**{k: good[k] for k in ("lr", "betas", "eps", "weight_decay")}, key: value})
