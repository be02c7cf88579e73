"""The AdamW element rule of csrc/adamw.hip written twice - numpy float32, operation for operation, and float64 - and the bars of
the first against the second.  Test infrastructure, not product code.

The rule (include/taseg_hip.h, ts_adamw_prepare / ts_adamw_apply_segments; torch.optim.AdamW's _single_tensor_adam in ATen's order):

    coefficients, in double from (lr, beta1, beta2, eps, wd) and the slot's step t, each rounded to float once
        decay = 1 - lr wd    w1 = 1 - beta1    b2 = beta2    w2 = 1 - beta2
        neg_step_size = -(lr / (1 - beta1^t))    bc2_sqrt = sqrt(1 - beta2^t)    eps
    per element
        g' = g gs
        p1 = p decay                                  (left out when wd == 0, as torch leaves out the mul_)
        d = g' - m;  m' = w1 < 0.5 ? m + w1 d : g' - d (1 - w1)                        (ATen's lerp)
        v' = b2 v + (w2 g') g'
        den = sqrt(v') / bc2_sqrt + eps
        p' = p1 + (neg_step_size m') / den

Bars of the float32 rule against the float64 rule ON THE SAME float coefficients (cast up) and the same float inputs.  u = 2^-24 is
the relative error of one float rounding, TINY = 2^-149 what one product or quotient may lose to underflow, SLACK = 1.01 covers the
second-order terms; every magnitude on the right is a float64 value:

    g'   one product                                  E_g  = u |g'| + TINY
    p1   one product (none without decay)             E_p1 = u |p1| + TINY
    d    g' carries E_g, one subtraction              E_d  = E_g + u |d|
    m'   w1 < 0.5:  the product w1 d, one addition    E_m  = w1 E_d + u |w1 d| + TINY + u |m'|
         else: 1 - w1 is exact in float (Sterbenz: w1 in [0.5, 1]), the product d (1 - w1), one subtraction
                                                      E_m  = E_g + (1 - w1) E_d + u |d (1 - w1)| + TINY + u |m'|
    v'   A = b2 v: one product; B = w2 g'^2: g' enters twice (2 u), two products (2 u); one addition of two non-negative numbers
                                                      E_v  = u A + 4 u B + u (A + B) + 3 TINY + 2 w2 |g'| TINY
    s = sqrt(v')   |sqrt a - sqrt b| <= min(|a - b| / (2 sqrt b), sqrt |a - b|), one rounding
                                                      E_s  = min(E_v / (2 sqrt v'), sqrt E_v) + u s
    q = s / bc2_sqrt                                  E_q  = E_s / bc2_sqrt + u q + TINY
    den = q + eps                                     E_den = E_q + u den                      (den >= eps > 0)
    num = neg_step_size m'                            E_num = |neg_step_size| E_m + u |num| + TINY
    r = num / den                                     E_r  = E_num / den + |num| E_den / den^2 + u |r| + TINY
    p' = p1 + r                                       E_p  = E_p1 + E_r + u |p'|

    |m'32 - m'64| <= SLACK E_m,   |v'32 - v'64| <= SLACK E_v,   |p'32 - p'64| <= SLACK E_p

Bar of a float coefficient against its double (ts_adamw_prepare against Python's arithmetic): one rounding to float, u |c|, plus
what the device's double pow may differ from the host's: OpenCL's bound for pow is 16 ulp (the device library keeps it), the host's
1 ulp, so beta^t carries at most 17 x 2^-53 beta^t, which 1 - beta^t magnifies by beta^t / (1 - beta^t); the subtraction, the
division and the square root add a few 2^-53 more (8 allowed):

    |c32 - c64| <= SLACK (u + (17 beta^t / (1 - beta^t) + 8) 2^-53) |c64| + TINY          with the larger of the two betas' terms
"""
import math

import numpy as np

U = 2.0 ** -24
D = 2.0 ** -53
TINY = 2.0 ** -149
SLACK = 1.01
POW_ULP = 17.0
F = np.float32
KEYS = ("decay", "w1", "b2", "w2", "neg_step_size", "bc2_sqrt", "eps")


def coefficients64(lr, beta1, beta2, eps, wd, t):
    """the scalars torch's _single_tensor_adam computes in Python floats at step t, and whether the decay product is made"""
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    return {"decay": 1 - lr * wd, "w1": 1 - beta1, "b2": beta2, "w2": 1 - beta2, "neg_step_size": -(lr / bc1),
            "bc2_sqrt": bc2 ** 0.5, "eps": eps, "has_decay": wd != 0}


def coefficients32(lr, beta1, beta2, eps, wd, t):
    """those, rounded to float once each"""
    c = coefficients64(lr, beta1, beta2, eps, wd, t)
    return {k: (F(v) if k != "has_decay" else v) for k, v in c.items()}


def coefficient_bars(lr, beta1, beta2, eps, wd, t):
    c = coefficients64(lr, beta1, beta2, eps, wd, t)
    amp = max(b ** t / (1 - b ** t) if b > 0 else 0.0 for b in (beta1, beta2))
    return {k: SLACK * (U + (POW_ULP * amp + 8) * D) * abs(c[k]) + TINY for k in KEYS}


def step32(p, g, m, v, gs, c):
    """one step in numpy float32, every operation rounded on its own; c: coefficients32() (or the record the kernel read)"""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    gs, decay, w1, b2, w2, nss, bc2, eps = (F(x) for x in (gs, c["decay"], c["w1"], c["b2"], c["w2"], c["neg_step_size"],
                                                              c["bc2_sqrt"], c["eps"]))
    with np.errstate(all="ignore"):
        gg = g * gs
        p1 = p * decay if c["has_decay"] else p
        d = gg - m
        if w1 < F(0.5):
            m1 = m + w1 * d
        else:
            m1 = gg - d * (F(1) - w1)
        v1 = b2 * v + (w2 * gg) * gg
        den = np.sqrt(v1) / bc2 + eps
        p2 = p1 + (nss * m1) / den
    assert p2.dtype == F and m1.dtype == F and v1.dtype == F
    return p2, m1, v1


def step64(p, g, m, v, gs, c):
    """the same rule in float64 on the same (float) coefficients and inputs, cast up; returns (p', m', v', bars) with the bars of
    the module docstring as float64 arrays {"p", "m", "v"}"""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    gs, decay, w1, b2, w2, nss, bc2, eps = (float(x) for x in (gs, c["decay"], c["w1"], c["b2"], c["w2"], c["neg_step_size"],
                                                                  c["bc2_sqrt"], c["eps"]))
    gg = g * gs
    e_g = U * np.abs(gg) + TINY
    if c["has_decay"]:
        p1 = p * decay
        e_p1 = U * np.abs(p1) + TINY
    else:
        p1, e_p1 = p, np.zeros_like(p)
    d = gg - m
    e_d = e_g + U * np.abs(d)
    if np.float32(w1) < np.float32(0.5):
        m1 = m + w1 * d
        e_m = w1 * e_d + U * np.abs(w1 * d) + TINY + U * np.abs(m1)
    else:
        m1 = gg - d * (1 - w1)
        e_m = e_g + (1 - w1) * e_d + U * np.abs(d * (1 - w1)) + TINY + U * np.abs(m1)
    a, b = b2 * v, w2 * gg * gg
    v1 = a + b
    e_v = U * np.abs(a) + 4 * U * np.abs(b) + U * (np.abs(a) + np.abs(b)) + 3 * TINY + 2 * w2 * np.abs(gg) * TINY
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(s > 0, np.minimum(e_v / (2 * s), np.sqrt(e_v)), np.sqrt(e_v)) + U * s
    q = s / bc2
    e_q = e_s / bc2 + U * q + TINY
    den = q + eps
    e_den = e_q + U * den
    num = nss * m1
    e_num = abs(nss) * e_m + U * np.abs(num) + TINY
    r = num / den
    e_r = e_num / den + np.abs(num) * e_den / den ** 2 + U * np.abs(r) + TINY
    p2 = p1 + r
    e_p = e_p1 + e_r + U * np.abs(p2)
    return p2, m1, v1, {"p": SLACK * e_p, "m": SLACK * e_m, "v": SLACK * e_v}


def adamw64(params, grads, state, lr, beta1, beta2, eps, wd, gs=1.0):
    """torch.optim.AdamW's step on lists of float64 arrays, in place; state: list of {"step", "exp_avg", "exp_avg_sq"}; a gradient
    of None skips its parameter.  The coefficients are Python floats (doubles), as torch computes them."""
    for p, g, st in zip(params, grads, state):
        if g is None:
            continue
        st["step"] += 1
        c = coefficients64(lr, beta1, beta2, eps, wd, st["step"])
        gg = g * gs
        if c["has_decay"]:
            p *= c["decay"]
        d = gg - st["exp_avg"]
        st["exp_avg"][...] = st["exp_avg"] + c["w1"] * d if c["w1"] < 0.5 else gg - d * (1 - c["w1"])
        st["exp_avg_sq"][...] = c["b2"] * st["exp_avg_sq"] + (c["w2"] * gg) * gg
        den = np.sqrt(st["exp_avg_sq"]) / c["bc2_sqrt"] + c["eps"]
        p += (c["neg_step_size"] * st["exp_avg"]) / den


def ulps64(a, b):
    """largest distance of two float64 arrays in units of the last place of the larger magnitude"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(a - b) / scale)) if a.size else 0.0


def isclose_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.int32), np.asarray(b, F).view(np.int32))


assert math.isclose(U, np.finfo(F).eps / 2)
