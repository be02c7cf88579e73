"""Float64 reference of the CE + Lovasz loss kernels (csrc/loss.hip), stage by stage - test infrastructure, not product code.

Written from the formulas of include/taseg_hip.h (ts_lovasz_errors, ts_lovasz_grad, ts_softmax_ce_forward, ts_ce_lovasz_finish,
ts_ce_lovasz_backward) and the docstrings of taseg_amd/pcseg/loss/lovasz.py, in torch CPU float64, with no autograd and none of
torch's loss functions.  The Lovasz stage takes the sort permutation as an INPUT: the Lovasz gradient is piecewise constant in the
order of the errors, so a test hands it the order the device sort produced and checks separately that this order is a valid
descending order of the float64 errors.  tests/test_loss_host.py checks this file against oracle.model.loss_ce_lovasz under autograd
in double; tests/test_gpu_loss_float64.py checks the kernels against this file.

`ignore` is an integer label value or None (nothing is ignored).  Rows with the ignored label keep their place with zero error and
zero foreground, as in the kernels: the value equals that of dropping them.
"""
import torch

ROWS = 256          # rows of one partial sum of ts_softmax_ce_forward


def _valid(labels, ignore):
    labels = labels.reshape(-1).long()
    return torch.ones_like(labels, dtype=torch.bool) if ignore is None else labels != int(ignore)


def softmax64(logits):
    """(probas, logp) [P, C] in float64 from the exact values of the logits."""
    x = logits.double()
    x = x - x.max(dim=1, keepdim=True).values
    lse = x.exp().sum(dim=1, keepdim=True).log()
    logp = x - lse
    return logp.exp(), logp


def errors64(probas, labels, ignore):
    """errors [C, P] = |(labels == c) - probas[p, c]| on the rows that count, 0 on the others; probas cast up unchanged."""
    pr = probas.double()
    c = pr.shape[1]
    labels = labels.reshape(-1).long()
    valid = _valid(labels, ignore)
    fg = (labels.view(1, -1) == torch.arange(c).view(-1, 1)) & valid.view(1, -1)
    return (fg.double() - pr.t()).abs() * valid.view(1, -1).double()


def partials64(logp, labels, ignore):
    """[ceil(P / 256), 3]: per block of 256 rows the sums over its rows that count of -logp[y] and of -sum_c logp_c, and their
    number.  A label that is neither ignored nor a class makes its block's first sum NaN."""
    p, c = logp.shape
    labels = labels.reshape(-1).long()
    valid = _valid(labels, ignore)
    inside = (labels >= 0) & (labels < c)
    picked = logp.gather(1, labels.clamp(0, c - 1).view(-1, 1)).view(-1)
    picked = torch.where(inside, picked, torch.full_like(picked, float("nan")))
    w = valid.double()
    cols = torch.stack([torch.where(valid, -picked, torch.zeros_like(picked)), -logp.sum(dim=1) * w, w], dim=1)
    pad = (-p) % ROWS
    if pad:
        cols = torch.cat([cols, cols.new_zeros(pad, 3)])
    return cols.view(-1, ROWS, 3).sum(dim=1)


def softmax_ce_forward64(logits, labels, ignore):
    """what ts_softmax_ce_forward writes: (probas [P, C], errors [C, P], partials [ceil(P / 256), 3])"""
    probas, logp = softmax64(logits)
    return probas, errors64(probas, labels, ignore), partials64(logp, labels, ignore)


def lovasz_from_perm64(errors_sorted, perm, labels, ignore):
    """Lovasz-softmax with classes = 'present' from a given order.  errors_sorted, perm [C, P]: the errors of every class in the order
    `perm` puts its rows in (cast up unchanged).  Returns (loss, d loss / d probas [P, C], #present, per-class dot products [C]).

    With fg the 0/1 foreground of class c in that order, gts = sum fg, cum_i = fg_0 + .. + fg_i and rank_i = i + 1:
        jaccard_i = 1 - (gts - cum_i) / (gts + rank_i - cum_i),   g_i = jaccard_i - jaccard_(i-1)   (jaccard_(-1) = 0)
        loss = mean over the classes with gts > 0 of sum_i errors_sorted_i g_i     (0 when no class has foreground)
        d loss / d probas[perm_i, c] = sign_i g_i [gts_c > 0] / #present,  sign_i = -1 on foreground, +1 elsewhere, 0 where the
        error is 0 (the derivative of |.| at 0 as torch takes it)."""
    es = errors_sorted.double()
    c, p = es.shape
    labels = labels.reshape(-1).long()
    valid = _valid(labels, ignore)
    fg = ((labels.view(1, -1) == torch.arange(c).view(-1, 1)) & valid.view(1, -1)).double()
    fgs = torch.gather(fg, 1, perm)
    gts = fgs.sum(dim=1, keepdim=True)
    cum = fgs.cumsum(dim=1)
    rank = torch.arange(1, p + 1, dtype=torch.float64).view(1, -1)
    jac = 1.0 - (gts - cum) / (gts + (rank - cum))
    g = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], dim=1)
    per_class = (es * g).sum(dim=1)
    present = (gts.view(-1) > 0).double()
    n_present = float(present.sum())
    scale = present / n_present if n_present > 0 else present * 0.0
    loss = (per_class * scale).sum()
    sign = torch.where(es > 0, 1.0 - 2.0 * fgs, torch.zeros_like(es))
    d_sorted = sign * g * scale.view(-1, 1)
    dprob = torch.zeros(c, p, dtype=torch.float64).scatter_(1, perm, d_sorted)
    return loss, dprob.t().contiguous(), n_present, per_class


def finish64(partials, n_classes, smoothing, w_ce, w_lov, lovasz):
    """out4 of ts_ce_lovasz_finish: [w_ce ce + w_lov lovasz, ce, lovasz, n]; ce = (1 - eps) nll / n + eps smooth / (n C), NaN when no
    row counts (the mean over nothing); lovasz None counts as 0."""
    s = partials.double().sum(dim=0)
    nll, smooth, n = float(s[0]), float(s[1]), float(s[2])
    nan = float("nan")
    ce = (1.0 - smoothing) * (nll / n if n else nan) + smoothing * (smooth / (n * n_classes) if n else nan)
    lov = 0.0 if lovasz is None else float(lovasz)
    return torch.tensor([w_ce * ce + w_lov * lov, ce, lov, n], dtype=torch.float64)


def backward64(probas, labels, ignore, grad_probas, n, grad_out, smoothing, w_ce, w_lov):
    """d loss / d logits [P, C] of ts_ce_lovasz_backward from given probas [P, C], d lovasz / d probas [P, C] (or None) and the
    number n of rows that count:
        go [ w_ce valid / n ((1 - eps)(p - onehot) + eps (p - 1 / C)) + w_lov p (dp - sum_c p_c dp_c) ]
    A row that does not count takes no cross-entropy term, whatever n is."""
    pr = probas.double()
    p, c = pr.shape
    labels = labels.reshape(-1).long()
    valid = _valid(labels, ignore)
    onehot = (labels.view(-1, 1) == torch.arange(c).view(1, -1)).double()
    ce = (1.0 - smoothing) * (pr - onehot) + smoothing * (pr - 1.0 / c)
    k = torch.where(valid, torch.full((p,), w_ce / n if n else 0.0, dtype=torch.float64), torch.zeros(p, dtype=torch.float64))
    out = k.view(-1, 1) * ce
    if grad_probas is not None:
        dp = grad_probas.double()
        out = out + w_lov * pr * (dp - (pr * dp).sum(dim=1, keepdim=True))
    return float(grad_out) * out


def argsort64(errors):
    """(errors_sorted, perm): a descending order of float64 errors [C, P] (stable)."""
    es, perm = torch.sort(errors, dim=1, descending=True, stable=True)
    return es, perm


def ce_lovasz64(logits, labels, ignore=0, smoothing=0.0, w_ce=1.0, w_lov=1.0, grad_out=1.0):
    """The whole chain in float64 with its own sort: (out4, d (grad_out * out4[0]) / d logits)."""
    probas, errors, partials = softmax_ce_forward64(logits, labels, ignore)
    es, perm = argsort64(errors)
    lov, dprob, _, _ = lovasz_from_perm64(es, perm, labels, ignore)
    out4 = finish64(partials, probas.shape[1], smoothing, w_ce, w_lov, lov)
    grad = backward64(probas, labels, ignore, dprob, float(out4[3]), grad_out, smoothing, w_ce, w_lov)
    return out4, grad
