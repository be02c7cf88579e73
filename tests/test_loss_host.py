"""oracle/loss64.py - the float64 reference tests/test_gpu_loss_float64.py holds the loss kernels against - checked without a device:
with the permutation of its own float64 sort it must give the value of oracle.model.loss_ce_lovasz (torch's cross_entropy + the
reference's per-class Lovasz loop) on double logits and that value's autograd gradient, to 1e-12.  The inputs are small and free of
ties among the rows that count (asserted), so the gradient is unique."""
import numpy as np
import pytest
import torch

from oracle import loss64 as L64
from oracle import model as OM

TOL = 1e-12


def _case(seed, p, c, ignore, absent=True, all_ignored=False):
    rs = np.random.RandomState(seed)
    logits = torch.from_numpy(rs.randn(p, c) * 2)
    labels = torch.from_numpy(rs.randint(0, c, size=p))
    if absent:
        labels[labels == c - 1] = 1                       # the last class never occurs
    if ignore is not None and ignore not in range(c):
        labels[rs.rand(p) < 0.2] = ignore
    if all_ignored:
        labels[:] = ignore
    return logits, labels


def _tie_free(logits, labels, ignore):
    """no two rows that count share an error in any class, and none of their errors is 0: one order, one gradient"""
    _, err, _ = L64.softmax_ce_forward64(logits, labels, ignore)
    keep = torch.ones(len(labels), dtype=torch.bool) if ignore is None else labels != ignore
    e = err[:, keep]
    if e.shape[1] == 0:
        return True
    s = torch.sort(e, dim=1).values
    return bool((s[:, 1:] > s[:, :-1]).all()) and bool((s > 0).all())


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("ignore", [0, None, -100])
@pytest.mark.parametrize("p,c", [(1, 3), (37, 5), (300, 4), (523, 20)])
def test_loss64_matches_the_oracle_and_its_autograd_gradient_in_double(p, c, ignore, smoothing):
    logits, labels = _case(p * 31 + c, p, c, ignore, absent=c > 2)
    if p == 1:
        labels[0] = 1                                     # the one row counts under every `ignore`
    assert _tie_free(logits, labels, ignore)
    oracle_ignore = -1 if ignore is None else ignore      # the oracle takes a label value: one that nothing has
    a = logits.clone().requires_grad_()
    want = OM.loss_ce_lovasz(a, labels, ignore=oracle_ignore, label_smoothing=smoothing)
    (want * 3.0).backward()
    out4, grad = L64.ce_lovasz64(logits, labels, ignore, smoothing, 1.0, 1.0, grad_out=3.0)
    assert abs(float(out4[0]) - float(want)) <= TOL * max(1.0, abs(float(want)))
    assert float((grad - a.grad).abs().max()) <= TOL * max(1.0, float(a.grad.abs().max()))
    # the parts: cross entropy, Lovasz, the number of rows that count
    ce = torch.nn.functional.cross_entropy(logits, labels, ignore_index=oracle_ignore, label_smoothing=smoothing)
    lov = OM.lovasz_softmax_ref(logits.softmax(1), labels, ignore=oracle_ignore)
    assert abs(float(out4[1]) - float(ce)) <= TOL * max(1.0, abs(float(ce)))
    assert abs(float(out4[2]) - float(lov)) <= TOL
    assert float(out4[3]) == float((labels != oracle_ignore).sum())


@pytest.mark.parametrize("w_ce,w_lov", [(1.0, 0.7), (1.0, 0.0), (0.0, 1.0)])
def test_loss64_weights_against_autograd(w_ce, w_lov):
    logits, labels = _case(5, 211, 7, 0)
    assert _tie_free(logits, labels, 0)
    a = logits.clone().requires_grad_()
    ce = torch.nn.functional.cross_entropy(a, labels, ignore_index=0, label_smoothing=0.1)
    want = w_ce * ce + w_lov * OM.lovasz_softmax_ref(a.softmax(1), labels, ignore=0)
    (want * 3.0).backward()
    out4, grad = L64.ce_lovasz64(logits, labels, 0, 0.1, w_ce, w_lov, grad_out=3.0)
    assert abs(float(out4[0]) - float(want)) <= TOL * max(1.0, abs(float(want)))
    assert float((grad - a.grad).abs().max()) <= TOL * max(1.0, float(a.grad.abs().max()))
    # the NULL forms: no Lovasz term in the finish, no d lovasz / d probas in the backward
    probas, _, partials = L64.softmax_ce_forward64(logits, labels, 0)
    o = L64.finish64(partials, 7, 0.1, w_ce, w_lov, None)
    assert abs(float(o[0]) - w_ce * float(ce)) <= TOL and float(o[2]) == 0.0
    b = logits.clone().requires_grad_()
    (torch.nn.functional.cross_entropy(b, labels, ignore_index=0, label_smoothing=0.1) * w_ce * 3.0).backward()
    g = L64.backward64(probas, labels, 0, None, float(o[3]), 3.0, 0.1, w_ce, w_lov)
    assert float((g - b.grad).abs().max()) <= TOL


def test_loss64_one_class_present_and_one_valid_row():
    logits, labels = _case(9, 64, 5, 0)
    labels[:] = 3
    assert _tie_free(logits, labels, 0)
    a = logits.clone().requires_grad_()
    want = OM.loss_ce_lovasz(a, labels, ignore=0, label_smoothing=0.0)
    want.backward()
    out4, grad = L64.ce_lovasz64(logits, labels, 0, 0.0)
    assert abs(float(out4[0]) - float(want)) <= TOL and float((grad - a.grad).abs().max()) <= TOL
    labels[:] = 0
    labels[17] = 2
    a = logits.clone().requires_grad_()
    want = OM.loss_ce_lovasz(a, labels, ignore=0, label_smoothing=0.1)
    want.backward()
    out4, grad = L64.ce_lovasz64(logits, labels, 0, 0.1)
    assert float(out4[3]) == 1.0
    assert abs(float(out4[0]) - float(want)) <= TOL and float((grad - a.grad).abs().max()) <= TOL
    assert float(grad[labels == 0].abs().max()) == 0.0


@pytest.mark.parametrize("ignore", [0, -100])
def test_loss64_all_rows_ignored(ignore):
    """nothing counts: Lovasz is 0 with a zero gradient, the cross entropy is the mean over nothing (NaN, as torch's), and the
    backward formula - no row takes a cross-entropy term - stays finite"""
    logits, labels = _case(3, 300, 6, ignore, all_ignored=True)
    out4, grad = L64.ce_lovasz64(logits, labels, ignore, 0.1, 1.0, 0.7, grad_out=3.0)
    a = logits.clone().requires_grad_()
    lov = OM.lovasz_softmax_ref(a.softmax(1), labels, ignore=ignore)
    lov.backward()
    ce = torch.nn.functional.cross_entropy(logits, labels, ignore_index=ignore, label_smoothing=0.1)
    assert float(lov) == 0.0 and float(out4[2]) == 0.0 and float(out4[3]) == 0.0
    assert bool(torch.isnan(ce)) and bool(torch.isnan(out4[1])) and bool(torch.isnan(out4[0]))
    assert float(a.grad.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0


def test_loss64_takes_the_order_it_is_given():
    """a tie: two orders of the same errors give the same value and trade the two rows' gradients - the reason the device tests hand
    the reference the device's permutation"""
    logits, labels = _case(11, 40, 4, None, absent=False)
    logits = torch.cat([logits, logits])
    labels = torch.cat([labels, labels])
    probas, err, _ = L64.softmax_ce_forward64(logits, labels, None)
    es, perm = L64.argsort64(err)
    assert bool((es[:, ::2] == es[:, 1::2]).all())
    swapped = perm.view(4, -1, 2).flip(2).reshape(4, -1)
    l1, d1, _, _ = L64.lovasz_from_perm64(es, perm, labels, None)
    l2, d2, _, _ = L64.lovasz_from_perm64(es, swapped, labels, None)
    assert abs(float(l1) - float(l2)) <= TOL
    assert float((d1[:40] - d2[40:]).abs().max()) <= TOL and float((d1[40:] - d2[:40]).abs().max()) <= TOL
    assert float((d1 - d2).abs().max()) > 1e-6
