"""Host side of the point augmentation (taseg_amd/data/augment.py), no GPU: the draw functions consume an
np.random.RandomState exactly as the reference consumes numpy's global generator (tools/utils/common/seg_utils.py:115-164), so
the fixtures' seeds reproduce the values the reference drew (tests/golden/make_golden_aug.py recorded them while it ran)."""
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN

from taseg_amd.data import augment as A

CASES_NUS = ("nus_s3", "single_s2")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_aug():
    return _load("multiscan_aug.npz")


@pytest.fixture(scope="module")
def g_aug_misc():
    return _load("multiscan_aug_misc.npz")


@pytest.fixture(scope="module")
def g_aug_tta():
    return _load("multiscan_aug_tta.npz")


def _check_case(g, c, switches):
    flip, scale, jitter, rotate = switches
    rng = np.random.RandomState(int(g[f"{c}_seed"]))
    n = len(g[f"{c}_samples"])
    for i in range(n):
        p = A.draw_train_params(rng, flip=flip, scale=scale, jitter=jitter, rotate=rotate)
        assert (p.rotate_on, p.scale_on, p.flip_on, p.translate_on) == (rotate, scale, flip, jitter)
        assert p.theta == g[f"{c}_theta"][i] and p.scale == g[f"{c}_scale"][i] and p.flip == g[f"{c}_flip"][i], (c, i)
        assert tuple(p.translate) == tuple(g[f"{c}_noise"][i]), (c, i)
        assert p.c == np.cos(g[f"{c}_theta"][i]) and p.s == np.sin(g[f"{c}_theta"][i])


def test_training_draws_reproduce_the_reference(g_aug, g_aug_misc):
    flips = []
    for c in g_aug["cases"].tolist():
        _check_case(g_aug, c, tuple(bool(v) for v in g_aug[f"{c}_switches"]))
        if g_aug[f"{c}_switches"][0]:
            flips += g_aug[f"{c}_flip"].tolist()
    assert set(flips) == {0, 1, 2, 3}                       # the fixture covers every flip type
    for c in g_aug_misc["cases"].tolist():
        _check_case(g_aug_misc, c, tuple(bool(v) for v in g_aug_misc[f"{c}_switches"]))
    for c in CASES_NUS:
        _check_case(g_aug_misc, c, (True, True, True, True))


def test_tta_draws_and_angle_table(g_aug_tta):
    g = g_aug_tta
    assert A.TTA_ANGLES == (0, 1, -1, 2, -2, 6, -6, 7, -7, 8)
    rng = np.random.RandomState(int(g["tta_seed"]))
    lo, hi = g["tta_votes"].tolist()
    assert (lo, hi) == (0, 10)
    for i, v in enumerate(range(lo, hi)):
        p = A.draw_tta_params(rng, v)
        assert p.theta == A.TTA_ANGLES[v] * np.pi / 8.0 == g["tta_theta"][i]
        assert p.scale == g["tta_scale"][i] and 0.9 <= p.scale <= 1.1
        assert (p.rotate_on, p.scale_on, p.flip_on, p.translate_on) == (True, True, False, False)
        assert p.flip == 0 and tuple(p.translate) == (0.0, 0.0, 0.0)
    # one uniform per vote and nothing else
    want = np.random.RandomState(int(g["tta_seed"]))
    for _ in range(lo, hi):
        want.uniform(0.9, 1.1)
    assert rng.uniform() == want.uniform()


def test_switched_off_steps_consume_no_draws():
    rng = np.random.RandomState(5)
    before = rng.get_state()
    p = A.draw_train_params(rng, flip=False, scale=False, jitter=False, rotate=False)
    after = rng.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert p.bits == 0 and p == A.AugParams()
    # every subset of the switches: the draws that remain come in the reference's order, from the generator's first values
    for mask in range(16):
        rotate, scale, flip, jitter = bool(mask & 1), bool(mask & 2), bool(mask & 4), bool(mask & 8)
        got = A.draw_train_params(np.random.RandomState(9), flip=flip, scale=scale, scale_range=(0.8, 1.3), jitter=jitter,
                                  rotate=rotate)
        ref = np.random.RandomState(9)
        if rotate:
            assert got.theta == ref.uniform(0, 2 * np.pi)
        if scale:
            assert got.scale == ref.uniform(0.8, 1.3)
        if flip:
            assert got.flip == int(ref.choice(4, 1)[0])
        if jitter:
            assert got.translate == tuple(float(ref.normal(0, 0.1, 1)[0]) for _ in range(3))
        assert got.bits & 15 == mask
        # numpy scales a float32 cloud in float32 unless the rotation has made it float64 first
        assert bool(got.bits & A.SCALE_F32) == (scale and not rotate)


def test_records():
    p = A.AugParams(c=0.5, s=-0.25, scale=1.05, flip=3, translate=(0.1, -0.2, 0.3), rotate_on=True, scale_on=True, flip_on=True,
                    translate_on=True)
    rec = A.pack_params([A.AugParams(), p])
    assert rec.dtype == np.float64 and rec.shape == (2, 8)
    assert rec[0].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert rec[1].tolist() == [0.5, -0.25, 1.05, 0.1, -0.2, 0.3, 15.0, 3.0]
    assert A.pack_params(rec) is rec and A.pack_params(p).shape == (1, 8)
    with pytest.raises(TypeError):
        A.pack_params([])
    with pytest.raises(TypeError):
        A.pack_params([(1.0, 0.0)])


def test_header_record_width_matches_the_host_records():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    assert "#define TS_AUG_RECORD 8" in text and len(A.AugParams().record()) == 8
    from taseg_amd import _lib
    assert "ts_stage_augment" in _lib.SIGNATURES


def test_stage_functions_take_aug():
    from taseg_amd.data import nuscenes as N
    from taseg_amd.data import stage as S
    for fn in (S.build_multiscan_batch, S.build_multiscan_batch_per_sample, S.voxelize_sample, S.voxelize_sample_ms,
               N.build_nuscenes_batch, N.build_nuscenes_batch_per_sample):
        assert inspect.signature(fn).parameters["aug"].default is None, fn.__name__
    for fn in (S.build_tta_batch, N.build_tta_batch):
        assert list(inspect.signature(fn).parameters)[:4] == [list(inspect.signature(fn).parameters)[0], "votes_min", "votes_max", "rng"]
    with pytest.raises(ValueError):
        S._aug_records([A.AugParams()], 2)


def test_cpu_tensors_fail_loudly():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.augment_points(torch.zeros((4, 4)), A.AugParams())
