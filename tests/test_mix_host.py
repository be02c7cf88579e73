"""Host side of the scan mixing (taseg_amd/data/mix.py), no GPU: `draw_omega` / `draw_mix_params` consume an
np.random.RandomState exactly as the reference's `__getitem__` consumes numpy's global generator (semantickitti_ms.py:14,
151-237; nuscenes_ms.py:16, 132-214), so the fixtures' seeds reproduce the values the reference drew
(tests/golden/make_golden_mix.py recorded them while it ran)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from taseg_amd import _lib
from taseg_amd.data import augment as A
from taseg_amd.data import mix as M


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_mix():
    return _load("multiscan_mix.npz")


@pytest.fixture(scope="module")
def g_mix_batch():
    return _load("multiscan_mix_batch.npz")


def _check(g, c, p, i=0):
    assert p.kind == g[f"{c}_kind"][i] and p.prob == g[f"{c}_prob"][i], (c, i)
    assert p.omega == tuple(g[f"{c}_omega"]), c
    if p.kind == M.LASER:
        assert p.strategy == g[f"{c}_strategy"][i] and not p.degrees
    if p.kind == M.POLAR:
        assert p.alpha == g[f"{c}_alpha"][i] and p.beta == p.alpha + np.pi
        assert p.swap == bool(g[f"{c}_swap"][i]) and p.paste == bool(g[f"{c}_paste"][i]) and p.paste


def test_draws_reproduce_the_reference(g_mix, g_mix_batch):
    kinds = set()
    for c in g_mix["cases"].tolist():
        seed = int(g_mix[f"{c}_seed"])
        if seed < 0:            # built from explicit flags / strategies: nothing was drawn
            continue
        rng = np.random.RandomState(seed)
        p = M.draw_mix_params(rng, M.draw_omega(rng))
        _check(g_mix, c, p)
        assert p.tail_all and p.instance_classes == tuple(range(1, 9))
        kinds.add((p.kind, p.swap))
    assert kinds == {(M.POLAR, False), (M.POLAR, True), (M.LASER, False)}
    # nuScenes: the partner draw behind the coin, the class list 1 .. 10, only column 3 into the rotated copies
    c = "nus_polar"
    rng = np.random.RandomState(int(g_mix[f"{c}_seed"]))
    p = M.draw_mix_params(rng, M.draw_omega(rng), dataset="nuscenes", n_partners=2)
    _check(g_mix, c, p)
    assert p.partner == g_mix[f"{c}_partner"] and not p.tail_all and p.instance_classes == tuple(range(1, 11))
    # whole batches: mix draws, then the augmentation's, sample after sample on one generator
    for c in g_mix_batch["cases"].tolist():
        rng = np.random.RandomState(int(g_mix_batch[f"{c}_seed"]))
        om = M.draw_omega(rng)
        for i in range(2):
            _check(g_mix_batch, c, M.draw_mix_params(rng, om), i)
            q = A.draw_train_params(rng)
            assert q.theta == g_mix_batch[f"{c}_theta"][i] and q.scale == g_mix_batch[f"{c}_scale"][i]
            assert q.flip == g_mix_batch[f"{c}_flip"][i] and tuple(q.translate) == tuple(g_mix_batch[f"{c}_noise"][i])


class Counting(np.random.RandomState):
    """counts the calls the draw functions make"""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def choice(self, *a, **k):
        self.calls.append("choice")
        return super().choice(*a, **k)

    def random_sample(self, *a, **k):
        self.calls.append("random")
        return super().random_sample(*a, **k)


@pytest.mark.parametrize("kw", [dict(augment="GlobalAugment"), dict(training=False), dict(augment="none", training=False),
                                dict(augment="GlobalAugment_L", dataset="semantickitti")])
def test_one_draw_when_nothing_is_mixed(kw):
    for seed in range(6):                # coins of both faces
        rng = Counting(seed)
        p = M.draw_mix_params(rng, (0.1, 2.2), **kw)
        assert p.kind == M.NONE and rng.calls == ["choice"]
        plain = np.random.RandomState(seed)
        assert p.prob == int(plain.choice(2, 1)[0])
        assert rng.random_sample() == plain.random_sample()           # the generators stand at the same place


def test_draw_counts_and_nuscenes_switches():
    seen = set()
    for seed in range(12):
        rng = Counting(seed)
        p = M.draw_mix_params(rng, (0.1, 2.2))
        assert rng.calls == {M.LASER: ["choice", "choice"], M.POLAR: ["choice", "random", "random", "random"]}[p.kind]
        assert p.kind == (M.LASER if p.prob == 1 else M.POLAR)
        if p.kind == M.POLAR:
            assert -np.pi <= p.alpha < 0 and p.paste
        for augment, kinds in (("GlobalAugment_L", {1: M.LASER, 0: M.NONE}), ("GlobalAugment_P", {1: M.NONE, 0: M.POLAR}),
                               ("GlobalAugment_LP", {1: M.LASER, 0: M.POLAR})):
            q = M.draw_mix_params(np.random.RandomState(seed), (0.1, 2.2), augment=augment, dataset="nuscenes")
            assert q.kind == kinds[q.prob]
            seen.add((augment, q.kind))
    assert len(seen) == 6
    rng = np.random.RandomState(5)
    om = M.draw_omega(rng)
    plain = np.random.RandomState(5)
    assert om == (plain.random_sample() * np.pi * 2 / 3, (plain.random_sample() + 1) * np.pi * 2 / 3)


def test_records_and_thresholds():
    assert M.laser_thresholds(0, True) == [-6.7, -13.4] and M.laser_thresholds(0, False) == [-6.7 / np.pi * 180, -13.4 / np.pi * 180]
    assert [len(t) for t in M.LASER_THRESHOLDS] == [2, 3, 4, 5]
    p = M.MixParams(kind=M.POLAR, alpha=-1.0, beta=2.0, swap=True, paste=True, omega=(0.5, 3.0), instance_classes=(3, 1))
    q = M.MixParams(kind=M.LASER, strategy=3, degrees=True)
    rec, cls, blocks = M.pack_mix([p, q, M.MixParams()], [300, 0, 5], [10, 257, 0])
    assert rec.shape == (3, M.RECORD) and rec.dtype == np.float64 and cls.shape == (3, M.MAX_CLASSES) and blocks == 2 + 2 + 1
    assert rec[0, :5].tolist() == [2, -1.0, 2.0, 1, 1] and rec[0, 5] == np.cos(0.5) and rec[0, 8] == np.sin(3.0)
    assert rec[:, 17].tolist() == [300, 0, 5] and rec[:, 18].tolist() == [10, 257, 0] and rec[:, 19].tolist() == [0, 310, 567]
    assert rec[:, 21].tolist() == [0, 2, 4] and rec[:, 22].tolist() == [2, 2, 1]
    assert cls[0, :3].tolist() == [3, 1, -1] and rec[1, 11] == 5 and rec[1, 12:17].tolist() == [-3.3, -6.6, -9.9, -13.2, -16.5]
    assert M.mix_capacity([p, q, M.MixParams()], [300, 0, 5], [10, 257, 0]) == 300 + 4 * 10 + 257 + 5
    with pytest.raises(ValueError):
        M.MixParams(instance_classes=(1, 1))
    with pytest.raises(ValueError):
        M.MixParams(instance_classes=tuple(range(17)))


def test_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    for name in ("ts_stage_mix", "ts_stage_mix_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, header), name
    assert "#define TS_MIX_RECORD %d" % M.RECORD in header and "#define TS_MIX_MAX_CLASSES %d" % M.MAX_CLASSES in header
    n_args = len(re.search(r"int ts_stage_mix\((.*?)\);", header, re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES["ts_stage_mix"][1])
