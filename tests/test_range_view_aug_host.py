"""The range-view training stage without a GPU: the host's draws (taseg_amd.data.range_view.draw_range_view_params), the bounds of the
RangeMix strategies and the numpy restatement tests/range_view_aug_ref.py against the REAL SemkittiRangeViewDataset.__getitem__ with
its augmentation on (tests/golden/range_view_aug.npz, made by tests/golden/make_golden_range_view_aug.py, which asserts every
condition relied on here).  The restatement equals the reference at every pixel that no UNDECIDED row touches (range_view_ref.
project_undecided on the augmented clouds, under either decision; at most 1 % of a case's pixels), the augmented float32 coordinates at
every row.  tests/test_gpu_range_view_aug.py holds the device to the restatement bit for bit."""
import os
import random
import zlib

import numpy as np
import pytest
import torch

import range_view_aug_ref as A
from taseg_amd.data import range_view as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = A.fixture_cases()


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "range_view_aug.npz"), allow_pickle=False))


def _aug(sw):
    return RV.RangeViewAug(*[bool(v) for v in sw[:5]], *[float(v) for v in sw[5:]])


def _draw(g, name):
    seed, index, sw, hw = CASES[name]
    clouds, labels = A.fixture_scans(g)
    rs, pyr = np.random.RandomState(seed), random.Random(seed)
    p = RV.draw_range_view_params(_aug(sw), index, len(clouds), lambda i: len(clouds[i]), rs, pyr, hw)
    return p, rs, pyr, clouds, labels, hw


@pytest.mark.parametrize("name", list(CASES))
def test_draws_leave_both_generators_where_the_reference_does(g, name):
    p, rs, pyr, clouds, _, hw = _draw(g, name)
    assert rs.random_sample() == g[name + "_next"][0] and pyr.random() == g[name + "_next"][1]
    sw = CASES[name][2]
    assert (p["partner"] is not None) == (sw[5] > 0 or sw[7] > 0 or sw[8] > 0)
    for d in (p["scan"], p["partner_scan"]):
        if d is None:
            continue
        for k, key in enumerate(("drop", "flip", "scale", "rotate", "jitter")):
            assert (d[key] is not None) == bool(sw[k]), key
        if d["drop"] is not None:
            assert np.array_equal(d["drop"], np.unique(d["drop"])) and d["drop"].max() < d["n"] - 1
        if d["scale"] is not None:
            assert d["scale"] == 1 / 1.05 or 1 <= d["scale"] < 1.05
        if d["jitter"] is not None:
            assert np.abs(d["jitter"]).max() <= 3 * 0.1
    assert p["shift"] == 0 or 100 <= p["shift"] <= hw[1] - 100


def test_the_cases_cover_both_mixtures_and_four_strategies(g):
    drawn = [_draw(g, name)[0] for name in CASES]
    assert {p["mixture"] for p in drawn} == {0, 1, 2}
    assert len({p["strategy"] for p in drawn if p["strategy"]}) >= 4
    assert any(p["union"] for p in drawn) and any(p["paste"] for p in drawn) and any(p["shift"] for p in drawn)


def test_all_switches_off_draws_what_the_reference_draws():
    """the shift draw is made whatever its probability (semantickitti_rv.py:138); nothing else, and nothing from `random`"""
    rs, pyr = np.random.RandomState(3), random.Random(3)
    p = RV.draw_range_view_params(RV.RangeViewAug(), 0, 3, lambda i: 5000, rs, pyr)
    want = np.random.RandomState(3)
    want.random_sample()
    assert rs.random_sample() == want.random_sample() and pyr.random() == random.Random(3).random()
    assert p["partner"] is None and p["shift"] == 0 and all(p["scan"][k] is None for k in ("drop", "flip", "scale", "rotate", "jitter"))


def test_union_at_zero_is_drawn_and_discarded():
    rs = np.random.RandomState(5)
    RV.draw_range_view_params(RV.RangeViewAug(range_paste=1.0), 0, 3, lambda i: 5000, rs, random.Random(5))
    want = np.random.RandomState(5)
    want.random_sample()                 # shift
    want.randint(0, 3)                   # partner
    for _ in range(4):                   # partner's shift, mix, paste, union
        want.random_sample()
    assert rs.random_sample() == want.random_sample()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_reference_outside_undecided_pixels(g, name):
    p, _, _, clouds, labels, hw = _draw(g, name)
    with_partners = p["partner"] is not None
    scan, label, aug, err = A.train_batch(clouds, labels, [p], hw, with_partners=with_partners)
    assert err == 0
    excl = A.excluded_pixels(aug, [p], hw[0], hw[1], with_partners)[0]
    assert excl.mean() <= 0.01
    bad = A.differs_from_stored(g, name, scan[0], label[0])
    print(f"{name}: excluded {int(excl.sum())} pixels of {excl.size}, differing inside them {int((bad & excl).sum())}")
    assert not (bad & ~excl).any()
    assert np.array_equal(scan[0, 5], (scan[0, 5] != 0).astype(np.float32))


@pytest.mark.parametrize("combo", list(A.STEP_COMBOS))
def test_augmented_coordinates_equal_the_reference_at_every_row(g, combo):
    cloud = g["cloud0"]
    aug = RV.RangeViewAug(*[bool(v) for v in A.STEP_COMBOS[combo]])
    p = RV.draw_range_view_params(aug, 0, 1, lambda i: len(cloud), np.random.RandomState(A.STEP_SEED), random.Random(0))
    mine, _ = A.augment_cloud(cloud, None, p["scan"])
    want = g["step_" + combo]
    assert len(mine) == len(want) and (len(mine) < len(cloud)) == bool(A.STEP_COMBOS[combo][0])
    assert np.array_equal(A.float_hash(mine[:, :3]), want)


@pytest.mark.parametrize("hw", A.MIX_SIZES)
def test_checkerboards_equal_the_references_methods(g, hw):
    h, w = hw
    la, lb = A.mix_probe(h, w)
    crcs = []
    for name in A.strategy_names():
        assert RV.mix_bounds(name, h, w) == A.bounds(name, h, w), name
        rec = RV.compose_record({"strategy": name, "mixture": 1}, h, w)
        rows, cols = A.bounds(name, h, w)
        assert rec[2] == len(rows) and rec[3] == len(cols) and list(rec[4:4 + len(rows)]) == rows and list(rec[9:9 + len(cols)]) == cols
        for mixture in (1, 2):
            crcs.append(zlib.crc32(np.ascontiguousarray(np.where(A.takes_partner(name, mixture, h, w), lb, la)).tobytes()))
    assert np.array_equal(np.array(crcs, dtype=np.uint32), g["mix_%dx%d" % (h, w)])
    if hw == (7, 203):
        assert A.bounds("col1row4", h, w)[0] == [1, 3, 3] and A.bounds("col6row4", h, w)[1] == [50, 100, 150, 200, 250]


def test_strategy_sets():
    assert len(RV.MIX_STRATEGIES["mixtureV2"]) == 17 and len(RV.MIX_STRATEGIES["mixture"]) == 7
    assert RV.RangeViewAug().strategy == "mixtureV2"
    for names in RV.MIX_STRATEGIES.values():
        assert set(names) <= set(A.strategy_names())
    rs = np.random.RandomState(1)
    p = RV.draw_range_view_params(RV.RangeViewAug(range_mix=1.0, strategy="col3row2"), 0, 2, lambda i: 100, rs, random.Random(1))
    assert p["strategy"] == "col3row2" and p["mixture"] in (1, 2)


def test_refusals():
    rs, pyr = np.random.RandomState(1), random.Random(1)
    state = rs.get_state()[1].copy()
    with pytest.raises(ValueError, match="W >= 200"):
        RV.draw_range_view_params(RV.RangeViewAug(range_shift=0.9), 0, 2, lambda i: 100, rs, pyr, (64, 199))
    for name in ("cutmix", "cutout", "mixup"):
        with pytest.raises(ValueError, match="not defined"):
            RV.draw_range_view_params(RV.RangeViewAug(range_mix=0.9, strategy=name), 0, 2, lambda i: 100, rs, pyr)
        with pytest.raises(ValueError, match="not defined"):
            RV.mix_bounds(name, 64, 512)
    with pytest.raises(ValueError):
        RV.mix_bounds("col5row5", 64, 512)
    assert np.array_equal(rs.get_state()[1], state) and pyr.random() == random.Random(1).random()       # before any draw
    with pytest.raises(ValueError, match="at least 10 rows"):
        RV.draw_range_view_params(RV.RangeViewAug(drop=True), 0, 2, lambda i: 9, rs, pyr)
    p = RV.draw_range_view_params(RV.RangeViewAug(), 0, 1, lambda i: 16, rs, pyr)
    cpu = {"points": torch.zeros(16, 4), "labels": torch.zeros(16, dtype=torch.int32), "name": "a"}
    with pytest.raises(RuntimeError, match="ROCm device"):
        RV.build_range_view_train_batch([cpu], None, [p])
    with pytest.raises(ValueError, match="at most 64"):
        RV.build_range_view_train_batch([cpu] * 33, [cpu] * 33, [p] * 33)
    with pytest.raises(ValueError, match="at most 64"):
        RV.build_range_view_train_batch([cpu] * 65, None, [p] * 65)
    with pytest.raises(ValueError, match="need the partners"):
        RV.build_range_view_train_batch([cpu], None, [dict(p, paste=True)])
