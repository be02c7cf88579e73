"""Host side of the SMSA recipe's moving-object augmentation (taseg_amd/data/moving.py), no GPU: the draw functions consume an
np.random.RandomState exactly as `static2moving` / `moving2static` and the `__getitem__` around them consume numpy's global
generator (semantickitti_ms_ms.py:152-289, :305-384), so the fixtures' seeds and statistics reproduce the values the reference
drew (tests/golden/make_golden_moving.py recorded them while it ran); the 26-class map; numpy's float32 mean in plain Python."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from taseg_amd import _lib
from taseg_amd.data import augment as A
from taseg_amd.data import mix as M
from taseg_amd.data import moving as MV
from taseg_amd.data import stage as S

RECIPE_STEPS = [0, 0, 2, 2, 2, 2, 2, 2, 2, 0, 4, 4, 4, 0, 4, 0, 2, 4, 2, 2]          # minkunet_mk34_cr10_smsa.yaml


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_mov():
    return _load("moving.npz")


@pytest.fixture(scope="module")
def g_mov_batch():
    return _load("moving_batch.npz")


def golden_table(g, n):
    return MV.MovingTable(g[f"{n}_cand"], g[f"{n}_counts"], g[f"{n}_stats"], len(g[f"{n}_fused"]))


def test_replay_of_the_two_passes(g_mov):
    g = g_mov
    kinds, centres, nan_shift = set(), set(), False
    for c in g["cases"].tolist():
        table = golden_table(g, "ab"[int(g[f"{c}_cloud"])])
        p = MV.draw_moving_params(np.random.RandomState(int(g[f"{c}_seed"])), table, int(g["maug_prob"]), *g["shift_range"].tolist())
        # one coin per candidate of each pass, in np.unique's order; the rand() values that followed
        assert [d[2] for d in p.draws] == g[f"{c}_coins"].tolist(), c
        assert [v for d in p.draws for v in d[3]] == g[f"{c}_rands"].tolist(), c
        assert [r.label for r in p.records] == g[f"{c}_moved"].tolist() and [r.kind for r in p.records] == g[f"{c}_kinds"].tolist()
        order = [d[1] for d in p.draws]
        first = [l for l in order if l & 0xFFFF in MV.STATIC_CLASSES]
        assert order == first + [l for l in order if l & 0xFFFF in MV.MOVING_CLASSES] and first == sorted(first)
        for r in p.records:
            kinds.add(r.kind)
            assert r.new_class == {**MV.STATIC_CLASSES, **MV.MOVING_CLASSES}[r.label & 0xFFFF]
            if r.kind == MV.S2M_X:
                centres.add(int(np.sign(r.center)))
                assert r.center == 0.0 or 2.0 <= abs(r.center) < 5.0
            if r.kind in (MV.S2M_X, MV.S2M_Y):
                assert 0.5 <= r.shift < 4.5
            nan_shift |= r.kind == MV.M2S and np.isnan(r.shift_x) and np.isnan(r.shift_y)
    assert kinds == {MV.S2M_X, MV.S2M_Y, MV.M2S} and centres == {-1, 0, 1} and nan_shift
    # a cloud without history, without a table or without candidates draws nothing
    rng = np.random.RandomState(5)
    state = rng.get_state()[1].copy()
    t = golden_table(g, "a")
    for table in (None, MV.MovingTable(), MV.MovingTable(t.labels, t.counts, t.stats, 0)):
        assert MV.draw_moving_params(rng, table) == MV.MovingParams()
    assert np.array_equal(state, rng.get_state()[1])


def test_replay_of_a_training_batch_with_the_partner_in_its_place(g_mov, g_mov_batch):
    g, tables = g_mov_batch, [golden_table(g_mov, "a"), golden_table(g_mov, "b")]
    kinds = set()
    for c in g["cases"].tolist():
        rng = np.random.RandomState(int(g[f"{c}_seed"]))
        om = M.draw_omega(rng)
        assert om == tuple(g[f"{c}_omega"])
        for b in range(2):
            mv, mix, pmv = MV.draw_smsa_sample(rng, om, tables[b], tables[1 - b])
            aug = A.draw_train_params(rng)
            kinds.add(mix.kind)
            assert mix.instance_classes == tuple(range(1, 9)) + tuple(range(20, 26)) and mix.tail_all
            assert [r.label for r in mv.records] == g[f"{c}_moved_{b}"].tolist()
            assert [r.label for r in pmv.records] == g[f"{c}_partner_moved_{b}"].tolist()
            # everything after the partner's draws only fits when they were taken at their place
            assert mix.kind == g[f"{c}_kind"][b] and mix.prob == g[f"{c}_prob"][b]
            if mix.kind == M.LASER:
                assert mix.strategy == g[f"{c}_strategy"][b]
            else:
                assert mix.alpha == g[f"{c}_alpha"][b] and mix.swap == bool(g[f"{c}_swap"][b]) and mix.paste
            assert aug.theta == g[f"{c}_theta"][b] and aug.scale == g[f"{c}_scale"][b] and aug.flip == g[f"{c}_flip"][b]
            assert list(aug.translate) == g[f"{c}_noise"][b].tolist()
    assert kinds == {M.LASER, M.POLAR}
    # outside training: the coin alone
    rng, ref = np.random.RandomState(3), np.random.RandomState(3)
    mv, mix, pmv = MV.draw_smsa_sample(rng, (0.1, 2.5), tables[0], tables[1], training=False)
    ref.choice(2, 1)
    assert mv == pmv == MV.MovingParams() and mix.kind == M.NONE and rng.random_sample() == ref.random_sample()


def test_draw_mix_params_keeps_its_draws():
    for seed in range(8):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        p = M.draw_mix_params(a, (0.3, 2.2))
        q = M.draw_mix_after_coin(b, M.draw_coin(b), (0.3, 2.2))
        assert p == q and a.random_sample() == b.random_sample() and p.instance_classes == tuple(range(1, 9))


def test_label_table_equals_the_recorded_map(g_mov):
    assert MV.LABEL_TABLE.dtype == np.int64 and np.array_equal(MV.LABEL_TABLE, g_mov["learning_map"])
    assert [MV.LEARNING_MAP_INV[c] for c in range(MV.NUM_CLASSES)] == g_mov["learning_map_inv"].tolist()
    assert MV.NUM_CLASSES == 26 == len(set(MV.CLASS_NAMES)) and MV.CLASS_NAMES[20:] == (
        "moving-car", "moving-bicyclist", "moving-person", "moving-motorcyclist", "moving-other-vehicle", "moving-truck")
    for c, raw in MV.LEARNING_MAP_INV.items():
        assert MV.LABEL_TABLE[raw] == c and MV.CANONICAL_CLASS[raw] == c
    assert (MV.CANONICAL_CLASS >= 0).sum() == 26
    # what the two passes write lands in the classes they are meant for
    assert [MV.CLASS_NAMES[MV.LABEL_TABLE[r]] for r in (258, 259, 31, 32)] == ["moving-truck", "moving-other-vehicle", "bicyclist",
                                                                              "motorcyclist"]


SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1000, 1023, 4097, 8191, 8192, 8193, 16384, 20000, 50001]


@pytest.mark.parametrize("n", SIZES)
def test_pairwise_mean_equals_numpy(n):
    rng = np.random.RandomState(n)
    for _ in range(20 if n < 5000 else 3):
        cloud = (rng.standard_normal((n, 4)) * rng.choice([0.01, 1.0, 40.0])).astype(np.float32)
        want = cloud[:, 1].mean()                      # the strided column of a fresh [n, 4] array, as the reference takes it
        got = MV.numpy_mean(cloud[:, 1])
        assert want.dtype == got.dtype == np.float32 and want.view(np.uint32) == got.view(np.uint32), (n, want, got)
    assert np.isnan(MV.numpy_mean(np.zeros(0, dtype=np.float32)))


def test_twenty_steps_keep_nothing_of_the_moving_classes():
    steps = MV.pad_steps(RECIPE_STEPS)
    assert len(RECIPE_STEPS) == 20 and len(steps) == 26 and steps[:20] == RECIPE_STEPS
    assert MV.pad_steps(steps) == steps
    for delta in range(-16, 0):
        row = S._kitti_row(delta, steps)
        assert len(row) == 27 and not any(row[20:]) and row[:20] == S._kitti_row(delta, RECIPE_STEPS)[:20]
    assert any(S._kitti_row(-2, steps)[:20])


def test_records_pack_per_cloud():
    a = MV.MovingParams((MV.MovingRecord((7 << 16) | 20, MV.S2M_Y, shift=1.5, new_class=259),
                         MV.MovingRecord((1 << 16) | 18, MV.S2M_X, center=-2.5, shift=3.0, new_class=258)))
    b = MV.MovingParams((MV.MovingRecord((0x8001 << 16) | 253, MV.M2S, shift_x=float("nan"), shift_y=0.25, new_class=31),))
    labels, start, rec = MV.pack_moving([a, None, b, MV.MovingParams()])
    assert labels.dtype == np.int64 and labels.tolist() == [(1 << 16) | 18, (7 << 16) | 20, (0x8001 << 16) | 253] and labels[2] >= 1 << 31
    assert start.dtype == np.int32 and start.tolist() == [0, 2, 2, 3, 3] and rec.shape == (3, MV.RECORD) and rec.dtype == np.float64
    assert rec[0].tolist()[:6] == [MV.S2M_X, -2.5, 3.0, 0.0, 0.0, 258.0] and np.isnan(rec[2, 3]) and rec[2, 4] == 0.25
    assert MV.pack_moving([None])[2].shape == (0, MV.RECORD)


def test_header_and_signatures_agree():
    header = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    for name, n_args in (("ts_stage_moving_workspace_bytes", 3), ("ts_stage_moving_stats", 18), ("ts_stage_moving_apply", 14)):
        decl = re.search(name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define TS_MOVING_RECORD (\d+)", header).group(1)) == MV.RECORD
    assert int(re.search(r"#define TS_MOVING_MAX_CANDIDATES (\d+)", header).group(1)) == S._MOVING_CAP
