"""Host side of the mask-distillation recipe's data stage (no GPU): the draws recorded in tests/golden/kd_stage.npz replay from
RandomState(seed) in the FSA recipe's order; the two things the stage reproduces without repairing - the head of the partner's
teacher cloud and `num_points_ms_gt` counted before the clamp - are VISIBLE in the fixture (its numbers differ from the repaired
ones, so the device tests cannot pass vacuously); `multiscan_sample(canon=True)` on a tiny on-disk sequence."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from taseg_amd.data import augment as A
from taseg_amd.data import mix as M
from taseg_amd.data import semantickitti as SK
from taseg_amd.data.stage import _kitti_row
from test_semantickitti_reader import _write_tree

PARTNER = [1, 2, 0]


@pytest.fixture(scope="module")
def g_kd():
    return dict(np.load(os.path.join(GOLDEN, "kd_stage.npz"), allow_pickle=False))


def replay(g_kd, c):
    rng = np.random.RandomState(int(g_kd[f"{c}_seed"]))
    om = M.draw_omega(rng)
    mix, aug = [], []
    for _ in g_kd[f"{c}_samples"]:
        mix.append(M.draw_mix_params(rng, om))             # coin and mix first, then the augmentation
        aug.append(A.draw_train_params(rng))
    return om, mix, aug


def test_recorded_draws_replay_from_the_seed(g_kd):
    seen = set()
    for c in g_kd["cases"].tolist():
        if not bool(g_kd[f"{c}_training"]):
            assert int(g_kd[f"{c}_seed"]) == -1 and f"{c}_alpha" not in g_kd
            continue
        om, mix, aug = replay(g_kd, c)
        assert list(om) == g_kd[f"{c}_omega"].tolist()
        assert [p.kind for p in mix] == g_kd[f"{c}_kind"].tolist() and [p.prob for p in mix] == g_kd[f"{c}_prob"].tolist()
        assert [p.strategy for p in mix] == g_kd[f"{c}_strategy"].tolist()
        assert [p.alpha for p in mix] == g_kd[f"{c}_alpha"].tolist()                 # float64, exactly
        assert [p.swap for p in mix] == g_kd[f"{c}_swap"].tolist() and [p.paste for p in mix] == g_kd[f"{c}_paste"].tolist()
        assert [p.theta for p in aug] == g_kd[f"{c}_theta"].tolist() and [p.scale for p in aug] == g_kd[f"{c}_scale"].tolist()
        assert [p.flip for p in aug] == g_kd[f"{c}_flip"].tolist()
        assert [list(p.translate) for p in aug] == g_kd[f"{c}_noise"].tolist()
        seen |= {(p.kind, p.swap) for p in mix}
    assert seen == {(M.LASER, False), (M.POLAR, True), (M.POLAR, False)}


def teacher_inputs(g, g_kd, b):
    """(current scan, fused history rows the annotation rule keeps) of sample b, from the fixtures alone"""
    Tn = int(g["T"])
    if b == 2:
        return g["b0_points_t0"], np.zeros((0, 4), np.float32)
    steps_gt = g_kd["steps_gt"].tolist()
    keep = np.concatenate([np.array(_kitti_row(t - Tn, steps_gt))[g_kd[f"b{b}_canon_t{t}"].astype(np.int64)] for t in range(Tn)])
    return g[f"b{b}_points_t{Tn}"], g[f"b{b}_fused_all"][keep]


def test_num_points_ms_gt_is_counted_before_the_clamp(g_multiscan, g_kd):
    g, c = g_multiscan, "eval"
    got = g_kd[f"{c}_batch_num_points_ms_gt"].reshape(-1).tolist()
    before, after = [], []
    for b in g_kd[f"{c}_samples"].tolist():
        cur, hist = teacher_inputs(g, g_kd, b)
        before.append(len(cur) + len(hist))
        after.append(len(cur) + int((hist[:, :3] >= cur[:, :3].min(0)).all(1).sum()))
    assert got == before and got != after, (got, before, after)
    # ... while num_points_ms IS the row count after the clamp: the student's differs from the teacher's, the steps being unequal
    assert g_kd[f"{c}_batch_num_points_ms"].reshape(-1).tolist() != got
    assert g_kd["steps_gt"].tolist() != g["steps"].tolist()


def sector(pts, p):
    """the rows PolarMix swaps (include/taseg_hip.h: the yaw in float64, rounded to float32, against float32 bounds)"""
    yaw = (-np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))).astype(np.float32)
    return (yaw > np.float32(p.alpha)) & (yaw < np.float32(p.beta))


def test_partner_head_rule_is_visible_in_the_fixture(g_multiscan, g_kd):
    """a swapped sample whose partner has history: the teacher's rows before the clamp count the SAMPLE's own scan in front of the
    partner's history (semantickitti_ms_kd.py:220), not the partner's scan; a partner without history brings its own scan (:228)"""
    g = g_multiscan
    seen = []
    for c in g_kd["cases"].tolist():
        if not bool(g_kd[f"{c}_training"]):
            continue
        _, mix, _ = replay(g_kd, c)
        got = g_kd[f"{c}_batch_num_points_ms_gt"].reshape(-1).tolist()
        for i, (b, p) in enumerate(zip(g_kd[f"{c}_samples"].tolist(), mix)):
            if p.kind != M.POLAR or not p.swap:
                continue
            cur, hist = teacher_inputs(g, g_kd, b)
            pcur, phist = teacher_inputs(g, g_kd, PARTNER[b])
            own = int((~sector(cur, p)).sum() + (~sector(hist, p)).sum())
            # (the teacher's labels are 0: PolarMix pastes no instance rows into it)
            faithful = own + int(sector(cur if len(phist) else pcur, p).sum() + sector(phist, p).sum())
            repaired = own + int(sector(pcur, p).sum() + sector(phist, p).sum())
            assert got[i] == faithful, (c, b, got[i], faithful, repaired)
            seen.append((len(phist) > 0, faithful != repaired))
    assert (True, True) in seen and any(not has for has, _ in seen), seen


def test_multiscan_sample_fills_the_canon_column(tmp_path):
    rs = np.random.RandomState(4)
    raw = [np.array([30, 254, 0, 81, 252, 52], dtype=np.uint32) | (rs.randint(0, 9, 6).astype(np.uint32) << 16) for _ in range(4)]
    pred = [np.array([31, 30, 40, 81, 10, 259], dtype=np.uint32) for _ in range(4)]
    d = _write_tree(str(tmp_path), 5, [rs.rand(6, 4).astype(np.float32)] * 4, raw, [np.eye(4)] * 4)
    os.makedirs(os.path.join(d, "predictions"))
    for t, p in enumerate(pred):
        p.tofile(os.path.join(d, "predictions", f"{t:06d}.label"))
    seq = SK.KittiSequence(str(tmp_path), 5)
    steps = [0, 0, 2, 2, 2, 2, 2, 2, 2, 0, 4, 4, 4, 0, 4, 0, 2, 4, 2, 2]
    s = SK.multiscan_sample(seq, 3, 2, steps, device="cpu", pseudo_subdir="predictions", canon=True)
    assert s["deltas"] == [-2, -1] and len(s["canon"]) == len(s["pseudo"]) == 2
    for t in range(2):
        # the annotation: the class for a canonical raw id, -1 for a moving-object id (254, 252) or another alias (52)
        assert s["canon"][t].tolist() == [6, -1, 0, 19, -1, -1] and s["canon"][t].dtype.is_floating_point is False
        assert s["pseudo"][t].tolist() == [7, 6, 9, 19, 1, -1]
        assert s["labels"][t].tolist() == [6, 6, 0, 19, 1, 0]
    plain = SK.multiscan_sample(seq, 3, 2, steps, device="cpu")
    assert "canon" not in plain and [p.tolist() for p in plain["pseudo"]] == [c.tolist() for c in s["canon"]]
