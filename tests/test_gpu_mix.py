"""Scan mixing on the device (-m gpu): ts_stage_mix and the `mix=` path of the data stage against the reference's own functions
(tests/golden/multiscan_mix*.npz: `polarmix`, `lasermix_aug`, `lasermix_aug_` in the order of semantickitti_ms.py:151-237, then
`get_single_sample` + `collate_batch`), rows, labels and order bit for bit; the edges against the device rule restated in numpy
below (include/taseg_hip.h).  The one permitted difference from the reference - a row whose yaw or inclination sits at a bound -
cannot occur: the generator asserts that no fixture row is within 1e-5 rad / 1e-4 degrees of one, and the random clouds here are
generated WITHOUT such rows (nothing is excluded when results are compared)."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from taseg_amd import backend as B  # noqa: E402
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import stage as S  # noqa: E402
from test_gpu_augment import T, check_batch, kitti_scan, same_batches, same_bits  # noqa: E402


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_mix():
    return _load("multiscan_mix.npz")


@pytest.fixture(scope="module")
def g_mix_batch():
    return _load("multiscan_mix_batch.npz")


def kitti_inputs(g):
    lm, Tn = g["learning_map"], int(g["T"])
    return [{"raw": g[f"b{b}_points_t{Tn}"], "lab": lm[g[f"b{b}_rawlabels_t{Tn}"] & 0xFFFF].astype(np.int64),
             "raw_ms": g[f"b{b}_raw_data_ms"], "lab_ms": g[f"b{b}_labels_ms"].astype(np.int64)} for b in range(2)]


def same_rows(got, want_pts, want_lab, what):
    pts, lab = got
    assert lab.dtype == torch.int64 and pts.dtype == torch.float32
    same_bits(pts, np.ascontiguousarray(want_pts, dtype=np.float32), (what, "rows"))
    assert np.array_equal(lab.cpu().numpy(), np.asarray(want_lab).reshape(-1).astype(np.int64)), (what, "labels")


def case_params(g, c):
    seed = int(g[f"{c}_seed"])
    if seed >= 0:
        rng = np.random.RandomState(seed)              # tests/test_mix_host.py pins the draws to the stored ones
        return M.draw_mix_params(rng, M.draw_omega(rng))
    if c.startswith("laserdeg"):
        return M.MixParams(kind=M.LASER, strategy=int(g[f"{c}_strategy"][0]), degrees=True)
    a = float(g[f"{c}_alpha"][0])
    return M.MixParams(kind=M.POLAR, alpha=a, beta=a + np.pi, swap=bool(g[f"{c}_swap"][0]), paste=bool(g[f"{c}_paste"][0]),
                       omega=tuple(g[f"{c}_omega"]))


# ------------------------------------------------------------------------------------------------ 1. against the golden
def test_points_match_the_reference(g_multiscan, g_multiscan_nus, g_mix):
    ins = kitti_inputs(g_multiscan)
    seen = []
    for c in g_mix["cases"].tolist():
        b = int(g_mix[f"{c}_sample"])
        e, e1 = ins[b], ins[1 - b]
        p = case_params(g_mix, c)
        seen.append((p.kind, p.degrees, p.swap, p.paste))
        for key, lab in (("raw", "lab"), ("raw_ms", "lab_ms")):
            args = (T(e[key]), T(e[lab]), T(e1[key]), T(e1[lab]))
            assert {4: "raw", 5: "raw_ms"}[args[0].shape[1]] == key
            same_rows(M.mix_points(*args, p), g_mix[f"{c}_{key}"], g_mix[f"{c}_{lab}"], (c, key))
            if p.kind == M.POLAR:
                same_rows(M.polarmix_points(*args, p), g_mix[f"{c}_{key}"], g_mix[f"{c}_{lab}"], (c, key, "polarmix_points"))
            else:
                for strategy in (p.strategy, M.STRATEGIES[p.strategy]):
                    same_rows(M.lasermix_points(*args, strategy, degrees=p.degrees), g_mix[f"{c}_{key}"], g_mix[f"{c}_{lab}"],
                              (c, key, "lasermix_points"))
            if p.kind == M.LASER and not p.degrees:
                # the faithful LaserMix branch returns its input bits - for every strategy
                for k in range(4):
                    same_rows(M.lasermix_points(*args, k), e[key], e[lab], (c, key, "identity", k))
    assert set(seen) == {(M.POLAR, False, False, True), (M.POLAR, False, True, True), (M.POLAR, False, True, False),
                         (M.LASER, False, False, False), (M.LASER, True, False, False)}
    # nuScenes: classes 1 .. 10; only column 3 reaches the rotated copies (5-column rows: column 4 of the copies is 0)
    gn, c = g_multiscan_nus, "nus_polar"
    rng = np.random.RandomState(int(g_mix[f"{c}_seed"]))
    p = M.draw_mix_params(rng, M.draw_omega(rng), dataset="nuscenes", n_partners=2)
    assert p.partner == g_mix[f"{c}_partner"]
    for key, lab, cols, want, want_lab in (("xyzret", "labels", 5, "raw", "lab"), ("xyzret_ms", "labels_ms", 5, "raw_ms", "lab_ms"),
                                           ("xyzret", "labels", 4, "raw4", "lab4")):
        got = M.polarmix_points(T(gn[f"b0_{key}"][:, :cols]), T(gn[f"b0_{lab}"]), T(gn[f"b1_{key}"][:, :cols]), T(gn[f"b1_{lab}"]), p)
        same_rows(got, g_mix[f"{c}_{want}"], g_mix[f"{c}_{want_lab}"], (c, key, cols))
    inst = np.isin(gn["b1_labels_ms"], p.instance_classes)
    got_ms = M.polarmix_points(T(gn["b0_xyzret_ms"]), T(gn["b0_labels_ms"]), T(gn["b1_xyzret_ms"]), T(gn["b1_labels_ms"]), p)[0]
    assert inst.sum() and gn["b1_xyzret_ms"][inst, 4].any() and not got_ms[-2 * int(inst.sum()):, 4].any()
    assert got_ms[-3 * int(inst.sum()):-2 * int(inst.sum()), 4].any()              # the un-rotated block keeps the column


# ------------------------------------------------------------------------------------------------ 2. edges against the rule
def fma(a, b, c):
    """a * b + c with ONE rounding, element by element (exact rational arithmetic; Fraction -> float rounds correctly)"""
    return np.array([float(Fraction(float(u)) * Fraction(float(b)) + Fraction(float(w))) for u, w in zip(a, c)], dtype=np.float64)


def rotate(xyz32, omega):
    """np.dot(xyz_f32, [[c, s, 0], [-s, c, 0], [0, 0, 1]]) as dgemm computes it (a fused-multiply-add chain in k order), stored
    into float32"""
    c, s = float(np.cos(omega)), float(np.sin(omega))
    x, y, z = (xyz32[:, i].astype(np.float64) for i in range(3))
    return np.stack([fma(y, -s, x * c), fma(y, c, x * s), z], 1).astype(np.float32)


def yaw64(pts):
    return -np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))


def inc64(pts, degrees=True):
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    inc = np.arctan2(z, np.sqrt(x * x + y * y))
    return inc / np.pi * 180 if degrees else inc


def device_rule(pts1, lab1, pts2, lab2, p, keep1=None, keep2=None):
    """ts_stage_mix restated in numpy for one job (include/taseg_hip.h) -> (points, labels)"""
    if keep1 is not None:
        pts1, lab1, pts2, lab2 = pts1[keep1], lab1[keep1], pts2[keep2], lab2[keep2]
    if p.kind == M.NONE:
        return pts1.copy(), lab1.copy()
    if p.kind == M.POLAR:
        def sector(pts):
            yaw = yaw64(pts).astype(np.float32)
            return (yaw > np.float32(p.alpha)) & (yaw < np.float32(p.beta)) if p.swap else np.zeros(len(pts), dtype=bool)
        out, lab = [pts1[~sector(pts1)], pts2[sector(pts2)]], [lab1[~sector(pts1)], lab2[sector(pts2)]]
        if p.paste:
            order = np.concatenate([np.nonzero(lab2 == c)[0] for c in p.instance_classes] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
            inst = pts2[order]
            out.append(inst)
            lab.append(lab2[order])
            for omega in p.omega:
                new = np.zeros_like(inst)
                new[:, :3] = rotate(inst[:, :3], omega)
                if p.tail_all:
                    new[:, 3:] = inst[:, 3:]
                else:
                    new[:, 3:4] = inst[:, 3:4]
                out.append(new)
                lab.append(lab2[order])
        return np.concatenate(out, 0), np.concatenate(lab, 0)
    thr = M.laser_thresholds(p.strategy, p.degrees)
    b1, b2 = (sum((inc64(q, p.degrees) <= t).astype(np.int64) for t in thr) for q in (pts1, pts2))
    out, lab = [], []
    for j in range(len(thr) + 1):
        src, l, b = (pts1, lab1, b1) if j % 2 == 0 else (pts2, lab2, b2)
        out.append(src[b == j])
        lab.append(l[b == j])
    return np.concatenate(out, 0), np.concatenate(lab, 0)


ALPHA = -2.1
BOUNDS = (ALPHA, ALPHA + np.pi, -0.7)                    # every bound the edge cases use (-0.7: the empty sector's)
THRESHOLDS = sorted({t for ts in M.LASER_THRESHOLDS for t in ts})


def cloud(rng, n, cols=4, classes=20, p_inst=None):
    """n uniform random rows without a row at a bound: yaw within 1e-5 rad of a sector bound or inclination within 1e-4 degrees of a
    band threshold (left out when the cloud is MADE - under 1 % of it - nothing is excluded later)"""
    m = n + max(8, n // 50)
    pts = np.concatenate([rng.uniform(-50, 50, (m, 2)), rng.uniform(-6, 1, (m, 1)), rng.uniform(0, 1, (m, cols - 3))], 1).astype(np.float32)
    yaw, inc = yaw64(pts), inc64(pts)
    ok = np.ones(m, dtype=bool)
    for b in BOUNDS:
        ok &= np.abs(yaw - b) > 1e-5
    for t in THRESHOLDS:
        ok &= np.abs(inc - t) > 1e-4
    assert (~ok).sum() * 100 < m and ok.sum() >= n
    pts = pts[ok][:n]
    if p_inst is None:
        lab = rng.randint(0, classes, n)
    else:                                # mostly background: the exact rotation above is slow
        lab = np.where(rng.uniform(size=n) < p_inst, rng.randint(1, 9, n), 0)
    return pts, lab.astype(np.int64)


def run_jobs(jobs, keeps=None):
    """jobs [(pts1, lab1, pts2, lab2, params)] in ONE ts_stage_mix call against the rule, job by job; twice: identical bits"""
    pts = np.concatenate([q for j in jobs for q in (j[0], j[2])], 0)
    lab = np.concatenate([q for j in jobs for q in (j[1], j[3])], 0)
    n1, n2, ps = [len(j[0]) for j in jobs], [len(j[2]) for j in jobs], [j[4] for j in jobs]
    keep = None if keeps is None else T(np.concatenate([k for pair in keeps for k in pair]))
    out, out_lab, out_job, totals = B.stage_mix(T(pts), T(lab), ps, n1, n2, keep=keep)
    again = B.stage_mix(T(pts), T(lab), ps, n1, n2, keep=keep)
    totals = totals.tolist()
    assert totals == again[3].tolist() and sum(totals) <= out.shape[0] == M.mix_capacity(ps, n1, n2)
    at = 0
    for i, (j, m) in enumerate(zip(jobs, totals)):
        k1, k2 = (None, None) if keeps is None else keeps[i]
        want, want_lab = device_rule(*j, k1, k2)
        assert m == len(want), (i, m, len(want))
        same_rows((out[at:at + m], out_lab[at:at + m]), want, want_lab, ("job", i))
        assert (out_job[at:at + m] == i).all()
        at += m
    assert torch.equal(out[:at].view(torch.int32), again[0][:at].view(torch.int32)) and torch.equal(out_lab[:at], again[1][:at])


def polar(**kw):
    base = dict(kind=M.POLAR, alpha=ALPHA, beta=ALPHA + np.pi, swap=True, paste=True, omega=(0.9, 2.9))
    base.update(kw)
    return M.MixParams(**base)


def laser(k):
    return M.MixParams(kind=M.LASER, strategy=k, degrees=True)


@pytest.mark.parametrize("n1,n2", [(1, 1), (255, 1), (256, 255), (257, 256), (0, 300), (300, 0), (256, 0), (0, 0), (255, 257)])
@pytest.mark.parametrize("cols", [4, 5])
def test_row_counts_at_the_block_size(n1, n2, cols):
    rng = np.random.RandomState(100 * n1 + n2 + cols)
    a, b = cloud(rng, n1, cols), cloud(rng, n2, cols)
    run_jobs([(*a, *b, polar()), (*a, *b, polar(swap=False, tail_all=False)), (*a, *b, laser(3)), (*a, *b, laser(0)),
              (*a, *b, M.MixParams())])


def test_edges_of_the_rule():
    rng = np.random.RandomState(7)
    a, b = cloud(rng, 700, 5), cloud(rng, 900, 5)
    background = (b[0], np.zeros_like(b[1]))
    few = (b[0], np.where(np.isin(b[1], (1, 3)), b[1], 0))
    jobs = [(*a, *b, polar(alpha=-0.7, beta=-0.7)),                                  # alpha == beta: an empty sector
            (*a, *background, polar()),                                             # a partner without instance rows
            (*a, *few, polar(instance_classes=(3, 2, 1, 15))),                      # absent classes, a list out of order
            (*a, *b, polar(paste=False)), (*a, *b, polar(swap=False, paste=False)),
            (*a, *b, polar(instance_classes=())),
            (*a, *b, M.MixParams(kind=M.LASER, strategy=2))]                         # the reference's branch: the identity
    run_jobs(jobs)
    out, lab = M.lasermix_points(T(a[0]), T(a[1]), T(b[0]), T(b[1]), 2)
    same_rows((out, lab), a[0], a[1], "identity")
    # rows that do not exist (the class-step filter's byte)
    keeps = [(rng.uniform(size=700) < 0.6, rng.uniform(size=900) < 0.5) for _ in range(3)]
    run_jobs([(*a, *b, polar()), (*a, *b, laser(1)), (*a, *b, M.MixParams())], keeps)
    # 3 columns, and rows that start 4 bytes off a 16-byte boundary (the plain-load path of 4-column rows)
    run_jobs([(a[0][:, :3].copy(), a[1], b[0][:, :3].copy(), b[1], polar(tail_all=False))])
    c4, d4 = cloud(rng, 300, 4), cloud(rng, 310, 4)
    flat = torch.zeros(4 * 610 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(-1, 4)
    view.copy_(T(np.concatenate([c4[0], d4[0]])))
    assert view.data_ptr() % 16 == 4
    got = B.stage_mix(view, T(np.concatenate([c4[1], d4[1]])), [polar()], [300], [310])
    want, want_lab = device_rule(*c4, *d4, polar())
    same_rows((got[0][:len(want)], got[1][:len(want)]), want, want_lab, "unaligned rows")
    assert got[3].tolist() == [len(want)]


def test_three_kinds_in_one_call_and_many_blocks():
    rng = np.random.RandomState(11)
    a, b, c = cloud(rng, 1000, 4), cloud(rng, 513, 4), cloud(rng, 777, 4)
    run_jobs([(*a, *b, M.MixParams()), (*b, *c, laser(1)), (*c, *a, polar())])
    # 391 blocks, the last one partial: 60001 + 40003 rows
    big1, big2 = cloud(rng, 60001, 4, p_inst=0.0), cloud(rng, 40003, 4, p_inst=0.03)
    assert (60001 + 40003) % 256 and -(-(60001 + 40003) // 256) == 391
    run_jobs([(*big1, *big2, polar()), (*a, *b, laser(2))])


# ------------------------------------------------------------------------------------------------ 3. the stage
def batch_params(g, c):
    rng = np.random.RandomState(int(g[f"{c}_seed"]))
    om = M.draw_omega(rng)
    mix, aug = [], []
    for _ in range(2):
        mix.append(M.draw_mix_params(rng, om))
        aug.append(A.draw_train_params(rng))
    return mix, aug


def test_stage_with_mix_matches_the_reference(g_multiscan, g_mix_batch):
    g = g_multiscan
    steps = g["steps"].tolist()
    scans = [kitti_scan(g, 0), kitti_scan(g, 1)]
    partners = [scans[1], scans[0]]
    resident = [p.clone() for s in scans for p in s["points"]]
    kinds = set()
    for c in g_mix_batch["cases"].tolist():
        mix, aug = batch_params(g_mix_batch, c)
        kinds |= {p.kind for p in mix}
        batched = S.build_multiscan_batch(scans, 0.05, steps, aug=aug, mix=mix, partners=partners)
        check_batch(batched, g_mix_batch, f"{c}_batch_")                       # point_mask among the dense tensors
        per_sample = S.build_multiscan_batch_per_sample(scans, 0.05, steps, aug=aug, mix=mix, partners=partners)
        check_batch(per_sample, g_mix_batch, f"{c}_batch_")
        same_batches(batched, per_sample)
        same_batches(batched, S.build_multiscan_batch(scans, 0.05, steps, aug=aug, mix=mix, partners=partners))   # two runs
    assert kinds == {M.LASER, M.POLAR}
    assert all(torch.equal(a, b) for a, b in zip(resident, [p for s in scans for p in s["points"]])), "resident scans changed"


def test_stage_paths_agree_and_mix_none_is_the_old_path(g_multiscan):
    g = g_multiscan
    steps = g["steps"].tolist()
    scans = [kitti_scan(g, 0), kitti_scan(g, 1), kitti_scan(g, 0)]
    partners = [scans[1], scans[0], None]
    rng = np.random.RandomState(31)
    aug = [A.draw_train_params(rng) for _ in scans]
    mix = [M.MixParams(kind=M.LASER, strategy=1, degrees=True), M.MixParams(kind=M.POLAR, alpha=-2.5, beta=-2.5 + np.pi, swap=True,
                                                                           paste=True, omega=(0.4, 3.1)), M.MixParams()]
    for au in (aug, None):
        a = S.build_multiscan_batch(scans, 0.05, steps, aug=au, mix=mix, partners=partners)
        same_batches(a, S.build_multiscan_batch_per_sample(scans, 0.05, steps, aug=au, mix=mix, partners=partners))
        same_batches(a, S.build_multiscan_batch(scans, 0.05, steps, aug=au, mix=mix, partners=partners))
    assert a["num_points"].view(-1).tolist()[2] == scans[2]["points"][-1].shape[0]
    assert a["num_points"].view(-1).tolist()[0] != scans[0]["points"][-1].shape[0]
    # mix=None: the tensors of the call without the argument; all-NONE records give them too, through the mix path
    plain = S.build_multiscan_batch(scans, 0.05, steps, aug=aug)
    same_batches(plain, S.build_multiscan_batch(scans, 0.05, steps, aug=aug, mix=None, partners=None))
    same_batches(plain, S.build_multiscan_batch(scans, 0.05, steps, aug=aug, mix=[M.MixParams()] * 3))
    check_batch(S.build_multiscan_batch(scans[:2], 0.05, steps, mix=None), g, "batch_")
    with pytest.raises(ValueError):
        S.build_multiscan_batch(scans, 0.05, steps, mix=mix[:2], partners=partners)
    with pytest.raises(ValueError):
        S.build_multiscan_batch(scans, 0.05, steps, mix=mix, partners=[None, None, None])


# ------------------------------------------------------------------------------------------------ 4. the shared tail at its edges
EDGE_STEPS = [0, 1, 2, 1, 1, 1, 1, 1, 1, 1, 3, 1]     # classes 1 .. 8: PolarMix's instances; 9 and 11: background from every scan
NAN_MARK, ZMIN_MARK, Z_MIN = 2.0, 3.0, -7.0           # intensities no cloud() row has (theirs are below 1); cloud() has z >= -6


def edge_scans():
    """Three scan dicts whose fused rows have 5 columns: current scans of 300, 257 and 130 points, history of 251 + 249, 40 and no
    points, identity-plus-small-translation poses (none along z: a fused row keeps its z bits).  The sample boundaries fall inside
    a 64-lane wave and inside a 256-row block.  In sample 0 the current row 0 lies below everything else, outside the PolarMix
    sector; one history row has z on that minimum exactly (ZMIN_MARK in column 3), another a NaN x (NAN_MARK); both of a class
    that every scan contributes and that is no instance class."""
    rng = np.random.RandomState(5)
    scans = []
    for b, sizes in enumerate(([251, 249, 300], [40, 257], [130])):
        clouds = [cloud(rng, n, 4, classes=len(EDGE_STEPS)) for n in sizes]
        poses = [np.eye(4, dtype=np.float32) for _ in sizes]
        for t, pose in enumerate(poses):
            pose[:2, 3] = 0.05 * (t + 1), -0.03 * (t + b)
        scans.append({"points": [c[0] for c in clouds], "labels": [c[1] for c in clouds], "poses": poses, "name": f"edge{b}"})
    pts, lab = scans[0]["points"], scans[0]["labels"]
    pts[2][0], lab[2][0] = (-4.16, -9.09, Z_MIN, 0.5), 9          # yaw +2.0: outside (ALPHA, ALPHA + pi)
    pts[0][5], lab[0][5] = (-5.0, -9.0, Z_MIN, ZMIN_MARK), 9
    pts[1][7], lab[1][7] = (np.nan, 3.0, -1.0, NAN_MARK), 11
    return [{k: [T(a) for a in v] if k != "name" else v for k, v in s.items()} for s in scans]


@pytest.mark.parametrize("with_aug", [False, True])
def test_shared_tail_at_its_edges(with_aug):
    scans = edge_scans()
    mix = [polar(), laser(1), M.MixParams()]
    partners = [scans[1], scans[2], None]            # a partner with history, one without; sample 0's marked rows are in job 0 only
    aug = [A.draw_train_params(np.random.RandomState(17 + b)) for b in range(3)] if with_aug else None
    calls = []
    real = B.stage_clamp_compact

    def record(*a):
        calls.append((a, real(*a)))
        return calls[-1][1]
    B.stage_clamp_compact = record
    try:
        batched = S.build_multiscan_batch(scans, 0.05, EDGE_STEPS, aug=aug, mix=mix, partners=partners)
        assert len(calls) == 1                                       # the kernel, once per batched call
        again = S.build_multiscan_batch(scans, 0.05, EDGE_STEPS, aug=aug, mix=mix, partners=partners)
        assert len(calls) == 2
        per_sample = S.build_multiscan_batch_per_sample(scans, 0.05, EDGE_STEPS, aug=aug, mix=mix, partners=partners)
        assert len(calls) == 2                                       # the per-sample path keeps its own clamp
    finally:
        B.stage_clamp_compact = real
    same_batches(batched, per_sample)
    same_batches(batched, again)
    n_ms = batched["num_points_ms"].view(-1)
    assert int(n_ms.sum()) == batched["point_mask"].numel() == batched["targets_mapped_ms"].F.shape[0]
    assert int(batched["num_points"][2]) == 130 and int(n_ms[2]) == 130          # un-mixed, no history: its own scan
    # what the clamp was given and what it let through
    (rows, _, sample32, lo), (out, _, _, _, counts) = calls[0]
    assert rows.ndim == 2 and rows.shape[1] == 5 and rows.shape[0] > int(n_ms.sum()) and lo.shape == (3, 3)
    assert torch.equal(counts.cpu(), n_ms) and bool((sample32[1:] >= sample32[:-1]).all())
    out = out[:int(counts.sum())]
    nan_in, nan_out = torch.isnan(rows).any(1), torch.isnan(out).any(1)
    assert int(nan_in.sum()) == 1 and float(rows[nan_in][0, 3]) == NAN_MARK and int(sample32[nan_in]) == 0
    assert not bool(nan_out.any()) and not bool((out[:, 3] == NAN_MARK).any())   # the NaN row fell to the clamp
    assert not bool(torch.isnan(batched["lidar_ms"].F).any())
    edge = rows[:, 3] == ZMIN_MARK
    assert int(edge.sum()) == 1 and int(sample32[edge]) == 0
    assert torch.equal(rows[edge][0, 2].view(torch.int32), lo[0, 2].view(torch.int32))      # z exactly on the minimum ...
    assert int((out[:, 3] == ZMIN_MARK).sum()) == 1                                         # ... survives
