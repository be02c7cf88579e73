"""The mask-distillation recipe's three-cloud data stage on the device (-m gpu): ts_stage_layout_pair (csrc/kd_stage.hip) against
its rule restated in numpy below and against the sequence it replaces (ts_stage_keep_flags -> nonzero -> searchsorted ->
ts_stage_layout, once per cloud), bit for bit; `build_kd_batch` (taseg_amd/data/kd.py) against the reference's own dataset code
(tests/golden/kd_stage.npz: `SemantickittiMsKdDataset.__getitem__`, then `get_single_sample` + `collate_batch` of
semantickitti_voxel_ms_kd.py), every key of every case bit for bit, and against the two `build_multiscan_batch` calls it replaces."""
import os
from itertools import accumulate

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from taseg_amd import backend as B  # noqa: E402
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import kd as KD  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import stage as S  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg  # noqa: E402
from test_gpu_augment import BATCH_DENSE, BATCH_SPARSE, T, check_batch, kitti_scan, same_batches  # noqa: E402

COLS = 6                     # five classes and the column of a negative class
NEG = COLS - 1


@pytest.fixture(scope="module")
def g_kd():
    return dict(np.load(os.path.join(GOLDEN, "kd_stage.npz"), allow_pickle=False))


# ------------------------------------------------------------------------------------------------ 1. the kernel against its rule
def make_inputs(seed, n_cur, scan_lengths, extreme=False):
    """n_cur[b] current rows and scan_lengths[b] = the lengths of sample b's history scans; random classes (some negative), unequal
    random tables, history spread wider than the current scans so that the clamp drops rows.  extreme: the first sample's scans pass
    rule A for every class and rule B for none, the last sample's the reverse, and nothing is clamped."""
    rng = np.random.RandomState(seed)
    nb = len(n_cur)
    lengths = [n for per in scan_lengths for n in per]
    sample_of_scan = np.array([b for b, per in enumerate(scan_lengths) for _ in per], dtype=np.int64)
    n_hist, n_scans = sum(lengths), max(len(lengths), 1)
    cur = (rng.standard_normal((sum(n_cur), 5)) * 10).astype(np.float32)          # stride 5: column 4 is not read
    cur_lab = rng.randint(0, 20, sum(n_cur)).astype(np.int64)
    hist = (rng.standard_normal((n_hist, 4)) * 14).astype(np.float32)
    hist_lab = rng.randint(0, 20, n_hist).astype(np.int64)
    scan = np.repeat(np.arange(len(lengths)), np.array(lengths, dtype=np.int64)).astype(np.int32)
    cls_a = rng.randint(-1, COLS - 1, n_hist).astype(np.int64)
    cls_b = np.where(rng.random_sample(n_hist) < 0.8, cls_a, rng.randint(-1, COLS - 1, n_hist)).astype(np.int64)
    table_a = rng.random_sample((n_scans, COLS)) < 0.6
    table_b = rng.random_sample((n_scans, COLS)) < 0.6
    table_a[::2, NEG], table_b[::2, NEG] = True, False                           # a negative class is looked up in column NEG
    if len(lengths) == 0:
        sample_of_scan = np.zeros(1, dtype=np.int64)
    start = list(accumulate(n_cur, initial=0))
    lo = np.stack([cur[a:b, :3].min(0) for a, b in zip(start[:-1], start[1:])]).astype(np.float32)
    if extreme:
        lo[:] = -1e30
        first, last = sample_of_scan == 0, sample_of_scan == nb - 1
        table_a[first], table_b[first], table_a[last], table_b[last] = True, False, False, True
    elif n_hist >= 200:
        # in the first sample and in the last one (the rows counted from the end)
        s = sample_of_scan[scan]
        for eq, nan, below in ((7, 11, 13), (n_hist - 8, n_hist - 12, n_hist - 14)):
            hist[eq, :3] = lo[s[eq]]                    # a row equal to the minimum: kept
            hist[nan, 0] = np.nan                       # NaN fails the comparison
            hist[below, :3] = lo[s[below]]
            hist[below, 2] = np.nextafter(hist[below, 2], np.float32(-np.inf))   # one ulp below in z: dropped
            for i in (eq, nan, below):
                cls_a[i] = cls_b[i] = 0
                table_a[scan[i], 0] = table_b[scan[i], 0] = True
    return dict(cur=cur, cur_lab=cur_lab, cur_start=np.array(start, dtype=np.int64), hist=hist, hist_lab=hist_lab, scan=scan,
                cls_a=cls_a, cls_b=cls_b, table_a=table_a, table_b=table_b, sample_of_scan=sample_of_scan, lo=lo, n_cur=list(n_cur))


def pair_rule(d):
    """ts_stage_layout_pair restated in numpy (include/taseg_hip.h) -> (rows A, labels A, sample A, is-current A, rows B, sample B,
    counts [B, 3])"""
    nb = len(d["n_cur"])
    s = d["sample_of_scan"][d["scan"]] if len(d["scan"]) else np.zeros(0, dtype=np.int64)

    def step(table, cls):
        c = np.where(cls < 0, NEG, cls)
        return table[d["scan"], c] if len(cls) else np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore"):
        inside = (d["hist"][:, :3] >= d["lo"][s]).all(1)
    step_a, step_b = step(d["table_a"], d["cls_a"]), step(d["table_b"], d["cls_b"])
    keep_a, keep_b = step_a & inside, step_b & inside
    counts = np.array([[(keep_a & (s == b)).sum(), (keep_b & (s == b)).sum(), (step_b & (s == b)).sum()] for b in range(nb)],
                      dtype=np.int64)
    out = []
    for keep in (keep_a, keep_b):
        rows, lab, smp, is_cur = [], [], [], []
        for b in range(nb):
            a, e = d["cur_start"][b], d["cur_start"][b + 1]
            k = keep & (s == b)
            rows += [np.concatenate([d["cur"][a:e, :4], np.ones((e - a, 1), np.float32)], 1),
                     np.concatenate([d["hist"][k], np.zeros((int(k.sum()), 1), np.float32)], 1)]
            lab += [d["cur_lab"][a:e], d["hist_lab"][k]]
            smp.append(np.full(e - a + int(k.sum()), b, dtype=np.int64))
            is_cur += [np.ones(e - a, dtype=bool), np.zeros(int(k.sum()), dtype=bool)]
        out.append((np.concatenate(rows), np.concatenate(lab), np.concatenate(smp), np.concatenate(is_cur)))
    (ra, la, sa, ia), (rb, _, sb, _) = out
    return ra, la, sa, ia, rb, sb, counts


def run_pair(d):
    (pa, la, ba, ba32, ia), (pb, bb, bb32), counts = B.stage_layout_pair(
        T(d["cur"]), T(d["cur_lab"]), T(d["cur_start"]), T(d["hist"]), T(d["hist_lab"]), T(d["scan"]), T(d["cls_a"]), T(d["cls_b"]),
        T(d["table_a"]), T(d["table_b"]), T(d["sample_of_scan"]), T(d["lo"]), neg_col=NEG)
    cap = len(d["cur"]) + len(d["hist"])
    assert pa.shape == pb.shape == (cap, 5) and counts.shape == (len(d["n_cur"]), 3) and counts.dtype == torch.int64
    counts = counts.cpu().numpy()
    na, nb_ = len(d["cur"]) + int(counts[:, 0].sum()), len(d["cur"]) + int(counts[:, 1].sum())
    assert na <= cap and nb_ <= cap
    got = [pa[:na], la[:na], ba[:na], ba32[:na], ia[:na], pb[:nb_], bb[:nb_], bb32[:nb_]]
    return [t.cpu().numpy() for t in got] + [counts]


def bits_equal(a, b):
    """float32 arrays: the same bits (a NaN row included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_rule(d, what):
    pa, la, ba, ba32, ia, pb, bb, bb32, counts = run_pair(d)
    ra, rl, rs, ri, rb, rsb, rcounts = pair_rule(d)
    assert np.array_equal(counts, rcounts), (what, "counts", counts.tolist(), rcounts.tolist())
    assert bits_equal(pa, ra) and bits_equal(pb, rb), (what, "rows")
    assert np.array_equal(la, rl), (what, "labels")
    assert np.array_equal(ba, rs) and np.array_equal(ba32, rs.astype(np.int32)) and ba32.dtype == np.int32, (what, "sample A")
    assert np.array_equal(bb, rsb) and np.array_equal(bb32, rsb.astype(np.int32)) and bb32.dtype == np.int32, (what, "sample B")
    assert ia.dtype == np.bool_ and np.array_equal(ia, ri), (what, "is-current")
    return counts


def split(n_hist, parts):
    """n_hist rows over `parts` scans (the first ones one row longer)"""
    return [n_hist // parts + (1 if i < n_hist % parts else 0) for i in range(parts)] if n_hist else []


@pytest.mark.parametrize("n_hist", [0, 1, 255, 256, 257, 513])
def test_layout_pair_one_sample_matches_the_rule(n_hist):
    d = make_inputs(100 + n_hist, [301], [split(n_hist, 3)])
    counts = check_against_rule(d, n_hist)
    if n_hist >= 200:
        assert 0 < counts[0, 0] < n_hist and 0 < counts[0, 1] <= counts[0, 2] < n_hist and counts[0, 0] != counts[0, 1]
        s = pair_rule(d)
        assert any(bits_equal(r[:3], d["lo"][0]) for r in s[0][301:]), "the row equal to the minimum is kept"


@pytest.mark.parametrize("n_hist", [0, 1, 255, 256, 257, 513, 256 * 257 + 1])
def test_layout_pair_three_samples_the_middle_one_without_history(n_hist):
    # sample 0: half of the rows in two scans; sample 1: none; sample 2: the rest in two scans - more than one block of current
    # rows too, and an odd number of them.  256 * 257 + 1 rows are 258 blocks: every thread of both clouds' scans owns two block
    # counts, the last chunks partial or empty
    d = make_inputs(200 + n_hist, [257, 130, 401], [split(n_hist // 2, 2), [], split(n_hist - n_hist // 2, 2)])
    counts = check_against_rule(d, n_hist)
    assert not counts[1].any()
    if n_hist >= 200:
        rows = pair_rule(d)[0]
        assert any(bits_equal(r[:3], d["lo"][2]) for r in rows[-(counts[2, 0]):]), "the last sample's row equal to its minimum is kept"


def test_layout_pair_a_nan_minimum_fails_every_row_of_its_sample():
    """a NaN on the OTHER side of the comparison: the samples whose minimum holds one keep no history row in either cloud, while
    the count before the clamp does not look at the minimum"""
    d = make_inputs(77, [90, 257, 40], [split(300, 2), split(400, 3), split(260, 2)])
    d["lo"][0, 2] = np.nan
    d["lo"][2, 0] = np.nan
    counts = check_against_rule(d, "nan lo")
    assert counts[0].tolist()[:2] == [0, 0] and counts[2].tolist()[:2] == [0, 0] and counts[0, 2] > 0 and counts[2, 2] > 0
    assert counts[1, 0] > 0 and counts[1, 1] > 0


def test_layout_pair_sixty_four_samples_a_wave_spans_many():
    rng = np.random.RandomState(5)
    d = make_inputs(64, rng.randint(1, 4, 64).tolist(), [[int(rng.randint(1, 4))] for _ in range(64)])
    d["lo"][:] = np.minimum(d["lo"], -20)                 # (one-row scans: keep the clamp from dropping nearly everything)
    counts = check_against_rule(d, 64)
    assert (counts[:, 0] > 0).sum() > 20 and (counts[:, 1] > 0).sum() > 20


def test_layout_pair_all_rows_to_one_cloud_only():
    d = make_inputs(9, [100, 50, 70], [split(300, 2), split(200, 1), split(281, 3)], extreme=True)
    counts = check_against_rule(d, "extreme")
    assert counts[0].tolist() == [300, 0, 0] and counts[2].tolist() == [0, 281, 281]


def test_layout_pair_equals_the_sequence_it_replaces_and_repeats_its_bits():
    d = make_inputs(33, [257, 130, 401], [split(700, 3), [], split(513, 2)])
    first, second = run_pair(d), run_pair(d)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and (bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b)), "two runs, other bits"
    pa, la, ba, ba32, ia, pb, bb, bb32, counts = first
    nb = len(d["n_cur"])
    cur_b = S.rows_index(d["n_cur"], torch.device("cuda"))
    cur_ms = torch.cat([T(d["cur"])[:, :4], torch.ones((len(d["cur"]), 1), device="cuda")], 1)
    hist_ms = torch.cat([T(d["hist"]), torch.zeros((len(d["hist"]), 1), device="cuda")], 1)
    for cls, table, want, col in ((d["cls_a"], d["table_a"], (pa, la, ba, ba32, ia), 0), (d["cls_b"], d["table_b"], (pb, None, bb, bb32, None), 1)):
        keep, hist_b = B.stage_keep_flags(hist_ms, T(d["scan"]), T(cls), T(table), T(d["sample_of_scan"]), T(d["lo"]), neg_col=NEG)
        idx = keep.nonzero().squeeze(1)
        kept_start = torch.searchsorted(hist_b[idx], torch.arange(nb + 1, device="cuda"))
        got = B.stage_layout(cur_ms, T(d["cur_lab"]), cur_b, hist_ms, T(d["hist_lab"]), hist_b, idx, T(d["cur_start"]), kept_start)
        assert (kept_start[1:] - kept_start[:-1]).cpu().numpy().tolist() == counts[:, col].tolist()
        for g, w in zip(got, want):
            if w is not None:
                g = g.cpu().numpy()
                assert g.dtype == w.dtype and (bits_equal(g, w) if w.dtype == np.float32 else np.array_equal(g, w))


def test_layout_pair_history_rows_off_a_16_byte_boundary():
    """rows that start 4 bytes off a 16-byte boundary take the plain-load path: the same outputs"""
    d = make_inputs(41, [130, 77], [split(300, 2), split(257, 1)])
    want = run_pair(d)
    args = [T(d[k]) for k in ("cur", "cur_lab", "cur_start", "hist", "hist_lab", "scan", "cls_a", "cls_b", "table_a", "table_b",
                              "sample_of_scan", "lo")]
    flat = torch.zeros(4 * len(d["hist"]) + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(-1, 4)
    view.copy_(args[3])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    (pa, la, ba, ba32, ia), (pb, bb, bb32), counts = B.stage_layout_pair(*args[:3], view, *args[4:], neg_col=NEG)
    assert np.array_equal(counts.cpu().numpy(), want[8])
    na, nb_ = len(want[0]), len(want[5])
    for g, w in zip((pa[:na], la[:na], ba[:na], ba32[:na], ia[:na], pb[:nb_], bb[:nb_], bb32[:nb_]), want[:8]):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and (bits_equal(g, w) if w.dtype == np.float32 else np.array_equal(g, w))


def test_layout_pair_checks_its_arguments():
    d = make_inputs(1, [10], [[20]])
    args = [T(d[k]) for k in ("cur", "cur_lab", "cur_start", "hist", "hist_lab", "scan", "cls_a", "cls_b", "table_a", "table_b",
                              "sample_of_scan", "lo")]
    with pytest.raises(ValueError):
        B.stage_layout_pair(*args[:11], torch.zeros((65, 3), device="cuda"))
    with pytest.raises(TypeError):
        B.stage_layout_pair(args[0][:, :3], *args[1:])
    with pytest.raises(ValueError):
        B.stage_layout_pair(*args[:2], args[2][:1], *args[3:])


# ------------------------------------------------------------------------------------------------ 2. the stage against the golden
PARTNER = [1, 2, 0]


def kd_scans(g, gk):
    """the three scan dicts of kd_stage.npz: samples 0 and 1 of multiscan.npz with the fixture's pseudo and canon columns, and the
    sample without history (scan 0 of cloud 0)"""
    Tn, lm = int(g["T"]), g["learning_map"]
    scans = []
    for b in range(2):
        s = kitti_scan(g, b)
        s["pseudo"] = [T(gk[f"b{b}_pseudo_canon_t{t}"].astype(np.int64)) for t in range(Tn)]
        s["canon"] = [T(gk[f"b{b}_canon_t{t}"].astype(np.int64)) for t in range(Tn)]
        scans.append(s)
    scans.append({"points": [T(g["b0_points_t0"])], "labels": [T(lm[g["b0_rawlabels_t0"]])], "poses": [T(g["b0_pose_t0"])],
                  "name": "2", "pseudo": [], "canon": []})
    return scans


def case_batch(g, gk, c):
    scans = kd_scans(g, gk)
    which = gk[f"{c}_samples"].tolist()
    steps, steps_gt = g["steps"].tolist(), gk["steps_gt"].tolist()
    kw = {}
    if bool(gk[f"{c}_training"]):
        rng = np.random.RandomState(int(gk[f"{c}_seed"]))     # tests/test_kd_host.py pins the draws to the stored ones
        om = M.draw_omega(rng)
        mix, aug = [], []
        for _ in which:
            mix.append(M.draw_mix_params(rng, om))
            aug.append(A.draw_train_params(rng))
        kw = dict(aug=aug, mix=mix, partners=[scans[PARTNER[b]] for b in which])
    return KD.build_kd_batch([scans[b] for b in which], 0.05, steps, steps_gt, **kw), kw


# both ways to lay the fused clouds out without a mix: ts_stage_layout_pair (the stage's path) and the launches it replaces
@pytest.mark.parametrize("pair_kernel", [False, True])
def test_build_kd_batch_matches_the_reference(g_multiscan, g_kd, monkeypatch, pair_kernel):
    monkeypatch.setattr(KD, "_PAIR_KERNEL", pair_kernel)
    cases = g_kd["cases"].tolist()
    assert cases == ["eval", "train_s4", "train_s2"]
    sparse, dense = BATCH_SPARSE + ("lidar_ms_gt",), BATCH_DENSE + ("offset_ms_gt", "num_points_ms_gt")
    kinds = []
    for c in cases:
        batch, kw = case_batch(g_multiscan, g_kd, c)
        prefix = f"{c}_batch_"
        check_batch(batch, g_kd, prefix, sparse=sparse, dense=dense)
        # every key of the case has been compared (the ring id is the reference's fifth `lidar` column: not carried here)
        stored = {k[len(prefix):] for k in g_kd if k.startswith(prefix)}
        compared = {f"{k}_{x}" for k in sparse for x in "CF"} | set(dense) | {"lidar_ring"}
        assert stored <= compared and len(stored) >= 18, sorted(stored - compared)
        assert batch["lidar"].F.shape[1] == 4 and batch["lidar_ms"].F.shape[1] == 5 and batch["lidar_ms_gt"].F.shape[1] == 5
        assert "_shift" not in batch
        kinds += [(p.kind, p.swap) for p in kw.get("mix", [])]
    assert set(kinds) == {(M.LASER, False), (M.POLAR, True), (M.POLAR, False)}


@pytest.mark.parametrize("pair_kernel", [False, True])
def test_build_kd_batch_equals_the_two_calls_it_replaces(g_multiscan, g_kd, monkeypatch, pair_kernel):
    monkeypatch.setattr(KD, "_PAIR_KERNEL", pair_kernel)
    g = g_multiscan
    steps = g["steps"].tolist()
    scans = [kitti_scan(g, 0), kitti_scan(g, 1)]               # two samples x 1500 points x 4 history scans, no pseudo / canon
    resident = [p.clone() for s in scans for p in s["points"]]
    want = S.build_multiscan_batch(scans, 0.05, steps)
    want_gt = S.build_multiscan_batch([dict(s) for s in scans], 0.05, steps)["lidar_ms"]
    got = KD.build_kd_batch(scans, 0.05, steps)
    assert set(got) == set(want) | {"lidar_ms_gt", "offset_ms_gt", "num_points_ms_gt"}
    same_batches({k: got[k] for k in want}, want)
    same_batches({"lidar_ms_gt": got["lidar_ms_gt"]}, {"lidar_ms_gt": want_gt})
    assert torch.equal(got["offset_ms_gt"], want["offset_ms"])
    assert all(torch.equal(a, b) for a, b in zip(resident, [p for s in scans for p in s["points"]])), "resident scans changed"
    # with the fixture's pseudo / canon columns and unequal steps, without and with the augmentation (no mix): the student's keys
    # are those of build_multiscan_batch, the teacher's cloud is the `lidar_ms` of a call whose pseudo column is the canon column
    # under steps_gt (both fused clouds hold the current scan and nothing below its minimum: one shift)
    scans = kd_scans(g, g_kd)
    as_teacher = [dict(s, pseudo=s["canon"]) for s in scans]
    steps_gt = g_kd["steps_gt"].tolist()
    rng = np.random.RandomState(3)
    for aug in (None, [A.draw_train_params(rng) for _ in scans]):
        got = KD.build_kd_batch(scans, 0.05, steps, steps_gt, aug=aug)
        want = S.build_multiscan_batch(scans, 0.05, steps, aug=aug)
        want_gt = S.build_multiscan_batch(as_teacher, 0.05, steps_gt, aug=aug)
        same_batches({k: got[k] for k in want}, want)
        same_batches({"lidar_ms_gt": got["lidar_ms_gt"]}, {"lidar_ms_gt": want_gt["lidar_ms"]})
        assert torch.equal(got["offset_ms_gt"], want_gt["offset_ms"]) and not torch.equal(got["offset_ms_gt"], got["offset_ms"])
    off = KD.build_kd_batch(scans, 0.05, steps, steps_gt, aug=[A.AugParams()] * len(scans))       # records without bits
    same_batches(off, KD.build_kd_batch(scans, 0.05, steps, steps_gt))


def test_kd_model_trains_on_a_mixed_augmented_batch(g_multiscan, g_kd):
    from taseg_amd.pcseg.model import build_network
    batch, kw = case_batch(g_multiscan, g_kd, "train_s4")
    assert kw["mix"] and kw["aug"]
    cfg = make_model_cfg("MinkUNetMsKd", in_dim=5, cr=0.5, num_layer=[1] * 8, SAMPLING_TYPE="random", MAX_VOXEL=100000,
                         FEAT_KD="mse", FEAT_KD_WEIGHT=10.0)
    model = fill_parameters(build_network(cfg, 20), seed=3).cuda().train()
    model.fix_part_param()
    ret, tb, _ = model(batch)
    loss = ret["loss"]
    assert torch.isfinite(loss).all() and np.isfinite(float(tb["loss_seg"])) and np.isfinite(float(tb["loss_feat_kd"]))
    loss.backward()
    grads = [p.grad for n, p in model.named_parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)


def test_more_than_32_samples_with_mix_are_refused(g_multiscan):
    scan = kitti_scan(g_multiscan, 0)
    with pytest.raises(ValueError):
        KD.build_kd_batch([scan] * 33, 0.05, g_multiscan["steps"].tolist(), mix=[M.MixParams()] * 33)
