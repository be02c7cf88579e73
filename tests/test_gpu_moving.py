"""Moving-object augmentation of the SMSA recipe on the device (-m gpu): ts_stage_moving_stats / ts_stage_moving_apply and the
`moving=` path of the data stage against the reference's own code (tests/golden/moving*.npz: `multiscan_fuse`, `static2moving`,
`moving2static`, the whole `__getitem__` of semantickitti_ms_ms.py, then `get_single_sample` + `collate_batch`), statistics, rows,
labels and order bit for bit - a NaN equal to a NaN at the same place: an instance without a row at frame offset -1 gets a NaN
shift in the reference and here; the edges against numpy's own `.mean()` / `.min()` / `.max()` and the device rule restated in
numpy below (include/taseg_hip.h)."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from taseg_amd import backend as B  # noqa: E402
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import moving as MV  # noqa: E402
from taseg_amd.data import stage as S  # noqa: E402
from test_gpu_augment import T, check_batch, kitti_scan, same_batches  # noqa: E402

CLASSES = (18, 20, 253, 255)
EYE = np.eye(4, dtype=np.float32)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


@pytest.fixture(scope="module")
def g_mov():
    return _load("moving.npz")


@pytest.fixture(scope="module")
def g_mov_batch():
    return _load("moving_batch.npz")


def same_bits_nan(got, want, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), (what, np.argwhere(~ok)[:4].tolist())


def golden_scan(g, n):
    """the scan dict of a fixture cloud: full labels only - `labels` is not read under moving="""
    tn = int(g["T"])
    return {"points": [T(g[f"{n}_points_t{t}"]) for t in range(tn + 1)],
            "raw_labels": [T(g[f"{n}_rawlabels_t{t}"].astype(np.int64)) for t in range(tn + 1)],
            "poses": [T(g[f"{n}_pose_t{t}"]) for t in range(tn + 1)], "name": n}


def golden_table(g, n):
    return MV.MovingTable(g[f"{n}_cand"], g[f"{n}_counts"], g[f"{n}_stats"], len(g[f"{n}_fused"]))


def same_table(got, want, what):
    assert got.labels.dtype == np.int64 and np.array_equal(got.labels, want.labels), (what, "candidates")
    assert got.counts.dtype == np.int32 and np.array_equal(got.counts, want.counts), (what, "counts")
    same_bits_nan(got.stats, want.stats, (what, "statistics"))
    assert got.n_history == want.n_history


# ------------------------------------------------------------------------------------------------ 1. against the golden
def test_statistics_match_the_reference(g_mov):
    a, b = golden_scan(g_mov, "a"), golden_scan(g_mov, "b")
    tables = S.moving_tables([a, b], [b, a])             # four clouds with two different tables in one call
    for (own, partner), n, m in zip(tables, "ab", "ba"):
        same_table(own, golden_table(g_mov, n), n)
        same_table(partner, golden_table(g_mov, m), ("partner", m))
    t = tables[0][0]
    assert (t.labels >= 1 << 31).any() and np.isnan(t.stats[:, 5]).any() and (t.counts[:, 1] == 0).any() and (t.counts[:, 1] == 1).any()
    again = S.moving_tables([a, b], [b, a])
    for (own, partner), (own2, partner2) in zip(tables, again):
        same_table(own2, own, "second run")
        same_table(partner2, partner, "second run")
    assert S.moving_tables([a])[0][1] is None
    same_table(S.moving_tables([b])[0][0], golden_table(g_mov, "b"), "alone")


def golden_rows(g, n):
    tn = int(g["T"])
    cur, fused = g[f"{n}_points_t{tn}"], g[f"{n}_fused"]
    full = np.concatenate([g[f"{n}_rawlabels_t{tn}"]] + [g[f"{n}_rawlabels_t{t}"] for t in range(tn)]).astype(np.int64)
    delta = np.concatenate([np.zeros(len(cur)), g[f"{n}_delta"]]).astype(np.int32)
    return cur, fused, full, delta


def apply_rows(cur, fused, full, delta, params, cloud=None, n_cur=None):
    """ts_stage_moving_apply on rows given as numpy arrays -> (rows after it, labels)"""
    pts = T(np.concatenate([cur, fused], 0))
    n_cur = len(cur) if n_cur is None else n_cur
    cloud = np.zeros(len(full), dtype=np.int32) if cloud is None else cloud
    labels, start, rec = MV.pack_moving(params)
    lab = B.stage_moving_apply(pts, n_cur, T(full), T(cloud), T(delta), T(labels), T(start), T(rec), T(MV.LABEL_TABLE))
    return pts, lab


def test_clouds_after_each_pass_match_the_reference(g_mov):
    g, lm = g_mov, g_mov["learning_map"]
    kinds = set()
    for c in g["cases"].tolist():
        n = "ab"[int(g[f"{c}_cloud"])]
        cur, fused, full, delta = golden_rows(g, n)
        p = MV.draw_moving_params(np.random.RandomState(int(g[f"{c}_seed"])), golden_table(g, n))   # (test_moving_host.py pins it)
        kinds |= {r.kind for r in p.records}
        s2m = MV.MovingParams(tuple(r for r in p.records if r.kind != MV.M2S))
        for name, q in (("s2m", s2m), ("m2s", p)):
            want_cur, want_hist = cur.copy(), fused.copy()
            want_cur[g[f"{c}_{name}_cur_idx"]] = g[f"{c}_{name}_cur_rows"]
            want_hist[g[f"{c}_{name}_hist_idx"]] = g[f"{c}_{name}_hist_rows"]
            pts, lab = apply_rows(cur, fused, full, delta, [q])
            same_bits_nan(pts[:len(cur)], want_cur, (c, name, "current rows"))
            same_bits_nan(pts[len(cur):], want_hist, (c, name, "history rows"))
            want_lab = lm[np.concatenate([g[f"{c}_{name}_cur_cls"], g[f"{c}_{name}_hist_cls"]]).astype(np.int64)]
            assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), want_lab), (c, name, "labels")
    assert kinds == {MV.S2M_X, MV.S2M_Y, MV.M2S}
    # no record: the rows as they were, every label through the 26-class table
    cur, fused, full, delta = golden_rows(g, "a")
    pts, lab = apply_rows(cur, fused, full, delta, [None])
    same_bits_nan(pts, np.concatenate([cur, fused]), "no record")
    assert np.array_equal(lab.cpu().numpy(), lm[full & 0xFFFF]) and lab.max() == 25


# ------------------------------------------------------------------------------------------------ 2. edges against numpy
def numpy_table(cur, full_c, hist, full_h, delta):
    """the statistics with numpy's own calls, as semantickitti_ms_ms.py:316-321, :362-370 takes them"""
    cand = np.unique(full_c[np.isin(full_c & 0xFFFF, CLASSES)]).astype(np.int64)
    counts, stats = np.zeros((len(cand), 3), dtype=np.int32), np.zeros((len(cand), 9), dtype=np.float32)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # numpy's "Mean of empty slice": the NaN is what is wanted
        for k, inst in enumerate(cand):
            c, h = cur[full_c == inst], hist[full_h == inst]
            p = hist[(full_h == inst) & (delta == -1)]
            counts[k] = len(c), len(h), len(p)
            ext = [h[:, 0].min(), h[:, 0].max(), h[:, 1].min(), h[:, 1].max()] if len(h) else [np.inf, -np.inf, np.inf, -np.inf]
            stats[k] = ext + [h[:, 1].mean(), p[:, 0].mean(), p[:, 1].mean(), c[:, 0].mean(), c[:, 1].mean()]
    return MV.MovingTable(cand, counts, stats, len(hist))


def numpy_rule(cur, full_c, hist, full_h, delta, p):
    """ts_stage_moving_apply restated in numpy (include/taseg_hip.h) -> (current rows, history rows, labels of both)"""
    cur, hist, f32 = cur.copy(), hist.copy(), np.float32
    cls_c, cls_h = full_c & 0xFFFF, full_h & 0xFFFF
    with np.errstate(invalid="ignore"):
        for r in p.records:
            mc, mh = full_c == r.label, full_h == r.label
            d = delta[mh]
            if r.kind == MV.S2M_X:
                if r.center != 0.0:
                    cur[mc, 1] = cur[mc, 1] + f32(r.center)
                    hist[mh, 1] = hist[mh, 1] + f32(r.center)
                hist[mh, 0] = hist[mh, 0] + (d.astype(np.float64) * r.shift).astype(f32)
            elif r.kind == MV.S2M_Y:
                hist[mh, 1] = hist[mh, 1] + (d.astype(np.float64) * r.shift).astype(f32)
            elif r.kind == MV.M2S:
                hist[mh, 0] = hist[mh, 0] + d.astype(f32) * f32(r.shift_x)
                hist[mh, 1] = hist[mh, 1] + d.astype(f32) * f32(r.shift_y)
            cls_c[mc], cls_h[mh] = r.new_class, r.new_class
    return cur, hist, MV.LABEL_TABLE[np.concatenate([cls_c, cls_h])]


def synthetic_cloud(rng, sizes, n_other, deltas=(-2, -1), hist_share=1.0):
    """A scan dict with identity poses (the pose fuse then returns its input bits) whose instance i has sizes[i] rows in the current
    scan and int(sizes[i] * hist_share) in every history scan, interleaved with n_other rows of other classes and of instances
    that are no candidates.  Returns (scan dict, current rows, full labels, history rows, full labels, frame offsets)."""
    def scan(share, with_strangers):
        rows, labels = [], []
        for i, n in enumerate(sizes):
            n = int(n * share)
            rows.append(rng.standard_normal((n, 4)) * [3.0, 1.0, 0.5, 0.2] + [10.0 * (i % 5) - 20.0, 4.0 * (i % 3) - 4.0, 0, 0])
            labels.append(np.full(n, ((i + 1) << 16) | CLASSES[i % 4], dtype=np.int64))
        rows.append(rng.uniform(-40, 40, (n_other, 4)))
        other = rng.choice([0, 10, 40, 48, 50, 70, 252, 254, 258, 259], n_other).astype(np.int64) | (rng.randint(0, 50, n_other) << 16)
        if with_strangers:                               # candidate classes under labels the current scan does not hold
            other[::7] = (900 << 16) | 18
            other[3::11] = (901 << 16) | 253
        labels.append(other)
        rows, labels = np.concatenate(rows).astype(np.float32), np.concatenate(labels)
        order = rng.permutation(len(rows))
        return np.ascontiguousarray(rows[order]), labels[order]
    cur, full_c = scan(1.0, False)
    hist = [scan(hist_share, True) for _ in deltas]
    s = {"points": [T(h[0]) for h in hist] + [T(cur)], "raw_labels": [T(h[1]) for h in hist] + [T(full_c)],
         "poses": [T(EYE)] * (len(deltas) + 1), "deltas": list(deltas), "name": "synthetic"}
    hp = np.concatenate([h[0] for h in hist]) if hist else np.zeros((0, 4), dtype=np.float32)
    hl = np.concatenate([h[1] for h in hist]) if hist else np.zeros(0, dtype=np.int64)
    hd = np.concatenate([np.full(len(h[0]), d, dtype=np.int32) for h, d in zip(hist, deltas)]) if hist else np.zeros(0, dtype=np.int32)
    return s, cur, full_c, hp, hl, hd


def test_means_follow_numpy_at_every_size_of_the_rule():
    # instance sizes at the edges of numpy's pairwise rule and of its 8192-term pieces; the history mean runs over twice as many
    sizes = [1, 7, 8, 9, 127, 128, 129, 8192, 8193]
    s, cur, full_c, hp, hl, hd = synthetic_cloud(np.random.RandomState(1), sizes, 4000)
    want = numpy_table(cur, full_c, hp, hl, hd)
    assert want.counts[:, 0].tolist() == sizes and want.counts[:, 2].tolist() == sizes and want.counts[:, 1].tolist() == [2 * n for n in sizes]
    got = S.moving_tables([s])[0][0]
    same_table(got, want, "sizes of the rule")
    same_table(S.moving_tables([s])[0][0], got, "second run")


@pytest.mark.parametrize("total", [255, 256, 257, 513, 64 * 256 + 3])
def test_rows_straddling_the_block_size(total):
    # (64 * 256 + 3 rows: 65 blocks, the last instance row's block offset is the carry of the scan's first wave-wide step)
    rng = np.random.RandomState(total)
    s, cur, full_c, hp, hl, hd = synthetic_cloud(rng, [25, 15], 20, deltas=(-1,), hist_share=1.0)
    # (40 + 20 current rows, 40 + 20 history rows; pad the history up to `total` rows in all, the last row an instance row)
    pad = total - len(cur) - len(hp) - 1
    assert pad >= 0
    hp = np.concatenate([hp, rng.uniform(-40, 40, (pad, 4)).astype(np.float32), [[1.0, 2.0, 3.0, 0.5]]]).astype(np.float32)
    hl = np.concatenate([hl, np.zeros(pad, dtype=np.int64), [(1 << 16) | 18]])
    hd = np.concatenate([hd, np.full(pad + 1, -1, dtype=np.int32)])
    s["points"][0], s["raw_labels"][0] = T(hp), T(hl)
    assert len(cur) + len(hp) == total
    want = numpy_table(cur, full_c, hp, hl, hd)
    got = S.moving_tables([s])[0][0]
    same_table(got, want, total)
    p = MV.MovingParams((MV.MovingRecord((1 << 16) | 18, MV.S2M_X, center=2.75, shift=1.3, new_class=258),
                         MV.MovingRecord((2 << 16) | 20, MV.S2M_Y, shift=3.1, new_class=259)))
    delta = np.concatenate([np.zeros(len(cur), dtype=np.int32), hd])
    pts, lab = apply_rows(cur, hp, np.concatenate([full_c, hl]), delta, [p])
    w_cur, w_hist, w_lab = numpy_rule(cur, full_c, hp, hl, hd, p)
    same_bits_nan(pts, np.concatenate([w_cur, w_hist]), (total, "rows"))
    assert np.array_equal(lab.cpu().numpy(), w_lab) and w_lab[-1] == 25 and pts[-1, 1] == np.float32(2.0) + np.float32(2.75)


def test_empty_tables_one_candidate_and_a_cloud_without_history():
    rng = np.random.RandomState(9)
    none, *rest = synthetic_cloud(rng, [], 700, deltas=(-1,))
    one, *rest_one = synthetic_cloud(rng, [30], 500, deltas=(-3, -1), hist_share=0.5)
    alone, cur, full_c, hp, hl, hd = synthetic_cloud(rng, [21, 5], 300, deltas=())
    tables = S.moving_tables([none, one, alone], [None, alone, None])
    assert [len(t[0].labels) for t in tables] == [0, 1, 2] and tables[0][1] is None and tables[2][1] is None
    same_table(tables[0][0], numpy_table(*rest), "no candidate")
    same_table(tables[1][0], numpy_table(*rest_one), "one candidate")
    want = numpy_table(cur, full_c, hp, hl, hd)
    same_table(tables[2][0], want, "no history")
    same_table(tables[1][1], want, "no history, as a partner")
    assert want.n_history == 0 and (want.counts[:, 1:] == 0).all() and np.isnan(want.stats[:, 4:7]).all() and np.isinf(want.stats[:, :4]).all()
    assert len(S.moving_tables([none])[0][0].labels) == 0                       # a call without any candidate
    # neither pass runs without history: nothing is drawn; the one-candidate cloud draws its coin
    rng = np.random.RandomState(0)
    state = rng.get_state()[1].copy()
    assert MV.draw_moving_params(rng, tables[2][0]) == MV.MovingParams() and np.array_equal(state, rng.get_state()[1])
    assert len(MV.draw_moving_params(rng, tables[1][0]).draws) == 1
    # the stage takes such clouds: a record for the one candidate, none for the others
    label = int(tables[1][0].labels[0])
    rec = MV.MovingRecord(label, MV.S2M_Y, shift=2.0, new_class=259) if label & 0xFFFF in (18, 20) else \
        MV.MovingRecord(label, MV.M2S, shift_x=0.5, shift_y=-0.25, new_class=MV.MOVING_CLASSES[label & 0xFFFF])
    moving = [MV.MovingParams(), MV.MovingParams((rec,)), None]
    steps = [0, 0, 2, 2, 2, 2, 2, 2, 2, 0, 4, 4, 4, 0, 4, 0, 2, 4, 2, 1]
    batched = S.build_multiscan_batch([none, one, alone], 0.05, steps, moving=moving)
    same_batches(batched, S.build_multiscan_batch_per_sample([none, one, alone], 0.05, steps, moving=moving))
    assert batched["num_points"].view(-1).tolist() == [700, 530, 326]
    assert int(batched["targets_mapped"].F.max()) >= 20                        # the moving classes of the 26-class map


def test_several_clouds_with_different_tables_in_one_apply():
    rng = np.random.RandomState(4)
    clouds = [synthetic_cloud(rng, sizes, 400, deltas=(-2, -1)) for sizes in ([40, 30, 20, 10], [25], [], [300, 3])]
    # instance 1 exists in every cloud under the same full label, with a record of its own in each (or none)
    params = [MV.MovingParams((MV.MovingRecord((1 << 16) | 18, MV.S2M_X, center=-3.5, shift=2.25, new_class=258),
                               MV.MovingRecord((3 << 16) | 253, MV.M2S, shift_x=0.75, shift_y=float("nan"), new_class=31))),
              MV.MovingParams((MV.MovingRecord((1 << 16) | 18, MV.S2M_Y, shift=0.5, new_class=258),)),
              None,
              MV.MovingParams((MV.MovingRecord((2 << 16) | 20, MV.S2M_X, shift=4.4, new_class=259),))]
    cur = np.concatenate([c[1] for c in clouds])
    hist = np.concatenate([c[3] for c in clouds])
    full = np.concatenate([c[2] for c in clouds] + [c[4] for c in clouds])
    delta = np.concatenate([np.zeros(len(cur), dtype=np.int32)] + [c[5] for c in clouds])
    cloud = np.concatenate([np.full(len(c[1]), i) for i, c in enumerate(clouds)] +
                           [np.full(len(c[3]), i) for i, c in enumerate(clouds)]).astype(np.int32)
    pts, lab = apply_rows(cur, hist, full, delta, params, cloud=cloud)
    want = [numpy_rule(c[1], c[2], c[3], c[4], c[5], p or MV.MovingParams()) for c, p in zip(clouds, params)]
    same_bits_nan(pts, np.concatenate([w[0] for w in want] + [w[1] for w in want]), "rows")
    n_c = [len(c[1]) for c in clouds]
    want_lab = np.concatenate([w[2][:n] for w, n in zip(want, n_c)] + [w[2][n:] for w, n in zip(want, n_c)])
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    assert np.isnan(pts.cpu().numpy()).any() and (pts[:len(cur)].cpu().numpy() != cur).any()
    again, lab2 = apply_rows(cur, hist, full, delta, params, cloud=cloud)
    assert torch.equal(pts.view(torch.int32), again.view(torch.int32)) and torch.equal(lab, lab2)


# ------------------------------------------------------------------------------------------------ 3. the stage
def batch_params(g, c, tables):
    rng = np.random.RandomState(int(g[f"{c}_seed"]))
    om = M.draw_omega(rng)
    moving, mix, partner_moving, aug = [], [], [], []
    for own, partner in tables:
        mv, mx, pmv = MV.draw_smsa_sample(rng, om, own, partner)
        moving.append(mv)
        mix.append(mx)
        partner_moving.append(pmv)
        aug.append(A.draw_train_params(rng))
    return moving, mix, partner_moving, aug


def test_stage_with_moving_mix_and_aug_matches_the_reference(g_mov, g_mov_batch):
    steps = g_mov["steps"].tolist()
    assert len(steps) == 20
    scans = [golden_scan(g_mov, "a"), golden_scan(g_mov, "b")]
    partners = [scans[1], scans[0]]
    resident = [p.clone() for s in scans for p in s["points"]]
    tables = S.moving_tables(scans, partners)
    kinds = set()
    for c in g_mov_batch["cases"].tolist():
        moving, mix, partner_moving, aug = batch_params(g_mov_batch, c, tables)
        kinds |= {p.kind for p in mix}
        assert all(m.records for m in moving) and any(m.records for m in partner_moving)
        kw = dict(aug=aug, mix=mix, partners=partners, moving=moving, partner_moving=partner_moving)
        batched = S.build_multiscan_batch(scans, 0.05, steps, **kw)
        check_batch(batched, g_mov_batch, f"{c}_batch_")
        per_sample = S.build_multiscan_batch_per_sample(scans, 0.05, steps, **kw)
        check_batch(per_sample, g_mov_batch, f"{c}_batch_")
        same_batches(batched, per_sample)
        same_batches(batched, S.build_multiscan_batch(scans, 0.05, steps, **kw))                       # two runs
    assert kinds == {M.LASER, M.POLAR}
    assert all(torch.equal(a, b) for a, b in zip(resident, [p for s in scans for p in s["points"]])), "resident scans changed"


def test_stage_paths_agree_without_mix_and_moving_none_is_the_old_path(g_multiscan, g_mov):
    steps = g_mov["steps"].tolist()
    scans = [golden_scan(g_mov, "a"), golden_scan(g_mov, "b"), golden_scan(g_mov, "a")]
    tables = S.moving_tables(scans)
    rng = np.random.RandomState(2)
    moving = [MV.draw_moving_params(rng, t[0], maug_prob=2) for t in tables[:2]] + [None]
    assert all(m.records for m in moving[:2])
    aug = [A.draw_train_params(rng) for _ in scans]
    for au in (aug, None):
        a = S.build_multiscan_batch(scans, 0.05, steps, aug=au, moving=moving)
        same_batches(a, S.build_multiscan_batch_per_sample(scans, 0.05, steps, aug=au, moving=moving))
        same_batches(a, S.build_multiscan_batch(scans, 0.05, steps, aug=au, moving=moving))
        # ... and through the mix path with records that mix nothing
        same_batches(a, S.build_multiscan_batch(scans, 0.05, steps, aug=au, moving=moving, mix=[M.MixParams()] * 3))
    # the shifts are there: sample 0 differs from its un-moved twin, sample 2
    n0 = int(a["num_points"].view(-1)[0])
    f = a["targets_mapped"].F
    assert not torch.equal(f[:n0], f[-n0:]) and a["num_points"].view(-1)[2] == n0
    with pytest.raises(ValueError):
        S.build_multiscan_batch(scans, 0.05, steps, moving=moving[:2])
    with pytest.raises(ValueError):
        S.build_multiscan_batch([kitti_scan(g_multiscan, 0)], 0.05, steps, moving=[None])      # no raw_labels
    # moving=None: today's tensors
    g = g_multiscan
    old = [kitti_scan(g, 0), kitti_scan(g, 1)]
    plain = S.build_multiscan_batch(old, 0.05, g["steps"].tolist())
    check_batch(plain, g, "batch_")
    same_batches(plain, S.build_multiscan_batch(old, 0.05, g["steps"].tolist(), moving=None, partner_moving=None))
    same_batches(plain, S.build_multiscan_batch_per_sample(old, 0.05, g["steps"].tolist(), moving=None))
