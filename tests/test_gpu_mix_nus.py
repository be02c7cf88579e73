"""The nuScenes scan mixing on the device (-m gpu): `mix=` / `partners=` of the nuScenes data stage and the nuScenes `lasermix_aug_`
against the reference's own functions (tests/golden/multiscan_mix_nus.npz: `polarmix` of PolarMix_nuscenes.py, `lasermix_aug` /
`lasermix_aug_` of LaserMix_nuscenes.py in the order of nuscenes_ms.py:132-214, then `get_single_sample` + `collate_batch` of
nuscenes_voxel_ms.py) - integer tensors exact, float32 features bit for bit -, the batched path against the per-sample one, and
what the stage refuses.  The generator asserts that no fixture row sits at a sector bound or a band threshold."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from taseg_amd import backend as B  # noqa: E402
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import nuscenes as N  # noqa: E402
from test_gpu_augment import T, check_batch, nus_samples, same_batches, same_bits  # noqa: E402

VOXEL = 0.1


@pytest.fixture(scope="module")
def g_mix_nus():
    return dict(np.load(os.path.join(GOLDEN, "multiscan_mix_nus.npz"), allow_pickle=False))


def nus_clouds(gn):
    """(samples, partners) as numpy clouds: what the reference's `__getitem__` holds of keyframe b as a sample (nuscenes_ms.py:131)
    and as a partner (:136-159: the keyframe as the file holds it, the kept sweep rows behind it)"""
    lm = gn["learning_map"]
    samples, partners = [], []
    for b in range(2):
        key, ann, mask = gn[f"b{b}_points_cur"], lm[gn[f"b{b}_rawlabels_cur"]].astype(np.int64), gn[f"b{b}_mask"]
        samples.append({"raw": gn[f"b{b}_xyzret"], "lab": gn[f"b{b}_labels"], "raw_ms": gn[f"b{b}_xyzret_ms"], "lab_ms": gn[f"b{b}_labels_ms"]})
        partners.append({"raw": key, "lab": ann, "raw_ms": np.concatenate([key, gn[f"b{b}_fused_all"][mask]]),
                         "lab_ms": np.concatenate([ann, gn[f"b{b}_labels_all"][mask]])})
    return samples, partners


def unpack_rows(step, new, pool):
    """a mixed cloud of the fixture: rows of `pool` by index (stored as first differences), -1 = the next row of `new`"""
    src = np.cumsum(step)
    rows = np.ascontiguousarray(pool, dtype=np.float32)[np.maximum(src, 0)]
    rows[src < 0] = new
    return rows


def batch_params(g, c):
    """the case's records: its seed through the draw functions (tests/test_mix_nus_host.py pins them to the stored draws)"""
    rng = np.random.RandomState(int(g[f"{c}_head"][0]))
    om = M.draw_omega(rng)
    mix, aug = [], []
    for _ in range(2):
        mix.append(M.draw_mix_params(rng, om, dataset="nuscenes", n_partners=2))
        aug.append(A.draw_train_params(rng))
    return mix, aug


def same_rows(got, want_pts, want_lab, what):
    pts, lab = got
    assert lab.dtype == torch.int64 and pts.dtype == torch.float32
    same_bits(pts, np.ascontiguousarray(want_pts, dtype=np.float32), (what, "rows"))
    assert np.array_equal(lab.cpu().numpy(), np.asarray(want_lab).reshape(-1).astype(np.int64)), (what, "labels")


def polar(**kw):
    base = dict(kind=M.POLAR, alpha=-2.1, beta=-2.1 + np.pi, swap=True, paste=True, omega=(0.9, 2.9), tail_all=False,
                instance_classes=M.INSTANCE_CLASSES["nuscenes"], dataset="nuscenes")
    base.update(kw)
    return M.MixParams(**base)


def bare(s):
    """the sample as the first keyframe of its scene: no history"""
    return dict(s, hist_points=[], hist_labels=[], hist_pseudo=[], params=s["params"][:0])


# ------------------------------------------------------------------------------------------------ 1. against the golden
def test_stage_with_mix_matches_the_reference(g_multiscan_nus, g_mix_nus):
    samples, steps = nus_samples(g_multiscan_nus)
    resident = [t.clone() for s in samples for t in [s["points"]] + s["hist_points"]]
    kinds = set()
    for c in g_mix_nus["cases"].tolist():
        mix, aug = batch_params(g_mix_nus, c)
        kinds |= {(p.kind, p.swap, p.partner == b) for b, p in enumerate(mix)}
        partners = [samples[p.partner] for p in mix]
        batched = N.build_nuscenes_batch(samples, VOXEL, steps, aug=aug, mix=mix, partners=partners)
        check_batch(batched, g_mix_nus, f"{c}_batch_")                          # point_mask among the dense tensors
        per_sample = N.build_nuscenes_batch_per_sample(samples, VOXEL, steps, aug=aug, mix=mix, partners=partners)
        check_batch(per_sample, g_mix_nus, f"{c}_batch_")
        same_batches(batched, per_sample)
        same_batches(batched, N.build_nuscenes_batch(samples, VOXEL, steps, aug=aug, mix=mix, partners=partners))   # two runs
    # PolarMix with and without the swap, the other keyframe and the sample itself as partner, the recipe's LaserMix
    assert {(M.POLAR, True, False), (M.POLAR, True, True), (M.POLAR, False, True), (M.LASER, False, False)} <= kinds
    assert all(torch.equal(a, b) for a, b in zip(resident, [t for s in samples for t in [s["points"]] + s["hist_points"]])), \
        "resident sweeps changed"


def test_mixed_clouds_and_lasermix_aug__match_the_reference(g_multiscan_nus, g_mix_nus):
    g = g_mix_nus
    samples, partners = nus_clouds(g_multiscan_nus)

    def check(c, e, e1, fn):
        for key, lab in (("raw", "lab"), ("raw_ms", "lab_ms")):
            want = unpack_rows(g[f"{c}_{key}_step"], g[f"{c}_{key}_new"], np.concatenate([e[key], e1[key]], 0))
            same_rows(fn(T(e[key]), T(e[lab]), T(e1[key]), T(e1[lab])), want, g[f"{c}_{lab}"], (c, key))
        return len(want)
    for c in g["cases"].tolist():
        for b, p in enumerate(batch_params(g, c)[0]):
            check(f"{c}_s{b}", samples[b], partners[p.partner], lambda *a: M.mix_points(*a, p))
    # `lasermix_aug_` of the nuScenes file: its own bands (LaserMix_nuscenes.py:138-194)
    for c, (b, other, k) in zip(g["laser_cases"].tolist(), g["laser_meta"].tolist()):
        e, e1 = samples[b], partners[other]
        p = M.MixParams(kind=M.LASER, strategy=k, degrees=True, dataset="nuscenes")
        n = check(c, e, e1, lambda *a: M.mix_points(*a, p))
        check(c, e, e1, lambda *a: M.lasermix_points(*a, k, degrees=True, dataset="nuscenes"))
        check(c, e, e1, lambda *a: M.lasermix_points(*a, M.STRATEGIES[k], degrees=True, dataset="nuscenes"))
        # ... which are not SemanticKITTI's
        other_rows = M.lasermix_points(T(e["raw_ms"]), T(e["lab_ms"]), T(e1["raw_ms"]), T(e1["lab_ms"]), k, degrees=True)[0]
        assert other_rows.shape[0] != n
    assert len(g["laser_cases"]) == 3


# ------------------------------------------------------------------------------------------------ 2. the paths agree
def test_paths_agree_on_mixed_kinds_and_missing_history(g_multiscan_nus):
    samples, steps = nus_samples(g_multiscan_nus)
    first = bare(samples[1])
    rng = np.random.RandomState(21)
    # a batch of three with one history-less sample; PolarMix, `lasermix_aug_` and no mix in one batch
    three = [samples[0], first, samples[1]]
    mix = [polar(), M.MixParams(kind=M.LASER, strategy=1, degrees=True, dataset="nuscenes"), M.MixParams()]
    partners = [samples[1], samples[0], None]
    aug = [A.draw_train_params(rng) for _ in three]
    calls = []
    real = B.stage_clamp_compact

    def record(*a):
        calls.append(a[0].shape)
        return real(*a)
    B.stage_clamp_compact = record
    try:
        for au in (aug, None):
            a = N.build_nuscenes_batch(three, VOXEL, steps, aug=au, mix=mix, partners=partners)
            n_calls = len(calls)
            same_batches(a, N.build_nuscenes_batch_per_sample(three, VOXEL, steps, aug=au, mix=mix, partners=partners))
            assert len(calls) == n_calls                             # the per-sample path keeps its own clamp
            same_batches(a, N.build_nuscenes_batch(three, VOXEL, steps, aug=au, mix=mix, partners=partners))
    finally:
        B.stage_clamp_compact = real
    # ts_stage_clamp_compact ran once per batched call, on rows of in_feature_dim columns
    assert len(calls) == 4 and all(len(shape) == 2 and shape[1] == 4 for shape in calls)
    n = a["num_points"].view(-1).tolist()
    assert n[2] == samples[1]["points"].shape[0] and n[0] != samples[0]["points"].shape[0]
    # a history-less partner, a self-partner (the same dict), a history-less sample that is mixed
    mix = [polar(), polar(alpha=-0.4, beta=-0.4 + np.pi), polar(swap=False)]
    partners = [first, samples[1], samples[0]]
    three = [samples[0], samples[1], first]
    a = N.build_nuscenes_batch(three, VOXEL, steps, aug=aug, mix=mix, partners=partners)
    same_batches(a, N.build_nuscenes_batch_per_sample(three, VOXEL, steps, aug=aug, mix=mix, partners=partners))
    # the recipe's LaserMix branch is the identity and needs no partner: the tensors of the un-mixed sample
    lone = [M.MixParams(kind=M.LASER, strategy=2, dataset="nuscenes")] * 2
    same_batches(N.build_nuscenes_batch(samples, VOXEL, steps, aug=aug[:2], mix=lone),
                 N.build_nuscenes_batch(samples, VOXEL, steps, aug=aug[:2]))


def test_five_columns_show_the_ring_and_the_zero_tails(g_multiscan_nus):
    samples, steps = nus_samples(g_multiscan_nus)
    # the files' column 4, the ring index: 1 .. 32 here (the fixture's files hold 0)
    for s in samples:
        s["points"] = s["points"].clone()
        s["points"][:, 4] = (torch.arange(s["points"].shape[0], device="cuda") % 32 + 1).float()
    mix = [polar(swap=False), polar()]
    partners = [samples[1], samples[0]]
    aug = [A.draw_train_params(np.random.RandomState(4)) for _ in samples]
    a = N.build_nuscenes_batch(samples, VOXEL, steps, in_feature_dim=5, aug=aug, mix=mix, partners=partners)
    same_batches(a, N.build_nuscenes_batch_per_sample(samples, VOXEL, steps, in_feature_dim=5, aug=aug, mix=mix, partners=partners))
    assert a["lidar"].F.shape[1] == 5 and a["lidar_ms"].F.shape[1] == 5
    # sample 0, no swap: its own keyframe (column 4 = 0) | the partner's instance rows (the ring) | two rotated copies (zeros)
    n_cur = samples[0]["points"].shape[0]
    n_inst = int(torch.isin(samples[1]["labels"], torch.tensor(M.INSTANCE_CLASSES["nuscenes"], device="cuda")).sum())
    assert n_inst > 0 and int(a["num_points"][0]) == n_cur + 3 * n_inst
    feats = a["lidar"].F[a["lidar"].C[:, 3] == 0]
    ring = feats[:, 4]
    assert 0 < int((ring != 0).sum()) <= n_inst and bool(((ring == 0) | ((ring >= 1) & (ring <= 32))).all())
    # with 4 columns none of it shows, and the rows are the same
    b = N.build_nuscenes_batch(samples, VOXEL, steps, aug=aug, mix=mix, partners=partners)
    assert torch.equal(b["num_points"], a["num_points"]) and torch.equal(b["num_points_ms"], a["num_points_ms"])
    assert torch.equal(b["lidar"].F.view(torch.int32), a["lidar"].F[:, :4].contiguous().view(torch.int32))


def test_no_mix_is_the_old_path_and_refusals(g_multiscan_nus):
    samples, steps = nus_samples(g_multiscan_nus)
    rng = np.random.RandomState(8)
    off = [M.draw_mix_params(rng, (0.3, 2.5), dataset="nuscenes", n_partners=2, training=False) for _ in samples]
    assert all(p.kind == M.NONE for p in off)
    for fn in (N.build_nuscenes_batch, N.build_nuscenes_batch_per_sample):
        for mix in (None, [M.MixParams()] * 2, off):
            check_batch(fn(samples, VOXEL, steps, mix=mix), g_multiscan_nus, "batch_")
        check_batch(fn(samples, VOXEL, steps, mix=off, partners=[samples[1], None]), g_multiscan_nus, "batch_")
        with pytest.raises(ValueError):
            fn(samples, VOXEL, steps, mix=[polar(), M.MixParams()])                             # a record that needs a partner
        with pytest.raises(ValueError):
            fn(samples, VOXEL, steps, mix=[polar(), M.MixParams()], partners=[None, samples[0]])
        with pytest.raises(ValueError):
            fn(samples, VOXEL, steps, mix=[polar()], partners=[samples[1]])                     # a wrong-length list
        with pytest.raises(ValueError):
            fn(samples, VOXEL, steps, mix=[polar(), polar()], partners=[samples[1]])
        with pytest.raises(ValueError):
            fn(samples, VOXEL, steps, mix=[polar(), "polar"], partners=[samples[1], samples[0]])
