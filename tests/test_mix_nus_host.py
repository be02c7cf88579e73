"""The nuScenes scan mixing on the host: the draws of tests/golden/multiscan_mix_nus.npz replayed through taseg_amd.data.mix (the
reference's order of nuscenes_ms.py:16, :132-214 - coin, partner, strategy or alpha / swap / paste - then the augmentation's), the
band thresholds of the nuScenes `lasermix_aug_` (LaserMix_nuscenes.py:116-201), the signatures of the stage functions and the
C ABI entry of the clamp compaction.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from taseg_amd.data import augment as A
from taseg_amd.data import mix as M


@pytest.fixture(scope="module")
def g_mix_nus():
    return dict(np.load(os.path.join(GOLDEN, "multiscan_mix_nus.npz"), allow_pickle=False))


def test_stored_draws_replay(g_mix_nus):
    g = g_mix_nus
    cols = g["draw_columns"].tolist()
    assert cols == ["prob", "partner", "kind", "strategy", "alpha", "swap", "paste", "theta", "scale", "flip", "noise_x", "noise_y",
                    "noise_z"]
    seen = []
    for c in g["cases"].tolist():
        seed, *omega = g[f"{c}_head"].tolist()
        rng = np.random.RandomState(int(seed))
        om = M.draw_omega(rng)
        assert list(om) == omega
        for row in g[f"{c}_draws"]:
            want = dict(zip(cols, row.tolist()))
            p = M.draw_mix_params(rng, om, dataset="nuscenes", n_partners=2)
            q = A.draw_train_params(rng)
            assert (p.prob, p.partner, p.kind, p.strategy) == tuple(int(want[k]) for k in ("prob", "partner", "kind", "strategy"))
            assert p.alpha == want["alpha"] and p.swap == bool(want["swap"]) and p.paste == bool(want["paste"])
            assert p.beta == p.alpha + np.pi or p.kind != M.POLAR
            assert not p.tail_all and not p.degrees and p.dataset == "nuscenes" and p.instance_classes == tuple(range(1, 11))
            assert p.omega == tuple(omega)
            assert (q.theta, q.scale, q.flip) == (want["theta"], want["scale"], int(want["flip"]))
            assert tuple(q.translate) == (want["noise_x"], want["noise_y"], want["noise_z"])
            seen.append((p.kind, p.swap, p.partner))
    # what the three seeds were chosen for: both kinds, the swap on and off, the other keyframe and the sample itself as partner
    assert seen == [(M.POLAR, True, 1), (M.LASER, False, 0), (M.POLAR, False, 0), (M.POLAR, True, 1), (M.POLAR, True, 0),
                    (M.POLAR, True, 1)]


def test_nuscenes_thresholds_per_strategy():
    assert M.laser_thresholds(0, True, "nuscenes") == [0.0, -10.0]
    assert M.laser_thresholds(1, True, "nuscenes") == [4.0, -2.0, -10.0]
    assert M.laser_thresholds(2, True, "nuscenes") == [4.0, 0.0, -4.0, -12.0]
    for k in range(4):
        # the defaults stay SemanticKITTI's; the recipe's `lasermix_aug` (radians against degrees) is the same in both files
        assert M.laser_thresholds(k, True) == list(M.LASER_THRESHOLDS[k]) == M.laser_thresholds(k, True, "semantickitti")
        assert M.laser_thresholds(k, False, "nuscenes") == M.laser_thresholds(k, False)
        assert M.MixParams(kind=M.LASER, strategy=k, degrees=True).dataset == "semantickitti"
    # the record: thresholds travel in fields 11 .. 16, the layout is the one ts_stage_mix knows
    p = M.MixParams(kind=M.LASER, strategy=2, degrees=True, dataset="nuscenes")
    rec, _, _ = M.pack_mix([p, M.MixParams(kind=M.LASER, strategy=2, degrees=True)], [3, 3], [2, 2])
    assert rec.shape == (2, M.RECORD) and rec[0, 10] == 1 and rec[0, 11] == 4 and rec[0, 12:17].tolist() == [4.0, 0.0, -4.0, -12.0, 0.0]
    assert rec[1, 11] == 4 and rec[1, 12:17].tolist() == [-4.0, -8.0, -12.0, -16.0, 0.0]


def test_inc6phi1_does_not_exist_on_nuscenes():
    with pytest.raises(ValueError):
        M.laser_thresholds(3, True, "nuscenes")
    with pytest.raises(ValueError):
        M.MixParams(kind=M.LASER, strategy=3, degrees=True, dataset="nuscenes")
    with pytest.raises(ValueError):
        M.lasermix_points(None, None, None, None, "inc6phi1", degrees=True, dataset="nuscenes")
    with pytest.raises(ValueError):
        M.MixParams(dataset="kitti")
    M.MixParams(kind=M.LASER, strategy=3, degrees=False, dataset="nuscenes")       # `lasermix_aug` has all four
    M.MixParams(kind=M.POLAR, strategy=3, degrees=True, dataset="nuscenes")        # (not a LaserMix record: nothing to look up)


def _laser_seed():
    return next(s for s in range(64) if int(np.random.RandomState(s).choice(2, 1)[0]) == 1)


def test_nuscenes_lasermix_aug__draws_from_a_one_element_list():
    seed = _laser_seed()
    rng, twin = np.random.RandomState(seed), np.random.RandomState(seed)
    p = M.draw_mix_params(rng, (0.1, 2.2), dataset="nuscenes", degrees=True, n_partners=5)
    assert int(twin.choice(2, 1)[0]) == 1 and int(twin.choice(5)) == p.partner
    assert int(twin.choice(1, 1)[0]) == 0                                   # LaserMix_nuscenes.py:135-136
    assert p.kind == M.LASER and p.strategy == 0 and p.degrees and p.dataset == "nuscenes"
    assert rng.random_sample() == twin.random_sample(), "the replay consumed something else"
    # the recipe's call (`lasermix_aug`, degrees=False) and SemanticKITTI's `lasermix_aug_` keep the four-element list
    for kw in (dict(dataset="nuscenes", n_partners=5), dict(degrees=True)):
        rng, twin = np.random.RandomState(seed), np.random.RandomState(seed)
        p = M.draw_mix_params(rng, (0.1, 2.2), **kw)
        twin.choice(2, 1)
        if "n_partners" in kw:
            twin.choice(5)
        assert p.strategy == int(twin.choice(4, 1)[0]) and rng.random_sample() == twin.random_sample()


def test_global_augment_l_and_p_are_honoured():
    laser, polar = _laser_seed(), next(s for s in range(64) if int(np.random.RandomState(s).choice(2, 1)[0]) == 0)
    want = {("GlobalAugment_LP", laser): M.LASER, ("GlobalAugment_LP", polar): M.POLAR, ("GlobalAugment_L", laser): M.LASER,
            ("GlobalAugment_L", polar): M.NONE, ("GlobalAugment_P", laser): M.NONE, ("GlobalAugment_P", polar): M.POLAR,
            ("none", laser): M.NONE, ("none", polar): M.NONE}
    for (augment, seed), kind in want.items():
        rng, twin = np.random.RandomState(seed), np.random.RandomState(seed)
        p = M.draw_mix_params(rng, (0.1, 2.2), augment=augment, dataset="nuscenes", n_partners=3)
        assert p.kind == kind, (augment, seed)
        # the coin and the partner are drawn whatever the switch says (nuscenes_ms.py:132-133)
        assert p.prob == int(twin.choice(2, 1)[0]) and p.partner == int(twin.choice(3))
        assert M.draw_mix_params(np.random.RandomState(seed), (0.1, 2.2), augment=augment, dataset="nuscenes", n_partners=3,
                                 training=False).kind == M.NONE


def test_stage_functions_take_mix_and_partners():
    from taseg_amd.data import nuscenes as N
    for fn in (N.build_nuscenes_batch, N.build_nuscenes_batch_per_sample):
        par = inspect.signature(fn).parameters
        assert par["mix"].default is None and par["partners"].default is None and par["aug"].default is None
        assert list(par)[:5] == ["samples", "voxel_size", "steps", "in_feature_dim", "aug"]
    assert "not yet" not in inspect.getdoc(__import__("taseg_amd.data.nuscenes_reader", fromlist=["x"]))


def test_clamp_compact_is_declared_and_bound():
    from taseg_amd import _lib
    text = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ts_stage_clamp_compact", "ts_stage_clamp_compact_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ts_stage_clamp_compact"][1]) == 15 and len(_lib.SIGNATURES["ts_stage_clamp_compact_workspace_bytes"][1]) == 2
    lib = _lib.load()
    # one int per block for the counts, one for the offsets, n_samples per block for the counts per sample; 256-byte pieces
    assert lib.ts_stage_clamp_compact_workspace_bytes(0, 1) == 256
    assert lib.ts_stage_clamp_compact_workspace_bytes(257, 4) == 3 * 256
    assert lib.ts_stage_clamp_compact_workspace_bytes(256 * 64, 64) == 256 + 256 + 64 * 64 * 4
    from taseg_amd import backend as B
    assert callable(B.stage_clamp_compact)
