"""Golden vectors of the nuScenes scan mixing (build container only; reads /root/reference).

    python tests/golden/make_golden_mix_nus.py

Runs the REAL reference functions - `polarmix` of PolarMix_nuscenes.py, `lasermix_aug` and `lasermix_aug_` of LaserMix_nuscenes.py,
then `NuscVoxelMsDataset.get_single_sample` + `collate_batch` of nuscenes_voxel_ms.py (in_feature_dim 4, voxel 0.1, all four
augmentations on) - on samples 0 and 1 of multiscan_nus.npz, which are also the partner pool (`len(self.nusc_infos)` = 2), after
`np.random.seed(seed)` with `Omega` drawn first from the same seed.  Writes multiscan_mix_nus.npz (data only): the seeds, every
value the reference DREW (the partner index included), the mixed clouds with their labels, the collated batches under the keys of
multiscan_nus.npz, and points-level cases of the three nuScenes `lasermix_aug_` strategies on the single-frame and the fused pair.
Three batches of incompressible float32 rows leave little room under the size of multiscan_mix_batch.npz, so what can be small is:
  * a mix moves rows and adds two rotated copies of a few.  A mixed cloud is stored as `*_step` - the first differences
    (np.diff(src, prepend=0)) of `src`, for every row the index of the row of concat(the sample's cloud, the partner's cloud) with
    the same bits, -1 for a row that is in neither - and `*_new`, the rows marked -1 in order (`pack_rows`, asserted to rebuild
    the cloud bit for bit; `unpack_rows` is what a test does);
  * the draws of a batch are one float64 table, `*_draws` [samples, len(DRAW_COLUMNS)] (every drawn value is a float64 or a small
    integer: nothing is rounded), beside `*_head` = seed, Omega[0], Omega[1];
  * the archive's members are LZMA-compressed (numpy.load reads them like any .npz).

What is restated and why: `NuscenesMsDataset.__getitem__` itself is not driven.  The two fixture samples come from two separate
synthetic scenes, each with info tables of its own (make_golden_r2.gen_nus), and `__getitem__` reads its partner out of the SAME
tables through `np.fromfile` and the devkit; one dataset object that holds both would be a new fixture, not multiscan_nus.npz.  So
lines :132-214 are restated in `ref_getitem_mix_nus` - the same calls, arguments and order, in the style of
make_golden_mix.ref_getitem_mix - on clouds built from the stored arrays: the sample's as `__getitem__` holds them at :131
(b*_xyzret, b*_xyzret_ms), the partner's as :136-159 build them (b*_points_cur with column 4 untouched, b*_fused_all[b*_mask]
behind it).  Everything from the mix functions on is the reference's own code.

Every case is also checked HERE, on the CPU: the recorded draws equal a replay of np.random.RandomState(seed) through draw_omega,
draw_mix_params(dataset="nuscenes", n_partners=2) and draw_train_params; the device rule restated in numpy reproduces the
reference's rows, labels and order bit for bit; no fixture row has a float64 yaw within 1e-5 rad of alpha or beta and none an
inclination within 1e-4 degrees of a band threshold; every `lasermix_aug_` case moves rows; at least one stored batch has a clamp
that removes a row and a sector that moves rows of a partner other than the sample.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_mix as GM  # noqa: E402  (arranges the reference's imports)

GA, R2, _ref_env, M, A = GM.GA, GM.R2, GM._ref_env, GM.M, GM.A

VOXEL = 0.1
SEEDS = (10, 3, 29)
CLASSES = list(M.INSTANCE_CLASSES["nuscenes"])
DRAW_COLUMNS = ("prob", "partner", "kind", "strategy", "alpha", "swap", "paste", "theta", "scale", "flip", "noise_x", "noise_y", "noise_z")


def nus_clouds(gn):
    """(samples, partners): what `__getitem__` holds at :131 for keyframe b, and what :136-159 build of it as a partner"""
    lm = gn["learning_map"]
    samples, partners = [], []
    for b in range(2):
        key = gn[f"b{b}_points_cur"]                                  # the file: column 4 as it is (:141)
        ann = lm[gn[f"b{b}_rawlabels_cur"]].reshape(-1, 1)              # :146-147
        mask = gn[f"b{b}_mask"]
        samples.append({"raw": gn[f"b{b}_xyzret"], "lab": gn[f"b{b}_labels"].reshape(-1, 1), "raw_ms": gn[f"b{b}_xyzret_ms"],
                        "lab_ms": gn[f"b{b}_labels_ms"].reshape(-1, 1)})
        partners.append({"raw": key.copy(), "lab": ann, "raw_ms": np.concatenate([key, gn[f"b{b}_fused_all"][mask]]),   # :155-156
                         "lab_ms": np.concatenate([ann, gn[f"b{b}_labels_all"][mask].reshape(-1, 1)])})
        assert np.array_equal(samples[b]["raw"][:, :4], key[:, :4]) and np.array_equal(samples[b]["lab"], ann)
        assert not samples[b]["raw"][:, 4].any() and len(partners[b]["raw_ms"]) == len(samples[b]["raw_ms"])
    return samples, partners


def pack_rows(rows, pool):
    """(src int32 [n], new float32 [k, F]) of a mixed cloud `rows` whose rows are rows of `pool` (bit for bit) or new ones"""
    rows, pool = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(pool, dtype=np.float32)
    where = {}
    for i, r in enumerate(pool):
        where.setdefault(r.tobytes(), i)
    src = np.array([where.get(r.tobytes(), -1) for r in rows], dtype=np.int32)
    new = np.ascontiguousarray(rows[src < 0])
    step = np.diff(src, prepend=0).astype(np.int32)
    assert GA.same_bits(unpack_rows(step, new, pool), rows)
    return step, new


def unpack_rows(step, new, pool):
    src = np.cumsum(step)
    rows = np.ascontiguousarray(pool, dtype=np.float32)[np.maximum(src, 0)]
    rows[src < 0] = new
    return rows


def store_clouds(out, c, e, e1, raw, lab, raw_ms, lab_ms):
    for key, rows, labels in (("raw", raw, lab), ("raw_ms", raw_ms, lab_ms)):
        out[f"{c}_{key}_step"], out[f"{c}_{key}_new"] = pack_rows(rows, np.concatenate([e[key], e1[key]], 0))
    out[f"{c}_lab"], out[f"{c}_lab_ms"] = np.asarray(lab).reshape(-1).astype(np.uint8), np.asarray(lab_ms).reshape(-1).astype(np.uint8)


def ref_getitem_mix_nus(fns, samples, partners, index, omega, augment="GlobalAugment_LP", split="train"):
    """nuscenes_ms.py:132-214: the same calls, arguments and order -> (raw, lab, raw_ms, lab_ms, kind, index_another)"""
    polarmix, lasermix_aug = fns
    e = samples[index]
    raw_data, annotated_data, raw_data_ms, annotated_data_ms = e["raw"], e["lab"], e["raw_ms"], e["lab_ms"]
    kind = M.NONE
    prob = np.random.choice(2, 1)
    index_another = np.random.choice(len(samples))
    if augment == 'GlobalAugment_LP' or augment == 'GlobalAugment_L' or augment == 'GlobalAugment_P':
        if split == 'train' and (augment == 'GlobalAugment_LP' or augment == 'GlobalAugment_L') and prob == 1:
            e1 = partners[index_another]
            raw_data, annotated_data, strategy = lasermix_aug(raw_data, annotated_data, e1["raw"], e1["lab"], return_strategy=True)
            raw_data_ms, annotated_data_ms, strategy_ms = lasermix_aug(raw_data_ms, annotated_data_ms, e1["raw_ms"], e1["lab_ms"],
                                                                       strategy=strategy, return_strategy=True)
            assert strategy == strategy_ms
            kind = M.LASER
        elif split == 'train' and (augment == 'GlobalAugment_LP' or augment == 'GlobalAugment_P') and prob == 0:
            e1 = partners[index_another]
            alpha = (np.random.random() - 1) * np.pi
            beta = alpha + np.pi
            raw_data, annotated_data, swap_flag, rotate_flag = polarmix(
                raw_data, annotated_data.reshape(-1), e1["raw"], e1["lab"].reshape(-1), alpha=alpha, beta=beta,
                instance_classes=CLASSES, Omega=omega, return_strategy=True)
            annotated_data = annotated_data.reshape(-1, 1)
            raw_data_ms, annotated_data_ms, swap_flag_ms, rotate_flag_ms = polarmix(
                raw_data_ms, annotated_data_ms.reshape(-1), e1["raw_ms"], e1["lab_ms"].reshape(-1), alpha=alpha, beta=beta,
                instance_classes=CLASSES, Omega=omega, swap_flag=swap_flag, rotate_flag=rotate_flag, return_strategy=True)
            annotated_data_ms = annotated_data_ms.reshape(-1, 1)
            assert swap_flag == swap_flag_ms and rotate_flag == rotate_flag_ms
            kind = M.POLAR
    # :216-222: the labels leave as uint8, the clouds as they are (the voxel dataset casts its columns to float32)
    return raw_data, annotated_data.astype(np.uint8), raw_data_ms, annotated_data_ms.astype(np.uint8), kind, int(index_another)


def device_rule(pts1, lab1, pts2, lab2, p):
    """ts_stage_mix restated in numpy for one job: make_golden_mix.device_rule, the bands of a LaserMix record from the
    dataset-aware table"""
    if p.kind != M.LASER:
        return GM.device_rule(pts1, lab1, pts2, lab2, p)
    pts1, pts2 = np.ascontiguousarray(pts1, dtype=np.float32), np.ascontiguousarray(pts2, dtype=np.float32)
    lab1, lab2 = np.asarray(lab1).reshape(-1).astype(np.int64), np.asarray(lab2).reshape(-1).astype(np.int64)
    thr = M.laser_thresholds(p.strategy, p.degrees, p.dataset)

    def bands(pts):
        return sum((inclination(pts, p.degrees) <= t).astype(np.int64) for t in thr)
    b1, b2 = bands(pts1), bands(pts2)
    out, lab = [], []
    for j in range(len(thr) + 1):
        src, l, b = (pts1, lab1, b1) if j % 2 == 0 else (pts2, lab2, b2)
        out.append(src[b == j])
        lab.append(l[b == j])
    return np.concatenate(out, 0), np.concatenate(lab, 0)


def inclination(pts, degrees):
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    inc = np.arctan2(z, np.sqrt(x * x + y * y))
    return inc / np.pi * 180 if degrees else inc


def check_margins(clouds, p):
    """no row of the fixture clouds sits at a bound of the rule -> the smallest gap (inf where the rule has no bound)"""
    gap = np.inf
    for pts in clouds:
        if p.kind == M.POLAR and p.swap:
            yaw = -np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))
            g = min(np.abs(yaw - p.alpha).min(), np.abs(yaw - p.beta).min())
            assert g > GM.YAW_MARGIN, ("yaw at a bound", g)
            gap = min(gap, g)
        if p.kind == M.LASER and p.degrees:
            inc = inclination(pts, True)
            g = min(np.abs(inc - t).min() for t in M.laser_thresholds(p.strategy, True, p.dataset))
            assert g > GM.INC_MARGIN, ("inclination at a threshold", g)
            gap = min(gap, g)
    return gap


def check_pair(c, e, e1, p, got):
    raw, lab, raw_ms, lab_ms = got
    gap = check_margins([e["raw"], e1["raw"], e["raw_ms"], e1["raw_ms"]], p)
    GM.same_rows(device_rule(e["raw"], e["lab"], e1["raw"], e1["lab"], p), (raw, lab), (c, "single"))
    GM.same_rows(device_rule(e["raw_ms"], e["lab_ms"], e1["raw_ms"], e1["lab_ms"], p), (raw_ms, lab_ms), (c, "fused"))
    return gap


def check_replay(log, mix, aug):
    """the recorded draws == what draw_mix_params(dataset="nuscenes", n_partners=2) and draw_train_params took from RandomState(seed)"""
    it = iter(log)
    for p, q in zip(mix, aug):
        name, _, v = next(it)
        assert name == "choice" and int(v[0]) == p.prob, (name, v, p.prob)
        name, a, v = next(it)
        assert name == "choice" and a[0] == 2 and int(v) == p.partner, (name, a, v, p.partner)
        if p.kind == M.LASER:
            name, a, v = next(it)
            assert name == "choice" and list(a[0]) == list(M.STRATEGIES) and v[0] == M.STRATEGIES[p.strategy]
        if p.kind == M.POLAR:
            name, _, v = next(it)
            assert name == "random" and float((v - 1) * np.pi) == p.alpha
            name, _, v = next(it)
            assert name == "random" and bool(v < 0.5) == p.swap
            name, _, v = next(it)
            assert name == "random" and p.paste
        for want in (q.theta, q.scale):
            name, _, v = next(it)
            assert name == "uniform" and float(v) == want
        name, _, v = next(it)
        assert name == "choice" and int(v[0]) == q.flip
        for k in range(3):
            name, _, v = next(it)
            assert name == "normal" and float(v[0]) == q.translate[k]
    assert next(it, None) is None, "the reference drew more than the replay"


class MixedFrames(list):
    """the frame reader of the voxel dataset: entry b is mixed with its drawn partner when it is read, as `__getitem__` does"""

    def __init__(self, fns, samples, partners, omega, seen):
        super().__init__(samples)
        self.fns, self.partners, self.omega, self.seen = fns, partners, omega, seen

    def __getitem__(self, b):
        raw, lab, raw_ms, lab_ms, kind, other = ref_getitem_mix_nus(self.fns, list(self), self.partners, b, self.omega)
        self.seen.append((b, np.array(raw), lab.copy(), np.array(raw_ms), lab_ms.copy(), kind, other))
        return {"xyzret": raw, "labels": lab, "path": f"s{b}", "xyzret_ms": raw_ms, "labels_ms": lab_ms}


def gen(gn, fname="multiscan_mix_nus.npz"):
    _ref_env.setup_datasets()
    R2._install_pyquaternion()
    _ref_env._pkg("pcseg.data.dataset.nuscenes", os.path.join(_ref_env.REF, "pcseg", "data", "dataset", "nuscenes"))
    for name in ("float", "bool"):
        if not hasattr(np, name):
            setattr(np, name, float if name == "float" else bool)        # aliases numpy >= 1.24 dropped
    from pcseg.data.dataset.nuscenes.PolarMix_nuscenes import polarmix
    from pcseg.data.dataset.nuscenes.LaserMix_nuscenes import lasermix_aug, lasermix_aug_
    from pcseg.data.dataset.nuscenes.nuscenes_voxel_ms import NuscVoxelMsDataset
    samples, partners = nus_clouds(gn)
    out = {"backend": np.array(R2.BACKEND_DESC), "cases": np.array([f"batch_s{s}" for s in SEEDS]),
           "draw_columns": np.array(DRAW_COLUMNS),
           "laser_cases": np.array([f"lasernus_{k}" for k in range(len(M.LASER_THRESHOLDS_NUSCENES))]),
           # per case: the sample, its partner, the strategy
           "laser_meta": np.array([[k % 2, 1 - k % 2, k] for k in range(len(M.LASER_THRESHOLDS_NUSCENES))])}
    # 1. `lasermix_aug_` of the nuScenes file, every strategy it has, on the single-frame pair and on the fused pair
    for k in range(len(M.LASER_THRESHOLDS_NUSCENES)):
        c, b = f"lasernus_{k}", k % 2
        e, e1 = samples[b], partners[1 - b]
        p = M.MixParams(kind=M.LASER, strategy=k, degrees=True, dataset="nuscenes", tail_all=False, instance_classes=CLASSES)
        raw, lab = lasermix_aug_(e["raw"], e["lab"], e1["raw"], e1["lab"], strategy=M.STRATEGIES[k])
        raw_ms, lab_ms = lasermix_aug_(e["raw_ms"], e["lab_ms"], e1["raw_ms"], e1["lab_ms"], strategy=M.STRATEGIES[k])
        gap = check_pair(c, e, e1, p, (raw, lab, raw_ms, lab_ms))
        for got, src in ((raw, e["raw"]), (raw_ms, e["raw_ms"])):
            assert len(got) and not GA.same_bits(np.ascontiguousarray(got, dtype=np.float32), src), "the strategy must move rows"
        store_clouds(out, c, e, e1, raw, lab, raw_ms, lab_ms)
        print(c, "rows", len(raw), len(raw_ms), "smallest inclination gap %.2e deg" % gap)
    # (inc6phi1: no branch of the nuScenes `lasermix_aug_` takes it - it would hand back its stale global `xyzil_mix_1`, :119)
    with GM.Draws() as d:                 # the strategy draw of the nuScenes `lasermix_aug_`: a one-element list (:135-136)
        np.random.seed(0)
        lasermix_aug_(samples[0]["raw"], samples[0]["lab"], partners[1]["raw"], partners[1]["lab"])
    assert [(n, list(a[0])) for n, a, _ in d.log] == [("choice", ["inc3phi1"])]
    # 2. whole training batches: mix + all four augmentations
    kinds, shows = [], False
    for seed in SEEDS:
        c = f"batch_s{seed}"
        np.random.seed(seed)
        omega = GM.global_omega()
        seen = []
        vox = GA.make_vox(NuscVoxelMsDataset, [], 4, VOXEL, True)
        vox.point_cloud_dataset = MixedFrames((polarmix, lasermix_aug), samples, partners, omega, seen)
        with GM.Draws() as d:
            got = [vox.get_single_sample(b) for b in (0, 1)]
        rng = np.random.RandomState(seed)
        om = M.draw_omega(rng)
        assert list(om) == omega
        mix, aug = [], []
        for _ in range(2):
            mix.append(M.draw_mix_params(rng, om, dataset="nuscenes", n_partners=2))
            aug.append(A.draw_train_params(rng))
        check_replay(d.log, mix, aug)
        gaps = []
        for (b, raw, lab, raw_ms, lab_ms, kind, other), p, s in zip(seen, mix, got):
            assert kind == p.kind and other == p.partner and not p.tail_all and not p.degrees
            e, e1 = samples[b], partners[other]
            gaps.append(check_pair(c, e, e1, p, (raw, lab, raw_ms, lab_ms)))
            store_clouds(out, f"{c}_s{b}", e, e1, raw, lab, raw_ms, lab_ms)
            clamped = int(s["num_points_ms"][0]) < len(raw_ms)
            if p.kind == M.POLAR and p.swap and other != b and clamped:
                yaw = -np.arctan2(e1["raw_ms"][:, 1].astype(np.float64), e1["raw_ms"][:, 0].astype(np.float64))
                shows = shows or bool(((yaw > p.alpha) & (yaw < p.beta)).any())
        kinds.append([(p.kind, p.swap, p.partner) for p in mix])
        out[f"{c}_head"] = np.array([seed, *omega], dtype=np.float64)
        out[f"{c}_draws"] = np.array([[p.prob, p.partner, p.kind, p.strategy, p.alpha, p.swap, p.paste, q.theta, q.scale, q.flip,
                                       *q.translate] for p, q in zip(mix, aug)], dtype=np.float64)
        out.update(GA.dump_batch(f"{c}_batch_", NuscVoxelMsDataset.collate_batch(got)))
        print(c, "kind / swap / partner", kinds[-1], "smallest yaw gap %.2e rad" % min(gaps))
    assert shows, "no batch with a clamp that removes a row and a sector of another keyframe"
    assert {k for ks in kinds for k, _, _ in ks} == {M.LASER, M.POLAR}
    with zipfile.ZipFile(os.path.join(HERE, fname), "w", compression=zipfile.ZIP_LZMA) as z:
        for key, value in out.items():
            with z.open(key + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(value), allow_pickle=False)
    back = np.load(os.path.join(HERE, fname), allow_pickle=False)
    assert sorted(back.files) == sorted(out) and all(np.array_equal(back[k], out[k]) for k in out)
    size, limit = os.path.getsize(os.path.join(HERE, fname)), os.path.getsize(os.path.join(HERE, "multiscan_mix_batch.npz"))
    print(fname, size // 1024, "KiB (multiscan_mix_batch.npz:", limit // 1024, "KiB)")
    assert size <= limit


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    gen(dict(np.load(os.path.join(HERE, "multiscan_nus.npz"), allow_pickle=False)))
