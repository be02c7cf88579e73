"""Golden vectors of the scan mixing - PolarMix and LaserMix (build container only; reads /root/reference).

    python tests/golden/make_golden_mix.py

Runs the REAL reference functions - `polarmix` of PolarMix_semantickitti.py / PolarMix_nuscenes.py, `lasermix_aug` and
`lasermix_aug_` of LaserMix_semantickitti.py, in the order and with the arguments of `SemantickittiMsDataset.__getitem__`
(semantickitti_ms.py:151-237), then `get_single_sample` + `collate_batch` of semantickitti_voxel_ms.py - on the clouds already
stored in multiscan.npz (samples 0 and 1 as each other's partners) and multiscan_nus.npz, after `np.random.seed(seed)` with
`Omega` drawn first from the same seed.  Stored (data only): the seeds, the values the reference DREW, the mixed clouds with their
labels and the collated batches under the keys of multiscan.npz.

  multiscan_mix.npz        PolarMix without the swap (seed 3) and with it (seed 2), paste on; swap on / paste off through the
                           explicit flags; the reference's LaserMix branch (the identity); `lasermix_aug_` for all four strategies;
                           one nuScenes PolarMix on 5- and 4-column rows
  multiscan_mix_batch.npz  full training batches of two samples: mix + all four augmentations

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through taseg_amd.data.mix.draw_mix_params
(and draw_train_params) gives the recorded draws; the device rule restated in numpy (`device_rule`: float64 atan2 rounded to
float32 against float32 bounds, stable partition, the rotation of make_golden_aug.formula) reproduces the reference's rows, labels
and order bit for bit; no fixture row has a float64 yaw within 1e-5 rad of alpha or beta and none an inclination within 1e-4
degrees of a band threshold, so the one permitted difference - a row at a bound - cannot occur on them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_aug as GA  # noqa: E402  (arranges the reference's imports)

R2, _ref_env = GA.R2, GA._ref_env
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402

VOXEL = 0.05
YAW_MARGIN, INC_MARGIN = 1e-5, 1e-4


class Draws(GA.Draws):
    """... of the four generator functions the mix and the augmentation use"""

    def __enter__(self):
        self.log, self.real = [], {n: getattr(np.random, n) for n in ("uniform", "choice", "normal", "random")}
        for name, fn in self.real.items():
            setattr(np.random, name, self._wrap(name, fn))
        return self


def global_omega():
    """semantickitti_ms.py:14, from numpy's global generator"""
    return [np.random.random() * np.pi * 2 / 3, (np.random.random() + 1) * np.pi * 2 / 3]


def ref_getitem_mix(fns, e, e1, omega, classes, augment="GlobalAugment_LP"):
    """the mix of semantickitti_ms.py:151-237: the same calls, arguments and order, on a sample `e` and its partner `e1`
    (dicts raw [n, 4], lab [n, 1], raw_ms [m, 5], lab_ms [m, 1]) -> (raw, lab, raw_ms, lab_ms, kind)"""
    polarmix, lasermix_aug = fns
    raw, lab, raw_ms, lab_ms = e["raw"], e["lab"], e["raw_ms"], e["lab_ms"]
    kind = M.NONE
    prob = np.random.choice(2, 1)
    if augment == "GlobalAugment_LP":
        if prob == 1:
            raw, lab, strategy = lasermix_aug(raw, lab, e1["raw"], e1["lab"], return_strategy=True)
            raw_ms, lab_ms, strategy_ms = lasermix_aug(raw_ms, lab_ms, e1["raw_ms"], e1["lab_ms"], strategy=strategy,
                                                       return_strategy=True)
            assert strategy == strategy_ms
            kind = M.LASER
        elif prob == 0:
            alpha = (np.random.random() - 1) * np.pi
            beta = alpha + np.pi
            raw, lab, swap_flag, rotate_flag = polarmix(raw, lab.reshape(-1), e1["raw"], e1["lab"].reshape(-1), alpha=alpha,
                                                        beta=beta, instance_classes=classes, Omega=omega, return_strategy=True)
            lab = lab.reshape(-1, 1)
            raw_ms, lab_ms, _, _ = polarmix(raw_ms, lab_ms.reshape(-1), e1["raw_ms"], e1["lab_ms"].reshape(-1), alpha=alpha,
                                            beta=beta, instance_classes=classes, Omega=omega, swap_flag=swap_flag,
                                            rotate_flag=rotate_flag, return_strategy=True)
            lab_ms = lab_ms.reshape(-1, 1)
            kind = M.POLAR
    # :240-247: the concatenation with the ring id casts to float32, the labels to uint8
    return raw.astype(np.float32), lab.astype(np.uint8), raw_ms.astype(np.float32), lab_ms.astype(np.uint8), kind


def rotate(xyz32, omega):
    return GA.formula(xyz32, A.AugParams(c=float(np.cos(omega)), s=float(np.sin(omega)), rotate_on=True))


def device_rule(pts1, lab1, pts2, lab2, p):
    """ts_stage_mix restated in numpy (include/taseg_hip.h) for one job -> (points, labels)"""
    pts1, pts2 = np.ascontiguousarray(pts1, dtype=np.float32), np.ascontiguousarray(pts2, dtype=np.float32)
    lab1, lab2 = np.asarray(lab1).reshape(-1).astype(np.int64), np.asarray(lab2).reshape(-1).astype(np.int64)
    if p.kind == M.NONE:
        return pts1.copy(), lab1.copy()
    if p.kind == M.POLAR:
        def sector(pts):
            yaw = (-np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))).astype(np.float32)
            return (yaw > np.float32(p.alpha)) & (yaw < np.float32(p.beta)) if p.swap else np.zeros(len(pts), dtype=bool)
        out, lab = [pts1[~sector(pts1)], pts2[sector(pts2)]], [lab1[~sector(pts1)], lab2[sector(pts2)]]
        if p.paste:
            order = np.concatenate([np.nonzero(lab2 == c)[0] for c in p.instance_classes]).astype(np.int64)
            inst = pts2[order]
            out.append(inst)
            lab.append(lab2[order])
            for omega in p.omega:
                new = np.zeros_like(inst)
                if len(inst):
                    new[:, :3] = rotate(np.ascontiguousarray(inst[:, :3]), omega)
                if p.tail_all:
                    new[:, 3:] = inst[:, 3:]
                else:
                    new[:, 3:4] = inst[:, 3:4]
                out.append(new)
                lab.append(lab2[order])
        return np.concatenate(out, 0), np.concatenate(lab, 0)
    thr = M.laser_thresholds(p.strategy, p.degrees)

    def bands(pts):
        x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
        inc = np.arctan2(z, np.sqrt(x * x + y * y))
        if p.degrees:
            inc = inc / np.pi * 180
        return sum((inc <= t).astype(np.int64) for t in thr)
    b1, b2 = bands(pts1), bands(pts2)
    out, lab = [], []
    for j in range(len(thr) + 1):
        src, l, b = (pts1, lab1, b1) if j % 2 == 0 else (pts2, lab2, b2)
        out.append(src[b == j])
        lab.append(l[b == j])
    return np.concatenate(out, 0), np.concatenate(lab, 0)


def check_margins(clouds, p):
    """no row of the fixture clouds sits at a bound of the rule"""
    for pts in clouds:
        x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
        if p.kind == M.POLAR and p.swap:
            yaw = -np.arctan2(y, x)
            gap = min(np.abs(yaw - p.alpha).min(), np.abs(yaw - p.beta).min())
            assert gap > YAW_MARGIN, ("yaw at a bound", gap)
        if p.kind == M.LASER and p.degrees:
            inc = np.arctan2(z, np.sqrt(x * x + y * y)) / np.pi * 180
            gap = min(np.abs(inc - t).min() for t in M.laser_thresholds(p.strategy, True))
            assert gap > INC_MARGIN, ("inclination at a threshold", gap)


def same_rows(got, want, what):
    (gp, gl), (wp, wl) = got, want
    wp = np.ascontiguousarray(wp, dtype=np.float32)
    assert GA.same_bits(np.ascontiguousarray(gp), wp), (what, "rows")
    assert np.array_equal(gl.reshape(-1), np.asarray(wl).reshape(-1).astype(np.int64)), (what, "labels")


def check_replay(log, mix, aug=None):
    """the recorded draws == what draw_mix_params (and draw_train_params) took from RandomState(seed), Omega first"""
    it = iter(log)
    for i, p in enumerate(mix):
        name, _, v = next(it)
        assert name == "choice" and int(v[0]) == p.prob, (name, v, p.prob)
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
        if aug is not None:
            q = aug[i]
            for want in (q.theta, q.scale):
                name, _, v = next(it)
                assert name == "uniform" and float(v) == want
            name, _, v = next(it)
            assert name == "choice" and int(v[0]) == q.flip
            for k in range(3):
                name, _, v = next(it)
                assert name == "normal" and float(v[0]) == q.translate[k]
    assert next(it, None) is None, "the reference drew more than the replay"


def store_mix(out, c, seed, omega, mix):
    out[f"{c}_seed"] = np.array(seed)
    out[f"{c}_omega"] = np.array(omega, dtype=np.float64)
    out[f"{c}_kind"] = np.array([p.kind for p in mix])
    out[f"{c}_prob"] = np.array([p.prob for p in mix])
    out[f"{c}_strategy"] = np.array([p.strategy for p in mix])
    out[f"{c}_alpha"] = np.array([p.alpha for p in mix], dtype=np.float64)
    out[f"{c}_swap"] = np.array([p.swap for p in mix])
    out[f"{c}_paste"] = np.array([p.paste for p in mix])


def store_clouds(out, c, raw, lab, raw_ms, lab_ms):
    out[f"{c}_raw"], out[f"{c}_lab"] = np.ascontiguousarray(raw, dtype=np.float32), np.asarray(lab).reshape(-1).astype(np.uint8)
    out[f"{c}_raw_ms"] = np.ascontiguousarray(raw_ms, dtype=np.float32)
    out[f"{c}_lab_ms"] = np.asarray(lab_ms).reshape(-1).astype(np.uint8)


def kitti_inputs(g):
    """what `__getitem__` holds at :151 for samples 0 and 1 of multiscan.npz"""
    lm, T = g["learning_map"], int(g["T"])
    return [{"raw": g[f"b{b}_points_t{T}"], "lab": lm[g[f"b{b}_rawlabels_t{T}"] & 0xFFFF].reshape(-1, 1),
             "raw_ms": g[f"b{b}_raw_data_ms"], "lab_ms": g[f"b{b}_labels_ms"].reshape(-1, 1)} for b in range(2)]


def check_pair(c, e, e1, p, got):
    """the device rule on both pairs == the reference; margins"""
    raw, lab, raw_ms, lab_ms = got
    check_margins([e["raw"], e1["raw"], e["raw_ms"], e1["raw_ms"]], p)
    same_rows(device_rule(e["raw"], e["lab"], e1["raw"], e1["lab"], p), (raw, lab), (c, "single"))
    same_rows(device_rule(e["raw_ms"], e["lab_ms"], e1["raw_ms"], e1["lab_ms"], p), (raw_ms, lab_ms), (c, "fused"))


def seeded_case(out, c, fns, ins, seed, b, want_kind, want_swap=None):
    np.random.seed(seed)
    omega = global_omega()
    with Draws() as d:
        got = ref_getitem_mix(fns, ins[b], ins[1 - b], omega, list(M.INSTANCE_CLASSES["semantickitti"]))
    rng = np.random.RandomState(seed)
    om = M.draw_omega(rng)
    assert list(om) == omega
    p = M.draw_mix_params(rng, om)
    check_replay(d.log, [p])
    assert p.kind == got[4] == want_kind and (want_swap is None or p.swap == want_swap), (c, p)
    check_pair(c, ins[b], ins[1 - b], p, got[:4])
    store_mix(out, c, seed, omega, [p])
    out[f"{c}_sample"] = np.array(b)
    store_clouds(out, c, *got[:4])
    return p


def gen_points(g, fname="multiscan_mix.npz"):
    _ref_env.setup_datasets()
    from pcseg.data.dataset.semantickitti.PolarMix_semantickitti import polarmix
    from pcseg.data.dataset.semantickitti.LaserMix_semantickitti import lasermix_aug, lasermix_aug_
    fns = (polarmix, lasermix_aug)
    ins = kitti_inputs(g)
    out = {"backend": np.array(R2.BACKEND_DESC)}
    seeded_case(out, "polar_s3", fns, ins, 3, 0, M.POLAR, want_swap=False)
    p2 = seeded_case(out, "polar_s2", fns, ins, 2, 1, M.POLAR, want_swap=True)
    # the reference's LaserMix branch: the first seed from 4 whose coin says LaserMix; the identity
    seed = next(s for s in range(4, 64) if M.draw_mix_params(_after_omega(s), (0.0, 0.0)).kind == M.LASER)
    seeded_case(out, "laser_ref", fns, ins, seed, 0, M.LASER)
    assert GA.same_bits(out["laser_ref_raw"], ins[0]["raw"]) and GA.same_bits(out["laser_ref_raw_ms"], ins[0]["raw_ms"])
    # paste off (and the swap on) through the explicit flags, the bounds of polar_s2
    c, e, e1 = "polar_nopaste", ins[0], ins[1]
    p = M.MixParams(kind=M.POLAR, alpha=p2.alpha, beta=p2.beta, swap=True, paste=False, omega=p2.omega)
    cls = list(p.instance_classes)
    raw, lab = polarmix(e["raw"], e["lab"].reshape(-1), e1["raw"], e1["lab"].reshape(-1), p.alpha, p.beta, cls, list(p.omega),
                        swap_flag=True, rotate_flag=False)
    raw_ms, lab_ms = polarmix(e["raw_ms"], e["lab_ms"].reshape(-1), e1["raw_ms"], e1["lab_ms"].reshape(-1), p.alpha, p.beta, cls,
                              list(p.omega), swap_flag=True, rotate_flag=False)
    check_pair(c, e, e1, p, (raw, lab, raw_ms, lab_ms))
    store_mix(out, c, -1, p.omega, [p])
    out[f"{c}_sample"] = np.array(0)
    store_clouds(out, c, raw, lab, raw_ms, lab_ms)
    # LaserMix as it was meant: lasermix_aug_ for all four strategies
    for k, name in enumerate(M.STRATEGIES):
        c, b = f"laserdeg_{k}", k % 2
        e, e1 = ins[b], ins[1 - b]
        p = M.MixParams(kind=M.LASER, strategy=k, degrees=True)
        raw, lab = lasermix_aug_(e["raw"], e["lab"], e1["raw"], e1["lab"], strategy=name)
        raw_ms, lab_ms = lasermix_aug_(e["raw_ms"], e["lab_ms"], e1["raw_ms"], e1["lab_ms"], strategy=name)
        check_pair(c, e, e1, p, (raw, lab, raw_ms, lab_ms))
        assert len(raw) and not GA.same_bits(raw.astype(np.float32), e["raw"]), "the strategy must move rows"
        store_mix(out, c, -1, p.omega, [p])
        out[f"{c}_sample"] = np.array(b)
        store_clouds(out, c, raw, lab, raw_ms, lab_ms)
    # nuScenes: the class list 1 .. 10 and the tail rule (only column 3 reaches the rotated copies) on 5- and 4-column rows
    _ref_env._pkg("pcseg.data.dataset.nuscenes", os.path.join(_ref_env.REF, "pcseg", "data", "dataset", "nuscenes"))
    from pcseg.data.dataset.nuscenes.PolarMix_nuscenes import polarmix as polarmix_nus
    gn = dict(np.load(os.path.join(HERE, "multiscan_nus.npz"), allow_pickle=False))
    seed = 2
    np.random.seed(seed)
    omega = global_omega()
    rng = np.random.RandomState(seed)
    om = M.draw_omega(rng)
    c = "nus_polar"
    with Draws() as d:
        prob = np.random.choice(2, 1)
        partner = np.random.choice(2)                  # nuscenes_ms.py:133
        assert prob == 0
        alpha = (np.random.random() - 1) * np.pi
        beta = alpha + np.pi
        cls = list(M.INSTANCE_CLASSES["nuscenes"])
        raw, lab, swap_flag, rotate_flag = polarmix_nus(gn["b0_xyzret"], gn["b0_labels"], gn["b1_xyzret"], gn["b1_labels"],
                                                        alpha=alpha, beta=beta, instance_classes=cls, Omega=omega,
                                                        return_strategy=True)
    p = M.draw_mix_params(rng, om, dataset="nuscenes", n_partners=2)
    assert p.kind == M.POLAR and p.alpha == alpha and p.swap == swap_flag and p.paste == rotate_flag and p.partner == partner
    assert not p.tail_all and [n for n, _, _ in d.log] == ["choice", "choice", "random", "random", "random"]
    raw_ms, lab_ms = polarmix_nus(gn["b0_xyzret_ms"], gn["b0_labels_ms"], gn["b1_xyzret_ms"], gn["b1_labels_ms"], alpha=alpha,
                                  beta=beta, instance_classes=cls, Omega=omega, swap_flag=swap_flag, rotate_flag=rotate_flag)
    raw4, lab4 = polarmix_nus(gn["b0_xyzret"][:, :4], gn["b0_labels"], gn["b1_xyzret"][:, :4], gn["b1_labels"], alpha=alpha,
                              beta=beta, instance_classes=cls, Omega=omega, swap_flag=swap_flag, rotate_flag=rotate_flag)
    e = {"raw": gn["b0_xyzret"], "lab": gn["b0_labels"], "raw_ms": gn["b0_xyzret_ms"], "lab_ms": gn["b0_labels_ms"]}
    e1 = {"raw": gn["b1_xyzret"], "lab": gn["b1_labels"], "raw_ms": gn["b1_xyzret_ms"], "lab_ms": gn["b1_labels_ms"]}
    check_pair(c, e, e1, p, (raw, lab, raw_ms, lab_ms))
    same_rows(device_rule(e["raw"][:, :4], e["lab"], e1["raw"][:, :4], e1["lab"], p), (raw4, lab4), (c, "4 columns"))
    # (the fused rows carry the sweep's time lag in column 4: the rotated copies lose it)
    inst = np.isin(gn["b1_labels_ms"], cls)
    n_inst = int(inst.sum())
    assert n_inst > 0 and not np.any(raw_ms[-2 * n_inst:, 4]) and np.any(gn["b1_xyzret_ms"][inst, 4]), \
        "the fixture must show the zero tail of the rotated copies"
    store_mix(out, c, seed, omega, [p])
    out[f"{c}_partner"] = np.array(p.partner)
    store_clouds(out, c, raw, lab, raw_ms, lab_ms)
    out[f"{c}_raw4"], out[f"{c}_lab4"] = np.ascontiguousarray(raw4), lab4.astype(np.uint8)
    out["cases"] = np.array(["polar_s3", "polar_s2", "laser_ref", "polar_nopaste"] + [f"laserdeg_{k}" for k in range(4)])
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; cases", out["cases"].tolist(), "+ nus_polar")


def _after_omega(seed):
    rng = np.random.RandomState(seed)
    M.draw_omega(rng)
    return rng


class MixedFrames(list):
    """the frame reader of the voxel dataset: entry i is mixed with its partner when it is read, as `__getitem__` does"""

    def __init__(self, fns, ins, omega, seen):
        super().__init__(ins)
        self.fns, self.omega, self.seen = fns, omega, seen

    def __getitem__(self, b):
        raw, lab, raw_ms, lab_ms, kind = ref_getitem_mix(self.fns, list.__getitem__(self, b), list.__getitem__(self, 1 - b),
                                                         self.omega, list(M.INSTANCE_CLASSES["semantickitti"]))
        self.seen.append((b, raw.copy(), lab.copy(), raw_ms.copy(), lab_ms.copy(), kind))   # the voxel dataset augments in place
        return {"xyzret": raw, "labels": lab, "path": f"/data/sequences/00/velodyne/{b:06d}.bin", "xyzret_ms": raw_ms,
                "labels_ms": lab_ms}


def gen_batches(g, seeds, fname="multiscan_mix_batch.npz"):
    _, SemVoxMs, _ = _ref_env.setup_datasets()
    from pcseg.data.dataset.semantickitti.PolarMix_semantickitti import polarmix
    from pcseg.data.dataset.semantickitti.LaserMix_semantickitti import lasermix_aug
    ins = kitti_inputs(g)
    out = {"backend": np.array(R2.BACKEND_DESC), "cases": np.array([f"batch_s{s}" for s in seeds])}
    kinds = []
    for seed in seeds:
        c = f"batch_s{seed}"
        np.random.seed(seed)
        omega = global_omega()
        seen = []
        vox = GA.make_vox(SemVoxMs, [], 5, VOXEL, True)
        vox.point_cloud_dataset = MixedFrames((polarmix, lasermix_aug), ins, omega, seen)
        with Draws() as d:
            samples = [vox.get_single_sample(b) for b in (0, 1)]
        rng = np.random.RandomState(seed)
        om = M.draw_omega(rng)
        mix, aug = [], []
        for _ in range(2):
            mix.append(M.draw_mix_params(rng, om))
            aug.append(A.draw_train_params(rng))
        check_replay(d.log, mix, aug)
        for (b, raw, lab, raw_ms, lab_ms, kind), p in zip(seen, mix):
            assert kind == p.kind
            check_pair(c, ins[b], ins[1 - b], p, (raw, lab, raw_ms, lab_ms))
        kinds.append([p.kind for p in mix])
        store_mix(out, c, seed, omega, mix)
        GA.store_params(out, c, aug)
        out.update(GA.dump_batch(f"{c}_batch_", SemVoxMs.collate_batch(samples)))
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; kinds", kinds)


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    g = dict(np.load(os.path.join(HERE, "multiscan.npz"), allow_pickle=False))
    gen_points(g)
    gen_batches(g, [2, 9])
