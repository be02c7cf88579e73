"""Golden vectors of the SMSA recipe's moving-object augmentation (build container only: it runs the reference, which
_ref_env locates; nothing here is imported by the tests or the product).

    python tests/golden/make_golden_moving.py

Runs the REAL reference code of pcseg/data/dataset/semantickitti/semantickitti_ms_ms.py on small synthetic clouds with full
uint32 labels (a current scan of about 3 000 rows and four history scans with poses, read through a patched `np.fromfile`):

  moving.npz        `multiscan_fuse`, then `static2moving` and `moving2static` on a bare `SemantickittiMsMsDataset` object carrying
                    `maug_prob`, `shift_*_range`, `multiscan`, `step`, `only_history`, after `np.random.seed(seed)`, for several
                    seeds per cloud.  Stored (data only): the scans, labels and poses; the fused history, its class-step mask and
                    frame offsets; the statistics numpy gives for every candidate (counts, extents, means); per case the values
                    drawn and the rows and raw classes that differ from the input after each pass; the reference's 26-class map
                    as a 260-entry array.
  moving_batch.npz  full training batches of the two clouds as each other's partners: the whole `__getitem__` (:127-303: both
                    passes, the mix with the partner's passes, `append_time_flag`), then `get_single_sample` + `collate_batch`
                    of semantickitti_voxel_ms_ms.py with all four augmentations, under the keys of multiscan.npz.  (The ring-id
                    column `__getitem__` appends is cut off again, as in the other stage fixtures.)

Cloud `a` holds, by construction and ASSERTED here on what the reference did: a class-18 instance longer in x with center_y > 4,
one with center_y < -2, one in between; a class-20 instance longer in y; an instance with equal extents (one history row); an
instance absent from history; a class-253 instance with 19 current rows and one with 20; a class-255 instance with no row at frame
offset -1 (a NaN shift); two instances sharing the instance bits under different classes; a full label >= 2^31; an instance that
only the history holds (no candidate: untouched).  The seeds are the first ones under which, together, every branch is taken.

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through taseg_amd.data.moving's draw functions
on the stored statistics gives the recorded draws (the partner's place in the order included); the plain-Python pairwise mean
(`moving.numpy_mean`, the rule of ts_stage_moving_stats) equals numpy's `.mean()` on every instance; the device rule restated in
numpy (`device_rule`) reproduces the reference's rows and raw classes bit for bit (NaN rows at the same places); no `center_y` lies
within 1e-3 of 4 or -2.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_mix as GM  # noqa: E402  (arranges the reference's imports)

GA, R2, _ref_env = GM.GA, GM.R2, GM._ref_env
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import moving as MV  # noqa: E402
from taseg_amd.data.synthetic import synth_pose, synth_scan  # noqa: E402

VOXEL, T = 0.05, 4
STEPS = [0, 0, 2, 2, 2, 2, 2, 2, 2, 0, 4, 4, 4, 0, 4, 0, 2, 4, 2, 2]            # FLEXIBLE_STEPS of minkunet_mk34_cr10_smsa.yaml
MAUG_PROB, SHIFT_X_RANGE, SHIFT_Y_RANGE = 4, 4.0, 4.0
CENTER_MARGIN = 1e-3
BIG = 0x8001                                             # instance bits of the label >= 2^31
ALL = {-4: 1, -3: 1, -2: 1, -1: 1}

# (tag, raw class, instance bits, centre x / y in the current frame, extent x / y, current rows, history rows per offset x 30,
#  velocity in x per frame)
SPECS_A = [
    ("x_high", 18, 1, (9.0, 8.0), (6.0, 2.0), 40, ALL, 0.0),
    ("x_low", 18, 2, (14.0, -6.0), (6.0, 2.0), 35, ALL, 0.0),
    ("x_mid", 18, 3, (20.0, 1.0), (6.0, 2.0), 30, ALL, 0.0),
    ("y_long", 20, 4, (12.0, 3.0), (2.0, 6.0), 30, ALL, 0.0),
    ("equal", 18, 5, (-8.0, 5.0), (4.0, 2.0), 10, {-2: 1 / 30}, 0.0),
    ("absent", 20, 6, (-10.0, -5.0), (2.0, 2.0), 15, {}, 0.0),
    ("cyc19", 253, 7, (6.0, -3.0), (1.0, 0.6), 19, ALL, 0.8),
    ("cyc20", 253, 8, (7.0, 5.5), (1.0, 0.6), 20, ALL, 0.8),
    ("noprev", 255, 9, (-6.0, 2.5), (1.0, 0.6), 25, {-4: 1, -3: 1, -2: 1}, 0.7),
    ("shared", 20, 1, (16.0, 9.0), (2.0, 5.0), 25, ALL, 0.0),
    ("big", 18, BIG, (24.0, 10.0), (6.0, 2.0), 30, ALL, 0.0),
    ("history_only", 18, 12, (-14.0, 8.0), (5.0, 2.0), 0, ALL, 0.0),
]
SPECS_B = [
    ("b_truck", 18, 1, (10.0, -7.0), (5.0, 2.0), 45, ALL, 0.0),
    ("b_other", 20, 2, (13.0, 6.0), (2.0, 5.0), 30, ALL, 0.0),
    ("b_cyc", 253, 3, (5.0, 4.0), (1.0, 0.6), 40, ALL, 0.6),
]
# what the cases of cloud `a` must show, together (tag -> branch)
WANTED = {"x_high": "s2m_x_minus", "x_low": "s2m_x_plus", "x_mid": "s2m_x", "y_long": "s2m_y", "equal": "s2m_y", "absent": "no_history",
          "cyc19": "too_few", "cyc20": "m2s", "noprev": "m2s_nan", "shared": "s2m_y", "big": "s2m_x_minus"}


class Draws(GM.Draws):
    """... and `rand`, which the two passes draw from"""

    def __enter__(self):
        self.log, self.real = [], {n: getattr(np.random, n) for n in ("uniform", "choice", "normal", "random", "rand")}
        for name, fn in self.real.items():
            setattr(np.random, name, self._wrap(name, fn))
        return self


def bits_equal(a, b):
    """float32 arrays: the same bits, a NaN equal to a NaN at the same place"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def make_cloud(seed, specs, maps):
    """{t: (points [n, 4] float32 in the sensor frame of frame t, full labels uint32 [n], pose)}: a synthetic scene whose background
    holds no candidate class, plus the instances of `specs`, rows shuffled"""
    inv, _ = maps
    rs = np.random.RandomState(seed)
    pose0 = synth_pose(0).astype(np.float64)
    scans = {}
    for t in range(T + 1):
        delta = t - T
        pose = synth_pose(T - t)
        pts, lab = synth_scan(1000 * seed + t, n_points=2700 if delta == 0 else 1000, n_beams=16, n_az=360, pose=pose, scene_seed=seed)
        lab = np.where(np.isin(lab, (4, 5, 7, 8)), 1, lab)
        full = inv[lab].astype(np.uint32)
        # a few rows of every other raw class of the label definition, with instance bits
        extra = [13, 16, 52, 60, 99, 252, 254, 256, 257, 258, 259, 31, 32, 1]
        at = rs.choice(len(full), 3 * len(extra), replace=False)
        full[at] = (np.repeat(extra, 3) | (np.arange(3 * len(extra)) % 3 + 20 << 16)).astype(np.uint32)
        rows, labels = [pts], [full]
        back = np.linalg.inv(pose.astype(np.float64)) @ pose0
        for _, cls, inst, centre, extent, n_cur, hist, vel in specs:
            n = n_cur if delta == 0 else int(round(30 * hist.get(delta, 0)))
            if n == 0:
                continue
            p = np.ones((n, 4))
            p[:, 0] = centre[0] + vel * delta + rs.uniform(-extent[0] / 2, extent[0] / 2, n)
            p[:, 1] = centre[1] + rs.uniform(-extent[1] / 2, extent[1] / 2, n)
            p[:, 2] = rs.uniform(-1.6, 0.4, n)
            q = (p @ back.T).astype(np.float32)
            q[:, 3] = rs.uniform(0, 1, n)
            rows.append(q)
            labels.append(np.full(n, (inst << 16) | cls, dtype=np.uint32))
        rows, labels = np.concatenate(rows, 0), np.concatenate(labels, 0)
        order = rs.permutation(len(rows))
        scans[t] = (np.ascontiguousarray(rows[order]), labels[order], pose)
    return scans


class Files:
    """`np.fromfile` of the dataset: the scans of both clouds under the paths the reference derives"""

    def __init__(self, clouds):
        self.files = {}
        for c, scans in enumerate(clouds):
            for t, (pts, full, _) in scans.items():
                path = f"/data/sequences/{c:02d}/velodyne/{t:06d}.bin"
                self.files[path] = pts
                self.files[path.replace("velodyne", "labels")[:-3] + "label"] = full

    def __enter__(self):
        self.real = np.fromfile
        np.fromfile = lambda path, dtype=None, **kw: self.files[path].copy()
        return self

    def __exit__(self, *exc):
        np.fromfile = self.real


def bare_dataset(cls, clouds, augment="GlobalAugment_LP"):
    ds = object.__new__(cls)
    ds.maug_prob, ds.shift_x_range, ds.shift_y_range = MAUG_PROB, SHIFT_X_RANGE, SHIFT_Y_RANGE
    ds.multiscan, ds.step, ds.only_history = T, 1, True
    ds.split, ds.seq, ds.pseudo_mask, ds.trainval_seqs, ds.if_scribble = "train", -1, "gt", ["00", "01"], False
    ds.flexible_steps, ds.augment = STEPS, augment
    ds.poses = {c: [scans[t][2] for t in range(T + 1)] for c, scans in enumerate(clouds)}
    ds.annos = [f"/data/sequences/{c:02d}/velodyne/{T:06d}.bin" for c in range(len(clouds))]
    ds.annos_another = ds.annos[::-1]
    return ds


def fused_inputs(ds, c):
    """what `__getitem__` holds at :152 for cloud c (the lines :128-151)"""
    raw = np.fromfile(ds.annos[c], dtype=np.float32).reshape((-1, 4))
    full = np.fromfile(ds.annos[c].replace("velodyne", "labels")[:-3] + "label", dtype=np.uint32).reshape((-1, 1))
    inst = full.copy().reshape(-1)
    raw_cls = full & 0xFFFF
    raw_ms, _, mask, inst_ms, raw_cls_ms, delta = ds.multiscan_fuse(ds.annos, c, ds.multiscan, ds.flexible_steps)
    return {"raw": raw, "inst": inst, "cls": raw_cls, "raw_ms": raw_ms, "mask": mask, "inst_ms": inst_ms, "cls_ms": raw_cls_ms,
            "delta": delta}


def numpy_table(e):
    """the statistics of every candidate, with numpy's own calls on the reference's arrays (:316-321, :362-370)"""
    cand = np.unique(e["inst"][np.isin(e["cls"].reshape(-1), (18, 20, 253, 255))]).astype(np.int64)
    counts, stats = np.zeros((len(cand), 3), dtype=np.int32), np.zeros((len(cand), 9), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k, inst in enumerate(cand):
            cur, ms = e["raw"][e["inst"] == inst], e["raw_ms"][e["inst_ms"] == inst]
            pre = e["raw_ms"][(e["inst_ms"] == inst) & (e["delta"] == -1)]
            counts[k] = len(cur), len(ms), len(pre)
            ext = [ms[:, 0].min(), ms[:, 0].max(), ms[:, 1].min(), ms[:, 1].max()] if len(ms) else [np.inf, -np.inf, np.inf, -np.inf]
            means = [ms[:, 1].mean(), pre[:, 0].mean(), pre[:, 1].mean(), cur[:, 0].mean(), cur[:, 1].mean()]
            stats[k] = ext + means
            ours = [MV.numpy_mean(col) for col in (ms[:, 1], pre[:, 0], pre[:, 1], cur[:, 0], cur[:, 1])]
            assert bits_equal(np.array(ours), np.array(means, dtype=np.float32)), ("pairwise mean != numpy", inst)
    return MV.MovingTable(cand, counts, stats, len(e["raw_ms"]))


def check_margins(table):
    for k in range(len(table.labels)):
        if int(table.labels[k]) & 0xFFFF in (18, 20) and table.counts[k, 1]:
            cy = float(table.stats[k, 4])
            assert abs(cy - 4) > CENTER_MARGIN and abs(cy + 2) > CENTER_MARGIN, ("center_y at a bound", table.labels[k], cy)


def device_rule(e, p):
    """ts_stage_moving_apply restated in numpy (include/taseg_hip.h) -> (current rows, their raw classes, history rows, theirs)"""
    cur, ms = e["raw"].copy(), e["raw_ms"].astype(np.float32).copy()
    cls, cls_ms = e["cls"].reshape(-1).astype(np.int64), e["cls_ms"].reshape(-1).astype(np.int64)
    delta = e["delta"].astype(np.int64)
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        for r in p.records:
            mc, mh = e["inst"] == r.label, e["inst_ms"] == r.label
            d = delta[mh]
            if r.kind == MV.S2M_X:
                if r.center != 0.0:
                    cur[mc, 1] = cur[mc, 1] + f32(r.center)
                    ms[mh, 1] = ms[mh, 1] + f32(r.center)
                ms[mh, 0] = ms[mh, 0] + (d.astype(np.float64) * r.shift).astype(f32)
            elif r.kind == MV.S2M_Y:
                ms[mh, 1] = ms[mh, 1] + (d.astype(np.float64) * r.shift).astype(f32)
            elif r.kind == MV.M2S:
                ms[mh, 0] = ms[mh, 0] + d.astype(f32) * f32(r.shift_x)
                ms[mh, 1] = ms[mh, 1] + d.astype(f32) * f32(r.shift_y)
            cls[mc], cls_ms[mh] = r.new_class, r.new_class
    return cur, cls, ms, cls_ms


def only(p, which):
    """the records of one pass"""
    kinds = (MV.S2M_X, MV.S2M_Y) if which == 0 else (MV.M2S,)
    return MV.MovingParams(tuple(r for r in p.records if r.kind in kinds), p.draws)


def expected_log(moving=None, mix=None, partner=None, aug=None):
    """the (function, first value) sequence the reference must have drawn for these records, in order"""
    out = []

    def passes(p):
        for _, _, coin, rands in p.draws:
            out.append(("choice", coin))
            out.extend(("rand", v) for v in rands)
    if moving is not None:
        passes(moving)
    if mix is not None:
        out.append(("choice", mix.prob))
        if partner is not None and mix.kind != M.NONE:
            passes(partner)
        if mix.kind == M.LASER:
            out.append(("choice", M.STRATEGIES[mix.strategy]))
        if mix.kind == M.POLAR:
            out += [("random", mix.alpha / np.pi + 1), ("random", None), ("random", None)]
    if aug is not None:
        out += [("uniform", aug.theta), ("uniform", aug.scale), ("choice", aug.flip)] + [("normal", v) for v in aug.translate]
    return out


def check_log(log, want):
    assert len(log) == len(want), ("the reference drew", [n for n, _, _ in log], "the replay", [n for n, _ in want])
    for (name, _, v), (wname, wv) in zip(log, want):
        v = np.ravel(v)[0]
        assert name == wname, (name, wname)
        if isinstance(wv, str):
            assert str(v) == wv
        elif wv is not None and name == "random":
            assert abs(float(v) - wv) < 1e-12             # (alpha is checked exactly where the mix records are compared)
        elif wv is not None:
            assert float(v) == float(wv), (name, v, wv)


def branches(specs, table, p):
    """tag -> the branch its instance took, from the statistics and the replayed records (both checked against the reference)"""
    rec = {r.label: r for r in p.records}
    coin = {label: c for _, label, c, _ in p.draws}
    out = {}
    for tag, cls, inst, *_ in specs:
        label = (inst << 16) | cls
        if coin.get(label) != 1:
            continue
        k = int(np.nonzero(table.labels == label)[0][0])
        n_cur, n_hist, _ = table.counts[k]
        r = rec.get(label)
        if n_hist == 0:
            out[tag] = "no_history"
        elif cls in (253, 255) and n_cur < 20:
            out[tag] = "too_few"
        elif r.kind == MV.M2S:
            out[tag] = "m2s_nan" if np.isnan(r.shift_x) else "m2s"
        elif r.kind == MV.S2M_Y:
            out[tag] = "s2m_y"
        else:
            out[tag] = "s2m_x_minus" if r.center < 0 else "s2m_x_plus" if r.center > 0 else "s2m_x"
        assert (r is None) == (out[tag] in ("no_history", "too_few"))
    return out


def store_sparse(out, key, before, after):
    """the rows of `after` whose bits differ from `before`"""
    before, after = np.ascontiguousarray(before, dtype=np.float32), np.ascontiguousarray(after, dtype=np.float32)
    idx = np.nonzero((before.view(np.uint32) != after.view(np.uint32)).any(1))[0]
    out[f"{key}_idx"], out[f"{key}_rows"] = idx.astype(np.int32), after[idx]


def run_case(out, c, ds, cloud, e, table, seed):
    """the two passes as `__getitem__` calls them (:152-163) after np.random.seed(seed); everything checked against the replay"""
    raw, cls, raw_ms, cls_ms = e["raw"].copy(), e["cls"].copy(), e["raw_ms"].copy(), e["cls_ms"].copy()
    np.random.seed(seed)
    states = []
    with Draws() as d, np.errstate(all="ignore"):
        for fn, classes in ((ds.static2moving, (18, 20)), (ds.moving2static, (253, 255))):
            if len(e["inst_ms"]) > 0 and np.isin(cls, classes).sum() > 0:
                raw, cls, raw_ms, cls_ms = fn(raw, cls, e["inst"], raw_ms, cls_ms, e["inst_ms"], e["delta"], cloud)
            states.append((raw.copy(), cls.copy().reshape(-1), raw_ms.copy(), cls_ms.copy().reshape(-1)))
    p = MV.draw_moving_params(np.random.RandomState(seed), table, MAUG_PROB, SHIFT_X_RANGE, SHIFT_Y_RANGE)
    check_log(d.log, expected_log(moving=p))
    for which, (w_raw, w_cls, w_ms, w_cls_ms) in enumerate(states):
        q = only(p, 0) if which == 0 else p
        g_raw, g_cls, g_ms, g_cls_ms = device_rule(e, q)
        assert bits_equal(g_raw, w_raw) and bits_equal(g_ms, w_ms), (c, which, "rows")
        assert np.array_equal(g_cls, w_cls) and np.array_equal(g_cls_ms, w_cls_ms), (c, which, "raw classes")
        assert bits_equal(w_raw[:, 2:], e["raw"][:, 2:]) and bits_equal(w_ms[:, 2:], e["raw_ms"][:, 2:])
        name = f"{c}_{'s2m' if which == 0 else 'm2s'}"
        store_sparse(out, f"{name}_cur", e["raw"], w_raw)
        store_sparse(out, f"{name}_hist", e["raw_ms"], w_ms)
        out[f"{name}_cur_cls"], out[f"{name}_hist_cls"] = w_cls.astype(np.uint16), w_cls_ms.astype(np.uint16)
    out[f"{c}_cloud"], out[f"{c}_seed"] = np.array(cloud), np.array(seed)
    out[f"{c}_coins"] = np.array([coin for _, _, coin, _ in p.draws], dtype=np.int64)
    out[f"{c}_rands"] = np.array([v for _, _, _, rands in p.draws for v in rands], dtype=np.float64)
    out[f"{c}_moved"] = np.array([r.label for r in p.records], dtype=np.int64)
    out[f"{c}_kinds"] = np.array([r.kind for r in p.records], dtype=np.int64)
    return p


def pick_seeds(specs, table, wanted, limit=4000):
    """the first seeds whose replays, together, take every wanted branch (greedy: a seed is taken when it adds one)"""
    seen, seeds = {}, []
    for seed in range(limit):
        p = MV.draw_moving_params(np.random.RandomState(seed), table, MAUG_PROB, SHIFT_X_RANGE, SHIFT_Y_RANGE)
        got = branches(specs, table, p)
        new = {t: b for t, b in got.items() if t in wanted and t not in seen}
        if new:
            seen.update(new)
            seeds.append(seed)
        if len(seen) == len(wanted):
            return seeds
    raise AssertionError(("no seeds for", sorted(set(wanted) - set(seen))))


def label_maps():
    from pcseg.data.dataset.semantickitti.semantickitti_utils_ms_ms import LEARNING_MAP, LEARNING_MAP_INV
    lm = np.zeros(260, dtype=np.int64)
    for k, v in LEARNING_MAP.items():
        lm[k] = v
    inv = np.array([LEARNING_MAP_INV[i] for i in range(len(LEARNING_MAP_INV))], dtype=np.int64)
    return inv, lm


def gen_points(ds, clouds, entries, tables, fname="moving.npz"):
    inv, lm = label_maps()
    out = {"backend": np.array(R2.BACKEND_DESC), "T": np.array(T), "steps": np.array(STEPS), "learning_map": lm,
           "learning_map_inv": inv, "maug_prob": np.array(MAUG_PROB), "shift_range": np.array([SHIFT_X_RANGE, SHIFT_Y_RANGE])}
    for c, (scans, e, table) in enumerate(zip(clouds, entries, tables)):
        n = "ab"[c]
        for t, (pts, full, pose) in scans.items():
            out[f"{n}_points_t{t}"], out[f"{n}_rawlabels_t{t}"], out[f"{n}_pose_t{t}"] = pts, full, pose
        out[f"{n}_fused"], out[f"{n}_mask"] = e["raw_ms"].astype(np.float32), e["mask"]
        out[f"{n}_delta"] = e["delta"].astype(np.int8)
        out[f"{n}_cand"], out[f"{n}_counts"], out[f"{n}_stats"] = table.labels, table.counts, table.stats
        check_margins(table)
    assert any(int(v) >= 1 << 31 for v in tables[0].labels)
    # cloud a: the seeds that show every branch; cloud b: the first seed that moves something in both passes
    seeds_a = pick_seeds(SPECS_A, tables[0], WANTED)
    seed_b = next(s for s in range(4000) if {r.kind for r in MV.draw_moving_params(np.random.RandomState(s), tables[1]).records}
                  >= {MV.M2S} and len(MV.draw_moving_params(np.random.RandomState(s), tables[1]).records) >= 2)
    cases, seen = [], {}
    for cloud, seed in [(0, s) for s in seeds_a] + [(1, seed_b)]:
        c = f"{'ab'[cloud]}_s{seed}"
        p = run_case(out, c, ds, cloud, entries[cloud], tables[cloud], seed)
        if cloud == 0:
            seen.update(branches(SPECS_A, tables[0], p))
        cases.append(c)
    assert {t: seen.get(t) for t in WANTED} == WANTED, seen
    # by construction: the history-only instance is no candidate, the shared instance bits are two candidates
    assert ((12 << 16) | 18) not in tables[0].labels and {(1 << 16) | 18, (1 << 16) | 20} <= set(tables[0].labels.tolist())
    out["cases"] = np.array(cases)
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; cases", cases, "branches", seen)


class Frames:
    """the frame reader of the voxel dataset: the real `__getitem__`, the ring-id column it appends cut off again"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds.annos)

    def __getitem__(self, b):
        with np.errstate(all="ignore"):
            pc = self.ds[b]
        return {"xyzret": np.ascontiguousarray(pc["xyzret"][:, :4]), "labels": pc["labels"], "path": pc["path"],
                "xyzret_ms": np.ascontiguousarray(pc["xyzret_ms"][:, :5]), "labels_ms": pc["labels_ms"]}


def replay_batch(seed, tables):
    rng = np.random.RandomState(seed)
    om = M.draw_omega(rng)
    rows = []
    for b in range(2):
        mv, mix, pmv = MV.draw_smsa_sample(rng, om, tables[b], tables[1 - b])
        rows.append((mv, mix, pmv, A.draw_train_params(rng)))
    return om, rows


def gen_batches(ds, mod, vox_cls, tables, fname="moving_batch.npz"):
    # the first seeds whose two samples are mixed once by LaserMix and once by PolarMix, move something of their own and - the
    # PolarMix sample - something of the partner
    def fits(seed):
        _, rows = replay_batch(seed, tables)
        kinds = {r[1].kind for r in rows}
        polar = [r for r in rows if r[1].kind == M.POLAR]
        return kinds == {M.LASER, M.POLAR} and all(r[0].records for r in rows) and bool(polar[0][2].records)
    seeds = [s for s in range(4000) if fits(s)][:2]
    out = {"backend": np.array(R2.BACKEND_DESC), "cases": np.array([f"batch_s{s}" for s in seeds])}
    for seed in seeds:
        c = f"batch_s{seed}"
        np.random.seed(seed)
        omega = GM.global_omega()
        mod.Omega = omega                                  # :16, drawn when the module is imported
        vox = GA.make_vox(vox_cls, [], 5, VOXEL, True)
        vox.point_cloud_dataset = Frames(ds)
        with Draws() as d:
            samples = [vox.get_single_sample(b) for b in (0, 1)]
        om, rows = replay_batch(seed, tables)
        assert list(om) == omega
        want = []
        for mv, mix, pmv, aug in rows:
            want += expected_log(mv, mix, pmv, aug)
        check_log(d.log, want)
        GM.store_mix(out, c, seed, omega, [r[1] for r in rows])
        GA.store_params(out, c, [r[3] for r in rows])
        for b, (mv, _, pmv, _) in enumerate(rows):
            out[f"{c}_moved_{b}"] = np.array([r.label for r in mv.records], dtype=np.int64)
            out[f"{c}_partner_moved_{b}"] = np.array([r.label for r in pmv.records], dtype=np.int64)
        out.update(GA.dump_batch(f"{c}_batch_", vox_cls.collate_batch(samples)))
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; seeds", seeds)


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    _ref_env.setup_datasets()
    import pcseg.data.dataset.semantickitti.semantickitti_ms_ms as MSMS
    from pcseg.data.dataset.semantickitti.semantickitti_voxel_ms_ms import SemkittiVoxelMsMsDataset
    maps = label_maps()
    assert np.array_equal(maps[1], MV.LABEL_TABLE) and [MV.LEARNING_MAP_INV[i] for i in range(26)] == maps[0].tolist()
    clouds = [make_cloud(41, SPECS_A, maps), make_cloud(42, SPECS_B, maps)]
    ds = bare_dataset(MSMS.SemantickittiMsMsDataset, clouds)
    with Files(clouds):
        entries = [fused_inputs(ds, c) for c in range(2)]
        tables = [numpy_table(e) for e in entries]
        gen_points(ds, clouds, entries, tables)
        gen_batches(ds, MSMS, SemkittiVoxelMsMsDataset, tables)
