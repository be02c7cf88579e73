"""Golden vectors of the mask-distillation recipe's three-cloud data stage (build container only: it runs the reference, which
_ref_env locates; nothing here is imported by the tests or the product).

    python tests/golden/make_golden_kd.py

Runs the REAL `SemantickittiMsKdDataset.__getitem__` (semantickitti_ms_kd.py:121-278, on a bare object carrying `multiscan`,
`flexible_steps`, `flexible_steps_gt`, `pseudo_mask='mink_notta'`, with `np.fromfile` served from a dict), then
`SemkittiVoxelMsKdDataset.get_single_sample` + `collate_batch` (semantickitti_voxel_ms_kd.py:77-245), on the clouds of multiscan.npz:
samples 0 and 1 (a current scan and four history scans each) and a third sample at frame 0 of a sequence of its own - scan 0 of
cloud 0 -, which has NO history.  Partners: 0 -> 1, 1 -> 2 (a partner without history), 2 -> 0.

  kd_stage.npz   inputs (data only): per history scan the pseudo labels - the annotation with about 15 % of the rows moved to
                 another class's canonical raw id and a few to raw id 252, drawn from RandomState(PSEUDO_SEED) - and the `canon`
                 columns of annotation and pseudo label (the class whose canonical raw id it is, else -1); FLEXIBLE_STEPS of
                 multiscan.npz and a FLEXIBLE_STEPS_GT that differs from it in both directions.
                 cases: `eval` (training=False: samples 0 and 2) and the training batches `train_s4` (samples 2, 0, 1: the LaserMix
                 identity on the sample without history, PolarMix with the swap and a partner with history, PolarMix without the
                 swap) and `train_s2` (sample 1: PolarMix with the swap and the partner WITHOUT history), GlobalAugment_LP with all
                 four augmentations; per case the seed, the samples, the values the reference DREW and the collated batch under the
                 keys of multiscan.npz plus `lidar_ms_gt`, `offset_ms_gt`, `num_points_ms_gt`.  The reference's `lidar` carries the
                 ring id as a fifth column (IN_FEATURE_DIM 5 of `xyzret`): stored under `lidar_ring`, `lidar_F` holds four columns,
                 what the device stage carries for the single-frame cloud.

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through draw_mix_params / draw_train_params
gives the recorded draws in the recorded ORDER (coin, mix, augmentation - the FSA recipe's); the device rule restated in numpy
(`kd_rule`: the two table lookups on the canon columns, the head of the partner's teacher cloud, the mix rule of
make_golden_mix.device_rule on three pairs with the teacher's labels 0) reproduces the rows of all three clouds of `__getitem__`
bit for bit; no fixture row has a yaw within 1e-5 rad of a sector bound (make_golden_mix.check_margins).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_moving as GMV  # noqa: E402  (arranges the reference's imports)

GM, GA, R2, _ref_env = GMV.GM, GMV.GA, GMV.R2, GMV._ref_env
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data.semantickitti import _CANON, LEARNING_MAP_INV  # noqa: E402
from taseg_amd.data.stage import _kitti_row  # noqa: E402

VOXEL, PSEUDO_SEED = 0.05, 77
STEPS_GT = [0, 0, 1, 2, 2, 2, 2, 2, 2, 4, 4, 4, 4, 0, 2, 0, 2, 4, 0, 2]
PARTNER = [1, 2, 0]
PLAN = [("eval", -1, [0, 2]), ("train_s4", 4, [2, 0, 1]), ("train_s2", 2, [1])]


def make_clouds(g):
    """{t: (points, raw annotation [n, 1] uint32, pose, raw pseudo label [n, 1] uint32)} per sample"""
    T = int(g["T"])
    rs = np.random.RandomState(PSEUDO_SEED)
    canon_ids = np.array([LEARNING_MAP_INV[c] for c in range(1, 20)], dtype=np.uint32)
    clouds = []
    for b in range(2):
        scans = {}
        for t in range(T + 1):
            raw = g[f"b{b}_rawlabels_t{t}"].astype(np.uint32)
            pseudo = raw.copy()
            move = rs.random_sample(len(raw)) < 0.15
            pseudo[move] = rs.choice(canon_ids, int(move.sum()))
            pseudo[rs.choice(len(raw), 6, replace=False)] = 252          # a moving-object id: no class's canonical id
            scans[t] = (g[f"b{b}_points_t{t}"], raw.reshape(-1, 1), g[f"b{b}_pose_t{t}"], pseudo.reshape(-1, 1))
        clouds.append(scans)
    pts, raw, pose, pseudo = clouds[0][0]
    clouds.append({0: (pts, raw, pose, pseudo)})
    return clouds


def path_of(c, t):
    return f"/data/sequences/{c:02d}/velodyne/{t:06d}.bin"


class Files(GMV.Files):
    """... and the predictions `mink_notta` reads (semantickitti_ms_kd.py:323-327: the path's `velodyne` -> `predictions`)"""

    def __init__(self, clouds):
        self.files = {}
        for c, scans in enumerate(clouds):
            for t, (pts, raw, _, pseudo) in scans.items():
                self.files[path_of(c, t)] = pts
                self.files[path_of(c, t).replace("velodyne", "labels")[:-3] + "label"] = raw
                self.files[path_of(c, t).replace("velodyne", "predictions")[:-3] + "label"] = pseudo


def bare_dataset(cls, clouds, steps, training):
    ds = object.__new__(cls)
    ds.multiscan, ds.only_history, ds.pseudo_mask = max(len(s) for s in clouds) - 1, True, "mink_notta"
    ds.flexible_steps, ds.flexible_steps_gt, ds.augment = list(steps), list(STEPS_GT), "GlobalAugment_LP"
    ds.split, ds.seq, ds.trainval_seqs, ds.if_scribble = "train" if training else "val", -1, ["00", "01", "02"], False
    ds.poses = {c: [scans[t][2] for t in range(len(scans))] for c, scans in enumerate(clouds)}
    ds.annos = [path_of(c, len(scans) - 1) for c, scans in enumerate(clouds)]
    ds.annos_another = [ds.annos[p] for p in PARTNER]
    return ds


class Recorded:
    """the frame reader of the voxel dataset: the real `__getitem__`, what it returned kept (the voxel dataset augments in place)"""

    def __init__(self, ds):
        self.ds, self.seen = ds, []

    def __len__(self):
        return len(self.ds.annos)

    def __getitem__(self, b):
        pc = self.ds[b]
        self.seen.append((b, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pc.items()}))
        return pc


def fused_inputs(ds, clouds, steps):
    """per sample what the device stage starts from: current scan, classes, un-filtered fused history with classes, the keep
    bytes of both rules from the canon columns - asserted equal to the reference's masks"""
    lm = np.zeros(260, dtype=np.int64)
    from pcseg.data.dataset.semantickitti.semantickitti_utils import LEARNING_MAP
    for k, v in LEARNING_MAP.items():
        lm[k] = v
    out = []
    for c, scans in enumerate(clouds):
        T = len(scans) - 1
        raw, ann = scans[T][0], lm[scans[T][1].reshape(-1) & 0xFFFF]
        e = {"raw": raw, "lab": ann, "T": T}
        if T:
            fused, lab_ms, mask, mask_gt = ds.multiscan_fuse(ds.annos, c, ds.multiscan, ds.flexible_steps, ds.flexible_steps_gt)
            deltas = [t - T for t in range(T)]
            rows, rows_gt = [_kitti_row(d, steps) for d in deltas], [_kitti_row(d, STEPS_GT) for d in deltas]
            keep = np.concatenate([np.array(rows[t])[_CANON[scans[t][3].reshape(-1)]] for t in range(T)])
            keep_gt = np.concatenate([np.array(rows_gt[t])[_CANON[scans[t][1].reshape(-1)]] for t in range(T)])
            assert np.array_equal(keep, mask) and np.array_equal(keep_gt, mask_gt), "table lookup != the reference's masks"
            assert not np.array_equal(mask, mask_gt)
            e.update(fused=fused.astype(np.float32), lab_ms=lab_ms.reshape(-1), keep=keep, keep_gt=keep_gt)
            assert GA.same_bits(np.ascontiguousarray(e["fused"]), np.ascontiguousarray(fused, dtype=np.float32))
        else:
            e.update(fused=np.zeros((0, 4), np.float32), lab_ms=np.zeros(0, np.int64), keep=np.zeros(0, bool), keep_gt=np.zeros(0, bool))
        out.append(e)
    return out


def flagged(head, hist):
    rows = np.concatenate([head, hist], 0)
    flag = np.zeros((len(rows), 1), np.float32)
    flag[:len(head)] = 1
    return np.concatenate([rows[:, :4], flag], 1)


def kd_rule(ins, b, p):
    """build_kd_batch's three clouds of sample b before the augmentation, restated in numpy -> (point, labels, point_ms, labels_ms,
    point_ms_gt)"""
    e, e1 = ins[b], ins[PARTNER[b]]
    zeros = lambda rows: np.zeros(len(rows), np.int64)  # noqa: E731
    ms, ms_lab = flagged(e["raw"], e["fused"][e["keep"]]), np.concatenate([e["lab"], e["lab_ms"][e["keep"]]])
    gt = flagged(e["raw"], e["fused"][e["keep_gt"]])
    if p.kind == M.NONE:
        return e["raw"], e["lab"], ms, ms_lab, gt
    ms1, ms1_lab = flagged(e1["raw"], e1["fused"][e1["keep"]]), np.concatenate([e1["lab"], e1["lab_ms"][e1["keep"]]])
    # the head of the partner's teacher cloud: the SAMPLE's current scan when the partner has history, else the partner's own
    gt1 = flagged(e["raw"] if e1["T"] else e1["raw"], e1["fused"][e1["keep_gt"]])
    raw, lab = GM.device_rule(e["raw"], e["lab"], e1["raw"], e1["lab"], p)
    ms, ms_lab = GM.device_rule(ms, ms_lab, ms1, ms1_lab, p)
    gt, _ = GM.device_rule(gt, zeros(gt), gt1, zeros(gt1), p)
    return raw, lab, ms, ms_lab, gt


def run_case(out, c, seed, which, g, clouds, steps, KD, VoxKd):
    training = seed >= 0
    ds = bare_dataset(KD.SemantickittiMsKdDataset, clouds, steps, training)
    ins = fused_inputs(ds, clouds, steps)
    vox = GA.make_vox(VoxKd, [], 5, VOXEL, training)
    frames = vox.point_cloud_dataset = Recorded(ds)
    np.random.seed(max(seed, 0))
    omega = GM.global_omega()
    KD.Omega = omega                                   # semantickitti_ms_kd.py:14, drawn when the module is imported
    with GMV.Draws() as d:
        samples = [vox.get_single_sample(b) for b in which]
    rng = np.random.RandomState(max(seed, 0))
    om = M.draw_omega(rng)
    assert list(om) == omega
    if training:
        mix, aug = [], []
        for _ in which:
            mix.append(M.draw_mix_params(rng, om))     # the coin and the mix first, then the augmentation: the FSA order
            aug.append(A.draw_train_params(rng))
        GM.check_replay(d.log, mix, aug)
        GM.store_mix(out, c, seed, omega, mix)
        GA.store_params(out, c, aug)
    else:
        # (the coin is drawn and not used, semantickitti_ms_kd.py:155-157)
        assert [n for n, _, _ in d.log] == ["choice"] * len(which)
        mix = [M.MixParams()] * len(which)
    out[f"{c}_seed"], out[f"{c}_samples"], out[f"{c}_training"] = np.array(seed), np.array(which), np.array(training)
    facts = []
    for (b, pc), p in zip(frames.seen, mix):
        raw, lab, ms, ms_lab, gt = kd_rule(ins, b, p)
        e1 = ins[PARTNER[b]]
        if p.kind != M.NONE:
            GM.check_margins([x for x in (ins[b]["raw"], e1["raw"], ins[b]["fused"], e1["fused"]) if len(x)], p)
        GM.same_rows((raw, lab), (pc["xyzret"][:, :4], pc["labels"]), (c, b, "point"))
        GM.same_rows((ms, ms_lab), (pc["xyzret_ms"][:, :5], pc["labels_ms"]), (c, b, "point_ms"))
        assert GA.same_bits(np.ascontiguousarray(gt, dtype=np.float32), np.ascontiguousarray(pc["xyzret_ms_gt"][:, :5])), (c, b, "gt")
        facts.append((p.kind, bool(p.swap), ins[b]["T"] > 0, e1["T"] > 0))
    batch = VoxKd.collate_batch(samples)
    prefix = f"{c}_batch_"
    out.update(GA.dump_batch(prefix, batch))
    feats = out[prefix + "lidar_F"]
    out[prefix + "lidar_ring"], out[prefix + "lidar_F"] = np.ascontiguousarray(feats[:, 4]), np.ascontiguousarray(feats[:, :4])
    out[prefix + "lidar_ms_gt_C"], out[prefix + "lidar_ms_gt_F"] = batch["lidar_ms_gt"].C.numpy(), batch["lidar_ms_gt"].F.numpy()
    out[prefix + "offset_ms_gt"] = batch["offset_ms_gt"].numpy()
    out[prefix + "num_points_ms_gt"] = batch["num_points_ms_gt"].numpy()
    return facts


def main(fname="kd_stage.npz"):
    _ref_env.setup_datasets()
    import pcseg.data.dataset.semantickitti.semantickitti_ms_kd as KD
    from pcseg.data.dataset.semantickitti.semantickitti_voxel_ms_kd import SemkittiVoxelMsKdDataset as VoxKd
    g = dict(np.load(os.path.join(HERE, "multiscan.npz"), allow_pickle=False))
    steps = g["steps"].tolist()
    assert steps != STEPS_GT and len(steps) == len(STEPS_GT)
    clouds = make_clouds(g)
    out = {"backend": np.array(R2.BACKEND_DESC), "steps_gt": np.array(STEPS_GT), "partner": np.array(PARTNER),
           "cases": np.array([c for c, _, _ in PLAN]), "pseudo_seed": np.array(PSEUDO_SEED)}
    for b in range(2):
        for t in range(int(g["T"])):
            _, raw, _, pseudo = clouds[b][t]
            out[f"b{b}_pseudo_t{t}"] = pseudo.reshape(-1).astype(np.uint16)
            out[f"b{b}_pseudo_canon_t{t}"] = _CANON[pseudo.reshape(-1)].astype(np.int8)
            out[f"b{b}_canon_t{t}"] = _CANON[raw.reshape(-1)].astype(np.int8)
            moved = float((pseudo != raw).mean())
            assert 0.1 < moved < 0.2 and (pseudo == 252).sum() >= 1, moved
    facts = []
    with Files(clouds):
        for c, seed, which in PLAN:
            facts += run_case(out, c, seed, which, g, clouds, steps, KD, VoxKd)
    kinds = {(k, s) for k, s, _, _ in facts}
    assert kinds >= {(M.NONE, False), (M.POLAR, True), (M.POLAR, False), (M.LASER, False)}, facts
    assert any(k == M.NONE and not own for k, _, own, _ in facts), "a sample without history"
    assert any(k == M.POLAR and s and own and not theirs for k, s, own, theirs in facts), "a swapped partner without history"
    assert any(k == M.POLAR and s and own and theirs for k, s, own, theirs in facts), "a swapped partner with history"
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; (kind, swap, history, partner's history)", facts)


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    main()
