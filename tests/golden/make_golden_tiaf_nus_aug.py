"""Golden vectors of the nuScenes TIAF recipe's training augmentation and TTA views (build container only: it runs the reference,
which _ref_env locates; nothing here is imported by the tests or the product).

    python tests/golden/make_golden_tiaf_nus_aug.py

Runs the REAL `NuscenesMsMmDataset.__getitem__` (nuscenes_ms_mm.py:142-401, on a bare object over the two synthetic scenes of
make_golden_r3.gen_tiaf_nus, files served from a dict, pyquaternion and the devkit's view_points under their import names from
oracle/ts_oracle.py as there), then `NuscVoxelMsMmDataset.get_single_sample` + `collate_batch` / `collate_batch_tta`
(nuscenes_voxel_ms_mm.py:67-318).  The scenes are regenerated from seeds 71 and 72 and ASSERTED equal to the arrays stored in
tiaf_nus.npz (clouds, labels, poses, images, the selected image keyframes, the un-augmented FOV cloud): the tests read every input
from that file, this one stores the draws and the outputs alone.

  tiaf_nus_aug.npz   `train`    (i) a training batch of both samples, all four point augmentations on, ONE `np.random.seed(seed)`
                                before the two `get_single_sample` calls (the samples draw one after the other)
                     `norot`    (ii) the same with ROTATE_AUG off: the cloud is still float32 when it is scaled, the one
                                combination numpy scales in float32
                     `tta`      (iii) votes 4 .. 6 of sample 0 through `__getitem__` and `collate_batch_tta`
                     per case the values the reference DREW, recorded by wrapping numpy's generator functions while it ran - theta /
                     scale / flip type / translation and NOTHING else: NuscenesMsMmDataset.__getitem__ draws no mix coin and no
                     image flip.  Coordinates that two keys share are stored once; the image planes equal tiaf_nus.npz's (asserted
                     here - the augmentation does not touch them; under TTA every vote carries sample 0's) and are not stored again.

The voxel dataset augments `xyzret_fov_ms` IN PLACE and a real dataset re-reads the sample on every access, so `point_cloud_dataset`
here is `Live`: every access runs `ds[index]` again.  The image keyframes are selected on the first read only (`token2samplelist_fov`
caches them): `random.seed(case rng)` before it, as in make_golden_r3.

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through draw_train_params / draw_tta_params gives
the recorded draws in the recorded ORDER; the float64 formula of ts_stage_augment on tiaf_nus.npz's un-augmented FOV cloud, clamped
to the augmented single-frame cloud's corner, gives the rows the reference voxelised; the clamp removes at least one FOV row and
every sample keeps some.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_aug as GA  # noqa: E402  (arranges the reference's imports)
import make_golden_r3 as G3  # noqa: E402
from make_golden_tiaf_aug import Draws, Live, Served  # noqa: E402

G2, _ref_env = G3.G2, G3._ref_env
from taseg_amd.data import augment as A  # noqa: E402

VOXEL = 0.1
SPARSE = ("lidar", "lidar_ms", "lidar_fov_ms", "targets_fov_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms",
          "targets_mapped", "targets_mapped_ms")
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map", "targets_mapped_ms": "inverse_map_ms",
               "targets_fov_ms": "lidar_ms"}
DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img")
TRAIN_SEED, NOROT_SEED, TTA_SEED, TTA_VOTES = 3, 20, 11, (4, 7)
ALL_ON, NO_ROTATION = (True, True, True, True), (True, True, True, False)          # flip, scale, jitter, rotate


def scene(g, b, Ds, learning_map):
    """(bare dataset, served files, index) of sample b, regenerated as make_golden_r3.gen_tiaf_nus builds it and compared with
    the arrays tiaf_nus.npz stores"""
    p = f"b{b}_"
    case = {k[len(p) + 4:]: g[k].tolist() for k in g if k.startswith(p + "cfg_")}
    sc = G2.nus_scene(case["seed"])
    tabs, cam_files = G3.camera_tables(sc, case["seed"])
    sc["files"].update(cam_files)

    class FakeNusc:
        dataroot = "/nus"

        def get(self, table, token):
            if table == "sample":
                return sc["sample_tab"][token]
            if table == "lidarseg":
                return sc["lidarseg_tab"][token]
            return tabs[table][token]

        def get_sample_data(self, token):
            rec = tabs["sample_data"][token]
            return os.path.join(self.dataroot, rec["filename"]), [], np.array(tabs["calibrated_sensor"][rec["calibrated_sensor_token"]]["camera_intrinsic"])

    ds = object.__new__(Ds)
    ds.root_path, ds.data_path_ceph, ds.split, ds.seq, ds.augment, ds.tta = "/nus", None, "val", -1, "none", False
    ds.nusc, ds.nusc_infos, ds.nusc_infos_sweep = FakeNusc(), sc["infos"], sc["sweeps"]
    ds.global_indexes, ds.local_indexes, ds.scene_tokens = sc["global_indexes"], sc["local_indexes"], sc["scene_tokens"]
    ds.token2samplelist, ds.token2samplelist_fov, ds.learning_map = {}, {}, learning_map
    ds.multiscan, ds.step, ds.flexible_steps, ds.pseudo_mask = int(g["multiscan"]), float(g["step"]), g["steps"].tolist(), "mink_sweep_notta"
    ds.img_view, ds.used_view, ds.resize = list(G3.VIEWS), case["used_view"], 0.5
    ds.multiscan_image, ds.step_image, ds.multiscan_interval = case["multiscan_image"], case["step_image"], case["interval"]
    ds.height, ds.width, ds.image_jitter, ds.image_flip, ds.paint_dist = int(g["height"]), int(g["width"]), False, False, case["paint_dist"]
    ds.get_path_infos_cam_lidar()
    index = len(sc["infos"]) - 1 - case["back"]
    assert index == int(g[p + "index"])
    # the inputs the tests will read from tiaf_nus.npz are the ones the reference reads here
    for i, info in enumerate(sc["infos"]):
        sd = sc["sample_tab"][info["token"]]["data"]["LIDAR_TOP"]
        assert np.array_equal(sc["files"]["/nus/" + info["lidar_path"][16:]], g[f"{p}key{i}_points"])
        assert np.array_equal(sc["files"]["/nus/" + sc["lidarseg_tab"][sd]["filename"]], g[f"{p}key{i}_rawlabels"])
    for name, field in (("key_l2e_q", "lidar2ego_rotation"), ("key_l2e_t", "lidar2ego_translation"),
                        ("key_e2g_q", "ego2global_rotation"), ("key_e2g_t", "ego2global_translation")):
        assert np.array_equal(np.array([i[field] for i in sc["infos"]], dtype=np.float64), g[p + name])
    for v in case["used_view"]:
        cs = tabs["calibrated_sensor"]["cs_" + G3.VIEWS[v]]
        assert np.array_equal(np.array(cs["camera_intrinsic"], dtype=np.float64), g[f"{p}view{v}_intrinsic"])
        for d in g[p + "image_keyframes"].tolist():
            tok = f"{G3.VIEWS[v]}_{index + d:02d}"
            assert np.array_equal(sc["files"]["/nus/" + tabs["sample_data"][tok]["filename"]], g[f"{p}key{index + d}_view{v}_image"])
            assert np.array_equal(np.array(tabs["ego_pose"]["pose_" + tok]["translation"]), g[f"{p}key{index + d}_view{v}_pose_t"])
    with Served(sc["files"]):
        random.seed(case["rng"])
        pc_data = ds[index]                     # the first read selects the image keyframes (and caches them)
    lidar_sd = sc["sample_tab"][sc["infos"][index]["token"]]["data"]["LIDAR_TOP"]
    assert list(ds.token2samplelist_fov[lidar_sd]) == g[p + "image_keyframes"].tolist()
    for k in ("xyzret", "xyzret_ms", "xyzret_fov_ms", "image_ms", "semantic_map_ms"):
        assert np.array_equal(np.asarray(pc_data[k], dtype=np.float32), g[p + k]), k
    assert np.array_equal(pc_data["labels_fov_ms"].reshape(-1).astype(np.int64), g[p + "labels_fov_ms"])
    return ds, sc["files"], index


def make_vox(Vox, ds, index, training, switches=ALL_ON):
    vox = GA.make_vox(Vox, [], 4, VOXEL, training, switches)
    vox.point_cloud_dataset, vox.num_points = Live(ds, index), 1000000
    return vox


def check_fov(g, b, p, sample, where):
    """rules (e) and (f) on the host: formula(tiaf_nus.npz's FOV cloud) clamped to the augmented single-frame corner == the rows the
    reference voxelised; the clamp removes rows and keeps rows"""
    fov = g[f"b{b}_xyzret_fov_ms"].copy()
    fov[:, :3] = GA.formula(np.ascontiguousarray(fov[:, :3]), p)
    point = GA.formula(np.ascontiguousarray(g[f"b{b}_xyzret"][:, :3]), p)
    inside = (fov[:, :3] >= point.min(0)).all(1)
    kept = fov[inside]
    assert 0 < len(kept) < len(fov), (where, b, len(kept), len(fov))
    rows = {r.tobytes() for r in kept}
    feats = np.asarray(sample["lidar_fov_ms"].F)
    assert feats.dtype == np.float32 and all(r.tobytes() in rows for r in feats), (where, b)
    pc = np.round(kept[:, :3] / VOXEL).astype(np.int32)
    assert len(np.unique(pc, axis=0)) == len(feats), (where, b)
    return len(fov) - len(kept), len(kept)


def dump(out, prefix, batch, g, images):
    for key in SPARSE:
        if key in SAME_COORDS:
            assert np.array_equal(batch[key].C.numpy(), batch[SAME_COORDS[key]].C.numpy()), key
        else:
            out[f"{prefix}{key}_C"] = batch[key].C.numpy()
        out[f"{prefix}{key}_F"] = batch[key].F.numpy()
    for key in DENSE:
        out[f"{prefix}{key}"] = batch[key].numpy()
    assert np.array_equal(batch["image_ms"].numpy(), images[0]) and np.array_equal(batch["semantic_map_ms"].numpy(), images[1])
    for key in ("depth_map_ms", "lidar_map_ms"):
        out[f"{prefix}{key}_shape"] = np.array(batch[key].shape)
        assert not batch[key].numpy().any()


def train_case(out, c, g, scenes, Vox, seed, switches):
    flip, scale, jitter, rotate = switches
    voxes = [make_vox(Vox, ds, index, True, switches) for ds, _, index in scenes]
    samples = []
    np.random.seed(seed)
    with Draws() as d:
        for vox, (_, files, _) in zip(voxes, scenes):
            with Served(files):
                samples.append(vox.get_single_sample(0))
    rng = np.random.RandomState(seed)
    params = [A.draw_train_params(rng, flip=flip, scale=scale, scale_range=voxes[0].scale_range, jitter=jitter, rotate=rotate)
              for _ in scenes]
    assert all(name != "rand" for name, _, _ in d.log)
    GA.check_replay(d.log, params)
    removed = [check_fov(g, b, p, s, c) for b, (p, s) in enumerate(zip(params, samples))]
    out[f"{c}_seed"], out[f"{c}_switches"], out[f"{c}_fov_removed_kept"] = np.array(seed), np.array(switches), np.array(removed)
    GA.store_params(out, c, params)
    dump(out, f"{c}_batch_", Vox.collate_batch(samples), g, (g["batch_image_ms"], g["batch_semantic_map_ms"]))
    return removed


def main(fname="tiaf_nus_aug.npz"):
    import yaml
    G2._install_pyquaternion()
    G3._install_devkit_stub()
    _ref_env._pkg("pcseg.data.dataset.nuscenes", os.path.join(_ref_env.REF, "pcseg", "data", "dataset", "nuscenes"))
    _ref_env._pkg("tools", os.path.join(_ref_env.REF, "tools"))
    _ref_env._pkg("tools.utils", os.path.join(_ref_env.REF, "tools", "utils"))
    _ref_env._pkg("tools.utils.common", os.path.join(_ref_env.REF, "tools", "utils", "common"))
    for alias, typ in (("int", int), ("bool", bool), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)                              # aliases numpy >= 1.24 dropped
    from pcseg.data.dataset.nuscenes.nuscenes_ms_mm import NuscenesMsMmDataset as Ds
    from pcseg.data.dataset.nuscenes.nuscenes_voxel_ms_mm import NuscVoxelMsMmDataset as Vox
    with open(os.path.join(_ref_env.REF, "pcseg", "data", "dataset", "nuscenes", "nuscenes.yaml")) as f:
        learning_map = yaml.safe_load(f)["learning_map"]
    g = dict(np.load(os.path.join(HERE, "tiaf_nus.npz"), allow_pickle=False))
    scenes = [scene(g, b, Ds, learning_map) for b in range(2)]
    out = {"backend": np.array(G2.BACKEND_DESC), "cases": np.array(["train", "norot", "tta"])}

    # (i) training batch, (ii) without the rotation
    removed = train_case(out, "train", g, scenes, Vox, TRAIN_SEED, ALL_ON)
    removed_norot = train_case(out, "norot", g, scenes, Vox, NOROT_SEED, NO_ROTATION)
    assert not np.array_equal(out["train_batch_lidar_F"], g["batch_lidar_F"])

    # (iii) TTA: three votes of sample 0
    ds, files, index = scenes[0]
    vox = make_vox(Vox, ds, index, False)
    vox.if_tta, (vox.votes_min, vox.votes_max) = True, TTA_VOTES
    np.random.seed(TTA_SEED)
    with Served(files), Draws() as d:
        views = vox[0]
    rng = np.random.RandomState(TTA_SEED)
    params = [A.draw_tta_params(rng, v, vox.scale_range) for v in range(*TTA_VOTES)]
    removed_tta = [check_fov(g, 0, p, s, "tta") for p, s in zip(params, views)]
    batch = Vox.collate_batch_tta([views])
    assert all(name != "rand" for name, _, _ in d.log)
    GA.check_replay(d.log, params, tta=True)                     # one scale per vote and nothing else: no mix coin
    n_votes = len(params)
    out["tta_seed"], out["tta_sample"], out["tta_votes"] = np.array(TTA_SEED), np.array(0), np.array(TTA_VOTES)
    out["tta_fov_removed_kept"] = np.array(removed_tta)
    GA.store_params(out, "tta", params)
    img = np.concatenate([g["b0_image_ms"]] * n_votes).transpose(0, 3, 1, 2)
    sem = np.concatenate([g["b0_semantic_map_ms"]] * n_votes).transpose(0, 3, 1, 2)
    dump(out, "tta_batch_", batch, g, (img, sem))

    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB against", os.path.getsize(os.path.join(HERE, "tiaf_nus.npz")) // 1024,
          "KiB; FOV rows (removed, kept) per sample / vote:", removed, removed_norot, removed_tta, "fov voxels",
          out["train_batch_lidar_fov_ms_C"].shape, out["norot_batch_lidar_fov_ms_C"].shape, out["tta_batch_lidar_fov_ms_C"].shape)


if __name__ == "__main__":
    print("reference backend:", G2.BACKEND_DESC)
    main()
