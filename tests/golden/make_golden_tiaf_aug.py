"""Golden vectors of the TIAF recipe's training augmentation, image flip and TTA views (build container only: it runs the reference,
which _ref_env locates; nothing here is imported by the tests or the product).

    python tests/golden/make_golden_tiaf_aug.py

Runs the REAL `SemantickittiMsMmDataset.__getitem__` (semantickitti_ms_mm.py:143-461, on a bare object, with `np.fromfile` /
`np.load` / `Image.open` served from a dict as make_golden_r2.gen_tiaf_data does), then `SemkittiVoxelMsMmDataset.get_single_sample`
+ `collate_batch` / `collate_batch_tta` (semantickitti_voxel_ms_mm.py:68-330), on the two sequences of tiaf_data.npz - their scans,
labels, poses, calibration and (cases a, c) camera frames are read from that file and not stored again.

  tiaf_aug.npz   `train`  (a) a training batch of both samples: IMAGE_FLIP on, all four point augmentations on, `np.random.seed(seed)`
                          before `ds[T]` of each sample; seeds 1 and 6 flip frames (T, F, T) and (F, T, F), oldest frame first.
                          Images 64 x 180 against the 60 x 192 crop: rows cropped, columns padded.
                 `wide`   (b) the same seeds with images 56 x 200 - WIDER than the crop, so the flip changes which points pass the
                          crop test and which part of the image is kept - and the point augmentation off (`training = False`).  The
                          images are `wide_image(seed)` below: the seeds are stored, the tests draw the same arrays.  The LiDAR keys
                          equal tiaf_data.npz's batch (asserted here) and are not stored again.
                 `tta`    (c) votes 1 .. 3 of sample 0 through `collate_batch_tta`, seed 11.  Every vote carries the same images
                          (asserted here): stored once.
                 per case the values the reference DREW, recorded by wrapping numpy's generator functions while it ran: the flip
                 draws (`rand`), the mix coin (`choice(2, 1)`, semantickitti_ms_mm.py:178: drawn for every `__getitem__`, not used
                 under AUGMENT 'none'), theta / scale / flip type / translation.  Coordinates that two keys share are stored once.

The voxel dataset augments `xyzret_ms` and `xyzret_fov_ms` IN PLACE through views and a real dataset re-reads the sample on every
access, so `point_cloud_dataset` here is `Live`: every access runs `ds[T]` again - which is also what puts the flip draws and
the coin in front of the augmentation's draws, per sample and, under TTA, per vote.

Every case is also checked HERE, on the CPU: replaying np.random.RandomState(seed) through draw_image_flips, mix.draw_coin and
draw_train_params / draw_tta_params gives the recorded draws in the recorded ORDER.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_aug as GA  # noqa: E402  (arranges the reference's imports)

R2, _ref_env = GA.R2, GA._ref_env
from taseg_amd.data import augment as A  # noqa: E402
from taseg_amd.data import mix as M  # noqa: E402
from taseg_amd.data import tiaf as TF  # noqa: E402

VOXEL = 0.05
SPARSE = ("lidar", "lidar_ms", "lidar_fov_ms", "inverse_map", "inverse_map_ms", "targets", "targets_ms", "targets_mapped",
          "targets_mapped_ms")
SAME_COORDS = {"targets": "lidar", "targets_ms": "lidar_ms", "targets_mapped": "inverse_map", "targets_mapped_ms": "inverse_map_ms"}
DENSE = ("num_points", "num_points_ms", "offset", "offset_ms", "point_mask", "offset_img")
TRAIN_SEEDS, TTA_SEED, TTA_VOTES = (1, 6), 11, (1, 4)
WIDE = (56, 200)


def wide_image(seed, h=WIDE[0], w=WIDE[1]):
    """(uint8 [h, w, 3] image, float32 [h, w, 1] semantic map) of case `wide`: the tests draw the same arrays from the stored seed"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8), rs.randint(0, 20, size=(h, w, 1)).astype(np.float32)


class Draws(GA.Draws):
    """... and `np.random.rand`, the flip draw (semantickitti_ms_mm.py:436)"""

    def __enter__(self):
        super().__enter__()
        self.real["rand"] = np.random.rand
        np.random.rand = self._wrap("rand", self.real["rand"])
        return self


class Served:
    """np.fromfile / np.load / Image.open from a dict; np.array(copy=False) as numpy 1.x understood it (:428)"""

    def __init__(self, files):
        self.files = files

    def __enter__(self):
        from PIL import Image
        self.Image = Image
        self.real = np.fromfile, np.load, Image.open, np.array
        files, real_array = self.files, np.array
        np.fromfile = lambda path, dtype=None, **kw: files[path].copy()
        np.load = lambda path, *a, **kw: files[path].copy()
        Image.open = lambda path, *a, **kw: Image.fromarray(files[path])
        np.array = lambda obj, *a, copy=True, **kw: real_array(obj, *a, copy=(None if copy is False else copy), **kw)
        return self

    def __exit__(self, *exc):
        np.fromfile, np.load, self.Image.open, np.array = self.real


class Live:
    """the frame reader of the voxel dataset: every access is the real `__getitem__` again"""

    def __init__(self, ds, index):
        self.ds, self.index = ds, index

    def __len__(self):
        return 1

    def __getitem__(self, _):
        return self.ds[self.index]


def sequence(g, b, images=None):
    """(files, poses, camera frames t) of sample b of tiaf_data.npz; images: {t: (image, semantic map)} instead of the stored ones"""
    T, step = int(g["T"]), int(g["step_image"])
    files, poses = {}, []
    cams = [t for t in range(T + 1) if (T - t) % step == 0]
    for t in range(T + 1):
        path = f"/data/sequences/00/velodyne/{t:06d}.bin"
        files[path] = g[f"b{b}_points_t{t}"]
        files[path.replace("velodyne", "labels")[:-3] + "label"] = g[f"b{b}_rawlabels_t{t}"].reshape(-1, 1)
        poses.append(g[f"b{b}_pose_t{t}"])
        if t in cams:
            img, sem = images[t] if images is not None else (g[f"b{b}_image_t{t}"], g[f"b{b}_semantic_t{t}"])
            files[path.replace("velodyne", "image_2").replace(".bin", ".png")] = img
            files[path.replace("velodyne", "semantic_map_dilate").replace(".bin", ".npy")] = sem
    return files, poses, cams


def bare_dataset(cls, g, poses, image_flip):
    T = int(g["T"])
    ds = object.__new__(cls)
    ds.poses, ds.proj_matrix = {0: poses}, {0: g["proj"]}
    ds.only_history, ds.split, ds.seq, ds.pseudo_mask, ds.trainval_seqs = True, "val", -1, "gt", ["00"]
    ds.if_scribble, ds.augment, ds.dynamic_step, ds.fov_dist = False, "none", False, -1
    ds.multiscan, ds.flexible_steps = int(g["multiscan"]), g["steps"].tolist()
    ds.multiscan_image, ds.step_image = int(g["multiscan_image"]), int(g["step_image"])
    ds.height, ds.width, ds.image_jitter, ds.image_flip, ds.flip_ratio = int(g["height"]), int(g["width"]), False, image_flip, 0.5
    ds.annos = [f"/data/sequences/00/velodyne/{t:06d}.bin" for t in range(T + 1)]
    ds.annos_another = list(ds.annos)
    return ds


def make_vox(cls, ds, T, training):
    vox = GA.make_vox(cls, [], 5, VOXEL, training)
    vox.point_cloud_dataset, vox.eval_range = Live(ds, T), [0, 1000]
    return vox


def replay_sample(log, seed, cams_delta, image_flip, training):
    """the recorded draws of one `get_single_sample` == flips, coin, augmentation taken from RandomState(seed), in this order"""
    rng = np.random.RandomState(seed)
    flips = TF.draw_image_flips(rng, cams_delta, image_flip=image_flip)
    coin = M.draw_coin(rng)
    p = A.draw_train_params(rng) if training else None
    k = len(cams_delta) if image_flip else 0
    for (name, _, v), d in zip(log[:k], sorted(cams_delta)):
        assert name == "rand" and bool(v < 0.5) == flips[d], (name, v, d)
    name, a, v = log[k]
    assert name == "choice" and tuple(a) == (2, 1) and int(v[0]) == coin, log[k]
    GA.check_replay(log[k + 1:], [p] if training else [])
    return flips, coin, p


def dump(out, prefix, batch, sparse=SPARSE, images=slice(None)):
    for key in sparse:
        if key in SAME_COORDS:
            assert np.array_equal(batch[key].C.numpy(), batch[SAME_COORDS[key]].C.numpy()), key
        else:
            out[f"{prefix}{key}_C"] = batch[key].C.numpy()
        out[f"{prefix}{key}_F"] = batch[key].F.numpy()
    for key in DENSE:
        out[f"{prefix}{key}"] = batch[key].numpy()
    img = batch["image_ms"].numpy()
    out[f"{prefix}image_ms_shape"] = np.array(img.shape)
    out[f"{prefix}image_ms_sub"] = img[images, :, ::3, ::3].copy()             # NCHW, every 3rd pixel
    out[f"{prefix}semantic_map_ms"] = batch["semantic_map_ms"].numpy()[images].copy()


def run_batch(out, c, g, Ds, Vox, images, training):
    """cases a / b: both samples, IMAGE_FLIP on, np.random.seed(seed) before ds[T] of each"""
    T = int(g["T"])
    samples, flips_all, coins, params = [], [], [], []
    for b, seed in enumerate(TRAIN_SEEDS):
        files, poses, cams = sequence(g, b, None if images is None else images[b])
        vox = make_vox(Vox, bare_dataset(Ds, g, poses, True), T, training)
        with Served(files), Draws() as d:
            np.random.seed(seed)
            samples.append(vox.get_single_sample(0))
        flips, coin, p = replay_sample(d.log, seed, [t - T for t in cams], True, training)
        assert len(set(flips.values())) == 2, "every sample needs a flipped and an un-flipped frame"
        flips_all.append([flips[d_] for d_ in sorted(flips)])
        coins.append(coin)
        params.append(p)
    out[f"{c}_seeds"], out[f"{c}_flips"], out[f"{c}_coin"] = np.array(TRAIN_SEEDS), np.array(flips_all), np.array(coins)
    out[f"{c}_camera_deltas"] = np.array(sorted(t - T for t in cams))
    if training:
        GA.store_params(out, c, params)
    return Vox.collate_batch(samples)


def main(fname="tiaf_aug.npz"):
    sys.modules.setdefault("mmcv", types.ModuleType("mmcv"))
    for alias, typ in (("int", int), ("bool", bool), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)
    _ref_env.setup_datasets()
    from pcseg.data.dataset.semantickitti.semantickitti_ms_mm import SemantickittiMsMmDataset as Ds
    from pcseg.data.dataset.semantickitti.semantickitti_voxel_ms_mm import SemkittiVoxelMsMmDataset as Vox
    g = dict(np.load(os.path.join(HERE, "tiaf_data.npz"), allow_pickle=False))
    T = int(g["T"])
    out = {"backend": np.array(R2.BACKEND_DESC), "cases": np.array(["train", "wide", "tta"])}

    # (a) training batch
    batch = run_batch(out, "train", g, Ds, Vox, None, True)
    dump(out, "train_batch_", batch)
    assert not np.array_equal(batch["lidar"].F.numpy(), g["batch_lidar_F"])

    # (b) wide images, the point augmentation off
    seeds = np.array([[7000 + 100 * b + t for t in sequence(g, b)[2]] for b in range(2)])
    images = [{t: wide_image(int(s)) for t, s in zip(sequence(g, b)[2], seeds[b])} for b in range(2)]
    batch = run_batch(out, "wide", g, Ds, Vox, images, False)
    out["wide_image_seeds"], out["wide_image_shape"] = seeds, np.array(WIDE)
    for key in SPARSE:
        if key != "lidar_fov_ms":       # the flip touches the camera side alone
            assert np.array_equal(batch[key].C.numpy(), g[f"batch_{key}_C"]) and np.array_equal(batch[key].F.numpy(), g[f"batch_{key}_F"])
    dump(out, "wide_batch_", batch, sparse=("lidar_fov_ms",))
    fov = batch["lidar_fov_ms"].F.numpy()
    assert fov[:, 5].max() < int(g["width"]) and out["wide_batch_image_ms_sub"][:, :, :, -1].any()     # no padding column left

    # (c) TTA: three votes of sample 0
    files, poses, cams = sequence(g, 0)
    vox = make_vox(Vox, bare_dataset(Ds, g, poses, False), T, False)
    vox.if_tta, (vox.votes_min, vox.votes_max) = True, TTA_VOTES
    with Served(files), Draws() as d:
        np.random.seed(TTA_SEED)
        batch = Vox.collate_batch_tta([vox[0]])
    rng = np.random.RandomState(TTA_SEED)
    coins, params, log = [], [], list(d.log)
    for v in range(*TTA_VOTES):                     # every vote re-reads the sample: the coin, then the scale
        coins.append(M.draw_coin(rng))
        params.append(A.draw_tta_params(rng, v, vox.scale_range))
        name, a, val = log.pop(0)
        assert name == "choice" and tuple(a) == (2, 1) and int(val[0]) == coins[-1]
        GA.check_replay(log[:1], params[-1:], tta=True)
        log.pop(0)
    assert not log
    out["tta_seed"], out["tta_sample"], out["tta_votes"], out["tta_coin"] = np.array(TTA_SEED), np.array(0), np.array(TTA_VOTES), np.array(coins)
    GA.store_params(out, "tta", params)
    img, sem, k = batch["image_ms"].numpy(), batch["semantic_map_ms"].numpy(), len(cams)
    for v in range(1, len(params)):
        assert np.array_equal(img[:k], img[v * k:(v + 1) * k]) and np.array_equal(sem[:k], sem[v * k:(v + 1) * k])
    dump(out, "tta_batch_", batch, images=slice(0, k))

    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB; flips", out["train_flips"].tolist(), out["wide_flips"].tolist(),
          "fov voxels", out["train_batch_lidar_fov_ms_C"].shape, out["wide_batch_lidar_fov_ms_C"].shape, out["tta_batch_lidar_fov_ms_C"].shape,
          "against", g["batch_lidar_fov_ms_C"].shape)


if __name__ == "__main__":
    print("reference backend:", R2.BACKEND_DESC)
    main()
