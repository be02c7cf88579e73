"""Golden vectors of the range-view TRAINING stage (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_range_view_aug.py        ->  tests/golden/range_view_aug.npz  (data only)

The REAL `SemkittiRangeViewDataset.__getitem__` (pcseg/data/dataset/semantickitti/semantickitti_rv.py:121-192) runs on the CPU with its
augmentation on: the synthetic clouds of tests/range_view_aug_ref.fixture_clouds are written as .bin / .label files into a temporary
`sequences/00` tree, the dataset is built from a SimpleNamespace config, both global generators are seeded per case.  No reference
code in this file.  Stand-ins: those of make_golden_range_view.py, plus the identity for `generate_label` (the labels are training
labels already).

Stored (a committed file stays under 1 MiB, so the reference's float rows are kept as ONE 32-bit hash each - range_view_aug_ref.
word_hash - and compared by it; labels and masks are kept as values):
  clouds, labels      the scans, and `order`: which cloud the dataset globbed at which position
  per case            seed, index, switches, hw; the pixels that differ from the background: a bit map, per pixel the hash of the
                      five float channels, the mask and the label; the NEXT value of np.random.random() and random.random()
  per step combination (drop, flip, scale, rotate, jitter alone; all): the row count and the per-row hash of `A.points` after
                      LaserScan.open_scan, at STEP_SEED
  per (size, strategy) the CRC-32 of the two label images MixTeacherSemkitti's method makes of range_view_aug_ref.mix_probe
main() asserts what tests/test_range_view_aug_host.py relies on: the draws end at the same generator states, the restatement equals
the reference outside the excluded pixels, at most 1 % of a case's pixels are excluded, no paste class of a partner image is near
the threshold, both mixtures and at least four strategies occur, a paste class at or below 20 pixels and one above occur."""
import os
import random
import shutil
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_range_view as G  # noqa: E402
import range_view_aug_ref as A  # noqa: E402
from taseg_amd.data.range_view import RangeViewAug, draw_range_view_params  # noqa: E402


def aug_of(sw):
    return RangeViewAug(*[bool(v) for v in sw[:5]], *[float(v) for v in sw[5:]])


def config(root, sw, hw):
    names = ("IF_DROP", "IF_FLIP", "IF_SCALE", "IF_ROTATE", "IF_JITTER", "IF_RANGE_MIX", "IF_RANGE_SHIFT", "IF_RANGE_PASTE",
             "IF_RANGE_UNION")
    vals = [bool(v) for v in sw[:5]] + [float(v) for v in sw[5:]]
    return types.SimpleNamespace(DATA_PATH=root + "/", DATA_SPLIT={"train": "train", "test": "val"}, H=hw[0], W=hw[1],
                                 DATASET="semantickitti", **dict(zip(names, vals)))


def sparse(scan, label):
    """scan [6, h, w], label [1, h, w] -> the stored arrays"""
    rows = scan.reshape(6, -1).T
    lab = label.reshape(-1)
    differ = (rows.view(np.uint32) != A.BACKGROUND.view(np.uint32)).any(1) | (lab != 0)
    at = np.flatnonzero(differ)
    return {"bits": np.packbits(differ), "hash": A.float_hash(rows[at, :5]), "mask": np.packbits(rows[at, 5] != 0),
            "label": lab[at].astype(np.int8)}


def main(fname="range_view_aug.npz"):
    SemLaserScan, Dataset, _ = G.setup()
    Dataset.generate_label = lambda self, semantic_label: semantic_label
    import pcseg.data.dataset.semantickitti.semantickitti_rv as rv_mod
    clouds, labels = A.fixture_clouds()
    root = os.path.join(tempfile.gettempdir(), "rv_aug_fixture_%d" % os.getpid())
    assert "bin" not in root and "velodyne" not in root                  # the dataset rewrites these words in the whole path
    out, report = {}, []
    try:
        for sub in ("velodyne", "labels"):
            os.makedirs(os.path.join(root, "sequences", "00", sub))
        for i, (c, l) in enumerate(zip(clouds, labels)):
            c.tofile(os.path.join(root, "sequences", "00", "velodyne", "%06d.bin" % i))
            l.astype(np.uint32).tofile(os.path.join(root, "sequences", "00", "labels", "%06d.label" % i))
        for i, (c, l) in enumerate(zip(clouds, labels)):
            out["cloud%d" % i], out["label%d" % i] = c, l.astype(np.int8)
        order = None
        strategies, mixtures, paste_small, paste_large = set(), set(), False, False
        for name, (seed, index, sw, hw) in A.fixture_cases().items():
            ds = Dataset(config(root, sw, hw), training=True)
            this = [int(os.path.basename(f)[:6]) for f in ds.lidar_list]
            assert order is None or order == this
            order = this
            ds_clouds, ds_labels = [clouds[o] for o in order], [labels[o] for o in order]
            np.random.seed(seed)
            random.seed(seed)
            d = ds[index]
            next_np, next_py = np.random.random(), random.random()
            scan, label, mask = d["scan_rv"].numpy(), d["label_rv"].numpy(), d["mask_rv"].numpy()
            assert scan.shape == (6,) + tuple(hw) and scan.dtype == np.float32 and label.shape == (1,) + tuple(hw)
            assert label.dtype == np.int64 and np.array_equal(mask[0], scan[5])
            # the draws: same calls, same order - both generators end where the reference's do
            rs, pyr = np.random.RandomState(seed), random.Random(seed)
            aug = aug_of(sw)
            p = draw_range_view_params(aug, index, len(order), lambda i: len(ds_clouds[i]), rs, pyr, hw)
            assert rs.random_sample() == next_np and pyr.random() == next_py, name
            with_partners = p["partner"] is not None
            s, l, augd, err = A.train_batch(ds_clouds, ds_labels, [p], hw, with_partners=with_partners)
            assert err == 0
            excl = A.excluded_pixels(augd, [p], hw[0], hw[1], with_partners)[0]
            assert excl.mean() <= 0.01, (name, excl.mean())
            bad = ((s[0].view(np.uint32) != scan.view(np.uint32)).any(0) | (l[0, 0] != label[0])) & ~excl
            assert not bad.any(), (name, int(bad.sum()))
            if with_partners:
                # a class's pixel count can move only through a row of that class in a tainted pixel, by one per row
                pp, plab = augd[1]
                pr = A.R.project32(pp, np.zeros(len(pp), dtype=np.int32), np.zeros(1, dtype=np.int32), 1, hw[0], hw[1], labels=plab)
                counts = A.label_counts(pr["label_rv"])[0]
                near = A.tainted_pixels(pp, hw[0], hw[1])[pr["proj_y"], pr["proj_x"]]
                for c in A.PASTE_CLASSES:
                    margin = int((near & (plab == c)).sum())
                    assert counts[c] <= 20 - margin or counts[c] > 20 + margin, (name, c, counts[c], margin)
                if p["paste"]:
                    paste_small |= any(0 < counts[c] <= 20 for c in A.PASTE_CLASSES)
                    paste_large |= any(counts[c] > 20 for c in A.PASTE_CLASSES)
            if p["mixture"]:
                strategies.add(p["strategy"])
                mixtures.add(p["mixture"])
            for k, v in sparse(scan, label).items():
                out["%s_%s" % (name, k)] = v
            out[name + "_next"] = np.array([next_np, next_py], dtype=np.float64)
            report.append("%s: strategy %s mixture %d shift %d / %d paste %d union %d, excluded %d pixels, differ inside %d" % (
                name, p["strategy"], p["mixture"], p["shift"], p["partner_shift"], p["paste"], p["union"], excl.sum(),
                int(((s[0].view(np.uint32) != scan.view(np.uint32)).any(0) & excl).sum())))
        assert mixtures == {1, 2} and len(strategies) >= 4, (mixtures, strategies)
        assert paste_small and paste_large
        out["order"] = np.array(order, dtype=np.int32)
        # ---- A.points per step combination
        path = os.path.join(root, "sequences", "00", "velodyne", "%06d.bin" % 0)
        for combo, sw5 in A.STEP_COMBOS.items():
            flags = dict(zip(("if_drop", "if_flip", "if_scale", "if_rotate", "if_jitter"), [bool(v) for v in sw5]))
            a = SemLaserScan(nclasses=20, sem_color_dict={0: [0, 0, 0]}, project=True, H=64, W=512, fov_up=3.0, fov_down=-25.0, **flags)
            np.random.seed(A.STEP_SEED)
            a.open_scan(path)
            aug = RangeViewAug(*[bool(v) for v in sw5])
            p = draw_range_view_params(aug, 0, 1, lambda i: len(clouds[0]), np.random.RandomState(A.STEP_SEED), random.Random(0))
            mine, _ = A.augment_cloud(clouds[0], None, p["scan"])
            assert a.points.dtype == np.float32 and mine[:, :3].shape == a.points.shape, (combo, mine.shape, a.points.shape)
            assert np.array_equal(mine[:, :3].view(np.uint32), np.ascontiguousarray(a.points).view(np.uint32)), combo
            assert np.array_equal(mine[:, 3], a.remissions)
            out["step_" + combo] = A.float_hash(np.ascontiguousarray(a.points))
            report.append("step %s: %d rows, bit-equal" % (combo, len(a.points)))
        # ---- checkerboards
        mixer = rv_mod.MixTeacherSemkitti(strategy="col1row2")
        for h, w in A.MIX_SIZES:
            la, lb = A.mix_probe(h, w)
            img_a, img_b = np.stack([la] * 2).astype(np.float32), np.stack([lb] * 2).astype(np.float32)
            crcs = []
            for sname in A.strategy_names():
                r = getattr(mixer, sname)(img_a, la, la, img_b, lb, lb)
                for mixture, (img, lbl, msk) in ((1, r[:3]), (2, r[3:])):
                    assert lbl.shape == (h, w) and img.shape == (2, h, w), (sname, lbl.shape)
                    take = A.takes_partner(sname, mixture, h, w)
                    assert np.array_equal(lbl, np.where(take, lb, la)) and np.array_equal(msk, lbl), (sname, h, w, mixture)
                    assert np.array_equal(img[1], lbl.astype(np.float32))
                    crcs.append(zlib.crc32(np.ascontiguousarray(lbl).tobytes()))
            out["mix_%dx%d" % (h, w)] = np.array(crcs, dtype=np.uint32)
        report.append("checkerboards: %d strategies at %s equal the reference's methods" % (len(A.strategy_names()), A.MIX_SIZES))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB")
    print("\n".join(report))


if __name__ == "__main__":
    main()
