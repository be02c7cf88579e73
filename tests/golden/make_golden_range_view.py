"""Golden vectors of the range-view projection and kNN step (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_range_view.py        ->  tests/golden/range_view.npz  (data only)

The REAL reference's `SemLaserScan` (pcseg/data/dataset/semantickitti/laserscan.py), `SemkittiRangeViewDataset.
prepare_input_label_semantic_with_mask` (semantickitti_rv.py:284-301) and `KNN` (pcseg/model/segmentor/range/utils.py:291-341) run on
the CPU on synthetic inputs (tests/range_view_ref.py makes them from seeds, so the fixture stores the clouds but only the PARAMETERS
of the kNN cases); no reference code in this file.  Stand-ins, written here:

  torchvision.transforms.functional.to_tensor   torchvision is not installed: an [H, W, C] (or [H, W]) array to a [C, H, W] tensor,
                                                values unchanged - what to_tensor does with a non-uint8 ndarray
  cv2, yaml (if missing)                        empty modules: imported by the reference's files, not used on this path
  np.float                                      = float: SemLaserScan.reset uses the alias removed in numpy >= 1.24
  generate_label                                the labels are training labels already (the identity map)
  default collate                               torch.stack of the per-scan tensors

Stored for the projection: the clouds and labels, per row the reference's proj_x / proj_y / unproj_range at 64 x 512 and its columns
and rows at 64 x 2048, the images sparsely (the pixels with a point: scan_rv's six values, range, index, label).  For the kNN step:
per case the reference's labels.  main() asserts the conditions tests/test_range_view_host.py holds the fixture to: at most 1 % of the
rows undecided, no disagreement outside them; no undecided point on the continuous kNN cases, at least 80 % decided on the quantised
ones, no disagreement at a decided point."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_env  # noqa: E402
import range_view_ref as R  # noqa: E402
from taseg_amd.data.range_view import knn_weight  # noqa: E402

torch.set_num_threads(1)
SEEDS, POINTS, HW, HW_WIDE, FOV = (41, 42), (6000, 5000), (64, 512), (64, 2048), (3.0, -25.0)


def to_tensor(pic):
    if pic.ndim == 2:
        pic = pic[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1))))


def setup():
    for name in ("cv2", "yaml", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.modules["torchvision.transforms.functional"].to_tensor = to_tensor
    if not hasattr(np, "float"):
        np.float = float
    sys.path.insert(0, _ref_env.REF)
    base = os.path.join(_ref_env.REF, "pcseg")
    for name, sub in (("pcseg", ()), ("pcseg.data", ("data",)), ("pcseg.data.dataset", ("data", "dataset")),
                      ("pcseg.data.dataset.semantickitti", ("data", "dataset", "semantickitti")), ("pcseg.model", ("model",)),
                      ("pcseg.model.segmentor", ("model", "segmentor")), ("pcseg.model.segmentor.range", ("model", "segmentor", "range"))):
        _ref_env._pkg(name, os.path.join(base, *sub))
    from pcseg.data.dataset.semantickitti.laserscan import SemLaserScan
    from pcseg.data.dataset.semantickitti.semantickitti_rv import SemkittiRangeViewDataset
    from pcseg.model.segmentor.range.utils import KNN
    return SemLaserScan, SemkittiRangeViewDataset, KNN


def reference_scan(SemLaserScan, Dataset, pts, labels, hw):
    """one scan through the reference: what __getitem__ returns without augmentation, plus the LaserScan's per-row arrays"""
    a = SemLaserScan(nclasses=20, sem_color_dict={0: [0, 0, 0]}, project=True, H=hw[0], W=hw[1], fov_up=FOV[0], fov_down=FOV[1])
    a.set_points(pts[:, :3].copy(), pts[:, 3].copy())
    a.set_label(labels.astype(np.uint32))
    sample = {"xyz": a.proj_xyz, "intensity": a.proj_remission, "range_img": a.proj_range, "xyz_mask": a.proj_mask,
              "semantic_label": a.proj_sem_label}
    scan, label, mask = Dataset.prepare_input_label_semantic_with_mask(types.SimpleNamespace(H=hw[0], W=hw[1]), sample)
    F = sys.modules["torchvision.transforms.functional"]
    return {"scan_rv": F.to_tensor(scan), "label_rv": F.to_tensor(label).to(dtype=torch.long), "mask_rv": F.to_tensor(mask),
            "proj_x": a.proj_x.copy(), "proj_y": a.proj_y.copy(), "unproj_range": a.unproj_range.copy(),
            "proj_range": a.proj_range.copy(), "proj_idx": a.proj_idx.copy()}


def reference_knn(KNN, case, search, knn, cutoff, nclasses):
    """the reference's module, one scan at a time as it is used, on the CPU"""
    mod = KNN({"knn": knn, "search": search, "sigma": 1.0, "cutoff": cutoff}, nclasses)
    out = np.zeros(len(case["batch"]), dtype=np.int64)
    for b in range(case["proj_range"].shape[0]):
        at = np.flatnonzero(case["batch"] == b)
        if len(at) == 0:
            continue
        got = mod(torch.from_numpy(case["proj_range"][b].copy()), torch.from_numpy(case["unproj_range"][at]),
                  torch.from_numpy(case["proj_class"][b].astype(np.int64)), torch.from_numpy(case["px"][at].astype(np.int64)),
                  torch.from_numpy(case["py"][at].astype(np.int64)))
        out[at] = got.numpy()
    return out


def main(fname="range_view.npz"):
    SemLaserScan, Dataset, KNN = setup()
    clouds = [R.synth_cloud(s, n) for s, n in zip(SEEDS, POINTS)]
    labels = [np.random.RandomState(s + 7).randint(0, 20, n).astype(np.int32) for s, n in zip(SEEDS, POINTS)]
    points = np.concatenate(clouds)
    batch = np.concatenate([np.full(len(c), i, dtype=np.int32) for i, c in enumerate(clouds)])
    first = np.concatenate([[0], np.cumsum(POINTS)[:-1]]).astype(np.int32)
    out = {"points": points, "labels": np.concatenate(labels), "batch": batch, "first": first, "hw": np.array(HW),
           "hw_wide": np.array(HW_WIDE), "fov": np.array(FOV)}
    report = []
    for tag, hw in (("", HW), ("_wide", HW_WIDE)):
        refs = [reference_scan(SemLaserScan, Dataset, c, l, hw) for c, l in zip(clouds, labels)]
        h, w = hw
        px = np.concatenate([r["proj_x"] for r in refs]).astype(np.int32)
        py = np.concatenate([r["proj_y"] for r in refs]).astype(np.int32)
        ours = R.project32(points, batch, first, len(clouds), h, w, *FOV, labels=out["labels"])
        undecided = R.project_undecided(points, h, w, *FOV)
        differ = (ours["proj_x"] != px) | (ours["proj_y"] != py)
        assert undecided.mean() <= 0.01, undecided.mean()
        assert not (differ & ~undecided).any()
        out["proj_x" + tag], out["proj_y" + tag] = px, py
        report.append("%d x %d: undecided %d (%.3f %%), differ %d" % (h, w, undecided.sum(), 100 * undecided.mean(), differ.sum()))
        if tag:
            continue
        unproj = np.concatenate([r["unproj_range"] for r in refs]).astype(np.float32)
        assert np.array_equal(unproj.view(np.uint32), ours["unproj_range"].view(np.uint32))          # depths: bit-equal at every row
        scan_rv = torch.stack([r["scan_rv"] for r in refs]).numpy()                                   # the default collate
        label_rv = torch.stack([r["label_rv"] for r in refs]).numpy()
        mask_rv = torch.stack([r["mask_rv"] for r in refs]).numpy()
        assert scan_rv.shape == (2, 6, h, w) and scan_rv.dtype == np.float32 and label_rv.shape == (2, 1, h, w)
        assert label_rv.dtype == np.int64 and np.array_equal(mask_rv[:, 0], scan_rv[:, 5])
        idx = np.stack([r["proj_idx"] for r in refs])
        rng = np.stack([r["proj_range"] for r in refs])
        at = np.flatnonzero(idx.reshape(-1) >= 0)
        # every pixel without a point holds the background
        bg = np.array([-1 / np.float32(50), -1 / np.float32(50), -1 / np.float32(3), -1, -1 / np.float32(80), 0], dtype=np.float32)
        rows = scan_rv.transpose(0, 2, 3, 1).reshape(-1, 6)
        empty = np.setdiff1d(np.arange(len(rows)), at)
        assert (rows[empty] == bg).all() and (rng.reshape(-1)[empty] == -1).all() and (label_rv.reshape(-1)[empty] == 0).all()
        out.update({"unproj_range": unproj, "image_at": at.astype(np.int32), "image_scan": rows[at].copy(),
                    "image_range": rng.reshape(-1)[at].copy(), "image_idx": idx.reshape(-1)[at].astype(np.int32),
                    "image_label": label_rv.reshape(-1)[at].astype(np.int8)})
    # ---- kNN
    for name, (spec, search, knn, cutoff, nclasses, continuous) in R.knn_cases().items():
        case = R.knn_case_inputs(spec)
        ref = reference_knn(KNN, case, search, knn, cutoff, nclasses)
        weight = knn_weight(search, 1.0).numpy()
        mine, err, undecided = R.knn32(case["proj_range"], case["proj_class"], case["unproj_range"], case["px"], case["py"],
                                       case["batch"], weight, knn, search, cutoff, nclasses)
        differ = mine != ref
        assert err == 0
        assert not (differ & ~undecided).any(), (name, int((differ & ~undecided).sum()))
        if continuous:
            assert not undecided.any(), (name, int(undecided.sum()))
        elif not isinstance(spec, str):
            assert undecided.mean() <= 0.2, (name, undecided.mean())
        out["knn_" + name] = ref.astype(np.int8)
        report.append("knn %s: points %d undecided %d differ %d" % (name, len(ref), undecided.sum(), differ.sum()))
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB")
    print("\n".join(report))


if __name__ == "__main__":
    main()
