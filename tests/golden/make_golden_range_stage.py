"""Golden vectors of RPVNet's range-input stage (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_range_stage.py        ->  tests/golden/range_stage.npz  (data only)

The REAL reference's `SemkittiFusionDataset.get_range_image` (pcseg/data/dataset/semantickitti/semantickitti_fusion.py:64-114) runs on
two synthetic scans through the import environment of _ref_env.py, and its `collate_batch` lines pad the batch index; no reference
code in this file.  `np.random.seed(s)` precedes every call, so `np.random.RandomState(s).rand()` reproduces the cut
(taseg_amd/data/range.py: draw_range_cut).  `cv2` is not installed here: the stand-in `resize` asserts that the target size is the
image's own and returns the image - the identity the stage takes a 64 x 2048 -> 64 x 2048 resize to be.

Stored: the scans (x, y, z, reflectivity, ring), the cuts, per row the reference's integer column and row (recovered from its px / py,
which are exact functions of them), `range_pxpy` as the collate returns it, the images sparsely (the pixels that differ from the
background -10, -10, 0, 0, 0) and per row the float64 `proj_x` (tests/rpvnet_ref.py: proj_x64).  main() asserts that at most 1 % of
the rows lie within tests/rpvnet_ref.py's stage_delta() of a half-integer column - the rows tests/test_rpvnet_host.py leaves out."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_env  # noqa: E402
import rpvnet_ref as R  # noqa: E402
from taseg_amd.data.range import draw_range_cut  # noqa: E402
from taseg_amd.data.synthetic import ring_column, synth_scan  # noqa: E402

torch.set_num_threads(1)
SEEDS, CUT_SEEDS, POINTS, N_AZ, HW = (31, 32), (5, 6), 8000, 3000, (64, 2048)
BACKGROUND = np.array([-10, -10, 0, 0, 0], dtype=np.float32)


def same_size_resize(img, size, interpolation=None):
    assert tuple(size) == (img.shape[1], img.shape[0]), (size, img.shape)
    return img


def setup():
    _ref_env.setup_torchsparse()
    _ref_env.setup_pcseg()
    import cv2
    cv2.resize, cv2.INTER_LINEAR = same_size_resize, 1
    from pcseg.data.dataset.semantickitti.semantickitti_fusion import SemkittiFusionDataset
    return SemkittiFusionDataset


def scan(seed):
    pts, _ = synth_scan(seed, n_points=POINTS, n_beams=16, n_az=N_AZ)
    return np.concatenate([pts[:, :4], ring_column(pts, 16, HW[0])[:, None]], 1).astype(np.float32)


def reference_inputs(cls, scans, cut_seeds):
    """(range_image [B, 5, H, W], range_pxpy [n, 3] float32, cuts) through get_range_image; the batch index is padded in front and the rows cast
    to float32 as collate_batch does (:212-219: np.pad, concatenate, .float())"""
    images, pxpys, cuts = [], [], []
    for pts, s in zip(scans, cut_seeds):
        np.random.seed(s)
        image, pxpy = cls.get_range_image(None, pts.copy())
        cuts.append(draw_range_cut(np.random.RandomState(s)))
        images.append(image)
        pxpys.append(pxpy)
    pad = [np.pad(p, ((0, 0), (1, 0)), mode="constant", constant_values=i) for i, p in enumerate(pxpys)]
    got = torch.from_numpy(np.concatenate(pad, axis=0)).float().numpy()
    return np.stack(images), got, np.array(cuts)


def sparse_image(image):
    """(flat pixel indices over [B, H, W], their five values [k, 5]) of the pixels that differ from the background"""
    b, _, h, w = image.shape
    rows = image.transpose(0, 2, 3, 1).reshape(-1, 5)
    at = np.flatnonzero((rows != BACKGROUND).any(1))
    return at.astype(np.int32), rows[at].copy()


def main(fname="range_stage.npz"):
    cls = setup()
    scans = [scan(s) for s in SEEDS]
    image, pxpy, cuts = reference_inputs(cls, scans, CUT_SEEDS)
    points = np.concatenate(scans)
    batch = np.concatenate([np.full(len(s), i, dtype=np.int32) for i, s in enumerate(scans)])
    h, w = HW
    col = np.rint((pxpy[:, 1].astype(np.float64) / 2.0 + 0.5) * (w - 1)).astype(np.int32)
    row = np.rint((pxpy[:, 2].astype(np.float64) / 2.0 + 0.5) * (h - 1)).astype(np.int32)
    assert np.array_equal((2.0 * (col / (w - 1) - 0.5)).astype(np.float32), pxpy[:, 1])          # px / py are functions of them
    assert np.array_equal((2.0 * (row / (h - 1) - 0.5)).astype(np.float32), pxpy[:, 2])
    px64 = R.proj_x64(points, batch, cuts, w)
    delta = R.stage_delta(w)
    near = np.abs(px64 - np.floor(px64) - 0.5) <= delta
    assert near.mean() <= 0.01, near.mean()
    ours = R.range_stage32(points, batch, cuts, h, w)
    differ = ours["col"] != col
    assert not (differ & ~near).any() and np.array_equal(ours["row"], row)
    at, vals = sparse_image(image)
    assert len(np.unique(batch.astype(np.int64) * h * w + row * w + col)) < len(points)          # two rows in one pixel
    out = {"points": points, "batch": batch, "cuts": cuts, "hw": np.array(HW), "col": col, "row": row, "range_pxpy": pxpy,
           "image_at": at, "image_values": vals, "proj_x64": px64, "delta": np.array(delta)}
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB; rows", len(points), "pixels set", len(at), "delta %.3g" % delta, "rows near a half-integer",
          int(near.sum()), "of which the restatement differs at", int(differ.sum()))


if __name__ == "__main__":
    main()
