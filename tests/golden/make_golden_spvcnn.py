"""Golden vectors of the SPVCNN segmentor (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_spvcnn.py        ->  tests/golden/model_spvcnn.npz  (data only)

Same arrangement as make_golden.py: the REAL reference's Python (pcseg/model/segmentor/fusion/spvcnn/spvcnn.py, its torchsparse
v1.4.0, its Losses) runs on the CPU through the import environment of _ref_env.py; no reference code in this file.

  batch   the two-scan recipe of make_golden.py's MinkUNet fixture (seeds 21 / 22, the reference's voxelisation lines through its
          library calls, sparse_collate_fn) with POINTS points per scan, plus what the evaluation branch reads - inverse_map,
          targets_mapped, num_points, name - laid out as semantickitti_voxel.py:146-153 returns them.
  model   SPVCNN, make_model_cfg("SPVCNN", in_dim=4, cr=0.5, num_layer=[1] * 8, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0),
          fill_parameters(PARAM_SEED); BatchNorm in training mode ("train") and on running statistics ("eval", training branch), and
          the evaluation branch.  For BLOCK="Bottleneck": state_dict keys and shapes only.

Gradients of tensors above 8192 elements are stored as `strided_sample`s (the fixture stays under 1 MiB); `*_gradnorms` covers every
parameter whole.  `--search` prints the first parameter seed that passes the margin rule below.
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import _ref_env  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample, synth_scan  # noqa: E402

torch.set_num_threads(1)
VOXEL = 0.05
SEEDS = (21, 22)
# points per scan: make_golden.py's 1500 leave no voxel with more rows than a piece of the mean rule (P rows, include/taseg_hip.h
# ts_voxelize_mean_forward), so the count is raised to everything the recipe's 16 x 360 grid of rays yields (5760 points a scan): a
# stride-16 voxel then holds 43 rows.  main() asserts that this exceeds P.  At stride 4 it cannot: the rows are distinct stride-1
# voxels, a stride-4 voxel holds at most 64 of them and a scanned surface fills ~5 here; the first such voxel above 16 rows
# appears at 24 000 points a scan, whose logits alone are four times the size a committed fixture may have.  The pieces at stride
# 4 are covered by tests/test_gpu_spvcnn_kernels.py, bit for bit, not by this fixture; `most_rows` records the counts.
POINTS = 8000
# rows of the per-voxel logits that are stored (11 520 rows x 20 classes x three passes do not fit the fixture)
LOGIT_STEP = 6
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
KEEP = ["stem.0.kernel", "stage1.0.net.0.kernel", "stage4.1.net.0.kernel", "up1.0.net.0.kernel", "up4.1.0.net.3.kernel",
        "classifier.0.weight", "classifier.0.bias", "point_transforms.0.0.weight", "point_transforms.0.1.weight",
        "point_transforms.1.0.weight", "point_transforms.1.1.bias", "point_transforms.2.0.weight", "point_transforms.2.1.bias"]
# (no bias of a point-transform Linear: BatchNorm in training mode removes the mean behind it, its exact gradient is zero and what the
# reference stores is rounding noise; `*_gradnorms` covers them with an absolute floor)
FULL_BELOW = 8192
MARGIN = 2e-3
# parameter seed: the first of 0, 1, 2 ... at which the evaluation branch leaves at most 1 % of the points with a top-2 logit margin
# <= MARGIN (`--search` finds it; main() asserts that this one passes)
PARAM_SEED = 3


def setup():
    desc = _ref_env.setup_torchsparse()
    _ref_env.setup_pcseg()
    base = os.path.join(_ref_env.REF, "pcseg", "model", "segmentor", "fusion")
    _ref_env._pkg("pcseg.model.segmentor.fusion", base)
    _ref_env._pkg("pcseg.model.segmentor.fusion.spvcnn", os.path.join(base, "spvcnn"))
    from pcseg.model.segmentor.fusion.spvcnn.spvcnn import SPVCNN
    return desc, SPVCNN


def make_batch():
    from torchsparse import SparseTensor
    from torchsparse.utils.collate import sparse_collate_fn
    from torchsparse.utils.quantize import sparse_quantize
    samples = []
    for s in SEEDS:
        pts, lab = synth_scan(s, n_points=POINTS, n_beams=16, n_az=360)
        pc_ = np.round(pts[:, :3] / VOXEL).astype(np.int32)                 # semantickitti_voxel.py:119-137 through the library calls
        pc_ -= pc_.min(0, keepdims=1)
        _, inds, inverse = sparse_quantize(pc_, return_index=True, return_inverse=True)
        samples.append({"name": "scan%d" % s, "lidar": SparseTensor(pts[inds], pc_[inds]), "targets": SparseTensor(lab[inds], pc_[inds]),
                        "targets_mapped": SparseTensor(lab, pc_), "inverse_map": SparseTensor(inverse, pc_),
                        "num_points": np.array([len(pts)])})
    batch = sparse_collate_fn(samples)
    batch["lidar"].F, batch["lidar"].C = batch["lidar"].F.float(), batch["lidar"].C.int()
    batch["offset"] = torch.tensor([0])
    return batch


def clone(batch):
    from torchsparse import SparseTensor
    out = {}
    for k, v in batch.items():
        out[k] = SparseTensor(v.F.clone(), v.C.clone()) if isinstance(v, SparseTensor) else (v.clone() if torch.is_tensor(v) else v)
    return out


def rows_per_voxel(coords, stride):
    """rows (stride-1 voxels of the batch) per stride-`stride` voxel, counted with numpy"""
    cell = np.concatenate([coords[:, :3] // stride, coords[:, 3:]], 1)
    return np.unique(cell, axis=0, return_counts=True)[1]


def run(cls, batch, bn_training, seed):
    model = fill_parameters(cls(make_model_cfg("SPVCNN", **CFG), 20), seed=seed)
    model.train()
    if not bn_training:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    got = {}
    handle = model.classifier.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach()))
    ret, _, _ = model(clone(batch))
    handle.remove()
    model.zero_grad()
    ret["loss"].backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    tag = "train" if bn_training else "eval"
    res = {f"{tag}_logits": got["logits"].numpy()[::LOGIT_STEP].copy(), f"{tag}_loss": np.array(ret["loss"].item()),
           f"{tag}_gradnorms": np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])}
    for k in KEEP:
        g = grads[k]
        res[f"{tag}_grad/{k}"] = (g if g.numel() <= FULL_BELOW else strided_sample(g)).numpy().copy()
    return res


def branch(cls, batch, seed):
    """the evaluation branch (model.eval()): per-point logits, predictions, labels and top-2 margins over the batch"""
    model = fill_parameters(cls(make_model_cfg("SPVCNN", **CFG), 20), seed=seed).eval()
    with torch.no_grad():
        ev = model(clone(batch))
    logits = np.concatenate(ev["point_predict_logits"])
    top2 = np.sort(logits, axis=1)[:, -2:]
    return ev, logits, (top2[:, 1] - top2[:, 0]).astype(np.float32)


def main(fname="model_spvcnn.npz"):
    desc, cls = setup()
    batch = make_batch()
    if "--search" in sys.argv:
        for seed in range(80):
            left_out = float((branch(cls, batch, seed)[2] <= MARGIN).mean())
            print("seed", seed, "margin <= %g: %.3f %%" % (MARGIN, 100 * left_out), flush=True)
            if left_out <= 0.01:
                return
        raise SystemExit("no seed passes")
    coords = batch["lidar"].C.numpy()
    most = {s: int(rows_per_voxel(coords, s).max()) for s in (1, 4, 16)}
    from taseg_amd import backend as B
    piece = B.voxelize_mean_piece_rows()
    assert most[16] > piece, (most, piece)                     # stride 16 cuts a voxel into pieces (stride 4: see POINTS)
    out = {"backend": np.array(desc), "cfg": np.array(repr(sorted(CFG.items()))), "full_below": np.array(FULL_BELOW),
           "margin": np.array(MARGIN), "param_seed": np.array(PARAM_SEED), "most_rows": np.array([most[1], most[4], most[16]]),
           "piece_rows": np.array(piece), "logit_step": np.array(LOGIT_STEP),
           "coords": coords.copy(), "feats": batch["lidar"].F.numpy().copy(), "labels": batch["targets"].F.numpy().astype(np.int64),
           "inverse_map": batch["inverse_map"].F.numpy().astype(np.int64),
           "point_batch": batch["inverse_map"].C[:, -1].numpy().astype(np.int32),
           "point_labels": batch["targets_mapped"].F.numpy().astype(np.uint8),
           "num_points": batch["num_points"].numpy().reshape(-1).astype(np.int64), "name": np.array(batch["name"])}
    for bn_training in (True, False):
        out.update(run(cls, batch, bn_training, PARAM_SEED))
    ev, logits, margin = branch(cls, batch, PARAM_SEED)
    n_pts = out["num_points"].tolist()
    assert [len(p) for p in ev["point_predict"]] == n_pts and ev["name"] == batch["name"]
    left_out = float((margin <= MARGIN).mean())
    assert left_out <= 0.01, left_out
    # the branch's logits are rows of the per-voxel logits on running statistics: stored per VOXEL ("branch_logits", every
    # LOGIT_STEP-th row, read through inverse_map); asserted bit for bit here
    model = fill_parameters(cls(make_model_cfg("SPVCNN", **CFG), 20), seed=PARAM_SEED).eval()
    got = {}
    model.classifier.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().numpy()))
    with torch.no_grad():
        model(clone(batch))
    start = np.concatenate([[0], np.cumsum([(coords[:, 3] == b).sum() for b in range(len(SEEDS))])])
    rows = out["inverse_map"] + start[out["point_batch"]]
    assert np.array_equal(logits, got["logits"][rows])
    out["branch_logits"] = got["logits"][::LOGIT_STEP].copy()
    out["branch_point_predict"] = np.concatenate(ev["point_predict"]).astype(np.uint8)
    out["branch_point_labels"] = np.concatenate(ev["point_labels"]).astype(np.uint8)
    out["branch_margin"] = margin
    sd = model.state_dict()
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["param_crc"] = np.array([zlib.crc32(v.numpy().tobytes()) for v in sd.values()], dtype=np.int64)
    bott = cls(make_model_cfg("SPVCNN", BLOCK="Bottleneck", **CFG), 20).state_dict()
    out["bottleneck_state_keys"] = np.array(list(bott.keys()))
    out["bottleneck_state_shapes"] = np.array([",".join(map(str, v.shape)) for v in bott.values()])
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB; voxels", len(coords), "points", sum(n_pts), "most rows per voxel at strides 1 / 4 / 16",
          most, "loss(train/eval)", out["train_loss"], out["eval_loss"], "margin <= %g: %.3f %%" % (MARGIN, 100 * left_out))


if __name__ == "__main__":
    main()
