"""Golden vectors of the Cylinder_TS segmentor (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_cylinder.py        ->  tests/golden/model_cylinder.npz  (data only)

Same arrangement as make_golden.py: the REAL reference's Python (pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py, its
torchsparse v1.4.0, its Losses) runs on the CPU through the import environment of _ref_env.py; no reference code in this file.

  batch   two seeded synthetic scans (taseg_amd.data.synthetic.synth_scan) put through the reference's OWN cylinder data stage:
          SemkittiCylinderDataset.get_single_sample (semantickitti_cylinder.py:104-174, evaluation form: no augmentation) and
          collate_batch (:176-219), on a grid of 96 x 80 x 16 cells - divisible by the network's total stride of 16 x 16 x 4.
  model   Cylinder_TS, IF_DIST False, INIT_SIZE 16, IN_FEATURE_DIM 9, LABEL_SMOOTHING 0 (the recipe's), fill_parameters(PARAM_SEED);
          BatchNorm in training mode ("train") and on running statistics ("eval", training branch), and the evaluation branch.

The one third-party piece the reference imports and this image lacks is `torch_scatter`; `scatter_max` below stands in for it and
is described there.  Gradients of tensors above 8192 elements are stored as `strided_sample`s (the fixture stays under 1 MiB);
`*_gradnorms` covers every parameter whole.
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
GRID, SPACE_MAX, SPACE_MIN = [96, 80, 16], [50, 180, 2], [0, -180, -4]
CFG = dict(in_dim=9, INIT_SIZE=16, LABEL_SMOOTHING=0.0, POINT_REFINEMENT=True, DROPOUT_P=0.0)
SEEDS, POINTS = (33, 34), 1000          # (seeds 31 / 32 leave one tie on running statistics: see scatter_max)
KEEP = ["downCntx.conv1.kernel", "logits.kernel", "logits.bias", "ReconNet.conv1_2.kernel", "upBlock3.up_subm.kernel",
        "point_logits.weight", "PPmodel.1.weight"]
FULL_BELOW = 8192
MARGIN = 2e-3
# parameter seed: the first of 0 .. 79 at which the evaluation branch leaves at most 1 % of the points with a top-2 logit margin
# <= MARGIN (seed 3, the other model fixtures': 2 - 3 %; logits of these parameters have a standard deviation of ~0.1) and no voxel
# ties in a channel (scatter_max below); main() asserts both
PARAM_SEED = 55
TIES = {"checked": 0}


def scatter_max(src, index, dim=0):
    """Stand-in for the ONE function of `torch_scatter` the reference's Cylinder_TS calls (seg_utils.py:391:
    `torch_scatter.scatter_max(z.F, idx_query, dim=0)[0]`; the package is not installed here and is not part of the reference's
    tree).  Same interface as far as it is used: a pair whose element 0 is out[v, ch] = max of src[i, ch] over the rows with
    index[i] == v, through torch's `scatter_reduce_('amax', include_self=False)`; element 1 (the arg-max) is never read and is
    None.  Values are those of torch_scatter (a maximum rounds nothing).  The GRADIENTS differ where two rows of a voxel tie in a
    channel - torch's amax splits the gradient between them, torch_scatter gives it to one - so every call asserts that no voxel
    with more than one row has such a tie: on this fixture the two agree."""
    assert dim == 0 and src.dim() == 2 and index.dim() == 1
    m = int(index.max()) + 1
    where = index.unsqueeze(1).expand_as(src)
    out = src.new_zeros((m, src.shape[1])).scatter_reduce_(0, where, src, "amax", include_self=False)
    with torch.no_grad():
        hits = torch.zeros((m, src.shape[1]), dtype=torch.int64).scatter_add_(0, where, (src == out[index]).long())
        assert int(hits.min()) == 1 and int(hits.max()) == 1, "two rows of a voxel tie in a channel: amax would split the gradient"
        TIES["checked"] += int((torch.bincount(index, minlength=m) > 1).sum())
    return out, None


def setup():
    desc = _ref_env.setup_torchsparse()
    _ref_env.setup_pcseg()
    sys.modules["torch_scatter"].scatter_max = scatter_max
    for alias, typ in (("int", int), ("bool", bool), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)                              # aliases numpy >= 1.24 dropped (semantickitti_cylinder.py:153)
    base = os.path.join(_ref_env.REF, "pcseg", "model", "segmentor", "voxel", "cylinder3d")
    _ref_env._pkg("pcseg.model.segmentor.voxel.cylinder3d", base)
    from pcseg.model.segmentor.voxel.cylinder3d.cylinder_ts import Cylinder_TS
    from pcseg.data.dataset.semantickitti.semantickitti_cylinder import SemkittiCylinderDataset
    return desc, Cylinder_TS, SemkittiCylinderDataset


def make_batch(dataset_cls):
    ds = object.__new__(dataset_cls)
    ds.training, ds.if_tta = False, False
    ds.class_names = ["c%d" % i for i in range(20)]
    ds.cylinder_space_max, ds.cylinder_space_min, ds.grid_size = np.array(SPACE_MAX), np.array(SPACE_MIN), np.array(GRID)
    ds.point_cloud_dataset = []
    for seed in SEEDS:
        pts, lab = synth_scan(seed, n_points=POINTS, n_beams=16, n_az=360)
        ds.point_cloud_dataset.append({"xyzret": pts.copy(), "labels": lab.astype(np.int64), "path": "scan%d" % seed})
    return dataset_cls.collate_batch([ds.get_single_sample(i) for i in range(len(SEEDS))])


def clone(batch):
    return {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in batch.items()}


def run(cls, cfg, batch, bn_training):
    model = fill_parameters(cls(cfg, 20), seed=PARAM_SEED)
    model.train()
    if not bn_training:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    got = {}
    hooks = [model.logits.register_forward_hook(lambda m, i, o: got.update(logits=o.F.detach(), coords=o.C.detach())),
             model.point_logits.register_forward_hook(lambda m, i, o: got.__setitem__("point_logits", o.detach()))]
    ret, tb, _ = model(clone(batch))
    for h in hooks:
        h.remove()
    model.zero_grad()
    ret["loss"].backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    tag = "train" if bn_training else "eval"
    res = {f"{tag}_logits": got["logits"].numpy(), f"{tag}_point_logits": got["point_logits"].numpy(),
           f"{tag}_loss": np.array(tb["loss"]), f"{tag}_loss_point": np.array(tb["loss_point"]),
           f"{tag}_loss_total": np.array(ret["loss"].item()),
           f"{tag}_gradnorms": np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])}
    for k in KEEP:
        g = grads[k]
        res[f"{tag}_grad/{k}"] = (g if g.numel() <= FULL_BELOW else strided_sample(g)).numpy().copy()
    return model, got["coords"].numpy(), res


def main(fname="model_cylinder.npz"):
    desc, cls, dataset_cls = setup()
    cfg = make_model_cfg("Cylinder_TS", **CFG)
    batch = make_batch(dataset_cls)
    out = {"backend": np.array(desc), "grid": np.array(GRID), "cfg": np.array(repr(sorted(CFG.items()))),
           "full_below": np.array(FULL_BELOW), "margin": np.array(MARGIN), "param_seed": np.array(PARAM_SEED)}
    for k, v in batch.items():
        out["batch_" + k] = np.array(v) if k == "name" else v.numpy()
    out["batch_point_coord"] = out["batch_point_coord"].astype(np.int32)
    out["batch_voxel_coord"] = out["batch_voxel_coord"].astype(np.int32)
    del out["batch_voxel_feature"]                               # (never read by the model)
    for bn_training in (True, False):
        model, coords, res = run(cls, cfg, batch, bn_training)
        out.update(res)
    out["voxel_order"] = coords.astype(np.int32)                 # the model's voxel rows (ascending hash)
    vc = out["batch_voxel_coord"]
    assert coords.shape == vc.shape and sorted(map(tuple, coords.tolist())) == sorted(map(tuple, vc.tolist()))
    moved = int((coords != vc).any(1).sum())
    assert moved > len(vc) // 2, "voxel_coord's order must differ from the model's: the reproduced indexing (:539-542) is untested"
    assert TIES["checked"] > 0, "no voxel with two points: the maximum is untested"
    # evaluation branch (model.eval()): running statistics, per-point predictions
    model.eval()
    with torch.no_grad():
        ev = model(clone(batch))
    n_pts = batch["num_points"].tolist()
    assert [len(p) for p in ev["point_predict"]] == n_pts and ev["name"] == batch["name"]
    logits = np.concatenate(ev["point_predict_logits"])
    out["branch_point_predict"] = np.concatenate(ev["point_predict"]).astype(np.int64)
    out["branch_point_labels"] = np.concatenate(ev["point_labels"]).astype(np.int64)
    # the branch's logits are rows of the voxel logits on running statistics: stored as the row of every point (a copy of "eval_logits"
    # rows would double the fixture); asserted bit for bit here
    pc = out["batch_point_coord"]
    row_of = {tuple(c): i for i, c in enumerate(coords.tolist())}
    rows = np.array([row_of[tuple(c)] for c in pc.tolist()], dtype=np.int32)
    assert np.array_equal(logits, out["eval_logits"][rows])
    out["branch_point_row"] = rows
    top2 = np.sort(logits, axis=1)[:, -2:]
    out["branch_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    left_out = float((out["branch_margin"] <= MARGIN).mean())
    assert left_out <= 0.01, left_out
    sd = model.state_dict()
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["param_crc"] = np.array([zlib.crc32(v.numpy().tobytes()) for v in fill_parameters(cls(cfg, 20), seed=PARAM_SEED).state_dict().values()],
                                dtype=np.int64)
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB; points", len(pc), "voxels", len(vc), "rows moved", moved, "voxels with > 1 point checked for ties",
          TIES["checked"], "loss(train/eval)", out["train_loss"], out["eval_loss"], "loss_point", out["train_loss_point"],
          out["eval_loss_point"], "margin <= %g: %.3f %%" % (MARGIN, 100 * left_out))


if __name__ == "__main__":
    main()
