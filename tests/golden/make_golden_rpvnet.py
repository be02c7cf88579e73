"""Golden vectors of the RPVNet segmentor (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_rpvnet.py        ->  tests/golden/model_rpvnet.npz  (data only)

Same arrangement as make_golden_spvcnn.py: the REAL reference's Python (pcseg/model/segmentor/fusion/rpvnet/rpvnet.py, its torchsparse
v1.4.0, its Losses, the dataset's get_range_image and collate_batch) runs on the CPU through the import environment of _ref_env.py;
no reference code in this file.

  batch   make_golden_spvcnn.py's two-scan batch (seeds 21 / 22, POINTS points a scan, the reference's voxelisation lines through its
          library calls) plus a ring column (taseg_amd.data.synthetic.ring_column); `range_image` / `range_pxpy` from the reference's
          get_range_image on every sample's kept rows (np.random.seed(CUT_SEEDS[i]) before each) and its collate_batch.
  model   RPVNet, make_model_cfg("RPVNet", in_dim=4, cr=0.5, num_layer=[1] * 8, IF_DIST=True, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0),
          every Dropout2d.p of the instance set to 0, fill_parameters(PARAM_SEED); BatchNorm in training mode ("train") and on running
          statistics ("eval", training branch), and the evaluation branch.  For BLOCK="Bottleneck": state_dict keys and shapes only.
          (IF_DIST=False cannot run in the reference: its point transforms then hold a sparse-tensor BatchNorm, rpvnet.py:574.)

Stand-ins, ours: `range_utils.nn.functional` (the reference's CUDA-only extension) - map_count as a bincount over (batch, y, x),
denselize as index_add of feat / count under autograd, the extension's documented contract (mean per pixel, zeros elsewhere; rows below
0 are dropped as its kernels do, rows above the map raise); `cv2.resize` asserts equal sizes and returns the image; SyncBatchNorm on the
CPU goes through _ref_env.setup_pcseg_mm's patch (one process: the local statistics).

Gradients of tensors above 8192 elements are stored as `strided_sample`s; `*_gradnorms` covers every parameter whole.  `--search`
prints the first parameter seed that passes the margin rule below.
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import _ref_env  # noqa: E402
from taseg_amd.data.range import draw_range_cut  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, ring_column, strided_sample, synth_scan  # noqa: E402

torch.set_num_threads(1)
VOXEL = 0.05
SEEDS, CUT_SEEDS = (21, 22), (3, 4)
POINTS = 8000                 # as make_golden_spvcnn.py: everything the 16 x 360 grid of rays yields
HW = (64, 2048)
LOGIT_STEP = 12               # rows of the per-voxel logits that are stored (the fixture stays under 1 MiB)
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, IF_DIST=True, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
KEEP = ["stem.0.kernel", "stage4.1.net.0.kernel", "up4.1.0.net.3.kernel", "classifier.0.weight", "classifier.0.bias",
        "point_transforms.0.0.weight", "point_transforms.0.1.weight", "point_transforms.1.0.weight", "point_transforms.1.1.bias",
        "point_transforms.3.0.weight", "point_transforms.3.1.bias", "range_branch.stem.0.conv1.weight",
        "range_branch.stem.2.bn2.weight", "range_branch.stage1.conv2.weight", "range_branch.mid_stage.conv2.weight",
        "range_branch.up2.conv1.weight", "range_branch.up4.conv1.weight", "range_branch.up4.bn1.bias"]
# (no bias of a Linear or Conv2d that sits in front of a training-mode BatchNorm: its exact gradient is zero)
FULL_BELOW = 8192
MARGIN = 2e-3
BACKGROUND = np.array([-10, -10, 0, 0, 0], dtype=np.float32)
# parameter seed: the first of 0, 1, 2 ... at which the evaluation branch leaves at most 1 % of the points with a top-2 logit margin
# <= MARGIN (`--search` finds it; main() asserts that this one passes)
PARAM_SEED = 0


def same_size_resize(img, size, interpolation=None):
    assert tuple(size) == (img.shape[1], img.shape[0]), (size, img.shape)
    return img


def map_count(pxpy, max_bs, h, w):
    flat = (pxpy[:, 0].long() * h + pxpy[:, 2].long()) * w + pxpy[:, 1].long()
    assert int(pxpy[:, 1].max()) < w and int(pxpy[:, 2].max()) < h and int(pxpy[:, 0].max()) < max_bs
    keep = (pxpy[:, 1] >= 0) & (pxpy[:, 2] >= 0)
    return torch.bincount(flat[keep], minlength=max_bs * h * w).view(max_bs, h, w).int()


def denselize(feat, count_map, pxpy):
    b, h, w = count_map.shape
    keep = (pxpy[:, 1] >= 0) & (pxpy[:, 2] >= 0)
    flat = ((pxpy[:, 0].long() * h + pxpy[:, 2].long()) * w + pxpy[:, 1].long())[keep]
    rows = feat[keep] / count_map.reshape(-1)[flat].to(feat.dtype).unsqueeze(1)
    out = feat.new_zeros((b * h * w, feat.shape[1])).index_add(0, flat, rows)
    return out.view(b, h, w, feat.shape[1]).permute(0, 3, 1, 2).contiguous()


def setup():
    desc = _ref_env.setup_torchsparse()
    _ref_env.setup_pcseg()
    _ref_env.setup_pcseg_mm()                                   # (its SyncBatchNorm patch for the CPU)
    import cv2
    cv2.resize, cv2.INTER_LINEAR = same_size_resize, 1
    fn = types.ModuleType("range_utils.nn.functional")
    fn.map_count, fn.denselize = map_count, denselize
    for name in ("range_utils", "range_utils.nn"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["range_utils.nn.functional"] = fn
    sys.modules["range_utils"].nn, sys.modules["range_utils.nn"].functional = sys.modules["range_utils.nn"], fn
    torch.Tensor([1]).cuda()                                    # (rpvnet.py:88 calls .cuda(): _ref_env made it the identity)
    base = os.path.join(_ref_env.REF, "pcseg", "model", "segmentor", "fusion")
    _ref_env._pkg("pcseg.model.segmentor.fusion", base)
    _ref_env._pkg("pcseg.model.segmentor.fusion.rpvnet", os.path.join(base, "rpvnet"))
    from pcseg.model.segmentor.fusion.rpvnet.rpvnet import RPVNet
    from pcseg.data.dataset.semantickitti.semantickitti_fusion import SemkittiFusionDataset
    return desc, RPVNet, SemkittiFusionDataset


def make_batch(ds):
    from torchsparse import SparseTensor
    from torchsparse.utils.quantize import sparse_quantize
    samples, cuts = [], []
    for s, cs in zip(SEEDS, CUT_SEEDS):
        pts, lab = synth_scan(s, n_points=POINTS, n_beams=16, n_az=360)
        pts = np.concatenate([pts[:, :4], ring_column(pts, 16, HW[0])[:, None]], 1).astype(np.float32)
        pc_ = np.round(pts[:, :3] / VOXEL).astype(np.int32)                 # semantickitti_fusion.py:166-183 through the library calls
        pc_ -= pc_.min(0, keepdims=1)
        _, inds, inverse = sparse_quantize(pc_, return_index=True, return_inverse=True)
        lidar = SparseTensor(pts[inds], pc_[inds])
        np.random.seed(cs)
        range_image, range_pxpy = ds.get_range_image(None, lidar.F)
        cuts.append(draw_range_cut(np.random.RandomState(cs)))
        samples.append({"name": "scan%d" % s, "lidar": lidar, "targets": SparseTensor(lab[inds], pc_[inds]),
                        "targets_mapped": SparseTensor(lab, pc_), "inverse_map": SparseTensor(inverse, pc_),
                        "num_points": np.array([len(pts)]), "range_image": range_image, "range_pxpy": range_pxpy})
    batch = ds.collate_batch(samples)
    batch["lidar"].F, batch["lidar"].C = batch["lidar"].F.float(), batch["lidar"].C.int()
    batch["offset"] = torch.tensor([0])
    return batch, np.array(cuts)


def clone(batch):
    from torchsparse import SparseTensor
    out = {}
    for k, v in batch.items():
        out[k] = SparseTensor(v.F.clone(), v.C.clone()) if isinstance(v, SparseTensor) else (v.clone() if torch.is_tensor(v) else v)
    return out


def build(cls, seed, **over):
    model = cls(make_model_cfg("RPVNet", **{**CFG, **over}), 20)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return fill_parameters(model, seed=seed)


def run(cls, batch, bn_training, seed):
    model = build(cls, seed)
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
    model = build(cls, seed).eval()
    with torch.no_grad():
        ev = model(clone(batch))
    logits = np.concatenate(ev["point_predict_logits"])
    top2 = np.sort(logits, axis=1)[:, -2:]
    return ev, logits, (top2[:, 1] - top2[:, 0]).astype(np.float32)


def main(fname="model_rpvnet.npz"):
    desc, cls, ds = setup()
    batch, cuts = make_batch(ds)
    if "--search" in sys.argv:
        for seed in range(80):
            left_out = float((branch(cls, batch, seed)[2] <= MARGIN).mean())
            print("seed", seed, "margin <= %g: %.3f %%" % (MARGIN, 100 * left_out), flush=True)
            if left_out <= 0.01:
                return
        raise SystemExit("no seed passes")
    coords = batch["lidar"].C.numpy()
    image = batch["range_image"].numpy()
    rows = image.transpose(0, 2, 3, 1).reshape(-1, 5)
    at = np.flatnonzero((rows != BACKGROUND).any(1))
    out = {"backend": np.array(desc), "cfg": np.array(repr(sorted(CFG.items()))), "full_below": np.array(FULL_BELOW),
           "margin": np.array(MARGIN), "param_seed": np.array(PARAM_SEED), "logit_step": np.array(LOGIT_STEP),
           "coords": coords.copy(), "feats": batch["lidar"].F.numpy().copy(), "labels": batch["targets"].F.numpy().astype(np.uint8),
           "inverse_map": batch["inverse_map"].F.numpy().astype(np.int32),
           "point_batch": batch["inverse_map"].C[:, -1].numpy().astype(np.uint8),
           "point_labels": batch["targets_mapped"].F.numpy().astype(np.uint8),
           "num_points": batch["num_points"].numpy().reshape(-1).astype(np.int64), "name": np.array(batch["name"]),
           "cuts": cuts, "hw": np.array(HW), "range_pxpy": batch["range_pxpy"].numpy().copy(),
           "image_at": at.astype(np.int32), "image_values": rows[at].copy()}
    assert batch["range_pxpy"].dtype == torch.float32 and batch["range_image"].shape == (len(SEEDS), 5) + HW
    for bn_training in (True, False):
        out.update(run(cls, batch, bn_training, PARAM_SEED))
    ev, logits, margin = branch(cls, batch, PARAM_SEED)
    n_pts = out["num_points"].tolist()
    assert [len(p) for p in ev["point_predict"]] == n_pts and ev["name"] == batch["name"]
    left_out = float((margin <= MARGIN).mean())
    assert left_out <= 0.01, left_out
    model = build(cls, PARAM_SEED).eval()
    got = {}
    model.classifier.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach().numpy()))
    with torch.no_grad():
        model(clone(batch))
    start = np.concatenate([[0], np.cumsum([(coords[:, 3] == b).sum() for b in range(len(SEEDS))])])
    at_rows = out["inverse_map"].astype(np.int64) + start[out["point_batch"]]
    assert np.array_equal(logits, got["logits"][at_rows])
    out["branch_logits"] = got["logits"][::LOGIT_STEP].copy()
    out["branch_point_predict"] = np.concatenate(ev["point_predict"]).astype(np.uint8)
    out["branch_point_labels"] = np.concatenate(ev["point_labels"]).astype(np.uint8)
    out["branch_margin"] = margin
    sd = model.state_dict()
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["param_crc"] = np.array([zlib.crc32(v.numpy().tobytes()) for v in sd.values()], dtype=np.int64)
    bott = build(cls, 0, BLOCK="Bottleneck").state_dict()
    out["bottleneck_state_keys"] = np.array(list(bott.keys()))
    out["bottleneck_state_shapes"] = np.array([",".join(map(str, v.shape)) for v in bott.values()])
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB; voxels", len(coords), "points", sum(n_pts), "pixels set", len(at), "loss(train/eval)",
          out["train_loss"], out["eval_loss"], "margin <= %g: %.3f %%" % (MARGIN, 100 * left_out))


if __name__ == "__main__":
    main()
