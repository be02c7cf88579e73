"""Golden vectors of SalsaNext (build container only; reads /root/reference, inert on the GPU box).

    python tests/golden/make_golden_salsanext.py        ->  tests/golden/model_salsanext.npz  (data only)

The REAL reference's `SalsaNext` (pcseg/model/segmentor/range/salsanext/model/semantic/salsanext.py) with its own losses
(range/utils.py) runs on the CPU in float32 through the import environment of make_golden_range_view.py (its stand-ins, plus `.cuda()`
as the identity on tensors and modules); no reference code in this file.  Batch: B = 2 at 32 x 64 - the smallest size with two pixels
at the 1/16 level - projected from two synthetic clouds by tests/range_view_ref.py's restatement.  Parameters: `fill_parameters(seed)`.
The Dropout2d modules are in eval mode (on both sides: their draws are not part of the comparison).

Stored, for LOSS 'wce' and 'dice' (IF_LS_LOSS and IF_BD_LOSS on, TOP_K_PERCENT_PIXELS 1.0; plus the 'wce' loss at 0.5) and BatchNorm in
training mode (`train`) and on running statistics (`eval`): the loss, every parameter's gradient norm, the gradients of the parameters
with at most `full_below` elements in full and `strided_sample`s of a few large ones; the logits once per BatchNorm mode (they do not
depend on the loss), every `logit_step`-th pixel; the evaluation branch's arg-max and top-2 margin; the state_dict keys and shapes; the 'wce' class-weight table as the reference
computes it (fill_parameters overwrites `WCE.weight` on both sides, so the model runs do not check it)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_range_view as MG  # noqa: E402
import range_view_ref as R  # noqa: E402
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg, strided_sample  # noqa: E402

torch.set_num_threads(1)
HW, SEEDS, POINTS, PARAM_SEED, LOGIT_STEP, FULL_BELOW = (32, 64), (51, 52), (1800, 1500), 11, 3, 64
SAMPLED = ("downCntx.conv2.weight", "resBlock1.conv4.weight", "resBlock3.conv5.weight", "resBlock5.conv5.weight",
           "upBlock1.conv1.weight", "upBlock3.conv4.weight", "upBlock4.conv2.weight", "logits.weight")


def cfg(loss, top_k=1.0):
    return make_model_cfg("SalsaNext", LOSS=loss, IF_LS_LOSS=True, IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=top_k)


def inputs():
    clouds = [R.synth_cloud(s, n, far=30.0) for s, n in zip(SEEDS, POINTS)]
    labels = np.concatenate([np.random.RandomState(s + 3).randint(0, 20, n) for s, n in zip(SEEDS, POINTS)]).astype(np.int32)
    batch = np.repeat(np.arange(2), POINTS)
    got = R.project32(np.concatenate(clouds), batch, [0, POINTS[0]], 2, HW[0], HW[1], labels=labels)
    return got["scan_rv"], got["label_rv"]


def step(model, scan, label, bn_training):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d) or (not bn_training and isinstance(m, torch.nn.modules.batchnorm._BatchNorm)):
            m.eval()
    got = {}
    hook = model.logits.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach()))
    ret, tb, disp = model({"scan_rv": torch.from_numpy(scan), "label_rv": torch.from_numpy(label)})
    hook.remove()
    model.zero_grad()
    ret["loss"].backward()
    return float(ret["loss"].detach()), got["logits"], {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def main(fname="model_salsanext.npz"):
    MG.setup()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from pcseg.model.segmentor.range.salsanext.model.semantic.salsanext import SalsaNext
    scan, label = inputs()
    from pcseg.model.segmentor.range.utils import ClassWeightSemikitti
    out = {"class_weight": np.array(ClassWeightSemikitti.get_weight(), dtype=np.float64),"scan_rv": scan, "label_rv": label.astype(np.int8), "hw": np.array(HW), "param_seed": np.array(PARAM_SEED),
           "logit_step": np.array(LOGIT_STEP), "full_below": np.array(FULL_BELOW), "sampled": np.array(SAMPLED)}
    for loss in ("wce", "dice"):
        model = fill_parameters(SalsaNext(cfg(loss), 20), seed=PARAM_SEED)
        sd = model.state_dict()
        out[f"{loss}_state_keys"] = np.array(list(sd.keys()))
        out[f"{loss}_state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        for tag, bn_training in (("train", True), ("eval", False)):
            model = fill_parameters(SalsaNext(cfg(loss), 20), seed=PARAM_SEED)
            value, logits, grads = step(model, scan, label, bn_training)
            rows = logits.permute(0, 2, 3, 1).reshape(-1, 20)[::LOGIT_STEP].numpy()
            if loss == "wce":
                out[f"{tag}_logits"] = rows
            else:
                assert np.array_equal(out[f"{tag}_logits"], rows)
            out[f"{loss}_{tag}_loss"] = np.array(value)
            out[f"{loss}_{tag}_gradnorms"] = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
            for n, gr in grads.items():
                if gr.numel() <= FULL_BELOW:
                    out[f"{loss}_{tag}_grad/{n}"] = gr.numpy()
                elif n in SAMPLED:
                    out[f"{loss}_{tag}_grad/{n}"] = strided_sample(gr).numpy()
                # (a sample must carry signal: the stride of a dilated 3 x 3 weight at the 2 x 4 level can hit taps that only see padding)
                assert f"{loss}_{tag}_grad/{n}" not in out or np.linalg.norm(out[f"{loss}_{tag}_grad/{n}"]) > 0, n
            print(loss, tag, "loss %.6f" % value, "logits up to %.2f" % float(logits.abs().max()))
    model = fill_parameters(SalsaNext(cfg("wce", 0.5), 20), seed=PARAM_SEED)
    out["wce_topk_train_loss"] = np.array(step(model, scan, label, True)[0])
    model = fill_parameters(SalsaNext(cfg("dice"), 20), seed=PARAM_SEED).eval()
    with torch.no_grad():
        res = model({"scan_rv": torch.from_numpy(scan), "label_rv": torch.from_numpy(label)})
    assert set(res) == {"point_predict", "point_labels"} and res["point_labels"].shape == (2,) + HW
    top = res["point_predict"].topk(2, dim=1).values
    out["branch_argmax"] = res["point_predict"].argmax(1).numpy().astype(np.uint8)
    out["branch_margin"] = (top[:, 0] - top[:, 1]).numpy()
    rows = res["point_predict"].permute(0, 2, 3, 1).reshape(-1, 20)[::LOGIT_STEP].numpy()
    assert np.abs(rows - out["eval_logits"]).max() < 1e-5                      # the evaluation branch is the BatchNorm-eval forward
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
