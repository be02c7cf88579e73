"""Golden vectors of FIDNet (needs the reference checkout that tests/golden/_ref_env.py names; inert without it).

    python tests/golden/make_golden_fidnet.py        ->  tests/golden/model_fidnet.npz  (data only)

The REAL reference's `FIDNet` (pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py) with its own losses (range/utils.py) runs
on the CPU in float32 through the import environment of make_golden_range_view.py (its stand-ins, plus `.cuda()` as the identity on
tensors and modules); no reference code in this file.  Batch: B = 2 at 16 x 64 - the levels are 8 x 32, 4 x 16 and 2 x 8 - projected
from two synthetic clouds by tests/range_view_ref.py's restatement.  Parameters: `fill_parameters(seed)`.

Stored, for LOSS 'wce' and 'dice' (IF_BN, IF_LS_LOSS and IF_BD_LOSS on, TOP_K_PERCENT_PIXELS 1.0; plus the 'wce' loss at 0.5) and
BatchNorm in training mode (`train`) and on running statistics (`eval`): the loss, every parameter's gradient norm, the gradients of
the parameters with at most `full_below` elements in full (but `backend.conv1.bias` in training mode: see store_runs) and `strided_sample`s of the `sampled` ones; the logits once per BatchNorm
mode (they do not depend on the loss), every `logit_step`-th pixel; the distance of each of those float32 results from a float64
evaluation of the reference itself (`*_dist64`: what the tests' bars may fall back on) and from the reference on a channels-last input
(`*_dist32`: a reported figure, no bar uses it); the evaluation branch's arg-max and top-2 margin; the state_dict
keys and shapes for both LOSS settings with IF_BN on and off (`keys/<loss>_bn<0|1>`).  make_golden_cenet.py runs CENet through the
same functions."""
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
HW, SEEDS, POINTS, PARAM_SEED, LOGIT_STEP, FULL_BELOW = (16, 64), (71, 72), (900, 800), 13, 2, 64
SAMPLED = ("backend.conv2.weight", "backend.bn.weight", "backend.conv4.weight", "backend.bn_2.bias", "backend.layer1.0.conv1.weight",
           "backend.layer1.2.bn2.weight", "backend.layer2.0.downsample.0.weight", "backend.layer2.0.downsample.1.bias",
           "backend.layer2.3.conv2.weight", "backend.layer3.0.conv1.weight", "backend.layer3.5.bn1.bias", "backend.layer4.0.bn2.weight",
           "backend.layer4.2.conv2.weight", "semantic_head.conv_1.weight", "semantic_head.bn1.weight", "semantic_head.conv_2.weight",
           "semantic_head.semantic_output.weight")


# the biases of the convolutions in front of a training-mode BatchNorm: their gradient is zero in exact arithmetic
ZERO_IN_TRAINING = ("backend.conv1.bias", "backend.conv2.bias", "backend.conv3.bias", "backend.conv4.bias", "semantic_head.conv_1.bias",
                    "semantic_head.conv_2.bias")


def cfg(name, loss="dice", top_k=1.0, if_bn=True, **kw):
    return make_model_cfg(name, IF_BN=if_bn, IF_INTENSITY=True, IF_RANGE=True, WITH_NORM=False, LOSS=loss, IF_LS_LOSS=True,
                          IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=top_k, **kw)


def inputs():
    clouds = [R.synth_cloud(s, n, far=30.0) for s, n in zip(SEEDS, POINTS)]
    labels = np.concatenate([np.random.RandomState(s + 3).randint(0, 20, n) for s, n in zip(SEEDS, POINTS)]).astype(np.int32)
    batch = np.repeat(np.arange(2), POINTS)
    got = R.project32(np.concatenate(clouds), batch, [0, POINTS[0]], 2, HW[0], HW[1], labels=labels)
    return got["scan_rv"], got["label_rv"]


def step(model, head, scan, label, bn_training, memory_format=torch.contiguous_format):
    model.train()
    for m in model.modules():
        if not bn_training and isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    got = {}
    hook = head(model).register_forward_hook(lambda m, i, o: got.__setitem__("logits", o.detach()))
    dtype = next(model.parameters()).dtype
    ret, tb, disp = model({"scan_rv": torch.from_numpy(scan).to(dtype).contiguous(memory_format=memory_format),
                           "label_rv": torch.from_numpy(label)})
    hook.remove()
    model.zero_grad()
    ret["loss"].backward()
    return float(ret["loss"].detach()), got["logits"], {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def store_keys(out, tag, model):
    sd = model.state_dict()
    out[f"keys/{tag}"] = np.array(list(sd.keys()))
    out[f"shapes/{tag}"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])


def store_runs(out, variants, build, head, scan, label, sampled, zero_in_training=()):
    """variants: (name, build arguments) - one training-mode and one running-statistics step each; the logits are stored once.
    zero_in_training: parameters whose training-mode gradient is zero in exact arithmetic (a bias in front of a training-mode BatchNorm:
    what float32 leaves there is rounding noise: not stored, and left out of the gradient norms' comparison - `zero_in_training`)"""
    for name, kw in variants:
        for tag, bn_training in (("train", True), ("eval", False)):
            model = fill_parameters(build(**kw), seed=PARAM_SEED)
            value, logits, grads = step(model, head, scan, label, bn_training)
            rows = logits.permute(0, 2, 3, 1).reshape(-1, 20)[::LOGIT_STEP].numpy()
            if f"{tag}_logits" not in out:
                out[f"{tag}_logits"] = rows
            else:
                assert np.array_equal(out[f"{tag}_logits"], rows)
            out[f"{name}_{tag}_loss"] = np.array(value)
            out[f"{name}_{tag}_gradnorms"] = np.array([float(grads[n].norm()) for n, _ in model.named_parameters()])
            for n, gr in grads.items():
                if bn_training and n in zero_in_training:
                    assert float(gr.norm()) < 1e-5, (n, float(gr.norm()))
                elif gr.numel() <= FULL_BELOW:
                    out[f"{name}_{tag}_grad/{n}"] = gr.numpy()
                elif n in sampled:
                    out[f"{name}_{tag}_grad/{n}"] = strided_sample(gr).numpy()
                assert f"{name}_{tag}_grad/{n}" not in out or np.linalg.norm(out[f"{name}_{tag}_grad/{n}"]) > 0, n
            # the reference's own distance from a float64 evaluation of itself (the same modules in double): what a float32 run of this
            # network can be held to - `dist64/<parameter>` = |g32 - g64| / |g64| over the stored elements, and the logits' and loss's
            # (stand-in for that run alone: `Tensor.float()` widens to double, so the reference's Lovasz term, which casts its masks
            # with `.float()`, stays in the model's precision)
            narrow, torch.Tensor.float = torch.Tensor.float, lambda self, *a, **k: self.double()
            try:
                value64, logits64, grads64 = step(fill_parameters(build(**kw), seed=PARAM_SEED).double(), head, scan, label, bn_training)
            finally:
                torch.Tensor.float = narrow
            out[f"{name}_{tag}_loss_dist64"] = np.array(abs(value - value64))
            out[f"{tag}_logits_dist64"] = np.array(float((logits.double() - logits64).abs().max()))
            # ... and from a second float32 evaluation of itself: the same modules on a channels-last input, where ATen's convolutions
            # add in another order (`dist32/<parameter>`).  An element that sits at a LeakyReLU's kink takes the other slope there, which
            # moves a gradient by a step and not by a rounding: one float32 sample need not show it, two may
            _, _, grads32 = step(fill_parameters(build(**kw), seed=PARAM_SEED), head, scan, label, bn_training, torch.channels_last)
            for n, gr in grads64.items():
                if f"{name}_{tag}_grad/{n}" in out:
                    pick = (lambda t: t) if gr.numel() <= FULL_BELOW else strided_sample
                    a, b, c = pick(grads[n]).double().reshape(-1), pick(gr).reshape(-1), pick(grads32[n]).double().reshape(-1)
                    out[f"{name}_{tag}_dist64/{n}"] = np.array(float((a - b).norm() / b.norm()))
                    out[f"{name}_{tag}_dist32/{n}"] = np.array(float((a - c).norm() / b.norm()))
            worst = max((float(v), k) for k, v in out.items() if k.startswith(f"{name}_{tag}_dist64/"))
            again = max((float(v), k) for k, v in out.items() if k.startswith(f"{name}_{tag}_dist32/"))
            print(name, tag, "float32 reference vs its float64 evaluation: logits %.2e, loss %.2e, worst stored gradient %.2e (%s); vs "
                  "itself on a channels-last input: %.2e (%s)" % (float(out[f"{tag}_logits_dist64"]), abs(value - value64), worst[0],
                                                                  worst[1].split("/", 1)[1], again[0], again[1].split("/", 1)[1]))
            print(name, tag, "loss %.6f" % value, "logits up to %.2f" % float(logits.abs().max()))


def store_branch(out, model, scan, label):
    model.eval()
    with torch.no_grad():
        res = model({"scan_rv": torch.from_numpy(scan), "label_rv": torch.from_numpy(label)})
    assert set(res) == {"point_predict", "point_labels"} and res["point_labels"].shape == (2,) + HW
    top = res["point_predict"].topk(2, dim=1).values
    out["branch_argmax"] = res["point_predict"].argmax(1).numpy().astype(np.uint8)
    out["branch_margin"] = (top[:, 0] - top[:, 1]).numpy()
    rows = res["point_predict"].permute(0, 2, 3, 1).reshape(-1, 20)[::LOGIT_STEP].numpy()
    assert np.abs(rows - out["eval_logits"]).max() < 1e-5                      # the evaluation branch is the BatchNorm-eval forward


def header(scan, label, sampled, zero_in_training=()):
    return {"zero_in_training": np.array(zero_in_training, dtype="U64"), "scan_rv": scan, "label_rv": label.astype(np.int8), "hw": np.array(HW), "param_seed": np.array(PARAM_SEED),
            "logit_step": np.array(LOGIT_STEP), "full_below": np.array(FULL_BELOW), "sampled": np.array(sampled)}


def save(out, fname):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(fname, size // 1024, "KiB;", len(out), "arrays")


def environment():
    MG.setup()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self


def main(fname="model_fidnet.npz"):
    environment()
    from pcseg.model.segmentor.range.fidnet.model.semantic.fidnet import FIDNet
    scan, label = inputs()
    out = header(scan, label, SAMPLED, ZERO_IN_TRAINING)
    build = lambda **kw: FIDNet(cfg("FIDNet", **kw), 20)  # noqa: E731
    head = lambda model: model.semantic_head.semantic_output  # noqa: E731
    for loss in ("wce", "dice"):
        for if_bn in (True, False):
            store_keys(out, f"{loss}_bn{int(if_bn)}", build(loss=loss, if_bn=if_bn))
    store_runs(out, [(loss, {"loss": loss}) for loss in ("wce", "dice")], build, head, scan, label, SAMPLED,
               zero_in_training=ZERO_IN_TRAINING)
    model = fill_parameters(build(loss="wce", top_k=0.5), seed=PARAM_SEED)
    out["wce_topk_train_loss"] = np.array(step(model, head, scan, label, True)[0])
    store_branch(out, fill_parameters(build(loss="dice"), seed=PARAM_SEED), scan, label)
    save(out, fname)


if __name__ == "__main__":
    main()
