"""Golden vectors of CENet (needs the reference checkout that tests/golden/_ref_env.py names; inert without it).

    python tests/golden/make_golden_cenet.py        ->  tests/golden/model_cenet.npz  (data only)

The REAL reference's `CENet` (pcseg/model/segmentor/range/cenet/model/semantic/cenet.py) on the CPU in float32, through the functions
and stand-ins of make_golden_fidnet.py (the same batch at 16 x 64, the same `fill_parameters(seed)`); no reference code in this file.

Stored, for IF_AUX on (`aux`) and off (`noaux`) with LOSS 'dice' (IF_BN, IF_LS_LOSS and IF_BD_LOSS on, TOP_K_PERCENT_PIXELS 1.0; plus
the `aux` loss at 0.5) what the FIDNet fixture stores; the main head's logits once per BatchNorm mode (the auxiliary heads do not move
them); the state_dict keys and shapes for LOSS 'wce' / 'dice', IF_BN and IF_AUX on and off (`keys/<loss>_bn<0|1>_aux<0|1>`)."""
import numpy as np

import make_golden_fidnet as G

SAMPLED = ("conv1.conv.weight", "conv2.bn.weight", "conv3.conv.weight", "layer1.0.conv1.weight", "layer1.2.bn2.weight",
           "layer2.0.downsample.0.weight", "layer2.0.downsample.1.bias", "layer2.3.conv2.weight", "layer3.0.conv1.weight",
           "layer3.5.bn1.bias", "layer4.0.bn2.weight", "layer4.2.conv2.weight", "conv_1.conv.weight", "conv_1.bn.weight",
           "conv_2.conv.weight", "semantic_output.weight", "aux_head1.weight", "aux_head2.weight", "aux_head3.weight")


def main(fname="model_cenet.npz"):
    G.environment()
    from pcseg.model.segmentor.range.cenet.model.semantic.cenet import CENet
    scan, label = G.inputs()
    out = G.header(scan, label, SAMPLED)
    build = lambda **kw: CENet(G.cfg("CENet", **kw), 20)  # noqa: E731
    head = lambda model: model.semantic_output  # noqa: E731
    for loss in ("wce", "dice"):
        for if_bn in (True, False):
            for aux in (True, False):
                G.store_keys(out, f"{loss}_bn{int(if_bn)}_aux{int(aux)}", build(loss=loss, if_bn=if_bn, IF_AUX=aux))
    G.store_runs(out, [("aux", {"IF_AUX": True}), ("noaux", {"IF_AUX": False})], build, head, scan, label, SAMPLED)
    model = G.fill_parameters(build(top_k=0.5, IF_AUX=True), seed=G.PARAM_SEED)
    out["aux_topk_train_loss"] = np.array(G.step(model, head, scan, label, True)[0])
    G.store_branch(out, G.fill_parameters(build(IF_AUX=True), seed=G.PARAM_SEED), scan, label)
    G.save(out, fname)


if __name__ == "__main__":
    main()
