"""FIDNet on the GPU against what the REAL reference produced for the same batch and parameters (tests/golden/model_fidnet.npz,
tests/golden/make_golden_fidnet.py), after tests/test_gpu_salsanext_model.py and with its bars (tests/fid_models.py holds the steps and the
comparison): logits and loss within 1e-3, the stored gradients within 2e-2 (BatchNorm in training mode) / 1e-4 (on running statistics)
of the reference's norm, every parameter's gradient norm, the evaluation branch's arg-max wherever the top-2 margin exceeds 2e-3.  A
stored gradient over its bar is held to 4 x the distance the float32 reference itself lies from a float64 evaluation of its own
expression (the fixture's `dist64`; fid_models.check_against_golden says why, profiles/fidnet_float64.txt has the numbers).  Every
step counts the calls of the four kernel wrappers: one decoder call per direction and one BatchNorm call per fused layer with the
kernel paths on, none through the chain - a quiet fall-back fails.  Both the kernel paths (csrc/fid.hip, csrc/bn.hip) and the chain of modules
(`image_fid_upcat` and `image_fused_bn` off) meet them.

Two training steps from one state give the same bits with the kernel paths on, once torch.backends.cudnn.deterministic keeps the
library's own convolutions to deterministic solvers.  Under autocast the logits stay within 4 x the distance that half storage moves a
float64 evaluation of the same model.  `evaluate_range_view` in "pixels" mode equals the host loop."""
import pytest

import fid_models as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernels", [True, False], ids=["kernels", "chain"])
@pytest.mark.parametrize("variant", ["wce", "dice"])
@pytest.mark.parametrize("tag", ["train", "eval"])
def test_model_vs_reference_golden(variant, tag, kernels):
    M.check_model_vs_golden("fidnet", variant, tag, kernels)


def test_top_k_percent_pixels_and_evaluation_branch():
    M.check_top_k_and_evaluation_branch("fidnet", "wce")


def test_two_training_steps_from_one_state_give_the_same_bits(monkeypatch):
    M.check_two_steps_give_the_same_bits("fidnet", "wce", monkeypatch)


def test_autocast_runs_and_stays_close_to_fp32():
    M.check_autocast("fidnet")


def test_evaluate_range_view_equals_the_host_loop():
    M.check_evaluate_range_view_pixels("fidnet")
