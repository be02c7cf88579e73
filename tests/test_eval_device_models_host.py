"""Evaluation of all five segmentors on the device and label export from validation batches, the parts that need no GPU: the
forwards' signatures, evaluate()'s new parameters and their argument errors, the remap table, and that CPU tensors are refused."""
import inspect

import numpy as np
import pytest
import torch


def test_the_three_forwards_take_defer_and_device_tail_and_todays_calls():
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet_ms import MinkUNetMs
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet_ms_kd import MinkUNetMsKd
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet_ms_mm import MinkUNetMsMm, MinkUNetMsMmNus
    want = inspect.signature(MinkUNetMs.forward)
    for cls in (MinkUNetMsMm, MinkUNetMsMmNus, MinkUNetMsKd):
        sig = inspect.signature(cls.forward)
        assert list(sig.parameters)[:5] == ["self", "batch_dict", "return_logit", "return_tta", "defer"]
        assert [sig.parameters[k].default for k in ("return_logit", "return_tta", "defer")] == [False, False, False]
        new = [k for k in sig.parameters if k not in ("self", "batch_dict", "return_logit", "return_tta", "defer")]
        assert new == ["device_tail"] and sig.parameters["device_tail"].default is None
        assert str(sig) == str(want)
        sig.bind(None, {}), sig.bind(None, {}, True, False), sig.bind(None, {}, return_tta=True, defer=True)
    assert MinkUNetMsMmNus.forward is MinkUNetMsMm.forward          # inherited, not a second copy


def test_evaluate_appends_predictions_and_remap():
    from taseg_amd.pcseg import eval as E
    p = inspect.signature(E.evaluate).parameters
    assert list(p) == ["model", "batches", "num_class", "tta_votes", "dataset", "save_dir", "prefetch", "on_device", "scores",
                       "predictions", "remap"]
    assert p["predictions"].default is False and p["remap"].default is None
    assert p["on_device"].default is False and p["scores"].default is None


@pytest.mark.parametrize("on_device", [False, True])
def test_argument_errors_come_before_the_model_runs(on_device):
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="tta_votes == 0"):
        E.evaluate(model, [], 20, tta_votes=3, predictions=True, on_device=on_device)
    with pytest.raises(ValueError, match="predictions=True or tta_votes > 0"):
        E.evaluate(model, [], 20, remap=LEARNING_MAP_INV, on_device=on_device)
    with pytest.raises(TypeError, match="dictionary or a lookup array"):
        E.evaluate(model, [], 20, predictions=True, remap=[0, 1, 2], on_device=on_device)
    with pytest.raises(TypeError, match="1-d and integer"):
        E.evaluate(model, [], 20, predictions=True, remap=np.zeros(30, np.float32), on_device=on_device)
    with pytest.raises(ValueError, match="20 classes"):
        E.evaluate(model, [], 20, predictions=True, remap=np.zeros(19, np.int32), on_device=on_device)
    with pytest.raises(ValueError, match="empty"):
        E.evaluate(model, [], 20, tta_votes=3, remap={}, on_device=on_device)


def test_host_path_without_batches_returns_the_new_key_only_when_asked():
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    model = torch.nn.Linear(1, 1)
    assert set(E.evaluate(model, [], 20)) == {"iou", "miou", "hist"}
    out = E.evaluate(model, [], 20, predictions=True, remap=LEARNING_MAP_INV, save_dir="unused")
    assert set(out) == {"iou", "miou", "hist", "predictions"} and out["predictions"] == []


def test_remap_table_and_payload_helpers():
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    lut = E._remap_table(LEARNING_MAP_INV, 20)
    assert lut.dtype == np.int32 and np.array_equal(lut, E.remap_lut(LEARNING_MAP_INV))
    assert np.array_equal(E._remap_table(lut.astype(np.int64), 20), lut)
    classes = np.array([0, 1, 19, 7, 7], np.int64)
    plain = E._class_payload(classes, "semantickitti")
    logits = np.full((5, 20), -1.0, np.float32)
    logits[np.arange(5), classes] = 1.0
    assert plain.dtype == np.uint32 and plain.shape == (5, 1) and np.array_equal(plain, E.vote_payload(logits))
    mapped = E._remapped(plain, lut)
    assert mapped.dtype == np.uint32 and mapped.shape == (5, 1)
    assert mapped[:, 0].tolist() == [LEARNING_MAP_INV[c] for c in classes.tolist()]
    assert np.array_equal(mapped[:, 0], E.remap_labels(plain, lut)) and E._remapped(plain, None) is plain
    with pytest.raises(ValueError, match="class 0"):
        E._class_payload(classes, "nuscenes")
    assert E._class_payload(classes[1:], "nuscenes").dtype == np.uint8


def test_device_tail_arguments_and_cpu_tensors():
    from taseg_amd import backend as B
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    with pytest.raises(ValueError, match="votes == 0"):
        DeviceEvalTail(20, "cpu", votes=3, predictions=True)
    with pytest.raises(ValueError, match="20 classes"):
        DeviceEvalTail(20, "cpu", predictions=True, remap=np.zeros(19, np.int32))
    tail = DeviceEvalTail(20, "cpu", predictions=True, remap=LEARNING_MAP_INV)
    assert tail.predictions and tail.lut.dtype == torch.int32 and tail.lut.tolist() == E.remap_lut(LEARNING_MAP_INV).tolist()
    assert DeviceEvalTail(20, "cpu").lut is None and not DeviceEvalTail(20, "cpu").predictions
    # the tail's launches still refuse host tensors - with the new outputs asked for, too
    logits, scene, inv = torch.zeros(4, 20), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    flags, hist = torch.zeros(1, dtype=torch.int32), torch.zeros((20, 20), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_confusion(logits, scene, scene, inv, torch.zeros(4, dtype=torch.uint8), scene, torch.tensor([4]), hist, flags,
                         want_pred=True, want_counts=True)
    from taseg_amd.torchsparse import SparseTensor
    coords = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tail.run(logits, scene, SparseTensor(inv, coords), SparseTensor(torch.zeros(4, dtype=torch.uint8), coords), torch.tensor([4]),
                 names=["a"])
