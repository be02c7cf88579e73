"""Evaluation on the device, the parts that need no GPU: the C ABI's new names (include/taseg_hip.h against the ctypes table and the
built library), the new parameters' defaults, and that CPU tensors are refused."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = {"ts_eval_rows_workspace_bytes": 2, "ts_eval_rows": 11, "ts_eval_confusion": 21, "ts_eval_votes": 21}


def test_abi_names_and_argument_counts():
    from taseg_amd import _lib
    header = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["ts_eval_rows_workspace_bytes"][0] is ctypes.c_size_t
    fn = _lib.load().ts_eval_rows_workspace_bytes
    assert fn(0, 1) >= 256 and fn(1000, 64) > fn(1000, 1) > 12 * 1000


def test_new_parameters_default_to_the_host_path():
    from taseg_amd.pcseg import eval as E
    p = inspect.signature(E.evaluate).parameters
    assert p["on_device"].default is False and p["scores"].default is None
    assert list(p)[:7] == ["model", "batches", "num_class", "tta_votes", "dataset", "save_dir", "prefetch"]


def test_forward_signatures_still_take_todays_calls():
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import MinkUNet
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet_ms import MinkUNetMs
    for cls in (MinkUNet, MinkUNetMs):
        sig = inspect.signature(cls.forward)
        assert list(sig.parameters)[:5] == ["self", "batch_dict", "return_logit", "return_tta", "defer"]
        assert [sig.parameters[k].default for k in ("return_logit", "return_tta", "defer")] == [False, False, False]
        new = [k for k in sig.parameters if k not in ("self", "batch_dict", "return_logit", "return_tta", "defer")]
        assert len(new) == 1 and sig.parameters[new[0]].default is None
        sig.bind(None, {}), sig.bind(None, {}, True, False), sig.bind(None, {}, return_tta=True, defer=True)


def test_cpu_tensors_are_refused():
    from taseg_amd import backend as B
    logits, scene, inv = torch.zeros(4, 20), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    flags, hist = torch.zeros(1, dtype=torch.int32), torch.zeros((20, 20), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_confusion(logits, scene, scene, inv, torch.zeros(4, dtype=torch.uint8), scene, torch.tensor([4]), hist, flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_votes(logits, scene, scene, inv, torch.tensor([4]), flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_votes(logits, scene, scene, inv, torch.tensor([4]), flags, point_mask=torch.ones(4, dtype=torch.bool))


def test_device_tail_arguments():
    from taseg_amd.pcseg import eval as E
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    with pytest.raises(ValueError, match="scores"):
        DeviceEvalTail(20, "cpu", votes=3, scores="best")
    with pytest.raises(ValueError, match="on_device=True"):
        E.evaluate(torch.nn.Linear(1, 1), [], 20, tta_votes=3, scores="all")
    with pytest.raises(ValueError, match="on_device=False"):
        E.evaluate(torch.nn.Linear(1, 1), [], 20, on_device=True)
    for bit, exc in ((1, IndexError), (2, ValueError), (4, IndexError), (8, IndexError), (16, ValueError), (32, IndexError)):
        with pytest.raises(exc):
            DeviceEvalTail.raise_flags(bit, 2)
    with pytest.raises(ValueError, match="on_device=False"):
        DeviceEvalTail.raise_flags(2, 2)
    DeviceEvalTail.raise_flags(0, 2)
