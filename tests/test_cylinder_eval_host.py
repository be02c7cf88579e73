"""Evaluation of Cylinder_TS on the device, the parts that need no GPU: the forward's new keyword, the C ABI's two new names (header,
ctypes table, built library), flag bit 64, the refusal of CPU tensors, and the numpy restatement of the tail
(tests/cylinder_eval_ref.py) against pcseg.eval's host functions."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cylinder_eval_ref as R
from conftest import ROOT

NAMES = {"ts_eval_confusion_rows": 18, "ts_eval_votes_rows": 18}


def test_forward_takes_the_tail_and_defaults_to_the_host_branch():
    from taseg_amd.pcseg.model.segmentor.voxel.cylinder3d.cylinder_ts import Cylinder_TS
    p = inspect.signature(Cylinder_TS.forward).parameters
    assert list(p) == ["self", "batch_dict", "ensemble", "device_tail"]
    assert p["ensemble"].default is False and p["device_tail"].default is None


def test_abi_names_and_argument_counts():
    from taseg_amd import _lib
    header = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int32


def test_flag_64_is_an_index_error_that_names_the_missing_row():
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    with pytest.raises(IndexError, match="no voxel row"):
        DeviceEvalTail.raise_flags(64, 2)
    with pytest.raises(IndexError, match="beyond the 2 scenes"):          # the lower bits keep their order
        DeviceEvalTail.raise_flags(64 | 1, 2)
    DeviceEvalTail.raise_flags(0, 2)


def test_cpu_tensors_are_refused():
    from taseg_amd import backend as B
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    logits, scene, rows = torch.zeros(4, 20), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    flags, hist = torch.zeros(1, dtype=torch.int32), torch.zeros((20, 20), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_confusion_rows(logits, rows, scene, torch.zeros(4, dtype=torch.uint8), torch.tensor([4]), hist, flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_votes_rows(logits, rows, scene, torch.tensor([4]), flags)
    coords = torch.zeros((4, 4), dtype=torch.int32)
    for votes in (0, 1):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DeviceEvalTail(20, "cpu", votes=votes).run_points(logits, coords, coords.long(), rows, torch.tensor([4]), ["a"])


def _random_batch(r, n_scenes, C, dtype, equal=False):
    pts = [int(r.randint(0, 400)) for _ in range(n_scenes)] if not equal else [211] * n_scenes
    n_vox = 97
    logits = r.randn(n_vox, C).astype(dtype)
    pts_scene = np.repeat(np.arange(n_scenes), pts).astype(np.int32)
    rows = r.randint(0, n_vox, len(pts_scene)).astype(np.int64)          # any voxel order: the rows are global
    labels = r.randint(-1, C + 1, len(pts_scene)).astype(np.int64)       # -1 and C lie outside fast_hist's mask
    return logits, rows, pts_scene, labels, pts


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_restatement_equals_the_host_confusion(dtype):
    from taseg_amd.pcseg import eval as E
    r = np.random.RandomState(0)
    for n_scenes, C in ((1, 3), (3, 20), (5, 33)):
        logits, rows, pts_scene, labels, pts = _random_batch(r, n_scenes, C, dtype)
        for shift in (-7, 0, 9):                                         # num_points below, equal to and above the scene's count
            num_points = [max(p + shift, 0) for p in pts]
            hist, pred, m, flags = R.confusion_rows(logits, rows, pts_scene, labels, num_points)
            ret = R.host_dictionary(logits, rows, pts_scene, labels, num_points)
            assert flags == 0 and m.tolist() == [len(p) for p in ret["point_predict"]]
            assert np.array_equal(pred, np.concatenate(ret["point_predict"]))
            full = sum(E.fast_hist(p, lab, C) for p, lab in zip(ret["point_predict"], ret["point_labels"]))
            assert np.array_equal(hist, full) and hist.sum() > 0
            assert np.array_equal(hist[1:, 1:], E.scan_confusions(ret, np.arange(C - 1)))


@pytest.mark.parametrize("V", [1, 3, 10])
def test_restatement_equals_the_host_votes(V):
    from taseg_amd.pcseg import eval as E
    r = np.random.RandomState(V)
    logits, rows, pts_scene, labels, pts = _random_batch(r, V, 20, np.float32, equal=True)
    total, label, flags = R.votes_rows(logits, rows, pts_scene, [200] * V)
    ret = R.host_dictionary(logits, rows, pts_scene, labels, [200] * V)
    want = E.accumulate_votes(ret, V)
    assert flags == 0 and total.dtype == want.dtype == np.float32 and np.array_equal(total.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(label.reshape(-1, 1).astype(np.uint32), E.vote_payload(want, "semantickitti"))
    # half votes are summed in float32: not accumulate_votes on float16 arrays, which rounds after every vote
    half = logits.astype(np.float16)
    total16, _, _ = R.votes_rows(half, rows, pts_scene, [200] * V)
    per_vote = R.host_dictionary(half, rows, pts_scene, labels, [200] * V)["point_predict_logits"]
    want16 = per_vote[0].astype(np.float32)
    for v in range(1, V):
        want16 += per_vote[v].astype(np.float32)
    assert np.array_equal(total16.view(np.uint32), want16.view(np.uint32))


def test_restatement_flags():
    r = np.random.RandomState(4)
    logits, rows, pts_scene, labels, pts = _random_batch(r, 3, 20, np.float32, equal=True)
    _, _, flags = R.votes_rows(logits, rows, pts_scene, [200, 199, 200])
    assert flags == R.FLAG_VOTES
    bad = rows.copy()
    bad[5], bad[300] = -1, 97
    hist, pred, m, flags = R.confusion_rows(logits, bad, pts_scene, np.abs(labels) % 20, pts)
    assert flags == R.FLAG_NO_ROW and pred[5] == pred[300] == 0 and hist.sum() == len(rows) - 2
    swapped = pts_scene.copy()
    swapped[0], swapped[-1] = 2, 0
    assert R.layout(swapped, pts)[2] == R.FLAG_ORDER
    beyond = pts_scene.copy()
    beyond[-1] = 3
    kept, m, flags = R.layout(beyond, pts)
    assert flags == R.FLAG_RANGE and m.tolist() == [211, 211, 210]
