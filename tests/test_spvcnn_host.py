"""SPVCNN on the host: its state_dict is the reference's (tests/golden/model_spvcnn.npz, made by tests/golden/make_golden_spvcnn.py
from the REAL reference) for both blocks and with SyncBatchNorm modules, the ABI rows of its kernels agree with the header, the numpy
restatement of the mean rule (tests/spvcnn_ref.py) keeps its bound, the reference's import path binds after install_as_dropin, and the
registry still refuses the name.  tests/test_gpu_spvcnn_model.py compares the HIP path with the same file."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import spvcnn_ref as R
from taseg_amd import _lib
from taseg_amd.data.synthetic import fill_parameters, make_model_cfg
from taseg_amd.pcseg.model.segmentor.fusion.spvcnn import SPVCNN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_dim=4, cr=0.5, num_layer=[1] * 8, LABEL_SMOOTHING=0.1, DROPOUT_P=0.0)
NEW_ENTRY_POINTS = (("ts_voxelize_mean_piece_rows", 0), ("ts_voxelize_mean_set_piece_rows", 1), ("ts_point_groups_workspace_bytes", 1),
                    ("ts_point_groups", 8), ("ts_voxelize_mean_workspace_bytes", 2), ("ts_voxelize_mean_forward", 12),
                    ("ts_voxelize_mean_backward", 9), ("ts_point_tail_forward", 15))


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_spvcnn.npz"), allow_pickle=False))


def test_state_dict_and_parameters_equal_the_reference(g):
    assert repr(sorted(CFG.items())) == str(g["cfg"])
    model = fill_parameters(SPVCNN(make_model_cfg("SPVCNN", **CFG), 20), seed=int(g["param_seed"]))
    assert model.name == "spvcnn"
    sd = model.state_dict()
    assert list(sd.keys()) == g["state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["state_shapes"].tolist()
    assert [zlib.crc32(v.numpy().tobytes()) for v in sd.values()] == g["param_crc"].tolist()
    # `point_transforms` sits behind `classifier`, as in the reference
    keys = list(sd.keys())
    assert keys.index("classifier.0.bias") + 1 == keys.index("point_transforms.0.0.weight")
    assert isinstance(model.point_transforms[0][1], torch.nn.BatchNorm1d) and isinstance(model.point_transforms[2][2], torch.nn.ReLU)


def test_bottleneck_and_sync_batch_norm_variants(g):
    bott = SPVCNN(make_model_cfg("SPVCNN", BLOCK="Bottleneck", **CFG), 20).state_dict()
    assert list(bott.keys()) == g["bottleneck_state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in bott.values()] == g["bottleneck_state_shapes"].tolist()
    dist = SPVCNN(make_model_cfg("SPVCNN", if_dist=True, **CFG), 20)
    assert list(dist.state_dict().keys()) == g["state_keys"].tolist()
    assert all(isinstance(t[1], torch.nn.SyncBatchNorm) for t in dist.point_transforms)
    assert isinstance(dist.stem[1], torch.nn.SyncBatchNorm) and isinstance(dist.stage1[1].net[1], torch.nn.SyncBatchNorm)


def test_multi_scale_other_than_concat_builds_no_classifier():
    """reproduced (spvcnn.py:330-333, :449): the head exists for 'concat' only, and forward reaches for it whatever the setting"""
    model = SPVCNN(make_model_cfg("SPVCNN", MULTI_SCALE="sum", **CFG), 20)
    assert not hasattr(model, "classifier") and not any(k.startswith("classifier") for k in model.state_dict())
    with pytest.raises(TypeError):
        model.forward_ensemble({})                                  # forward(ensemble=True): no such parameter (:483-484)


def test_header_and_signatures_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taseg_hip.h")).read(), flags=re.S)      # declarations only
    for name, n_args in NEW_ENTRY_POINTS:
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1).strip()
        declared = 0 if decl == "void" else len(decl.split(","))
        assert declared == n_args == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    piece = lib.ts_voxelize_mean_piece_rows()
    assert piece in (16, 32, 64)
    # the workspace holds one float32 row per full piece: it grows with the rows and with the width
    small, more_rows, wider = (lib.ts_voxelize_mean_workspace_bytes(n, c) for n, c in ((1000, 64), (100000, 64), (1000, 256)))
    assert 0 < small < more_rows and small < wider and small >= (1000 // piece) * 64 * 4
    assert lib.ts_voxelize_mean_set_piece_rows(48) != 0 and lib.ts_voxelize_mean_piece_rows() == piece      # 16, 32 or 64 only


def test_build_compiles_the_kernels_without_fused_multiply_add():
    from taseg_amd.csrc import build
    assert "spvcnn.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["spvcnn.hip"]


@pytest.mark.parametrize("piece", [16, 32, 64])
@pytest.mark.parametrize("c", [4, 48])
def test_restated_mean_rule_keeps_its_bound(piece, c):
    """pieces of P, ascending order, np.float32 at every step: within gamma(cnt + 1) * sum |f| / cnt of the float64 mean"""
    feat, idx, m = R.piece_map(piece, c)
    got = R.mean32(feat, idx, m, piece)
    ref, bound, cnt = R.mean64(feat, idx, m)
    assert got.dtype == np.float32 and sorted(cnt.tolist())[-1] == 4 * piece and {0, 1, piece, piece + 1, 3 * piece + 5} <= set(cnt.tolist())
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (got[cnt == 0] == 0).all() and err.max() > 0                      # rounding is there to be bounded
    # the order is part of the rule: one sequential sum over a long voxel gives other bits
    long_v = int(np.flatnonzero(cnt == 4 * piece)[0])
    assert not np.array_equal(R.mean32(feat, idx, m, 10 ** 6)[long_v], got[long_v])
    # the adjoint restated: a gather, zero rows where the row took no part
    gout = np.random.RandomState(3).randn(m, c).astype(np.float32)
    back = R.mean_backward(gout, idx, m)
    out_of_map = (idx < 0) | (idx >= m)
    assert out_of_map.sum() == 10 and (back[out_of_map] == 0).all()
    inside = np.flatnonzero(~out_of_map)
    assert np.array_equal(back[inside], gout[idx[inside]] / cnt[idx[inside]].astype(np.float32)[:, None])


def test_host_form_of_the_op_is_the_mean():
    """functional.spvoxelize_mean on the host (double rows anywhere): the tensor ops, equal to the float64 mean"""
    from taseg_amd.torchsparse.nn import functional as F
    feat, idx, m = R.piece_map(16, 8)
    x = torch.from_numpy(feat).double().requires_grad_()
    y = F.spvoxelize_mean(x, torch.from_numpy(idx), m)
    ref, _, cnt = R.mean64(feat, idx, m)
    assert np.abs(y.detach().numpy() - ref).max() <= 1e-12
    y.sum().backward()
    want = np.where(((idx >= 0) & (idx < m))[:, None], 1.0 / np.maximum(cnt[np.clip(idx, 0, m - 1)], 1)[:, None], 0.0)
    assert np.abs(x.grad.numpy() - want).max() <= 1e-12


def test_reference_import_path_binds_after_install_as_dropin():
    code = ("import taseg_amd; names = taseg_amd.install_as_dropin()\n"
            "from pcseg.model.segmentor.fusion.spvcnn import SPVCNN\n"
            "import pcseg.model.segmentor, pcseg.model.segmentor.fusion\n"
            "from pcseg.model.segmentor.fusion.spvcnn.utils import initial_voxelize, point_to_voxel, voxel_to_point\n"
            "import taseg_amd.pcseg.model.segmentor.fusion.spvcnn as mine\n"
            "assert SPVCNN is mine.SPVCNN and names['pcseg.model.segmentor.fusion.spvcnn'] is mine\n"
            "print('SPVCNN_DROPIN_OK')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "SPVCNN_DROPIN_OK" in r.stdout, r.stdout + r.stderr


def test_the_registry_still_refuses_the_name():
    """build_network(NAME='SPVCNN') stays NotImplementedError and `_OUT_OF_SCOPE` keeps the name: tests/test_host_logic.py::
    test_registry_errors and tests/test_cylinder_host.py::test_the_other_six_names_stay_refused pin both, and existing test files are
    not edited.  The model is constructed through the reference's module path, `SPVCNN(model_cfgs, num_class)`; the one-line registry
    entry is left to whoever next touches those two tests."""
    from taseg_amd.pcseg.model import build_network
    from taseg_amd.pcseg.model import segmentor
    assert "SPVCNN" in segmentor._OUT_OF_SCOPE and "SPVCNN" not in segmentor.__all__
    with pytest.raises(NotImplementedError):
        build_network(make_model_cfg("SPVCNN", **CFG), 20)
