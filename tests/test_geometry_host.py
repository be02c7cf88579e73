"""tests/golden/ops_geometry.npz (the real reference's overlapping-window `spdownsample` and its convolutions over kernel 3 /
stride 2, anisotropic strides and anisotropic kernels) pinned on the CPU: a numpy restatement of downsample.py:32-51 gives the
fixture's coordinates, the oracle gives its kernel maps and convolution results.  tests/test_gpu_geometry.py compares the HIP
path with the same fixture and the same restatement."""
import itertools
import os
import re

import numpy as np
import pytest

from oracle import ts_oracle as O
from taseg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDED = {"a": ((3, 3, 3), (2, 2, 2), (1, 1, 1)), "b": ((3, 3, 3), (2, 2, 1), (1, 1, 1)),
           "c": ((3, 3, 3), (2, 2, 2), (2, 2, 2)), "d": ((3, 1, 3), (2, 1, 2), (1, 1, 1))}      # kernel, stride, input tensor stride
PLAIN = {"e133": (1, 3, 3), "e313": (3, 1, 3), "e113": (1, 1, 3)}


def ntuple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def windows_ref(coords, stride, kernel_size, tensor_stride=1):
    """downsample.py:32-51 restated per axis: the offsets of an axis that pass both tests (multiple of stride * tensor_stride,
    not below the minimum over ALL rows), the product of the three lists per row, `np.unique` over (b, x, y, z)."""
    stride, kernel_size, tensor_stride = ntuple(stride), ntuple(kernel_size), ntuple(tensor_stride)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    if len(coords) == 0:
        return np.zeros((0, 4), np.int32)
    cmin = coords[:, :3].min(0)
    rows = []
    for c in coords:
        lists = []
        for a in range(3):
            step = stride[a] * tensor_stride[a]
            cand = [c[a] + o * tensor_stride[a] for o in range(-kernel_size[a] // 2 + 1, kernel_size[a] // 2 + 1)]
            lists.append([v for v in cand if v % step == 0 and v >= cmin[a]])
        rows += [(c[3], x, y, z) for x, y, z in itertools.product(*lists)]
    if not rows:
        return np.zeros((0, 4), np.int32)
    u = np.unique(np.array(rows, dtype=np.int64), axis=0)
    return u[:, [1, 2, 3, 0]].astype(np.int32)


def windows_ref_candidates(coords, stride, kernel_size, tensor_stride=1):
    """the same rows in the reference's own form (downsample.py:32-48: all K candidates of every row, the two masks), one offset
    at a time on numpy - for clouds too large for the per-row loop above"""
    stride, kernel_size, tensor_stride = ntuple(stride), ntuple(kernel_size), ntuple(tensor_stride)
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    step = np.array([stride[a] * tensor_stride[a] for a in range(3)])
    cmin = c[:, :3].min(0) if len(c) else np.zeros(3, np.int64)
    kept = [np.zeros((0, 4), np.int64)]
    for off in O.get_kernel_offsets(kernel_size, tensor_stride).astype(np.int64):
        xyz = c[:, :3] + off
        keep = ((xyz % step == 0) & (xyz >= cmin)).all(1)
        kept.append(np.concatenate([c[keep, 3:], xyz[keep]], 1))
    rows = np.concatenate(kept)
    lo = rows.min(0) if len(rows) else np.zeros(4, np.int64)
    span = (rows.max(0) - lo + 1) if len(rows) else np.ones(4, np.int64)
    key = np.zeros(len(rows), np.int64)
    for col in range(4):                                   # (b, x, y, z) as one integer: a 1-D unique instead of a row-wise one
        key = key * span[col] + (rows[:, col] - lo[col])
    rows = rows[np.unique(key, return_index=True)[1]]
    return rows[:, [1, 2, 3, 0]].astype(np.int32)


def cap(kernel_size, stride):
    return int(np.prod([-(-k // s) for k, s in zip(ntuple(kernel_size), ntuple(stride))]))


def close(a, b, tol=1e-5):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, (err, scale)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ops_geometry.npz"), allow_pickle=False))


def test_fixture_input_is_what_the_geometries_need(g):
    c = g["coords"]
    assert c.dtype == np.int32 and 500 <= len(c) <= 580 and len(np.unique(c, axis=0)) == len(c)
    s0, s1 = c[c[:, 3] == 0, :3], c[c[:, 3] == 1, :3]
    assert s0.min() == 3 and s0.max() <= 13 and s1.min(0).tolist() == [-2, -2, -2] and s1.max() <= 8
    # one voxel alone at the global minimum: nothing else of its scene within two cells
    near = np.abs(s1 - (-2)).max(1) <= 2
    assert int(near.sum()) == 1
    assert np.array_equal(g["c_coords_in"], g["a_coords"]) and np.array_equal(g["a_coords_in"], c)


@pytest.mark.parametrize("tag", sorted(STRIDED))
def test_restatement_equals_the_reference_coordinates(g, tag):
    kernel, stride, ts = STRIDED[tag]
    src = g[f"{tag}_coords_in"]
    want = g[f"{tag}_coords"]
    got = windows_ref(src, stride, kernel, ts)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert len(want) <= cap(kernel, stride) * len(src)


def test_global_minimum_and_row_growth(g):
    c = g["coords"]
    # a per-scene minimum would drop rows of scene 0 that the reference keeps: x = 2 lies below scene 0's own minimum of 3
    a = g["a_coords"]
    assert bool(((a[:, 3] == 0) & (a[:, :3].min(1) < 3)).any())
    per_scene = np.concatenate([windows_ref(c[c[:, 3] == b], 2, 3, 1) for b in (0, 1)])
    assert len(per_scene) < len(a)
    # stride (2, 2, 1): more rows out than in - buffers sized by the input would overflow
    assert len(g["b_coords"]) > len(c) and cap(3, (2, 2, 1)) == 12 and cap(3, 2) == 8 and cap(5, 2) == 27


@pytest.mark.parametrize("kernel,stride,ts", [(5, 2, 1), (1, 2, 1), ((3, 1, 3), (2, 1, 2), (2, 2, 1)), (3, (2, 2, 1), (2, 2, 1)),
                                              (4, 3, 1), (2, (2, 1, 3), 2)])
def test_restatement_equals_the_candidate_list_form(g, kernel, stride, ts):
    """the per-axis product against the formulation of downsample.py:32-48 written out on numpy (all K candidates, two masks)"""
    kernel, stride, ts = ntuple(kernel), ntuple(stride), ntuple(ts)
    c = g["coords"].astype(np.int64)
    c[:, :3] *= np.array(ts)
    got = windows_ref(c, stride, kernel, ts)
    assert np.array_equal(got, windows_ref_candidates(c, stride, kernel, ts)) and len(got) <= cap(kernel, stride) * len(c)
    assert windows_ref_candidates(c[:0], stride, kernel, ts).shape == (0, 4)


@pytest.mark.parametrize("tag", sorted(STRIDED) + sorted(PLAIN))
def test_oracle_kernel_map_and_convolution(g, tag):
    if tag in STRIDED:
        kernel, _, ts = STRIDED[tag]
        src, dst = g[f"{tag}_coords_in"], g[f"{tag}_coords"]
        x = g["c_x"] if tag == "c" else g["x"]
    else:
        kernel, ts = PLAIN[tag], (1, 1, 1)
        src = dst = g["coords"]
        x = g["x"]
    _, nbmaps, nbsizes = O.build_kmap(src, dst, O.get_kernel_offsets(kernel, ts))
    assert np.array_equal(nbmaps, g[f"{tag}_nbmaps"]) and np.array_equal(nbsizes, g[f"{tag}_nbsizes"])
    assert len(nbsizes) == int(np.prod(kernel)) and int(nbsizes.sum()) == len(nbmaps)
    sizes = (len(src), len(dst))
    y = O.conv_forward(x, g[f"{tag}_w"], nbmaps, nbsizes, sizes)
    close(y, g[f"{tag}_y"])
    if tag in STRIDED:
        close(O.conv_forward(y, g[f"{tag}_wu"], nbmaps, nbsizes, sizes, transposed=True), g[f"{tag}_yu"])


def test_header_and_signatures_agree():
    header = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    for name, n_args in (("ts_downsample_windows_workspace_bytes", 7), ("ts_downsample_windows", 16)):
        decl = re.search(name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
