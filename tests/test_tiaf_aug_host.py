"""Host side of the TIAF recipe's training augmentation, image flip and TTA views (no GPU): the draws recorded in
tests/golden/tiaf_aug.npz - what the REAL reference took from numpy's generator while `SemantickittiMsMmDataset.__getitem__` and
`SemkittiVoxelMsMmDataset.get_single_sample` ran - replay from np.random.RandomState(seed) through draw_image_flips, mix.draw_coin
and draw_train_params / draw_tta_params, in the reference's order; the frame record's layout; the new entry points' bindings."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from taseg_amd.data import augment as A
from taseg_amd.data import mix as M
from taseg_amd.data import tiaf as TF


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "tiaf_aug.npz"), allow_pickle=False))


def test_flips_coin_and_augmentation_replay_the_reference_draws(g):
    deltas = g["train_camera_deltas"].tolist()
    assert deltas == sorted(deltas) and deltas[-1] == 0                      # oldest frame first, the current frame last
    for b, seed in enumerate(g["train_seeds"].tolist()):
        rng = np.random.RandomState(seed)
        flips = TF.draw_image_flips(rng, reversed(deltas))                   # any order in: the walk is delta ascending
        assert list(flips) == deltas and [flips[d] for d in deltas] == g["train_flips"][b].tolist()
        assert len(set(flips.values())) == 2                                 # a flipped and an un-flipped frame in every sample
        assert M.draw_coin(rng) == int(g["train_coin"][b])                   # semantickitti_ms_mm.py:178, between the two
        p = A.draw_train_params(rng)
        assert p.theta == g["train_theta"][b] and p.scale == g["train_scale"][b] and p.flip == g["train_flip"][b]
        assert list(p.translate) == g["train_noise"][b].tolist()
        assert p.rotate_on and p.scale_on and p.flip_on and p.translate_on
    # case `wide`: the same seeds, the same flips, no augmentation draws behind the coin
    assert np.array_equal(g["wide_flips"], g["train_flips"]) and np.array_equal(g["wide_coin"], g["train_coin"])


def test_no_draw_without_image_flip_or_for_a_missing_frame():
    probe = np.random.RandomState(3).rand(4)
    rng = np.random.RandomState(3)
    assert TF.draw_image_flips(rng, [-8, -4, 0], image_flip=False) == {-8: False, -4: False, 0: False}
    assert rng.rand() == probe[0]                                            # nothing was consumed
    # the head of a sequence: frame -8 does not exist, the dictionary has no entry for it
    frames = {0: {"image": None}, -4: {"image": None}, -1: {}, -2: {}}
    rng = np.random.RandomState(3)
    flips = TF.draw_image_flips(rng, frames)
    assert flips == {-4: bool(probe[0] < 0.5), 0: bool(probe[1] < 0.5)}
    assert rng.rand() == probe[2]
    rng = np.random.RandomState(3)
    assert TF.draw_image_flips(rng, [0], flip_ratio=0.0) == {0: False} and rng.rand() == probe[1]     # drawn, never below 0


def test_tta_parameters_replay_the_reference_draws(g):
    rng = np.random.RandomState(int(g["tta_seed"]))
    lo, hi = g["tta_votes"].tolist()
    assert (lo, hi) == (1, 4)
    for i, v in enumerate(range(lo, hi)):
        assert M.draw_coin(rng) == int(g["tta_coin"][i])                     # every vote reads the sample again
        p = A.draw_tta_params(rng, v)
        assert p.theta == g["tta_theta"][i] == A.TTA_ANGLES[v] * np.pi / 8.0 and p.scale == g["tta_scale"][i]
        assert not p.flip_on and not p.translate_on


def test_frame_record_has_the_headers_layout(tmp_path):
    """FRAME_DTYPE crosses the boundary as bytes: the size and the field offsets a C compiler gives TsTiafFrame"""
    assert TF.FRAME_DTYPE.itemsize == 256 and TF._HOST_FIELDS.itemsize == 32
    assert TF.FRAME_DTYPE.fields["row_offset"][1] == 224                     # the host's fields are the record's tail
    if shutil.which("gcc") is None:
        return
    names = TF.FRAME_DTYPE.names
    offs = ", ".join(f"offsetof(TsTiafFrame, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "taseg_hip.h"\nint main(void) {\n  printf("'
                   + " ".join(["%zu"] * (1 + len(names))) + '\\n", sizeof(TsTiafFrame), ' + offs + ");\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert seen == [TF.FRAME_DTYPE.itemsize] + [TF.FRAME_DTYPE.fields[n][1] for n in names]


def test_tiaf_entry_points_are_declared_and_bound():
    from taseg_amd import _lib
    from taseg_amd import backend as B
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ts_tiaf_image_stack", "ts_tiaf_fov_cloud", "ts_tiaf_fov_cloud_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["ts_tiaf_image_stack"][1]) == 14 and len(_lib.SIGNATURES["ts_tiaf_fov_cloud"][1]) == 19
    lib = _lib.load()
    assert lib.ts_tiaf_fov_cloud_workspace_bytes(0, 1) == 256
    assert lib.ts_tiaf_fov_cloud_workspace_bytes(257, 4) == 3 * 256
    assert (B.TIAF_IMAGE_FRAMES, B.TIAF_MAX_SAMPLES, B.TIAF_MAX_FRAMES, B.TIAF_FRAME_BYTES) == (16, 64, 1024, 256)
    text = open(os.path.join(ROOT, "include", "taseg_hip.h")).read()
    for line in ("#define TS_TIAF_IMAGE_FRAMES 16", "#define TS_TIAF_MAX_SAMPLES 64", "#define TS_TIAF_MAX_FRAMES 1024"):
        assert line in text
    assert callable(B.tiaf_image_stack) and callable(B.tiaf_fov_cloud)
