"""Evaluation of Cylinder_TS on the device (-m gpu): csrc/evaltail.hip ts_eval_confusion_rows / ts_eval_votes_rows through
backend.eval_*_rows against the numpy restatement of tests/cylinder_eval_ref.py, then `Cylinder_TS.forward(device_tail=)`,
DeviceEvalTail.run_points and pcseg.eval.evaluate(on_device=True) against the host branch of the same model.

Every comparison is exact: integers are integers, and the float32 vote sums are formed in one fixed order, so their bits are
numpy's.  The one tolerance is the golden's own: the reference's predictions are compared where its top-2 margin exceeds the
fixture's `margin` (tests/test_gpu_cylinder_model.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cylinder_eval_ref as R  # noqa: E402
from taseg_amd.data.synthetic import synth_scan  # noqa: E402

N_PTS = (0, 1, 255, 256, 257, 1025)          # around one 256-thread block, and several blocks
SCENES = (1, 2, 3, 64)
N_VOX = 97
LABEL_TYPES = (np.uint8, np.int32, np.int64)


def _coords(scene):
    """an [n, 4] int32 coordinate matrix whose last column is the scene index: the kernels read it with stride 4"""
    c = np.zeros((len(scene), 4), np.int32)
    c[:, -1] = scene
    return torch.from_numpy(c).cuda()[:, -1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _split(r, n_pts, n_scenes):
    """points per scene, ascending scene index; with more than one scene, one of them has no point"""
    cuts = np.sort(r.randint(0, n_pts + 1, n_scenes - 1))
    cnt = np.diff(np.concatenate([[0], cuts, [n_pts]]))
    if n_scenes > 1:
        empty = int(r.randint(0, n_scenes))
        other = (empty + 1) % n_scenes
        cnt[other] += cnt[empty]
        cnt[empty] = 0
    return cnt


def _logits(r, C, dtype):
    logits = r.randn(N_VOX, C).astype(dtype)
    logits[10, [1, C - 1]] = 50               # an exact tie: the first maximum wins
    logits[11, C // 2] = np.nan               # a NaN wins
    return logits


def _labels(r, n, C, dtype):
    labels = r.randint(0, C, n).astype(dtype)
    labels[::7] = 255 if dtype == np.uint8 else -1          # outside 0 .. C - 1 (C <= 33)
    labels[3::11] = 255 if dtype == np.uint8 else C
    return labels


def _num_points(cnt, variant):
    """below, equal to and above the scene's count, 0 and negative - one of them per scene, moved on by `variant`"""
    return [(max(c - 3, 0), c, c + 5, 0, -2)[(s + variant) % 5] for s, c in enumerate(cnt.tolist())]


def _confusion(B, logits, rows, pts_scene, labels, num_points, hist=None, flags=None):
    C = logits.shape[1]
    hist = torch.zeros((C, C), dtype=torch.int64, device="cuda") if hist is None else hist
    flags = torch.zeros(1, dtype=torch.int32, device="cuda") if flags is None else flags
    pred, m = B.eval_confusion_rows(_dev(logits), _dev(rows), _coords(pts_scene), _dev(labels), torch.tensor(num_points, dtype=torch.int64),
                                    hist, flags, want_pred=True, want_counts=True)
    return hist, pred, m, flags


def _assert_confusion(got, want, who):
    (hist, pred, m, flags), (w_hist, w_pred, w_m, w_flags) = got, want
    assert int(flags) == w_flags, who
    assert np.array_equal(m.cpu().numpy(), w_m), who
    assert np.array_equal(hist.cpu().numpy(), w_hist), who
    assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy()[:len(w_pred)], w_pred), who


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("C", [3, 20, 32, 33])          # 33: global atomics in place of the LDS table
def test_confusion_equals_the_restatement(C, dtype):
    from taseg_amd import backend as B
    r = np.random.RandomState(C)
    logits = _logits(r, C, dtype)
    seen = 0
    for n_pts in N_PTS:
        for n_scenes in SCENES:
            cnt = _split(r, n_pts, n_scenes)
            pts_scene = np.repeat(np.arange(n_scenes), cnt).astype(np.int32)
            rows = r.randint(0, N_VOX, n_pts).astype(np.int64)          # any order: the rows are global, not grouped by scene
            rows[:2] = (10, 11)[:n_pts]
            for variant in range(5):
                labels = _labels(r, n_pts, C, LABEL_TYPES[variant % 3])
                num_points = _num_points(cnt, variant)
                want = R.confusion_rows(logits, rows, pts_scene, labels, num_points)
                assert want[3] == 0
                got = _confusion(B, logits, rows, pts_scene, labels, num_points)
                _assert_confusion(got, want, (n_pts, n_scenes, variant))
                seen += int(want[0].sum())
                if variant == 0:      # the call ADDS: a second one into the same matrix doubles it
                    again = _confusion(B, logits, rows, pts_scene, labels, num_points, hist=got[0], flags=got[3])
                    assert np.array_equal(again[0].cpu().numpy(), 2 * want[0]) and int(again[3]) == 0
    assert seen > 5000          # (the cases are not empty)
    # the planted rows, kept: scene 0 holds both points
    want = R.confusion_rows(logits, np.array([10, 11]), np.zeros(2, np.int32), np.zeros(2, np.int64), [2])
    assert want[1].tolist() == [1, C // 2]
    got = _confusion(B, logits, np.array([10, 11]), np.zeros(2, np.int32), np.zeros(2, np.int64), [2])
    _assert_confusion(got, want, "tie and NaN")


def _vote_inputs(r, V, n, C, dtype):
    """V votes of n kept points each: vote v has n + (v % 3) points, num_points trims them to n"""
    cnt = np.array([n + (v % 3) for v in range(V)])
    pts_scene = np.repeat(np.arange(V), cnt).astype(np.int32)
    logits = r.randn(N_VOX, C).astype(dtype)
    rows = r.randint(0, N_VOX - 2, len(pts_scene)).astype(np.int64)
    start = np.cumsum(cnt) - cnt
    if n > 3:
        # kept point 3: an exact tie of the sums (columns 0 and C - 1 hold 4.0 in every vote, the rest less); kept point 1: a NaN in vote 0
        logits[N_VOX - 2] = -1.0
        logits[N_VOX - 2, [0, C - 1]] = 4.0
        logits[N_VOX - 1] = logits[5]
        logits[N_VOX - 1, 2] = np.nan
        rows[start + 3] = N_VOX - 2
        rows[start[0] + 1] = N_VOX - 1
    return logits, rows, pts_scene, [n] * V


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("C", [3, 20, 32, 33])          # 33: a second walk over the votes for the columns past 32
@pytest.mark.parametrize("V", [1, 3, 10])
def test_votes_equal_the_sequential_float32_sum(V, C, dtype):
    from taseg_amd import backend as B
    r = np.random.RandomState(100 * V + C)
    for n in N_PTS:
        logits, rows, pts_scene, num_points = _vote_inputs(r, V, n, C, dtype)
        total, want_label, want_flags = R.votes_rows(logits, rows, pts_scene, num_points)
        assert want_flags == 0 and total.shape == (n, C) and total.dtype == np.float32
        if dtype == np.float16 and n:    # the float32 sum of the per-vote arrays, not half accumulation
            per_vote = R.host_dictionary(logits, rows, pts_scene, np.zeros(len(rows)), num_points)["point_predict_logits"]
            check = per_vote[0].astype(np.float32)
            for v in range(1, V):
                check += per_vote[v].astype(np.float32)
            assert per_vote[0].dtype == np.float16 and np.array_equal(check.view(np.uint32), total.view(np.uint32))
        clean = ~np.isnan(total).any(1)
        if n > 3:
            assert want_label[3] == 0 and total[3, 0] == total[3, C - 1] == 4.0 * V and not clean[1] and want_label[1] == 2
        for label_bytes in (4, 1):
            flags = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = B.eval_votes_rows(_dev(logits), _dev(rows), _coords(pts_scene), torch.tensor(num_points), flags, label_bytes=label_bytes,
                                    want_sums=True, want_top3=True)
            assert int(flags) == 0 and int(got["n"]) == n and got["label"].shape[0] == len(pts_scene) // V >= n
            label = got["label"].cpu().numpy()[:n]
            assert label.dtype == (np.uint8 if label_bytes == 1 else np.int32) and np.array_equal(label.astype(np.int64), want_label)
            sums = got["sums"].cpu().numpy()[:n]
            assert sums.dtype == np.float32 and np.array_equal(sums.view(np.uint32), total.view(np.uint32)), (n, label_bytes)
            top3 = got["top3"].cpu().numpy()[:n]
            assert np.array_equal(top3[clean], np.sort(total, 1)[:, ::-1][:, :3][clean])
        got = B.eval_votes_rows(_dev(logits), _dev(rows), _coords(pts_scene), torch.tensor(num_points), flags)      # no optional outputs
        assert got["sums"] is None and got["top3"] is None and np.array_equal(got["label"].cpu().numpy()[:n], want_label)


def _flag_inputs(C=20, dtype=np.float32, cnt=(255, 1, 514)):
    r = np.random.RandomState(7)
    pts_scene = np.repeat(np.arange(len(cnt)), cnt).astype(np.int32)
    n = len(pts_scene)
    return r, _logits(r, C, dtype), r.randint(0, N_VOX, n).astype(np.int64), pts_scene, _labels(r, n, C, np.int64), list(cnt)


@pytest.mark.parametrize("C", [20, 33])
def test_flag_64_a_point_without_a_row_is_not_tallied(C):
    from taseg_amd import backend as B
    r, logits, rows, pts_scene, labels, cnt = _flag_inputs(C)
    labels[:] = r.randint(0, C, len(labels))          # every point would be tallied
    rows[100], rows[300] = -1, N_VOX                  # not found; beyond the logits
    want = R.confusion_rows(logits, rows, pts_scene, labels, cnt)
    assert want[3] == 64 and want[0].sum() == len(rows) - 2 and want[1][100] == want[1][300] == 0
    _assert_confusion(_confusion(B, logits, rows, pts_scene, labels, cnt), want, "bit 64")
    # flags are OR-ed into what the caller's int holds
    held = torch.full((1,), 128, dtype=torch.int32, device="cuda")
    assert int(_confusion(B, logits, rows, pts_scene, labels, cnt, flags=held)[3]) == 128 | 64
    # votes: the vote without a row leaves its term out of the sum
    logits, rows, pts_scene, num_points = _vote_inputs(r, 3, 257, C, np.float32)
    rows[5], rows[257 + 9] = -1, N_VOX + 3            # vote 0 of point 5, vote 1 of point 9
    total, want_label, want_flags = R.votes_rows(logits, rows, pts_scene, num_points)
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = B.eval_votes_rows(_dev(logits), _dev(rows), _coords(pts_scene), torch.tensor(num_points), flags, want_sums=True)
    assert want_flags == 64 and int(flags) == 64
    assert np.array_equal(got["sums"].cpu().numpy()[:257].view(np.uint32), total.view(np.uint32))
    assert np.array_equal(got["label"].cpu().numpy()[:257], want_label)


def test_flag_2_a_batch_column_that_is_not_ascending():
    from taseg_amd import backend as B
    r, logits, rows, pts_scene, labels, cnt = _flag_inputs()
    swapped = pts_scene.copy()
    swapped[0], swapped[-1] = 2, 0
    want = R.confusion_rows(logits, rows, swapped, labels, cnt)
    assert want[3] == 2
    _assert_confusion(_confusion(B, logits, rows, swapped, labels, cnt), want, "bit 2")


def test_flag_1_a_scene_index_beyond_the_batch():
    from taseg_amd import backend as B
    r, logits, rows, pts_scene, labels, cnt = _flag_inputs()
    beyond = pts_scene.copy()
    beyond[-1] = 3
    want = R.confusion_rows(logits, rows, beyond, labels, cnt)
    assert want[3] == 1 and want[2].tolist() == [255, 1, 513]
    _assert_confusion(_confusion(B, logits, rows, beyond, labels, cnt), want, "bit 1")


def test_flag_16_votes_of_unequal_length_write_nothing():
    from taseg_amd import backend as B
    r = np.random.RandomState(9)
    logits, rows, pts_scene, _ = _vote_inputs(r, 3, 270, 20, np.float32)
    args = (_dev(logits), _dev(rows), _coords(pts_scene))
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = B.eval_votes_rows(*args, torch.tensor([270] * 3), flags, want_sums=True, want_top3=True)
    assert int(flags) == 0 and int(out["n"]) == 270
    out["label"].fill_(-7), out["sums"].fill_(-7.0), out["top3"].fill_(-7.0), out["n"].fill_(-7)
    assert R.votes_rows(logits, rows, pts_scene, [270, 269, 270])[2] == 16
    again = B.eval_votes_rows(*args, torch.tensor([270, 269, 270]), flags, want_sums=True, want_top3=True, out=out)
    assert again is out and int(flags) == 16
    assert all(bool((out[k] == -7).all()) for k in ("label", "sums", "top3", "n"))


def test_the_wrappers_own_checks():
    from taseg_amd import backend as B
    r, logits, rows, pts_scene, labels, cnt = _flag_inputs()
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    many = np.arange(65, dtype=np.int32)
    with pytest.raises(ValueError, match="64 scenes"):
        B.eval_votes_rows(_dev(np.zeros((65, 20), np.float32)), _dev(many.astype(np.int64)), _coords(many), torch.ones(65, dtype=torch.int64), flags)
    with pytest.raises(ValueError, match="float32 or float16"):
        B.eval_votes_rows(_dev(logits).double(), _dev(rows), _coords(pts_scene), torch.tensor(cnt), flags)
    with pytest.raises(ValueError, match="uint8, int32 or int64"):
        _confusion(B, logits, rows, pts_scene, labels.astype(np.int16), cnt)
    with pytest.raises(ValueError, match="one label per point"):
        _confusion(B, logits, rows, pts_scene, labels[:-1], cnt)
    with pytest.raises(ValueError, match="one int64 logits row per point"):
        _confusion(B, logits, rows.astype(np.int32), pts_scene, labels, cnt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_votes_rows(_dev(logits).cpu(), _dev(rows), _coords(pts_scene), torch.tensor(cnt), flags)


# ------------------------------------------------------------------------------------------------ model and loop
@pytest.fixture(scope="module")
def g():
    from test_gpu_cylinder_model import ROOT
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "model_cylinder.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def model(g):
    from test_gpu_cylinder_model import _model
    return _model(g).eval()


def _tail(**kw):
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import DeviceEvalTail
    return DeviceEvalTail(20, "cuda", **kw)


def test_golden_batch_tail_equals_the_host_branch_and_the_reference(g, model):
    from test_gpu_cylinder_model import _batch, _model
    from taseg_amd.pcseg import eval as E
    from taseg_amd.pcseg.model.segmentor.voxel.minkunet.minkunet import PendingLabels
    with torch.no_grad():
        host = model(_batch(g))
        tail = _tail()
        assert model(_batch(g), device_tail=tail) is tail
        labelled = _tail(predictions=True)
        pending = model(_batch(g), device_tail=labelled)
    want = sum(E.fast_hist(p, lab, 20) for p, lab in zip(host["point_predict"], host["point_labels"]))
    full = tail.read()
    assert full.shape == (20, 20) and full.dtype == np.int64 and want.sum() > 0
    assert np.array_equal(full, want)
    assert isinstance(pending, PendingLabels)
    out = pending.result()
    assert out["name"] == g["batch_name"].tolist() and len(out["payload"]) == len(host["point_predict"])
    for payload, pred in zip(out["payload"], host["point_predict"]):
        assert payload.dtype == np.uint32 and payload.shape == (len(pred), 1) and np.array_equal(payload[:, 0], pred)
    assert np.array_equal(labelled.read(), want)
    sure = g["branch_margin"] > float(g["margin"])
    assert sure.mean() >= 0.99
    assert np.array_equal(np.concatenate(out["payload"])[:, 0][sure], g["branch_point_predict"][sure])
    # in training mode a tail is ignored: the training tuple, as without it (a model of its own: the pass moves the running statistics)
    ret = _model(g).train()(_batch(g), device_tail=_tail())
    assert isinstance(ret, tuple) and set(ret[0]) == {"loss"}


GRID = ([0, -180, -4], [50, 180, 2], [96, 80, 16])


def _scans(seeds, n_points):
    out = []
    for s in seeds:
        pts, lab = synth_scan(s, n_points=n_points, n_beams=16, n_az=360)
        out.append({"points": torch.from_numpy(pts).cuda(), "labels": torch.from_numpy(lab.astype(np.int64)).cuda(),
                    "name": "dataset/sequences/08/velodyne/%06d.bin" % s})
    return out


@pytest.fixture(scope="module")
def batches():
    from taseg_amd.data import CylinderGrid, build_cylinder_batch
    grid = CylinderGrid(*GRID)
    built = [build_cylinder_batch(_scans(seeds, 1500), grid) for seeds in ((61, 62), (63, 64, 65))]
    return lambda: [dict(b) for b in built]


def test_evaluate_on_device_equals_the_host_loop(model, batches, tmp_path):
    from taseg_amd.data.semantickitti import LEARNING_MAP_INV
    from taseg_amd.pcseg import eval as E
    host = E.evaluate(model, batches(), 20, predictions=True, remap=LEARNING_MAP_INV, save_dir=str(tmp_path / "host"))
    dev = E.evaluate(model, batches(), 20, predictions=True, remap=LEARNING_MAP_INV, save_dir=str(tmp_path / "dev"), on_device=True)
    assert not model.training and host["hist"].sum() > 1000 and host["hist"].shape == dev["hist"].shape == (19, 19)
    assert dev["hist"].dtype == host["hist"].dtype and np.array_equal(dev["hist"], host["hist"])
    assert np.array_equal(dev["iou"], host["iou"]) and dev["miou"] == host["miou"]
    assert len(dev["predictions"]) == len(host["predictions"]) == 5
    for a, b in zip(dev["predictions"], host["predictions"]):
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b)
    written = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "host") for d, _, fs in os.walk(tmp_path / "host") for f in fs)
    assert len(written) == 5 and all(w.endswith(".label") for w in written)
    for w in written:
        assert open(tmp_path / "host" / w, "rb").read() == open(tmp_path / "dev" / w, "rb").read()
    plain = E.evaluate(model, batches(), 20, on_device=True)
    assert set(plain) == {"iou", "miou", "hist"} and np.array_equal(plain["hist"], host["hist"])


def test_a_validation_pass_reads_the_host_once_at_the_end(model, batches):
    """the existing eval-device tests do not count copies: the objects say where the data is - every batch returns the tail itself,
    whose matrix and flags are device tensors, and `read()` is the call that returns host memory"""
    from taseg_amd.pcseg import eval as E
    tail = _tail()
    with torch.no_grad():
        for batch in batches():
            assert model(batch, device_tail=tail) is tail
            assert tail.hist.is_cuda and tail.flags.is_cuda
    full = tail.read()
    assert isinstance(full, np.ndarray)
    assert np.array_equal(full[1:, 1:], E.evaluate(model, batches(), 20)["hist"])


def _tta_batch():
    from taseg_amd.data import CylinderGrid, build_cylinder_tta_batch
    return build_cylinder_tta_batch(_scans((71,), 1500)[0], 0, 3, np.random.RandomState(5), CylinderGrid(*GRID))


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast"])
def test_tta_on_device_gives_the_host_payload_and_sums(model, amp):
    from taseg_amd.pcseg import eval as E
    batch = _tta_batch()
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        with torch.no_grad():
            ret = model(dict(batch))
        dev = E.evaluate(model, [dict(batch)], 20, tta_votes=3, on_device=True, scores="all")
        top3 = E.evaluate(model, [dict(batch)], 20, tta_votes=3, on_device=True, scores="top3")
    per_vote = ret["point_predict_logits"]
    assert len(per_vote) == 3 and len(per_vote[0]) == 1500
    total = per_vote[0].astype(np.float32)
    for v in range(1, 3):
        total += per_vote[v].astype(np.float32)              # NOT accumulate_votes on float16 arrays: that rounds after every vote
    if not amp:
        assert np.array_equal(total.view(np.uint32), E.accumulate_votes(ret, 3).view(np.uint32))
    assert set(dev) == {"predictions", "scores"} and len(dev["predictions"]) == 1
    assert dev["scores"][0].dtype == np.float32 and np.array_equal(dev["scores"][0].view(np.uint32), total.view(np.uint32))
    assert dev["predictions"][0].dtype == np.uint32 and np.array_equal(dev["predictions"][0], E.vote_payload(total, "semantickitti"))
    assert np.array_equal(top3["scores"][0], np.sort(total, 1)[:, ::-1][:, :3])
    if not amp:
        host = E.evaluate(model, [dict(batch)], 20, tta_votes=3)
        assert np.array_equal(host["predictions"][0], dev["predictions"][0])
        with pytest.raises(ValueError, match="votes"):
            E.evaluate(model, [dict(batch)], 20, tta_votes=4, on_device=True)


def test_a_cell_without_a_voxel_row_raises_at_the_read():
    """the stated difference from the host path, on run_points itself: the query's -1 is an IndexError, not the scene's last row"""
    tail = _tail()
    vox = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32, device="cuda")
    pts = torch.tensor([[1, 0, 0, 0], [5, 5, 5, 0], [0, 0, 0, 1]], dtype=torch.int64, device="cuda")
    logits = torch.zeros((3, 20), device="cuda")
    logits[1, 4] = logits[2, 6] = 1.0
    assert tail.run_points(logits, vox, pts, torch.tensor([2, 2, 3], device="cuda"), torch.tensor([2, 1]), ["a", "b"]) is tail
    assert int(tail.hist[2, 4]) == int(tail.hist[3, 6]) == int(tail.hist.sum()) - 1 == 1
    with pytest.raises(IndexError, match="no voxel row"):
        tail.read()
