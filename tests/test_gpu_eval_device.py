"""Evaluation on the device (-m gpu): csrc/evaltail.hip ts_eval_rows / ts_eval_confusion / ts_eval_votes through backend.eval_*,
the two segmentors' `device_tail` keyword and pcseg.eval.evaluate(on_device=True).

The kernels are compared with a numpy restatement of their semantics written here (include/taseg_hip.h: kept points, m_s,
fast_hist's label mask, the float32 vote sum in vote order).  Every comparison is exact: integers are integers, and the float32
sums are formed in one fixed order, so their bits are numpy's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from taseg_amd.data.synthetic import fill_parameters, make_model_cfg  # noqa: E402


# ------------------------------------------------------------------------------------------------ numpy restatement
def _scene_layout(vox_scene, pts_scene, n_scenes):
    cnt_v = np.bincount(vox_scene, minlength=n_scenes)
    return cnt_v, np.cumsum(cnt_v) - cnt_v, [np.flatnonzero(pts_scene == s) for s in range(n_scenes)]


def _kept(points, mask, num_points, s):
    p = points[s] if mask is None else points[s][mask[points[s]].astype(bool)]
    return p[:min(len(p), max(int(num_points[s]), 0))]


def ref_confusion(logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points, num_points_ms=None):
    """(hist [C, C] int64, pred of the kept rows scene-major with -1 where the inverse map is out of range, flags)"""
    n_scenes, C = len(num_points), logits.shape[1]
    cnt_v, start_v, points = _scene_layout(vox_scene, pts_scene, n_scenes)
    hist, preds, flags = np.zeros((C, C), np.int64), [], 0
    x = logits.astype(np.float32)
    for s in range(n_scenes):
        p = _kept(points, mask, num_points, s)
        local = inv[p]
        ok = (local >= 0) & (local < cnt_v[s])
        flags |= 4 if (~ok).any() else 0
        pred = np.full(len(p), -1, np.int64)
        pred[ok] = np.argmax(x[start_v[s] + local[ok]], axis=1) if ok.any() else 0
        preds.append(pred)
        l_idx = np.flatnonzero(lab_scene == s)
        if num_points_ms is not None and int(num_points_ms[s]) != len(points[s]):
            flags |= 32
        if min(len(l_idx), max(int(num_points[s]), 0)) != len(p):
            flags |= 8
            continue
        lab = labels[l_idx[:len(p)]].astype(np.int64)
        k = ok & (lab >= 0) & (lab < C)
        np.add.at(hist, (lab[k], pred[k]), 1)
    return hist, np.concatenate(preds), flags


def ref_votes(logits, vox_scene, pts_scene, inv, mask, num_points):
    """total [n, C] float32 = ((x_0 + x_1) + x_2) + ... in vote order"""
    V = len(num_points)
    cnt_v, start_v, points = _scene_layout(vox_scene, pts_scene, V)
    rows = [start_v[v] + inv[_kept(points, mask, num_points, v)] for v in range(V)]
    assert len({len(r) for r in rows}) == 1
    total = logits[rows[0]].astype(np.float32)
    for v in range(1, V):
        total += logits[rows[v]].astype(np.float32)
    return total


# ------------------------------------------------------------------------------------------------ inputs
def _coords(scene):
    """an [n, 4] int32 coordinate matrix whose last column is the scene index: the kernels read it with stride 4"""
    c = np.zeros((len(scene), 4), np.int32)
    c[:, -1] = scene
    return torch.from_numpy(c).cuda()[:, -1]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


VOX, PTS = (5, 1, 300), (255, 1, 514)      # scene boundaries inside a wave; 770 rows = four 256-row compaction blocks


def _confusion_inputs(C, dtype, seed=0):
    r = np.random.RandomState(seed)
    vox_scene = np.repeat(np.arange(3), VOX).astype(np.int32)
    pts_scene = np.repeat(np.arange(3), PTS).astype(np.int32)
    logits = r.randn(sum(VOX), C).astype(dtype)
    inv = np.concatenate([r.randint(0, v, p) for v, p in zip(VOX, PTS)]).astype(np.int64)
    first = PTS[0] + PTS[1]
    inv[first], inv[first + 1] = 10, 11                        # scene 2: its rows 10 / 11 are read for sure
    logits[VOX[0] + VOX[1] + 10, [1, C - 1]] = 50              # an exact tie: the first maximum wins
    logits[VOX[0] + VOX[1] + 11, C // 2] = np.nan              # a NaN wins
    return r, logits, vox_scene, pts_scene, inv


def _masks(r):
    n = sum(PTS)
    one_scene_off = np.ones(n, bool)
    one_scene_off[:PTS[0]] = False
    prefix = np.zeros(n, bool)
    prefix[:300] = True
    return {"none": None, "all": np.ones(n, bool), "scene0_off": one_scene_off, "prefix": prefix, "random": r.rand(n) < 0.6}


def _labels(r, kept_per_scene, C, dtype):
    lab_scene = np.repeat(np.arange(3), kept_per_scene).astype(np.int32)
    if dtype == np.uint8:
        labels = r.randint(0, C, len(lab_scene)).astype(np.uint8)
        labels[::7], labels[3::11] = 255, 0
    else:
        labels = r.randint(0, C, len(lab_scene)).astype(dtype)
        labels[::7], labels[3::11] = -1, C
    return labels, lab_scene


def _run_confusion(B, logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points, num_points_ms=None, hist=None, flags=None):
    C = logits.shape[1]
    hist = torch.zeros((C, C), dtype=torch.int64, device="cuda") if hist is None else hist
    flags = torch.zeros(1, dtype=torch.int32, device="cuda") if flags is None else flags
    pred = B.eval_confusion(_dev(logits), _coords(vox_scene), _coords(pts_scene), _dev(inv), _dev(labels), _coords(lab_scene),
                            torch.from_numpy(np.asarray(num_points, np.int64)).cuda(), hist, flags, point_mask=_dev(mask),
                            num_points_ms=None if num_points_ms is None else torch.tensor(num_points_ms).cuda(), want_pred=True)
    return hist, pred, flags


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("C", [20, 17, 3])
def test_confusion_equals_numpy(C, dtype):
    from taseg_amd import backend as B
    r, logits, vox_scene, pts_scene, inv = _confusion_inputs(C, dtype)
    seen = 0
    for mname, mask in _masks(r).items():
        kept = [int(PTS[s] if mask is None else mask[pts_scene == s].sum()) for s in range(3)]
        for shift in (-3, 0, 5):                                      # num_points below, equal to and above K_s
            num_points = [max(k + shift, 0) for k in kept]
            for ldtype in (np.uint8, np.int64, np.int32):
                labels, lab_scene = _labels(r, kept, C, ldtype)
                want, want_pred, want_flags = ref_confusion(logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points)
                assert want_flags == 0
                hist, pred, flags = _run_confusion(B, logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points)
                assert np.array_equal(hist.cpu().numpy(), want), (mname, shift, ldtype)
                assert np.array_equal(pred.cpu().numpy()[:len(want_pred)], want_pred) and int(flags) == 0
                seen += int(want.sum())
                # the call adds and never clears: a second call on the same matrix doubles it; a fresh run gives the same bits
                _run_confusion(B, logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points, hist=hist, flags=flags)
                assert np.array_equal(hist.cpu().numpy(), 2 * want) and int(flags) == 0
                again, _, _ = _run_confusion(B, logits, vox_scene, pts_scene, inv, mask, labels, lab_scene, num_points)
                assert np.array_equal(again.cpu().numpy(), want)
    assert seen > 10000          # (the cases are not empty)
    tie, nan = sum(PTS[:2]), sum(PTS[:2]) + 1
    _, want_pred, _ = ref_confusion(logits, vox_scene, pts_scene, inv, None, *_labels(r, PTS, C, np.int64), PTS)
    assert want_pred[tie] == 1 and want_pred[nan] == C // 2


def _vote_inputs(V, C, dtype, seed=1):
    r = np.random.RandomState(seed)
    pts = [300 + d for d in (0, -20, 10, -5, 25, -30, 15, 5, -10, 20)][:V]
    vox = [40 + 3 * v for v in range(V)]
    vox_scene = np.repeat(np.arange(V), vox).astype(np.int32)
    pts_scene = np.repeat(np.arange(V), pts).astype(np.int32)
    logits = r.randn(sum(vox), C).astype(dtype)
    inv = np.concatenate([r.randint(0, v, p) for v, p in zip(vox, pts)]).astype(np.int64)
    return r, logits, vox_scene, pts_scene, inv, pts


def _plant(logits, vox_scene, pts_scene, inv, mask, num_points, C):
    """kept point 3 of the scan: an exact tie of the sums (columns 3 and 9 hold 4.0 in every vote, the rest less); a NaN in vote 0
    for the first kept point on another voxel - returns that point"""
    V = len(num_points)
    cnt_v, start_v, points = _scene_layout(vox_scene, pts_scene, V)
    for v in range(V):
        p = _kept(points, mask, num_points, v)
        logits[start_v[v] + inv[p[3]]] = -1.0
        logits[start_v[v] + inv[p[3]], [3, 9]] = 4.0
    p = _kept(points, mask, num_points, 0)
    j = int(np.flatnonzero(inv[p] != inv[p[3]])[0])
    logits[start_v[0] + inv[p[j]], 2] = np.nan
    return j


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("C", [20, 17])
@pytest.mark.parametrize("V", [1, 3, 10])
def test_votes_equal_the_sequential_float32_sum(V, C, dtype):
    from taseg_amd import backend as B
    n = 257                                                    # one more than a block
    for form in ("mask", "num_points"):
        r, logits, vox_scene, pts_scene, inv, pts = _vote_inputs(V, C, dtype)
        if form == "mask":
            mask = np.zeros(len(pts_scene), bool)
            at = 0
            for p in pts:
                mask[at + r.choice(p, n, replace=False)] = True
                at += p
            num_points = [1000] * V
        else:
            mask, num_points = None, [n] * V
        nan_at = _plant(logits, vox_scene, pts_scene, inv, mask, num_points, C)
        total = ref_votes(logits, vox_scene, pts_scene, inv, mask, num_points)
        assert total.shape == (n, C) and total.dtype == np.float32
        want_label = np.argmax(total, axis=1)
        assert want_label[3] == 3 and total[3, 3] == total[3, 9] == 4.0 * V
        clean = ~np.isnan(total).any(1)
        assert not clean[nan_at] and clean[3] and want_label[nan_at] == 2
        for label_bytes in (4, 1):
            flags = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = B.eval_votes(_dev(logits), _coords(vox_scene), _coords(pts_scene), _dev(inv), torch.tensor(num_points).cuda(), flags,
                               point_mask=_dev(mask), label_bytes=label_bytes, want_sums=True, want_top3=True)
            assert int(flags) == 0 and int(got["n"]) == n and got["label"].shape[0] == len(pts_scene) // V >= n
            label = got["label"].cpu().numpy()[:n]
            assert label.dtype == (np.uint8 if label_bytes == 1 else np.int32) and np.array_equal(label.astype(np.int64), want_label)
            sums = got["sums"].cpu().numpy()[:n]
            assert sums.dtype == np.float32 and np.array_equal(sums.view(np.uint32), total.view(np.uint32))      # bit-equal
            top3 = got["top3"].cpu().numpy()[:n]
            assert np.array_equal(top3[clean], np.sort(total, 1)[:, ::-1][:, :3][clean])
        # without the optional outputs: the same labels
        got = B.eval_votes(_dev(logits), _coords(vox_scene), _coords(pts_scene), _dev(inv), torch.tensor(num_points).cuda(), flags,
                           point_mask=_dev(mask))
        assert got["sums"] is None and got["top3"] is None and np.array_equal(got["label"].cpu().numpy()[:n], want_label)


def test_flags_and_argument_checks():
    from taseg_amd import backend as B
    C = 20
    r, logits, vox_scene, pts_scene, inv = _confusion_inputs(C, np.float32)
    labels, lab_scene = _labels(r, PTS, C, np.int64)
    # bit 2: one inverse map entry outside its scene; every other row as expected
    bad_inv = inv.copy()
    bad_inv[100] = VOX[0]
    want, want_pred, want_flags = ref_confusion(logits, vox_scene, pts_scene, bad_inv, None, labels, lab_scene, PTS)
    hist, pred, flags = _run_confusion(B, logits, vox_scene, pts_scene, bad_inv, None, labels, lab_scene, PTS)
    ok = want_pred >= 0
    assert want_flags == 4 and int(flags) == 4 and (~ok).sum() == 1
    assert np.array_equal(hist.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy()[ok], want_pred[ok])
    mask = np.ones(len(inv), bool)
    hist, pred, flags = _run_confusion(B, logits, vox_scene, pts_scene, bad_inv, mask, labels, lab_scene, PTS)
    assert int(flags) == 4 and np.array_equal(hist.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy()[ok], want_pred[ok])
    # bit 3: scene 1 has three labels for its one point (num_points 5): it contributes nothing, the others do
    labels3, lab_scene3 = _labels(r, (PTS[0], 3, PTS[2]), C, np.int64)
    num_points = [PTS[0], 5, PTS[2]]
    want, _, want_flags = ref_confusion(logits, vox_scene, pts_scene, inv, None, labels3, lab_scene3, num_points)
    hist, _, flags = _run_confusion(B, logits, vox_scene, pts_scene, inv, None, labels3, lab_scene3, num_points)
    assert want_flags == 8 and int(flags) == 8 and np.array_equal(hist.cpu().numpy(), want) and want.sum() > 0
    # bit 5: num_points_ms against the points per scene; flags are OR-ed into what the caller's int holds
    want, _, want_flags = ref_confusion(logits, vox_scene, pts_scene, inv, None, labels, lab_scene, PTS, num_points_ms=[255, 2, 514])
    held = torch.full((1,), 64, dtype=torch.int32, device="cuda")
    hist, _, flags = _run_confusion(B, logits, vox_scene, pts_scene, inv, None, labels, lab_scene, PTS, num_points_ms=[255, 2, 514], flags=held)
    assert want_flags == 32 and int(flags) == 64 | 32 and np.array_equal(hist.cpu().numpy(), want)
    _, _, flags = _run_confusion(B, logits, vox_scene, pts_scene, inv, None, labels, lab_scene, PTS, num_points_ms=list(PTS))
    assert int(flags) == 0
    # bit 1 (ts_scene_counts'): a point array that is not grouped by scene
    swapped = pts_scene.copy()
    swapped[0], swapped[-1] = 2, 0
    _, _, flags = _run_confusion(B, logits, vox_scene, swapped, np.zeros_like(inv), None, labels, lab_scene, PTS)
    assert int(flags) & 2
    # bit 4: votes of unequal m_s leave every output as it was
    V = 3
    r, vl, vvs, vps, vinv, pts = _vote_inputs(V, C, np.float32)
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (_dev(vl), _coords(vvs), _coords(vps), _dev(vinv))
    out = B.eval_votes(*args, torch.tensor([270] * V).cuda(), flags, want_sums=True, want_top3=True)
    assert int(flags) == 0 and int(out["n"]) == 270
    out["label"].fill_(-7), out["sums"].fill_(-7.0), out["top3"].fill_(-7.0), out["n"].fill_(-7)
    again = B.eval_votes(*args, torch.tensor([270, 269, 270]).cuda(), flags, want_sums=True, want_top3=True, out=out)
    assert again is out and int(flags) == 16
    assert all(bool((out[k] == -7).all()) for k in ("label", "sums", "top3", "n"))
    # the wrapper's own checks
    many = np.arange(65, dtype=np.int32)
    with pytest.raises(ValueError, match="64 scenes"):
        B.eval_votes(_dev(np.zeros((65, C), np.float32)), _coords(many), _coords(many), _dev(np.zeros(65, np.int64)),
                     torch.ones(65, dtype=torch.int64).cuda(), flags)
    with pytest.raises(ValueError, match="64 scenes"):
        _run_confusion(B, np.zeros((65, C), np.float32), many, many, np.zeros(65, np.int64), None, np.zeros(65, np.int64), many, [1] * 65)
    with pytest.raises(ValueError, match="float32 or float16"):
        B.eval_votes(_dev(vl).double(), *args[1:], torch.tensor([270] * V).cuda(), flags)
    with pytest.raises(ValueError, match="uint8, int32 or int64"):
        _run_confusion(B, logits, vox_scene, pts_scene, inv, None, labels.astype(np.int16), lab_scene, PTS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_votes(_dev(vl).cpu(), *args[1:], torch.tensor([270] * V).cuda(), flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.eval_confusion(*args, _dev(labels), _coords(lab_scene), torch.tensor(PTS), torch.zeros((C, C), dtype=torch.int64), flags)
    # zero points is a valid call (with and without a mask)
    none32, none64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
    for mask in (None, np.zeros(0, bool)):
        hist, pred, flags = _run_confusion(B, np.zeros((0, C), np.float32), none32, none32, none64, mask, none64, none32, [0, 0])
        assert int(flags) == 0 and int(hist.sum()) == 0 and pred.shape[0] == 0
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = B.eval_votes(_dev(np.zeros((0, C), np.float32)), _coords(none32), _coords(none32), _dev(none64), torch.tensor([0, 0]).cuda(),
                           flags, point_mask=_dev(mask), want_sums=True)
        assert int(flags) == 0 and int(got["n"]) == 0 and got["label"].shape[0] == 0


# ------------------------------------------------------------------------------------------------ model level
MODELS = [("MinkUNet", 4), ("MinkUNetMs", 5)]


@pytest.fixture(scope="module")
def models():
    from taseg_amd.pcseg.model import build_network
    return {name: fill_parameters(build_network(make_model_cfg(name, in_dim=in_dim, cr=0.5, num_layer=[1] * 8), 20), seed=3).cuda().eval()
            for name, in_dim in MODELS}


def _batch(g, prefix):
    from test_gpu_parity_r2 import _eval_batch
    return _eval_batch(g, prefix)


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_validation_on_device_gives_the_host_matrix(g_eval_ms, models, name):
    from taseg_amd.pcseg import eval as E
    model = models[name].train()
    host = E.evaluate(model, (_batch(g_eval_ms, "batch_") for _ in range(2)), 20)
    dev = E.evaluate(model, (_batch(g_eval_ms, "batch_") for _ in range(2)), 20, on_device=True)
    assert model.training                                      # the caller's mode is restored
    model.eval()
    assert dev["hist"].shape == (19, 19) and dev["hist"].dtype == host["hist"].dtype and host["hist"].sum() > 1000
    assert np.array_equal(dev["hist"], host["hist"]) and dev["miou"] == host["miou"] and np.array_equal(dev["iou"], host["iou"])
    dev = E.evaluate(model, (_batch(g_eval_ms, "batch_") for _ in range(2)), 20, on_device=True, prefetch=False)
    assert np.array_equal(dev["hist"], host["hist"]) and not model.training


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_tta_on_device_gives_the_host_payload_and_sums(g_eval_ms, models, name):
    from taseg_amd.pcseg import eval as E
    model, g = models[name], g_eval_ms
    votes = int(g["votes"])
    batches = lambda: (_batch(g, "tta_") for _ in range(2))  # noqa: E731
    host = E.evaluate(model, batches(), 20, tta_votes=votes)
    dev = E.evaluate(model, batches(), 20, tta_votes=votes, on_device=True)
    assert set(dev) == {"predictions"} and len(dev["predictions"]) == 2
    for a, b in zip(dev["predictions"], host["predictions"]):
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape and a.shape[1] == 1 and np.array_equal(a, b)
    with torch.no_grad():
        total = E.accumulate_votes(model(_batch(g, "tta_")), votes)
    everything = E.evaluate(model, batches(), 20, tta_votes=votes, on_device=True, scores="all")
    assert np.array_equal(everything["predictions"][1], host["predictions"][1])
    assert everything["scores"][0].dtype == np.float32 and np.array_equal(everything["scores"][0].view(np.uint32), total.view(np.uint32))
    assert np.array_equal(everything["scores"][0], everything["scores"][1])
    top3 = E.evaluate(model, batches(), 20, tta_votes=votes, on_device=True, scores="top3")["scores"][0]
    assert np.array_equal(top3, np.sort(total, 1)[:, ::-1][:, :3])
    nus = E.evaluate(model, batches(), 20, tta_votes=votes, on_device=True, dataset="nuscenes") if (host["predictions"][0] != 0).all() else None
    if nus is not None:
        assert nus["predictions"][0].dtype == np.uint8 and np.array_equal(nus["predictions"][0], E.vote_payload(total, "nuscenes"))
    with pytest.raises(ValueError, match="votes"):
        E.evaluate(model, batches(), 20, tta_votes=votes + 1, on_device=True)


def test_tta_under_autocast_sums_the_half_votes_in_float32(g_eval_ms, models):
    from taseg_amd.pcseg import eval as E
    model, g = models["MinkUNetMs"], g_eval_ms
    votes = int(g["votes"])
    with torch.autocast("cuda", dtype=torch.float16):
        with torch.no_grad():
            per_vote = model(_batch(g, "tta_"))["point_predict_logits"]
        dev = E.evaluate(model, [_batch(g, "tta_")], 20, tta_votes=votes, on_device=True, scores="all")
    assert per_vote[0].dtype == np.float16
    total = per_vote[0].astype(np.float32)
    for v in range(1, votes):
        total += per_vote[v].astype(np.float32)              # NOT accumulate_votes on float16 arrays: that rounds after every vote
    assert np.array_equal(dev["scores"][0].view(np.uint32), total.view(np.uint32))
    assert np.array_equal(dev["predictions"][0][:, 0], np.argmax(total, 1))


def test_a_segmentor_without_the_keyword_is_refused(models):
    from taseg_amd.pcseg import eval as E

    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, batch_dict, defer=False):
            raise AssertionError("not reached")
    with pytest.raises(ValueError, match="on_device=False"):
        E.evaluate(Plain().cuda(), [], 20, on_device=True)
    with pytest.raises(ValueError, match="scores"):
        E.evaluate(models["MinkUNet"], [], 20, scores="all")
