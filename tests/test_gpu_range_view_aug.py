"""The range-view training stage on the GPU (csrc/range_view.hip: ts_rv_augment, ts_rv_label_counts, ts_rv_compose behind
taseg_amd.data.range_view.build_range_view_train_batch): every output equals the numpy restatement of tests/range_view_aug_ref.py BIT
FOR BIT, with no exclusions - on hand-made clouds and images and on the cases of the reference fixture (tests/golden/
range_view_aug.npz; tests/test_range_view_aug_host.py compares that restatement with the reference's own output) - and the reference's
recorded images outside the pixels an undecided row may touch.  Two calls give the same bits; SalsaNext takes a training step on a
recipe batch."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import range_view_aug_ref as A  # noqa: E402
import range_view_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = A.fixture_cases()


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "range_view_aug.npz"), allow_pickle=False))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- rv_augment
LENS = (257, 1000)                                                     # 257 crosses one compaction block of 256
DRAWS = {"flip1": {"flip": 1}, "flip2": {"flip": 2}, "flip3": {"flip": 3}, "flip0": {"flip": 0}, "scale": {"scale": 1.0371},
         "scale_const": {"scale": 1 / 1.05}, "rotate": {"rotate": (float(np.cos(2.1)), float(np.sin(2.1)))},
         "rotate_45": {"rotate": (float(np.cos(np.pi / 4)), float(np.sin(np.pi / 4)))},
         "jitter": {"jitter": np.array([0.3, -0.017, 0.2999])},
         "all": {"flip": 3, "scale": 1.0123, "rotate": (float(np.cos(5.0)), float(np.sin(5.0))), "jitter": np.array([-0.3, 0.1, 0.05])}}


def _clouds():
    clouds = [R.synth_cloud(70 + i, n) for i, n in enumerate(LENS)]
    clouds[1][:50, 1] = clouds[1][:50, 0]                              # 45 degrees of azimuth: x c and y s cancel under rotate_45
    labels = [np.random.RandomState(80 + i).randint(0, 20, n).astype(np.int32) for i, n in enumerate(LENS)]
    return clouds, labels


def _run_augment(clouds, labels, draws):
    """rv_augment on the clouds under one draw dict per cloud; returns the device's outputs and the restatement's"""
    from taseg_amd import backend as B
    from taseg_amd.data.range_view import aug_record
    lens = [len(c) for c in clouds]
    nc = len(clouds)
    feat = torch.from_numpy(np.concatenate(clouds)).cuda()
    label = torch.from_numpy(np.concatenate(labels)).cuda()
    before = feat.clone()
    batch = torch.from_numpy(np.repeat(np.arange(nc, dtype=np.int32), lens)).cuda()
    first = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)).cuda()
    params = torch.from_numpy(np.stack([aug_record(d) for d in draws])).cuda()
    drop = off = None
    if any(d.get("drop") is not None for d in draws):
        lists = [np.asarray(d["drop"], dtype=np.int32) if d.get("drop") is not None else np.zeros(0, dtype=np.int32) for d in draws]
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)).cuda()
        drop = torch.from_numpy(np.concatenate(lists)).cuda()
    out, out_label, out_batch, counts, err = B.rv_augment(feat, batch, first, nc, params, label=label, drop=drop, drop_off=off)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), feat.view(torch.int32))          # the resident rows are never written
    want = [A.augment_cloud(c, l, d) for c, l, d in zip(clouds, labels, draws)]
    kept = [len(w[0]) for w in want]
    m = sum(kept)
    assert counts.cpu().tolist() == kept
    assert np.array_equal(_bits(out[:m].cpu().numpy()), _bits(np.concatenate([w[0] for w in want])))
    assert np.array_equal(out_label[:m].cpu().numpy(), np.concatenate([w[1] for w in want]))
    assert np.array_equal(out_batch[:m].cpu().numpy(), np.repeat(np.arange(nc, dtype=np.int32), kept))
    return out[:m].cpu().numpy(), int(err)


@pytest.mark.parametrize("name", list(DRAWS))
def test_augment_steps_equal_the_restatement(name):
    clouds, labels = _clouds()
    other = {"scale": 1.0499} if name != "scale" else {"flip": 2}
    _, err = _run_augment(clouds, labels, [DRAWS[name], other])
    assert err == 0
    _, err = _run_augment(clouds, labels, [other, DRAWS[name]])
    assert err == 0


def test_augment_with_drop_lists():
    clouds, labels = _clouds()
    # cloud 0: its row 0 and its last row; cloud 1: rows 255 .. 510 = the whole block of global rows 512 .. 767, row 0 and the last
    d0 = np.array([0, 100, 256], dtype=np.int64)
    d1 = np.unique(np.concatenate([[0], np.arange(255, 511), [999]])).astype(np.int64)
    out, err = _run_augment(clouds, labels, [dict(DRAWS["all"], drop=d0), dict(DRAWS["rotate"], drop=d1)])
    assert err == 0 and len(out) == 257 - 3 + 1000 - 258
    # only drop, one cloud with an empty list; both lists empty
    out, err = _run_augment(clouds, labels, [{"drop": np.zeros(0, dtype=np.int64)}, {"drop": d1}])
    assert err == 0 and np.array_equal(_bits(out[:257]), _bits(clouds[0]))
    out, err = _run_augment(clouds, labels, [{"drop": np.zeros(0, dtype=np.int64)}, {"drop": np.zeros(0, dtype=np.int64)}])
    assert err == 0 and np.array_equal(_bits(out), _bits(np.concatenate(clouds)))


def test_augment_record_without_bits_returns_the_input_bits():
    clouds, labels = _clouds()
    clouds[0][:4, :3] = np.array([[-0.0, 0.0, -0.0], [np.inf, 1, 2], [1e-42, -1e-42, 3], [np.nan, 0, 0]], dtype=np.float32)
    out, err = _run_augment(clouds, labels, [{}, {}])
    assert err == 0 and np.array_equal(_bits(out), _bits(np.concatenate(clouds)))


def test_augment_ignores_and_flags_a_drop_index_outside_its_cloud():
    clouds, labels = _clouds()
    inside = np.array([3, 256], dtype=np.int64)
    out, err = _run_augment(clouds, labels, [{"drop": np.array([3, 256, 257, 900], dtype=np.int64)}, {"drop": np.array([-1, 1000], dtype=np.int64)}])
    assert err == A.ERR_DROP
    want, _ = A.augment_cloud(clouds[0], None, {"drop": inside})
    assert np.array_equal(_bits(out[:255]), _bits(want)) and np.array_equal(_bits(out[255:]), _bits(clouds[1]))


# ---------------------------------------------------------------------------------------- rv_label_counts + rv_compose
def _images(seed, b, h, w):
    """b hand-made images: random values, a random mask channel of zeros and ones OVER real values, labels 0, 1, 9 .. 19 at random
    and, per image, class 2 on exactly 20 pixels, class 3 on 21, class 4 on none (all three are paste classes; 9 is not)"""
    rng = np.random.RandomState(seed)
    scan = rng.uniform(-1, 1, (b, 6, h, w)).astype(np.float32)
    scan[:, 5] = (rng.uniform(size=(b, h, w)) < 0.6).astype(np.float32)
    label = rng.choice([0, 1, 9, 10, 13, 14, 15, 17], size=(b, 1, h, w)).astype(np.int64)
    for i in range(b):
        at = rng.choice(h * w, 41, replace=False)
        label[i].reshape(-1)[at[:20]] = 2
        label[i].reshape(-1)[at[20:]] = 3
    return scan, label


def _compose(scan_a, label_a, scan_b, label_b, params):
    from taseg_amd import backend as B
    from taseg_amd.data.range_view import compose_record
    _, _, h, w = scan_a.shape
    rec = torch.from_numpy(np.stack([compose_record(p, h, w) for p in params])).cuda()
    ta, tla = torch.from_numpy(scan_a).cuda(), torch.from_numpy(label_a).cuda()
    if scan_b is None:
        got = B.rv_compose(ta, tla, rec)
    else:
        tb, tlb = torch.from_numpy(scan_b).cuda(), torch.from_numpy(label_b).cuda()
        counts = B.rv_label_counts(tlb)
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), A.label_counts(label_b))
        got = B.rv_compose(ta, tla, rec, tb, tlb, counts)
    want = A.compose(scan_a, label_a, scan_b, label_b, params)
    assert got[1].dtype == torch.int64 and got[0].shape == scan_a.shape and got[1].shape == label_a.shape
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1])
    return want


@pytest.mark.parametrize("hw", [(7, 203), (64, 512)])
def test_compose_equals_the_restatement(hw):
    h, w = hw
    scan_a, label_a = _images(1, 2, h, w)
    scan_b, label_b = _images(2, 2, h, w)
    counts = A.label_counts(label_b)
    assert (counts[:, 2] == 20).all() and (counts[:, 3] == 21).all() and (counts[:, 4] == 0).all() and (counts[:, 9] > 21).all()
    none = {"shift": 0, "partner_shift": 0, "strategy": None, "mixture": 0, "paste": False, "union": False}
    # every strategy, both mixtures, with and without the shifts
    for k, name in enumerate(A.strategy_names()):
        shifts = ((0, 0), (100, w - 100), (w - 100, 0), (0, 100))[k % 4]
        for m0, m1 in ((1, 2), (2, 1)):
            _compose(scan_a, label_a, scan_b, label_b, [dict(none, strategy=name, mixture=m0, shift=shifts[0], partner_shift=shifts[1]),
                                                        dict(none, strategy=name, mixture=m1, shift=shifts[1], partner_shift=shifts[0])])
    # the shift alone, different for primary and partner, with and without partner images
    _compose(scan_a, label_a, None, None, [dict(none, shift=100), dict(none, shift=w - 100)])
    want = _compose(scan_a, label_a, scan_b, label_b, [dict(none, shift=w - 100, partner_shift=100), none])
    assert np.array_equal(_bits(want[0][1]), _bits(scan_a[1]))
    # paste: 20 pixels stay, 21 go over, class 9 is not in the set
    want = _compose(scan_a, label_a, scan_b, label_b, [dict(none, paste=True), dict(none, paste=True, partner_shift=100, shift=w - 100)])
    took = (want[1][0, 0] != label_a[0, 0]) | (_bits(want[0][0]) != _bits(scan_a[0])).any(0)
    assert took[label_b[0, 0] == 3].sum() == 21 and not took[label_b[0, 0] != 3].any()
    # union: a pixel whose mask is 0 takes the partner although its values are real; after mix and paste
    want = _compose(scan_a, label_a, scan_b, label_b, [dict(none, union=True), dict(none, union=True, shift=100)])
    empty = scan_a[0, 5] == 0
    assert empty.any() and np.array_equal(_bits(want[0][0][:, empty]), _bits(scan_b[0][:, empty]))
    assert np.array_equal(_bits(want[0][0][:, ~empty]), _bits(scan_a[0][:, ~empty]))
    _compose(scan_a, label_a, scan_b, label_b, [dict(none, strategy="col3row4", mixture=2, paste=True, union=True, shift=100, partner_shift=0),
                                                dict(none, strategy="col6row4", mixture=1, paste=True, union=True, partner_shift=w - 100)])
    # nothing set: the primary, bit for bit
    want = _compose(scan_a, label_a, scan_b, label_b, [none, none])
    assert np.array_equal(_bits(want[0]), _bits(scan_a)) and np.array_equal(want[1], label_a)


# ------------------------------------------------------------------------------------- build_range_view_train_batch
def _aug(sw):
    from taseg_amd.data.range_view import RangeViewAug
    return RangeViewAug(*[bool(v) for v in sw[:5]], *[float(v) for v in sw[5:]])


def _scan_dicts(clouds, labels, which):
    return [{"points": torch.from_numpy(clouds[i]).cuda(), "labels": torch.from_numpy(labels[i]).cuda(), "name": "scan%d" % i}
            for i in which]


GROUPS = {"partners": [n for n, c in CASES.items() if c[3] == A.HW and (c[2][5] > 0 or c[2][7] > 0 or c[2][8] > 0)],
          "alone": [n for n, c in CASES.items() if c[3] == A.HW and not (c[2][5] > 0 or c[2][7] > 0 or c[2][8] > 0)],
          "wide": [n for n, c in CASES.items() if c[3] == A.HW_WIDE]}


@pytest.mark.parametrize("group", list(GROUPS))
def test_train_batch_on_the_fixture_cases(g, group):
    """the cases of one image size as ONE batch: the restatement's bits everywhere, the reference's outside the excluded pixels"""
    from taseg_amd.data.range_view import build_range_view_train_batch, draw_range_view_params
    names = GROUPS[group]
    assert names
    clouds, labels = A.fixture_scans(g)
    hw = CASES[names[0]][3]
    params = []
    for name in names:
        seed, index, sw, _ = CASES[name]
        params.append(draw_range_view_params(_aug(sw), index, len(clouds), lambda i: len(clouds[i]), np.random.RandomState(seed),
                                             random.Random(seed), hw))
    with_partners = group != "alone"
    assert all((p["partner"] is not None) == with_partners for p in params)
    resident = _scan_dicts(clouds, labels, range(len(clouds)))
    before = [s["points"].clone() for s in resident]
    scans = [resident[p["index"]] for p in params]
    partners = [resident[p["partner"]] for p in params] if with_partners else None
    got = build_range_view_train_batch(scans, partners, params, hw)
    again = build_range_view_train_batch(scans, partners, params, hw)
    assert int(got["range_view_err"]) == 0
    assert all(torch.equal(a.view(torch.int32), s["points"].view(torch.int32)) for a, s in zip(before, resident))
    for key in ("scan_rv", "label_rv", "mask_rv"):
        assert torch.equal(got[key], again[key]) and (key == "label_rv" or torch.equal(got[key].view(torch.int32), again[key].view(torch.int32)))
    b = len(names)
    assert got["scan_rv"].shape == (b, 6) + tuple(hw) and got["label_rv"].shape == (b, 1) + tuple(hw) and got["label_rv"].dtype == torch.int64
    assert got["mask_rv"].shape == (b, 1) + tuple(hw) and got["mask_rv"].data_ptr() == got["scan_rv"][:, 5:6].data_ptr()
    assert got["scan_name"] == ["scan%d" % p["index"] for p in params]
    scan, label = got["scan_rv"].cpu().numpy(), got["label_rv"].cpu().numpy()
    want_scan, want_label, aug, err = A.train_batch(clouds, labels, params, hw, with_partners=with_partners)
    assert err == 0
    assert np.array_equal(_bits(scan), _bits(want_scan)) and np.array_equal(label, want_label)
    excl = A.excluded_pixels(aug, params, hw[0], hw[1], with_partners)
    for i, name in enumerate(names):
        bad = A.differs_from_stored(g, name, scan[i], label[i])
        assert not (bad & ~excl[i]).any(), name


def test_salsanext_trains_on_a_recipe_batch(g, monkeypatch):
    from taseg_amd.data.range_view import RangeViewAug, build_range_view_train_batch, draw_range_view_params
    from taseg_amd.data.synthetic import fill_parameters, make_model_cfg
    from taseg_amd.pcseg.model.segmentor.range.salsanext.model.semantic.salsanext import SalsaNext
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    clouds, labels = A.fixture_scans(g)
    hw = (32, 256)
    rs, pyr = np.random.RandomState(11), random.Random(11)
    params = [draw_range_view_params(RangeViewAug.recipe(), i, len(clouds), lambda k: len(clouds[k]), rs, pyr, hw) for i in (0, 1)]
    resident = _scan_dicts(clouds, labels, range(len(clouds)))
    batch = build_range_view_train_batch([resident[p["index"]] for p in params], [resident[p["partner"]] for p in params], params, hw)
    assert int(batch["range_view_err"]) == 0 and int((batch["label_rv"] > 0).sum()) > 100
    runs = []
    for _ in range(2):
        cfg = make_model_cfg("SalsaNext", LOSS="dice", IF_LS_LOSS=True, IF_BD_LOSS=True, TOP_K_PERCENT_PIXELS=1.0)
        torch.manual_seed(0)
        model = fill_parameters(SalsaNext(cfg, 20), seed=3).cuda().train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        ret, tb, disp = model({"scan_rv": batch["scan_rv"], "label_rv": batch["label_rv"]})
        opt.zero_grad()
        ret["loss"].float().backward()
        opt.step()
        assert bool(torch.isfinite(ret["loss"]).all()) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
        runs.append((ret["loss"].detach().clone(), [p.detach().clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_refusals():
    from taseg_amd.data.range_view import RangeViewAug, build_range_view_train_batch, draw_range_view_params, mix_bounds
    rs, pyr = np.random.RandomState(1), random.Random(1)
    p = draw_range_view_params(RangeViewAug(), 0, 1, lambda i: 16, rs, pyr)
    cpu = {"points": torch.zeros(16, 4), "labels": torch.zeros(16, dtype=torch.int32), "name": "a"}
    dev = {"points": torch.ones(16, 4).cuda(), "labels": torch.zeros(16, dtype=torch.int32).cuda(), "name": "a"}
    with pytest.raises(RuntimeError, match="ROCm device"):
        build_range_view_train_batch([cpu], None, [p])
    with pytest.raises(RuntimeError, match="ROCm device"):
        build_range_view_train_batch([dev], [cpu], [p])
    with pytest.raises(ValueError, match="at most 64"):
        build_range_view_train_batch([dev] * 33, [dev] * 33, [p] * 33)
    with pytest.raises(ValueError, match="W >= 200"):
        draw_range_view_params(RangeViewAug(range_shift=0.9), 0, 1, lambda i: 16, rs, pyr, (64, 128))
    for name in ("cutmix", "cutout", "mixup"):
        with pytest.raises(ValueError, match="not defined"):
            mix_bounds(name, 64, 512)
        with pytest.raises(ValueError, match="not defined"):
            build_range_view_train_batch([dev], [dev], [dict(p, strategy=name, mixture=1)])
    got = build_range_view_train_batch([dev] * 32, [dev] * 32, [p] * 32, (8, 16))       # 64 clouds are taken
    assert got["scan_rv"].shape == (32, 6, 8, 16) and int(got["range_view_err"]) == 0
