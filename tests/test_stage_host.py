"""The data stage's shared host helpers on CPU tensors: the walks over scan dicts and sample dicts, both class-step rules and their
lookup, the default frame offsets, the bounded layout cache and the prefix mask (taseg_amd/data/stage.py, nuscenes.py)."""
import torch

from taseg_amd.data import nuscenes as N
from taseg_amd.data import stage as S

STEPS = [0, 1, 2, 5]          # never aggregated / from every scan / from some of the deltas below / from -5 alone


def _scan_dict(sizes, seed, cols=4, **extra):
    """a scan dict with len(sizes) - 1 history scans; every tensor is distinct, so identity tells which one was picked"""
    g = torch.Generator().manual_seed(seed)
    return dict(points=[torch.randn(n, cols, generator=g) for n in sizes],
                labels=[torch.randint(0, len(STEPS), (n,), generator=g) for n in sizes],
                poses=[torch.randn(4, 4, generator=g) for _ in sizes], **extra)


def test_walk_scans_lists_every_history_scan_once():
    pseudo = [torch.tensor([-1, 3, 3]), torch.tensor([2, 0])]
    clouds = [_scan_dict([4], 0, cols=5),                                        # no history
              _scan_dict([3, 2, 5], 1, deltas=[-5, -2], pseudo=pseudo),
              _scan_dict([2, 1, 3, 2], 2)]                                       # default deltas -3, -2, -1; no pseudo
    (pts, lab, ps, lengths, owner, pose0s, poses, rows), current = S._walk_scans(clouds, STEPS)
    assert lengths == [3, 2, 2, 1, 3] and owner == [1, 1, 2, 2, 2]
    want_pts = clouds[1]["points"][:2] + clouds[2]["points"][:3]
    assert all(p.shape[1] == 4 and torch.equal(p, w[:, :4]) for p, w in zip(pts, want_pts))
    assert all(a is b for a, b in zip(lab, clouds[1]["labels"][:2] + clouds[2]["labels"][:3]))
    assert all(a is b for a, b in zip(ps, pseudo + clouds[2]["labels"][:3]))    # pseudo where given, else the labels
    assert all(a is b for a, b in zip(pose0s, [clouds[1]["poses"][2]] * 2 + [clouds[2]["poses"][3]] * 3))
    assert all(a is b for a, b in zip(poses, clouds[1]["poses"][:2] + clouds[2]["poses"][:3]))
    assert [(first, count) for _, _, first, count in current] == [(0, 0), (0, 5), (5, 6)]
    for (cur, cur_lab, _, _), c in zip(current, clouds):
        assert cur is c["points"][-1] and cur_lab.dtype == torch.int64 and torch.equal(cur_lab, c["labels"][-1])
    assert current[0][0].shape[1] == 5                                           # the current scan keeps its columns
    # steps:           0      1      2      5     (pseudo class -1)
    assert rows == [[False, True, False, True, False],       # delta -5
                    [False, True, True, False, False],       # delta -2
                    [False, True, False, False, False],      # delta -3
                    [False, True, True, False, False],       # delta -2
                    [False, True, False, False, False]]      # delta -1


def _sample_dict(n_key, sweeps, seed):
    """a nuScenes sample dict with len(sweeps) selected sweeps; every tensor is distinct"""
    g = torch.Generator().manual_seed(seed)
    return dict(points=torch.randn(n_key, 5, generator=g), labels=torch.randint(0, len(STEPS), (n_key,), generator=g),
                hist_points=[torch.randn(n, 5, generator=g) for n in sweeps],
                hist_labels=[torch.randint(0, len(STEPS), (n,), generator=g) for n in sweeps],
                hist_pseudo=[torch.randint(0, len(STEPS), (n,), generator=g) for n in sweeps],
                params=torch.randn(len(sweeps), 28, generator=g, dtype=torch.float64))


def test_walk_sweeps_lists_every_sweep_once():
    clouds = [_sample_dict(4, [], 0),                                            # the first keyframe of its scene: no sweeps
              _sample_dict(3, [2, 5, 1], 1),
              _sample_dict(2, [3, 2], 2)]                                        # a partner: walked like a sample
    pts, lab, pseudo, lengths, owner, rows, params = N._walk_sweeps(clouds, STEPS)
    assert lengths == [2, 5, 1, 3, 2] and owner == [1, 1, 1, 2, 2]
    for got, key in ((pts, "hist_points"), (lab, "hist_labels"), (pseudo, "hist_pseudo")):
        want = clouds[1][key] + clouds[2][key]
        assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    # one row per sweep, by its position in ITS cloud: the partner's sweeps start at 0 again
    assert rows == [N._nusc_row(pos, STEPS) for pos in (0, 1, 2, 0, 1)]
    assert len(params) == 2 and params[0] is clouds[1]["params"] and params[1] is clouds[2]["params"]
    assert N._walk_sweeps(clouds[:1], STEPS) == ([],) * 7


def test_step_keep_against_a_loop():
    g = torch.Generator().manual_seed(3)
    for neg_last in (True, False):
        table = torch.rand(5, len(STEPS) + neg_last, generator=g) < 0.5
        assert table.any() and not table.all()
        scan = torch.randint(0, 5, (200,), generator=g, dtype=torch.int32)
        cls = torch.randint(-1 if neg_last else 0, len(STEPS), (200,), generator=g)
        assert not neg_last or (cls == -1).sum() > 10
        got = S._step_keep(table, scan, cls, neg_last=neg_last)
        want = [bool(table[int(s_), int(c) if c >= 0 else table.shape[1] - 1]) for s_, c in zip(scan, cls)]
        assert got.dtype == torch.bool and got.tolist() == want
        assert S._step_keep(table, scan.long(), cls, neg_last=neg_last).tolist() == want
        none = S._step_keep(table, scan[:0], cls[:0], neg_last=neg_last)
        assert none.dtype == torch.bool and none.shape == (0,)
    # the SemanticKITTI rows: class -1 is never kept, whatever the scan
    table = torch.tensor([S._kitti_row(d, STEPS) for d in (-5, -2)])
    assert S._step_keep(table, torch.tensor([0, 1, 0, 1]), torch.tensor([-1, -1, 3, 3]), neg_last=True).tolist() == [False, False, True, False]


def test_deltas_default_and_given():
    assert S._deltas(_scan_dict([2, 1, 3, 2], 0)) == [-3, -2, -1]
    assert S._deltas(_scan_dict([3, 2, 5], 1, deltas=[-5, -2])) == [-5, -2]
    assert S._deltas(_scan_dict([4], 2)) == [] and S._deltas(_scan_dict([4], 2, deltas=None)) == []


def test_nuscenes_rows_by_sweep_position():
    # steps:                                          0      1      2      5
    assert [N._nusc_row(pos, STEPS) for pos in range(4)] == [[False, True, False, False],     # (pos + 1) = 1
                                                            [False, True, True, False],      # 2
                                                            [False, True, False, False],     # 3
                                                            [False, True, True, False]]      # 4
    assert N._nusc_row(4, STEPS) == [False, True, False, True]
    assert N._layout([2, 1, 3, 1], STEPS, "cpu")[1].tolist() == [N._nusc_row(pos, STEPS) for pos in range(4)]


def test_layout_cache_is_bounded_and_returns_the_same_tensors():
    S._cache.clear()
    layouts = [[1, k + 1, 2] for k in range(70)]
    for lengths in layouts:
        i64, i32 = S.rows_index(lengths, "cpu"), S.rows_index32(lengths, "cpu")
        assert len(S._cache) <= 64
        assert i64.dtype == torch.int64 and i32.dtype == torch.int32
        assert S.rows_index(lengths, "cpu") is i64 and S.rows_index32(lengths, "cpu") is i32
    want = torch.tensor([0] + [1] * 70 + [2, 2])
    assert torch.equal(i64, want) and torch.equal(i32, want.int())
    # 140 entries went in: the first layouts are long gone, and come back with the same contents
    assert not any(tuple(layouts[0]) in key for key in S._cache if isinstance(key, tuple))
    assert S.rows_index(layouts[0], "cpu").tolist() == [0, 1, 2, 2]
    assert S.rows_index32(layouts[0], "cpu").tolist() == [0, 1, 2, 2] and len(S._cache) <= 64


def test_prefix_mask():
    mask = S._prefix_mask([2, 0, 3], [4, 1, 3], "cpu")
    assert mask.dtype == torch.bool and mask.tolist() == [True, True, False, False, False, True, True, True]
    assert S._prefix_mask([2], [5], "cpu").tolist() == [True, True, False, False, False]
    assert S._prefix_mask([3], [3], "cpu").tolist() == [True, True, True]
