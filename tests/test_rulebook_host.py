"""tests/rulebook_ref.py on the CPU: the table model pinned on hand-computed values, the adversarial inputs of
tests/test_gpu_rulebook_edges.py shown to have the property they are named for, broken models and broken references shown to
answer differently on them (so a kernel with that flaw would fail the GPU test), and the plain references shown to agree with
oracle/ts_oracle.py wherever that states the rule.  `pytest -s` prints the chain lengths."""
import numpy as np
import pytest

import rulebook_ref as R
from oracle import ts_oracle as O


# --------------------------------------------------------------------------- pinned values
def test_slot0_and_capacity_pinned():
    """by hand: 1 * G = 0x9E3779B97F4A7C15, high half 0x9E3779B9, & 1023 = 0x1B9; 2 * G mod 2^64 = 0x3C6EF372FE94F82A, high half
    0x3C6EF372, & 1023 = 0x372; 2^32 * G mod 2^64 = 0x7F4A7C1500000000, high half 0x7F4A7C15, & 2047 = 0x415.  Capacity: the
    first power of two >= 2 n + 2 and >= 1024: 2 * 511 + 2 = 1024 fits, 2 * 512 + 2 = 1026 does not."""
    assert R.slot0(1, 1023) == 0x1B9 and R.slot0(2, 1023) == 0x372 and R.slot0(1 << 32, 2047) == 0x415
    assert R.slot0(0, 1023) == 0
    assert R.slot0_np(np.array([1, 2, 1 << 32, -2], np.int64), 1023).tolist() == [0x1B9, 0x372, 0x015, R.slot0(-2, 1023)]
    assert R.capacity(0) == 1024 and R.capacity(511) == 1024 and R.capacity(512) == 2048 and R.capacity(1023) == 2048
    assert R.capacity(1024) == 4096


def test_the_box_holds_264_tail_coordinates_and_no_hash_collision():
    box = R._box(0)
    assert len(box) == 64000
    slots = R.slot0_np(R.coord_keys(box), 1023)
    assert int((slots > 1023 - R.TAIL_SLOTS).sum()) == 264
    assert R.no_hash_collisions(box)
    keys = R._random_keys(100)
    assert keys.min() >= 0 and keys.max() < 1 << 59
    assert 300 <= int((R.slot0_np(keys, 1023) == 1023).sum()) <= 500          # "about 400"


# --------------------------------------------------------------------------- chain shape
def _chain_holds(name, keys, probes):
    """the chain runs across the end of the table, some key sits >= 64 slots from its first slot, and every probe is absent,
    starts inside the chain and walks through the wrap before it meets an empty slot"""
    st = R.chain_stats(keys)
    t = st["table"]
    assert st["run"] is not None, name
    first, last = st["run"]
    assert st["longest"] >= 64, (name, st["longest"])
    walks = []
    for p in probes:
        w = t.miss_walk(p)
        assert t.find(p) == -1 and t.keys[w[0]] != R.EMPTY and t.keys[w[-1]] == R.EMPTY
        assert w[0] >= first and t.mask in w and 0 in w and w[-1] == last + 1, (name, w[0], w[-1])
        walks.append(len(w))
    print(f"chain {name}: keys {len(keys)} slots {t.mask + 1} run {first}..{t.mask},0..{last} longest displacement "
          f"{st['longest']} miss walks {min(walks) if walks else 0}..{max(walks) if walks else 0}")
    return st


@pytest.mark.parametrize("name", R.QUERY_CASES)
def test_query_cases_form_a_chain_across_the_end(name):
    refs, ref_idx, queries = R.query_case(name)
    assert R.capacity(len(refs)) == {"n512": 2048}.get(name, 1024)
    want = R.query_ref(queries, refs, ref_idx)
    mask = R.capacity(len(refs)) - 1
    assert (R.slot0_np(refs[refs != -1], mask) > mask - R.TAIL_SLOTS).all()
    if name == "n1":                      # one key: a hit in the last slots, no chain to speak of
        assert (want >= 0).sum() == 1
        return
    misses = queries[(want < 0) & (queries != -1)]
    first = R.chain_stats(refs)["run"][0]
    into = [q for q in misses if R.slot0(q, mask) >= first]
    assert len(into) >= 50 and len(misses) - len(into) >= 50            # misses that start before the wrap, and misses elsewhere
    _chain_holds(name, refs, into)
    assert (want >= 0).sum() == (refs != -1).sum()
    # the model, being a correct table, agrees with the value-keyed reference (positions; ref_idx applied on top)
    pos = R.model_query(queries, refs)
    assert np.array_equal(np.where(pos >= 0, pos if ref_idx is None else ref_idx[pos], -1), want)


@pytest.mark.parametrize("n", R.COLLISION_ROWS)
def test_kmap_collision_cases_form_a_chain_across_the_end(n):
    cin, cout = R.collision_case(n)
    assert len(cin) == n and len(np.unique(cin, axis=0)) == n and R.capacity(n) == 1024
    probes = cout[n:]
    assert len(probes) == 40 and not set(map(tuple, probes)) & set(map(tuple, cin))
    _chain_holds(f"coords{n}", R.coord_keys(cin), R.coord_keys(probes))
    for K in (1, 27):
        assert R.no_hash_collisions(R.kmap_coordinates(cin, cout, R.offsets_for(K)))


def test_unique_case_forms_a_chain():
    keys = R.unique_tail_case()
    st = R.chain_stats(np.unique(keys))
    assert R.capacity(len(keys)) == 1024 and st["run"] is not None and st["longest"] >= 64


# --------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("name", [c for c in R.QUERY_CASES if c != "n1"])
@pytest.mark.parametrize("flaw", [dict(wrap=False), dict(max_steps=1)])
def test_a_table_that_does_not_wrap_or_gives_up_fails_every_tail_set(name, flaw):
    refs, ref_idx, queries = R.query_case(name)
    pos = R.model_query(queries, refs, **flaw)
    got = np.where(pos >= 0, pos if ref_idx is None else ref_idx[pos], -1)
    assert not np.array_equal(got, R.query_ref(queries, refs, ref_idx))


@pytest.mark.parametrize("n", R.COLLISION_ROWS)
@pytest.mark.parametrize("flaw", [dict(wrap=False), dict(max_steps=1)])
def test_a_broken_table_fails_the_kmap_collision_sets(n, flaw):
    cin, cout = R.collision_case(n)
    want = R.kmap_ref(cin, cout, R.offsets_for(1))["nbr"][0]
    got = R.model_query(R.coord_keys(cout), R.coord_keys(cin), **flaw)
    assert not np.array_equal(got, want)
    assert np.array_equal(R.model_query(R.coord_keys(cout), R.coord_keys(cin)), want)


def test_a_table_that_keeps_the_last_writer_fails_the_duplicate_case():
    refs, ref_idx, queries = R.query_case("thrice")
    pos = R.model_query(queries, refs, keep="last")
    assert not np.array_equal(np.where(pos >= 0, ref_idx[pos], -1), R.query_ref(queries, refs, ref_idx))


LANE63 = ("every", "lane63", "lane255", "wave1")       # patterns with a hit in lane 63 of some wave (n_out = 257; wave1 = rows 64..127)
TWO_WAVES = ("every", "alternate")                     # patterns with hits in two waves of one block


@pytest.mark.parametrize("n_out", [257, 513])
def test_broken_compactions_differ_on_the_lane_patterns(n_out):
    offs = R.offsets_for(1)
    for pattern in R.LANE_PATTERNS:
        case = R.lane_case(pattern, n_out)
        assert case is not None
        ref = R.kmap_ref(*case, offs)
        hits = np.flatnonzero(ref["nbr"][0] >= 0)
        assert np.array_equal(hits, R.lane_rows(pattern, n_out))               # the hits sit in the lanes the pattern names
        lane63 = R.kmap_ref(*case, offs, flaw="lane63")
        wave = R.kmap_ref(*case, offs, flaw="wave_rank")
        assert R.same_tables(ref, lane63) == (pattern not in LANE63), pattern
        assert R.same_tables(ref, wave) == (pattern not in TWO_WAVES), pattern


def test_short_lines_skip_only_the_patterns_they_cannot_hold():
    for n_out in R.LINE_ROWS:
        have = [p for p in R.LANE_PATTERNS if R.lane_case(p, n_out) is not None]
        want = [p for p in R.LANE_PATTERNS if {"lane63": 64, "lane64": 65, "lane255": 256, "block1_first": 257}.get(p, 1) <= n_out]
        assert have == want, n_out


# --------------------------------------------------------------------------- agreement with the oracle
def _same_as_oracle(cin, cout, offs):
    ref = R.kmap_ref(cin, cout, offs)
    res, nbmaps, nbsizes = O.build_kmap(cin, cout, offs)
    assert np.array_equal(ref["nbr"], res) and np.array_equal(ref["nbmaps"], nbmaps) and np.array_equal(ref["nbsizes"], nbsizes)
    assert np.array_equal(ref["nboffs"], np.concatenate([[0], np.cumsum(nbsizes)]))
    # the inverse and position tables restate the pair list
    for k in range(len(offs)):
        for p in range(ref["nboffs"][k], ref["nboffs"][k + 1]):
            i, j = ref["nbmaps"][p]
            assert ref["pos_out"][k, j] == p and ref["pos_in"][k, i] == p and ref["nbr_t"][k, i] == j
    assert (ref["pos_out"] >= 0).sum() == (ref["pos_in"] >= 0).sum() == (ref["nbr_t"] >= 0).sum() == ref["nboffs"][-1]


@pytest.mark.parametrize("K", [1, 8, 10, 27])
def test_kmap_ref_equals_the_oracle(K):
    c = R.blob(300, seed=K)
    _same_as_oracle(c, c, R.offsets_for(K))
    _same_as_oracle(c, O.spdownsample(c, 2, 2, 1), R.offsets_for(8))
    cin, cout = R.collision_case(200)
    _same_as_oracle(cin, cout, R.offsets_for(K))


def test_kmap_ref_lowest_row_wins():
    c = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    ref = R.kmap_ref(c, c[:2], R.offsets_for(3))
    assert ref["nbr"].tolist() == [[-1, 0], [0, 1], [1, -1]] and ref["nbr_t"][:, 2].tolist() == [-1, -1, -1]
    both = R.kmap_ref(c, c, R.offsets_for(1))
    assert both["nbr"].tolist() == [[0, 1, 0]] and R.contested(both, 3).tolist() == [[True, False, False]]


def test_query_unique_downsample_quantize_voxel_refs_equal_the_oracle():
    rs = np.random.RandomState(0)
    refs = rs.randint(0, 1 << 40, 400).astype(np.int64)
    refs = np.concatenate([refs, refs[:50]])
    q = np.concatenate([refs[::3], rs.randint(0, 1 << 40, 200).astype(np.int64)])
    idx = rs.randint(0, 1 << 30, len(refs)).astype(np.int64)
    assert np.array_equal(R.query_ref(q, refs), O.sphashquery(q, refs))
    assert np.array_equal(R.query_ref(q, refs, idx), O.sphashquery(q, refs, idx))
    u, inv = R.unique_ref(refs)
    wu, winv = np.unique(refs, return_inverse=True)
    assert np.array_equal(u, wu) and np.array_equal(inv, winv)
    c = np.concatenate([rs.randint(-9, 9, (500, 3)), rs.randint(0, 2, (500, 1))], 1).astype(np.int32)
    for s in (1, 2, 3, 4):
        assert np.array_equal(R.downsample_ref(c, (s, s, s)), O.spdownsample(c, s, s, 1))
    assert np.array_equal(R.downsample_ref(c, (2, 1, 2)), O.spdownsample(c, (2, 1, 2), (2, 1, 2), 1))
    assert R.downsample_ref(np.array([[-1, -3, 3, 0]]), (2, 2, 2)).tolist() == [[0, -2, 2, 0]]
    index, inverse = R.quantize_ref(c)
    oi, ov = O.sparse_quantize(c[:, [3, 0, 1, 2]])
    assert np.array_equal(index, oi) and np.array_equal(inverse, ov)
    pts = (rs.rand(700, 4) * 100 - 50).astype(np.float32)
    got, mins = R.voxel_coords_ref(pts, 0.05)
    want = O.voxel_coords(pts, 0.05)
    assert np.array_equal(mins[0], want.min(0)) and np.array_equal(got[:, :3], want - want.min(0)) and (got[:, 3] == 0).all()
    half = np.array([[0.25, -0.25, 0.75], [-0.75, 1.25, -1.25]], np.float32)            # quotients +-0.5, +-1.5, +-2.5: to even
    assert R.voxel_coords_ref(half, 0.5, shift=np.zeros((1, 3), np.int32))[0][:, :3].tolist() == [[0, 0, 2], [-2, 2, -2]]
    seg = R.segment_min_ref(np.array([[1, np.nan, -0.0], [2, np.nan, 0.0], [0, 0, 0]], np.float32), [0, 0, 5], 2)
    assert seg[0].tolist() == [1.0, np.inf, 0.0] and np.isinf(seg[1]).all()
    assert R.count_ref([-1, 0, 2, 2, 3], 3).tolist() == [1, 0, 2]


def test_edge_coordinates_do_not_wrap():
    c = R.edge_coords().astype(np.int64)
    assert len(np.unique(c, axis=0)) == len(c) and set(c[:, 3].tolist()) == {0, (1 << 31) - 1}
    assert c[:, :3].max() == (1 << 31) - 2 and c[:, :3].min() == -(1 << 31) + 1
    assert R.no_hash_collisions(R.kmap_coordinates(c, c, R.offsets_for(27)))
