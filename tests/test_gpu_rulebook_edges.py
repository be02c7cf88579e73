"""The integer kernels that build the rulebook - the open-addressing table of csrc/common.h, ts_hash_query / ts_count
(csrc/hash.hip), ts_downsample / ts_unique_i64 / ts_build_kmap / ts_build_kmap_sym (csrc/coords.hip), ts_voxel_coords /
ts_segment_min3 / ts_sparse_quantize (csrc/quantize.hip) - against the plain references of tests/rulebook_ref.py at the edges random
blobs do not reach: probe chains that run across the end of the table, 63 / 64 / 65 and 255 / 256 / 257 rows with hits in chosen
lanes, 1 .. 343 offsets, coordinates at the ends of int32 and of the packed key, every reduction path of the minima.

Bars: every result is an integer table or a rounded integer - every comparison is bit for bit over every element, no tolerance.
Every call runs twice over recycled, garbage-filled allocator blocks and must give the same bits.  The inputs' properties (chains
across the end, no 60-bit hash collision) are proven on the CPU by tests/test_rulebook_host.py; the table model there is never an
expected value here.

Contracts that differ from a naive reference by design, stated here and beside the kernels:
  * the key -1 is the table's empty marker: as a reference of ts_hash_query it is skipped, as a query it is a miss;
  * nbr_t / pos_in hold ONE pair per (offset, input row): where an output coordinate is held twice, two pairs contend for the
    entry and either may stay (`R.contested`); every other entry is compared.
`pytest -s` prints one line per case (rows, pairs, longest chain of the host model): profiles/rulebook_edges.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rulebook_ref as R  # noqa: E402
from oracle import ts_oracle as O  # noqa: E402

DEV = "cuda"
TS_ERR_INVALID_ARGUMENT, TS_ERR_WORKSPACE_TOO_SMALL = -1, -2        # include/taseg_hip.h


@pytest.fixture(scope="module")
def B():
    from taseg_amd import backend
    return backend


@pytest.fixture(scope="module")
def F():
    from taseg_amd.torchsparse.nn import functional
    return functional


@pytest.fixture(scope="module")
def abi():
    from taseg_amd import _lib as L
    return L, L.load()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def C4(a):
    return T(np.asarray(a, dtype=np.int32).reshape(-1, 4))


def dirty():
    """fill blocks of the caching allocator with garbage and hand them back: a table a kernel forgets to clear shows"""
    junk = [torch.full((s,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) for s in (64, 1024, 16 << 10, 256 << 10, 1 << 20)]
    del junk


def host(x):
    if isinstance(x, torch.Tensor):
        return x.cpu().numpy()
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items() if v is not None}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def twice(fn, same=same_bits):
    dirty()
    a = host(fn())
    dirty()
    b = host(fn())
    assert same(a, b), "two runs of one call differ"
    return a


def exact(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype.kind in "iu" and want.dtype.kind in "iu", (what, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, int((got != want).sum()), "elements differ")


def report(case, rows, pairs=0, chain=0):
    print(f"rulebook {case}: rows {rows} pairs {pairs} chain {chain}")


# --------------------------------------------------------------------------- kernel maps: helpers
def gpu_kmap(B, cin, cout, offs, same=same_bits):
    def call():
        km = B.build_kmap(C4(cin), C4(cout), T(np.asarray(offs, dtype=np.int32)), want_inverse=True, want_pos=True)
        km["nbmaps"] = km["nbmaps"][:int(km["nboffs"][-1])]              # (the buffer has room for K * n_out pairs)
        return km
    return twice(call, same)


def check_kmap(got, ref, open_entries=None, what=""):
    """all seven tables against kmap_ref; `open_entries` [K, n_in]: the contested entries of nbr_t / pos_in"""
    for t in R.KMAP_TABLES:
        assert got[t].shape == ref[t].shape, (what, t, got[t].shape, ref[t].shape)
        if open_entries is not None and t in ("nbr_t", "pos_in"):
            exact(got[t][~open_entries], ref[t][~open_entries], (what, t))
        else:
            exact(got[t], ref[t], (what, t))


def run_kmap_case(B, what, cin, cout, offs, chain=0):
    assert R.no_hash_collisions(R.kmap_coordinates(cin, cout, offs)), what
    ref = R.kmap_ref(cin, cout, offs)
    check_kmap(gpu_kmap(B, cin, cout, offs), ref, what=what)
    report(what, f"{len(cin)}->{len(cout)} K {len(offs)}", int(ref["nboffs"][-1]), chain)
    return ref


# --------------------------------------------------------------------------- 1. the table through ts_hash_query
@pytest.mark.parametrize("name", R.QUERY_CASES)
def test_hash_query_over_a_chain_across_the_end_of_the_table(B, name):
    """references whose first slot is one of the last four of the table, so the chain wraps; queries: every reference, absent keys
    that start inside the chain before the wrap, random absent keys.  "thrice": every key three times with an explicit ref_idx,
    the first occurrence wins.  "minus1": the key -1 among the references and the queries is never found (see the module text)."""
    refs, ref_idx, queries = R.query_case(name)
    want = R.query_ref(queries, refs, ref_idx)
    got = twice(lambda: B.hash_query_cuda(T(queries), T(refs), None if ref_idx is None else T(ref_idx)))
    exact(got - 1, want, name)                                         # (the ABI's 0 = miss, idx + 1 = hit)
    if name == "minus1":
        assert (want[queries == -1] == -1).all() and (refs == -1).sum() == 1
    report(f"query {name}", f"{len(refs)} refs {len(queries)} queries", int((want >= 0).sum()), R.chain_stats(refs)["longest"])


def test_hash_query_empty_sets(B):
    q = R.tail_keys(200, 1023)
    none = np.zeros(0, np.int64)
    exact(twice(lambda: B.hash_query_cuda(T(q), T(none), None)), np.zeros(200, np.int64))        # no references: all misses
    assert twice(lambda: B.hash_query_cuda(T(none), T(q), None)).shape == (0,)                   # no queries: nothing
    report("query empty", "0 refs / 0 queries")


# --------------------------------------------------------------------------- 2. the table through ts_build_kmap
@pytest.mark.parametrize("K", [1, 27])
@pytest.mark.parametrize("n", R.COLLISION_ROWS)
def test_kmap_over_a_chain_across_the_end_of_the_table(B, n, K):
    """tail coordinates as inputs (their table: 1024 slots, a chain of n across the end); outputs: the inputs in another order,
    then absent coordinates that start inside the chain - ts_table_find_n's sequential tail on hits and on misses"""
    cin, cout = R.collision_case(n)
    run_kmap_case(B, f"collisions n {n}", cin, cout, R.offsets_for(K), R.chain_stats(R.coord_keys(cin))["longest"])


# --------------------------------------------------------------------------- 3. block and wave edges of the map
@pytest.mark.parametrize("K", [1, 27])
@pytest.mark.parametrize("n_out", R.LINE_ROWS)
def test_kmap_hits_in_chosen_lanes(B, n_out, K):
    """output rows on a line (row j = lane j % 64 of wave j / 64 % 4 of block j / 256), the inputs the subset that puts the centre
    hits in no lane (no input rows at all / inputs away from the line), every lane, thread 0 / 63 / 64 / 255 of every block, the
    first row of the second block, alternate lanes, one whole wave - where the line is long enough to have such a row"""
    ran = 0
    for pattern in R.LANE_PATTERNS:
        case = R.lane_case(pattern, n_out)
        if case is None:
            continue
        ref = run_kmap_case(B, f"lanes {pattern}", *case, R.offsets_for(K))
        ran += 1
        if pattern in ("no_rows", "disjoint"):
            assert (ref["nbr"] == -1).all() and (ref["nbsizes"] == 0).all() and (ref["nboffs"] == 0).all()
            assert ref["nbr_t"].shape == (K, len(case[0])) and len(case[0]) == (0 if pattern == "no_rows" else min(n_out, 70))
    assert ran >= 5


# --------------------------------------------------------------------------- 4. offset counts
@pytest.mark.parametrize("K", [1, 8, 9, 10, 27, 28, 125, 343])
def test_kmap_offset_counts(B, K):
    """rounds of 9 probes with the index clamped in the last one (K = 1, 8, 10, 28), exactly full rounds (9, 27), the strided LDS
    counter loop (K = 343 > 256 threads): 300 voxels of a dense 8^3 blob in two samples, shuffled"""
    c = R.blob(300, seed=4)
    run_kmap_case(B, "offsets", c, c, R.offsets_for(K))


@pytest.mark.parametrize("ts", [1, 2])
def test_kmap_between_two_coordinate_sets(B, F, ts):
    """in != out: the outputs are the stride-2 down-sampling of the inputs, the offsets those of a 2x2x2 kernel at tensor stride ts"""
    cin = R.blob(300, seed=5)
    cin[:, :3] *= ts
    cout = R.downsample_ref(cin, (2 * ts,) * 3)
    exact(twice(lambda: F.spdownsample(C4(cin), 2, 2, ts)), cout, "spdownsample")
    assert np.array_equal(cout, O.spdownsample(cin, 2, 2, ts))
    ref = run_kmap_case(B, f"strided ts {ts}", cin, cout, O.get_kernel_offsets(2, ts).astype(np.int32))
    assert int(ref["nboffs"][-1]) == len(cin)                          # every input row feeds exactly one output row


# --------------------------------------------------------------------------- 5. the symmetric builder, through the C ABI
def sym_call(abi, c, offs, with_nbr=True, n=None, K=None):
    """ts_build_kmap_sym as the index plan calls it; returns (code, tables)"""
    L, lib = abi
    n = len(c) if n is None else n
    K = len(offs) if K is None else K
    ct, ot = C4(c), T(np.asarray(offs, dtype=np.int32))
    ws = L.workspace(lib.ts_build_kmap_workspace_bytes(n, n, K), ct.device)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=DEV)
    t = dict(nbr=i32(K, n), nbr_t=i32(K, n), nbmaps=i32(max(K * n, 1), 2), nbsizes=i32(K), nboffs=i32(K + 1), pos_out=i32(K, n),
             pos_in=i32(K, n))
    rc = lib.ts_build_kmap_sym(L.ptr(ct), n, L.ptr(ot), K, L.ptr(t["nbr"]) if with_nbr else None, L.ptr(t["nbr_t"]),
                               L.ptr(t["nbmaps"]), L.ptr(t["nbsizes"]), L.ptr(t["nboffs"]), L.ptr(t["pos_out"]), L.ptr(t["pos_in"]),
                               L.ptr(ws), ws.numel(), L.stream())
    return rc, t


@pytest.mark.parametrize("K", [3, 27, 125, 343])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_symmetric_builder_equals_the_full_probe_and_the_reference(B, abi, n, K):
    """K / 2 + 1 = 2, 14, 63, 172 look-ups per row: the 9-wide template in one clamped round, the 14-wide one, the 9-wide one in 7
    rounds, and the strided LDS counter loop; every table equals ts_build_kmap's and kmap_ref's"""
    c, offs = R.blob(n, seed=n), R.offsets_for(K)
    assert np.array_equal(offs[::-1], -offs)                            # the symmetry the builder relies on

    def call():
        rc, t = sym_call(abi, c, offs)
        assert rc == 0, rc
        t["nbmaps"] = t["nbmaps"][:int(t["nboffs"][-1])]
        return t
    got = twice(call)
    ref = run_kmap_case(B, "symmetric", c, c, offs)
    check_kmap(got, ref, what=("sym", n, K))
    assert same_bits({k: got[k] for k in R.KMAP_TABLES}, {k: v for k, v in gpu_kmap(B, c, c, offs).items() if k in R.KMAP_TABLES})


def test_symmetric_builder_reports_a_repeated_coordinate_and_refuses_bad_calls(abi):
    L, lib = abi
    c = R.blob(257, seed=1)
    twin = np.concatenate([c, c[100:101]])
    for K in (3, 27, 125):
        rc, t = sym_call(abi, twin, R.offsets_for(K))
        assert rc == 0 and int(t["nboffs"][K]) == -1, K                 # the pair total reads -1: the caller probes in full
        rc, t = sym_call(abi, c, R.offsets_for(K))
        assert rc == 0 and int(t["nboffs"][K]) > 0
    for what, args in (("even K", dict(offs=R.offsets_for(8))), ("K = 1", dict(offs=R.offsets_for(1))),
                       ("n = 0", dict(offs=R.offsets_for(27), n=0)), ("null nbr", dict(offs=R.offsets_for(27), with_nbr=False))):
        rc, _ = sym_call(abi, c, **args)
        assert rc == TS_ERR_INVALID_ARGUMENT, (what, rc)
        assert b"ts_build_kmap_sym" in lib.ts_last_error()
    rc, t = sym_call(abi, c, R.offsets_for(27))                         # the next valid call is unaffected
    assert rc == 0
    exact(host(t["nbr"]), R.kmap_ref(c, c, R.offsets_for(27))["nbr"])
    report("symmetric refusals", 257)


def test_workspace_and_alignment_refusals(B, abi):
    """a workspace one byte short is TS_ERR_WORKSPACE_TOO_SMALL, a misaligned pointer TS_ERR_INVALID_ARGUMENT, before anything is
    launched; the next valid call is unaffected"""
    L, lib = abi
    c, offs = R.blob(300, seed=2), R.offsets_for(27)
    pad = torch.zeros(301 * 4 + 4, dtype=torch.int32, device=DEV)
    pad[1:1201] = C4(c).reshape(-1)
    ct, ot = C4(c), T(offs)
    need = lib.ts_build_kmap_workspace_bytes(300, 300, 27)
    ws = L.workspace(need, ct.device)
    nbr, sizes, offs_out = (torch.empty(s, dtype=torch.int32, device=DEV) for s in ((27, 300), (27,), (28,)))

    def kmap(coords_ptr, ws_bytes):
        return lib.ts_build_kmap(coords_ptr, 300, coords_ptr, 300, L.ptr(ot), 27, L.ptr(nbr), None, None, L.ptr(sizes), L.ptr(offs_out),
                                 None, None, L.ptr(ws), ws_bytes, L.stream())
    assert kmap(L.ptr(ct), need - 1) == TS_ERR_WORKSPACE_TOO_SMALL
    assert kmap(L.ptr(pad) + 4, need) == TS_ERR_INVALID_ARGUMENT
    assert kmap(L.ptr(ct), need) == 0
    exact(host(nbr), R.kmap_ref(c, c, offs)["nbr"])
    keys = T(R.tail_keys(200, 1023))
    out = torch.empty(200, dtype=torch.int64, device=DEV)
    need = lib.ts_hash_query_workspace_bytes(200)
    assert need == 1024 * 12
    assert lib.ts_hash_query(L.ptr(keys), 200, L.ptr(keys), None, 200, L.ptr(out), L.ptr(ws), need - 1, L.stream()) \
        == TS_ERR_WORKSPACE_TOO_SMALL
    assert lib.ts_hash_query(L.ptr(keys), 200, L.ptr(keys), None, 200, L.ptr(out), L.ptr(ws) + 4, need, L.stream()) \
        == TS_ERR_INVALID_ARGUMENT
    assert lib.ts_hash_query(L.ptr(keys), 200, L.ptr(keys), None, 200, L.ptr(out), L.ptr(ws), need, L.stream()) == 0
    exact(host(out), np.arange(1, 201))
    need = lib.ts_downsample_workspace_bytes(300)
    ws = L.workspace(need + 256, ct.device)
    down, cnt = torch.empty((300, 4), dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)

    def ds(coords_ptr, ws_ptr, ws_bytes):
        return lib.ts_downsample(coords_ptr, 300, 2, 2, 2, L.ptr(down), L.ptr(cnt), ws_ptr, ws_bytes, L.stream())
    assert ds(L.ptr(ct), L.ptr(ws), need - 1) == TS_ERR_WORKSPACE_TOO_SMALL
    assert ds(L.ptr(ct), L.ptr(ws) + 8, need) == TS_ERR_INVALID_ARGUMENT
    assert ds(L.ptr(pad) + 4, L.ptr(ws), need) == TS_ERR_INVALID_ARGUMENT
    assert ds(L.ptr(ct), L.ptr(ws), need) == 0
    want = R.downsample_ref(c, (2, 2, 2))
    assert int(cnt) == len(want)
    exact(host(down[:len(want)]), want)
    report("refusals", 300)


# --------------------------------------------------------------------------- 6. the ends of int32 and of the batch field
def test_kmap_at_the_ends_of_int32(B):
    """x, y or z within 2 of +-2^31 (coordinate + offset does not wrap), batch 0 and 2^31 - 1"""
    c = R.edge_coords()
    ref = run_kmap_case(B, "int32 ends", c, c, R.offsets_for(27))
    assert int(ref["nboffs"][-1]) > 3 * len(c)                          # the clusters are dense: neighbours beside the centre hits


def test_kmap_with_repeated_input_coordinates(B):
    """a repeated input coordinate: the lowest row wins in every table.  Outputs without a repeat: all seven tables are defined
    (the losing rows have no pair).  in == out: two output rows then share their neighbours, and the nbr_t / pos_in entries of
    those neighbours are contested - excluded, as test_symmetric_submanifold_kernel_maps_equal_the_full_probe excludes pos_in"""
    base = R.edge_coords()
    rep = np.concatenate([base[:40], base[5:9], base[40:], base[7:8], base[100:103]])
    offs = R.offsets_for(27)
    ref = run_kmap_case(B, "repeated inputs", rep, base, offs)
    losers = np.array([i for i in range(len(rep)) if any((rep[:i] == rep[i]).all(1))])
    assert len(losers) == 8 and (ref["nbr_t"][:, losers] == -1).all() and not np.isin(ref["nbr"], losers).any()
    assert not R.contested(ref, len(rep)).any()
    both = R.kmap_ref(rep, rep, offs)
    open_entries = R.contested(both, len(rep))
    assert open_entries.any() and open_entries.sum() < open_entries.size // 4

    def same(a, b):
        return all((a[t][~open_entries].tobytes() == b[t][~open_entries].tobytes()) if t in ("nbr_t", "pos_in")
                   else same_bits(a[t], b[t]) for t in R.KMAP_TABLES)
    got = gpu_kmap(B, rep, rep, offs, same)
    check_kmap(got, both, open_entries, "repeated in == out")
    k, i = np.nonzero(open_entries)                                     # a contested entry holds ONE of its pairs
    p = got["pos_in"][k, i]
    assert (p >= both["nboffs"][k]).all() and (p < both["nboffs"][k + 1]).all() and (both["nbmaps"][p, 0] == i).all()
    assert (both["nbr"][k, got["nbr_t"][k, i]] == i).all()
    report("repeated in == out", len(rep), int(both["nboffs"][-1]))


# --------------------------------------------------------------------------- 7. ts_downsample
def ds_cloud(n, seed=7):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.randint(-9, 9, (n, 3)), rs.randint(0, 2, (n, 1))], 1).astype(np.int32)


@pytest.mark.parametrize("stride", [(2, 2, 2), (4, 4, 4), (2, 1, 2), (1, 1, 1), (3, 3, 3)])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_downsample_strides_and_block_edges(F, n, stride):
    """coordinates in [-9, 9): truncation toward zero (-1 -> 0, -3 -> -2 at stride 2), per-axis strides"""
    c = ds_cloud(257)[:n]
    want = R.downsample_ref(c, stride)
    got = twice(lambda: F.spdownsample(C4(c), stride, stride, 1))
    assert got.dtype == np.int32
    exact(got, want, (n, stride))
    report(f"downsample {stride}", n, len(want))


def test_downsample_truncates_toward_zero_and_merges_equal_rows(F):
    c = np.array([[-1, -3, 3, 0], [-2, -1, 1, 0], [1, 1, -1, 0]], np.int32)
    exact(host(F.spdownsample(C4(c), 2, 2, 1)), [[-2, 0, 0, 0], [0, -2, 2, 0], [0, 0, 0, 0]])
    one = np.repeat(np.array([[5, -7, 3, 1]], np.int32), 257, 0)
    exact(twice(lambda: F.spdownsample(C4(one), 2, 2, 1)), [[4, -6, 2, 1]])


LO, HI = -(1 << 17), (1 << 17) - 1       # the packed key's coordinate range, tested on the truncated value


@pytest.mark.parametrize("what,row,stride,ok", [
    ("lowest", [LO, 0, 0, 0], 1, True), ("highest", [0, HI, 0, 0], 1, True), ("highest at stride 2", [0, 0, HI, 0], 2, True),
    ("below, truncates into range", [LO - 1, 0, 0, 0], 2, True), ("below at stride 1", [0, LO - 1, 0, 0], 1, False),
    ("above", [HI + 1, 0, 0, 0], 2, False), ("above at stride 1", [0, 0, HI + 1, 0], 1, False),
    ("batch 1023", [1, 2, 3, 1023], 2, True), ("batch 1024", [1, 2, 3, 1024], 2, False), ("batch -1", [1, 2, 3, -1], 2, False)])
def test_downsample_range(F, what, row, stride, ok):
    c = np.concatenate([ds_cloud(64), np.array([row], np.int32), ds_cloud(64, seed=8)])
    if ok:
        exact(twice(lambda: F.spdownsample(C4(c), stride, stride, 1)), R.downsample_ref(c, (stride,) * 3), what)
    else:
        with pytest.raises(ValueError):
            F.spdownsample(C4(c), stride, stride, 1)
        good = ds_cloud(64)                                             # the next valid call is unaffected
        exact(host(F.spdownsample(C4(good), stride, stride, 1)), R.downsample_ref(good, (stride,) * 3), what)


# --------------------------------------------------------------------------- 8. ts_unique_i64
@pytest.mark.parametrize("case", ["n0", "n1", "n2_equal", "n2_descending", "all_equal", "descending", "ends", "tail_chain"])
def test_unique_i64_edges(B, case):
    top = (1 << 62) - 1
    keys = {"n0": [], "n1": [12345], "n2_equal": [7, 7], "n2_descending": [9, 3], "all_equal": [top] * 257,
            "descending": list(range(5 * 257, 0, -5)), "ends": [top, 0, 5, top, 0, 1 << 61] * 40 + [top - 1] * 17,
            "tail_chain": R.unique_tail_case()}[case]
    keys = np.asarray(keys, dtype=np.int64)
    wu, winv = R.unique_ref(keys)
    u, inv = twice(lambda: B.unique_i64(T(keys)))
    exact(u, wu, case)
    exact(inv, winv, case)
    assert inv.dtype == np.int32 and u.dtype == np.int64
    exact(twice(lambda: B.unique_i64(T(keys), return_inverse=False)), wu, case)
    report(f"unique {case}", len(keys), len(wu), R.chain_stats(wu)["longest"] if len(wu) else 0)


@pytest.mark.parametrize("bad", [1 << 62, -1, -(1 << 63), (1 << 63) - 1])
def test_unique_i64_refuses_keys_outside_62_bits(B, bad):
    keys = np.concatenate([R.tail_keys(100, 1023), [bad], R.tail_keys(200, 1023)[100:]]).astype(np.int64)
    with pytest.raises(ValueError):
        B.unique_i64(T(keys))
    with pytest.raises(ValueError):
        B.unique_i64(T(keys), return_inverse=False)
    good = keys[keys != bad]
    exact(host(B.unique_i64(T(good))[0]), np.unique(good))


# --------------------------------------------------------------------------- 9. ts_sparse_quantize
def interleaved_voxels(n, seed=9):
    """n rows over voxels held by 1 .. 5 points each, the points of a voxel spread over the rows; two samples whose coordinates
    coincide"""
    rs = np.random.RandomState(seed)
    vox = R.blob(max(1, n // 2), seed=seed, side=6, batches=1)
    vox = np.concatenate([vox, vox * [1, 1, 1, 0] + [0, 0, 0, 1]]).astype(np.int32)      # the same cells in sample 1
    vox[:, :3] -= 3
    rows = np.concatenate([np.repeat(v, 1 + v % 5) for v in range(len(vox))])
    return vox[rs.permutation(rows)[:n]]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_sparse_quantize_edges(B, n):
    c = interleaved_voxels(n)
    windex, winverse = R.quantize_ref(c)
    index, inverse = twice(lambda: B.sparse_quantize(C4(c)))
    exact(index, windex, n)
    exact(inverse, winverse, n)
    if n >= 255:
        held = np.bincount(winverse)
        assert held.max() >= 3 and held.min() == 1 and len(np.unique(c[windex][:, 3])) == 2
        assert np.array_equal(c[windex][winverse], c) and (np.diff(windex) < 0).any()
    report("quantize", n, len(windex))


@pytest.mark.parametrize("what,row,ok", [
    ("lowest", [LO, 0, 0, 0], True), ("highest", [0, HI, HI, 1], True), ("below", [LO - 1, 0, 0, 0], False),
    ("above", [0, 0, HI + 1, 0], False), ("batch 1023", [1, 2, 3, 1023], True), ("batch 1024", [1, 2, 3, 1024], False),
    ("batch -1", [1, 2, 3, -1], False)])
def test_sparse_quantize_range(B, what, row, ok):
    """the range of ts_downsample's key without its truncation: -2^17 - 1 is outside"""
    c = np.concatenate([interleaved_voxels(64), np.array([row, row], np.int32), interleaved_voxels(64, seed=10)])
    if ok:
        index, inverse = twice(lambda: B.sparse_quantize(C4(c)))
        windex, winverse = R.quantize_ref(c)
        exact(index, windex, what)
        exact(inverse, winverse, what)
    else:
        with pytest.raises(ValueError):
            B.sparse_quantize(C4(c))
        good = interleaved_voxels(64)
        exact(host(B.sparse_quantize(C4(good))[1]), R.quantize_ref(good)[1], what)


# --------------------------------------------------------------------------- 10. ts_voxel_coords
TIES = np.array([[1, -1, 3], [-3, 5, -5], [7, -7, 1], [-1, 3, -3]])       # odd k: the quotient k / 2 is exactly on .5


def vc_points(n, stride, vs, rs):
    p = (rs.rand(n, stride) * 100 - 50).astype(np.float32)
    if vs != 0.05:
        k = rs.randint(-41, 41, (n, 3))
        k[:min(n, 4)] = TIES[:min(n, 4)]
        p[:, :3] = (k * (vs / 2)).astype(np.float32)                    # small integers times a power of two: exact, as is the quotient
        assert ((p[:, :3] / np.float32(vs)) * 2 == k).all()
    return p


def vc_batch(n, n_batch, rs):
    """rows spread over the samples; sample n_batch // 2 owns none (n_batch >= 2); one row at -1 and one at n_batch"""
    empty = n_batch // 2 if n_batch > 1 else -1
    b = rs.choice([s for s in range(n_batch) if s != empty], n).astype(np.int32)
    if n >= 3:
        b[1], b[2] = -1, n_batch
    return b, empty


@pytest.mark.parametrize("n_batch", [1, 2, 64, 65])
def test_voxel_coords_reduction_paths_and_ties(B, n_batch):
    """the minima in registers (one sample), in LDS (2 .. 64), with global atomics (65); rows of 3, 4 and 6 floats; quotients
    exactly on .5 at voxel sizes 0.5 and 0.25 round to even; a sample without rows keeps the fill value; a batch index outside
    [0, n_batch) leaves the row unshifted and out of the minima; the shift= form subtracts what it is given"""
    rs = np.random.RandomState(n_batch)
    for n in (1, 255, 256, 257, 1025):
        for vs, stride in ((0.5, 3), (0.25, 4), (0.05, 6)):
            p = vc_points(n, stride, vs, rs)
            b, empty = vc_batch(n, n_batch, rs)
            want, wmins = R.voxel_coords_ref(p, vs, b, n_batch)
            got, mins = twice(lambda: B.voxel_coords(T(p), vs, T(b), n_batch))
            exact(got, want, (n, vs))
            exact(mins, wmins, (n, vs))
            if empty >= 0:
                assert (mins[empty] == R.MIN_FILL).all()
            if n >= 3:
                raw = np.round(p[1:3, :3] / np.float32(vs)).astype(np.int32)
                assert np.array_equal(got[1:3, :3], raw) and got[1, 3] == -1 and got[2, 3] == n_batch
            shift = rs.randint(-5, 6, (n_batch, 3)).astype(np.int32)
            want_s, _ = R.voxel_coords_ref(p, vs, b, n_batch, shift)
            got_s, used = twice(lambda: B.voxel_coords(T(p), vs, T(b), n_batch, shift=T(shift)))
            exact(got_s, want_s, (n, vs, "shift"))
            exact(used, shift)
            if n_batch == 1:                                            # without batch indices: every row is sample 0
                want0, wmins0 = R.voxel_coords_ref(p, vs)
                got0, mins0 = twice(lambda: B.voxel_coords(T(p), vs))
                exact(got0, want0, (n, vs, "no batch"))
                exact(mins0, wmins0)
        report(f"voxel_coords n_batch {n_batch}", n)


def test_voxel_coords_rounds_half_to_even(B):
    q = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 0.49999997, 0.50000006], np.float32)
    even = [0, 0, 2, -2, 2, -2, 4, -4, 0, 1]
    for vs in (0.5, 0.25):
        p = np.zeros((len(q), 3), np.float32)
        p[:, 0] = p[:, 2] = q * np.float32(vs)
        got, _ = twice(lambda: B.voxel_coords(T(p), vs, shift=T(np.zeros((1, 3), np.int32))))
        exact(got[:, 0], even, vs)
        exact(got, R.voxel_coords_ref(p, vs, shift=np.zeros((1, 3), np.int32))[0], vs)


# --------------------------------------------------------------------------- 11. ts_segment_min3
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("n_seg", [1, 2, 64])
def test_segment_min3_edges(B, n_seg):
    """a NaN among finite values never wins; a segment of only NaN rows and a segment without rows stay +inf; segment ids outside
    [0, n_seg) - -1, n_seg, +-2^32 (which a 32-bit cast would fold onto segment 0) - belong to no segment"""
    rs = np.random.RandomState(n_seg)
    n = 700
    p = (rs.rand(n, 5) * 100 - 50).astype(np.float32)
    seg = rs.randint(0, n_seg, n).astype(np.int64)
    nan_seg, empty_seg = (3, 63) if n_seg == 64 else (1, -1) if n_seg == 2 else (-1, -1)
    seg[seg == empty_seg] = 0
    p[rs.choice(n, 40, replace=False), rs.randint(0, 3, 40)] = np.nan
    if nan_seg >= 0:
        p[seg == nan_seg, :3] = np.nan
    outside = rs.choice(n, 8, replace=False)
    seg[outside] = [-1, n_seg, 1 << 32, -(1 << 32), (1 << 32) + n_seg - 1, 1 << 31, 1 << 40, -(1 << 63)]
    p[outside, :3] = -1000.0                                            # would win every minimum if it were counted
    want = R.segment_min_ref(p, seg, n_seg)
    got = twice(lambda: B.segment_min3(T(p), T(seg), n_seg))
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert want.min() > -1000 and np.isfinite(want[0]).all()
    if nan_seg >= 0:
        assert np.isposinf(got[nan_seg]).all()
    if empty_seg >= 0:
        assert np.isposinf(got[empty_seg]).all()
    report(f"segment_min3 n_seg {n_seg}", n)


def test_segment_min3_zeros_empty_input_and_refusals(B):
    from taseg_amd._lib import BackendError
    p = np.array([[-0.0, 0.0, 5.0], [0.0, -0.0, 7.0], [3.0, 2.0, -0.0]], np.float32)
    got = twice(lambda: B.segment_min3(T(p), T(np.zeros(3, np.int64)), 1))
    assert np.array_equal(got, [[0.0, 0.0, 0.0]])                       # -0.0 and +0.0 in one segment: compared by value
    got = twice(lambda: B.segment_min3(T(p[2:]), T(np.zeros(1, np.int64)), 1))
    assert np.array_equal(bits(got), bits([[3.0, 2.0, -0.0]]))
    got = twice(lambda: B.segment_min3(T(np.zeros((0, 4), np.float32)), T(np.zeros(0, np.int64)), 64))
    assert got.shape == (64, 3) and np.isposinf(got).all()
    for n_seg in (65, 0):
        with pytest.raises(BackendError):
            B.segment_min3(T(p), T(np.zeros(3, np.int64)), n_seg)
    assert np.array_equal(host(B.segment_min3(T(p), T(np.zeros(3, np.int64)), 1)), [[0.0, 0.0, 0.0]])


# --------------------------------------------------------------------------- 12. ts_count
def test_count_edges(B):
    rs = np.random.RandomState(12)
    idx = rs.randint(-1, 51, 1000).astype(np.int32)                     # -1 and n_out = 50 among them: ignored
    assert (idx == -1).any() and (idx == 50).any()
    exact(twice(lambda: B.count_cuda(T(idx), 50)), R.count_ref(idx, 50))
    assert np.array_equal(R.count_ref(idx, 50), O.spcount(idx[idx < 50], 50))
    assert twice(lambda: B.count_cuda(T(idx), 0)).shape == (0,)
    exact(twice(lambda: B.count_cuda(T(idx[:0]), 7)), np.zeros(7, np.int32))
    one = np.full(257, 3, np.int32)
    exact(twice(lambda: B.count_cuda(T(one), 5)), [0, 0, 0, 257, 0])
    extreme = np.array([-(1 << 31), (1 << 31) - 1, 0, 4, 5], np.int32)
    exact(twice(lambda: B.count_cuda(T(extreme), 5)), [1, 0, 0, 0, 1])
    report("count", 1000)
