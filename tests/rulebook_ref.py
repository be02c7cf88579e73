"""Plain references for the integer kernels that build the rulebook (csrc/common.h's hash table, csrc/hash.hip, csrc/coords.hip,
csrc/quantize.hip), a model of the hash table, and builders of inputs that force what random input almost never does: probe chains
that run across the end of the table.

Three kinds of code, kept apart:
  * references (`kmap_ref`, `query_ref`, `unique_ref`, `quantize_ref`, `downsample_ref`, `voxel_coords_ref`, `segment_min_ref`,
    `count_ref`): Python loops and dicts keyed on the VALUES (coordinate tuples, keys), never on a hash slot - the only expected
    values the GPU tests compare with;
  * `TableModel`: `ts_table_capacity`, `ts_slot0` and linear probing transcribed from csrc/common.h.  It constructs inputs and
    proves that they have the property they are named for (tests/test_rulebook_host.py); it is never an expected value;
  * builders (`tail_keys`, `tail_coords`, `probe_into`, the case tables below): deterministic, a fixed seed and fixed boxes.

tests/test_rulebook_host.py runs all of it on the CPU; tests/test_gpu_rulebook_edges.py compares the kernels with the references."""
import functools

import numpy as np

from oracle import ts_oracle as O

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15          # ts_slot0's multiplier
EMPTY = M64                          # TS_EMPTY_KEY: the key -1, which the kernels skip and no FNV-60 value equals
MIN_FILL = 0x7F7F7F7F                # ts_voxel_coords: the minima of a sample that owns no row (its memset's 0x7F bytes)
I32 = (-(1 << 31), (1 << 31) - 1)


# ------------------------------------------------------------------------------------------------ the table, as a model
def capacity(n):
    """ts_table_capacity: the smallest power of two >= max(1024, 2 n + 2)"""
    cap = 1024
    while cap < 2 * n + 2:
        cap <<= 1
    return cap


def slot0(key, mask):
    """ts_slot0: the high half of key * GOLDEN (mod 2^64), masked"""
    return (((int(key) & M64) * GOLDEN & M64) >> 32) & mask


def slot0_np(keys, mask):
    with np.errstate(over="ignore"):
        m = np.asarray(keys).astype(np.uint64) * np.uint64(GOLDEN)
    return ((m >> np.uint64(32)) & np.uint64(mask)).astype(np.int64)


class TableModel:
    """ts_table_insert / ts_table_find: open addressing, linear probing with (s + 1) & mask, the smallest value wins for a repeated
    key, the key -1 is never stored and never found.  The three flaws are what the host tests' teeth cases switch on:
      wrap=False      the walk stops at the last slot instead of going on at slot 0
      max_steps=1     the walk gives up after one step past the first slot
      keep="last"     a repeated key keeps the value of the last writer"""

    def __init__(self, n, wrap=True, max_steps=None, keep="min"):
        self.cap = capacity(n)
        self.mask = self.cap - 1
        self.keys = [EMPTY] * self.cap
        self.vals = [None] * self.cap
        self.wrap, self.max_steps, self.keep = wrap, max_steps, keep

    def walk(self, key):
        s = slot0(key, self.mask)
        for probe in range(self.cap):
            if self.max_steps is not None and probe > self.max_steps:
                return
            yield s
            if not self.wrap and s == self.mask:
                return
            s = (s + 1) & self.mask

    def insert(self, key, val):
        key = int(key) & M64
        if key == EMPTY:
            return
        for s in self.walk(key):
            if self.keys[s] in (EMPTY, key):
                old = self.vals[s] if self.keys[s] == key else None
                self.keys[s] = key
                self.vals[s] = val if old is None or self.keep == "last" else min(old, val)
                return

    def find(self, key):
        key = int(key) & M64
        if key == EMPTY:
            return -1
        for s in self.walk(key):
            if self.keys[s] == key:
                return self.vals[s]
            if self.keys[s] == EMPTY:
                return -1
        return -1

    def fill(self, keys):
        for i, k in enumerate(keys):
            self.insert(k, i)
        return self

    def displacement(self, key):
        """slots between the key's first slot and the slot it sits in (-1: not stored)"""
        key = int(key) & M64
        for d, s in enumerate(self.walk(key)):
            if self.keys[s] == key:
                return d
            if self.keys[s] == EMPTY:
                return -1
        return -1

    def miss_walk(self, key):
        """the slots a look-up of an absent key reads, the empty one that ends it included"""
        out = []
        for s in self.walk(key):
            out.append(s)
            if self.keys[s] == EMPTY:
                break
        return out

    def run_across_the_end(self):
        """(first, last) slot of the run of occupied slots that holds the last slot and slot 0, or None"""
        if self.keys[self.mask] == EMPTY or self.keys[0] == EMPTY or EMPTY not in self.keys:
            return None
        a = self.mask
        while self.keys[a - 1] != EMPTY:
            a -= 1
        b = 0
        while self.keys[b + 1] != EMPTY:
            b += 1
        return a, b


def model_query(queries, refs, **flaws):
    """position of every query among refs through the model (-1 = miss)"""
    t = TableModel(len(refs), **flaws).fill(refs)
    return np.array([t.find(q) for q in queries], dtype=np.int64)


def chain_stats(keys):
    """what the host test asserts and the GPU test prints: the run across the end of the table and the longest displacement"""
    t = TableModel(len(keys)).fill(keys)
    disp = [t.displacement(k) for k in keys if int(k) & M64 != EMPTY]
    return dict(mask=t.mask, run=t.run_across_the_end(), longest=max(disp) if disp else 0, table=t)


def coord_keys(coords):
    """the table keys of coordinates: their 60-bit FNV hashes"""
    return O.sphash(np.asarray(coords, dtype=np.int32).reshape(-1, 4))


# ------------------------------------------------------------------------------------------------ adversarial inputs
TAIL_SLOTS = 4        # a "tail" key's first slot is one of the last four slots of the table
BOX = 20              # coordinates come from [-BOX, BOX)^3, one batch index after the other
PROBE_BATCH = 512     # ... `probe_into`'s from the same box at batch indices from here on: never a `tail_coords` row


@functools.lru_cache(maxsize=None)
def _box(batch):
    r = np.arange(-BOX, BOX, dtype=np.int32)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(x.size, batch, np.int32)], 1)


@functools.lru_cache(maxsize=None)
def _random_keys(seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 1 << 30, 400000).astype(np.int64) << 29) | rs.randint(0, 1 << 29, 400000).astype(np.int64)   # [0, 2^59)


def _collect(n, chunks, keep):
    got, have = [], 0
    for c in chunks:
        sel = c[keep(c)]
        got.append(sel)
        have += len(sel)
        if have >= n:
            return np.concatenate(got)[:n].copy()
    raise ValueError("not enough candidates")


def tail_coords(n, mask):
    """n distinct coordinates of the box whose first slot is one of the last TAIL_SLOTS slots of a table with `mask`"""
    return _collect(n, (_box(b) for b in range(PROBE_BATCH)), lambda c: slot0_np(coord_keys(c), mask) > mask - TAIL_SLOTS)


def tail_keys(n, mask):
    """the same for raw int64 keys in [0, 2^59) (seeded)"""
    keys = _collect(n, (_random_keys(s) for s in range(100, 164)), lambda k: slot0_np(k, mask) > mask - TAIL_SLOTS)
    assert len(np.unique(keys)) == n
    return keys


def probe_into(chain, mask, n):
    """n absent coordinates ([m, 4] chain) or keys ([m] chain) whose first slot lies inside the run of occupied slots that the
    chain's table holds across its end - before the wrap, so that the look-up has to walk through it to reach an empty slot"""
    chain = np.asarray(chain)
    coords = chain.ndim == 2
    keys = coord_keys(chain) if coords else chain
    t = TableModel(len(keys)).fill(keys)
    assert t.mask == mask, (t.mask, mask)
    first, _ = t.run_across_the_end()
    if coords:
        assert chain[:, 3].max() < PROBE_BATCH
        return _collect(n, (_box(b) for b in range(PROBE_BATCH, 2 * PROBE_BATCH)), lambda c: slot0_np(coord_keys(c), mask) >= first)
    have = set(keys.tolist())
    out = _collect(n, (_random_keys(s) for s in range(200, 264)),
                   lambda k: (slot0_np(k, mask) >= first) & ~np.isin(k, keys))
    assert not have & set(out.tolist())
    return out


def no_hash_collisions(coords):
    """no two DISTINCT coordinates among the rows share a 60-bit hash: keying on coordinates and keying on hashes then agree"""
    u = np.unique(np.asarray(coords, dtype=np.int64).reshape(-1, 4), axis=0)
    assert u[:, :3].min() >= I32[0] and u.max() <= I32[1], "a coordinate left int32"
    return len(np.unique(coord_keys(u.astype(np.int32)))) == len(u)


def kmap_coordinates(in_coords, out_coords, offsets):
    """every coordinate a kernel-map build hashes: the input rows and output row + offset"""
    o = np.asarray(out_coords, dtype=np.int64).reshape(-1, 4)
    q = np.repeat(o[None], len(offsets), 0)
    q[:, :, :3] += np.asarray(offsets, dtype=np.int64)[:, None, :]
    return np.concatenate([np.asarray(in_coords, dtype=np.int64).reshape(-1, 4), q.reshape(-1, 4)])


# ------------------------------------------------------------------------------------------------ references
def query_ref(queries, refs, ref_idx=None):
    """ts_hash_query: the position (or ref_idx value) of the FIRST reference equal to the query, -1 where there is none.
    The key -1 is the table's empty marker: as a reference it is skipped, as a query it is a miss (the stated contract)."""
    first = {}
    for i, r in enumerate(np.asarray(refs, dtype=np.int64).tolist()):
        if r != -1 and r not in first:
            first[r] = i if ref_idx is None else int(ref_idx[i])
    return np.array([first.get(q, -1) if q != -1 else -1 for q in np.asarray(queries, dtype=np.int64).reshape(-1).tolist()],
                    dtype=np.int64)


def unique_ref(keys):
    """sorted distinct keys and, per key, its rank among them"""
    keys = np.asarray(keys, dtype=np.int64).tolist()
    uniq = sorted(set(keys))
    rank = {k: i for i, k in enumerate(uniq)}
    return np.array(uniq, dtype=np.int64), np.array([rank[k] for k in keys], dtype=np.int32)


def quantize_ref(coords):
    """ts_sparse_quantize: voxels in ascending (b, x, y, z) order; (row of the first point of every voxel in input order,
    voxel of every row)"""
    first = {}
    rows = [(int(b), int(x), int(y), int(z)) for x, y, z, b in np.asarray(coords).reshape(-1, 4)]
    for i, r in enumerate(rows):
        first.setdefault(r, i)
    order = sorted(first)
    rank = {r: v for v, r in enumerate(order)}
    return np.array([first[r] for r in order], dtype=np.int32), np.array([rank[r] for r in rows], dtype=np.int32)


def _trunc_div(c, s):
    return -(-c // s) if c < 0 else c // s


def downsample_ref(coords, strides):
    """ts_downsample: trunc(c / s) * s per axis (toward zero), the distinct rows in ascending (b, x, y, z) order"""
    sx, sy, sz = (int(s) for s in strides)
    rows = {(int(b), _trunc_div(int(x), sx) * sx, _trunc_div(int(y), sy) * sy, _trunc_div(int(z), sz) * sz)
            for x, y, z, b in np.asarray(coords).reshape(-1, 4)}
    return np.array([[x, y, z, b] for b, x, y, z in sorted(rows)], dtype=np.int32).reshape(-1, 4)


def voxel_coords_ref(points, voxel_size, batch_idx=None, n_batch=1, shift=None):
    """ts_voxel_coords: int32(np.round(xyz / voxel_size)) in float32 (half to even), minus the minimum of the row's sample over
    the rows whose batch index is in [0, n_batch) - or minus a given shift; a row outside that range is rounded, not shifted and
    not counted; a sample without rows keeps MIN_FILL.  Returns (coords [n, 4], shift actually used [n_batch, 3])."""
    p = np.asarray(points, dtype=np.float32)
    q = np.round(p[:, :3] / np.float32(voxel_size)).astype(np.int32)
    b = np.zeros(len(p), np.int32) if batch_idx is None else np.asarray(batch_idx, dtype=np.int32)
    if shift is None:
        use = np.full((n_batch, 3), MIN_FILL, np.int32)
        for i in range(len(p)):
            if 0 <= b[i] < n_batch:
                use[b[i]] = np.minimum(use[b[i]], q[i])
    else:
        use = np.asarray(shift, dtype=np.int32)
    out = np.concatenate([q, b[:, None]], 1)
    for i in range(len(p)):
        if 0 <= b[i] < n_batch:
            out[i, :3] -= use[b[i]]
    return out, use


def segment_min_ref(points, seg, n_seg):
    """ts_segment_min3: per segment the minimum of x, y, z over its rows; NaN never wins; +inf where nothing finite arrived; a
    segment id outside [0, n_seg) belongs to no segment"""
    p = np.asarray(points, dtype=np.float32)
    out = np.full((n_seg, 3), np.inf, np.float32)
    for i, s in enumerate(np.asarray(seg, dtype=np.int64).tolist()):
        if 0 <= s < n_seg:
            for d in range(3):
                if p[i, d] < out[s, d]:                # (False for NaN)
                    out[s, d] = p[i, d]
    return out


def count_ref(idx, n_out):
    out = np.zeros(n_out, np.int32)
    for v in np.asarray(idx).tolist():
        if 0 <= v < n_out:
            out[v] += 1
    return out


KM_BLOCK, KM_WAVE = 256, 64      # rows per workgroup / per wave of the compaction (csrc/coords.hip)


def kmap_ref(in_coords, out_coords, offsets, flaw=None):
    """ts_build_kmap.  A dict keyed on the coordinate tuple (x, y, z, b) holds the LOWEST row of every input coordinate; for every
    offset k and output row j the input row at out[j] + offsets[k] (or -1) is nbr[k, j]; the pairs (in, out) with a hit, ordered
    by (k, out), are nbmaps; nbsizes / nboffs count them per offset; nbr_t[k, in] = out and pos_in[k, in] = the pair's row
    (-1 without a pair; the LAST pair in that order where an input row has several - `contested` names those entries);
    pos_out[k, out] = the pair's row or -1.

    `flaw` builds the two broken compactions the host tests' teeth cases need: "lane63" loses the hit of lane 63 of every wave,
    "wave_rank" ranks the hits of every wave of a 256-row block from the block's base."""
    in_coords = np.asarray(in_coords, dtype=np.int64).reshape(-1, 4)
    out_coords = np.asarray(out_coords, dtype=np.int64).reshape(-1, 4)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    n_in, n_out, K = len(in_coords), len(out_coords), len(offsets)
    where = {}
    for i, c in enumerate(in_coords.tolist()):
        where.setdefault(tuple(c), i)
    nbr = np.full((K, n_out), -1, np.int32)
    for k, (ox, oy, oz) in enumerate(offsets.tolist()):
        for j, (x, y, z, b) in enumerate(out_coords.tolist()):
            nbr[k, j] = where.get((x + ox, y + oy, z + oz, b), -1)
    nbsizes = np.zeros(K, np.int32)
    pos_out = np.full((K, n_out), -1, np.int32)
    at = 0
    for k in range(K):
        hits = [j for j in range(n_out) if nbr[k, j] >= 0 and not (flaw == "lane63" and j % KM_WAVE == KM_WAVE - 1)]
        nbsizes[k] = len(hits)
        for rank, j in enumerate(hits):
            pos_out[k, j] = at + rank
            if flaw == "wave_rank":
                in_block = [h for h in hits if h // KM_BLOCK == j // KM_BLOCK]
                before_block = sum(1 for h in hits if h // KM_BLOCK < j // KM_BLOCK)
                pos_out[k, j] = at + before_block + sum(1 for h in in_block if h // KM_WAVE == j // KM_WAVE and h < j)
        at += len(hits)
    nboffs = np.concatenate([[0], np.cumsum(nbsizes)]).astype(np.int32)
    nbmaps = np.full((int(nboffs[-1]), 2), -1, np.int32)
    nbr_t = np.full((K, n_in), -1, np.int32)
    pos_in = np.full((K, n_in), -1, np.int32)
    for k in range(K):
        for j in range(n_out):
            p = pos_out[k, j]
            if p >= 0:
                nbmaps[p] = (nbr[k, j], j)
                nbr_t[k, nbr[k, j]] = j
                pos_in[k, nbr[k, j]] = p
    return dict(nbr=nbr, nbmaps=nbmaps, nbsizes=nbsizes, nboffs=nboffs, nbr_t=nbr_t, pos_out=pos_out, pos_in=pos_in)


KMAP_TABLES = ("nbr", "nbmaps", "nbsizes", "nboffs", "nbr_t", "pos_out", "pos_in")


def contested(ref, n_in):
    """[K, n_in] bool: the entries of nbr_t / pos_in that more than one pair writes (an output coordinate held twice) - which
    pair's value stays there is not defined"""
    K = len(ref["nbsizes"])
    cnt = np.zeros((K, n_in), np.int64)
    for k in range(K):
        seg = ref["nbmaps"][ref["nboffs"][k]:ref["nboffs"][k + 1]]
        np.add.at(cnt[k], seg[:, 0], 1)
    return cnt > 1


def same_tables(a, b):
    return all(np.array_equal(a[t], b[t]) for t in KMAP_TABLES)


# ------------------------------------------------------------------------------------------------ the cases, shared by both test files
def offsets_for(K):
    """the offset lists of the given length: cubes and 2x2x2 from get_kernel_offsets, 10 and 28 = 9 and 27 plus one row, 3 = a line"""
    sizes = {1: 1, 8: 2, 9: (3, 3, 1), 27: 3, 125: 5, 343: 7}
    if K in sizes:
        return O.get_kernel_offsets(sizes[K]).astype(np.int32)
    if K == 3:
        return np.array([[-1, 0, 0], [0, 0, 0], [1, 0, 0]], np.int32)
    extra = {10: [2, 0, 0], 28: [2, 2, 2]}[K]
    return np.concatenate([offsets_for(K - 1), np.array([extra], np.int32)])


def blob(n, seed=0, side=8, batches=2):
    """n distinct voxels of a dense side^3 cube in `batches` samples, in shuffled order"""
    rs = np.random.RandomState(seed)
    cells = rs.choice(batches * side ** 3, n, replace=False)
    b, cells = cells // side ** 3, cells % side ** 3
    return np.concatenate([np.stack(np.unravel_index(cells, (side,) * 3), 1), b[:, None]], 1).astype(np.int32)


LINE_ROWS = (1, 63, 64, 65, 255, 256, 257, 513)
LANE_PATTERNS = ("no_rows", "disjoint", "every", "lane0", "lane63", "lane64", "lane255", "block1_first", "alternate", "wave1")


def line(n_out):
    """output rows on a line: row j sits at x = j - 7, so its lane, wave and block are known"""
    c = np.zeros((n_out, 4), np.int32)
    c[:, 0] = np.arange(n_out) - 7
    return c


def lane_rows(pattern, n_out):
    """the output rows whose coordinate is also an input row (the rows with a hit at the centre offset), or None where the line
    is too short to have such a row"""
    j = np.arange(n_out)
    rows = {"no_rows": j[:0], "disjoint": j[:0], "every": j, "lane0": j[j % KM_BLOCK == 0], "lane63": j[j % KM_BLOCK == 63],
            "lane64": j[j % KM_BLOCK == 64], "lane255": j[j % KM_BLOCK == 255], "block1_first": j[j == KM_BLOCK],
            "alternate": j[j % 2 == 0], "wave1": j[(j >= 64) & (j < 128)] if n_out > 64 else j[:64]}[pattern]
    return rows if len(rows) or pattern in ("no_rows", "disjoint") else None


def lane_case(pattern, n_out):
    """(in_coords, out_coords) of one lane pattern; the inputs in shuffled order"""
    out = line(n_out)
    rows = lane_rows(pattern, n_out)
    if rows is None:
        return None
    if pattern == "disjoint":
        away = line(min(n_out, 70))
        away[:, 1] = 5
        return away, out
    return out[np.random.RandomState(n_out).permutation(rows)], out


def edge_coords():
    """coordinates within 2 of the ends of int32 on one axis at a time (an offset of +-1 does not wrap), batch 0 and 2^31 - 1"""
    hi, lo = (1 << 31) - 1, -(1 << 31)
    rows = []
    for b in (0, hi):
        for axis in range(3):
            for base in (hi - 2, hi - 1, lo + 1, lo + 2):
                for u in (0, 1, 2):
                    for v in (0, 1, 2):
                        c = [u, v]
                        c.insert(axis, base)
                        rows.append(c + [b])
    c = np.unique(np.array(rows, dtype=np.int64), axis=0)
    return c[np.random.RandomState(6).permutation(len(c))].astype(np.int32)


QUERY_CASES = ("n1", "n200", "n511", "n512", "thrice", "minus1")


@functools.lru_cache(maxsize=None)
def query_case(name):
    """(refs, ref_idx or None, queries) of one ts_hash_query case: the references are tail keys in shuffled order, the queries
    every reference, `probe_into` misses and random misses.  "thrice": 170 keys three times each with an explicit ref_idx;
    "minus1": the key -1 among the references and the queries."""
    rs = np.random.RandomState(len(name) * 131 + sum(map(ord, name)))
    n = {"n1": 1, "n200": 200, "n511": 511, "n512": 512, "thrice": 170, "minus1": 199}[name]
    total = {"thrice": 3 * n, "minus1": n + 1}.get(name, n)
    mask = capacity(total) - 1
    keys = tail_keys(n, mask)
    refs = np.concatenate([keys] * 3) if name == "thrice" else keys
    refs = refs[rs.permutation(len(refs))]
    if name == "minus1":
        refs = np.insert(refs, 77, -1)
    ref_idx = rs.randint(0, 1 << 40, len(refs)).astype(np.int64) if name == "thrice" else None
    misses = np.setdiff1d(_random_keys(300)[:100], keys)
    into = probe_into(keys, mask, 50) if n > 1 else np.zeros(0, np.int64)
    queries = np.concatenate([refs, into, misses, np.full(1 if name == "minus1" else 0, -1, np.int64)])
    assert queries.dtype == np.int64
    return refs, ref_idx, queries[rs.permutation(len(queries))]


COLLISION_ROWS = (200, 511)


@functools.lru_cache(maxsize=None)
def collision_case(n):
    """(in_coords, out_coords) of one ts_build_kmap collision case: tail coordinates of a 1024-slot table in shuffled order; the
    outputs are the inputs in another order followed by `probe_into` coordinates"""
    rs = np.random.RandomState(n)
    mask = capacity(n) - 1
    c = tail_coords(n, mask)
    return c[rs.permutation(n)], np.concatenate([c[rs.permutation(n)], probe_into(c, mask, 40)])


def unique_tail_case():
    """300 tail keys of a 1024-slot table, 200 of them a second time, shuffled: the chain ts_unique_i64's inverse walks"""
    keys = tail_keys(300, 1023)
    keys = np.concatenate([keys, keys[:200]])
    assert capacity(len(keys)) == 1024
    return keys[np.random.RandomState(8).permutation(len(keys))]
