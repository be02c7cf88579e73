"""The class-sorted implicit GEMM - ts_conv_class_plan[_pairs], ts_conv_nbr_transposed, ts_conv_class_gemm[_f16], pass 2 on the plan's
position table and ts_conv_class_conv[_f16] - against float64 (oracle/class64.py) on hand-made neighbour tables (-m gpu).

Every element is compared.  Every check of a case is evaluated; the case fails with the list of those that missed and prints one line
of worst error / bar per stage (profiles/class_float64.txt keeps a run's lines).  Every bar is computed from the inputs and the
float64 reference, never from a kernel's output; oracle/class64.py derives them from the kernels' own order, and
tests/test_class64_host.py shows on the same cases that a float32 emulation stays inside them and that twelve wrong kernels do not.
Pass 2 and the finish receive the device's own Z', cast up unchanged.

The walk through a case is class64.run_case (the host file runs the same walk on its emulation); this file supplies the calls.
Every call goes through the C ABI on buffers of this file: Z' and every result have 256 guard rows behind them (0x4B1D4B1D) that must
keep their bits, and hold NaN or 7.0 before the launch - a result never depends on what its buffer held.

No case hands a kernel an index outside its arrays: class64.check_plan compares the device's plan with the expected one, element by
element and every index against its range, before the first product launch on it, and nothing is launched on a plan that missed;
every buffer has the size its entry point documents.

The weight-gradient sum that rides on a launch (`side` of ts_conv_class_gemm_ex) and the block calls of csrc/block.hip:
oracle/block64.py and tests/test_gpu_block_float64.py (tests/test_block64_host.py on the CPU)."""
import numpy as np
import pytest
import torch

from oracle import class64 as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND = 256
BAND_BITS = 0x4B1D4B1D
TS_ERR_INVALID_ARGUMENT, TS_ERR_UNSUPPORTED = -1, -4


def _L():
    from taseg_amd import _lib as L
    return L, L.load()


def T(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def bits_t(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def buffer(rows, c, dtype, fill=0):
    """[rows + BAND, c]: NaN (fill 0) or 7.0 (fill 1) in the rows the call owns, the band pattern behind them"""
    z = torch.full((rows + BAND, c), [float("nan"), 7.0][fill], dtype=dtype, device=DEV)
    bits_t(z)[rows:] = BAND_BITS if dtype == torch.float32 else BAND_BITS & 0xFFFF
    return z


def band_kept(z, rows):
    return bool((bits_t(z)[rows:] == (BAND_BITS if z.dtype == torch.float32 else BAND_BITS & 0xFFFF)).all())


class Device:
    """the calls of class64.run_case on the device; plans keep their device arrays under "dev" """

    def __init__(self):
        self.ck = None

    def _plan(self, dev, n, k, groups):
        p = {key: (None if t is None else H(t)) for key, t in dev.items()}
        direct = dev["rows"] is not None
        p = {key: v for key, v in p.items() if v is not None}
        p.update(dev=dev, m_pad=dev["src"].shape[1], n=n, K=k, groups=groups, direct=direct)
        return p

    def plan(self, nbr, groups, direct):
        L, lib = _L()
        k, n = nbr.shape
        m_pad = int(lib.ts_conv_class_rows2(n, groups))
        assert m_pad == groups * K.npad_of(n)
        i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)  # noqa: E731
        dev = dict(src=i32(k // groups, m_pad), tile_info=i32(max(m_pad // 128, 1), 2), n_tiles=i32(2),
                   pos=None if direct else i32(groups, n), rows=i32(m_pad) if direct else None)
        ws = L.workspace(lib.ts_conv_class_plan_workspace_bytes(n), torch.device(DEV))
        table = T(nbr)                                                     # (named: an operand lives until its call has been made)
        L.check(lib.ts_conv_class_plan(L.ptr(table), n, k, groups, L.ptr(dev["src"]), L.ptr(dev["tile_info"]), L.ptr(dev["n_tiles"]),
                                       L.ptr(dev["pos"]), L.ptr(dev["rows"]), L.ptr(ws), ws.numel(), L.stream()), "ts_conv_class_plan")
        return self._plan(dev, n, k, groups)

    def plan_pairs(self, nbmaps, nboffs, k, n_pairs):
        L, lib = _L()
        m_pad = int(lib.ts_conv_class_rows2(n_pairs, 1))
        i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)  # noqa: E731
        dev = dict(src=i32(k, m_pad), tile_info=i32(max(m_pad // 128, 1), 2), n_tiles=i32(2), pos=None, rows=i32(m_pad))
        ws = L.workspace(4 * (m_pad // 128) + 256, torch.device(DEV))
        pairs, offs = T(nbmaps), T(nboffs)
        L.check(lib.ts_conv_class_plan_pairs(L.ptr(pairs), L.ptr(offs), k, n_pairs, L.ptr(dev["src"]), L.ptr(dev["tile_info"]),
                                             L.ptr(dev["n_tiles"]), L.ptr(dev["rows"]), L.ptr(ws), ws.numel(), L.stream()),
                "ts_conv_class_plan_pairs")
        return self._plan(dev, int(n_pairs), k, 1)

    def nbr_transposed(self, pos_in, nbmaps, k):
        L, lib = _L()
        out = torch.full(pos_in.shape, -7, dtype=torch.int32, device=DEV)
        positions, pairs = T(pos_in), T(nbmaps)
        L.check(lib.ts_conv_nbr_transposed(L.ptr(positions), L.ptr(pairs), k, pos_in.shape[1], L.ptr(out), L.stream()),
                "ts_conv_nbr_transposed")
        return H(out)

    def gemm_rc(self, xd, wd, plan, transposed, z):
        """the raw call: its return code"""
        L, lib = _L()
        d = plan["dev"]
        c_red = xd.shape[1]
        c = wd.shape[1] if transposed else wd.shape[2]
        assert (wd.shape[2] if transposed else wd.shape[1]) == c_red and z.shape[1] == c
        fn = lib.ts_conv_class_gemm_f16 if xd.dtype == torch.float16 else lib.ts_conv_class_gemm
        return fn(L.ptr(xd), c_red, L.ptr(wd), plan["K"], plan["groups"], c, L.ptr(d["src"]), plan["m_pad"], L.ptr(d["tile_info"]),
                  L.ptr(d["n_tiles"]), int(transposed), int(transposed and not plan["direct"]), L.ptr(d["rows"]), L.ptr(z), L.stream())

    def gemm(self, x, w, plan, transposed, fill=0):
        L, lib = _L()
        xd, wd = T(x), T(w)
        rows = plan["n"] if plan["direct"] else plan["m_pad"]
        z = buffer(rows, w.shape[1] if transposed else w.shape[2], xd.dtype, fill)
        L.check(self.gemm_rc(xd, wd, plan, transposed, z), "ts_conv_class_gemm")
        self.ck.true("band", "ts_conv_class_gemm wrote behind its rows", band_kept(z, rows))
        return H(z[:rows])

    def gather_sum(self, z, plan):
        L, lib = _L()
        zd, n = T(z), plan["n"]
        out = buffer(n, z.shape[1], zd.dtype, 0)
        fn = lib.ts_conv_gather_sum_f16 if zd.dtype == torch.float16 else lib.ts_conv_gather_sum
        L.check(fn(L.ptr(zd), z.shape[1], L.ptr(plan["dev"]["pos"]), plan["groups"], n, z.shape[0], L.ptr(out), L.stream()), "ts_conv_gather_sum")
        self.ck.true("band", "ts_conv_gather_sum wrote behind its rows", band_kept(out, n))
        return H(out[:n])

    def conv_rc(self, xd, wd, plan, transposed, ad, zp, out):
        """the raw call: its return code"""
        L, lib = _L()
        d, c = plan["dev"], wd.shape[1] if transposed else wd.shape[2]
        assert (wd.shape[2] if transposed else wd.shape[1]) == xd.shape[1] and zp.shape[1] == c and out.shape[1] == c
        assert ad is None or tuple(ad.shape) == (plan["n"], c)
        fn = lib.ts_conv_class_conv_f16 if xd.dtype == torch.float16 else lib.ts_conv_class_conv
        return fn(L.ptr(xd), xd.shape[1], L.ptr(wd), plan["K"], plan["groups"], c, L.ptr(d["src"]), plan["m_pad"], L.ptr(d["tile_info"]),
                  L.ptr(d["n_tiles"]), int(transposed), int(transposed), L.ptr(d["pos"]), plan["n"], L.ptr(ad), L.ptr(zp), L.ptr(out), L.stream())

    def conv(self, x, w, plan, transposed, addend, fill=0):
        L, lib = _L()
        xd, wd, ad = T(x), T(w), T(addend)
        n, c = plan["n"], w.shape[1] if transposed else w.shape[2]
        zp, out = buffer(plan["m_pad"], c, xd.dtype, fill), buffer(n, c, xd.dtype, fill)
        L.check(self.conv_rc(xd, wd, plan, transposed, ad, zp, out), "ts_conv_class_conv")
        self.ck.true("band", "ts_conv_class_conv wrote behind Z' or the result", band_kept(zp, plan["m_pad"]) and band_kept(out, n))
        return H(out[:n])

    def two_pass(self, x, w, nbmaps, nboffs, pos, gather_col, transposed):
        from taseg_amd import backend as B
        z = B.conv_pair_gemm(T(x), T(w), T(nbmaps), T(nboffs), int(nboffs[-1]), gather_col, weight_transposed=transposed)
        return H(B.conv_gather_sum(z, T(pos), pos.shape[1]))


# -------------------------------------------------------------------------------------------------------------- the stages

@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_stages(case):
    """the plan; the forward and the weight_transposed product (mirror = 1 on the pass-2 plans, the per-direction plans on the direct
    ones) in fp32 and half, every operand family; pass 2; ts_conv_class_conv[_f16] with and without an addend"""
    ck = K.Checks(K.case_id(case), "class_float64")
    K.run_case(ck, case, Device())
    ck.done()


@pytest.mark.parametrize("case", [(t, c) for t in K.EDGE_TABLES for c in K.FEW_CHANNELS], ids=K.case_id)
def test_contracts(case):
    """the same launch twice and a freshly built plan give the same bits; NaN in input row 0 - the row a dead slot would read - and in
    a row that three offsets list appears in exactly the Z' and result rows whose src lists that row"""
    name, (c_red, c_out) = case
    ck = K.Checks("contracts " + K.case_id(case), "class_float64")
    K.run_contracts(ck, name, c_red, c_out, Device())
    ck.done()


def off_boundary(a, elements):
    """the same values, contiguous, starting `elements` elements into a flat buffer: 4 bytes off a 16-byte boundary"""
    flat = torch.zeros(a.size + 8, dtype=torch.float16 if a.dtype == np.float16 else torch.float32, device=DEV)
    view = flat[elements:elements + a.size].view(a.shape)
    view.copy_(T(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("name", K.EDGE_TABLES)
def test_refused_calls_launch_nothing(name):
    """operands off a 16-byte boundary (feat, kernel, Z'; the result and the addend of ts_conv_class_conv): TS_ERR_INVALID_ARGUMENT; channel pairs the kernels do not take (c_red 48, c_out 20, 24) and a K
    that does not split into groups of at most nine: TS_ERR_UNSUPPORTED - and Z' keeps what it held"""
    L, lib = _L()
    nbr, n_in, groups, _ = K.table(name)
    drv, ck = Device(), K.Checks("refused " + name, "class_float64")
    drv.ck = ck
    plan = drv.plan(nbr, groups, False)
    assert K.check_plan(ck, nbr, groups, plan, False, n_in)
    untouched = lambda z: bool(torch.isnan(z[:plan["m_pad"]]).all()) and band_kept(z, plan["m_pad"])  # noqa: E731
    for half in (False, True):
        for transposed in (False, True):
            for c_red, c_out in K.FEW_CHANNELS:
                x, w = K.operands("dense", n_in, 27, c_red, c_out, transposed, half)
                xd, wd, step = T(x), T(w), 2 if half else 1
                z = buffer(plan["m_pad"], c_out, xd.dtype)
                for what, args in (("feat", (off_boundary(x, step), wd, z)), ("kernel", (xd, off_boundary(w, step), z)),
                                   ("Z'", (xd, wd, off_boundary(H(z), step)))):
                    rc = drv.gemm_rc(args[0], args[1], plan, transposed, args[2])
                    ck.true("refused", f"{what} off the boundary, half={half}: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
                ck.true("refused", "a refused call wrote to Z'", untouched(z))
                # ts_conv_class_conv[_f16]: its two further operands, the result and the addend
                n = plan["n"]
                out = buffer(n, c_out, xd.dtype)
                add = torch.ones((n, c_out), dtype=xd.dtype, device=DEV)
                for what, ad, res in (("the result", add, off_boundary(H(out), step)), ("the result, no addend", None, off_boundary(H(out), step)),
                                      ("the addend", off_boundary(H(add), step), out)):
                    rc = drv.conv_rc(xd, wd, plan, transposed, ad, z, res)
                    ck.true("refused", f"ts_conv_class_conv, {what} off the boundary, half={half}: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
                ck.true("refused", "a refused ts_conv_class_conv wrote to Z' or the result",
                        untouched(z) and bool(torch.isnan(out[:n]).all()) and band_kept(out, n))
            for c_red, c_out in K.REFUSED_CHANNELS:
                dt = torch.float16 if half else torch.float32
                xd = torch.ones((n_in, c_red), dtype=dt, device=DEV)
                wd = torch.ones((27, c_out, c_red) if transposed else (27, c_red, c_out), dtype=dt, device=DEV)
                z = buffer(plan["m_pad"], c_out, dt)
                rc = drv.gemm_rc(xd, wd, plan, transposed, z)
                ck.true("refused", f"{c_red} -> {c_out}, half={half}: code {rc}", rc == TS_ERR_UNSUPPORTED and untouched(z))
                ck.true("refused", f"ts_conv_class_supported({c_red}, {c_out})", lib.ts_conv_class_supported(c_red, c_out) == 0)
            # K = 27 in one group, K = 26 in three: no split into groups of at most nine
            x, w = K.operands("dense", n_in, 27, 32, 32, transposed, half)
            xd, wd = T(x), T(w)
            z = buffer(plan["m_pad"], 32, xd.dtype)
            for k_vol, grp in ((27, 1), (26, 3), (30, 3)):
                bad = dict(plan, K=k_vol, groups=grp)
                rc = drv.gemm_rc(xd, wd, bad, transposed, z)
                ck.true("refused", f"K {k_vol} in {grp} groups, half={half}: code {rc}", rc == TS_ERR_UNSUPPORTED and untouched(z))
    d = plan["dev"]
    ws = L.workspace(lib.ts_conv_class_plan_workspace_bytes(nbr.shape[1]), torch.device(DEV))
    before = H(d["src"]).copy()
    table = T(nbr)
    for k_vol, grp in ((27, 1), (26, 3), (30, 3)):
        rc = lib.ts_conv_class_plan(L.ptr(table), nbr.shape[1], k_vol, grp, L.ptr(d["src"]), L.ptr(d["tile_info"]), L.ptr(d["n_tiles"]),
                                    L.ptr(d["pos"]), None, L.ptr(ws), ws.numel(), L.stream())
        ck.true("refused", f"ts_conv_class_plan, K {k_vol} in {grp} groups: code {rc}", rc == TS_ERR_UNSUPPORTED)
    ck.true("refused", "a refused plan call wrote to src", np.array_equal(H(d["src"]), before))
    ck.done()


# -------------------------------------------------------------------------------------------------------------------- LONG

def test_the_half_kernels_persistent_walk():
    """LONG: 32 -> 32 half rows on a three-group table with at least 2 * 8 * cus + 1 listed tiles - more than two rounds of the largest
    grid the launch can size (a CU holds at most 8 workgroups of 256 threads), so every slot walks forward, reversed and forward again.
    Z' is NaN before the launch: a tile that is skipped shows, and so does one that another slot's reversed round should have run.
    The reference and the comparison run in chunks of 256 tiles."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nbr, tiles = K.long_table(cus)
    n = nbr.shape[1]
    drv, ck = Device(), K.Checks("LONG", "class_float64")
    drv.ck = ck
    plan = drv.plan(nbr, 3, False)
    assert K.check_plan(ck, nbr, 3, plan, False, n), ck.missed
    listed, steps = (int(v) for v in plan["n_tiles"])
    assert listed >= tiles and listed == plan["m_pad"] // 128
    print(f"class_float64 LONG: cus {cus}, rows {n}, listed tiles {listed} (>= 2 * 8 * cus + 1 = {tiles}), plan steps {steps}")
    slot_row = K.plan64(nbr, 3, False)["rows"]                            # the row of every slot (check_plan held pos to the same list)
    for transposed in (False, True):
        x, w = K.operands("dense", n, 27, 32, 32, transposed, True)
        x64, w64 = K.f64(x), K.f64(w)
        z = drv.gemm(x, w, plan, transposed)
        what = "transposed, mirror" if transposed else "forward"
        for t0 in range(0, plan["m_pad"] // 128, 256):
            t1 = min(t0 + 256, plan["m_pad"] // 128)
            for g in range(3):                                            # a chunk may straddle two groups
                lo, hi = max(t0, g * (n // 128)), min(t1, (g + 1) * (n // 128))
                if lo >= hi:
                    continue
                slots = np.arange(lo * 128, hi * 128)
                ref = K.class_gemm64(x64, w64, nbr, 3, transposed, transposed, rows=slot_row[slots], group=g)
                K.check_product(ck, "class_half", f"{what} tiles {lo}..{hi - 1}", z[slots], ref.z[0], K.bar_class_half(ref)[0], ref.L[0])
    ck.done()
