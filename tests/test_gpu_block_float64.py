"""The fused conv-block calls of csrc/block.hip - ts_conv_block_forward, ts_conv_block_backward (with ts_conv_block_wgrad_side) and
ts_conv_block_eval - against float64 (oracle/block64.py) on the hand-made rulebooks and neighbour tables of oracle/conv64.py and
oracle/class64.py (-m gpu).

Every element is compared.  Every check of a case is evaluated; the case fails with the list of those that missed and prints one line
of worst error / bar per stage (profiles/block_float64.txt keeps a run's lines).  Every bar is computed from the inputs and the
float64 reference, never from a kernel's output; oracle/block64.py composes them from the bars of the kernels a call launches, and
tests/test_block64_host.py shows on the same cases that the reference agrees with autograd in double, that a float32 / half emulation
of the calls stays inside every bar and that twelve wrong calls do not.  Every stage receives the device's own previous stage, cast
up unchanged; the gradient w.r.t. the convolution output, no output of the call, comes from ts_bn_act_train_backward[_f16] on the
same operands (second stream: also from the head of wgrad_ws, the same bits).

Every call goes through the C ABI on buffers of this file.  Every output has 256 guard rows behind it (0x4B1D4B1D) and holds NaN on
one run and 7.0 on the other; the workspace has exactly ts_conv_block_workspace_bytes(...) bytes, wgrad_ws exactly
ts_conv_block_wgrad_ws_bytes(...), each with a guard band and the same two prefills.  The two runs must give the same bits - but for
grad_kernel in the atomic form of the weight gradient, whose float atomics land in the order the workgroups finish (the header says so
of ts_conv_wgrad; one device run in three showed other last bits): there both runs are held to the float64 bars.  A
third, profiled run is held to the launches its route consists of (block64.expected_kinds): a call that quietly falls back to the two
passes does not pass as a class-plan case.

No case hands a kernel an index outside its arrays: conv64.check_rulebook runs on every rulebook and class64.check_plan on every plan
before the first launch on it, and nothing is launched on a plan that missed."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import block64 as B
from oracle import class64 as K
from oracle import conv64 as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND = 256
TS_ERR_INVALID_ARGUMENT = -1
SLOT = 3                                       # the ring slot of the second-stream cases


def _L():
    from taseg_amd import _lib as L
    return L, L.load()


def T(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def H(t):
    return None if t is None else t.detach().cpu().numpy()


class Buf:
    """a buffer of exactly `shape` elements that starts `off` bytes into its allocation, the band pattern (0x4B1D...) in front of and
    behind it (256 rows behind); the elements hold `init`, or NaN (all bits set; fill 0) or 7.0 (fill 1)"""

    def __init__(self, shape, dtype, fill=0, off=0, init=None):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        body = int(np.prod(shape)) * item
        row = max(int(np.prod(shape[1:])) * item, item)
        total = off + body + BAND * row
        total += total % 2
        self.raw = torch.tensor([0x1D, 0x4B], dtype=torch.uint8, device=DEV).repeat(total // 2)
        self.lo, self.hi = off, off + body
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(init)
        elif fill == 0:
            self.raw[self.lo:self.hi] = 0xFF
        elif dtype == torch.uint8 and body % 4 == 0 and len(shape) == 1 and body >= 256:      # scratch: floats of 7.0
            self.raw[self.lo:self.hi].view(torch.float32).fill_(7.0)
        else:
            self.t.fill_(7)
        self.guard = torch.cat([self.raw[:self.lo], self.raw[self.hi:]]).clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def nbytes(self):
        return self.hi - self.lo

    def kept(self):
        return bool(torch.equal(torch.cat([self.raw[:self.lo], self.raw[self.hi:]]), self.guard))

    def host(self):
        return H(self.t)


def dtype_of(half):
    return torch.float16 if half else torch.float32


@contextlib.contextmanager
def library_state(impl=0, finish=False, tail_option=True):
    """conv_impl, the finish thresholds and eval_tail_in_pass2 for the calls inside; the defaults again afterwards"""
    from taseg_amd import backend
    from taseg_amd.options import options
    L, lib = _L()
    kw = dict(eval_tail_in_pass2=bool(tail_option))
    if finish:
        kw.update(class_finish_rows=1, class_finish_rows_half=1)
    with options.override(**kw):
        L.push_options()
        backend.set_conv_impl(impl)
        try:
            assert bool(lib.ts_conv_class_finish_pays(1000, 0)) == bool(finish) and bool(lib.ts_conv_class_finish_pays(1000, 1)) == bool(finish)
            yield
        finally:
            backend.set_conv_impl(0)
    L.push_options()


# ------------------------------------------------------------------------------------------------------------------- plans

def build_plan(ck, nbr, groups, direct, n_in, mirror, map_id):
    """ts_conv_class_plan on a table, checked element by element (class64.check_plan) before anything is launched on it: the dict
    backend.class_plan_struct takes, or None where the plan missed"""
    L, lib = _L()
    k, n = nbr.shape
    m_pad = int(lib.ts_conv_class_rows2(n, groups))
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)  # noqa: E731
    dev = dict(src=i32(k // groups, m_pad), tile_info=i32(max(m_pad // 128, 1), 2), n_tiles=i32(2),
               pos=None if direct else i32(groups, n), rows=i32(m_pad) if direct else None)
    ws = torch.empty(int(lib.ts_conv_class_plan_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    table = T(nbr)
    L.check(lib.ts_conv_class_plan(L.ptr(table), n, k, groups, L.ptr(dev["src"]), L.ptr(dev["tile_info"]), L.ptr(dev["n_tiles"]),
                                   L.ptr(dev["pos"]), L.ptr(dev["rows"]), L.ptr(ws), ws.numel(), L.stream()), "ts_conv_class_plan")
    torch.cuda.synchronize()
    host = {key: H(t) for key, t in dev.items() if t is not None}
    host["m_pad"] = m_pad
    if not K.check_plan(ck, nbr, groups, host, direct, n_in):
        return None
    return dict(dev, n=n, m_pad=m_pad, z_rows=0, K=k, groups=groups, mirror=mirror, map_id=map_id)


def plans_for(ck, cs, bk, sd, d_nboffs):
    """(forward plan, input-gradient plan) of a case, as the product builds them: ONE mirrored plan on a submanifold table, the direct
    plans of the two directions on a strided one.  spoil: map_id names another kernel map; the plan is built for one row less"""
    if not (cs["plan_f"] or cs["plan_d"]):
        return None, None, True
    map_id = torch.zeros(bk.k + 1, dtype=torch.int32, device=DEV) if cs["spoil"] == "map_id" else d_nboffs
    cut = (lambda t: np.ascontiguousarray(t[:, :-1])) if cs["spoil"] == "rows" else (lambda t: t)
    if bk.kind == "sub":
        p = build_plan(ck, cut(bk.nbr), 3, False, bk.n_in, 1, map_id)
        pf = pd = p
    else:
        pf = build_plan(ck, cut(sd["nbr_f"]), 1, True, sd["n_feat"], 0, map_id)
        pd = build_plan(ck, cut(sd["nbr_d"]), 1, True, sd["n_out"], 0, map_id)
    ok = pf is not None and pd is not None
    return (pf if cs["plan_f"] else None), (pd if cs["plan_d"] else None), ok


# ----------------------------------------------------------------------------------------------------------------- the calls

class Call:
    """the device side of one case: rulebook and operands uploaded once, the calls made on fresh guarded buffers"""

    def __init__(self, ck, cs, ops):
        from taseg_amd import backend
        L, lib = _L()
        self.ck, self.cs, self.ops = ck, cs, ops
        self.bk = bk = B.book(cs["book"])
        self.sd = sd = bk.sides(cs["transposed"])
        assert C.check_rulebook(bk.nbmaps, bk.nboffs, bk.pos_out, bk.pos_in, bk.n_in, bk.n_out)           # before any launch
        self.half, self.c_in, self.c_out = cs["half"], cs["c_in"], cs["c_out"]
        self.dt = dtype_of(self.half)
        self.d = {k: T(v) for k, v in ops.items() if v is not None and k != "w16"}
        self.nbmaps, self.nboffs = T(bk.nbmaps), T(bk.nboffs)
        self.pos, self.pos_d = T(sd["pos"]), T(sd["pos_dgrad"])
        self.pf, self.pd, self.plans_ok = plans_for(ck, cs, bk, sd, self.nboffs)
        self.sf = None if self.pf is None else ctypes.pointer(backend.class_plan_struct(self.pf))
        self.sdg = None if self.pd is None else ctypes.pointer(backend.class_plan_struct(self.pd))
        self.rows_max = max(sd["n_feat"], sd["n_out"], sd["n_dgrad"])
        self.ws_bytes = int(lib.ts_conv_block_workspace_bytes(bk.p, self.rows_max, self.c_in, self.c_out, bk.k, int(self.half)))
        self.wg_bytes = int(lib.ts_conv_block_wgrad_ws_bytes(bk.p, sd["n_out"], self.c_in, self.c_out, bk.k, int(self.half)))
        self.side = torch.cuda.Stream() if cs["stream"] else None
        self.planes = self.w16_kept = None
        if cs["kept"] and not self.half:         # what the caller keeps in step with the weight: the pre-split planes
            self.planes = torch.empty(3 * ops["kernel"].size, dtype=torch.int16, device=DEV)
            L.check(lib.ts_conv_split_planes(L.ptr(self.d["kernel"]), bk.k, self.c_in, self.c_out, L.ptr(self.planes), L.stream()), "ts_conv_split_planes")
        elif cs["kept"]:                         # ... the half copy (w16_current: the call casts nothing)
            self.w16_kept = T(ops["w16"])

    def opts(self, plan_f=None, plan_d=None, addend=None, wgrad_ws=None, deferred=0):
        L, _ = _L()
        side = self.side.cuda_stream if (self.side is not None and wgrad_ws is not None) else None
        return L.TsConvBlockOpts(plan_f, plan_d, L.ptr(self.planes), 0 if self.w16_kept is None else 1, L.ptr(addend), side, None if wgrad_ws is None else wgrad_ws.ptr,
                                 0 if wgrad_ws is None else wgrad_ws.nbytes, SLOT, deferred, 1 if self.cs["natural"] else 0)

    def band(self, what, bufs):
        for name, b in bufs.items():
            if b is not None:
                self.ck.true("band", f"{what}: the call wrote outside {name}", b.kept())

    def forward(self, fill, comms=(None,)):
        """ts_conv_block_forward (comms: (None,), or the two sentinels of a split call); returns the buffers"""
        L, lib = _L()
        cs, sd, bk, d = self.cs, self.sd, self.bk, self.d
        n, c = sd["n_out"], self.c_out
        ve = 8 if self.half else 4
        o = dict(conv_out=Buf((n, c), self.dt, fill), out=Buf((n, c), self.dt, fill), mean=Buf((c,), torch.float32, fill),
                 invstd=Buf((c,), torch.float32, fill), mask=Buf((n * (c // ve),), torch.uint8, fill) if cs["relu"] else None,
                 running_mean=Buf((c,), torch.float32, init=d["rm0"]), running_var=Buf((c,), torch.float32, init=d["rv0"]),
                 nbt=Buf((1,), torch.int64, init=torch.zeros(1, dtype=torch.int64, device=DEV)),
                 w16=Buf((bk.k, self.c_in, c), torch.float16, fill, init=self.w16_kept) if self.half else None,
                 pack=Buf((2 * c + 1,), torch.float64, fill) if comms != (None,) else None,
                 ws=Buf((self.ws_bytes,), torch.uint8, fill))
        opts = self.opts(plan_f=self.sf)
        p = lambda b: None if b is None else b.ptr  # noqa: E731
        for comm in comms:
            L.check(lib.ts_conv_block_forward(
                L.ptr(d["feat"]), sd["n_feat"], self.c_in, L.ptr(d["kernel"]), bk.k, L.ptr(self.nbmaps), L.ptr(self.nboffs), bk.p,
                sd["gather_col"], L.ptr(self.pos), n, c, L.ptr(d.get("residual")), L.ptr(d["bn_w"]), L.ptr(d["bn_b"]),
                o["running_mean"].ptr, o["running_var"].ptr, o["nbt"].ptr, B.EPS, B.MOMENTUM, int(cs["relu"]), int(self.half),
                None if comm is None else ctypes.c_void_p(comm), p(o["pack"]), o["conv_out"].ptr, o["mean"].ptr, o["invstd"].ptr,
                o["out"].ptr, p(o["mask"]), p(o["w16"]), ctypes.byref(opts), o["ws"].ptr, self.ws_bytes, L.stream()), "ts_conv_block_forward")
        torch.cuda.synchronize()
        self.band("forward", o)
        return o

    def bn_backward(self, f):
        """the stand-alone BatchNorm backward on the forward's own outputs: the bits of the gradient w.r.t. the convolution output"""
        L, lib = _L()
        n, c = self.sd["n_out"], self.c_out
        gx, gres = Buf((n, c), self.dt), Buf((n, c), self.dt)
        gw, gb = Buf((c,), torch.float32), Buf((c,), torch.float32)
        ws = Buf((int(lib.ts_bn_train_workspace_bytes(c)),), torch.uint8)
        fn = lib.ts_bn_act_train_backward_f16 if self.half else lib.ts_bn_act_train_backward
        L.check(fn(L.ptr(self.d["grad_out"]), None if f["mask"] is None else f["mask"].ptr, f["conv_out"].ptr, f["mean"].ptr, f["invstd"].ptr,
                   L.ptr(self.d["bn_w"]), n, c, gx.ptr, gres.ptr, gw.ptr, gb.ptr, ws.ptr, ws.nbytes, L.stream()), "ts_bn_act_train_backward")
        torch.cuda.synchronize()
        self.band("stand-alone BatchNorm backward", dict(grad_x=gx, grad_residual=gres, grad_weight=gw, grad_bias=gb, ws=ws))
        return gx

    def backward_rc(self, f, o, opts, comm=None, stream=None):
        L, lib = _L()
        cs, sd, bk, d = self.cs, self.sd, self.bk, self.d
        p = lambda b: None if b is None else b.ptr  # noqa: E731
        total_dev = None if f["pack"] is None else f["pack"].ptr + 8 * 2 * self.c_out
        return lib.ts_conv_block_backward(
            L.ptr(d["grad_out"]), p(f["mask"]), f["conv_out"].ptr, f["mean"].ptr, f["invstd"].ptr, L.ptr(d["bn_w"]), total_dev,
            None if comm is None else ctypes.c_void_p(comm), p(o.get("sums")), sd["n_out"], self.c_out, int(self.half), L.ptr(d["feat"]),
            sd["n_feat"], self.c_in, f["w16"].ptr if self.half else L.ptr(d["kernel"]), bk.k, L.ptr(self.nbmaps), L.ptr(self.nboffs), bk.p,
            sd["dgrad_gather_col"], L.ptr(self.pos_d), sd["n_dgrad"], sd["wgrad_col_a"], p(o["grad_feat"]), p(o["grad_residual"]),
            o["grad_kernel"].ptr, o["grad_bn_weight"].ptr, o["grad_bn_bias"].ptr, ctypes.byref(opts), o["ws"].ptr, self.ws_bytes,
            L.stream() if stream is None else stream)

    def backward_buffers(self, fill, gk_off=None):
        cs, sd, c = self.cs, self.sd, self.c_out
        gk_off = cs["gk_off"] if gk_off is None else gk_off
        return dict(grad_feat=Buf((sd["n_dgrad"], self.c_in), self.dt, fill) if cs["grad_feat"] else None,
                    grad_residual=Buf((sd["n_out"], c), self.dt, fill) if cs["residual"] else None,
                    grad_kernel=Buf((self.bk.k, self.c_in, c), torch.float32, fill, off=4 if gk_off else 0),
                    grad_bn_weight=Buf((c,), torch.float32, fill), grad_bn_bias=Buf((c,), torch.float32, fill),
                    sums=Buf((2 * c,), torch.float64, fill) if cs["split"] else None,
                    ws=Buf((self.ws_bytes,), torch.uint8, fill), wgrad_ws=Buf((self.wg_bytes,), torch.uint8, fill) if cs["stream"] else None)

    def backward(self, f, fill, comms=(None,)):
        L, lib = _L()
        cs, sd, bk = self.cs, self.sd, self.bk
        o = self.backward_buffers(fill)
        if cs["gk_off"]:
            assert o["grad_kernel"].ptr % 16 == 4
        deferred = cs["stream"] == "deferred"
        opts = self.opts(plan_d=self.sdg, addend=self.d.get("addend") if cs["addend"] else None, wgrad_ws=o["wgrad_ws"], deferred=int(deferred))
        owed = False
        try:
            for comm in comms:
                L.check(self.backward_rc(f, o, opts, comm), "ts_conv_block_backward")
                owed = deferred
        finally:
            if owed:                            # a deferred call is always followed by its weight gradient: no slot is left owed
                rc = lib.ts_conv_block_wgrad_side(
                    L.ptr(self.d["feat"]), sd["n_feat"], self.c_in, bk.k, L.ptr(self.nbmaps), L.ptr(self.nboffs), bk.p, sd["wgrad_col_a"],
                    sd["n_out"], self.c_out, int(self.half), o["grad_kernel"].ptr, 1 if cs["grad_feat"] else 0, o["wgrad_ws"].ptr, self.wg_bytes,
                    SLOT, self.side.cuda_stream)
            if self.side is not None:
                L.check(lib.ts_stream_join(L.stream(), self.side.cuda_stream), "ts_stream_join")
            torch.cuda.synchronize()
        if owed:
            L.check(rc, "ts_conv_block_wgrad_side")
        self.band("backward", o)
        return o

    def train(self, fill):
        """forward, the stand-alone BatchNorm backward, backward: what block64.check_training takes"""
        cs = self.cs
        comms = (1, 2) if cs["split"] else (None,)
        f = self.forward(fill, comms)
        gx = self.bn_backward(f)
        if cs["addend"] and "addend" not in self.d:
            self.ops["addend"] = B.make_addend(cs, self.ops, gx.host())
            self.d["addend"] = T(self.ops["addend"])
        b = self.backward(f, fill, comms)
        got = {k: f[k].host() if f[k] is not None else None for k in ("conv_out", "out", "mean", "invstd", "mask", "running_mean", "running_var", "w16")}
        got["nbt"] = f["nbt"].host()[0]
        got.update({k: b[k].host() if b[k] is not None else None for k in ("grad_feat", "grad_residual", "grad_kernel", "grad_bn_weight", "grad_bn_bias")})
        got["grad_conv"] = gx.host()
        if cs["stream"]:                        # the head of wgrad_ws: the gradient w.r.t. the convolution output
            n, c = self.sd["n_out"], self.c_out
            w = b["wgrad_ws"]
            got["ws_grad_conv"] = H(w.raw[w.lo:w.lo + n * c * (2 if self.half else 4)].view(self.dt).view(n, c))
        return got


_NAMES = {"pair_gemm": 0, "gather_sum": 1, "conv_wgrad": 2, "class_gemm": 3, "wgrad_reduce": 5}


def record_kinds(records):
    """the record kinds (include/taseg_hip.h) of backend.profile_end()'s list, in order.  profile_end names kinds 3 and 4 alike: the
    finish inside the product is the class GEMM that both moves Z' rows and stores result rows"""
    out = []
    for name, _, _, meta in records:
        kind = _NAMES[name]
        out.append(4 if kind == 3 and meta["z_rows"] > 0 and meta["out_rows"] > 0 else kind)
    return out


def same_bits(ck, a, b, what="the two runs (NaN and 7.0 before the launch)"):
    for key in a:
        if a[key] is None or b[key] is None:
            ck.true("bits", f"{key}: present on one run only", a[key] is None and b[key] is None)
        else:
            x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
            ck.true("bits", f"{key}: {what} differ", x.tobytes() == y.tobytes())


def run_training(cs, title="block_float64"):
    """a case: two compared runs, one profiled run held to its route, the float64 walk on the first run"""
    from taseg_amd import backend
    ck = C.Checks(B.case_id(cs), title)
    ops = B.operands(cs)
    with library_state(cs["impl"], finish="finish" in (cs["route_f"], cs["route_d"])):
        call = Call(ck, cs, ops)
        if not call.plans_ok:                   # nothing is launched on a plan that missed
            ck.done()
        runs = [call.train(fill) for fill in (0, 1)]
        # the atomic form of the weight gradient (grad_kernel off the boundary, the scalar kernels) adds its partial tiles in the order
        # the workgroups finish (include/taseg_hip.h, ts_conv_wgrad): no run-to-run bits to hold it to - both runs meet the bars instead
        atomic = cs["gk_off"] or cs["impl"] == 1
        same_bits(ck, *({k: v for k, v in r.items() if not (atomic and k == "grad_kernel")} for r in runs))
        backend.profile_begin()
        f = call.forward(0, (1, 2) if cs["split"] else (None,))
        kinds_f = record_kinds(backend.profile_end())
        backend.profile_begin()
        call.backward(f, 0, (1, 2) if cs["split"] else (None,))
        kinds_b = record_kinds(backend.profile_end())
    ck.true("route", f"forward launches {kinds_f}, expected {B.expected_kinds(cs, 'forward')}", kinds_f == B.expected_kinds(cs, "forward"))
    ck.true("route", f"backward launches {kinds_b}, expected {B.expected_kinds(cs, 'backward')}", sorted(kinds_b) == sorted(B.expected_kinds(cs, "backward"))
            and (cs["stream"] is not None or kinds_b == B.expected_kinds(cs, "backward")))
    got = runs[0]
    if cs["stream"]:
        ck.true("bits", "the head of wgrad_ws does not hold the bits of the stand-alone BatchNorm backward",
                np.array_equal(B.bits(got["ws_grad_conv"]), B.bits(got["grad_conv"])))
    B.check_training(ck, cs, ops, got)
    if atomic:
        B.check_training(ck, cs, ops, runs[1], sfx=("_half" if cs["half"] else "_f32") + " (7.0 before)")
    return ck, got, call


# ------------------------------------------------------------------------------------------------------------------ groups

@pytest.mark.parametrize("cs", B.TWO_PASS, ids=B.case_id)
def test_training_on_the_two_pass_route(cs):
    """fp32 and half; relu 0 / 1 (mask = NULL without); residual and grad_residual present or absent; grad_feat present (the ordered
    weight-gradient sum rides on pass 2) or absent (ts_wgrad_reduce); grad_kernel aligned, and 4 bytes off a 16-byte boundary - the
    atomic form with already_zero = 0, the prefill must not survive; conv_impl 1 (K-register pass 2, no riding)"""
    run_training(cs)[0].done()


@pytest.mark.parametrize("cs", B.ADDEND, ids=B.case_id)
def test_the_addend(cs):
    """the addend in the store of the input gradient: pass 2 of the two-pass route, pass 2 and the finish of a three-group plan, and a
    direct plan, which the call must decline.  Where the header states the same bits - the finish against class GEMM + pass 2, the
    addend against a separate add - they are asserted as well as the float64 bars"""
    ck, got, call = run_training(cs)
    if cs["route_d"] == "finish":               # the same call without the finish: class GEMM + pass 2
        other = dict(cs, route_d="class")
        ck2, got2, _ = run_training(other, "block_float64 (pass 2)")
        ck.true("bits", "the finish inside the product and class GEMM + pass 2 differ in grad_feat", np.array_equal(B.bits(got["grad_feat"]), B.bits(got2["grad_feat"])))
        ck.missed += ck2.missed
    # a separate add of the addend: fl(grad_feat without addend + addend), one rounding from the float32 sum - for fp32 rows that is
    # the float32 sum of the two; half rows are rounded twice by a separate add, so only fp32 is held to it
    if not cs["half"]:
        plain = dict(cs, addend=False, route_d="direct" if B.book(cs["book"]).kind == "down" else cs["route_d"])   # (no addend: the direct plan is taken)
        ckp, gotp, _ = run_training(plain, "block_float64 (no addend)")
        want = gotp["grad_feat"] + call.ops["addend"]
        ck.true("bits", "the addend in the store and a separate add differ", np.array_equal(B.bits(got["grad_feat"]), B.bits(want)))
        ck.missed += ckp.missed
    ck.done()


@pytest.mark.parametrize("cs", B.PLANS, ids=B.case_id)
def test_class_plans_inside_the_block(cs):
    """the forward plan and the mirrored input-gradient plan of the submanifold tables; the direct plans of both directions of the
    strided tables, as the strided and as the transposed block (n_dgrad_rows != n_out)"""
    run_training(cs)[0].done()


@pytest.mark.parametrize("cs", B.KEPT, ids=B.case_id)
def test_kept_planes_and_half_weights_change_no_bit(cs):
    """TsConvBlockOpts.planes (fp32: the direct-rows pair GEMM, the class GEMM's persistent walk) and w16_current (half: no cast
    inside the call): the bars, and every output bit of the call without them"""
    ck, got, _ = run_training(cs)
    ck1, got1, _ = run_training(dict(cs, kept=False), "block_float64 (nothing kept)")
    same_bits(ck, got, got1, "the call with and without what the caller keeps")
    ck.missed += ck1.missed
    if not cs["half"]:                           # that the call did read its planes: planes of zeros give another result
        call = Call(ck, cs, B.operands(cs))
        call.planes.zero_()
        junk = call.forward(0)["conv_out"].host()
        ck.true("bits", "the call did not take the planes", not np.array_equal(B.bits(junk), B.bits(got["conv_out"])))
    ck.done()


@pytest.mark.parametrize("cs", B.REFUSED_PLANS, ids=B.case_id)
def test_plans_the_call_must_decline(cs):
    """a plan of another kernel map (map_id), a plan built for another row count, a plan whose Z' does not fit where Z would have gone
    (SUB1: m_pad 384 against one pair) and channel pairs the class kernels do not take: the two passes, and a correct result"""
    run_training(cs)[0].done()


@pytest.mark.parametrize("cs", B.NATURAL, ids=B.case_id)
def test_the_natural_form(cs):
    """K = 1 on the identity rulebook: the product's rows are the result rows, in both directions"""
    run_training(cs)[0].done()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_the_natural_form_refuses_an_addend_and_K_3(half):
    """the argument errors the header promises: natural with an addend, natural with K = 3 - TS_ERR_INVALID_ARGUMENT, nothing written"""
    L, lib = _L()
    cs = B.case("ID257", 32, 32, natural=True, route_f="natural", route_d="natural", half=half)
    ck = C.Checks(B.case_id(cs) + "-refused", "block_float64")
    ops = B.operands(cs)
    call = Call(ck, cs, ops)
    f = call.forward(0)
    o = call.backward_buffers(0)
    add = torch.ones((257, 32), dtype=call.dt, device=DEV)
    rc = call.backward_rc(f, o, call.opts(addend=add))
    ck.true("refused", f"natural with an addend: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
    # K = 3: the same rows as three offsets, two of them empty
    k3 = torch.tensor([0, 257, 257, 257], dtype=torch.int32, device=DEV)
    w3 = torch.ones((3, 32, 32), dtype=torch.float32, device=DEV)
    w16 = Buf((3, 32, 32), torch.float16)
    ws = Buf((int(lib.ts_conv_block_workspace_bytes(257, 257, 32, 32, 3, int(half))),), torch.uint8)
    out = {k: Buf((257, 32), call.dt) for k in ("conv_out", "out")}
    stats = {k: Buf((32,), torch.float32) for k in ("mean", "invstd")}
    opts = call.opts()
    rc = lib.ts_conv_block_forward(
        L.ptr(call.d["feat"]), 257, 32, L.ptr(w3), 3, L.ptr(call.nbmaps), L.ptr(k3), 257, 0, L.ptr(call.pos), 257, 32, None, L.ptr(call.d["bn_w"]),
        L.ptr(call.d["bn_b"]), f["running_mean"].ptr, f["running_var"].ptr, f["nbt"].ptr, B.EPS, B.MOMENTUM, 1, int(half), None, None,
        out["conv_out"].ptr, stats["mean"].ptr, stats["invstd"].ptr, out["out"].ptr, f["mask"].ptr, w16.ptr, ctypes.byref(opts), ws.ptr, ws.nbytes,
        L.stream())
    ck.true("refused", f"natural with K = 3, forward: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
    torch.cuda.synchronize()
    for name, b in list(o.items()) + list(out.items()) + list(stats.items()):
        if b is not None and name != "ws":
            ck.true("refused", f"a refused call wrote to {name}", b.kept() and bool((b.raw[b.lo:b.hi] == 0xFF).all()))
    ck.true("refused", "a refused forward moved num_batches_tracked", int(f["nbt"].host()[0]) == 1)
    ck.done()


@pytest.mark.parametrize("cs", B.SECOND_STREAM, ids=B.case_id)
def test_the_weight_gradient_on_a_second_stream(cs):
    """wgrad_stream with the call launching the gradient itself, and wgrad_deferred followed by ts_conv_block_wgrad_side from the same
    thread; the streams joined with ts_stream_join before reading.  grad_kernel carries the bits of the one-stream form, the head of
    wgrad_ws those of the stand-alone BatchNorm backward"""
    ck, got, _ = run_training(cs)
    ck1, got1, _ = run_training(dict(cs, stream=None), "block_float64 (one stream)")
    for key in ("grad_kernel", "grad_feat", "grad_residual", "grad_bn_weight", "grad_bn_bias"):
        if got[key] is not None:
            ck.true("bits", f"{key}: other bits than on one stream", np.array_equal(B.bits(got[key]), B.bits(got1[key])))
    ck.missed += ck1.missed
    ck.done()


def test_the_second_stream_refuses_what_the_header_says():
    """deferred with a misaligned grad_kernel, and wgrad_stream equal to the caller's stream: TS_ERR_INVALID_ARGUMENT, no slot left owed"""
    L, lib = _L()
    cs = dict(B.case("K8", 32, 32), stream="deferred")
    ck = C.Checks(B.case_id(cs) + "-refused", "block_float64")
    call = Call(ck, cs, B.operands(cs))
    f = call.forward(0)
    o = call.backward_buffers(0, gk_off=True)
    rc = call.backward_rc(f, o, call.opts(wgrad_ws=o["wgrad_ws"], deferred=1))
    ck.true("refused", f"deferred with grad_kernel off the boundary: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
    o = call.backward_buffers(0)
    caller = torch.cuda.Stream()
    torch.cuda.synchronize()
    opts = call.opts(wgrad_ws=o["wgrad_ws"], deferred=1)
    opts.wgrad_stream = caller.cuda_stream
    rc = call.backward_rc(f, o, opts, stream=caller.cuda_stream)
    ck.true("refused", f"wgrad_stream = the caller's stream: code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
    torch.cuda.synchronize()
    ck.true("refused", "a refused call wrote to grad_kernel", bool((o["grad_kernel"].raw[o["grad_kernel"].lo:o["grad_kernel"].hi] == 0xFF).all()))
    ck.done()


@pytest.mark.parametrize("cs", B.SPLIT, ids=B.case_id)
def test_the_split_call(cs):
    """comm = (void *)1, then (void *)2, on one rank: pack and sums are left as the first half wrote them (what an all-reduce over one
    rank returns); forward and backward stay within the same float64 bars"""
    run_training(cs)[0].done()


@pytest.mark.parametrize("cs", B.EVAL, ids=B.eval_id)
def test_the_evaluation_block(cs):
    """the tail in the store of pass 2 and the separate pass (eval_tail_in_pass2; c_out 12 below the list form, half rows below 64
    channels, a direct plan: no pass 2 to ride on); with and without residual and ReLU, fp32 and half; c_out 16, 20 (51 rows per
    workgroup) and 12; a class plan in front of the tail; half sums beyond the half range (half_large)"""
    from taseg_amd import backend
    L, lib = _L()
    ck = C.Checks(B.eval_id(cs), "block_float64")
    ops = B.operands(cs)
    ops["mean"], ops["invstd"] = B.eval_statistics(cs, ops)
    with library_state(0, False, cs["option"]):
        call = Call(ck, cs, ops)
        if not call.plans_ok:
            ck.done()
        sd, bk, d = call.sd, call.bk, call.d
        n, c = sd["n_out"], call.c_out

        def run(fill):
            o = dict(out=Buf((n, c), call.dt, fill), w16=Buf((bk.k, call.c_in, c), torch.float16, fill) if call.half else None,
                     ws=Buf((call.ws_bytes,), torch.uint8, fill))
            opts = call.opts(plan_f=call.sf)
            L.check(lib.ts_conv_block_eval(
                L.ptr(d["feat"]), sd["n_feat"], call.c_in, L.ptr(d["kernel"]), bk.k, L.ptr(call.nbmaps), L.ptr(call.nboffs), bk.p, sd["gather_col"],
                L.ptr(call.pos), n, c, L.ptr(d.get("residual")), L.ptr(d["bn_w"]), L.ptr(d["bn_b"]), L.ptr(d["mean"]), L.ptr(d["invstd"]),
                int(cs["relu"]), int(call.half), o["out"].ptr, None if o["w16"] is None else o["w16"].ptr, ctypes.byref(opts), o["ws"].ptr,
                call.ws_bytes, L.stream()), "ts_conv_block_eval")
            torch.cuda.synchronize()
            call.band("eval", o)
            return {k: o[k].host() for k in ("out", "w16") if o[k] is not None}
        runs = [run(fill) for fill in (0, 1)]
        same_bits(ck, runs[0], runs[1])
        backend.profile_begin()
        run(0)
        kinds = record_kinds(backend.profile_end())
        ck.true("route", f"launches {kinds}, expected {B.expected_kinds(cs, 'forward')}", kinds == B.expected_kinds(cs, "forward"))
        got = runs[0]
        if call.half:
            ck.true("cast", "w16 is not the weight rounded to half", np.array_equal(B.bits(got["w16"]), B.bits(ops["w16"])))
        if not (call.half and cs["tail"]):       # the stored convolution output of a training forward on the same operands
            got["conv_out"] = call.forward(0)["conv_out"].host()
    if not call.half and cs["tail"]:             # fp32: the riding tail has the bits of the separate pass, so it meets that bar too
        B.check_eval(ck, dict(cs, tail=False), ops, got, sfx="_f32 (as the separate pass)")
    B.check_eval(ck, cs, ops, got)
    ck.done()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_the_evaluation_block_refuses_a_residual_off_a_16_byte_boundary(half):
    """pass 2 cannot carry the tail (TS_ERR_UNSUPPORTED inside the call), and the separate pass it falls back to takes aligned pointers
    only, like the training forward: the call returns TS_ERR_INVALID_ARGUMENT and `out` keeps what it held"""
    L, lib = _L()
    cs = B.eval_case("K8", 64, 64, False, half=half)
    ck = C.Checks(B.eval_id(cs) + "-resoff", "block_float64")
    ops = B.operands(cs)
    ops["mean"], ops["invstd"] = B.eval_statistics(cs, ops)
    call = Call(ck, cs, ops)
    sd, bk, d = call.sd, call.bk, call.d
    n, c = sd["n_out"], call.c_out
    res = Buf((n, c), call.dt, off=4, init=d["residual"])
    assert res.ptr % 16 == 4
    out, ws = Buf((n, c), call.dt), Buf((call.ws_bytes,), torch.uint8)
    w16 = Buf((bk.k, call.c_in, c), torch.float16) if half else None
    opts = call.opts()
    rc = lib.ts_conv_block_eval(
        L.ptr(d["feat"]), sd["n_feat"], call.c_in, L.ptr(d["kernel"]), bk.k, L.ptr(call.nbmaps), L.ptr(call.nboffs), bk.p, sd["gather_col"],
        L.ptr(call.pos), n, c, res.ptr, L.ptr(d["bn_w"]), L.ptr(d["bn_b"]), L.ptr(d["mean"]), L.ptr(d["invstd"]), 1, int(half), out.ptr,
        None if w16 is None else w16.ptr, ctypes.byref(opts), ws.ptr, call.ws_bytes, L.stream())
    torch.cuda.synchronize()
    ck.true("refused", f"code {rc}", rc == TS_ERR_INVALID_ARGUMENT)
    ck.true("refused", "the refused call wrote to out", out.kept() and bool((out.raw[out.lo:out.hi] == 0xFF).all()))
    ck.true("band", "the call wrote outside its workspace", ws.kept())
    ck.done()


def test_every_route_is_among_the_cases():
    """group 8 in one place: every route - pair GEMM + pass 2, class GEMM + pass 2, the finish inside the product, a direct plan, the
    natural form, the ordered sum as its own launch - is what at least one case of the tables above must show in its records"""
    train = B.TWO_PASS + B.ADDEND + B.PLANS + B.KEPT + B.REFUSED_PLANS + B.NATURAL + B.SECOND_STREAM + B.SPLIT
    seen = set()
    for cs in train:
        seen |= {("f", tuple(B.expected_kinds(cs, "forward"))), ("b", tuple(B.expected_kinds(cs, "backward")))}
    for cs in B.EVAL:
        seen.add(("e", tuple(B.expected_kinds(cs, "forward"))))
    for want in (("f", (0, 1)), ("f", (3, 1)), ("f", (4,)), ("f", (3,)), ("f", (0,)), ("b", (2, 0, 1)), ("b", (2, 3, 1)), ("b", (2, 4)), ("b", (2, 3)),
                 ("b", (2, 0)), ("b", (2,)), ("b", (0, 1, 2, 5)), ("b", (2, 5)), ("e", (0, 1)), ("e", (3, 1)), ("e", (3,))):
        assert want in seen, want
