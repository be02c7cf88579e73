"""Flat-bucket SGD and AdamW for the training step (reference R/train.py:399-417, R/pcseg/optim/__init__.py:13-34).

`FlatSGD` keeps parameters, gradients and momentum in a few flat fp32 buckets and performs
`GradScaler.unscale_ -> clip_grad_norm_ -> SGD.step -> GradScaler.update` with three kinds of HIP launches per
step (ts_sgd_grad_stats per bucket, ts_sgd_decide once, ts_sgd_apply_segments per bucket) and NO device->host read: the
skip decision on non-finite gradients, the clip coefficient and the loss-scale schedule live on the device.  torch's
equivalent is ~10 multi-tensor launches over 380 tensors plus `found_inf.item()`, a queue-draining read per step.

Gradients arrive through `parallel.GradBucketReducer` (one multi-tensor copy per bucket during backward, then the
all-reduce over ranks when there are several), whose buckets this optimizer shares.

    opt = FlatSGD(model, lr=..., momentum=0.9, weight_decay=1e-4, max_norm=10.0, amp=True)
    with torch.autocast("cuda", dtype=torch.float16): loss = ...
    (loss * opt.loss_scale()).backward()        # device scalar, no sync
    opt.step()                                  # reducer.finish() + the three launches

Hyper-parameters live in `opt.param_groups`, a list of dictionaries in torch.optim.SGD's shape (one group unless `groups=`
is given); `opt.lr` / `opt.momentum` / `opt.weight_decay` read and write the single group.  `state_dict()` /
`load_state_dict()` speak torch.optim.SGD's format, `scaler_state_dict()` / `load_scaler_state_dict()`
torch.amp.GradScaler's.  `taseg_amd.pcseg.optim.FlatOptimizer` wraps all this as a torch.optim.Optimizer for schedulers.

`FlatAdamW` is the same step with torch.optim.AdamW's update (the range-view recipes' optimizer): what the two share - groups, reducer,
buckets, aliases, AMP state, the stats + decide launches, the scaler dictionaries - is `_FlatBase`; see FlatAdamW's docstring.
"""
import numpy as np
import torch

from . import _lib as L
from . import planes as _planes
from .parallel import GradBucketReducer, slot_view

__all__ = ["FlatSGD", "FlatAdamW"]

# include/taseg_hip.h TsSgdSlot / TsSgdGroup
_SLOT = np.dtype([("offset", "<i8"), ("count", "<i8"), ("group", "<i4"), ("unused", "<i4"), ("flag_index", "<i4"),
                  ("reserved", "<i4")])
_GROUP = np.dtype([("lr", "<f4"), ("momentum", "<f4"), ("weight_decay", "<f4"), ("nesterov", "<i4")])
# include/taseg_hip.h TsAdamwGroup / TsAdamwCoef
_ADAMW_GROUP = np.dtype([("lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("weight_decay", "<f8")])
_ADAMW_COEF = np.dtype([("decay", "<f4"), ("w1", "<f4"), ("b2", "<f4"), ("w2", "<f4"), ("neg_step_size", "<f4"),
                        ("bc2_sqrt", "<f4"), ("eps", "<f4"), ("live", "<i4")])


def _check_group(g):
    """what torch.optim.SGD refuses, plus the two things the kernel does not do"""
    if g["lr"] < 0.0:
        raise ValueError(f"Invalid learning rate: {g['lr']}")
    if g["momentum"] < 0.0:
        raise ValueError(f"Invalid momentum value: {g['momentum']}")
    if g["weight_decay"] < 0.0:
        raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
    if g.get("dampening", 0) != 0:
        raise ValueError(f"FlatSGD: 'dampening' = {g['dampening']} is not supported (the flat update has dampening 0)")
    if g.get("maximize", False):
        raise ValueError("FlatSGD: 'maximize' = True is not supported")
    if g["nesterov"] and g["momentum"] <= 0:
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


def _upload(dst, host_array):
    """stream-ordered host -> device copy that does not drain the queue: a FRESH pinned block per upload (torch's host allocator
    keeps it alive until the copy has run), so the host array may be rewritten at once"""
    dst.copy_(torch.from_numpy(host_array.view(np.uint8)).pin_memory(), non_blocking=True)


class _FlatBase:
    """What FlatSGD and FlatAdamW share: the parameter groups (every trainable parameter exactly once), the reducer and its gradient
    buckets, the parameter buckets the model's parameters alias, the slot tables of the *_apply_segments kernels, the AMP state
    and the stats + decide launches that fill it.  A subclass names its defaults (`_defaults`), its group check (`_check`), allocates
    its state buckets in `_add_state(bucket, flat)` / `_slot_state(bucket, i, off, p)` and issues its own update launches in step()."""

    _check = staticmethod(lambda g: None)

    def _add_state(self, b, flat):
        raise NotImplementedError

    def _slot_state(self, b, i, off, p):
        raise NotImplementedError

    def _build(self, model, defaults, groups, max_norm, amp, init_scale, growth_factor, backoff_factor, growth_interval,
               process_group, bucket_mb):
        name = type(self).__name__
        self.defaults = dict(defaults)  # what a group takes where it says nothing (torch.optim.Optimizer.defaults' role)
        self.max_norm = max_norm
        self.amp, self.growth, self.backoff, self.interval = amp, growth_factor, backoff_factor, growth_interval
        if groups is None:
            groups = [{"params": [p for p in model.parameters() if p.requires_grad]}]
        self.param_groups, group_of = [], {}
        for gi, g in enumerate(groups):
            g = dict(g)
            params = g.pop("params")
            params = [params] if isinstance(params, torch.Tensor) else list(params)
            params = [p for p in params if p.requires_grad]
            for p in params:
                if id(p) in group_of:
                    raise ValueError("some parameters appear in more than one parameter group")
                group_of[id(p)] = gi
            group = {**defaults, **g, "params": params}
            self._check(group)
            self.param_groups.append(group)
        trainable = {id(p): n for n, p in model.named_parameters() if p.requires_grad}
        missing = [n for i, n in trainable.items() if i not in group_of]
        foreign = sum(1 for i in group_of if i not in trainable)
        if missing or foreign:
            raise ValueError(f"{name}: the groups must hold every trainable parameter of the model exactly once (the flat buckets "
                             f"are updated whole); in no group: {missing[:5]}{' ...' if len(missing) > 5 else ''}, "
                             f"not of the model: {foreign}")
        self.reducer = GradBucketReducer(model, process_group=process_group, bucket_mb=bucket_mb)
        dev = self.reducer.buckets[0]["flat"].device
        L.require_device(self.reducer.buckets[0]["flat"])
        # parameters move into flat buckets too (p.data becomes a view): the update is one launch per bucket
        names = {id(p): n for n, p in model.named_parameters()}
        self._aliases = []              # (parameter, name, address of its slice): step() refuses a rebound parameter
        for b in self.reducer.buckets:
            flat = torch.zeros_like(b["flat"])
            self._add_state(b, flat)
            for i, (p, off) in enumerate(zip(b["params"], b["offsets"])):      # the gradient bucket's layout and strides
                if p.dtype != torch.float32:
                    raise TypeError(f"{name} keeps fp32 master parameters")
                view = slot_view(flat, off, p)
                view.copy_(p.data)
                p.data = view
                self._aliases.append((p, names.get(id(p), "?"), view.data_ptr()))
                self._slot_state(b, i, off, p)
            b["pflat"] = flat
            # what the *_apply_segments kernels read: one record per slot, and for every tile of the bucket the slot of its first
            # element.  The layout never changes; the `unused` column is sent again only when this rank's unused set differs from the
            # last step's
            rec = np.zeros(len(b["params"]), dtype=_SLOT)
            rec["offset"], rec["count"] = b["offsets"], [p.numel() for p in b["params"]]
            rec["group"], rec["flag_index"] = [group_of[id(p)] for p in b["params"]], np.arange(len(rec))
            starts = np.arange(-(-flat.numel() // L.SGD_TILE), dtype=np.int64) * L.SGD_TILE
            tile_first = (np.searchsorted(rec["offset"], starts, side="right") - 1).astype(np.int32)
            b["slot_host"], b["unused_sent"] = rec, ()
            b["slots"] = torch.from_numpy(rec.view(np.uint8)).to(dev)
            b["tile_first"] = torch.from_numpy(tile_first).to(dev)
        self._groups_sent = None
        self.state = torch.zeros(8, dtype=torch.float32, device=dev)
        self.state[0] = init_scale if amp else 1.0
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        return dev

    def _single(self, key):
        if len(self.param_groups) != 1:
            raise AttributeError(f"{type(self).__name__}.{key}: there are {len(self.param_groups)} parameter groups - use "
                                 f"param_groups[i]['{key}']")
        return self.param_groups[0]

    lr = property(lambda self: self._single("lr")["lr"], lambda self, v: self._single("lr").__setitem__("lr", v))
    weight_decay = property(lambda self: self._single("weight_decay")["weight_decay"],
                            lambda self, v: self._single("weight_decay").__setitem__("weight_decay", v))

    def loss_scale(self) -> torch.Tensor:
        """Device scalar to multiply the loss with before backward (1 without AMP)."""
        return self.state[0]

    def zero_grad(self, set_to_none: bool = True):
        from .parallel import bump_grad_epoch
        bump_grad_epoch()
        for b in self.reducer.buckets:
            for p in b["params"]:
                p.grad = None
                p._taseg_dest_claimed = False

    def check_aliases(self):
        """raises unless every parameter still IS its slice of the flat buckets: a `p.data = ...` after construction (Module.to,
        load_state_dict(assign=True), ...) leaves a tensor the flat update never writes - the parameter would silently freeze"""
        for p, name, ptr in self._aliases:
            if p.data_ptr() != ptr:
                raise RuntimeError(f"{type(self).__name__}: parameter '{name}' no longer aliases its slice of the flat bucket (its "
                                   ".data was rebound after the optimizer was built); the update would not reach it")

    def _decide(self, lib, st):
        """gradients into the buckets (reduced over ranks), then norm, skip flag, clip coefficient and loss scale into self.state"""
        self.check_aliases()
        self.reducer.finish()                         # gradients sit in the flat buckets (reduced over ranks)
        for b in self.reducer.buckets:
            L.check(lib.ts_sgd_grad_stats(L.ptr(b["flat"]), b["flat"].numel(), L.ptr(self._sumsq), L.ptr(self._bad), st),
                    "ts_sgd_grad_stats")
        L.check(lib.ts_sgd_decide(L.ptr(self._sumsq), L.ptr(self._bad), L.ptr(self.state), float(self.max_norm),
                                  float(self.growth), float(self.backoff), int(self.interval), 1 if self.amp else 0, st),
                "ts_sgd_decide")
        for g in self.param_groups:
            self._check(g)

    @staticmethod
    def _send_unused(b):
        """parameters that received no gradient on ANY rank this step (an unused head, a frozen branch): torch's optimizers skip them
        entirely and so do the kernels, slot by slot.  b["unused"] is this rank's list; with several ranks the reducer's all-reduced
        flag of the parameter says whether some OTHER rank had a gradient for it - then the averaged gradient is applied here too
        (DDP's rule) and the replicas stay identical.  The flag is read on the device."""
        unused = tuple(b.get("unused", ()))
        if unused != b["unused_sent"]:
            b["slot_host"]["unused"] = 0
            b["slot_host"]["unused"][list(unused)] = 1
            _upload(b["slots"], b["slot_host"])
            b["unused_sent"] = unused

    def _ordered(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _check_saved(self, state_dict):
        """the saved groups, and saved parameter number -> parameter, as torch's load_state_dict pairs them"""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        return saved, dict(zip((i for s in saved for i in s["params"]), self._ordered()))

    def _groups_out(self):
        index = {id(p): i for i, p in enumerate(self._ordered())}
        return index, [{**{k: v for k, v in g.items() if k != "params"}, "params": [index[id(p)] for p in g["params"]]}
                       for g in self.param_groups]

    def scaler_state_dict(self):
        """torch.amp.GradScaler.state_dict()'s format ({} without AMP, as a disabled GradScaler).  Loss scale and growth tracker live on
        the device: this reads them."""
        if not self.amp:
            return {}
        scale, tracker = self.state[:2].tolist()
        return {"scale": scale, "growth_factor": self.growth, "backoff_factor": self.backoff, "growth_interval": self.interval,
                "_growth_tracker": int(tracker)}

    def load_scaler_state_dict(self, state_dict):
        """an empty dictionary (a disabled scaler's) leaves everything as constructed"""
        if not self.amp or not state_dict:
            return
        self.state[0] = float(state_dict["scale"])
        self.state[1] = float(state_dict["_growth_tracker"])
        self.growth, self.backoff = state_dict["growth_factor"], state_dict["backoff_factor"]
        self.interval = state_dict["growth_interval"]


class FlatSGD(_FlatBase):
    _check = staticmethod(_check_group)

    def __init__(self, model: torch.nn.Module, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                 max_norm: float = 0.0, amp: bool = False, init_scale: float = 65536.0, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000, process_group=None, bucket_mb: float = 32.0,
                 nesterov: bool = False, groups=None):
        """`groups`: None (every trainable parameter of `model` in one group) or a list of dictionaries as torch.optim.SGD takes
        them - {"params": tensors, and any of lr / momentum / weight_decay / nesterov} - that together hold every trainable
        parameter of `model` exactly once (parameters with requires_grad False are dropped from them)."""
        defaults = {"lr": lr, "momentum": momentum, "dampening": 0, "weight_decay": weight_decay, "nesterov": nesterov,
                    "maximize": False}
        self._momentum_of = {}          # id(parameter) -> its view of the momentum bucket (what state_dict() hands out)
        dev = self._build(model, defaults, groups, max_norm, amp, init_scale, growth_factor, backoff_factor, growth_interval,
                          process_group, bucket_mb)
        # several groups: their values in a small device array, sent again only when one changed (under a scheduler: once a step)
        self._groups_dev = torch.zeros(max(len(self.param_groups), 1) * _GROUP.itemsize, dtype=torch.uint8, device=dev)

    def _add_state(self, b, flat):
        b["mflat"] = torch.zeros_like(flat)

    def _slot_state(self, b, i, off, p):
        self._momentum_of[id(p)] = slot_view(b["mflat"], off, p)

    momentum = property(lambda self: self._single("momentum")["momentum"],
                        lambda self, v: self._single("momentum").__setitem__("momentum", v))

    def state_of(self, p):
        """torch.optim.SGD's state[p]: the live view of the momentum bucket"""
        return {"momentum_buffer": self._momentum_of[id(p)]}

    def step(self):
        lib, st = L.load(), L.stream()
        self._decide(lib, st)
        values = [(float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), int(bool(g["nesterov"])))
                  for g in self.param_groups]
        groups_ptr = None
        if len(values) > 1:                           # one group (the `sgd` recipe): its values travel as kernel arguments
            if values != self._groups_sent:
                _upload(self._groups_dev, np.array(values, dtype=_GROUP))
                self._groups_sent = values
            groups_ptr = L.ptr(self._groups_dev)
        lr, momentum, weight_decay, nesterov = values[0]
        for b in self.reducer.buckets:
            # a slot without a gradient: no weight decay, no momentum update (R/pcseg/optim/__init__.py:15-21 builds
            # torch.optim.SGD, which skips a parameter whose .grad is None).
            # There is no "first step" flag: a slot that has never been stepped holds m = 0, and momentum * 0 + d = d is torch's
            # "no buffer yet: buf = d" to the bit (a skipped slot keeps its zeros, so this holds for a parameter whose first
            # gradient arrives late, after a skipped first step, and after load_state_dict() of a state without buffers).
            self._send_unused(b)
            n = b["flat"].numel()
            L.check(lib.ts_sgd_apply_segments(L.ptr(b["pflat"]), L.ptr(b["flat"]), L.ptr(b["mflat"]), n, L.ptr(self.state),
                                              L.ptr(b["slots"]), len(b["params"]), L.ptr(b["tile_first"]),
                                              b["tile_first"].numel(), L.ptr(b["flags"]) if self.reducer.world > 1 else None,
                                              groups_ptr, len(values), lr, momentum, weight_decay, nesterov, 0, st),
                    "ts_sgd_apply_segments")
        _planes.invalidate()       # the kernel wrote the parameters through raw pointers: pre-split weights are stale

    # ---- checkpoints: torch.optim.SGD's and torch.amp.GradScaler's own formats (R/train.py:339,359) ------------------------
    def state_dict(self):
        """torch.optim.SGD.state_dict()'s format.  Parameters are numbered through the groups in order (one group: the order of
        model.parameters() filtered by requires_grad); every parameter carries its momentum buffer, a VIEW of the momentum bucket -
        zeros for a parameter never stepped, which torch.optim.SGD continues from exactly as from "no buffer"."""
        index, groups = self._groups_out()
        return {"state": {index[id(p)]: {"momentum_buffer": self._momentum_of[id(p)]} for p in self._ordered()},
                "param_groups": groups}

    def load_state_dict(self, state_dict):
        """adopts a torch.optim.SGD / FlatSGD state: the saved momentum buffers are copied into the bucket views (a parameter without
        one gets zeros), the saved hyper-parameters replace the current ones as torch does"""
        saved, param_of = self._check_saved(state_dict)
        for s in saved:
            if s.get("dampening", 0) != 0:
                raise ValueError(f"FlatSGD.load_state_dict: saved 'dampening' = {s['dampening']} is not supported (must be 0)")
            if s.get("maximize", False):
                raise ValueError("FlatSGD.load_state_dict: saved 'maximize' = True is not supported")
        for b in self.reducer.buckets:
            b["mflat"].zero_()
        for i, st in state_dict["state"].items():
            buf = st.get("momentum_buffer")
            if buf is not None:
                self._momentum_of[id(param_of[i])].copy_(buf)
        for s, g in zip(saved, self.param_groups):           # in place: whoever shares the dictionaries sees the new values
            g.update({k: v for k, v in s.items() if k != "params"})
            _check_group(g)


def _check_adamw_group(g):
    """what torch.optim.AdamW refuses, plus what the kernels do not do"""
    if not 0.0 <= g["lr"]:
        raise ValueError(f"Invalid learning rate: {g['lr']}")
    if not 0.0 <= g["eps"]:
        raise ValueError(f"Invalid epsilon value: {g['eps']}")
    if not 0.0 <= g["betas"][0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {g['betas'][0]}")
    if not 0.0 <= g["betas"][1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {g['betas'][1]}")
    if not 0.0 <= g["weight_decay"]:
        raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
    if g["eps"] == 0.0:         # the padding between slots stays zero through 0 / eps
        raise ValueError("FlatAdamW: 'eps' = 0 is not supported (the flat update needs eps > 0)")
    if g.get("amsgrad", False):
        raise ValueError("FlatAdamW: 'amsgrad' = True is not supported")
    if g.get("maximize", False):
        raise ValueError("FlatAdamW: 'maximize' = True is not supported")
    if not g.get("decoupled_weight_decay", True):
        raise ValueError("FlatAdamW: 'decoupled_weight_decay' = False (plain Adam) is not supported")


class FlatAdamW(_FlatBase):
    """torch.optim.AdamW (decoupled weight decay, no amsgrad) on the flat buckets, for the range-view recipes (OPTIMIZER adamw,
    GRAD_NORM_CLIP 10, SCHEDULER onecycle): FlatSGD's step with its own update -

        ts_sgd_grad_stats per bucket, ts_sgd_decide once              norm, skip, clip coefficient, loss scale on the device
        ts_adamw_prepare per bucket                                   step counters of the live slots + 1, their scalars in double
        ts_adamw_apply_segments per bucket                            p, exp_avg, exp_avg_sq in place

    and no device->host read.  Two state buckets per gradient bucket (b["mflat"] = exp_avg, b["vflat"] = exp_avg_sq), one int32 step
    counter per slot (b["step"]) and one coefficient record per slot (b["coef"]), all on the device: a skipped step and a parameter
    without a gradient do not advance the counter, and the host never learns of either.  The group values are read at every step (lr
    AND betas: OneCycleLR cycles betas[0]) and sent as doubles when they changed."""
    _check = staticmethod(_check_adamw_group)

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_norm: float = 0.0, amp: bool = False, init_scale: float = 65536.0, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000, process_group=None, bucket_mb: float = 32.0,
                 groups=None):
        """`groups`: None or a list of dictionaries as torch.optim.AdamW takes them - {"params": tensors, and any of lr / betas / eps /
        weight_decay} - that together hold every trainable parameter of `model` exactly once."""
        defaults = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False, "maximize": False,
                    "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True}
        self._moments_of = {}           # id(parameter) -> (its view of exp_avg, of exp_avg_sq, of the step counters)
        dev = self._build(model, defaults, groups, max_norm, amp, init_scale, growth_factor, backoff_factor, growth_interval,
                          process_group, bucket_mb)
        self._groups_dev = torch.zeros(max(len(self.param_groups), 1) * _ADAMW_GROUP.itemsize, dtype=torch.uint8, device=dev)

    def _add_state(self, b, flat):
        b["mflat"], b["vflat"] = torch.zeros_like(flat), torch.zeros_like(flat)
        b["step"] = torch.zeros(len(b["params"]), dtype=torch.int32, device=flat.device)
        b["coef"] = torch.zeros(len(b["params"]) * _ADAMW_COEF.itemsize, dtype=torch.uint8, device=flat.device)

    def _slot_state(self, b, i, off, p):
        self._moments_of[id(p)] = (slot_view(b["mflat"], off, p), slot_view(b["vflat"], off, p), b["step"][i])

    betas = property(lambda self: self._single("betas")["betas"], lambda self, v: self._single("betas").__setitem__("betas", v))
    eps = property(lambda self: self._single("eps")["eps"], lambda self, v: self._single("eps").__setitem__("eps", v))

    def state_of(self, p):
        """torch.optim.AdamW's state[p] as live views: the moments' slices of the buckets and the slot's int32 counter ON THE DEVICE
        (state_dict() hands the counter out as torch keeps it, a float32 CPU scalar)"""
        m, v, step = self._moments_of[id(p)]
        return {"step": step, "exp_avg": m, "exp_avg_sq": v}

    def step(self):
        lib, st = L.load(), L.stream()
        self._decide(lib, st)
        values = [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
                  for g in self.param_groups]
        if values != self._groups_sent:
            _upload(self._groups_dev, np.array(values, dtype=_ADAMW_GROUP))
            self._groups_sent = values
        flags_of = (lambda b: L.ptr(b["flags"])) if self.reducer.world > 1 else (lambda b: None)
        for b in self.reducer.buckets:
            # a slot without a gradient: torch.optim.AdamW skips a parameter whose .grad is None - no decay, no moments, no step
            self._send_unused(b)
            L.check(lib.ts_adamw_prepare(L.ptr(b["slots"]), len(b["params"]), flags_of(b), L.ptr(self.state),
                                         L.ptr(self._groups_dev), len(values), L.ptr(b["step"]), L.ptr(b["coef"]), st),
                    "ts_adamw_prepare")
            L.check(lib.ts_adamw_apply_segments(L.ptr(b["pflat"]), L.ptr(b["flat"]), L.ptr(b["mflat"]), L.ptr(b["vflat"]),
                                                b["flat"].numel(), L.ptr(self.state), L.ptr(b["slots"]), len(b["params"]),
                                                L.ptr(b["tile_first"]), b["tile_first"].numel(), flags_of(b), L.ptr(b["coef"]), st),
                    "ts_adamw_apply_segments")
        _planes.invalidate()       # the kernel wrote the parameters through raw pointers: pre-split weights are stale

    # ---- checkpoints: torch.optim.AdamW's format ----------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.AdamW.state_dict()'s format: every parameter carries `step` (a 0-dim float32 CPU tensor, as torch keeps it) and
        `exp_avg` / `exp_avg_sq`, VIEWS of the state buckets.  A parameter never stepped carries step 0 and zeros, which is the state
        torch.optim.AdamW creates itself before its first step.  Reading the counters is the one host read."""
        index, groups = self._groups_out()
        steps = torch.cat([b["step"] for b in self.reducer.buckets]).cpu().to(torch.float32)
        at, k = {}, 0
        for b in self.reducer.buckets:
            for p in b["params"]:
                at[id(p)], k = k, k + 1
        state = {}
        for p in self._ordered():
            m, v, _ = self._moments_of[id(p)]
            state[index[id(p)]] = {"step": steps[at[id(p)]].clone(), "exp_avg": m, "exp_avg_sq": v}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        """adopts a torch.optim.AdamW / FlatAdamW state: moments copied into the bucket views and counters into the step arrays (a
        parameter without state gets zeros and step 0), the saved hyper-parameters replace the current ones as torch does"""
        saved, param_of = self._check_saved(state_dict)
        for s in saved:
            _check_adamw_group({**self.param_groups[0], **s})
        steps = {}
        for b in self.reducer.buckets:
            b["mflat"].zero_()
            b["vflat"].zero_()
        for i, st in state_dict["state"].items():
            m, v, _ = self._moments_of[id(param_of[i])]
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            steps[id(param_of[i])] = int(float(st["step"]))
        for b in self.reducer.buckets:
            b["step"].copy_(torch.tensor([steps.get(id(p), 0) for p in b["params"]], dtype=torch.int32))
        for s, g in zip(saved, self.param_groups):           # in place: whoever shares the dictionaries sees the new values
            g.update({k: v for k, v in s.items() if k != "params"})
            g["betas"] = tuple(g["betas"])
            _check_adamw_group(g)
