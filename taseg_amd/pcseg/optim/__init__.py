"""`pcseg.optim` for the hot path: `build_optimizer` / `build_scheduler` with the reference's names and argument lists
(reference pcseg/optim/__init__.py), on the flat buckets of taseg_amd.optim.FlatSGD and FlatAdamW.

`sgd`, `sgd_fc` and `adamw` return a `FlatOptimizer`: a torch.optim.Optimizer whose param_groups are the live hyper-parameters of a
FlatSGD / FlatAdamW, so the schedulers (`LambdaLR`, `OneCycleLR` - which cycles `momentum` of the one and `betas[0]` of the other), a
trainer's `optimizer.param_groups[0]['lr']` log line and `state_dict()` work as on torch.optim.SGD / torch.optim.AdamW.  Two ways to
run it:

    optimizer = build_optimizer(model, cfg.OPTIM)                     # the reference's loop, unchanged (one process)
    scaler.scale(loss).backward(); scaler.unscale_(optimizer); clip_grad_norm_(model.parameters(), 10)
    scaler.step(optimizer); scaler.update(); scheduler.step()

    optimizer = build_optimizer(model, cfg.OPTIM, max_norm=10.0, amp=True)     # clip and loss scale decided on the device
    (loss * optimizer.flat.loss_scale()).backward(); optimizer.step(); scheduler.step()

`adamw` is the spelling of the four range-view recipes (tools/cfgs/range/*.yaml), with their BETA1 / BETA2 / EPS keys.  The reference's
build_optimizer knows only `adamW`, raises NotImplementedError on `adamw` and never reads those keys, so the recipes do not start
there; here they do.  `adam` / `adamW` stay torch's own optimizers, built as the reference builds them; `adam_onecycle` (fastai's
wrapper) is outside the path and raises.
"""
import numpy as np
import torch
from torch.optim import lr_scheduler as lr_sched

from ...optim import FlatAdamW, FlatSGD

__all__ = ["FlatOptimizer", "build_optimizer", "build_scheduler", "linear_warmup_with_cosdecay", "cos_warmup_with_cosdecay",
           "linear_warmup_with_stepdecay", "coswarmup_with_stepdecay"]


class FlatOptimizer(torch.optim.Optimizer):
    """torch.optim.Optimizer face of a FlatSGD or a FlatAdamW (`.flat`).  `param_groups` are the flat object's own dictionaries: what
    a scheduler writes there is what the next step() hands to the kernels.  `defaults` are the flat object's (for AdamW they hold
    `betas`, which is what lets OneCycleLR(cycle_momentum=True) accept it).  `state[p]` holds views of the state buckets:
    'momentum_buffer' for SGD; 'exp_avg', 'exp_avg_sq' and 'step' (the slot's int32 counter ON THE DEVICE) for AdamW.

    `kind="adamw"` takes lr / betas / eps / weight_decay, else lr / momentum / weight_decay / nesterov; the other keyword arguments
    go to the flat class."""

    def __init__(self, model, groups=None, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, kind="sgd", betas=(0.9, 0.999),
                 eps=1e-8, **flat_kwargs):
        if kind == "adamw":
            self.flat = FlatAdamW(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, groups=groups, **flat_kwargs)
        elif kind == "sgd":
            self.flat = FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, groups=groups,
                                **flat_kwargs)
        else:
            raise ValueError(f"FlatOptimizer: kind '{kind}'")
        super().__init__(self.flat.param_groups, dict(self.flat.defaults))       # (keeps the dictionaries it is given)
        self.flat.param_groups = self.param_groups
        for p in self.flat._ordered():
            self.state[p] = self.flat.state_of(p)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.flat.param_groups = self.param_groups               # (someone may have rebound the list)
        self.flat.step()
        return loss

    def zero_grad(self, set_to_none: bool = True):
        # GradScaler.step() leaves step() out when it found a non-finite gradient: the gradient buckets of that backward pass are
        # still open then, and the next backward pass would be refused as a second one - close them here
        if any(b["launched"] or b["pending"] != len(b["params"]) for b in self.flat.reducer.buckets):
            self.flat.reducer.finish()
        self.flat.zero_grad()

    def state_dict(self):
        self.flat.param_groups = self.param_groups
        return self.flat.state_dict()

    def load_state_dict(self, state_dict):
        self.flat.param_groups = self.param_groups
        self.flat.load_state_dict(state_dict)


def build_optimizer(model, optim_cfg, *, max_norm=0.0, amp=False, **flat_kwargs):
    """reference build_optimizer(model, optim_cfg); the keyword arguments go to FlatSGD / FlatAdamW (`process_group=`, `bucket_mb=`,
    ...).  The yaml's NESTEROV key is ignored, as the reference ignores it.  `adamw` reads LR, WEIGHT_DECAY and, where the config has
    them, BETA1 / BETA2 / EPS (torch's defaults 0.9 / 0.999 / 1e-8 where it has not)."""
    key = optim_cfg.OPTIMIZER
    if key in ("sgd", "sgd_fc"):
        groups = None
        if key == "sgd_fc":          # ten times the learning rate for the classifier; every other parameter a group of its own
            groups = [{"params": [p]} for name, p in model.named_parameters() if "classifier" not in name]
            groups.append({"params": list(model.classifier.parameters()), "lr": optim_cfg.LR * 10})
        return FlatOptimizer(model, groups, lr=optim_cfg.LR, momentum=optim_cfg.MOMENTUM, weight_decay=optim_cfg.WEIGHT_DECAY,
                             max_norm=max_norm, amp=amp, **flat_kwargs)
    if key == "adamw":
        get = optim_cfg.get if hasattr(optim_cfg, "get") else (lambda k, d: getattr(optim_cfg, k, d))
        return FlatOptimizer(model, None, kind="adamw", lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY,
                             betas=(get("BETA1", 0.9), get("BETA2", 0.999)), eps=get("EPS", 1e-8), max_norm=max_norm, amp=amp,
                             **flat_kwargs)
    if key == "adam":
        return torch.optim.Adam(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY)
    if key == "adamW":
        return torch.optim.AdamW(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY)
    if key == "adam_onecycle":
        raise NotImplementedError("optimizer 'adam_onecycle' is outside the TASeg hot path built here")
    raise NotImplementedError(f"optimizer '{key}'")


# ---- learning-rate factors.  float64 and numpy's cosine, operation for operation the reference's: tests/golden/optim_sched.npz holds
# its values and tests/test_optim_host.py asks for equality ------------------------------------------------------------------
def _cos_decay(cur_step, warmup_steps, total_steps, min_scale):
    # reproduced, not repaired: the ratio runs over total_steps, not over total_steps - warmup_steps, so the factor at the last step
    # is above min_scale (warm-up 10 of 100 steps: 0.0245)
    ratio = (cur_step - warmup_steps) / total_steps
    return (1 - min_scale) * 0.5 * (1 + np.cos(np.pi * ratio)) + min_scale


def _step_decay(cur_step, decay_steps, decay_scales):
    factor = 1
    for at, scale in zip(decay_steps, decay_scales):
        if cur_step >= at:
            factor = factor * scale
    return factor


def linear_warmup_with_cosdecay(cur_step, warmup_steps, total_steps, min_scale=1e-5):
    if cur_step < warmup_steps:
        return (1 - min_scale) * cur_step / warmup_steps + min_scale
    return _cos_decay(cur_step, warmup_steps, total_steps, min_scale)


def cos_warmup_with_cosdecay(cur_step, warmup_steps, total_steps, min_scale=1e-5):
    if cur_step < warmup_steps:
        return (1 - min_scale) * (1 - np.cos(np.pi * cur_step / warmup_steps)) / 2 + min_scale
    return _cos_decay(cur_step, warmup_steps, total_steps, min_scale)


def linear_warmup_with_stepdecay(cur_step, warmup_steps, total_steps, decay_steps, decay_scales):
    if cur_step < warmup_steps:
        return cur_step / warmup_steps
    return _step_decay(cur_step, decay_steps, decay_scales)


def coswarmup_with_stepdecay(cur_step, warmup_steps, total_steps, decay_steps, decay_scales):
    if cur_step < warmup_steps:
        return (1 - np.cos(np.pi * cur_step / warmup_steps)) / 2
    return _step_decay(cur_step, decay_steps, decay_scales)


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, optim_cfg):
    if optim_cfg.OPTIMIZER == "adam_onecycle":
        raise NotImplementedError("optimizer 'adam_onecycle' (and its OneCycle schedule) is outside the TASeg hot path built here")
    warmup_steps = optim_cfg.WARMUP_EPOCH * total_iters_each_epoch
    total_steps = total_epochs * total_iters_each_epoch
    name = optim_cfg.SCHEDULER
    if name == "linear_warmup_with_cosdecay":
        return lr_sched.LambdaLR(optimizer, lr_lambda=lambda x: linear_warmup_with_cosdecay(x, warmup_steps, total_steps))
    if name == "cos_warmup_with_cosdecay":
        return lr_sched.LambdaLR(optimizer, lr_lambda=lambda x: cos_warmup_with_cosdecay(x, warmup_steps, total_steps))
    if name in ("linear_warmup_with_stepdecay", "coswarmup_with_stepdecay"):
        if len(optim_cfg.DECAY_SCALES) != len(optim_cfg.DECAY_EPOCHS):
            raise AssertionError("DECAY_SCALES not match the DECAY_EPOCHS")
        decay_steps = [e * total_iters_each_epoch for e in optim_cfg.DECAY_EPOCHS]
        factor = linear_warmup_with_stepdecay if name == "linear_warmup_with_stepdecay" else coswarmup_with_stepdecay
        return lr_sched.LambdaLR(optimizer, lr_lambda=lambda x: factor(x, warmup_steps, total_steps, decay_steps,
                                                                       optim_cfg.DECAY_SCALES))
    if name == "onecycle":           # (the reference reads LEARNING_RATE here, not LR)
        return lr_sched.OneCycleLR(optimizer, max_lr=optim_cfg.LEARNING_RATE, epochs=total_epochs,
                                   steps_per_epoch=total_iters_each_epoch, pct_start=0.2, anneal_strategy="cos",
                                   cycle_momentum=True, div_factor=25.0, final_div_factor=100.0)
    raise NotImplementedError("Not Supported SCHEDULER")
