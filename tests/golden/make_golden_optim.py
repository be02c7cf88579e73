"""Golden numbers of the learning-rate schedules (build container only; reads /root/reference).

    python tests/golden/make_golden_optim.py

Imports the REAL reference module pcseg/optim/__init__.py by path (as a package of its own name whose __path__ is that directory, so
its two relative imports resolve) and writes tests/golden/optim_sched.npz - numbers only, a few KB:

  factor_<function>_<w>_<t>   the float64 factors of the four schedule functions for (warm-up w, total t) = (10, 100) and (0, 7) at the
                              steps in steps_<w>_<t>: 0, 1, w - 1, w, w + 1, t / 2, t - 1, t, each once and none negative (the step-decay pair with DECAY_EPOCHS
                              [3, 6] x DECAY_SCALES [0.1, 0.5] at one iteration per epoch, i.e. decay steps [3, 6])
  lr_sequence                 param_groups[0]['lr'] after build_optimizer('sgd', LR 0.24) + build_scheduler(4 iterations x 3 epochs,
                              WARMUP_EPOCH 1, linear_warmup_with_cosdecay) on nn.Linear(2, 3): the value at construction, then after each
                              of 12 optimizer.step(); scheduler.step() pairs
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SETTINGS = ((10, 100), (0, 7))
DECAY_STEPS, DECAY_SCALES = [3, 6], [0.1, 0.5]
FUNCTIONS = ("linear_warmup_with_cosdecay", "cos_warmup_with_cosdecay", "linear_warmup_with_stepdecay", "coswarmup_with_stepdecay")


def steps_of(warmup, total):
    """(without warm-up, step w - 1 = -1 does not exist: the reference divides by the warm-up length there)"""
    steps = [0, 1, warmup - 1, warmup, warmup + 1, total // 2, total - 1, total]
    return [s for i, s in enumerate(steps) if s >= 0 and s not in steps[:i]]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def sequence_cfg():
    return Cfg(OPTIMIZER="sgd", LR=0.24, WEIGHT_DECAY=1e-4, MOMENTUM=0.9, NESTEROV=True, SCHEDULER="linear_warmup_with_cosdecay",
               WARMUP_EPOCH=1)


def load_reference():
    path = os.path.join(REF, "pcseg", "optim")
    spec = importlib.util.spec_from_file_location("ref_pcseg_optim", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_pcseg_optim"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    out = {}
    for warmup, total in SETTINGS:
        steps = steps_of(warmup, total)
        out[f"steps_{warmup}_{total}"] = np.array(steps, dtype=np.int64)
        for name in FUNCTIONS:
            extra = (DECAY_STEPS, DECAY_SCALES) if name.endswith("stepdecay") else ()
            out[f"factor_{name}_{warmup}_{total}"] = np.array([getattr(ref, name)(s, warmup, total, *extra) for s in steps],
                                                              dtype=np.float64)
    torch.manual_seed(0)
    net = torch.nn.Linear(2, 3)
    cfg = sequence_cfg()
    opt = ref.build_optimizer(net, cfg)
    sched = ref.build_scheduler(opt, 4, 3, cfg)
    lrs = [opt.param_groups[0]["lr"]]
    for _ in range(12):
        net(torch.ones(1, 2)).sum().backward()
        opt.step()
        sched.step()
        lrs.append(opt.param_groups[0]["lr"])
    out["lr_sequence"] = np.array(lrs, dtype=np.float64)
    np.savez(os.path.join(HERE, "optim_sched.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
