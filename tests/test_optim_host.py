"""taseg_amd.pcseg.optim on the host: the schedule factors against the reference's own numbers (tests/golden/optim_sched.npz, written by
tests/golden/make_golden_optim.py from the reference's module), the key dispatch of build_optimizer, and the third drop-in name."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from taseg_amd.pcseg import optim as PO

FUNCTIONS = ("linear_warmup_with_cosdecay", "cos_warmup_with_cosdecay", "linear_warmup_with_stepdecay", "coswarmup_with_stepdecay")


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def g_sched():
    return dict(np.load(os.path.join(GOLDEN, "optim_sched.npz"), allow_pickle=False))


@pytest.mark.parametrize("warmup,total", [(10, 100), (0, 7)])
@pytest.mark.parametrize("name", FUNCTIONS)
def test_schedule_factors_equal_the_reference_as_float64(g_sched, name, warmup, total):
    steps = g_sched[f"steps_{warmup}_{total}"].tolist()
    assert set(steps) >= {0, 1, warmup, warmup + 1, total // 2, total - 1, total}
    extra = ([3, 6], [0.1, 0.5]) if name.endswith("stepdecay") else ()
    got = np.array([getattr(PO, name)(s, warmup, total, *extra) for s in steps], dtype=np.float64)
    want = g_sched[f"factor_{name}_{warmup}_{total}"]
    assert want.dtype == np.float64 and np.array_equal(got, want), (got - want)


def test_cosine_decay_keeps_the_reference_ratio():
    """(step - warmup) / total_steps, not / (total_steps - warmup): the last factor is not min_scale"""
    last = PO.linear_warmup_with_cosdecay(100, 10, 100)
    assert abs(last - 0.0245) < 5e-5 and last > 1e-3
    assert PO.linear_warmup_with_cosdecay(7, 0, 7) == 1e-5          # without warm-up the two forms agree


def test_scheduler_lr_sequence_equals_the_reference(g_sched):
    """build_scheduler over a torch optimizer on the host (build_optimizer's `sgd` needs a device: tests/test_gpu_flat_optim.py runs
    the same sequence through it)"""
    net = torch.nn.Linear(2, 3)
    cfg = Cfg(OPTIMIZER="sgd", LR=0.24, WEIGHT_DECAY=1e-4, MOMENTUM=0.9, SCHEDULER="linear_warmup_with_cosdecay", WARMUP_EPOCH=1)
    opt = torch.optim.SGD(net.parameters(), lr=cfg.LR, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY)
    sched = PO.build_scheduler(opt, 4, 3, cfg)
    lrs = [opt.param_groups[0]["lr"]]
    for _ in range(12):
        net(torch.ones(1, 2)).sum().backward()
        opt.step()
        sched.step()
        lrs.append(opt.param_groups[0]["lr"])
    assert np.array_equal(np.array(lrs, dtype=np.float64), g_sched["lr_sequence"])


@pytest.mark.parametrize("name", FUNCTIONS + ("onecycle",))
def test_build_scheduler_builds_every_schedule(name):
    net = torch.nn.Linear(2, 3)
    opt = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
    cfg = Cfg(OPTIMIZER="sgd", LR=0.1, LEARNING_RATE=0.1, SCHEDULER=name, WARMUP_EPOCH=1, DECAY_EPOCHS=[1, 2], DECAY_SCALES=[0.1, 0.5])
    sched = PO.build_scheduler(opt, 5, 3, cfg)
    want = torch.optim.lr_scheduler.OneCycleLR if name == "onecycle" else torch.optim.lr_scheduler.LambdaLR
    assert isinstance(sched, want)
    for _ in range(14):
        opt.step()
        sched.step()
    if name == "linear_warmup_with_stepdecay":
        assert opt.param_groups[0]["lr"] == 0.1 * (0.1 * 0.5)        # step 14 >= both decay steps (5, 10)
    if name == "onecycle":
        assert opt.param_groups[0]["momentum"] != 0.9                # cycle_momentum moves it
    with pytest.raises(NotImplementedError):
        PO.build_scheduler(opt, 5, 3, Cfg(OPTIMIZER="sgd", SCHEDULER="no_such_schedule", WARMUP_EPOCH=1))
    with pytest.raises(AssertionError):
        PO.build_scheduler(opt, 5, 3, Cfg(OPTIMIZER="sgd", SCHEDULER="coswarmup_with_stepdecay", WARMUP_EPOCH=1, DECAY_EPOCHS=[1],
                                          DECAY_SCALES=[0.1, 0.5]))


def test_build_optimizer_key_dispatch_on_a_host_module():
    net = torch.nn.Linear(2, 3)
    adam = PO.build_optimizer(net, Cfg(OPTIMIZER="adam", LR=0.01, WEIGHT_DECAY=0.1))
    assert type(adam) is torch.optim.Adam and adam.defaults["lr"] == 0.01 and adam.defaults["weight_decay"] == 0.1
    adamw = PO.build_optimizer(net, Cfg(OPTIMIZER="adamW", LR=0.02, WEIGHT_DECAY=0.2))
    assert type(adamw) is torch.optim.AdamW and adamw.defaults["lr"] == 0.02 and adamw.defaults["weight_decay"] == 0.2
    with pytest.raises(NotImplementedError, match="adam_onecycle"):
        PO.build_optimizer(net, Cfg(OPTIMIZER="adam_onecycle", LR=0.01, WEIGHT_DECAY=0.1))
    with pytest.raises(NotImplementedError, match="adam_onecycle"):
        PO.build_scheduler(adam, 5, 3, Cfg(OPTIMIZER="adam_onecycle"))
    with pytest.raises(NotImplementedError):
        PO.build_optimizer(net, Cfg(OPTIMIZER="lion", LR=0.01, WEIGHT_DECAY=0.1))
    # the flat optimizers have no host form: a module on the host is refused, not updated by some other code
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PO.build_optimizer(net, Cfg(OPTIMIZER="sgd", LR=0.01, WEIGHT_DECAY=0.1, MOMENTUM=0.9))


def test_flat_sgd_refuses_what_torch_refuses_before_touching_the_model():
    from taseg_amd.optim import FlatSGD
    net = torch.nn.Linear(2, 3)
    before = net.weight.data_ptr()
    with pytest.raises(ValueError, match="Nesterov"):
        FlatSGD(net, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="exactly once"):
        FlatSGD(net, lr=0.1, groups=[{"params": [net.weight]}])                                 # the bias is in no group
    with pytest.raises(ValueError, match="more than one"):
        FlatSGD(net, lr=0.1, groups=[{"params": [net.weight, net.bias]}, {"params": [net.bias], "lr": 1.0}])
    assert net.weight.data_ptr() == before


def test_pcseg_optim_resolves_after_install_as_dropin():
    code = ("import taseg_amd; names = taseg_amd.install_as_dropin()\n"
            "import pcseg.optim\n"
            "from pcseg.optim import build_optimizer, build_scheduler\n"
            "import taseg_amd.pcseg.optim as mine\n"
            "assert pcseg.optim is mine and build_optimizer is mine.build_optimizer and build_scheduler is mine.build_scheduler\n"
            "assert names['pcseg.optim'] is mine\n"
            "print('OPTIM_DROPIN_OK')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert "OPTIM_DROPIN_OK" in out.stdout, out.stderr[-2000:]
