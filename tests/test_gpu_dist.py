"""N > 1 on the GPU box: the data-parallel path of bench.py (one scan set per rank, SyncBatchNorm statistics over the
ranks, gradients averaged by GradBucketReducer during backward - R/dist_train.sh:17-19, R/train.py:247-251) run by
real rank processes on the real segmentor and HIP kernels, against ONE process on the concatenated batch.

* test_ranks_share_one_device: 2 / 4 ranks on ONE card (the GPU box has one) with the gloo transport - everything but
  the RCCL wire: process-group set-up, weight broadcast, bucket hooks, SyncBatchNorm's packed all-reduce, finish().
* test_two_ranks_rccl: needs >= 2 devices (skipped on the one-GPU box; runs wherever the driver has a multi-GPU
  node): RCCL transport, SyncBatchNorm on the library-owned communicator vs through torch.distributed, all-reduce
  bus bandwidth printed.
* test_bench_gpus_flag: `bench.py --gpus N` must not silently run one rank.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_worker.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, backend, out_dir, extra_env=None):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), TASEG_DIST_BACKEND=backend, OUT=str(out_dir), HSA_ENABLE_IPC_MODE_LEGACY="0",
                   OMP_NUM_THREADS="2")
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=420)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if any(rc != 0 for rc, _, _ in outs):
        # every rank's tail: the rank that reports "connection closed by peer" is rarely the one that failed first
        report = "\n".join(f"---- rank {r}: exit code {rc}\n{e[-2500:]}" for r, (rc, _, e) in enumerate(outs))
        raise AssertionError(report)
    return [dict(np.load(os.path.join(out_dir, f"rank{r}.npz"))) for r in range(world)], outs


def _single_process(world, amp=False):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker as W
    batches = [W.make_scan(41 + r, batch_index=r) for r in range(world)]
    logits, grads, stats, loss = W.one_step(W.build(False), batches, amp=amp)
    sizes = np.cumsum([0] + [len(b[0]) for b in batches])
    return [logits[sizes[r]:sizes[r + 1]] for r in range(world)], grads, stats, loss


def _check_against_single(ranks, prefix="", amp=False):
    """fp32: logits 1e-3, gradients 2e-3 relative L2.  amp: half storage rounds every activation (2^-11 relative) and the
    per-rank / whole-batch runs round different partial sums - logits within 5e-2 + 4 half-precision ulps of the largest
    logit; gradients within 0.2 relative L2 (cosine > 0.98, the bar of test_gpu_amp.py's AMP-vs-fp32 comparison): two
    half-storage evaluations that round different partial sums differ from each other by as much as either differs from
    fp32 - measured 8.7e-2 on stem.0.kernel, 1.25e-1 worst, whose output gradient has crossed ~40 half-rounded layers.  What the AMP case
    pins exactly is the distributed property: every rank ends with bit-identical averaged gradients."""
    world = len(ranks)
    want_logits, want_grads, want_stats, want_loss = _single_process(world, amp)
    ltol, gtol, stol = (5e-2, 0.2, 2e-3) if amp else (1e-3, 2e-3, 1e-4)
    for r, got in enumerate(ranks):
        # SyncBatchNorm statistics span the ranks: each rank's logits are its slice of the whole batch's logits
        tol = ltol + (4 * 2.0 ** -11 * float(np.abs(want_logits[r]).max()) if amp else 0.0)
        assert np.abs(got[prefix + "logits"] - want_logits[r]).max() <= tol
    assert abs(np.mean([float(g[prefix + "loss"]) for g in ranks]) - want_loss) <= (5e-3 if amp else 1e-4)
    worst = 0.0
    for name, want in want_grads.items():
        a = ranks[0][prefix + "grad/" + name]
        for other in ranks[1:]:
            assert np.array_equal(a, other[prefix + "grad/" + name]), name      # every rank holds the same averaged gradient
        err = np.linalg.norm(a - want) / max(np.linalg.norm(want), 1e-12)
        worst = max(worst, err)
        assert err <= gtol, (name, err)
    for name, want in want_stats.items():
        assert np.allclose(ranks[0][prefix + "stat/" + name], want, rtol=stol, atol=1e-5), name
    return worst


@pytest.mark.parametrize("world,amp", [(2, False), (4, False), (2, True)])
def test_ranks_share_one_device(tmp_path, world, amp):
    """2 and 4 real rank processes on ONE card (gloo transport), fp32 and under autocast: SyncBatchNorm's statistics through
    torch.distributed on the default group (the default transport), the gradient buckets on a group of their own"""
    env = {"TASEG_WORKER_AMP": "1" if amp else "0"}
    ranks, _ = _run_ranks(world, "gloo", tmp_path, env)
    worst = _check_against_single(ranks, amp=amp)
    print(f"{world} ranks (gloo, one device, {'AMP' if amp else 'fp32'}) vs one process on the "
          f"concatenated batch: worst relative gradient error {worst:.2e}")


def test_second_stream_is_refused_under_more_than_one_rank(tmp_path):
    """Under N > 1 the weight gradients stay on the stream of their backward pass: a request for the second stream is refused
    (taseg_amd._fast.require_single_stream, set by GradBucketReducer when world > 1 - the workers assert it), and the step is the
    one-stream step bit for bit.  (Rounds 5 and 6 ran the second stream under the gradient buckets in this two-rank rehearsal:
    intermittent memory-access faults, a crashed rank, wrong gradients - no cause found, so the combination is off.)"""
    env = {"TASEG_WORKER_AMP": "0", "TASEG_WORKER_LOCAL_BN": "1"}
    (tmp_path / "one").mkdir()
    (tmp_path / "two").mkdir()
    one, _ = _run_ranks(2, "gloo", tmp_path / "one", env)
    two, _ = _run_ranks(2, "gloo", tmp_path / "two", dict(env, TASEG_WORKER_SIDE="1"))
    for a, b in zip(one, two):
        assert set(a) == set(b)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad[:5]


def test_flat_sgd_unused_parameter_rule_is_global(tmp_path):
    """A parameter with a gradient on rank 0 only: FlatSGD applies the averaged gradient on BOTH ranks (replicas stay
    bit-identical, DDP's find_unused_parameters rule); a parameter unused on every rank is left untouched (torch.optim.SGD)."""
    ranks, _ = _run_ranks(2, "gloo", tmp_path, {"TASEG_WORKER_MODE": "unused"})
    a, b = ranks
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                       # no silent divergence of the replicas
    assert np.array_equal(a["step2/nobody"], np.ones(3, np.float32))          # no weight decay, no momentum: untouched
    moved = [float(np.abs(a[f"step{s}/one_rank_only"] - 1.0).max()) for s in range(3)]
    assert moved[0] > 1e-4 and moved[2] > moved[0]                  # updated on both ranks, momentum building up


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two ROCm devices (RCCL refuses two ranks on one)")
def test_two_ranks_rccl(tmp_path):
    """the RCCL wire (needs two devices), the DEFAULT arrangement: SyncBatchNorm's all-reduces through torch.distributed on the
    default group, gradient buckets on a group of their own - against ONE process on the concatenated batch"""
    ranks, outs = _run_ranks(2, "nccl", tmp_path)
    assert int(ranks[0]["direct_rccl"]) == 0 and int(ranks[0]["borrowed"]) == 0      # torch.distributed is the default transport
    _check_against_single(ranks)
    line = [ln for ln in outs[0][1].splitlines() if ln.startswith("{")]
    assert line, outs[0][1]
    print("gradient all-reduce over RCCL:", line[-1])
    assert json.loads(line[-1])["bus_GBps"] > 1.0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two ROCm devices (RCCL refuses two ranks on one)")
@pytest.mark.parametrize("transport", ["borrow", "create"])
def test_two_ranks_rccl_opt_in_transports(tmp_path, transport):
    """the two OPT-IN transports of SyncBatchNorm's statistics (taseg_amd/rccl.py: the process group's own communicator called
    from the library / a communicator the library creates), each against ONE process on the concatenated batch and against the
    same step through torch.distributed (the "c10d/" half of every worker)"""
    ranks, outs = _run_ranks(2, "nccl", tmp_path, {"TASEG_RCCL_DIRECT": transport})
    assert int(ranks[0]["direct_rccl"]) == 1 and int(ranks[0]["borrowed"]) == (1 if transport == "borrow" else 0)
    _check_against_single(ranks)
    _check_against_single(ranks, "c10d/")
    for got in ranks:                  # both SyncBatchNorm transports run the same kernels around the same sums
        for k in got:
            if k.startswith("c10d/"):
                assert np.allclose(got[k], got[k[5:]], rtol=1e-6, atol=1e-7), k


def test_bench_gpus_flag():
    """--gpus N with fewer devices exits non-zero before touching the GPU; --gpus != WORLD_SIZE is refused"""
    have = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(have + 1), "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "device" in (r.stderr + r.stdout)
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env2, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_two_ranks_rehearsal_on_one_device():
    """`bench.py --gpus 2` starts its own two ranks and reports n_gpus 2 (gloo transport, both ranks on this card: a
    rehearsal of the launch + reducer + SyncBatchNorm path, not a performance number); --full adds the all-reduce bandwidth"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(TASEG_BENCH_SHARE_DEVICE="1", TASEG_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--points", "30000", "--no-cpu-baseline", "--no-kernel-events", "--full"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout
    rec = json.loads(line[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2" and np.isfinite(rec["loss"])
    assert rec["grad_allreduce"]["bytes"] > 100e6 and rec["grad_allreduce"]["bus_GBps"] > 0
