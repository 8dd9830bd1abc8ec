"""GPU (-m gpu): sharded BATCHES -- K hyper-parameter points per record exchange (``gwi_eval_batch_sharded``), every rank
assembling the same K results -- with a REAL exchange between ranks: ranks sharing one GPU over the node-local shared-memory
segment (R = 2 and 8), the engine's own ncclAllGather (R = 1 on every box; R = 2 / 8 on boxes with that many GPUs), and the
lock-step sampler on sharded engines (``nuts_engine_lockstep(..., sharded=True)``).

Children are fresh processes (tests/sharded_batch_child.py) started with subprocess -- never an exec of this process, which
does not open the GPU -- and a child that does not finish in time is killed by its PID and fails the test.  At most 8 children
open the GPU at a time.
"""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "sharded_batch_child.py")


def _device_count():
    import torch  # counting devices does not initialise the GPU

    return torch.cuda.device_count()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_ranks(mode, world, configs, out_prefix, limit_s):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["GWI_QUIET"] = "1"
    port = _free_port()
    logs = [open(f"{out_prefix}.{r}.log", "w") for r in range(world)]  # files, not pipes: a rank blocked on a full pipe would stall the group
    kids = [subprocess.Popen([sys.executable, CHILD, mode, str(r), str(world), str(port), out_prefix, ",".join(configs)], env=env, stdout=logs[r], stderr=subprocess.STDOUT)
            for r in range(world)]
    deadline = time.monotonic() + limit_s
    hung = []
    for r, k in enumerate(kids):
        try:
            k.wait(timeout=max(1.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            k.kill()  # this exact PID
            k.wait()
            hung.append(r)
    for f in logs:
        f.close()
    tails = "\n".join(f"[rank {r}] rc={k.returncode}\n{open(f'{out_prefix}.{r}.log').read()[-1500:]}" for r, k in enumerate(kids) if k.returncode != 0)
    assert not hung, f"ranks {hung} of {world} did not finish within {limit_s:.0f} s and were killed\n{tails}"
    assert all(k.returncode == 0 for k in kids), f"a rank failed\n{tails}"
    return [np.load(f"{out_prefix}.{r}.npz") for r in range(world)]


def check(results, configs, world):
    from golden_util import rel_err

    r0 = results[0]
    for cfg in configs:
        ev = [tuple(int(v) for v in r[f"{cfg}/events"]) for r in results]
        assert ev[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ev[:-1], ev[1:]))
        for b in range(int(r0[f"{cfg}/n_batches"])):
            p = f"{cfg}/{b}"
            ll, g, mu = r0[f"{p}/ll"], r0[f"{p}/grad"], r0[f"{p}/log_mu"]
            K = ll.shape[0]
            assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g)) and np.any(g != 0.0)
            for r in results[1:]:  # every rank assembles identical bits from the gathered records
                assert np.array_equal(r[f"{p}/ll"], ll) and np.array_equal(r[f"{p}/grad"], g) and np.array_equal(r[f"{p}/log_mu"], mu)
            # against the unsharded gwi_eval_batch over the whole catalog on the same GPU
            for k in range(K):
                assert rel_err(float(ll[k]), float(r0[f"{p}/full_ll"][k])) < 1e-10, (p, k)
                f_g = r0[f"{p}/full_grad"][k]
                assert float(np.max(np.abs(g[k] - f_g))) / max(1.0, float(np.max(np.abs(f_g)))) < 1e-8, (p, k)
                assert abs(float(mu[k]) - float(r0[f"{p}/full_log_mu"][k])) < 1e-10 * abs(float(r0[f"{p}/full_log_mu"][k])), (p, k)
            # each rank's per-event sites are the unsharded engine's for the same events
            for r, (e0, e1) in zip(results, ev):
                assert np.allclose(r[f"{p}/log_bfs"], r0[f"{p}/full_log_bfs"][:, e0:e1], rtol=1e-12, atol=1e-11), p
            # ... and two of the points against the C oracle
            if f"{p}/oracle_ll" in r0.files:
                for k in range(2):
                    assert rel_err(float(ll[k]), float(r0[f"{p}/oracle_ll"][k])) < 1e-9, (p, k)
                    o_g = r0[f"{p}/oracle_grad"][k]
                    assert float(np.max(np.abs(g[k] - o_g))) / max(1.0, float(np.max(np.abs(o_g)))) < 1e-8, (p, k)


@pytest.mark.parametrize("world", [2, 8])
def test_shared_memory_ranks_on_one_gpu(tmp_path, world):
    """R ranks on one GPU over shared memory: ragged small catalog (K = 1, 3, 16, max_batch, and a marginalised batch with a
    gradient), configs 2, 3 and 5 at full size (K = 1, 3, 16)."""
    configs = ["small", "c2", "c3", "c5"]
    results = run_ranks("shm", world, configs, str(tmp_path / f"s{world}"), limit_s=900)
    check(results, configs, world)


def test_rccl_with_a_communicator_of_one_rank(tmp_path):
    """Any box: the RCCL form (one all-gather of K records, publish_batch_kernel) with R = 1, on the parametric (C2) and the
    matrix-core spline (C3, C5) batched paths."""
    configs = ["small", "c2", "c3", "c5"]
    results = run_ranks("rccl", 1, configs, str(tmp_path / "r1"), limit_s=600)
    check(results, configs, 1)


@pytest.mark.skipif(_device_count() < 2, reason="needs >= 2 GPUs: RCCL cannot place two ranks of one communicator on one device")
def test_rccl_two_ranks_on_two_gpus(tmp_path):
    configs = ["small", "c2", "c3", "c5"]
    results = run_ranks("rccl", 2, configs, str(tmp_path / "r2"), limit_s=900)
    check(results, configs, 2)


@pytest.mark.skipif(_device_count() < 8, reason="needs 8 GPUs")
def test_rccl_eight_ranks_on_eight_gpus(tmp_path):
    configs = ["c3", "c5"]
    results = run_ranks("rccl", 8, configs, str(tmp_path / "r8"), limit_s=1200)
    check(results, configs, 8)


def test_lockstep_sampler_on_sharded_engines(tmp_path):
    """2 ranks sharing the GPU over shared memory, 7 chains over 2 engines x 3 slots (gwi_nuts_engine_queue_sharded): identical
    draws on both ranks, and chain by chain the draws of the callback queue fed by gwi_eval_batch_sharded of the same engines."""
    a, b = run_ranks("sampler", 2, ["small"], str(tmp_path / "q"), limit_s=600)
    for key in ("samples", "n_evals", "depth", "ref_samples", "ref_n_evals"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["n_evals"], a["ref_n_evals"]) and np.array_equal(a["depth"], a["ref_depth"])
    assert np.allclose(a["samples"], a["ref_samples"], rtol=1e-4, atol=1e-5)
    assert np.all(np.isfinite(a["samples"])) and np.std(a["samples"][0], axis=0).max() > 0
