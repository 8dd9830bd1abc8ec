"""CPU: sharded BATCHES -- K hyper-parameter points per record exchange -- on host-only handles, records made with NumPy (as in
test_distributed_cpu.py).  gwi_shm_exchange_batch + gwi_combine_batch over shared memory (worlds 2 and 3, K = 1, 3, 16) against
the NumPy oracle's unsharded value and the C oracle's gradient; the exchange's failure and mismatch reports; and
ShardedLikelihood.evaluate_batch over gloo (one all-gather of K records per rank).  The GPU side of the same path is
test_gpu_sharded_batch.py."""
import os
import socket
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 16)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _setup(rank, world, port, comp_name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist

    from gwinferno_amd import _native as N
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.engine import NativePopulationLikelihood
    from gwinferno_amd.synthetic import make_catalog

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    pe, inj, total = make_catalog(7, 96, 1001, seed=31)
    comp = COMPOSITIONS[comp_name](pe, inj)
    p = draw_params(comp_name, np.random.default_rng(9))
    eng = NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), device=N.DEVICE_HOST_ONLY, rank=rank, world=world)
    return dist, comp, eng, total


def _points(comp, eng, comp_name, K, seed):
    from gwinferno_amd.compositions import draw_params

    rng = np.random.default_rng(seed)  # same stream on every rank
    return np.stack([eng.bound.theta_of(comp.weights(draw_params(comp_name, rng), True)) for _ in range(K)])


def _records_with_fine_differences():
    """The NumPy stand-in records of test_distributed_cpu.py with a finer difference step for the gradient numerators (some points
    drawn here have narrow peaks, whose fifth derivative makes the default step's truncation error approach 1e-8 of the gradient's
    scale).  Worker processes only."""
    import test_distributed_cpu as T

    fd = T._dlogw_dtheta
    T._dlogw_dtheta = lambda bm, theta: fd(bm, theta, h=2.5e-4)
    return T._numpy_partial_record


def _shm_worker(rank, world, port, comp_name, out_path):
    dist, comp, eng, total = _setup(rank, world, port, comp_name)
    _numpy_partial_record = _records_with_fine_differences()
    from gwinferno_amd.distributed import init_shared_memory_exchange

    init_shared_memory_exchange(eng)
    out = {}
    for K in KS:
        thetas = _points(comp, eng, comp_name, K, 100 + K)
        recs = np.stack([_numpy_partial_record(eng, eng.bound, th, want_grad=True)[0] for th in thetas])
        if rank == world - 1:
            time.sleep(0.05)  # ranks drift apart; the stamps keep them in step
        gathered = eng.shm_exchange_batch(recs)
        assert gathered.shape == (world, K, eng.partial_len)
        assert np.array_equal(gathered[rank], recs)
        res = eng.combine_batch(thetas, gathered, total, nobs=eng.n_ev_global, min_neff_cut=False)
        out[f"theta{K}"] = thetas
        out[f"log_l{K}"] = np.array([r.log_likelihood for r in res])
        out[f"grad{K}"] = np.stack([r.grad for r in res])
        out[f"log_mu{K}"] = np.array([r.summary.log_det_eff for r in res])
        # point k of the batched assembly is, bit for bit, gwi_combine of the ranks' records of point k
        ones = []
        for k in range(K):
            eng.prepare_combine(thetas[k])
            ones.append(eng.combine(gathered[:, k, :], total, nobs=eng.n_ev_global, min_neff_cut=False))
        out[f"combine{K}"] = np.array([o.log_likelihood for o in ones])
        out[f"combine_grad{K}"] = np.stack([o.grad for o in ones])
    np.savez(f"{out_path}.{rank}", **out)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


@pytest.mark.parametrize("comp_name", ["plpeak", "bspline_test"])
@pytest.mark.parametrize("world", [2, 3])
def test_shared_memory_batches_match_oracles_and_agree_across_ranks(tmp_path, world, comp_name):
    import torch.multiprocessing as mp

    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog
    from oracle import numpy_oracle as O
    from oracle.c_oracle import COracle

    out = str(tmp_path / "b")
    mp.spawn(_shm_worker, args=(world, _free_port(), comp_name, out), nprocs=world, join=True)
    got = [np.load(f"{out}.{r}.npz") for r in range(world)]
    for r in range(1, world):  # every rank assembles identical bits
        for key in got[0].files:
            assert np.array_equal(got[0][key], got[r][key]), key
    g = got[0]
    for K in KS:
        assert np.array_equal(g[f"combine{K}"], g[f"log_l{K}"]) and np.array_equal(g[f"combine_grad{K}"], g[f"grad{K}"])
    pe, inj, total = make_catalog(7, 96, 1001, seed=31)
    orc = O.COMPOSITIONS[comp_name](pe, inj)
    from gwinferno_amd.compositions import draw_params

    corc = COracle(COMPOSITIONS[comp_name](pe, inj).engine(device=-2).bound)
    for K in KS:
        rng = np.random.default_rng(100 + K)
        for k in range(K):
            ref = orc.evaluate(draw_params(comp_name, rng), total, min_neff_cut=False)
            assert abs(g[f"log_l{K}"][k] - float(ref["log_likelihood"])) < 1e-10 * abs(float(ref["log_likelihood"])), (K, k)
            assert abs(np.exp(g[f"log_mu{K}"][k]) / float(ref["detection_efficiency"]) - 1) < 1e-10
            if k < 2:  # (the stand-in's gradient numerators are finite differences, which a point whose steps cross a truncation edge spoils)
                want = corc.evaluate(g[f"theta{K}"][k], total, min_neff_cut=False)["grad"]
                scale = max(1.0, float(np.max(np.abs(want))))
                assert np.max(np.abs(g[f"grad{K}"][k] - want)) < 1e-8 * scale, (K, k)


def _failure_worker(rank, world, port, out_path):
    dist, comp, eng, total = _setup(rank, world, port, "plpeak")
    from gwinferno_amd import _native as N
    from gwinferno_amd.distributed import init_shared_memory_exchange

    init_shared_memory_exchange(eng)
    n = eng.partial_len
    report = {}
    # 1: the ranks disagree about K
    t0 = time.monotonic()
    try:
        eng.shm_exchange_batch(np.zeros((3 if rank == 0 else 2, n)))
        report["mismatch"] = "no error"
    except N.NativeEngineError as exc:
        report["mismatch"] = str(exc)
    report["mismatch_s"] = time.monotonic() - t0
    # 2: the last rank's local half failed and says so
    t0 = time.monotonic()
    try:
        r = eng.shm_exchange_batch(None, k=4) if rank == world - 1 else eng.shm_exchange_batch(np.zeros((4, n)))
        report["failure"] = "returned" if r is None else "no error"
    except N.NativeEngineError as exc:
        report["failure"] = str(exc)
    report["failure_s"] = time.monotonic() - t0
    # 2b: the last rank's gwi_eval_batch_sharded fails before its exchange (a host-only handle has no device): it publishes that
    t0 = time.monotonic()
    try:
        if rank == world - 1:
            eng.evaluate_batch_sharded(np.zeros((4, eng.n_theta)), total, min_neff_cut=False)
            report["begin_failure"] = "no error"
        else:
            eng.shm_exchange_batch(np.zeros((4, n)))
            report["begin_failure"] = "no error"
    except N.NativeEngineError as exc:
        report["begin_failure"] = str(exc)
    report["begin_failure_s"] = time.monotonic() - t0
    # 3: the exchange is still in step afterwards
    recs = np.full((2, n), float(rank))
    gathered = eng.shm_exchange_batch(recs)
    report["after"] = bool(all(np.all(gathered[r] == r) for r in range(world)))
    np.save(f"{out_path}.{rank}.npy", np.array([report], dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_shared_memory_batch_mismatch_and_failure_are_reported_at_once(tmp_path, world):
    import torch.multiprocessing as mp

    out = str(tmp_path / "f")
    mp.spawn(_failure_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    reps = [np.load(f"{out}.{r}.npy", allow_pickle=True)[0] for r in range(world)]
    last = world - 1
    for rank, rep in enumerate(reps):
        other = 1 if rank == 0 else 0  # the first rank whose K differs from this rank's (rank 0 publishes 3 records, the others 2)
        assert rep["mismatch"].startswith("GWI_ERR_INVALID") and f"rank {other} published" in rep["mismatch"], rep["mismatch"]
        assert rep["mismatch_s"] < 1.0 and rep["failure_s"] < 1.0 and rep["begin_failure_s"] < 1.0
        assert rep["after"]  # every rank waited for every stamp: the exchanges are still in step, whatever was reported
        if rank != last:
            assert f"rank {last} failed its local evaluation" in rep["failure"], rep["failure"]
            assert f"rank {last} failed its local evaluation" in rep["begin_failure"], rep["begin_failure"]
    assert reps[last]["failure"] == "returned"  # the rank that published its failure
    assert reps[last]["begin_failure"].startswith("GWI_ERR_"), reps[last]["begin_failure"]


def _gloo_worker(rank, world, port, comp_name, out_path):
    dist, comp, eng, total = _setup(rank, world, port, comp_name)
    _numpy_partial_record = _records_with_fine_differences()

    from gwinferno_amd.distributed import ShardedLikelihood

    class _Eng:  # stand-in for the device scan: the same K records, computed with NumPy
        def __getattr__(self, name):
            return getattr(eng, name)

        def eval_batch_partial(self, thetas):
            parts = [_numpy_partial_record(eng, eng.bound, th, want_grad=True) for th in thetas]
            return tuple(np.stack([p[i] for p in parts]) for i in range(4))

    sh = ShardedLikelihood(_Eng(), total)
    thetas = _points(comp, eng, comp_name, 3, 77)
    res = sh.evaluate_batch(thetas, min_neff_cut=False)
    np.savez(f"{out_path}.{rank}", theta=thetas, log_l=np.array([r.log_likelihood for r in res]), grad=np.stack([r.grad for r in res]),
             log_bfs=np.stack([r.log_bfs for r in res]))
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


@pytest.mark.parametrize("comp_name", ["plpeak", "bspline_test"])
def test_gloo_world2_evaluate_batch_matches_oracles(tmp_path, comp_name):
    import torch.multiprocessing as mp

    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.synthetic import make_catalog
    from oracle import numpy_oracle as O
    from oracle.c_oracle import COracle

    out = str(tmp_path / "g")
    mp.spawn(_gloo_worker, args=(2, _free_port(), comp_name, out), nprocs=2, join=True)
    r0, r1 = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    assert np.array_equal(r0["log_l"], r1["log_l"]) and np.array_equal(r0["grad"], r1["grad"])
    pe, inj, total = make_catalog(7, 96, 1001, seed=31)
    orc = O.COMPOSITIONS[comp_name](pe, inj)
    corc = COracle(COMPOSITIONS[comp_name](pe, inj).engine(device=-2).bound)
    rng = np.random.default_rng(77)
    for k in range(3):
        ref = orc.evaluate(draw_params(comp_name, rng), total, min_neff_cut=False)
        assert abs(r0["log_l"][k] - float(ref["log_likelihood"])) < 1e-10 * abs(float(ref["log_likelihood"]))
        got = np.concatenate([r0["log_bfs"][k], r1["log_bfs"][k]])
        assert np.max(np.abs(got - ref["logBFs"])) < 1e-10
        want = corc.evaluate(r0["theta"][k], total, min_neff_cut=False)["grad"]
        assert np.max(np.abs(r0["grad"][k] - want)) < 1e-8 * max(1.0, float(np.max(np.abs(want))))
