"""Child process of tests/test_gpu_sharded_batch.py (and of nothing else): ONE rank of an R-rank sharded BATCH evaluation -- K
hyper-parameter points per record exchange (``gwi_eval_batch_sharded``).

    python tests/sharded_batch_child.py MODE RANK WORLD PORT OUT_PREFIX CONFIGS

MODE "shm": every rank on device 0, records exchanged through the node-local shared-memory segment (``gwi_shm_comm_init``);
"rccl": rank r on device r, the engine's own ncclAllGather (``gwi_comm_init``); "sampler": ``nuts_engine_lockstep(...,
sharded=True)`` on two engines per rank sharing device 0 over shared memory.  Started by the parent BEFORE the parent has touched
a GPU; the rendezvous travels over a gloo process group on 127.0.0.1.  Every rank writes OUT_PREFIX.<rank>.npz; rank 0 also
evaluates the same batches on an UNSHARDED engine over the whole catalog (gwi_eval_batch) and two points with the C oracle.  The
parent does the asserting.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name -> (composition, catalog)
    "small": ("bspline_test", None),  # 7 events x 96 PE x 1001 injections: ragged shards
    "c2": ("plpeak", "c2"),
    "c3": ("bspline_iid", "c3"),
    "c5": ("bspline_full", "c5"),
}


def _catalog(cat):
    from gwinferno_amd.synthetic import make_catalog, make_config_catalog

    return make_config_catalog(cat) if cat else make_catalog(7, 96, 1001, seed=31)


def _attach(eng, mode):
    from gwinferno_amd.distributed import init_engine_communicator, init_shared_memory_exchange

    if mode == "rccl":
        init_engine_communicator(eng)
    else:
        init_shared_memory_exchange(eng)


def evaluations(mode, rank, world, configs):
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params

    dev = rank if mode == "rccl" else 0
    res = {}
    for cfg in configs:
        comp_name, cat = CASES[cfg]
        pe, inj, total = _catalog(cat)
        comp = COMPOSITIONS[comp_name](pe, inj)  # model objects from the GLOBAL arrays
        eng = comp.engine(device=dev, rank=rank, world=world)
        _attach(eng, mode)
        full = COMPOSITIONS[comp_name](pe, inj).engine(device=dev) if rank == 0 else None
        res[f"{cfg}/events"] = np.array(eng.event_range)
        rng = np.random.default_rng(23)
        batches = [(K, False) for K in (1, 3, 16)]
        if cfg == "small":
            batches += [(eng.max_batch, False), (3, True)]  # the engine's largest batch; the squared-weight exchange first
        for b, (K, marg) in enumerate(batches):
            thetas = np.stack([comp.theta(draw_params(comp_name, rng)) for _ in range(K)])
            kw = dict(min_neff_cut=False, marginalize_selection=marg)
            out = eng.evaluate_batch_sharded(thetas, total, **kw)
            p = f"{cfg}/{b}"
            res[f"{p}/theta"] = thetas
            res[f"{p}/ll"] = np.array([r.log_likelihood for r in out])
            res[f"{p}/grad"] = np.stack([r.grad for r in out])
            res[f"{p}/log_mu"] = np.array([r.summary.log_det_eff for r in out])
            res[f"{p}/log_bfs"] = np.stack([r.log_bfs for r in out])
            if full is not None:
                ref = full.evaluate_batch(thetas, total, **kw)
                res[f"{p}/full_ll"] = np.array([r.log_likelihood for r in ref])
                res[f"{p}/full_grad"] = np.stack([r.grad for r in ref])
                res[f"{p}/full_log_mu"] = np.array([r.summary.log_det_eff for r in ref])
                res[f"{p}/full_log_bfs"] = np.stack([r.log_bfs for r in ref])
                if K == 3:
                    from oracle.c_oracle import COracle  # the checker (test infrastructure)

                    orc = COracle(full.bound)
                    o = [orc.evaluate(thetas[k], total, **kw) for k in range(2)]
                    res[f"{p}/oracle_ll"] = np.array([x["log_likelihood"] for x in o])
                    res[f"{p}/oracle_grad"] = np.stack([x["grad"] for x in o])
        res[f"{cfg}/n_batches"] = np.array(len(batches))
        res[f"{cfg}/repeats"] = np.array(eng.two_pass_repeats())
        eng.close()
        if full is not None:
            full.close()
    return res


def sampler(rank, world):
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.sampling import Bijector, GaussianSmoothingPrior, nuts_engine_lockstep, nuts_native_lockstep

    pe, inj, total = _catalog(None)
    comps = [COMPOSITIONS["bspline_test"](pe, inj) for _ in range(2)]  # (a composition holds one engine)
    engs = [c.engine(device=0, rank=rank, world=world) for c in comps]
    comp = comps[0]
    for e in engs:
        _attach(e, "shm")  # one segment per engine
    n = engs[0].n_theta
    theta0 = comp.theta(draw_params("bspline_test", np.random.default_rng(17)))
    prior = GaussianSmoothingPrior(n).normal(slice(0, n), 5.0)
    bij = Bijector(n)
    slots, C = 3, 7
    starts = np.stack([theta0 + 0.02 * c for c in range(C)])
    kw = dict(n_warmup=8, n_samples=20, seed=5, max_tree_depth=5)
    res = nuts_engine_lockstep(engs, slots, total, prior, bij, starts, sharded=True, min_neff_cut=False, **kw)
    out = {"samples": np.stack([r["samples"] for r in res]), "n_evals": np.array([r["n_evals"] for r in res]), "depth": np.stack([r["tree_depth"] for r in res])}

    def batch_target(us, ids):
        fw = [bij.forward(u) for u in us]
        got = engs[0].evaluate_batch_sharded(np.stack([f[0] for f in fw]), total, min_neff_cut=False)
        lps, grads = [], []
        for (theta, dth, dlogj, logj), r in zip(fw, got):
            lp, gp = prior(theta)
            lps.append(r.log_likelihood + lp + logj)
            grads.append((r.grad + gp) * dth + dlogj)
        return np.array(lps), np.stack(grads)

    ref = nuts_native_lockstep(batch_target, np.stack([bij.inverse(t) for t in starts]), slots=slots, **kw)
    out["ref_samples"] = np.stack([np.array([bij.forward(u)[0] for u in r["samples"]]) for r in ref])
    out["ref_n_evals"] = np.array([r["n_evals"] for r in ref])
    out["ref_depth"] = np.stack([r["tree_depth"] for r in ref])
    for e in engs:
        e.close()
    return out


def main(argv):
    mode, rank, world, port, out, configs = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4], argv[5].split(",")
    import torch
    import torch.distributed as dist

    if mode == "rccl" and torch.cuda.device_count() < world:  # counting devices does not initialise the GPU
        raise SystemExit(f"{world} RCCL ranks need {world} GPUs")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    res = sampler(rank, world) if mode == "sampler" else evaluations(mode, rank, world, configs)
    np.savez(f"{out}.{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
