#!/usr/bin/env python3
"""Measurement (GPU box): what an 8-GPU run of K-point sharded batches (gwi_eval_batch_sharded) would spend per batch.

  python tools/shard_batch_time.py shard  [--configs c2,c3,c5] [--k 16] [--n 200] [--out DIR]
      1. one GPU, no exchange: the BLOCKING K-point batch (gwi_eval_batch) of shard 0 of 8 and of the whole catalog, host clock
         around work that ends in a synchronise (the batch returns its host results), after warm-up; median of n batches.
         (Run this under rocprofv3 --kernel-trace --stats for the scan's kernel time: --configs c5.)
  python tools/shard_batch_time.py exchange [--config c5] [--k 16] [--n 200] [--world 8] [--out DIR]
      2. `world` ranks SHARING one GPU over shared memory: host stamps around gwi_shm_exchange_batch and gwi_combine_batch of
         each batch (records from gwi_eval_batch_partial of the rank's shard).  CONTENDED: the ranks share the GPU and the host.
         The exchange is timed on a second exchange of the same records, after a first one has aligned the ranks (the first
         also waits for the slowest rank's batch, which on one shared GPU queues behind the other ranks' batches).
  python tools/shard_batch_time.py project --out DIR
      3. the implied 8-GPU evaluations per second, K / (shard batch + exchange + assembly): a PROJECTION, written beside the
         measured single-GPU whole-catalog figure.
  python tools/shard_batch_time.py split-trace TRACE.csv [--out DIR]
      4. the kernel trace of step 1 (rocprofv3 ... --output-format csv, one config) split into its two engines -- the whole catalog,
         then shard 0 of 8, each on a HIP stream of its own -- as per-kernel statistics of each (DIR/<trace>_split.csv): rocprofv3's
         own --stats file pools the two into one row per kernel.
Results go to DIR/*.json (default: profiles/sharded_batch)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"c2": ("plpeak", "c2"), "c3": ("bspline_iid", "c3"), "c5": ("bspline_full", "c5")}


def _points(comp, comp_name, eng, K, seed=0):
    from gwinferno_amd.compositions import draw_params

    rng = np.random.default_rng(seed)
    return np.stack([eng.bound.theta_of(comp.weights(draw_params(comp_name, rng), True)) for _ in range(K)])


def shard(a):
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_config_catalog

    out = {}
    for cfg in a.configs.split(","):
        comp_name, cat = CASES[cfg]
        pe, inj, total = make_config_catalog(cat)
        row = {}
        for label, world in (("whole", 1), ("shard0of8", 8)):
            comp = COMPOSITIONS[comp_name](pe, inj)
            eng = comp.engine(device=0, rank=0, world=world)
            ths = _points(comp, comp_name, eng, a.k)
            run = eng.configure_batch(a.k, total, nobs=eng.n_ev_global, min_neff_cut=False)
            for _ in range(50):
                run(ths)
            ts = np.empty(a.n)
            for i in range(a.n):
                t0 = time.perf_counter()
                run(ths)
                ts[i] = time.perf_counter() - t0
            us = 1e6 * float(np.median(ts))
            row[label] = {"events": eng.n_ev, "injections": eng.n_inj, "batch_us_median": us, "batch_us_p10": 1e6 * float(np.percentile(ts, 10)),
                          "batch_us_p90": 1e6 * float(np.percentile(ts, 90)), "evals_per_s": a.k / (us * 1e-6), "path": eng.batch_path(a.k)}
            print(f"{cfg} {label}: {eng.n_ev} events + {eng.n_inj} injections: K = {a.k} batch {us:.1f} us (median of {a.n})", flush=True)
            eng.close()
        row["shard_over_whole"] = row["shard0of8"]["batch_us_median"] / row["whole"]["batch_us_median"]
        out[cfg] = row
    _save(a.out, f"shard_batch_{a.configs.replace(',', '_')}.json", {"what": "measured: one GPU, no exchange, blocking K-point batch, host clock, median", "k": a.k,
                                                                       "n": a.n, "configs": out})


def _exchange_rank(rank, world, port, a, q):
    import torch.distributed as dist

    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.distributed import init_shared_memory_exchange
    from gwinferno_amd.synthetic import make_config_catalog

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    comp_name, cat = CASES[a.config]
    pe, inj, total = make_config_catalog(cat)
    comp = COMPOSITIONS[comp_name](pe, inj)
    eng = comp.engine(device=0, rank=rank, world=world)
    init_shared_memory_exchange(eng)
    ths = _points(comp, comp_name, eng, a.k)
    rec = eng.eval_batch_partial(ths)[0]
    t_w, t_x, t_c = np.empty(a.n), np.empty(a.n), np.empty(a.n)
    for i in range(a.n + 20):
        rec = eng.eval_batch_partial(ths)[0]
        t0 = time.perf_counter()
        eng.shm_exchange_batch(rec)  # waits for the slowest rank: on a shared GPU the ranks' batches queue behind each other
        t1 = time.perf_counter()
        g = eng.shm_exchange_batch(rec)  # the ranks now arrive together: the exchange itself
        t2 = time.perf_counter()
        eng.combine_batch(ths, g, total, nobs=eng.n_ev_global, min_neff_cut=False)
        t3 = time.perf_counter()
        if i >= 20:
            t_w[i - 20], t_x[i - 20], t_c[i - 20] = t1 - t0, t2 - t1, t3 - t2
    np.save(os.path.join(a.out, f"exchange_rank{rank}.npy"), np.stack([t_w, t_x, t_c]))
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


def exchange(a):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.makedirs(a.out, exist_ok=True)
    mp.spawn(_exchange_rank, args=(a.world, port, a, None), nprocs=a.world, join=True)
    per = [np.load(os.path.join(a.out, f"exchange_rank{r}.npy")) for r in range(a.world)]
    w = np.concatenate([p[0] for p in per]) * 1e6
    x = np.concatenate([p[1] for p in per]) * 1e6
    c = np.concatenate([p[2] for p in per]) * 1e6
    rec = {"what": "measured, CONTENDED: ranks share one GPU and the host; host stamps around gwi_shm_exchange_batch / gwi_combine_batch. exchange_us: a second "
                   "exchange of the same records right after a first one that aligned the ranks (the exchange itself); first_exchange_us: the first one, which "
                   "also waits for the slowest rank's batch (on one shared GPU the ranks' batches queue behind each other: not an 8-GPU figure)",
           "config": a.config, "k": a.k, "world": a.world, "n": a.n, "exchange_us_median": float(np.median(x)), "exchange_us_p10": float(np.percentile(x, 10)),
           "exchange_us_p90": float(np.percentile(x, 90)), "assembly_us_median": float(np.median(c)), "assembly_us_p90": float(np.percentile(c, 90)),
           "first_exchange_us_median": float(np.median(w)), "first_exchange_us_p10": float(np.percentile(w, 10))}
    for r in range(a.world):
        os.remove(os.path.join(a.out, f"exchange_rank{r}.npy"))
    print(json.dumps(rec), flush=True)
    _save(a.out, f"exchange_{a.config}_w{a.world}.json", rec)


def project(a):
    rows = {}
    for cfg in CASES:
        shards = [json.load(open(os.path.join(a.out, f))) for f in sorted(os.listdir(a.out)) if f.startswith("shard_batch_")]
        row = next((s["configs"][cfg] for s in shards if cfg in s["configs"]), None)
        ex_file = os.path.join(a.out, f"exchange_{cfg}_w8.json")
        ex = json.load(open(ex_file)) if os.path.exists(ex_file) else None
        if row is None or ex is None:
            continue
        k = ex["k"]
        per_batch = row["shard0of8"]["batch_us_median"] + ex["exchange_us_median"] + ex["assembly_us_median"]
        rows[cfg] = {"PROJECTION_8gpu_evals_per_s": k / (per_batch * 1e-6), "per_batch_us": per_batch, "measured_single_gpu_whole_catalog_evals_per_s": row["whole"]["evals_per_s"],
                     "projected_speedup": row["whole"]["batch_us_median"] / per_batch, "inputs": {"shard_batch_us": row["shard0of8"]["batch_us_median"],
                                                                                                 "exchange_us_contended": ex["exchange_us_median"],
                                                                                                 "assembly_us": ex["assembly_us_median"]}}
    _save(a.out, "projection.json", {"what": "PROJECTION: K / (shard batch + exchange + assembly); exchange measured contended on one GPU", "configs": rows})
    print(json.dumps(rows, indent=1))


def split_trace(a):
    import csv

    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    # every engine launches on a HIP stream of its own: the stream of the first scan is the whole catalog's (step 1 creates that
    # engine first), the next one shard 0 of 8's; launches on any other stream (set-up copies) are listed as "other"
    streams = []
    for r in rows:
        if "scan" in r["Kernel_Name"] and r["Stream_Id"] not in streams:
            streams.append(r["Stream_Id"])
    names = dict(zip(streams, ("whole", "shard0of8")))
    out = []
    for phase in ("whole", "shard0of8", "other"):
        by_kernel = {}
        for r in rows:
            if names.get(r["Stream_Id"], "other") == phase:
                by_kernel.setdefault(r["Kernel_Name"], []).append(r)
        for name, rs in sorted(by_kernel.items(), key=lambda kv: -sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in kv[1])):
            d = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs])
            grids = sorted({int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])) for r in rs})
            out.append({"engine": phase, "kernel": name, "calls": len(d), "median_us": round(float(np.median(d)), 3), "mean_us": round(float(d.mean()), 3),
                        "min_us": round(float(d.min()), 3), "max_us": round(float(d.max()), 3), "workgroups_x": " ".join(map(str, grids))})
    os.makedirs(a.out, exist_ok=True)
    dst = os.path.join(a.out, os.path.basename(a.trace).replace(".csv", "_split.csv"))
    with open(dst, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(out[0]))
        w.writeheader()
        w.writerows(out)
    for o in out:
        print(o)


def _save(d, name, obj):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name), "w") as f:
        json.dump(obj, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["shard", "exchange", "project", "split-trace"])
    ap.add_argument("trace", nargs="?", help="split-trace: the kernel_trace.csv of a rocprofv3 run of step 1")
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--config", default="c5")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_batch"))
    a = ap.parse_args()
    os.environ.setdefault("GWI_QUIET", "1")
    {"shard": shard, "exchange": exchange, "project": project, "split-trace": split_trace}[a.what](a)


if __name__ == "__main__":
    main()
