#!/usr/bin/env python3
"""Time the effective-spin catalog step on the device (gwi_effective_spins, gwi_chi_p_conditional_prior) on the sample counts of
configs 3 and 5, and the NumPy statement on a slice (16 threads, each a contiguous part of the slice with its own first_index; NumPy
releases the interpreter lock inside its array loops).  Prints one JSON object.
      python tools/effective_spins_time.py [--configs c3,c5] [--ndraws 10000] [--max-samples N] [--host-slice 2000] [--host-threads 16]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gwinferno_amd import spin_priors as S  # noqa: E402
from gwinferno_amd.synthetic import CONFIG_SIZES  # noqa: E402

FP64_VECTOR_PEAK_FMA_PER_S = 256 * 4 * 16 * 2.4e9 / 1.0  # 256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz: fused multiply-adds per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--ndraws", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=0, help="time at most this many samples per config and scale (0: all)")
    ap.add_argument("--host-slice", type=int, default=2000)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    out = {"ndraws": a.ndraws, "configs": {}}
    rng = np.random.default_rng(1)
    for name in a.configs.split(","):
        _, n_ev, n_pe, n_inj = CONFIG_SIZES[name]
        n_all = n_ev * n_pe + n_inj
        n = min(n_all, a.max_samples) if a.max_samples else n_all
        cols = [rng.uniform(0.05, 1.0, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)]
        S.effective_spins(*(c[:256] for c in cols), backend="device")  # (the first call loads the code object)
        t0 = time.perf_counter()
        res = S.effective_spins(*cols, backend="device")
        wall_closed = time.perf_counter() - t0
        ms_closed = S.last_device_times()[0]
        t0 = time.perf_counter()
        p, acc = S.chi_p_prior_given_chi_eff_q(res["chi_p"], res["chi_eff"], cols[0], ndraws=a.ndraws, backend="device", return_accepted=True)
        wall_cond = time.perf_counter() - t0
        total_ms, longest_ms, launches = S.last_device_times()
        exps = float(n) * a.ndraws * S.N_GRID
        out["configs"][name] = {
            "samples_in_config": n_all, "samples_timed": n,
            "closed_forms": {"kernel_ms": ms_closed, "wall_s": wall_closed, "samples_per_s_kernel": n / (ms_closed * 1e-3)},
            "conditional": {"kernel_ms": total_ms, "wall_s": wall_cond, "launches": launches, "largest_launch_ms": longest_ms, "samples_per_s_kernel": n / (total_ms * 1e-3),
                            "exponentials_per_s": exps / (total_ms * 1e-3), "fp64_vector_peak_fma_per_s": FP64_VECTOR_PEAK_FMA_PER_S,
                            "mean_accepted": float(acc.mean()), "nan": int(np.isnan(p).sum()), "whole_config_s_at_this_rate": n_all / (n / (total_ms * 1e-3))},
        }
    m = a.host_slice
    if m:
        pts = (rng.uniform(0.05, 0.8, m), rng.uniform(-0.5, 0.5, m), rng.uniform(0.3, 1.0, m))
        cuts = np.linspace(0, m, a.host_threads + 1).astype(int)
        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(a.host_threads) as pool:
            jobs = [pool.submit(S.chi_p_prior_given_chi_eff_q, *(v[lo:hi] for v in pts), ndraws=a.ndraws, first_index=int(lo), backend="host")
                    for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
            host = np.concatenate([j.result() for j in jobs])
        wall = time.perf_counter() - t0
        k = min(m, 8)
        t0 = time.perf_counter()
        S.chi_p_prior_given_chi_eff_q(*(v[:k] for v in pts), ndraws=a.ndraws, backend="host")
        one = (time.perf_counter() - t0) / k
        out["host_statement"] = {"samples": m, "threads": a.host_threads, "wall_s": wall, "samples_per_s": m / wall, "seconds_per_sample_one_thread": one,
                                 "nan": int(np.isnan(host).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
