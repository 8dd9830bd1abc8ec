#!/usr/bin/env python3
"""Posterior-predictive index draws: host path against device path, per hyper-parameter point, at configs 2, 3 and 5.

host    likelihood._ppc_indices in "host" mode: gwi_log_weights copies every per-sample log-weight back, NumPy exponentiates,
        cumulates and searches event by event (what the parent of this feature does)
device  the same function in "device" mode (gwi_draw_indices through the Python surface, k = 1), and
        NativePopulationLikelihood.draw_indices on its own with k = 1 and k = 64 points per call

    python tools/draw_indices_time.py [--configs c2,c3,c5] [--reps 20] [--out profiles/ppc_draws/times.json]
    python tools/draw_indices_time.py --kernels c5        # a few device calls only: the command to put under rocprofv3 --kernel-trace --stats

Times are host wall clock around calls that end with the results in host memory (best and median of --reps)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}


def _timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"best_us": 1e6 * min(ts), "median_us": 1e6 * float(np.median(ts))}


def _setup(cfg):
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.synthetic import make_config_catalog

    pe, inj, total = make_config_catalog(cfg)
    comp = COMPOSITIONS[CONFIGS[cfg]](pe, inj)
    eng = comp.engine()
    rng = np.random.default_rng(5)
    thetas = np.stack([comp.theta(draw_params(CONFIGS[cfg], rng)) for _ in range(64)])
    return pe, inj, total, eng, thetas


def measure(cfg, reps):
    from gwinferno_amd import likelihood as L

    pe, inj, total, eng, thetas = _setup(cfg)
    cuts = (5.0, 3.0, 100.0)
    n_obs = eng.n_ev
    row = {"config": cfg, "composition": CONFIGS[cfg], "n_ev": eng.n_ev, "n_pe": eng.n_pe, "n_inj": eng.n_inj, "kernel": eng.scan_kernel_name()}
    row["evaluate_us"] = _timed(lambda: eng.evaluate(thetas[0], total, min_neff_cut=False), reps)
    L.set_ppc_draws("host")
    host_idx = L._ppc_indices(eng, thetas[0], pe, inj, n_obs, *cuts)
    row["host_ppc_indices_us"] = _timed(lambda: L._ppc_indices(eng, thetas[0], pe, inj, n_obs, *cuts), reps)
    row["host_log_weights_only_us"] = _timed(lambda: eng.log_weights(thetas[0]), reps)
    L.set_ppc_draws("device")
    dev_idx = L._ppc_indices(eng, thetas[0], pe, inj, n_obs, *cuts)
    row["device_ppc_indices_us"] = _timed(lambda: L._ppc_indices(eng, thetas[0], pe, inj, n_obs, *cuts), reps)
    L.set_ppc_draws("host")
    row["indices_equal"] = int(np.sum(host_idx == dev_idx))
    row["indices_total"] = int(host_idx.size)
    u = L.ppc_uniforms(n_obs)
    u_pe1, u_inj1 = u[0][None, :, None], u[1][None]
    row["device_draw_indices_k1_us"] = _timed(lambda: eng.draw_indices(thetas[:1], u_pe1, u_inj1), reps)
    u_pe64, u_inj64 = np.repeat(u_pe1, 64, axis=0), np.repeat(u_inj1, 64, axis=0)
    k64 = _timed(lambda: eng.draw_indices(thetas, u_pe64, u_inj64), max(3, reps // 4))
    row["device_draw_indices_k64_us_per_point"] = {k: v / 64 for k, v in k64.items()}
    row["bytes_to_host"] = {"host": 8 * (eng.n_ev * eng.n_pe + eng.n_inj), "device": 4 * 2 * n_obs}
    eng.close()
    return row


def kernels_only(cfg):
    _, _, _, eng, thetas = _setup(cfg)
    rng = np.random.default_rng(1)
    for _ in range(5):
        eng.draw_indices(thetas[:4], rng.uniform(size=(4, eng.n_ev, 1)), rng.uniform(size=(4, eng.n_ev)))
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, help="run a few device calls at this config and exit (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if args.kernels:
        kernels_only(args.kernels)
        return
    rows = []
    for cfg in args.configs.split(","):
        row = measure(cfg, args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
