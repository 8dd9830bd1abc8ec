#!/usr/bin/env python3
"""Time the weighted kernel density estimates on the device (gwi_weighted_kde, gwi_weighted_kde2d, gwinferno_amd/csrc/gwi_kde.h) at
the catalogs of BASELINE configs 2 and 5 with C = 3 quantities on G = 256 grid points and one pair at 64 x 64 and at 128 x 128.  Per
config and query: the device time of the statistics launches and of the evaluation and sum launches (HIP events on the engine's
stream: gwi_kde_times), the wall time of the call, and the bytes that travel to the host, over --repeats calls (median, smallest,
largest); as the yardstick the host route of the same commit for the same figures: Engine.marginal_weights() read back once, then
scipy.stats.gaussian_kde per segment and quantity (or pair), timed on the first --host-segments events and the injection set and
reported per segment -- the remaining segments are NOT run.  No ratio is fixed in advance; what is not measured is named as
unmeasured.  Writes a Markdown report.
      python tools/weighted_kde_time.py [--configs c2,c5] [--repeats 10] [--host-segments 2] [--out profiles/weighted_kde/RESULTS.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402
from gwinferno_amd.compositions import COMPOSITIONS, draw_params  # noqa: E402
from gwinferno_amd.synthetic import make_config_catalog  # noqa: E402

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}
COLUMNS = ("mass_1", "mass_ratio", "redshift")
PAIR = (0, 1)
N_GRID = 256
MAPS = (64, 128)
K = 4
HOST_MAX_TERMS = 3e9  # the host route is not run for a map of more Gaussian evaluations than this (minutes of one CPU)


def kde_times(lib):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    lib.gwi_kde_times(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms] + [n.value]


def spread(v):
    return f"{np.median(v):.3f} ({min(v):.3f} ... {max(v):.3f})"


def timed(eng, call, repeats):
    call()  # (the first call loads the code object and allocates)
    wall, stats, evals, launches = [], [], [], 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        s, e, _, launches = kde_times(eng.lib)
        stats.append(s)
        evals.append(e)
    return wall, stats, evals, launches


def host_route(W, x_cols, grids, pair, maps, seg_label):
    """scipy.stats.gaussian_kde on one segment: the C curves, then the map of the pair at every size; seconds each."""
    from scipy.stats import gaussian_kde

    t0 = time.perf_counter()
    for c in range(len(x_cols)):
        gaussian_kde(x_cols[c], weights=W)(grids[c])
    t_1d = time.perf_counter() - t0
    t_2d = []
    for n in maps:
        gx, gy = np.linspace(x_cols[pair[0]].min(), x_cols[pair[0]].max(), n), np.linspace(x_cols[pair[1]].min(), x_cols[pair[1]].max(), n)
        X, Y = np.meshgrid(gx, gy, indexing="ij")
        if W.size * n * n > HOST_MAX_TERMS:  # (named as not run in the report)
            t_2d.append(float("nan"))
            continue
        t0 = time.perf_counter()
        gaussian_kde(np.vstack([x_cols[pair[0]], x_cols[pair[1]]]), weights=W)(np.vstack([X.ravel(), Y.ravel()]))
        t_2d.append(time.perf_counter() - t0)
    print(f"host route, {seg_label}: {t_1d:.3f} s for {len(x_cols)} curves, " + ", ".join(f"{t:.3f} s for {n} x {n}" for t, n in zip(t_2d, maps)), flush=True)
    return t_1d, t_2d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-segments", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_kde", "RESULTS.md"))
    a = ap.parse_args()
    dev_rows = ["| config | events x samples, injections | query | wall per query (ms) | statistics launches (ms) | evaluation + sum launches (ms) | launches | to the host per query (bytes) |",
                "|---|---|---|---|---|---|---|---|"]
    host_rows = ["| config | W read-back: wall (ms), bytes | segment | samples | scipy, 3 curves at G = 256 (s) | scipy, 64 x 64 (s) | scipy, 128 x 128 (s) |", "|---|---|---|---|---|---|---|"]
    for cfg in a.configs.split(","):
        name = COMPOSITION_OF[cfg]
        pe, inj, _ = make_config_catalog(cfg)
        comp = COMPOSITIONS[name](pe, inj)
        eng = comp.engine()
        rng = np.random.default_rng(3)
        thetas = np.stack([comp.theta(draw_params(name, rng)) for _ in range(K)])
        x_pe, x_inj = np.stack([pe[k] for k in COLUMNS]), np.stack([inj[k] for k in COLUMNS])
        lo, hi = np.minimum(x_pe.min(axis=(1, 2)), x_inj.min(axis=1)), np.maximum(x_pe.max(axis=(1, 2)), x_inj.max(axis=1))
        grid = np.stack([np.linspace(lo[c], hi[c], N_GRID) for c in range(len(COLUMNS))])
        eng.set_kde_columns(x_pe, x_inj)
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas)
        n_segs, shape = eng.n_ev + 1, f"{eng.n_ev} x {eng.n_pe}, {eng.n_inj}"
        wall, stats, evals, launches = timed(eng, lambda: eng.weighted_kde(grid), a.repeats)
        back = 8 * n_segs * len(COLUMNS) * N_GRID + n_segs * (8 * len(COLUMNS) + 8 + 4 * len(COLUMNS))
        dev_rows.append(f"| {cfg} ({name}) | {shape} | 1-D, C = {len(COLUMNS)}, G = {N_GRID} | {spread(wall)} | {spread(stats)} | {spread(evals)} | {launches} | {back} |")
        print(dev_rows[-1], flush=True)
        for n in MAPS:
            gx, gy = np.linspace(lo[PAIR[0]], hi[PAIR[0]], n), np.linspace(lo[PAIR[1]], hi[PAIR[1]], n)
            wall, stats, evals, launches = timed(eng, lambda: eng.weighted_kde2d([PAIR], gx, gy), a.repeats)
            back = 8 * n_segs * n * n + n_segs * (24 + 8 + 4)
            dev_rows.append(f"| {cfg} ({name}) | {shape} | 2-D, 1 pair, {n} x {n} | {spread(wall)} | {spread(stats)} | {spread(evals)} | {launches} | {back} |")
            print(dev_rows[-1], flush=True)
        r_wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            W_pe, W_inj, _, _ = eng.marginal_weights()
            r_wall.append(1e3 * (time.perf_counter() - t0))
        readback = f"{spread(r_wall)}, {8 * (eng.n_ev * eng.n_pe + eng.n_inj)}"
        segs = [(f"event {ev}", W_pe[ev], x_pe[:, ev]) for ev in range(min(a.host_segments, eng.n_ev))] + [("the injection set", W_inj, x_inj)]
        for label, W, cols in segs:
            live = W > 0  # (gaussian_kde takes every sample; those without weight only cost time, so they are left out, in its favour)
            t_1d, t_2d = host_route(W[live], cols[:, live], grid, PAIR, MAPS, f"{cfg} {label}")
            host_rows.append(f"| {cfg} ({name}) | {readback} | {label} | {int(live.sum())} | {t_1d:.3f} | " + " | ".join("not run" if t != t else f"{t:.3f}" for t in t_2d) + " |")
        eng.close()
    res = kernel_resources(r"kde_\w+_kernel")
    text = ["# Weighted kernel density estimates: measured times", "",
            f"`tools/weighted_kde_time.py` on one MI355X, ONE run on ONE box, nothing tuned.  After K = {K} points have been accumulated, every query is called once to load and allocate and "
            f"then {a.repeats} times: the table gives the median and (smallest ... largest) of the wall time of the Python call (host clock; the copies to the host and the allocation of the "
            "result arrays included) and of the device time of its launches (`gwi_kde_times`: HIP events on the engine's stream around the four statistics launches and around the "
            f"evaluation and sum launches).  C = {len(COLUMNS)} quantities ({', '.join(COLUMNS)}), the pair is ({COLUMNS[PAIR[0]]}, {COLUMNS[PAIR[1]]}).", "",
            *dev_rows, "",
            "The host route of the same commit for the same figures: `Engine.marginal_weights()` read back (median and spread of 3), then `scipy.stats.gaussian_kde(weights=W)` per segment, "
            f"timed ONCE each on the first {a.host_segments} events and on the injection set, samples without weight left out.  The other events were not run: a whole figure costs the "
            "per-event time times the number of events, plus the injection set.  A map of more than 3e9 Gaussian evaluations (samples x grid points) was not run on the host.  scipy's time is one host process on a shared box.", "",
            *host_rows, "",
            "Not measured: other C, G and numbers of pairs, reflection, masks, Silverman's rule (the same launches), kernel-level counters, a second box.", "",
            "## The kernels' resources (code object metadata)", "",
            "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
            *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
