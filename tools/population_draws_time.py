#!/usr/bin/env python3
"""Time the population draws (gwi_table_draws, gwinferno_amd/csrc/gwi_popdraw.h): for K tables of 800 points and n draws per table the
wall time of the call, the two kernels' times from HIP events, the NumPy statement's time on the same inputs (on the first tables
only where the whole request would take minutes; the row says how many) and the bytes moved.  Writes a Markdown report.
      python tools/population_draws_time.py [--tables 1,64,1024] [--draws 10000,1000000] [--grid 800] [--host-draws 4000000] [--out profiles/population_draws/RESULTS.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402
from gwinferno_amd import population_draws as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="1,64,1024")
    ap.add_argument("--draws", default="10000,1000000")
    ap.add_argument("--grid", type=int, default=800)
    ap.add_argument("--host-draws", type=int, default=4_000_000, help="the NumPy statement is timed on at most this many draws per case")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_draws", "RESULTS.md"))
    a = ap.parse_args()
    G = a.grid
    rng = np.random.default_rng(1)
    grid = np.linspace(0.0, 1.0, G)
    P.table_draws(0.0, 1.0, np.ones((1, G)), 256, seed=0)  # (the first call loads the code object)
    lines = ["| tables K | draws n | wall (ms) | prefix kernel (ms) | draw kernel(s) (ms) | launches | draws / s (draw kernel) | stores of the draw kernel (MB) | host <-> device (MB) | "
             "NumPy statement | statement draws / s |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for K in (int(k) for k in a.tables.split(",")):
        pdf = 0.05 + rng.uniform(0.0, 1.0, (K, 1)) * np.exp(-0.5 * ((grid[None, :] - rng.uniform(0.2, 0.8, (K, 1))) / 0.1) ** 2)
        for n in (int(v) for v in a.draws.split(",")):
            walls, cdf_ms, draw_ms = [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                x = P.table_draws(0.0, 1.0, pdf, n, seed=5)
                walls.append(time.perf_counter() - t0)
                c, d, launches = P.last_device_times()
                cdf_ms.append(c)
                draw_ms.append(d)
            assert x.shape == (K, n) and x.min() >= 0.0 and x.max() <= 1.0
            del x
            k_host = max(1, min(K, a.host_draws // n))
            t0 = time.perf_counter()
            P.table_draws(0.0, 1.0, pdf[:k_host], n, seed=5, backend="host")
            host = time.perf_counter() - t0
            stores = K * n * 8 / 1e6
            moved = (K * G * 8 + 2 * K * 8 + K * n * 8) / 1e6
            lines.append(f"| {K} | {n} | {1e3 * min(walls):.2f} | {min(cdf_ms):.3f} | {min(draw_ms):.3f} | {launches} | {K * n / (min(draw_ms) * 1e-3):.3e} | {stores:.1f} | {moved:.1f} | "
                         f"{host:.2f} s on {k_host} of {K} tables | {k_host * n / host:.3e} |")
            print(lines[-1], flush=True)
    res = kernel_resources(r"table_\w+_kernel")
    text = ["# Population draws: measured times", "",
            f"`tools/population_draws_time.py` on one MI355X: K tables of {G} points, n draws per table, no lower bound; the best of {a.repeats} calls.  The wall time is the "
            "whole `gwi_table_draws` call (allocation, upload of the tables, the launches, the copy of the draws back into pageable host memory); the kernel times are HIP "
            "events around the launches.  The NumPy statement (`backend=\"host\"`, one thread) is timed on the same tables, on the first few only where the column says so.", "",
            *lines, "", "## The kernels' resources (code object metadata)", "",
            "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
            *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), "",
            f"`table_draw_kernel` adds (2 G - 1) x 8 bytes of dynamic LDS per workgroup: {(2 * G - 1) * 8} bytes at G = {G}, 23 992 at the reference's largest grid of 1 500 points.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
