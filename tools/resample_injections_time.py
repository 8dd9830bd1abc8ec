#!/usr/bin/env python3
"""Time the resampling of found injections (gwi_resample_injections, gwinferno_amd/csrc/gwi_resample.h) against the host path --
gwi_log_weights copies every log-weight back, NumPy exponentiates, cumsum, searchsorted (catalog.resample_injections(backend="host"))
-- at the injection sets of BASELINE configs 2 and 5, at one fiducial point each.  Per config: the wall time of both paths (the best
of --repeats calls, each ending in a device synchronise inside the library), the device path's parts from gwi_resample_times (the
blocking log-weight pass by the host clock; the tile / merge / prefix / stats launches and the select launches by HIP events), N, and
the bytes that travel to the host.  No ratio is fixed in advance; whatever is not measured is named as unmeasured.  Writes a Markdown
report.
      python tools/resample_injections_time.py [--configs c2,c5] [--repeats 5] [--out profiles/resample_injections/RESULTS.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402
from gwinferno_amd import catalog as K  # noqa: E402
from gwinferno_amd.compositions import COMPOSITIONS, draw_params  # noqa: E402
from gwinferno_amd.synthetic import make_config_catalog  # noqa: E402

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}


def device_times(lib):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    lib.gwi_resample_times(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms], n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_injections", "RESULTS.md"))
    a = ap.parse_args()
    lines = ["| config | injections | N | device wall (ms) | log-weight pass (ms) | tile + merge + prefix + stats (ms) | select (ms) | to the host (kB) | host path wall (ms) | "
             "host path to the host (MB) | same N | indices that differ |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for cfg in a.configs.split(","):
        name = COMPOSITION_OF[cfg]
        pe, inj, total = make_config_catalog(cfg)
        comp = COMPOSITIONS[name](pe, inj)
        eng = comp.engine()
        theta = comp.theta(draw_params(name, np.random.default_rng(3)))
        K.resample_injections(1, eng, theta, inj, total)  # (the first call loads the code object and allocates)
        dev, parts, host = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            idx_d, lw_d, sums = eng.resample_injections(theta, 1)
            dev.append(time.perf_counter() - t0)
            parts.append(device_times(eng.lib)[0])
            t0 = time.perf_counter()
            new_h, n_h, _ = K.resample_injections(1, eng, theta, inj, total, backend="host")
            host.append(time.perf_counter() - t0)
        new_d, n_d, _ = K.resample_injections(1, eng, theta, inj, total)
        differ = int(np.sum(new_d["mass_1"] != new_h["mass_1"])) if n_d == n_h else -1
        best = parts[int(np.argmin(dev))]
        lines.append(f"| {cfg} ({name}) | {eng.n_inj} | {n_d} | {1e3 * min(dev):.3f} | {best[0]:.3f} | {best[1]:.3f} | {best[2]:.3f} | {(12 * n_d + 40) / 1e3:.1f} | {1e3 * min(host):.3f} | "
                     f"{8 * (eng.n_inj + eng.n_ev * eng.n_pe) / 1e6:.1f} | {n_d == n_h} | {differ} |")
        print(lines[-1], flush=True)
        eng.close()
    res = kernel_resources(r"resample_\w+_kernel")
    text = ["# Resampled injection sets: measured times", "",
            f"`tools/resample_injections_time.py` on one MI355X: `Engine.resample_injections(theta, seed)` (the reference's N draws) against the host path "
            f"(`catalog.resample_injections(backend=\"host\")`: `gwi_log_weights`, NumPy `exp`, `cumsum`, `searchsorted`, and the gather of the columns) at one fiducial "
            f"point per config; the best of {a.repeats} calls by the host clock (every call ends in a device synchronise inside the library).  The parts of the device path "
            "are those of the best call: the blocking log-weight pass by the host clock, the other launches by HIP events (`gwi_resample_times`).  The host path's wall time "
            "includes the gather of every column, which the device column does not.  Not measured: other hyper-parameter points, `n_request` above N, kernel-level "
            "counters, and the evaluations per second of an engine built from the resampled set.", "",
            *lines, "", "## The kernels' resources (code object metadata)", "",
            "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
            *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
