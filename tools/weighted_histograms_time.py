#!/usr/bin/env python3
"""Time the weighted histograms on the device (gwi_weighted_histograms, gwinferno_amd/csrc/gwi_hist.h) against the host path --
gwi_log_weights copies every log-weight back and NumPy histograms it (gwinferno_amd/draws.py: weighted_histograms_reference) -- at
the catalogs of BASELINE configs 2 and 5 with C = 3 binned quantities and B = 64 bins, for K = 1 and K = 64 points per call.  Per
config and K: the wall time per point of both paths (the best of --repeats calls), the device path's parts from
gwi_histogram_times (the blocking log-weight passes by the host clock; the draw tile / draw merge / histogram tile launches and the
histogram merge launches by HIP events), the bytes that travel to the host, and the largest deviation between the two.  No ratio is
fixed in advance; what is not measured is named as unmeasured.  Writes a Markdown report.
      python tools/weighted_histograms_time.py [--configs c2,c5] [--repeats 3] [--out profiles/weighted_histograms/RESULTS.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402
from gwinferno_amd import draws as D  # noqa: E402
from gwinferno_amd.compositions import COMPOSITIONS, draw_params  # noqa: E402
from gwinferno_amd.synthetic import make_config_catalog  # noqa: E402

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}
COLUMNS = ("mass_1", "mass_ratio", "redshift")
N_BINS = 64


def device_times(lib):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    lib.gwi_histogram_times(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms], n.value


def host_path(eng, thetas, pe_bins, inj_bins):
    hp, hi = np.zeros((eng.n_ev, len(COLUMNS), N_BINS)), np.zeros((len(COLUMNS), N_BINS))
    for th in thetas:
        lw_pe, lw_inj = eng.log_weights(th)
        a, b, _ = D.weighted_histograms_reference(lw_pe, lw_inj, None, None, pe_bins, inj_bins, N_BINS)
        hp += a
        hi += b
    return hp, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_histograms", "RESULTS.md"))
    a = ap.parse_args()
    lines = ["| config | events x samples, injections | K per call | device wall per point (ms) | log-weight pass per point (ms) | draw tile + merge + histogram tile per point (ms) | "
             "histogram merge per point (ms) | to the host per call (kB) | host path wall per point (ms) | host path to the host per point (MB) | largest relative deviation |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for cfg in a.configs.split(","):
        name = COMPOSITION_OF[cfg]
        pe, inj, _ = make_config_catalog(cfg)
        comp = COMPOSITIONS[name](pe, inj)
        eng = comp.engine()
        rng = np.random.default_rng(3)
        thetas = np.stack([comp.theta(draw_params(name, rng)) for _ in range(64)])
        edges = {k: np.quantile(np.concatenate([pe[k].ravel(), inj[k]]), np.linspace(0.01, 0.99, N_BINS + 1)) for k in COLUMNS}
        pe_bins, inj_bins = np.stack([D.digitize(pe[k], edges[k]) for k in COLUMNS]), np.stack([D.digitize(inj[k], edges[k]) for k in COLUMNS])
        eng.set_histogram_bins(pe_bins, inj_bins, n_bins=N_BINS)
        eng.weighted_histograms(thetas[0])  # (the first call loads the code object and allocates)
        for k in (1, 64):
            dev, parts, host = [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                hp, hi, dead = eng.weighted_histograms(thetas[:k])
                dev.append(time.perf_counter() - t0)
                parts.append(device_times(eng.lib)[0])
            for _ in range(a.repeats if k == 1 else 1):  # (64 points through the host path once: it is the slow side)
                t0 = time.perf_counter()
                want_pe, want_inj = host_path(eng, thetas[:k], pe_bins, inj_bins)
                host.append(time.perf_counter() - t0)
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.concatenate([np.abs(hp - want_pe)[want_pe > 0] / want_pe[want_pe > 0], np.abs(hi - want_inj)[want_inj > 0] / want_inj[want_inj > 0]])
            best = parts[int(np.argmin(dev))]
            back = 8 * (eng.n_ev + 1) * len(COLUMNS) * N_BINS + 4 * (eng.n_ev + 1)
            lines.append(f"| {cfg} ({name}) | {eng.n_ev} x {eng.n_pe}, {eng.n_inj} | {k} | {1e3 * min(dev) / k:.3f} | {best[0] / k:.3f} | {best[1] / k:.3f} | {best[2] / k:.3f} | "
                         f"{back / 1e3:.1f} | {1e3 * min(host) / k:.3f} | {8 * (eng.n_inj + eng.n_ev * eng.n_pe) / 1e6:.1f} | {rel.max():.2e} (dead: {int(dead.sum())}) |")
            print(lines[-1], flush=True)
        eng.close()
    res = kernel_resources(r"hist_\w+_kernel")
    text = ["# Weighted histograms: measured times", "",
            f"`tools/weighted_histograms_time.py` on one MI355X: `Engine.weighted_histograms(thetas[:K])` with C = {len(COLUMNS)} binned quantities ({', '.join(COLUMNS)}) and "
            f"B = {N_BINS} bins against the host path of the same commit (`Engine.log_weights` per point, then `draws.weighted_histograms_reference`: NumPy `exp`, `bincount`); "
            f"the best of {a.repeats} calls by the host clock (the host path at K = 64 once), divided by K.  The parts of the device path are those of the best call, summed over "
            "its points and divided by K: the blocking log-weight passes by the host clock, the launches by HIP events (`gwi_histogram_times`).  Both paths include the same "
            "log-weight pass.  Not measured: other C and B, masks, kernel-level counters.", "",
            *lines, "", "## The kernels' resources (code object metadata)", "",
            "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
            *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
