#!/usr/bin/env python3
"""Time the marginal weights and weighted quantiles on the device (gwi_marginal_weights_add, gwi_weighted_quantiles,
gwinferno_amd/csrc/gwi_quant.h) at the catalogs of BASELINE configs 2 and 5 with C = 3 quantities and 3 levels.  Per config: the wall
and device time per point of marginal_weights_add for K = 1 and K = 64 (the parts from gwi_quantile_times), one weighted_quantiles
query, one marginal_weights read-back and the bytes that travel to the host; as yardsticks the host path of the same commit
(Engine.log_weights per point, then the NumPy statement gwinferno_amd/draws.py: marginal_weights_reference,
weighted_quantiles_reference) and weighted_histograms (C = 3, B = 64) per point -- of this build and, with --parent-lib, of another
build of the engine run in a child process of its own between this build's rounds.  No ratio is fixed in advance; what is not
measured is named as unmeasured.  Writes a Markdown report.
      python tools/weighted_quantiles_time.py [--configs c2,c5] [--repeats 3] [--rounds 2] [--parent-lib PATH] [--out profiles/weighted_quantiles/RESULTS.md]"""
import argparse
import ctypes as C
import json
import os
import subprocess
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
LEVELS = (0.05, 0.5, 0.95)
N_BINS = 64
KS = (1, 64)


def setup(cfg):
    name = COMPOSITION_OF[cfg]
    pe, inj, _ = make_config_catalog(cfg)
    comp = COMPOSITIONS[name](pe, inj)
    eng = comp.engine()
    rng = np.random.default_rng(3)
    thetas = np.stack([comp.theta(draw_params(name, rng)) for _ in range(max(KS))])
    return name, pe, inj, eng, thetas


def histogram_times(eng, pe, inj, thetas, repeats):
    """Best wall time per point of weighted_histograms (C = 3, B = 64) for every K of KS."""
    edges = {k: np.quantile(np.concatenate([pe[k].ravel(), inj[k]]), np.linspace(0.01, 0.99, N_BINS + 1)) for k in COLUMNS}
    eng.set_histogram_bins(np.stack([D.digitize(pe[k], edges[k]) for k in COLUMNS]), np.stack([D.digitize(inj[k], edges[k]) for k in COLUMNS]), n_bins=N_BINS)
    eng.weighted_histograms(thetas[0])  # (the first call loads the code object and allocates)
    out = {}
    for k in KS:
        best = np.inf
        for _ in range(repeats):
            t0 = time.perf_counter()
            eng.weighted_histograms(thetas[:k])
            best = min(best, time.perf_counter() - t0)
        out[str(k)] = 1e3 * best / k
    return out


def histograms_only(cfg, repeats):
    """The child process of --parent-lib: whatever build GWI_ENGINE_LIB names."""
    _, pe, inj, eng, thetas = setup(cfg)
    print("HIST " + json.dumps(histogram_times(eng, pe, inj, thetas, repeats)), flush=True)
    eng.close()


def parent_histograms(cfg, lib, repeats):
    env = dict(os.environ, GWI_ENGINE_LIB=lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--histograms-only", "--configs", cfg, "--repeats", str(repeats)], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("HIST ")]
    if res.returncode != 0 or not line:
        raise RuntimeError(f"the child process with {lib} failed ({res.returncode}): {res.stderr[-400:]}")
    return json.loads(line[-1][5:])


def quantile_times(lib):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    lib.gwi_quantile_times(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="another build of libgwi_engine.so: its weighted_histograms is timed in a child process between this build's rounds")
    ap.add_argument("--histograms-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_quantiles", "RESULTS.md"))
    a = ap.parse_args()
    if a.histograms_only:
        return histograms_only(a.configs, a.repeats)
    add_rows = ["| config | events x samples, injections | K per call | add: wall per point (ms) | log-weight pass per point (ms) | draw tile + merge + marginal add per point (ms) | "
                "weighted_histograms of this build, wall per point (ms) | weighted_histograms of the other build, wall per point (ms) | add / other build's histograms |",
                "|---|---|---|---|---|---|---|---|---|"]
    query_rows = ["| config | quantile query: wall (ms) | its three launches (ms) | to the host per query (bytes) | W read-back: wall (ms) | W read-back (MB) | host path: log_weights + marginal statement, "
                  "wall per point (ms) | host path to the host per point (MB) | host quantile statement, once (ms) | indices equal to the statement's | largest relative deviation of W |",
                  "|---|---|---|---|---|---|---|---|---|---|---|"]
    for cfg in a.configs.split(","):
        name, pe, inj, eng, thetas = setup(cfg)
        x_pe, x_inj = np.stack([pe[k] for k in COLUMNS]), np.stack([inj[k] for k in COLUMNS])
        eng.set_quantile_columns(x_pe, x_inj)
        eng.marginal_weights_add(thetas[0])  # (the first call loads the code object and allocates)
        eng.weighted_quantiles(LEVELS)
        add = {k: (np.inf, None) for k in KS}
        hist_own, hist_other = {str(k): np.inf for k in KS}, {str(k): np.inf for k in KS}
        for _ in range(a.rounds):  # this build's add, the other build's histograms, this build's histograms: interleaved on the same box
            for k in KS:
                for _ in range(a.repeats):
                    eng.marginal_weights_reset()
                    t0 = time.perf_counter()
                    eng.marginal_weights_add(thetas[:k])
                    dt = time.perf_counter() - t0
                    if dt < add[k][0]:
                        add[k] = (dt, quantile_times(eng.lib))
            if a.parent_lib:
                got = parent_histograms(cfg, a.parent_lib, a.repeats)
                hist_other = {k: min(hist_other[k], got[k]) for k in hist_other}
            got = histogram_times(eng, pe, inj, thetas, a.repeats)
            hist_own = {k: min(hist_own[k], got[k]) for k in hist_own}
        for k in KS:
            dt, parts = add[k]
            other = hist_other[str(k)]
            add_rows.append(f"| {cfg} ({name}) | {eng.n_ev} x {eng.n_pe}, {eng.n_inj} | {k} | {1e3 * dt / k:.3f} | {parts[0] / k:.3f} | {parts[1] / k:.3f} | {hist_own[str(k)]:.3f} | "
                            + (f"{other:.3f} | {1e3 * dt / k / other:.3f} |" if np.isfinite(other) else "not measured | not measured |"))
            print(add_rows[-1], flush=True)
        # one accumulation of K = 1 for the comparisons: the query, the read-back, the host path
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas[:1])
        q_wall, q_dev = np.inf, 0.0
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(LEVELS)
            dt = time.perf_counter() - t0
            if dt < q_wall:
                q_wall, q_dev = dt, quantile_times(eng.lib)[2]
        r_wall = np.inf
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            W_pe, W_inj, dead, _ = eng.marginal_weights()
            r_wall = min(r_wall, time.perf_counter() - t0)
        h_wall = np.inf
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            lw_pe, lw_inj = eng.log_weights(thetas[0])
            want_pe, want_inj, _, _ = D.marginal_weights_reference(lw_pe[None], lw_inj[None], None, None)
            h_wall = min(h_wall, time.perf_counter() - t0)
        t0 = time.perf_counter()
        same, total = 0, 0
        for c in range(len(COLUMNS)):
            for seg in range(eng.n_ev + 1):
                W, x, got = (W_pe[seg], x_pe[c, seg], idx_pe[seg, c]) if seg < eng.n_ev else (W_inj, x_inj[c], idx_inj[c])
                want = D.weighted_quantiles_reference(W, np.argsort(x, kind="stable"), x, LEVELS)[0]
                same += int(np.count_nonzero(want == got))
                total += len(LEVELS)
        s_wall = time.perf_counter() - t0
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.concatenate([(np.abs(W_pe - want_pe) / want_pe)[want_pe > 0], (np.abs(W_inj - want_inj) / want_inj)[want_inj > 0]])
        n_samples = eng.n_inj + eng.n_ev * eng.n_pe
        back = (eng.n_ev + 1) * len(COLUMNS) * (4 * len(LEVELS) + 16) + 8 * (eng.n_ev + 1)
        query_rows.append(f"| {cfg} ({name}) | {1e3 * q_wall:.3f} | {q_dev:.3f} | {back} | {1e3 * r_wall:.3f} | {8 * n_samples / 1e6:.1f} | {1e3 * h_wall:.3f} | {8 * n_samples / 1e6:.1f} | "
                          f"{1e3 * s_wall:.1f} | {same} of {total} | {rel.max():.2e} (dead: {int(dead.sum())}) |")
        print(query_rows[-1], flush=True)
        eng.close()
    res = kernel_resources(r"(?:quant_|marg_)\w+_kernel")
    text = ["# Marginal weights and weighted quantiles: measured times", "",
            f"`tools/weighted_quantiles_time.py` on one MI355X, ONE run on ONE box, nothing tuned.  `Engine.marginal_weights_add(thetas[:K])`: the best of {a.repeats} calls in each of "
            f"{a.rounds} rounds by the host clock, divided by K; its parts are those of the best call (`gwi_quantile_times`: the blocking log-weight passes by the host clock, the draw tile / "
            f"draw merge / marginal add launches by HIP events).  Between the rounds `weighted_histograms` (C = {len(COLUMNS)}, B = {N_BINS}) of this build and, where a second build was given "
            "(`--parent-lib`: the parent commit's), of that build in a child process of its own, on the same box.  Every path includes the same log-weight pass.", "",
            *add_rows, "",
            f"One `Engine.weighted_quantiles` query with C = {len(COLUMNS)} quantities ({', '.join(COLUMNS)}) and the levels {LEVELS} after one point, one `Engine.marginal_weights` read-back, and "
            "the host path of the same commit: `Engine.log_weights` and `draws.marginal_weights_reference` per point (NumPy `exp`, `math.fsum`), then `draws.weighted_quantiles_reference` for "
            "every (segment, quantity) once (an argsort and exact integer prefixes: the statement is written to be exact, not fast).  The gather of the injection set through the sort order "
            "is part of the query's launches; it is recorded here and not tuned.  Not measured: other C and numbers of levels, masks, kernel-level counters.", "",
            *query_rows, "", "## The kernels' resources (code object metadata)", "",
            "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
            *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
