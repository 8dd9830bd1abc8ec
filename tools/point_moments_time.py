#!/usr/bin/env python
"""Time the per-point moments on the device (gwi_point_moments, gwinferno_amd/csrc/gwi_moment.h) at the catalogs of configs 2
and 5, K = 64 points per call and C = 3 columns: the device time after the log-weight passes (HIP events: gwi_point_moment_times) of
every call, its median and spread over the calls, and the host route it replaces -- Engine.log_weights plus np.cov(aweights=) per
segment.  Beside it the two existing entries that share its inputs, weighted_kde (after marginal_weights_add) and point_cdfs, and with
--parent-lib the same two on another build of the engine (the parent commit's), in child processes of their own, half of the calls
before this build's and half after.

      python tools/point_moments_time.py [--configs c2,c5] [--repeats 10] [--parent-lib PATH] [--out profiles/point_moments/RESULTS.md]"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}
COLUMNS = ("mass_1", "mass_ratio", "chi_eff")
N_GRID = 64
K = 64
HOST_POINTS = 2  # points of the host route (it is the slow side; once)
TITLE = "# Per-point moments: measured times"
KERNELS = "moment_sum_kernel|moment_mean_kernel|moment_cov_kernel|moment_merge_kernel|draw_tile_kernel|draw_merge_kernel"


def kernel_resources():
    """VGPRs, SGPRs, LDS and scratch of the new kernels and of the two they run behind, from the code object's metadata (the columns of
    tools/kernel_resources.py)."""
    from gwinferno_amd import _native

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    path = os.path.join(os.path.dirname(_native.LIB_PATH), "gwi_kernels.hsaco")
    if not readelf or not os.path.exists(path):
        return []
    notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
    rows = []
    for block in re.split(r"\n\s+- \.agpr_count", notes):
        name = re.search(r"\.name:\s+(\S+)", block)
        found = re.search(r"\d+(%s)(ILi(\d)E)?" % KERNELS, name.group(1)) if name else None
        if not found:
            continue
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
        label = found.group(1) + (f"<{found.group(3)}>" if found.group(3) else "")
        rows.append((label, get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size")))
    return sorted(rows)


def setup(cfg):
    from gwinferno_amd import draws as D
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.synthetic import make_config_catalog

    name = COMPOSITION_OF[cfg]
    pe, inj, _ = make_config_catalog(cfg)
    comp = COMPOSITIONS[name](pe, inj)
    eng = comp.engine()
    rng = np.random.default_rng(3)
    thetas = np.stack([comp.theta(draw_params(name, rng)) for _ in range(K)])
    grid = np.stack([np.linspace(*np.quantile(np.concatenate([pe[k].ravel(), inj[k]]), [0.01, 0.99]), N_GRID) for k in COLUMNS])
    codes = np.stack([D.cdf_codes(pe[k], grid[i]) for i, k in enumerate(COLUMNS)]), np.stack([D.cdf_codes(inj[k], grid[i]) for i, k in enumerate(COLUMNS)])
    x_pe, x_inj = np.stack([np.asarray(pe[k], dtype=np.float64) for k in COLUMNS]), np.stack([np.asarray(inj[k], dtype=np.float64) for k in COLUMNS])
    eng.set_histogram_bins(*codes, n_bins=N_GRID)
    eng.set_kde_columns(x_pe, x_inj)
    eng.marginal_weights_reset()
    eng.marginal_weights_add(thetas[:4])  # (something for weighted_kde to smooth)
    return name, eng, thetas, grid, x_pe, x_inj


def stage_times(fn):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    fn(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms]


def one_round(eng, thetas, grid, moments):
    """Device times (ms) by HIP events: point_cdfs and point_moments per point after the log-weight passes, weighted_kde per query; and
    the wall time per point of the point_moments call."""
    out = {}
    eng.point_cdfs(thetas)
    t = stage_times(eng.lib.gwi_point_cdf_times)
    out["cdf"] = (t[1] + t[2]) / len(thetas)
    eng.weighted_kde(grid)
    t = stage_times(eng.lib.gwi_kde_times)
    out["kde"] = t[0] + t[1]
    if moments:
        t0 = time.perf_counter()
        eng.point_moments(thetas)
        out["moment wall"] = 1e3 * (time.perf_counter() - t0) / len(thetas)
        t = stage_times(eng.lib.gwi_point_moment_times)
        out["moment"], out["moment cov"], out["moment logw"] = (t[1] + t[2]) / len(thetas), t[2] / len(thetas), t[0] / len(thetas)
    return out


def host_route(eng, thetas, x_pe, x_inj):
    """Wall time per point (ms) of Engine.log_weights plus np.average / np.cov(aweights=) per segment, and the last point's result."""
    t0 = time.perf_counter()
    for th in thetas:
        lw_pe, lw_inj = eng.log_weights(th)
        mean, cov = np.empty((eng.n_ev + 1, x_pe.shape[0])), np.empty((eng.n_ev + 1, x_pe.shape[0], x_pe.shape[0]))
        for seg in range(eng.n_ev + 1):
            lw, x = (lw_pe[seg], x_pe[:, seg]) if seg < eng.n_ev else (lw_inj, x_inj)
            w = np.exp(lw - lw.max())
            mean[seg], cov[seg] = np.average(x, axis=1, weights=w), np.cov(x, aweights=w, ddof=0)
    return 1e3 * (time.perf_counter() - t0) / len(thetas), (mean, cov)


def measure(cfg, repeats, moments):
    name, eng, thetas, grid, x_pe, x_inj = setup(cfg)
    extra = {"shape": f"{eng.n_ev} x {eng.n_pe}, {eng.n_inj}", "name": name, "host_mb": 8 * (eng.n_inj + eng.n_ev * eng.n_pe) / 1e6, "n_ev": eng.n_ev}
    one_round(eng, thetas[:2], grid, moments)  # (the first calls load the code object and allocate)
    one_round(eng, thetas, grid, moments)      # ... and one call of the timed shape
    rounds = [one_round(eng, thetas, grid, moments) for _ in range(repeats)]
    times = {k: [r[k] for r in rounds] for k in rounds[0]}
    if moments:
        extra["host_ms"], want = host_route(eng, thetas[:HOST_POINTS], x_pe, x_inj)
        got = eng.point_moments(thetas[HOST_POINTS - 1])
        extra["deviation"] = float(np.nanmax(np.abs(got[1][0] - want[1]) / np.sqrt(np.einsum("scc,sdd->scd", want[1], want[1]))))
        extra["dead"] = int(got[2].sum())
    eng.close()
    return times, extra


def child(cfg, lib, repeats):
    """point_cdfs and weighted_kde of whatever build GWI_ENGINE_LIB names, in a process of its own."""
    env = dict(os.environ, GWI_ENGINE_LIB=lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--configs", cfg, "--repeats", str(repeats)], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("TIMES ")]
    if res.returncode != 0 or not line:
        raise RuntimeError(f"the child process with {lib} failed ({res.returncode}): {res.stderr[-400:]}")
    return json.loads(line[-1][6:])


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.median(x)), float(x.min()), float(x.max())


def have_device():
    try:
        import torch

        return bool(torch.cuda.is_available())
    except Exception:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="another build of libgwi_engine.so (the parent commit's): its point_cdfs and weighted_kde are timed in child processes")
    ap.add_argument("--existing-only", action="store_true", help="time point_cdfs and weighted_kde only and print one TIMES line (what the child processes run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_moments", "RESULTS.md"))
    a = ap.parse_args()
    configs = [c for c in a.configs.split(",") if c]
    if a.existing_only:
        times, _ = measure(configs[0], a.repeats, False)
        print("TIMES " + json.dumps(times))
        return
    res = kernel_resources()
    resources = ["## Kernel resources (gfx950 code object)", "", "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes |", "|---|---|---|---|---|"]
    resources += [f"| `{n}` | {v} | {s} | {lds} | {scr} |" for n, v, s, lds, scr in res] + [""]
    if res:
        resources.append(f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed: the {max(int(r[1]) for r in res)} VGPRs of `moment_cov_kernel<8>` hold its 36 running sums "
                         "without a spill.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if not have_device():
        with open(a.out, "w") as f:
            f.write("\n".join([TITLE, "", "NOT MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the "
                               "parent commit is claimed.", "", *resources, ""]))
        print(f"no device: wrote {a.out} without times")
        return
    table, notes = [], []
    for cfg in configs:
        half = max(1, a.repeats // 2)
        parent = child(cfg, a.parent_lib, half) if a.parent_lib else None
        own, extra = measure(cfg, a.repeats, True)
        if a.parent_lib and a.repeats > half:
            more = child(cfg, a.parent_lib, a.repeats - half)
            parent = {k: parent[k] + more.get(k, []) for k in parent}
        row = lambda what, who, x: table.append(f"| {cfg} ({extra['shape']}) | {what} | {who} | " + ("%.4f | %.4f | %.4f | %d |" % (*stats(x), len(x)) if x else "not measured | | | |"))  # noqa: E731
        row("`point_moments`, device time per point after the log-weight pass", "this", own["moment"])
        row("... of which the two covariance launches", "this", own["moment cov"])
        row("`point_moments`, log-weight pass per point (host clock)", "this", own["moment logw"])
        row("`point_moments`, wall time per point of the call", "this", own["moment wall"])
        for key, entry in (("cdf", "`point_cdfs`, device time per point after the log-weight pass"), ("kde", "`weighted_kde`, device time per query")):
            row(entry, "this", own[key])
            row(entry, "parent", parent and parent[key])
            if parent:
                (qm, qlo, qhi), om = stats(parent[key]), stats(own[key])[0]
                where = "inside that span" if qlo <= om <= qhi else ("BELOW that span (faster than every call of the parent's)" if om < qlo else "ABOVE that span (SLOWER than every call of the parent's)")
                notes.append(f"- {cfg}: {entry.split(',')[0]} (unchanged code): this build's median is {om:.4f} ms, the parent's {qm:.4f} ({om - qm:+.4f}, {100 * (om - qm) / qm:+.2f} %); "
                             f"the parent's own calls span {qlo:.4f} ... {qhi:.4f}: this build's median lies {where}.")
        notes.append(f"- {cfg}: host route (`Engine.log_weights` + `np.average` / `np.cov(aweights=)` per segment, {extra['host_mb']:.1f} MB to the host per point): {extra['host_ms']:.1f} ms per "
                     f"point over {HOST_POINTS} points, ONE run, no spread taken.  Largest |device - host| covariance entry of the last of them, as a fraction of sqrt(V_cc V_dd): "
                     f"{extra['deviation']:.2e}; dead segments: {extra['dead']}.")
    lines = [TITLE, "", f"K = {K} points per call, C = {len(COLUMNS)} columns ({', '.join(COLUMNS)}), {a.repeats} calls per row after two warm-up calls.  Times in ms; device times are "
             "HIP-event times of the launches after the log-weight pass (draw tile, draw merge and the entry's own), summed over the call and divided by K.  `parent`: "
             + ("the parent commit's build of the engine loaded into child processes of their own, half of the calls before this build's and half after, on the same device."
                if a.parent_lib else "NOT MEASURED (no --parent-lib)."), "",
             "| config (n_ev x n_pe, n_inj) | what | build | median | min | max | calls |", "|---|---|---|---|---|---|---|", *table, "", *notes, "", *resources, ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
