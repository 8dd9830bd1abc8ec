#!/usr/bin/env python3
"""Time the exact per-point PITs on the device (gwi_point_pits_exact, gwinferno_amd/csrc/gwi_rank.h) at the catalogs of
BASELINE configs 2 and 5 with C = 3 quantities and 64 points per call: the device time per point of the launches after the log-weight
passes (HIP events: gwi_point_rank_times) of every call and the share of the two PIT launches in it, its median and spread over the
repeats after a warm-up; the same for gwi_point_pits at G = 64 and G = 256 grid points and for gwi_weighted_histograms in the same run;
and the wall time per point of the host route, Engine.log_weights plus draws.point_pits_exact_reference, with the bytes either route
moves to the host.  With --parent-lib the two existing entries are timed on another build of the engine too (the parent commit's), in
child processes of their own before and after this build's calls.  No figure is fixed in advance; what is not measured is named as
unmeasured.  Writes a Markdown report.
      python tools/point_ranks_time.py [--configs c2,c5] [--repeats 10] [--parent-lib PATH] [--out profiles/point_ranks/RESULTS.md]"""
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
COLUMNS = ("mass_1", "mass_ratio", "redshift")
N_GRIDS = (64, 256)
K = 64
HOST_POINTS = 2  # points of the host route (it is the slow side; once)
TITLE = "# Exact per-point PITs: measured times"
KERNELS = "rank_tile_kernel|rank_merge_kernel|rank_prefix_kernel|pit_rank_kernel|pit_rank_merge_kernel|draw_tile_kernel|draw_merge_kernel"


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
        found = re.search(r"\d+(%s)E" % KERNELS, name.group(1)) if name else None
        if not found:
            continue
        get = lambda key: re.search(r"\.%s:\s+(\d+)" % key, block).group(1)  # noqa: E731
        rows.append((found.group(1), get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size")))
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
    codes = {}
    for g in N_GRIDS:
        grid = {k: np.linspace(*np.quantile(np.concatenate([pe[k].ravel(), inj[k]]), [0.01, 0.99]), g) for k in COLUMNS}
        codes[g] = np.stack([D.cdf_codes(pe[k], grid[k]) for k in COLUMNS]), np.stack([D.cdf_codes(inj[k], grid[k]) for k in COLUMNS])
    x_pe, x_inj = np.stack([np.asarray(pe[k], dtype=np.float64) for k in COLUMNS]), np.stack([np.asarray(inj[k], dtype=np.float64) for k in COLUMNS])
    return name, eng, thetas, codes, x_pe, x_inj


def stage_times(fn):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    fn(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms]


def one_round(eng, thetas, codes, ranks):
    """Device time per point (ms) of the launches after the log-weight passes, by HIP events, and the wall time per point of the call."""
    out = {}
    for g in N_GRIDS:
        eng.set_histogram_bins(*codes[g], n_bins=g)
        if g == N_GRIDS[0]:
            eng.weighted_histograms(thetas)
            t = stage_times(eng.lib.gwi_histogram_times)
            out["hist"] = (t[1] + t[2]) / len(thetas)
        eng.point_pits(thetas)
        t = stage_times(eng.lib.gwi_point_pit_times)
        out[f"pit{g}"] = (t[1] + t[2]) / len(thetas)
    if ranks:
        t0 = time.perf_counter()
        eng.point_pits_exact(thetas)
        out["rank wall"] = 1e3 * (time.perf_counter() - t0) / len(thetas)
        t = stage_times(eng.lib.gwi_point_rank_times)
        out["rank"], out["rank pit"] = (t[1] + t[2]) / len(thetas), t[2] / len(thetas)
    return out


def host_route(eng, thetas, codes):
    """Wall time per point (ms) of Engine.log_weights plus draws.point_pits_exact_reference, and the last point's result."""
    from gwinferno_amd import draws as D

    t0 = time.perf_counter()
    for th in thetas:
        lw_pe, lw_inj = eng.log_weights(th)
        out = D.point_pits_exact_reference(lw_pe, lw_inj, None, None, *codes)
    return 1e3 * (time.perf_counter() - t0) / len(thetas), out


def measure(cfg, repeats, ranks):
    from gwinferno_amd import draws as D

    name, eng, thetas, codes, x_pe, x_inj = setup(cfg)
    extra = {"shape": f"{eng.n_ev} x {eng.n_pe}, {eng.n_inj}", "name": name, "host_mb": 8 * (eng.n_inj + eng.n_ev * eng.n_pe) / 1e6, "n_ev": eng.n_ev}
    if ranks:
        t0 = time.perf_counter()
        eng.set_rank_columns(x_pe, x_inj)
        extra["setup_s"] = time.perf_counter() - t0
    one_round(eng, thetas[:2], codes, ranks)  # (the first calls load the code object and allocate)
    one_round(eng, thetas, codes, ranks)      # ... and one call of the timed shape
    rounds = [one_round(eng, thetas, codes, ranks) for _ in range(repeats)]
    times = {k: [r[k] for r in rounds] for k in rounds[0]}
    if ranks:
        extra["host_ms"], want = host_route(eng, thetas[:HOST_POINTS], D.rank_codes(x_pe, x_inj))
        got = eng.point_pits_exact(thetas[HOST_POINTS - 1])
        ok = np.isfinite(want[0])
        extra["deviation"] = float(np.max(np.abs(got[0][0][ok] - want[0][ok]) / want[0][ok])) if ok.any() else float("nan")
        extra["flags"] = bool(np.array_equal(got[1][0], want[1]))
    eng.close()
    return times, extra


def child(cfg, lib, repeats):
    """point_pits and weighted_histograms of whatever build GWI_ENGINE_LIB names, in a process of its own."""
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
    ap.add_argument("--parent-lib", default=None, help="another build of libgwi_engine.so (the parent commit's): its point_pits and weighted_histograms are timed in child processes")
    ap.add_argument("--existing-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_ranks", "RESULTS.md"))
    a = ap.parse_args()
    if a.existing_only:
        times, _ = measure(a.configs, a.repeats, ranks=False)
        print("TIMES " + json.dumps(times), flush=True)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = kernel_resources()
    resources = ["## The kernels' resources (code object metadata)", "", "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
                 *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    if not have_device():
        with open(a.out, "w") as f:
            f.write("\n".join([TITLE, "", "No GPU was available to `tools/point_ranks_time.py`: NOTHING WAS MEASURED.  Not `point_pits_exact`, not `point_pits`, not "
                               "`weighted_histograms`, not the host route, not the parent commit.", "", *resources]))
        print(f"no device: wrote {a.out}")
        return
    rows = ["| config | events x samples, injections | entry | build | median (ms per point) | min | max | spread (max - min) |", "|---|---|---|---|---|---|---|---|"]
    notes = []
    existing = (("pit64", "point_pits, G = 64"), ("pit256", "point_pits, G = 256"), ("hist", "weighted_histograms, G = 64"))
    for cfg in a.configs.split(","):
        half = max(1, a.repeats // 2)
        parent = child(cfg, a.parent_lib, half) if a.parent_lib else None
        own, extra = measure(cfg, a.repeats, ranks=True)
        if a.parent_lib:
            more = child(cfg, a.parent_lib, a.repeats - half) if a.repeats > half else {}
            parent = {k: parent[k] + more.get(k, []) for k in parent}
        label = f"{cfg} ({extra['name']}) | {extra['shape']}"
        table = [("point_pits_exact, device time after the log-weight passes", "this", own["rank"]), ("... of which the two PIT launches", "this", own["rank pit"]),
                 ("point_pits_exact, wall", "this", own["rank wall"])]
        for key, entry in existing:
            table += [(entry + ", device time after the log-weight passes", "this", own[key]), (entry + ", device time after the log-weight passes", "parent", parent and parent[key])]
        for entry, build, times in table:
            if times is None:
                rows.append(f"| {label} | {entry} | {build} | not measured | | | |")
                continue
            med, lo, hi = stats(times)
            rows.append(f"| {label} | {entry} | {build} ({len(times)} calls) | {med:.4f} | {lo:.4f} | {hi:.4f} | {hi - lo:.4f} |")
            print(rows[-1], flush=True)
        rm, km, wm = stats(own["rank"])[0], stats(own["rank pit"])[0], stats(own["rank wall"])[0]
        back = 8 * 2 * extra["n_ev"] * len(COLUMNS) + 4 * (extra["n_ev"] + 1)
        notes.append(f"- {cfg}: `point_pits_exact` takes {rm:.4f} ms of device time per point after the log-weight pass, {km:.4f} of it in the two PIT launches "
                     f"({100 * km / rm:.1f} %), against {stats(own['pit64'])[0]:.4f} for `point_pits` at G = 64 and {stats(own['pit256'])[0]:.4f} at G = 256, and {wm:.3f} ms of wall "
                     f"time per point with the log-weight pass; {back} bytes per point go to the host.  `set_rank_columns` (the sort, the ranks, the checks and the upload, once per "
                     f"catalog) took {extra['setup_s']:.2f} s.  The host route (`Engine.log_weights` + `draws.point_pits_exact_reference`, {HOST_POINTS} points, once) takes "
                     f"{extra['host_ms']:.1f} ms of wall time per point and moves {extra['host_mb']:.1f} MB per point; largest deviation between the two at one point: "
                     f"{extra['deviation']:.2e} relative, flags {'equal' if extra['flags'] else 'DIFFERENT'}.")
        for key, entry in existing if parent else ():
            (qm, qlo, qhi), om = stats(parent[key]), stats(own[key])[0]
            where = "inside that span" if qlo <= om <= qhi else ("BELOW that span (faster than every call of the parent's)" if om < qlo else "ABOVE that span (SLOWER than every call of the parent's)")
            notes.append(f"- {cfg}: `{entry}` (unchanged code): this build's median is {om:.4f} ms per point, the parent's {qm:.4f} ({om - qm:+.4f}, {100 * (om - qm) / qm:+.2f} %); "
                         f"the parent's own calls span {qlo:.4f} ... {qhi:.4f} (spread {qhi - qlo:.4f}): this build's median lies {where}.")
    text = [TITLE, "",
            f"`tools/point_ranks_time.py` on one MI355X, ONE run on ONE box, nothing tuned.  Every call takes K = {K} points with C = {len(COLUMNS)} quantities ({', '.join(COLUMNS)}); a "
            "device time is that of the call's launches after the log-weight passes by HIP events (`gwi_point_rank_times`: draw tile, draw merge, rank tile, rank merge, rank prefix, PIT "
            "rank, PIT merge; `gwi_point_pit_times`: draw tile, draw merge, histogram tile, CDF segment, PIT; `gwi_histogram_times`: draw tile, draw merge, histogram tile, histogram "
            f"merge) divided by K, a wall time the host clock around the whole call divided by K.  `this`: this build, {a.repeats} calls of each entry in turn after two warm-up calls; "
            "`parent`: "
            + ("the parent commit's build of the engine loaded into child processes of their own, half of the calls before this build's and half after, on the same box.  "
               if a.parent_lib else "NOT MEASURED (no --parent-lib).  ")
            + "Not measured: other C and K, masks, kernel-level counters, config 3.", "", *rows, "", *notes, "", *resources]
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
