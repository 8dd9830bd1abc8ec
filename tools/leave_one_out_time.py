#!/usr/bin/env python3
"""Time the point-weighted device sums (gwi_marginal_weights_add_weighted, gwi_weighted_histograms_weighted; gwinferno_amd/csrc/
gwi_quant.h, gwi_hist.h) beside the entries without weights at the catalogs of BASELINE configs 2 and 5, 64 points per
call: the device time per point (HIP events: gwi_quantile_times, gwi_histogram_times) of every call, its median and spread over the
repeats.  With --parent-lib the entries without weights are timed on another build of the engine too (the parent commit's), in child
processes of their own before and after this build's calls, and the two are compared against that build's own run-to-run spread.  No
ratio is fixed in advance for the weighted entries; what is not measured is named as unmeasured.  Writes a Markdown report.
      python tools/leave_one_out_time.py [--configs c2,c5] [--repeats 10] [--parent-lib PATH] [--out profiles/leave_one_out/RESULTS.md]"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}
COLUMNS = ("mass_1", "mass_ratio", "redshift")
N_BINS = 64
K = 64


def kernel_resources():
    """VGPRs, SGPRs, LDS and scratch of the kernels the weights touch, from the code object's metadata."""
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
        found = re.search(r"(marg_add_kernel|hist_merge_kernel|hist_tile_kernel)(ILb([01])E)?", name.group(1)) if name else None
        if not found:
            continue
        label = found.group(1) + ("" if found.group(3) is None else ("<true> (weighted)" if found.group(3) == "1" else "<false>"))
        get = lambda key: re.search(r"\.%s:\s+(\d+)" % key, block).group(1)  # noqa: E731
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
    edges = {k: np.quantile(np.concatenate([pe[k].ravel(), inj[k]]), np.linspace(0.01, 0.99, N_BINS + 1)) for k in COLUMNS}
    eng.set_histogram_bins(np.stack([D.digitize(pe[k], edges[k]) for k in COLUMNS]), np.stack([D.digitize(inj[k], edges[k]) for k in COLUMNS]), n_bins=N_BINS)
    v = 2.0 ** np.random.default_rng(4).uniform(-20.0, 0.0, size=(K, eng.n_ev + 1))
    return name, eng, thetas, v


def stage_times(fn):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    fn(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms]


def one_round(eng, thetas, v, weighted):
    """Device time per point (ms) of one marginal_weights_add and one weighted_histograms call of K points, with and without weights:
    the launches after the log-weight passes, by HIP events."""
    out = {}
    for label, kw in (("plain", {}),) + ((("weighted", {"point_weights": v}),) if weighted else ()):
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas, **kw)
        out["add " + label] = stage_times(eng.lib.gwi_quantile_times)[1] / K
        eng.weighted_histograms(thetas, **kw)
        t = stage_times(eng.lib.gwi_histogram_times)
        out["hist " + label] = (t[1] + t[2]) / K
    return out


def measure(cfg, repeats, weighted):
    name, eng, thetas, v = setup(cfg)
    one_round(eng, thetas[:1], v[:1], weighted)  # (the first calls load the code object and allocate)
    rounds = [one_round(eng, thetas, v, weighted) for _ in range(repeats)]
    shape = f"{eng.n_ev} x {eng.n_pe}, {eng.n_inj}"
    eng.close()
    return name, shape, {k: [r[k] for r in rounds] for k in rounds[0]}


def child(cfg, lib, repeats):
    """The entries without weights of whatever build GWI_ENGINE_LIB names, in a process of its own."""
    env = dict(os.environ, GWI_ENGINE_LIB=lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--configs", cfg, "--repeats", str(repeats)], env=env, capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--parent-lib", default=None, help="another build of libgwi_engine.so (the parent commit's): its entries without weights are timed in child processes")
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leave_one_out", "RESULTS.md"))
    a = ap.parse_args()
    if a.plain_only:
        _, _, times = measure(a.configs, a.repeats, weighted=False)
        print("TIMES " + json.dumps(times), flush=True)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = kernel_resources()
    resources = ["## The kernels' resources (code object metadata)", "", "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|",
                 *(f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} |" for r in res), ""]
    if not have_device():
        with open(a.out, "w") as f:
            f.write("\n".join(["# Point-weighted device sums: measured times", "", "No GPU was available to `tools/leave_one_out_time.py`: NOTHING WAS MEASURED.  Not the weighted "
                               "entries, not the entries without weights, not the parent commit.", "", *resources]))
        print(f"no device: wrote {a.out}")
        return
    rows = ["| config | events x samples, injections | entry | build | median (ms per point) | min | max | spread (max - min) |", "|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for cfg in a.configs.split(","):
        half = max(1, a.repeats // 2)
        parent = child(cfg, a.parent_lib, half) if a.parent_lib else None
        name, shape, own = measure(cfg, a.repeats, weighted=True)
        if a.parent_lib:
            more = child(cfg, a.parent_lib, a.repeats - half) if a.repeats > half else {}
            parent = {k: parent[k] + more.get(k, []) for k in parent}
        for entry, key in (("marginal_weights_add", "add"), ("weighted_histograms", "hist")):
            for build, times in (("parent", parent and parent[key + " plain"]), ("this", own[key + " plain"]), ("this, weighted", own[key + " weighted"])):
                if times is None:
                    rows.append(f"| {cfg} ({name}) | {shape} | {entry} | {build} | not measured | | | |")
                    continue
                med, lo, hi = stats(times)
                rows.append(f"| {cfg} ({name}) | {shape} | {entry} | {build} ({len(times)} calls) | {med:.4f} | {lo:.4f} | {hi:.4f} | {hi - lo:.4f} |")
                print(rows[-1], flush=True)
            if parent:
                (pm, plo, phi), (om, _, _) = stats(parent[key + " plain"]), stats(own[key + " plain"])
                slower = om - pm
                verdicts.append(f"- {cfg} `{entry}` without weights: this build's median is {om:.4f} ms per point, the parent's {pm:.4f} ({slower:+.4f}, {100 * slower / pm:+.2f} %); the "
                                f"parent's own spread is {phi - plo:.4f}: " + ("not slower than the parent by more than its spread." if slower <= phi - plo else
                                                                                f"SLOWER than the parent by {slower - (phi - plo):.4f} ms per point more than its spread."))
            wm, om = stats(own[key + " weighted"])[0], stats(own[key + " plain"])[0]
            verdicts.append(f"- {cfg} `{entry}` with weights: {wm:.4f} ms per point against {om:.4f} without ({100 * (wm - om) / om:+.2f} %); no ratio was promised.")
    text = ["# Point-weighted device sums: measured times", "",
            f"`tools/leave_one_out_time.py` on one MI355X, ONE run on ONE box, nothing tuned.  Every call adds K = {K} points; the figure is the device time of the call's launches after "
            "the log-weight passes (HIP events: `gwi_quantile_times` -- draw tile, draw merge, marginal add -- and `gwi_histogram_times` -- draw tile, draw merge, histogram tile, "
            f"histogram merge; C = {len(COLUMNS)}, B = {N_BINS}) divided by K.  `this`: this build, {a.repeats} calls of each entry, with and without weights in turn; `parent`: "
            + ("the parent commit's build of the engine loaded into child processes of their own, half of the calls before this build's and half after, on the same box.  "
               if a.parent_lib else "NOT MEASURED (no --parent-lib).  ")
            + "The weights are log-uniform in [2^-20, 1].  Not measured: the log-weight passes (unchanged), other K, masks, kernel-level counters.", "", *rows, "", *verdicts, "", *resources]
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
