#!/usr/bin/env python3
"""Time one of the per-point post-processing entries on the device at the catalogs of BASELINE configs 2 and 5, K = 64 points per call:
the device time per point of the launches after the log-weight passes (HIP events: the entry's gwi_*_times) of every call, its median
and spread over the repeats after two warm-up calls; the same for the existing entries it runs beside, in the same run; and, once, the
wall time per point of the host route it replaces with the largest deviation between the two.  With --parent-lib the same calls are
timed on another build of the engine (the parent commit's), in child processes of their own, half of the calls before this build's and
half after, and this build's median is placed against the span of that build's own calls.  No figure is fixed in advance; what is not
measured is named as unmeasured.  Writes a Markdown report.

      python tools/post_time.py --entry {leave_one_out,point_cdfs,point_pits,point_ranks,point_moments,point_conditionals,point_rankcorr,point_tails,point_bootstrap,hist2d} [--configs c2,c5] [--repeats 10]
                                [--parent-lib PATH] [--out profiles/<entry>/RESULTS.md]

What differs per entry is one record of ENTRIES: the set-up calls, one_round, the host route, the kernels to list and the row labels."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMPOSITION_OF = {"c2": "plpeak", "c3": "bspline_iid", "c5": "bspline_full"}
K = 64
CHILD_LIMIT_S = 900
MASS_Z, MASS_CHI = ("mass_1", "mass_ratio", "redshift"), ("mass_1", "mass_ratio", "chi_eff")
DEVICE = ", device time after the log-weight passes"


# ---- shared: the catalog and the engine of a config, the stage times, the calls, the child process, the report ----------------------
def catalog(cfg, columns):
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.synthetic import make_config_catalog

    name = COMPOSITION_OF[cfg]
    pe, inj, _ = make_config_catalog(cfg)
    comp = COMPOSITIONS[name](pe, inj)
    eng = comp.engine()
    rng = np.random.default_rng(3)
    thetas = np.stack([comp.theta(draw_params(name, rng)) for _ in range(K)])
    x_pe, x_inj = (np.stack([np.asarray(d[k], dtype=np.float64) for k in columns]) for d in (pe, inj))
    return SimpleNamespace(name=name, eng=eng, thetas=thetas, columns=columns, x_pe=x_pe, x_inj=x_inj)


def cdf_codes(c, n_grid):
    """``(grid (C, n_grid), (pe codes, inj codes))``: cumulative codes of the columns against grids between their 1 % and 99 % quantiles."""
    from gwinferno_amd import draws as D

    grid = np.stack([np.linspace(*np.quantile(np.concatenate([p.ravel(), i]), [0.01, 0.99]), n_grid) for p, i in zip(c.x_pe, c.x_inj)])
    return grid, tuple(np.stack([D.cdf_codes(v, g) for v, g in zip(x, grid)]) for x in (c.x_pe, c.x_inj))


def stage_times(fn):
    ms, n = [C.c_double(0.0) for _ in range(3)], C.c_int32(0)
    fn(*[C.byref(m) for m in ms], C.byref(n))
    return [m.value for m in ms]


def timed(out, key, call, times_fn, thetas):
    """One call of an entry: its wall time per point under ``key wall``, its stage times per point ``[logw, stage 1, stage 2]`` returned."""
    t0 = time.perf_counter()
    call()
    out[key + " wall"] = 1e3 * (time.perf_counter() - t0) / len(thetas)
    return [t / len(thetas) for t in stage_times(times_fn)]


def measure(entry, cfg, repeats, full):
    """``full``: the entry itself is timed beside the existing ones, and checked against its host route once."""
    c = catalog(cfg, entry.columns)
    eng = c.eng
    extra = {"shape": f"{eng.n_ev} x {eng.n_pe}, {eng.n_inj}", "name": c.name, "host_mb": 8 * (eng.n_inj + eng.n_ev * eng.n_pe) / 1e6, "n_ev": eng.n_ev}
    entry.setup(c, extra, full)
    entry.one_round(c, c.thetas[:2], full)  # (the first calls load the code object and allocate)
    entry.one_round(c, c.thetas, full)      # ... and one call of the timed shape
    rounds = [entry.one_round(c, c.thetas, full) for _ in range(repeats)]
    if full:
        entry.check(c, extra)
    eng.close()
    return {k: [r[k] for r in rounds] for k in rounds[0]}, extra


def child(entry, cfg, lib, repeats):
    """The same calls on whatever build GWI_ENGINE_LIB names, in a process of its own: the entry itself too where that build has it."""
    env = dict(os.environ, GWI_ENGINE_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--entry", entry.name, "--configs", cfg, "--repeats", str(repeats)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("TIMES ")]
    if res.returncode != 0 or not line:
        raise RuntimeError(f"the child process with {lib} failed ({res.returncode}): {res.stderr[-400:]}")
    return json.loads(line[-1][6:])


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.median(x)), float(x.min()), float(x.max())


def span_note(cfg, what, own, parent, unit=" per point"):
    (qm, qlo, qhi), om = stats(parent), stats(own)[0]
    where = "inside that span" if qlo <= om <= qhi else ("BELOW that span (faster than every call of the parent's)" if om < qlo else "ABOVE that span (SLOWER than every call of the parent's)")
    return (f"- {cfg}: {what}: this build's median is {om:.4f} ms{unit}, the parent's {qm:.4f} ({om - qm:+.4f}, {100 * (om - qm) / qm:+.2f} %); "
            f"the parent's own calls span {qlo:.4f} ... {qhi:.4f} (spread {qhi - qlo:.4f}): this build's median lies {where}.")


def have_device():
    try:
        import torch

        return bool(torch.cuda.is_available())
    except Exception:
        return False


def row_spread(cfg, extra, label, build, x):
    head = f"| {cfg} ({extra['name']}) | {extra['shape']} | {label} | {build}"
    return head + (" | not measured | | | |" if x is None else " ({} calls) | {:.4f} | {:.4f} | {:.4f} | {:.4f} |".format(len(x), *stats(x), stats(x)[2] - stats(x)[1]))


def row_calls(cfg, extra, label, build, x):
    return f"| {cfg} ({extra['shape']}) | {label} | {build} | " + ("%.4f | %.4f | %.4f | %d |" % (*stats(x), len(x)) if x else "not measured | | | |")


STYLES = {
    "spread": SimpleNamespace(row=row_spread, table=["| config | events x samples, injections | entry | build | median (ms per point) | min | max | spread (max - min) |", "|---|---|---|---|---|---|---|---|"],
                              resources=["## The kernels' resources (code object metadata)", "", "| kernel | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes) |", "|---|---|---|---|---|"]),
    "calls": SimpleNamespace(row=row_calls, table=["| config (n_ev x n_pe, n_inj) | what | build | median | min | max | calls |", "|---|---|---|---|---|---|---|"],
                             resources=["## Kernel resources (gfx950 code object)", "", "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes |", "|---|---|---|---|---|"]),
}


def report(entry, a):
    from kernel_resources import kernel_resources

    style, configs = STYLES[entry.style], [c for c in a.configs.split(",") if c]
    res = kernel_resources(entry.kernels)
    resources = style.resources + [f"| `{entry.relabel.get(n, n)}` | {v} | {s} | {lds} | {scr} |" for n, v, s, lds, scr in res] + [""] + (entry.resources_tail(res) if res else [])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not have_device():
        with open(a.out, "w") as f:
            f.write("\n".join([entry.title, "", entry.unmeasured, "", *resources]))
        print(f"no device: wrote {a.out} without times")
        return
    table, notes = [], []
    for cfg in configs:
        half = max(1, a.repeats // 2)
        parent = child(entry, cfg, a.parent_lib, half) if a.parent_lib else None
        own, extra = measure(entry, cfg, a.repeats, True)
        if a.parent_lib and a.repeats > half:
            more = child(entry, cfg, a.parent_lib, a.repeats - half)
            parent = {k: parent[k] + more.get(k, []) for k in parent}
        for key, label in entry.rows:
            table.append(style.row(cfg, extra, label, "this", own[key]))
            if key in entry.compare:
                table.append(style.row(cfg, extra, label, "parent", parent and parent.get(key)))
            print(table[-1], flush=True)
        notes += entry.notes(cfg, own, extra)
        notes += [span_note(cfg, what, own[key], parent[key], unit) for key, what, unit in entry.spans if parent and key in parent]
    how = ("the parent commit's build of the engine loaded into child processes of their own, half of the calls before this build's and half after, on the same box.  "
           if a.parent_lib else "NOT MEASURED (no --parent-lib).  ")
    lines = [entry.title, "", entry.intro(a.repeats, how), "", *style.table, *table, "", *notes, "", *resources]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {a.out}")


def intro(entry, what, events, repeats, how, not_measured):
    return (f"`tools/post_time.py --entry {entry}` on one MI355X, ONE run on ONE box, nothing tuned.  Every call takes K = {K} points with {what}; a device time is that of the "
            f"call's launches after the log-weight passes by HIP events ({events}) divided by K, a wall time the host clock around the whole call divided by K.  `this`: this build, "
            f"{repeats} calls of each entry in turn after two warm-up calls; `parent`: {how}Not measured: {not_measured}.")


def unmeasured(entry, what):
    return f"No GPU was available to `tools/post_time.py --entry {entry}`: NOTHING WAS MEASURED.  Not {what}, not the parent commit."


HIST_EVENTS = "`gwi_histogram_times`: draw tile, draw merge, histogram tile, histogram merge"
PIT_EVENTS = "`gwi_point_pit_times`: draw tile, draw merge, histogram tile, CDF segment, PIT"


def hist_round(c, thetas, out, **kw):
    t = timed(out, "hist", lambda: c.eng.weighted_histograms(thetas, **kw), c.eng.lib.gwi_histogram_times, thetas)
    out["hist"] = t[1] + t[2]


def cdf_round(c, thetas, out):
    t = timed(out, "cdf", lambda: c.eng.point_cdfs(thetas), c.eng.lib.gwi_point_cdf_times, thetas)
    out["cdf"], out["cdf reduce"] = t[1] + t[2], t[2]


def pit_round(c, thetas, out, key="pit"):
    t = timed(out, key, lambda: c.eng.point_pits(thetas), c.eng.lib.gwi_point_pit_times, thetas)
    out[key], out[key + " walk"] = t[1] + t[2], t[2]


def host_route(c, points, reference):
    """Wall time per point (ms) of Engine.log_weights plus ``reference(lw_pe, lw_inj)``, and the last point's result."""
    t0 = time.perf_counter()
    for th in c.thetas[:points]:
        out = reference(*c.eng.log_weights(th))
    return 1e3 * (time.perf_counter() - t0) / points, out


# ---- leave_one_out: the point-weighted device sums (gwi_quant.h, gwi_hist.h) -------------------------------------------------
def loo_setup(c, extra, full):
    from gwinferno_amd import draws as D

    edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.01, 0.99, 65)) for p, i in zip(c.x_pe, c.x_inj)]
    c.eng.set_histogram_bins(np.stack([D.digitize(p, e) for p, e in zip(c.x_pe, edges)]), np.stack([D.digitize(i, e) for i, e in zip(c.x_inj, edges)]), n_bins=64)
    c.v = 2.0 ** np.random.default_rng(4).uniform(-20.0, 0.0, size=(K, c.eng.n_ev + 1))


def loo_round(c, thetas, full):
    out = {}
    for label, kw in (("plain", {}),) + ((("weighted", {"point_weights": c.v[:len(thetas)]}),) if full else ()):
        c.eng.marginal_weights_reset()
        c.eng.marginal_weights_add(thetas, **kw)
        out["add " + label] = stage_times(c.eng.lib.gwi_quantile_times)[1] / len(thetas)
        part = {}
        hist_round(c, thetas, part, **kw)
        out["hist " + label] = part["hist"]
    return out


def loo_notes(cfg, own, extra):
    return [f"- {cfg} `{e}` with weights: {stats(own[k + ' weighted'])[0]:.4f} ms per point against {stats(own[k + ' plain'])[0]:.4f} without "
            f"({100 * (stats(own[k + ' weighted'])[0] - stats(own[k + ' plain'])[0]) / stats(own[k + ' plain'])[0]:+.2f} %); no ratio was promised."
            for e, k in (("marginal_weights_add", "add"), ("weighted_histograms", "hist"))]


# ---- point_cdfs (gwi_cdf.h) ------------------------------------------------------------------------------------------------
def cdfs_setup(c, extra, full):
    c.grid, c.codes = cdf_codes(c, 64)
    c.eng.set_histogram_bins(*c.codes, n_bins=64)


def cdfs_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    if full:
        cdf_round(c, thetas, out)
    return out


def cdfs_check(c, extra):
    from gwinferno_amd import draws as D

    extra["host_ms"], (want, _) = host_route(c, 4, lambda lw_pe, lw_inj: D.point_cdfs_reference(lw_pe, lw_inj, None, None, c.codes[0], c.codes[1], 64))
    got = c.eng.point_cdfs(c.thetas[3])[0][0]
    # slots 0-2 relative to the statement; slot 3 through exp(): log1p(-F) is ill-conditioned where an event's F is within rounding of 1
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(want[:3]) & (want[:3] != 0.0)
        extra["deviation"] = float(np.max(np.abs(got[:3][ok] - want[:3][ok]) / np.abs(want[:3][ok])))
        extra["deviation_sf"] = float(np.max(np.abs(np.exp(got[3]) - np.exp(want[3]))))


def cdfs_notes(cfg, own, extra):
    cm, hm, wm = stats(own["cdf"])[0], stats(own["hist"])[0], stats(own["cdf wall"])[0]
    return [f"- {cfg}: `point_cdfs` takes {cm:.4f} ms of device time per point after the log-weight pass against {hm:.4f} for `weighted_histograms` on the same codes "
            f"({100 * (cm - hm) / hm:+.1f} %), and {wm:.3f} ms of wall time per point with the log-weight pass; {8 * 4 * 3 * 64 + 8} bytes per point go to the host.  The host route "
            f"(`Engine.log_weights` + `draws.point_cdfs_reference`, 4 points, once) takes {extra['host_ms']:.2f} ms of wall time per point and moves "
            f"{extra['host_mb']:.1f} MB per point; largest deviation between the two at one point: {extra['deviation']:.2e} relative in slots 0-2, {extra['deviation_sf']:.2e} absolute in exp(slot 3)."]


# ---- point_pits (gwi_pit.h) ------------------------------------------------------------------------------------------------
def pits_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    cdf_round(c, thetas, out)
    if full:
        pit_round(c, thetas, out)
    return out


def pits_check(c, extra):
    from gwinferno_amd import draws as D

    extra["host_ms"], want = host_route(c, 4, lambda lw_pe, lw_inj: D.point_pits_reference(lw_pe, lw_inj, None, None, c.codes[0], c.codes[1], 64))
    got = c.eng.point_pits(c.thetas[3])
    ok = np.isfinite(want[0])
    extra["deviation"] = float(np.max(np.abs(got[0][0][ok] - want[0][ok]))) if ok.any() else float("nan")
    extra["width"] = float(np.median((want[0][..., 1] - want[0][..., 0])[ok[..., 0]])) if ok.any() else float("nan")
    extra["flags"] = bool(np.array_equal(got[2][0], want[2]))


def pits_notes(cfg, own, extra):
    pm, cm, wm, km = stats(own["pit"])[0], stats(own["cdf"])[0], stats(own["pit wall"])[0], stats(own["pit walk"])[0]
    back = 8 * (2 * extra["n_ev"] * 3 + 3 * 64) + 4 * (extra["n_ev"] + 1)
    return [f"- {cfg}: `point_pits` takes {pm:.4f} ms of device time per point after the log-weight pass, {km:.4f} of it in the CDF segment and PIT launches "
            f"({100 * km / pm:.1f} %), against {cm:.4f} for `point_cdfs` on the same codes ({100 * (pm - cm) / cm:+.1f} %), and {wm:.3f} ms of wall time per point with the "
            f"log-weight pass; {back} bytes per point go to the host.  The host route (`Engine.log_weights` + `draws.point_pits_reference`, 4 points, once) takes "
            f"{extra['host_ms']:.2f} ms of wall time per point and moves {extra['host_mb']:.1f} MB per point; largest deviation between the two at one point: "
            f"{extra['deviation']:.2e} absolute in a bracket end, flags {'equal' if extra['flags'] else 'DIFFERENT'}; median width of a bracket there: {extra['width']:.4f}."]


# ---- point_ranks: the exact per-point PITs (gwi_rank.h) ---------------------------------------------------------------------
def ranks_setup(c, extra, full):
    c.codes = {g: cdf_codes(c, g)[1] for g in (64, 256)}
    if full:
        t0 = time.perf_counter()
        c.eng.set_rank_columns(c.x_pe, c.x_inj)
        extra["setup_s"] = time.perf_counter() - t0


def ranks_round(c, thetas, full):
    out = {}
    for g in (64, 256):
        c.eng.set_histogram_bins(*c.codes[g], n_bins=g)
        if g == 64:
            hist_round(c, thetas, out)
        pit_round(c, thetas, out, f"pit{g}")
    if full:
        t = timed(out, "rank", lambda: c.eng.point_pits_exact(thetas), c.eng.lib.gwi_point_rank_times, thetas)
        out["rank"], out["rank pit"] = t[1] + t[2], t[2]
    return out


def ranks_check(c, extra):
    from gwinferno_amd import draws as D

    codes = D.rank_codes(c.x_pe, c.x_inj)
    extra["host_ms"], want = host_route(c, 2, lambda lw_pe, lw_inj: D.point_pits_exact_reference(lw_pe, lw_inj, None, None, *codes))
    got = c.eng.point_pits_exact(c.thetas[1])
    ok = np.isfinite(want[0])
    extra["deviation"] = float(np.max(np.abs(got[0][0][ok] - want[0][ok]) / want[0][ok])) if ok.any() else float("nan")
    extra["flags"] = bool(np.array_equal(got[1][0], want[1]))


def ranks_notes(cfg, own, extra):
    rm, km, wm = stats(own["rank"])[0], stats(own["rank pit"])[0], stats(own["rank wall"])[0]
    back = 8 * 2 * extra["n_ev"] * 3 + 4 * (extra["n_ev"] + 1)
    return [f"- {cfg}: `point_pits_exact` takes {rm:.4f} ms of device time per point after the log-weight pass, {km:.4f} of it in the two PIT launches "
            f"({100 * km / rm:.1f} %), against {stats(own['pit64'])[0]:.4f} for `point_pits` at G = 64 and {stats(own['pit256'])[0]:.4f} at G = 256, and {wm:.3f} ms of wall "
            f"time per point with the log-weight pass; {back} bytes per point go to the host.  `set_rank_columns` (the sort, the ranks, the checks and the upload, once per "
            f"catalog) took {extra['setup_s']:.2f} s.  The host route (`Engine.log_weights` + `draws.point_pits_exact_reference`, 2 points, once) takes "
            f"{extra['host_ms']:.1f} ms of wall time per point and moves {extra['host_mb']:.1f} MB per point; largest deviation between the two at one point: "
            f"{extra['deviation']:.2e} relative, flags {'equal' if extra['flags'] else 'DIFFERENT'}."]


# ---- point_moments (gwi_moment.h) ------------------------------------------------------------------------------------------
def moments_setup(c, extra, full):
    cdfs_setup(c, extra, full)
    c.eng.set_kde_columns(c.x_pe, c.x_inj)
    c.eng.marginal_weights_reset()
    c.eng.marginal_weights_add(c.thetas[:4])  # (something for weighted_kde to smooth)


def moments_round(c, thetas, full):
    out = {}
    cdf_round(c, thetas, out)
    c.eng.weighted_kde(c.grid)
    t = stage_times(c.eng.lib.gwi_kde_times)
    out["kde"] = t[0] + t[1]
    if full:
        t = timed(out, "moment", lambda: c.eng.point_moments(thetas), c.eng.lib.gwi_point_moment_times, thetas)
        out["moment"], out["moment cov"], out["moment logw"] = t[1] + t[2], t[2], t[0]
    return out


def moments_check(c, extra):
    def reference(lw_pe, lw_inj):
        n_ev, n_cols = c.eng.n_ev, c.x_pe.shape[0]
        mean, cov = np.empty((n_ev + 1, n_cols)), np.empty((n_ev + 1, n_cols, n_cols))
        for seg in range(n_ev + 1):
            lw, x = (lw_pe[seg], c.x_pe[:, seg]) if seg < n_ev else (lw_inj, c.x_inj)
            w = np.exp(lw - lw.max())
            mean[seg], cov[seg] = np.average(x, axis=1, weights=w), np.cov(x, aweights=w, ddof=0)
        return mean, cov

    extra["host_ms"], want = host_route(c, 2, reference)
    got = c.eng.point_moments(c.thetas[1])
    extra["deviation"] = float(np.nanmax(np.abs(got[1][0] - want[1]) / np.sqrt(np.einsum("scc,sdd->scd", want[1], want[1]))))
    extra["dead"] = int(got[2].sum())


def moments_notes(cfg, own, extra):
    return [f"- {cfg}: host route (`Engine.log_weights` + `np.average` / `np.cov(aweights=)` per segment, {extra['host_mb']:.1f} MB to the host per point): {extra['host_ms']:.1f} ms per "
            f"point over 2 points, ONE run, no spread taken.  Largest |device - host| covariance entry of the last of them, as a fraction of sqrt(V_cc V_dd): "
            f"{extra['deviation']:.2e}; dead segments: {extra['dead']}."]


def moments_intro(repeats, how):
    return (f"K = {K} points per call, C = 3 columns ({', '.join(MASS_CHI)}), {repeats} calls per row after two warm-up calls.  Times in ms; device times are HIP-event times of the "
            f"launches after the log-weight pass (draw tile, draw merge and the entry's own), summed over the call and divided by K.  `parent`: {how}".rstrip())


def moments_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed: the {max(r[1] for r in res)} VGPRs of `moment_cov_kernel<8>` hold its 36 running sums without a spill.", ""]


# ---- point_conditionals (gwi_cond.h) ----------------------------------------------------------------------------------------
COND_BINS = 16


def conditionals_setup(c, extra, full):
    from gwinferno_amd import draws as D

    c.edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.01, 0.99, COND_BINS + 1)) for p, i in zip(c.x_pe, c.x_inj)]
    c.codes = tuple(np.stack([D.digitize(v, e) for v, e in zip(x, c.edges)]) for x in (c.x_pe, c.x_inj))
    c.eng.set_histogram_bins(*c.codes, n_bins=COND_BINS)
    c.eng.set_kde_columns(c.x_pe, c.x_inj)
    c.pairs = [(1, 2)]  # chi_eff given the mass-ratio bin


def conditionals_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    t = timed(out, "moment", lambda: c.eng.point_moments(thetas), c.eng.lib.gwi_point_moment_times, thetas)
    out["moment"] = t[1] + t[2]
    if full:
        t = timed(out, "cond", lambda: c.eng.point_conditionals(thetas, c.pairs), c.eng.lib.gwi_point_conditional_times, thetas)
        out["cond"], out["cond var"], out["cond logw"] = t[1] + t[2], t[2], t[0]
    return out


def conditionals_check(c, extra):
    from gwinferno_amd import draws as D

    def reference(lw_pe, lw_inj):
        return D.point_conditionals_reference(lw_pe, lw_inj, c.codes[0], c.codes[1], c.x_pe, c.x_inj, c.pairs, COND_BINS)

    extra["host_ms"], (want, want_dead) = host_route(c, 2, reference)
    share, mean, var, dead = c.eng.point_conditionals(c.thetas[1], c.pairs)
    ok = ~np.isnan(want[:, 0, 2]) & (want[:, 0, 2] > 0.0)
    extra["deviation"] = float(np.max(np.abs(var[0][:, 0][ok] - want[:, 0, 2][ok]) / want[:, 0, 2][ok])) if ok.any() else float("nan")
    extra["flags"] = bool(np.array_equal(dead[0], want_dead)) and bool(np.array_equal(np.isnan(mean[0][:, 0]), np.isnan(want[:, 0, 1])))


def conditionals_notes(cfg, own, extra):
    back = 8 * 3 * (extra["n_ev"] + 1) * COND_BINS + 4 * (extra["n_ev"] + 1)
    return [f"- {cfg}: host route (`Engine.log_weights` + `draws.point_conditionals_reference`, {extra['host_mb']:.1f} MB to the host per point against {back} bytes from the device): "
            f"{extra['host_ms']:.1f} ms per point over 2 points, ONE run, no spread taken.  Largest relative |device - host| conditional variance of the last of them: "
            f"{extra['deviation']:.2e}; flags and NaN positions {'equal' if extra['flags'] else 'DIFFERENT'}."]


def conditionals_intro(repeats, how):
    return (f"K = {K} points per call, C = 3 columns ({', '.join(MASS_CHI)}) as bin columns (B = {COND_BINS}) and as value columns, one pair (chi_eff given the mass-ratio bin), "
            f"{repeats} calls per row after two warm-up calls.  Times in ms; device times are HIP-event times of the launches after the log-weight pass (draw tile, draw merge and the "
            f"entry's own), summed over the call and divided by K.  No ratio was promised in advance.  `parent`: {how}".rstrip())


def conditionals_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed.  `cond_tile_kernel<N, centred>` holds 8 KB of weights and 10 KB per staged column in LDS (N = 1, 2, 4, 8: the "
            "larger number of distinct bin / value columns of the pairs, rounded up), the centred pass 4 KB of means more.", ""]


# ---- point_rankcorr: the per-point rank correlations (gwi_rankcorr.h) --------------------------------------------------------
def rankcorr_setup(c, extra, full):
    cdfs_setup(c, extra, full)
    c.eng.set_kde_columns(c.x_pe, c.x_inj)
    c.eng.set_rank_columns(c.x_pe, c.x_inj)
    if full:
        t0 = time.perf_counter()
        c.eng.set_rankcorr_columns(c.x_pe, c.x_inj)
        extra["setup_s"] = time.perf_counter() - t0


def rankcorr_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    t = timed(out, "rank", lambda: c.eng.point_pits_exact(thetas), c.eng.lib.gwi_point_rank_times, thetas)
    out["rank"] = t[1] + t[2]
    t = timed(out, "moment", lambda: c.eng.point_moments(thetas), c.eng.lib.gwi_point_moment_times, thetas)
    out["moment"] = t[1] + t[2]
    if full:
        t = timed(out, "rankcorr", lambda: c.eng.point_rank_correlations(thetas), c.eng.lib.gwi_point_rankcorr_times, thetas)
        out["rankcorr"], out["rankcorr prefix"], out["rankcorr cov"], out["rankcorr logw"] = t[1] + t[2], t[1], t[2], t[0]
    return out


def rankcorr_check(c, extra):
    from gwinferno_amd import draws as D

    n_cols = c.x_pe.shape[0]
    codes = D.rankcorr_codes(c.x_pe.reshape(n_cols, -1)), D.rankcorr_codes(c.x_inj)
    extra["host_ms"], (want, want_dead) = host_route(c, 2, lambda lw_pe, lw_inj: D.point_rank_correlations_reference(lw_pe, lw_inj, *codes))
    total, mean_rank, cov, dead, dead_set = c.eng.point_rank_correlations(c.thetas[1])
    _, _, want_cov = D.rankcorr_matrix(want, n_cols)
    extra["deviation"] = float(np.nanmax(np.abs(cov[0] - want_cov)))
    extra["mean_error"] = float(np.nanmax(np.abs(mean_rank[0] - 0.5)))
    extra["flags"] = bool(np.array_equal(dead[0], want_dead[:-1])) and int(dead_set[0, 0]) == int(want_dead[-1])
    extra["table_mb"] = 8 * (c.eng.n_ev * c.eng.n_pe + 1) / 1e6


def rankcorr_notes(cfg, own, extra):
    items = 1 + 3 + 6
    return [f"- {cfg}: `set_rankcorr_columns` (the two sorts, the ranks, the checks and the upload, once per catalog) took {extra['setup_s']:.2f} s.  Host route (`Engine.log_weights` + "
            f"`draws.point_rank_correlations_reference`, {extra['host_mb']:.1f} MB to the host per point against {8 * 2 * items + 4 * (extra['n_ev'] + 2)} bytes from the device): "
            f"{extra['host_ms']:.1f} ms per point over 2 points, ONE run, no spread taken.  Largest absolute |device - host| entry of R of the last of them: {extra['deviation']:.2e}; largest "
            f"|m_c - 1/2| on the device: {extra['mean_error']:.2e}; flags {'equal' if extra['flags'] else 'DIFFERENT'}.  The covariance launch gathers 2 C = 6 doubles per sample from "
            f"prefix tables of {extra['table_mb']:.1f} MB per quantity (observed set): its time is the row `... of which the covariance and merge launches`; nothing was tuned for it."]


def rankcorr_intro(repeats, how):
    return (f"K = {K} points per call, C = 3 columns ({', '.join(MASS_CHI)}), {repeats} calls per row after two warm-up calls.  Times in ms; device times are HIP-event times of the "
            f"launches after the log-weight pass (draw tile, draw merge and the entry's own), summed over the call and divided by K.  No ratio was promised in advance.  `parent`: {how}".rstrip())


def rankcorr_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed: the {max(r[1] for r in res)} VGPRs of `rankcorr_cov_kernel<8>` hold its 45 running sums without a spill.", ""]


# ---- point_tails: the per-point tails of the inner importance sums (gwi_tail.h) ----------------------------------------------
def tails_setup(c, extra, full):
    cdfs_setup(c, extra, full)
    c.eng.set_kde_columns(c.x_pe, c.x_inj)
    if full:
        c.eng.set_tail_sizes()  # the rule on n_pe / n_inj
        extra["m"] = c.eng._tail_shape


def tails_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    t = timed(out, "moment", lambda: c.eng.point_moments(thetas), c.eng.lib.gwi_point_moment_times, thetas)
    out["moment"] = t[1] + t[2]
    if full:
        t = timed(out, "tails", lambda: c.eng.point_tails(thetas), c.eng.lib.gwi_point_tail_times, thetas)
        out["tails"], out["tails select"], out["tails collect"], out["tails logw"] = t[1] + t[2], t[1], t[2], t[0]
    return out


def tails_check(c, extra):
    from gwinferno_amd import draws as D

    m_pe, m_inj = extra["m"]
    extra["host_ms"], want = host_route(c, 2, lambda lw_pe, lw_inj: D.point_tails_reference(lw_pe, lw_inj, None, None, m_pe, m_inj))
    got = c.eng.point_tails(c.thetas[1])
    extra["equal"] = bool(np.array_equal(got[0][0], want[0]) and np.array_equal(got[1][0], want[1]) and np.array_equal(got[3][0], want[3])
                          and np.array_equal(got[2][0][:, [0, 3]], want[2][:, [0, 3]]))
    ok = want[2][:, 2] > 0.0
    extra["deviation"] = float(np.max(np.abs(got[2][0][ok, 2] - want[2][ok, 2]) / want[2][ok, 2])) if ok.any() else float("nan")
    extra["bytes"] = 8 * (c.eng.n_ev * m_pe + m_inj + 4 * (c.eng.n_ev + 1)) + 4 * 4 * (c.eng.n_ev + 1)


def tails_notes(cfg, own, extra):
    return [f"- {cfg}: m_pe = {extra['m'][0]}, m_inj = {extra['m'][1]} (the rule).  {extra['bytes']} bytes ({extra['bytes'] / 1e6:.3f} MB) come back per point against {extra['host_mb']:.1f} MB of "
            f"log-weights on the host route (`Engine.log_weights` + `draws.point_tails_reference`): {extra['host_ms']:.1f} ms per point over 2 points, ONE run, no spread taken.  tail, counts, "
            f"max and below_max of the last of them {'EQUAL the statement in every bit' if extra['equal'] else 'DIFFER from the statement'}; largest relative |device - host| body: "
            f"{extra['deviation']:.2e}."]


def tails_intro(repeats, how):
    return (f"K = {K} points per call, the default tail sizes, {repeats} calls per row after two warm-up calls.  Times in ms; device times are HIP-event times of the launches after the "
            f"log-weight pass, summed over the call and divided by K: `selection` is draw tile, draw merge and the six passes of histogram and pick, `collection` the collect and merge "
            f"launches.  No ratio was promised in advance.  The digit widths (11, 11, 11, 11, 10, 10 bits: six passes) were not chosen by measurement; no alternative was timed.  "
            f"`parent`: {how}".rstrip())


def tails_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed.  `tail_hist_kernel` and `tail_pick_kernel` hold one pass's 2 048 counters (8 KB) in LDS, `tail_merge_kernel` the "
            "4 096 keys it sorts (32 KB).", ""]


# ---- point_bootstrap: bootstrap replicates of the inner importance sums (gwi_boot.h) ------------------------------------------
BOOT_REPLICATES, BOOT_SEED = 128, 1


def boot_setup(c, extra, full):
    tails_setup(c, extra, False)
    c.eng.set_tail_sizes()
    if full:
        c.eng.set_bootstrap(BOOT_SEED, BOOT_REPLICATES)


def boot_round(c, thetas, full):
    out = {}
    hist_round(c, thetas, out)
    t = timed(out, "tails", lambda: c.eng.point_tails(thetas), c.eng.lib.gwi_point_tail_times, thetas)
    out["tails"] = t[1] + t[2]
    if full:
        t = timed(out, "boot", lambda: c.eng.point_bootstrap(thetas), c.eng.lib.gwi_point_bootstrap_times, thetas)
        out["boot"], out["boot tile"], out["boot merge"], out["boot logw"] = t[1] + t[2], t[1], t[2], t[0]
    return out


def boot_check(c, extra):
    from gwinferno_amd import draws as D

    extra["host_ms"], want = host_route(c, 2, lambda lw_pe, lw_inj: D.point_bootstrap_reference(lw_pe, lw_inj, None, BOOT_SEED, BOOT_REPLICATES))
    got = c.eng.point_bootstrap(c.thetas[1])
    extra["equal"] = bool(np.array_equal(got[3], want[3]) and np.array_equal(got[2][0], want[2]) and np.array_equal(got[1][0][:, 0], want[1][:, 0]))
    ok = want[0] > 0.0
    extra["deviation"] = float(np.max(np.abs(got[0][0][ok] - want[0][ok]) / want[0][ok])) if ok.any() else float("nan")
    extra["bytes"] = (c.eng.n_ev + 1) * (8 * (BOOT_REPLICATES + 2) + 4)
    extra["count_bytes"] = 8 * (c.eng.n_ev + 1) * BOOT_REPLICATES


def boot_notes(cfg, own, extra):
    return [f"- {cfg}: B = {BOOT_REPLICATES} replicates.  {extra['bytes']} bytes ({extra['bytes'] / 1e6:.3f} MB) come back per point, and {extra['count_bytes']} bytes of counts once per call, "
            f"against {extra['host_mb']:.1f} MB of log-weights per point on the host route (`Engine.log_weights` + `draws.point_bootstrap_reference`): {extra['host_ms']:.1f} ms per point over "
            f"2 points, ONE run, no spread taken.  counts, dead and M of the last of them {'EQUAL the statement in every bit' if extra['equal'] else 'DIFFER from the statement'}; largest "
            f"relative |device - host| of a sum: {extra['deviation']:.2e}."]


def boot_intro(repeats, how):
    return (f"K = {K} points per call, B = {BOOT_REPLICATES} replicates, {repeats} calls per row after two warm-up calls.  ONE run, nothing tuned, no ratio promised.  Times in ms; device "
            f"times are HIP-event times of the launches after the log-weight pass, summed over the call and divided by K: `tile` is draw tile, draw merge and the bootstrap tile launch, "
            f"`merge` the bootstrap merge launch.  The block shape (8 slices of 128 samples x 32 replicate groups) was not chosen by measurement; no alternative was timed.  "
            f"`parent`: {how}".rstrip())


def boot_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed.  `boot_tile_kernel` holds the tile's 1 024 weights (8 KB), a byte per sample, and the 8 x 128 slice sums and "
            "counts of a pass (8 KB + 4 KB) in LDS.", ""]


# ---- hist2d: the per-point joint histograms (gwi_hist2d.h) --------------------------------------------------------------------
H2D_BINS = (32, 64)
MASS_PAIR = ("mass_1", "mass_ratio")


def hist2d_setup(c, extra, full):
    from gwinferno_amd import draws as D

    c.codes = {}
    for b in H2D_BINS:
        edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.01, 0.99, b + 1)) for p, i in zip(c.x_pe, c.x_inj)]
        c.codes[b] = tuple(np.stack([D.digitize(v, e) for v, e in zip(x, edges)]) for x in (c.x_pe, c.x_inj))
    c.eng.set_kde_columns(c.x_pe, c.x_inj)
    c.eng.marginal_weights_reset()
    c.eng.marginal_weights_add(c.thetas[:4])  # (something for weighted_kde2d to smooth)
    c.grids = [np.linspace(*np.quantile(np.concatenate([p.ravel(), i]), [0.01, 0.99]), 128) for p, i in zip(c.x_pe, c.x_inj)]
    n_tiles = c.eng.n_ev * -(-c.eng.n_pe // 1024) + -(-c.eng.n_inj // 1024)
    extra["workspace"] = {b: 8 * b * b * (n_tiles + c.eng.n_ev + 1 + 2 * K) for b in H2D_BINS}


def hist2d_round(c, thetas, full):
    out = {}
    c.rounds = getattr(c, "rounds", 0) + 1
    for b in H2D_BINS if c.rounds % 2 else H2D_BINS[::-1]:  # (the two bin counts take turns at being first after the bins are set)
        c.eng.set_histogram_bins(*c.codes[b], n_bins=b)
        if full:
            c.eng.point_histograms2d(thetas[:2], [(0, 1)], accumulate=False)  # (untimed: the first call after new bins)
            key = f"h2d{b}"
            t = timed(out, key, lambda: c.eng.point_histograms2d(thetas, [(0, 1)], accumulate=False), c.eng.lib.gwi_point_hist2d_times, thetas)
            out[key], out[key + " tile"], out[key + " merge"] = t[1] + t[2], t[1], t[2]
    c.eng.set_histogram_bins(*c.codes[H2D_BINS[-1]], n_bins=H2D_BINS[-1])
    hist_round(c, thetas, out)  # (B = 64, the same two columns)
    t = timed(out, "cond", lambda: c.eng.point_conditionals(thetas, [(0, 1)]), c.eng.lib.gwi_point_conditional_times, thetas)
    out["cond"] = t[1] + t[2]
    c.eng.weighted_kde2d([(0, 1)], c.grids[0], c.grids[1])
    t = stage_times(c.eng.lib.gwi_kde_times)
    out["kde2d"] = t[0] + t[1]
    return out


def hist2d_check(c, extra):
    b = H2D_BINS[-1]
    c.eng.set_histogram_bins(*c.codes[b], n_bins=b)
    edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.01, 0.99, b + 1)) for p, i in zip(c.x_pe, c.x_inj)]

    def table(lw, x):
        live = np.isfinite(lw)
        if not live.any():
            return None
        w = np.where(live, np.exp(np.where(live, lw, 0.0) - lw[live].max()), 0.0)
        return np.histogram2d(x[0], x[1], bins=edges, weights=w)[0] / w.sum()

    def reference(lw_pe, lw_inj):  # the host route: Engine.log_weights + np.histogram2d of every event and of the injection set, the mixture
        events = [t for t in (table(lw_pe[e], c.x_pe[:, e]) for e in range(lw_pe.shape[0])) if t is not None]
        return sum(events) / len(events), table(lw_inj, c.x_inj)

    extra["host_ms"], want = host_route(c, 2, reference)
    got = c.eng.point_histograms2d(c.thetas[1], [(0, 1)], accumulate=False)
    worst, same = 0.0, True
    for mine, theirs in ((got["obs"][0, 0], want[0]), (got["pred"][0, 0], want[1])):
        ok = theirs > 0.0
        worst = max(worst, float(np.max(np.abs(mine[ok] - theirs[ok]) / theirs[ok])))
        same = same and bool(np.array_equal(mine > 0.0, ok))
    extra["deviation"], extra["flags"] = worst, same


def hist2d_notes(cfg, own, extra):
    return [f"- {cfg}: host route (`Engine.log_weights` + `np.histogram2d` of every event and of the injection set, the mixture formed on the host: the same work, {extra['host_mb']:.1f} MB to the host per point against "
            f"{2 * 8 * H2D_BINS[-1] ** 2 + 8} bytes from the device at B = {H2D_BINS[-1]}): {extra['host_ms']:.1f} ms per point over 2 points, ONE run, no spread taken.  Largest relative "
            f"|device - host| cell of the observed and the predicted table of the last of them: {extra['deviation']:.2e}; occupied cells {'equal' if extra['flags'] else 'DIFFERENT'}.",
            f"- {cfg}: workspace (one pair's partials and shares, the staged rows of 64 points): " + ", ".join(f"{extra['workspace'][b] / 1e6:.1f} MB at B = {b}" for b in H2D_BINS)
            + "; returned per point: " + ", ".join(f"{2 * 8 * b * b + 8} bytes at B = {b}" for b in H2D_BINS) + "."]


def hist2d_intro(repeats, how):
    return (f"K = {K} points per call, C = 2 bin columns ({', '.join(MASS_PAIR)}), one pair, B = {H2D_BINS[0]} and {H2D_BINS[1]}, accumulate=False, {repeats} calls per row after two "
            f"warm-up calls; the two bin counts take turns at being first in a round, and each timed call follows one untimed call of two points after the bins were set.  ONE run on ONE box: no spread between runs or boxes was taken.  Nothing was tuned: the owner rule (cell j mod 256), four codes per LDS read and the 256-cell merge "
            f"blocks are the first shapes written; no alternative was timed.  No ratio was promised in advance.  Times in ms; device times are HIP-event times of the launches after the "
            f"log-weight pass, summed over the call and divided by K: `tile` is draw tile, draw merge and the joint tile launch, `merge + mix` the two launches after it.  `weighted_kde2d` "
            f"is one 128 x 128 map of one pair under the marginal weights of 4 points, per query.  `parent`: {how}".rstrip())


def hist2d_tail(res):
    return [f"Scratch is {max(r[4] for r in res)} bytes in every kernel listed.  `hist2d_tile_kernel` holds 8 KB of weights and 2 KB of joint codes in static LDS and the B x B cells in dynamic "
            "LDS (8 KB at B = 32, 32 KB at B = 64), which the column above does not show.", ""]


QUANTITIES = f"C = 3 quantities ({', '.join(MASS_Z)})"
WEIGHTED_LABEL = {"hist_merge_kernel<true>": "hist_merge_kernel<true> (weighted)", "marg_add_kernel<true>": "marg_add_kernel<true> (weighted)"}
COMMON = dict(style="spread", columns=MASS_Z, relabel={}, resources_tail=lambda res: [], check=lambda c, extra: None)


def record(**own):
    return SimpleNamespace(**{**COMMON, **own})


ENTRIES = {e.name: e for e in (
    record(relabel=WEIGHTED_LABEL, name="leave_one_out", symbol="gwi_weighted_histograms_weighted", title="# Point-weighted device sums: measured times",
           kernels="marg_add_kernel|hist_merge_kernel|hist_tile_kernel", setup=loo_setup, one_round=loo_round, notes=loo_notes,
           rows=[("add plain", "marginal_weights_add"), ("add weighted", "marginal_weights_add, weighted"), ("hist plain", "weighted_histograms"),
                 ("hist weighted", "weighted_histograms, weighted")],
           compare=("add plain", "hist plain", "add weighted", "hist weighted"),
           spans=[("add plain", "`marginal_weights_add` without weights", " per point"), ("hist plain", "`weighted_histograms` without weights", " per point"),
                  ("add weighted", "`marginal_weights_add` with weights", " per point"), ("hist weighted", "`weighted_histograms` with weights", " per point")],
           intro=lambda repeats, how: intro("leave_one_out", "C = 3, B = 64, with and without weights in turn (the weights log-uniform in [2^-20, 1])",
                                            "`gwi_quantile_times`: draw tile, draw merge, marginal add; " + HIST_EVENTS, repeats, how,
                                            "the log-weight passes (unchanged), other K, masks, kernel-level counters"),
           unmeasured=unmeasured("leave_one_out", "the weighted entries, not the entries without weights")),
    record(check=cdfs_check, relabel=WEIGHTED_LABEL, name="point_cdfs", symbol="gwi_point_cdfs", title="# Per-point CDFs: measured times", kernels="cdf_segment_kernel|cdf_catalog_kernel|hist_tile_kernel|hist_merge_kernel",
           setup=cdfs_setup, one_round=cdfs_round, notes=cdfs_notes,
           rows=[("cdf", "point_cdfs" + DEVICE), ("cdf reduce", "... of which the two CDF launches"), ("cdf wall", "point_cdfs, wall"), ("hist wall", "weighted_histograms, wall"),
                 ("hist", "weighted_histograms" + DEVICE)],
           compare=("cdf", "hist"), spans=[("cdf", "`point_cdfs`", " per point"), ("hist", "`weighted_histograms`", " per point")],
           intro=lambda repeats, how: intro("point_cdfs", QUANTITIES + " and G = 64 grid points",
                                            "`gwi_point_cdf_times`: draw tile, draw merge, histogram tile, CDF segment, CDF catalog; " + HIST_EVENTS, repeats, how,
                                            "other C, G and K, masks, kernel-level counters"),
           unmeasured=unmeasured("point_cdfs", "`point_cdfs`, not `weighted_histograms`, not the host route")),
    record(check=pits_check, name="point_pits", symbol="gwi_point_pits", title="# Per-point PIT brackets: measured times", kernels="pit_kernel|cdf_segment_kernel|cdf_catalog_kernel|hist_tile_kernel",
           setup=cdfs_setup, one_round=pits_round, notes=pits_notes,
           rows=[("pit", "point_pits" + DEVICE), ("pit walk", "... of which the CDF segment + PIT launches"), ("pit wall", "point_pits, wall"), ("cdf", "point_cdfs" + DEVICE),
                 ("hist", "weighted_histograms" + DEVICE)],
           compare=("pit", "cdf", "hist"), spans=[("pit", "`point_pits`", " per point"), ("cdf", "`point_cdfs`", " per point"), ("hist", "`weighted_histograms`", " per point")],
           intro=lambda repeats, how: intro("point_pits", QUANTITIES + " and G = 64 grid points",
                                            PIT_EVENTS + "; `gwi_point_cdf_times`: the same with CDF catalog in the place of PIT; " + HIST_EVENTS, repeats, how,
                                            "other C, G and K, masks, kernel-level counters"),
           unmeasured=unmeasured("point_pits", "`point_pits`, not `point_cdfs`, not `weighted_histograms`, not the host route")),
    record(name="point_ranks", symbol="gwi_point_pits_exact", title="# Exact per-point PITs: measured times",
           kernels="rank_tile_kernel|rank_merge_kernel|rank_prefix_kernel|pit_rank_kernel|pit_rank_merge_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=ranks_setup, one_round=ranks_round, notes=ranks_notes,
           rows=[("rank", "point_pits_exact" + DEVICE), ("rank pit", "... of which the two PIT launches"), ("rank wall", "point_pits_exact, wall"),
                 ("pit64", "point_pits, G = 64" + DEVICE), ("pit256", "point_pits, G = 256" + DEVICE), ("hist", "weighted_histograms, G = 64" + DEVICE)],
           compare=("rank", "pit64", "pit256", "hist"),
           spans=[("rank", "`point_pits_exact`", " per point"), ("pit64", "`point_pits, G = 64`", " per point"), ("pit256", "`point_pits, G = 256`", " per point"),
                  ("hist", "`weighted_histograms, G = 64`", " per point")],
           intro=lambda repeats, how: intro("point_ranks", QUANTITIES, "`gwi_point_rank_times`: draw tile, draw merge, rank tile, rank merge, rank prefix, PIT rank, PIT merge; "
                                            + PIT_EVENTS + "; " + HIST_EVENTS, repeats, how, "other C and K, masks, kernel-level counters, config 3"),
           unmeasured=unmeasured("point_ranks", "`point_pits_exact`, not `point_pits`, not `weighted_histograms`, not the host route"), check=ranks_check),
    record(style="calls", columns=MASS_CHI, resources_tail=moments_tail, name="point_moments", symbol="gwi_point_moments",
           title="# Per-point moments: measured times", kernels="moment_sum_kernel|moment_mean_kernel|moment_cov_kernel|moment_merge_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=moments_setup, one_round=moments_round, notes=moments_notes, check=moments_check, intro=moments_intro,
           rows=[("moment", "`point_moments`, device time per point after the log-weight pass"), ("moment cov", "... of which the two covariance launches"),
                 ("moment logw", "`point_moments`, log-weight pass per point (host clock)"), ("moment wall", "`point_moments`, wall time per point of the call"),
                 ("cdf", "`point_cdfs`, device time per point after the log-weight pass"), ("kde", "`weighted_kde`, device time per query")],
           compare=("moment", "cdf", "kde"), spans=[("moment", "`point_moments`", " per point"), ("cdf", "`point_cdfs`", " per point"), ("kde", "`weighted_kde`", " per query")],
           unmeasured="NOT MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
    record(style="calls", columns=MASS_CHI, resources_tail=conditionals_tail, name="point_conditionals", symbol="gwi_point_conditionals",
           title="# Per-point conditional moments: measured times", kernels="cond_tile_kernel|cond_mean_kernel|cond_var_kernel|hist_tile_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=conditionals_setup, one_round=conditionals_round, notes=conditionals_notes, check=conditionals_check, intro=conditionals_intro,
           rows=[("cond", "`point_conditionals`, device time per point after the log-weight pass"), ("cond var", "... of which the two variance launches"),
                 ("cond logw", "`point_conditionals`, log-weight pass per point (host clock)"), ("cond wall", "`point_conditionals`, wall time per point of the call"),
                 ("moment", "`point_moments`, device time per point after the log-weight pass"), ("hist", "`weighted_histograms`, device time per point after the log-weight pass")],
           compare=("moment", "hist"), spans=[("moment", "`point_moments` (unchanged code)", " per point"), ("hist", "`weighted_histograms` (unchanged code)", " per point")],
           unmeasured="NOT MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
    record(style="calls", columns=MASS_CHI, resources_tail=rankcorr_tail, name="point_rankcorr", symbol="gwi_point_rank_correlations",
           title="# Per-point rank correlations: measured times",
           kernels="rankcorr_tile_kernel|rankcorr_offset_kernel|rankcorr_prefix_kernel|rankcorr_cov_kernel|rankcorr_merge_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=rankcorr_setup, one_round=rankcorr_round, notes=rankcorr_notes, check=rankcorr_check, intro=rankcorr_intro,
           rows=[("rankcorr", "`point_rank_correlations`, device time per point after the log-weight pass"), ("rankcorr prefix", "... of which draw tile / merge, tile sums, offsets, prefix"),
                 ("rankcorr cov", "... of which the covariance and merge launches"), ("rankcorr logw", "`point_rank_correlations`, log-weight pass per point (host clock)"),
                 ("rankcorr wall", "`point_rank_correlations`, wall time per point of the call"), ("rank", "`point_pits_exact`, device time per point after the log-weight pass"),
                 ("moment", "`point_moments`, device time per point after the log-weight pass"), ("hist", "`weighted_histograms`, device time per point after the log-weight pass")],
           compare=("rank", "moment", "hist"),
           spans=[("rank", "`point_pits_exact` (unchanged code)", " per point"), ("moment", "`point_moments` (unchanged code)", " per point"),
                  ("hist", "`weighted_histograms` (unchanged code)", " per point")],
           unmeasured="NOT MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
    record(style="calls", columns=MASS_CHI, resources_tail=tails_tail, name="point_tails", symbol="gwi_point_tails", title="# Per-point tails of the inner importance sums: measured times",
           kernels="tail_hist_kernel|tail_pick_kernel|tail_collect_kernel|tail_merge_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=tails_setup, one_round=tails_round, notes=tails_notes, check=tails_check, intro=tails_intro,
           rows=[("tails", "`point_tails`, device time per point after the log-weight pass"), ("tails select", "... of which draw tile / merge and the selection's twelve launches"),
                 ("tails collect", "... of which the collect and merge launches"), ("tails logw", "`point_tails`, log-weight pass per point (host clock)"),
                 ("tails wall", "`point_tails`, wall time per point of the call"), ("moment", "`point_moments`, device time per point after the log-weight pass"),
                 ("hist", "`weighted_histograms`, device time per point after the log-weight pass")],
           compare=("moment", "hist"), spans=[("moment", "`point_moments` (unchanged code)", " per point"), ("hist", "`weighted_histograms` (unchanged code)", " per point")],
           unmeasured="NOT MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
    record(style="calls", columns=MASS_CHI, resources_tail=boot_tail, name="point_bootstrap", symbol="gwi_point_bootstrap", title="# Bootstrap replicates of the importance sums: measured times",
           kernels="boot_tile_kernel|boot_merge_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=boot_setup, one_round=boot_round, notes=boot_notes, check=boot_check, intro=boot_intro,
           rows=[("boot", "`point_bootstrap`, device time per point after the log-weight pass"), ("boot tile", "... of which draw tile / merge and the bootstrap tile launch"),
                 ("boot merge", "... of which the merge launch"), ("boot logw", "`point_bootstrap`, log-weight pass per point (host clock)"),
                 ("boot wall", "`point_bootstrap`, wall time per point of the call"), ("tails", "`point_tails`, device time per point after the log-weight pass"),
                 ("hist", "`weighted_histograms`, device time per point after the log-weight pass")],
           compare=("tails", "hist"), spans=[("tails", "`point_tails` (unchanged code; a difference is process noise)", " per point"),
                                             ("hist", "`weighted_histograms` (unchanged code; a difference is process noise)", " per point")],
           unmeasured="NOTHING WAS MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
    record(style="calls", columns=MASS_PAIR, resources_tail=hist2d_tail, name="hist2d", symbol="gwi_point_histograms2d", title="# Per-point joint histograms: measured times",
           kernels="hist2d_tile_kernel|hist2d_merge_kernel|hist2d_mix_kernel|hist_tile_kernel|draw_tile_kernel|draw_merge_kernel",
           setup=hist2d_setup, one_round=hist2d_round, notes=hist2d_notes, check=hist2d_check, intro=hist2d_intro,
           rows=[(f"h2d{b}{part}", f"`point_histograms2d`, B = {b}{label}") for b in H2D_BINS
                 for part, label in (("", ", device time per point after the log-weight pass"), (" tile", ": ... of which draw tile / merge and the joint tile launch"),
                                     (" merge", ": ... of which merge + mix"), (" wall", ", wall time per point of the call"))]
           + [("hist", "`weighted_histograms`, the same two columns, B = 64, device time per point after the log-weight pass"),
              ("cond", "`point_conditionals`, one pair, B = 64, device time per point after the log-weight pass"), ("kde2d", "`weighted_kde2d`, one 128 x 128 pair, device time per query")],
           compare=("hist", "cond"), spans=[("hist", "`weighted_histograms` (unchanged code)", " per point"), ("cond", "`point_conditionals` (unchanged code)", " per point")],
           unmeasured="NOTHING WAS MEASURED: no GPU was available where this file was written.  No time, no ratio and no comparison with the host route or the parent commit is claimed."),
)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", required=True, choices=sorted(ENTRIES))
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="another build of libgwi_engine.so (the parent commit's): the same calls are timed on it in child processes")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="the report (default: profiles/<entry>/RESULTS.md)")
    a = ap.parse_args()
    entry = ENTRIES[a.entry]
    if a.child:  # (what child() runs: one TIMES line; the entry itself only where this build of the library has it)
        from gwinferno_amd import _native

        times, _ = measure(entry, a.configs, a.repeats, hasattr(_native.load_library(), entry.symbol))
        print("TIMES " + json.dumps(times), flush=True)
        return
    a.out = a.out or os.path.join(ROOT, "profiles", a.entry, "RESULTS.md")
    report(entry, a)


if __name__ == "__main__":
    main()
