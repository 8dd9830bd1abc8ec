#!/usr/bin/env python3
"""Measurement (GPU box): wide (float64) against narrow (float32, narrow_columns="auto") spline coordinates on the BASELINE
catalogs whose spline coordinates -- spin magnitudes and tilts, and the mass ratio -- are cast through float32, so that both
engines read the same numbers and give the same bits (tests/test_gpu_narrow_columns.py).

  time CFG OUT.json          both engines in one process, interleaved: step us (gwi_eval_sequence, blocking value + gradient),
                             scan us from the engine's own HIP events, K = 16 batched evaluations per second on the kernel the
                             static rule picks, resident bytes (gwi_resident_bytes)
  scan CFG MODE [N]          N sequential evaluations of ONE engine (MODE wide | narrow) and nothing else: what the
                             `rocprofv3 --kernel-trace --stats` and `--pmc` runs trace
  summarize DIR OUT_DIR      every time_*.json and rocprofv3 CSV under DIR -> OUT_DIR/narrow_columns.json + a table on stdout

The job script runs each step under its own time limit (profiles/narrow_columns/RESULTS.md has the commands)."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COORDS = ("mass_ratio", "a_1", "a_2", "cos_tilt_1", "cos_tilt_2")


def _catalog(cfg):
    from bench import CONFIGS
    from gwinferno_amd.synthetic import make_config_catalog

    comp_name, cat, _, _ = CONFIGS[cfg]
    pe, inj, total = make_config_catalog(cat)
    for k in COORDS:
        pe[k] = pe[k].astype(np.float32).astype(np.float64)
        inj[k] = inj[k].astype(np.float32).astype(np.float64)
    return comp_name, pe, inj, total


def _engine(comp_name, pe, inj, mode):
    from gwinferno_amd.compositions import COMPOSITIONS

    comp = COMPOSITIONS[comp_name](pe, inj)
    eng = comp.engine(narrow_columns="auto" if mode == "narrow" else False)
    return comp, eng


def _thetas(comp_name, comp, n):
    from gwinferno_amd.compositions import draw_params

    rng = np.random.default_rng(0)
    return np.ascontiguousarray(np.stack([comp.theta(draw_params(comp_name, rng)) for _ in range(n)]))


def cmd_time(cfg, out):
    comp_name, pe, inj, total = _catalog(cfg)
    runs = {m: _engine(comp_name, pe, inj, m) for m in ("wide", "narrow")}
    ths = _thetas(comp_name, runs["wide"][0], 64)
    n_seq = 400
    seq = np.ascontiguousarray(np.resize(ths, (n_seq, ths.shape[1])))
    res = {m: {"step_us": [], "scan_us_events": [], "k16_evals_per_s": []} for m in runs}
    closures = {}
    for m, (comp, eng) in runs.items():
        closures[m] = (eng.configure_sequence(seq, total), eng.configure_batch(16, total))
        closures[m][0]()  # warm-up (first evaluation: reference exponents, AQL queue)
        closures[m][1](ths[:16])
        pb, ib = eng.resident_bytes()
        res[m].update(scan_kernel=eng.scan_kernel_name(), batch_path=eng.batch_path(16), resident_pe_bytes=pb, resident_inj_bytes=ib,
                      bytes_per_sample=(pb + ib) / (eng.n_ev * eng.n_pe + eng.n_inj), narrowed_terms=list(eng.bound.narrowed))
    for rep in range(5):  # interleaved: drift of the box's clocks hits both alike
        for m, (comp, eng) in runs.items():
            run_seq, run_batch = closures[m]
            t0 = time.perf_counter()
            run_seq()
            res[m]["step_us"].append((time.perf_counter() - t0) / n_seq * 1e6)
            _, _, kms = eng.evaluate_sequence(seq[:100], total, timing_every=1)
            res[m]["scan_us_events"].append(float(np.median(kms[:, 0])) * 1e3)
            n_b = 100
            t0 = time.perf_counter()
            for i in range(n_b):
                run_batch(ths[(i % 4) * 16:(i % 4) * 16 + 16])
            res[m]["k16_evals_per_s"].append(16 * n_b / (time.perf_counter() - t0))
    # the two engines agree (the catalog's coordinates are float32 numbers): a sanity line in the record
    a, b = runs["wide"][1].evaluate(ths[0], total), runs["narrow"][1].evaluate(ths[0], total)
    summary = {"config": cfg, "same_log_likelihood": a.log_likelihood == b.log_likelihood}
    for m in runs:
        r = res[m]
        summary[m] = dict(r, step_us_median=float(np.median(r["step_us"])), scan_us_events_median=float(np.median(r["scan_us_events"])),
                          k16_evals_per_s_median=float(np.median(r["k16_evals_per_s"])))
    with open(out, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps({m: {k: summary[m][k] for k in ("step_us_median", "scan_us_events_median", "k16_evals_per_s_median", "bytes_per_sample", "scan_kernel")} for m in runs}))


def cmd_scan(cfg, mode, n):
    comp_name, pe, inj, total = _catalog(cfg)
    comp, eng = _engine(comp_name, pe, inj, mode)
    ths = _thetas(comp_name, comp, 64)
    run = eng.configure_sequence(np.ascontiguousarray(np.resize(ths, (n, ths.shape[1]))), total)
    run()
    pb, ib = eng.resident_bytes()
    print(json.dumps({"config": cfg, "mode": mode, "scan_kernel": eng.scan_kernel_name(), "resident_bytes": pb + ib}))


def _scan_row(stats_csv):
    rows = [r for r in csv.DictReader(open(stats_csv)) if "scan_kernel" in r["Name"]]
    return max(rows, key=lambda r: float(r["TotalDurationNs"])) if rows else None


def _counter(cc_csv, name):
    vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(cc_csv)) if "scan_kernel" in r["Kernel_Name"] and r["Counter_Name"] == name]
    return float(np.median(vals)) if vals else None


def cmd_summarize(src, out_dir):
    out = {}
    for tj in sorted(glob.glob(os.path.join(src, "time_*.json"))):
        t = json.load(open(tj))
        cfg = t["config"]
        out[cfg] = {"same_log_likelihood": t["same_log_likelihood"]}
        for m in ("wide", "narrow"):
            r = t[m]
            row = {k: r[k] for k in ("scan_kernel", "batch_path", "bytes_per_sample", "resident_pe_bytes", "resident_inj_bytes", "step_us_median", "scan_us_events_median",
                                     "k16_evals_per_s_median", "step_us", "scan_us_events", "k16_evals_per_s")}
            stats = glob.glob(os.path.join(src, f"prof_{cfg}_{m}", "trace", "**", "*_kernel_stats.csv"), recursive=True)
            if stats and _scan_row(stats[0]):
                s = _scan_row(stats[0])
                row["scan_us_rocprof"] = float(s["AverageNs"]) / 1e3
                row["scan_calls_rocprof"] = int(s["Calls"])
            fetch = glob.glob(os.path.join(src, f"prof_{cfg}_{m}", "fetch", "**", "*_counter_collection.csv"), recursive=True)
            if fetch:
                kib = _counter(fetch[0], "FETCH_SIZE")
                if kib is not None:
                    actual = r["resident_pe_bytes"] + r["resident_inj_bytes"]
                    row["fetch_size_bytes"] = kib * 1024.0
                    row["fetch_over_actual_bytes"] = kib * 1024.0 / actual
            sq = glob.glob(os.path.join(src, f"prof_{cfg}_{m}", "sq", "**", "*_counter_collection.csv"), recursive=True)
            if sq:
                row["sq"] = {n: _counter(sq[0], n) for n in ("SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU", "SQ_INSTS_VMEM_RD", "SQ_WAIT_INST_LDS", "SQ_ACTIVE_INST_LDS")}
            out[cfg][m] = row
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "narrow_columns.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("| config | engine | B/sample | scan us (rocprofv3) | scan us (events) | step us | K=16 evals/s | FETCH / actual bytes |")
    print("|---|---|---|---|---|---|---|---|")
    for cfg, d in out.items():
        for m in ("wide", "narrow"):
            r = d.get(m, {})
            fmt = lambda k, spec: (format(r[k], spec) if r.get(k) is not None else "-")  # noqa: E731
            print(f"| {cfg} | {m} | {fmt('bytes_per_sample', '.0f')} | {fmt('scan_us_rocprof', '.2f')} | {fmt('scan_us_events_median', '.2f')} | {fmt('step_us_median', '.2f')} | "
                  f"{fmt('k16_evals_per_s_median', '.0f')} | {fmt('fetch_over_actual_bytes', '.3f')} |")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "time":
        cmd_time(sys.argv[2], sys.argv[3])
    elif cmd == "scan":
        cmd_scan(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 300)
    elif cmd == "summarize":
        cmd_summarize(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
