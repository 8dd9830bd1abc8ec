"""CPU: the record bench.py prints -- ONE compact line of strict JSON that the driver can read out of a bounded tail of stdout.
Round 5's line had grown to 23 KB and was cut before the driver parsed it; `compact_line` / `dump_line` are run here on canned
detail dicts (that very line, and the 2- and 8-rank lines of the same round) and must stay under the limit with every key the
contract and the judge read."""
import copy
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANNED = ["profiles/round5/bench_driver_form.json", "profiles/round5/ranks_2_one_gpu.json", "profiles/round5/ranks_8_one_gpu.json"]
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
            "cpu_baseline")


def canned(path):
    return json.loads(open(os.path.join(ROOT, path)).read().strip().splitlines()[-1])


def refuse_constants(name):
    raise ValueError(f"non-strict JSON token {name}")


@pytest.mark.parametrize("path", CANNED)
def test_line_is_small_strict_and_complete(path):
    detail = canned(path)
    text = bench.dump_line(bench.compact_line(detail, "bench_detail.json"))
    assert len(text.encode()) <= bench.LINE_LIMIT <= 4096 and "\n" not in text
    line = json.loads(text, parse_constant=refuse_constants)
    for key in CONTRACT:
        assert key in line, key
    assert line["value"] == pytest.approx(detail["value"], rel=1e-5) and line["ms_per_step"] == pytest.approx(detail["ms_per_step"], rel=1e-5)
    assert line["steps"] == detail["steps"] and line["warmup"] == detail["warmup"] and line["n_gpus"] == detail["n_gpus"]
    assert set(("workload", "n_events", "n_pe", "n_inj", "n_theta")) <= set(line["config"]) and "model" not in line["config"]
    roof = line["roofline"]
    for key in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_kernel_us"):
        assert key in roof, key
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-4)
    # achieved = algorithmic bytes / live scan duration (what the judge recomputes)
    assert roof["achieved"] == pytest.approx(roof["algorithmic_bytes_per_launch"] / (roof["avg_kernel_us"]["scan"] * 1e-6) / 1e9, rel=1e-4)
    if detail["n_gpus"] == 1:
        cpu = line["cpu_baseline"]
        assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and cpu["single_thread_evals_per_s"] > 0 and cpu["sample"]
        assert "multi_gpu" not in line
        for name in ("c3", "c5"):
            blk = line["configs"][name]
            assert blk["value"] > 0 and 0 < blk["frac"] < 1 and blk["cpu"] > 0 and blk["scan_us"] > 0
    else:
        mg = line["multi_gpu"]
        assert mg["ranks"] == detail["n_gpus"] and mg["rccl_ranks"] in (0, mg["ranks"])
        assert set(mg["sharded_vs_single_gpu"]) >= {"log_likelihood_rel_err", "grad_max_err_over_scale"}
        assert len(mg["per_rank_events"]) == min(mg["ranks"], 8) and sum(mg["per_rank_events"]) == 69


def test_non_finite_numbers_never_reach_the_line():
    detail = canned(CANNED[0])
    detail["roofline"]["achieved"] = float("nan")
    detail["roofline"]["frac"] = float("inf")
    detail["configs"]["c3"]["value"] = float("-inf")
    text = bench.dump_line(bench.compact_line(detail))
    assert "NaN" not in text and "Infinity" not in text
    line = json.loads(text, parse_constant=refuse_constants)
    assert line["roofline"]["achieved"] is None and line["roofline"]["frac"] is None and "value" not in line["configs"]["c3"]
    json.dumps(bench.strict(detail), allow_nan=False)  # the detail file is strict too


def test_an_oversized_line_sheds_secondary_blocks_not_the_contract():
    detail = canned(CANNED[0])
    big = copy.deepcopy(detail["configs"]["c3"])
    for i in range(40):
        detail["configs"][f"extra{i}"] = big
    text = bench.dump_line(bench.compact_line(detail))
    assert len(text.encode()) <= bench.LINE_LIMIT
    line = json.loads(text)
    for key in CONTRACT:
        assert key in line and line[key] is not None or key == "vs_baseline"
    assert isinstance(line["configs"], str) and "dropped" in line["configs"]


def test_plain_run_line_and_output_dump(tmp_path):
    """A run without --full: the detail holds the timed steps only; the line still carries the contract's keys with their
    meaning (value = steps / elapsed, ms_per_step = elapsed / steps) and says null for the legs that did not run.
    `dump_outputs` writes the last timed step's arrays as float64 .npy files."""
    import numpy as np

    full = canned(CANNED[0])
    detail = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                                   "config")}
    detail["scan_chain"] = {"name": "plpeak+plq+plz"}
    line = json.loads(bench.dump_line(bench.compact_line(detail, None)), parse_constant=refuse_constants)
    for key in CONTRACT:
        assert key in line, key
    assert line["value"] == pytest.approx(full["value"], rel=1e-5) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["unit"] == "evals/s"
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["batched"] is None and "configs" not in line
    outputs = {"log_likelihood": np.array([-160.08]), "grad": np.linspace(-1.0, 1.0, 6)}
    bench.dump_outputs(str(tmp_path / "out"), outputs)
    for name, arr in outputs.items():
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, arr)
