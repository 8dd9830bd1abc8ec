"""CPU: the launch planning of gwi_create (gwinferno_amd/csrc/gwi_plan.h: knobs -> launch geometries, gradient-row replicas)
compiled on its own with g++ and held to tests/golden/launch_plan_cases.json, integer for integer.  The table was recorded
from the engine's own code before the planning moved into the header (inputs -> both geometries, distinct, rep, scan_lds), so
it pins the summation order of every evaluation; the invariants of the tail kernels are asserted on top.  The second build
runs the same cases under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program; nothing is preloaded)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "launch_plan_cases.json")


def _chunk_packs(c):
    return c > 0 and (c < 32768 or (c % 256 == 0 and c // 256 < 32768))


@pytest.mark.parametrize("flags", ["", "-fsanitize=address,undefined -fno-sanitize-recover=all"])
def test_plan_matches_recorded_cases(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    with open(CASES) as f:
        doc = json.load(f)
    gcol = {name: i for i, name in enumerate(doc["geometry_columns"])}
    n_gin, n_lin = gcol["refused"], doc["lds_columns"].index("rep")
    exe = str(tmp_path / "plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", *flags.split(), "-I" + os.path.join(ROOT, "gwinferno_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "plan_driver.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    lines = ["G " + " ".join(map(str, r[: n_gin - 1])) + " " + " ".join(doc["geometry_knobs"][r[n_gin - 1]]) for r in doc["geometry"]]
    lines += ["L " + " ".join(map(str, r[: n_lin - 1])) + " " + " ".join(doc["lds_knobs"][r[n_lin - 1]]) for r in doc["lds"]]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GWI_") and k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr[-4000:]
    got = [[int(x) for x in ln.split()] for ln in run.stdout.splitlines()[:-1]]
    assert len(got) == len(lines)
    n_geo = len(doc["geometry"])
    assert n_geo >= 2000 and len(doc["lds"]) == 80
    for row, out in zip(doc["geometry"], got[:n_geo]):
        want = row[n_gin:]
        if want[0] == 1:  # refused before the batched geometry was derived: the single one and the refusal
            want, out = want[:8], out[:8]
        assert out == want, (row[:n_gin], doc["geometry_knobs"][row[n_gin - 1]], out, want)
        if want[0]:
            continue
        # what the tail kernels rely on: a group's tile records map to the lanes of one wave, tile sizes travel in 16 bits
        n_ev = row[gcol["n_ev"]]
        geos = [out[1:8]] + ([out[8:15]] if out[15] else [])
        for chunk_pe, chunk_inj, tiles_per_event, n_inj_tiles, n_scan_blocks, tiles_per_inj_group, n_inj_groups in geos:
            assert tiles_per_event <= 64 and tiles_per_inj_group <= 64 and n_inj_groups <= 64, row
            assert _chunk_packs(chunk_pe) and _chunk_packs(chunk_inj), row
            assert n_scan_blocks == n_ev * tiles_per_event + n_inj_tiles, row
            assert tiles_per_event * chunk_pe >= row[gcol["n_pe"]] and n_inj_tiles * chunk_inj >= row[gcol["n_inj"]], row
            assert n_inj_groups * tiles_per_inj_group >= n_inj_tiles, row
    for row, out in zip(doc["lds"], got[n_geo:]):
        assert out == row[n_lin:], (row, out)
