"""CPU: a queue of chains (gwi_nuts_engine_queue) whose batched evaluation fails while chains are still queued -- what a peer
rank's failure looks like to the sharded queue (gwi_nuts_engine_queue_sharded) -- returns GWI_ERR_HIP instead of switching to
the never-started chains.  gwinferno_amd/csrc/gwi_sampler.cpp built on its own under AddressSanitizer +
UndefinedBehaviorSanitizer with tests/native/sampler_queue_failure_driver.cpp standing in for the engine."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_queue_with_a_failing_batch_begin_returns_an_error(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "sampler_queue_failure_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "gwinferno_amd", "csrc", "gwi_sampler.cpp"), os.path.join(ROOT, "tests", "native", "sampler_queue_failure_driver.cpp"), "-o", exe, "-lpthread"]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr[-4000:]
