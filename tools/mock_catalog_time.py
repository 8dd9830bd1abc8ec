"""Device times of the mock-catalog entries against their NumPy statement (diagnostic; writes profiles/mock_catalog/times.json).

    python tools/mock_catalog_time.py [--host]      # --host also times the statement (minutes at 10^7 sources)

Shapes: posterior samples at 69 events x 5000 samples x 7 coordinates; 10^7 observed injections at 3 coordinates.  Kernel times are
HIP events around the launches (gwi_mock_times); wall times include the host-to-device copies of a stand-alone entry."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gwinferno_amd import mock_catalog as MC  # noqa: E402


def timed(fn, repeats=3):
    best = np.inf
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    with_host = "--host" in sys.argv
    out = {}
    m7, m3 = MC.default_model(spins=True), MC.default_model()
    rng = np.random.default_rng(1)
    t_lo, t_hi, _ = m7.t_bounds()
    data = np.ascontiguousarray(t_lo[:, None] + (t_hi - t_lo)[:, None] * rng.uniform(0.1, 0.9, (7, 69)))
    MC.posterior_samples(data, m7, 5000, 1)  # (warm-up: module load)
    out["posteriors_69x5000x7"] = {"wall_s": timed(lambda: MC.posterior_samples(data, m7, 5000, 1)), "kernel_ms": MC.last_device_times()[1]}
    x = np.ascontiguousarray(m3.lo[:, None] + (m3.hi - m3.lo)[:, None] * rng.uniform(0.05, 0.95, (3, 10_000_000)))
    out["observe_1e7x3"] = {"wall_s": timed(lambda: MC.observe(x, m3, 2)), "kernel_ms": MC.last_device_times()[0], "launches": MC.last_device_times()[2]}
    if with_host:
        out["posteriors_69x5000x7"]["host_statement_s"] = timed(lambda: MC.posterior_samples(data, m7, 5000, 1, backend="host"), 1)
        out["observe_1e7x3"]["host_statement_s"] = timed(lambda: MC.observe(x, m3, 2, backend="host"), 1)
    path = os.path.join(ROOT, "profiles", "mock_catalog", "times.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
