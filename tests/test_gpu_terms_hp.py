"""GPU (-m gpu): term-level VALUES AND GRADIENTS of the engine against the high-precision fixture (tests/golden/terms_hp.npz,
mpmath at 80 digits from the reference's definitions; tests/golden/make_terms_hp.py), including the sweep of 1 + alpha and
1 + beta through 0 -- the removable singularity of the power-law normalisers, where the closed form the engine once shared with
its C oracle cancels and no oracle-based test could see it.

Bars (tests/terms_hp_util.py): |log w - ref| < 1e-11 and -inf exactly where the fixture has it; every gradient COMPONENT within
1e-8 max(1, |ref_j|); log_l within 1e-9.  The engine returns only the summed gradient, so the catalogs make the sum transparent
(ibid.: one sample per event and one injection; and events of 3 samples with 5 injections).

Paths: the ahead-of-time chains (config 2's plpeak+plq with PL+Peak as the absorbing term among them), the generic kernel, a chain
compiled at run time, and batched launches (one grid row per point, and scan_pbatch_kernel) that mix exact -1, +-1e-10, +-1e-6 and
ordinary exponents in one launch.  With GWI_TERMS_HP_REPORT=<file> the worst error per term and path is appended to that file
(profiles/near_singular/RESULTS.md keeps one such run)."""
import os

import numpy as np
import pytest
import terms_hp_util as U

pytestmark = pytest.mark.gpu

TERMS = ["powerlaw", "plpeak", "plpeak_ratio", "ratio", "plpeak_smooth", "tilt", "tilt_joint", "beta", "truncnorm"]


@pytest.fixture(scope="module")
def fixture():
    return U.load()


class EngineEvaluator:
    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import NativePopulationLikelihood

        self.eng = NativePopulationLikelihood(d_pe, d_inj)
        self.bound = self.eng.bound

    def log_weights(self, theta):
        return self.eng.log_weights(theta)[0]

    def evaluate(self, theta, total_inj):
        r = self.eng.evaluate(theta, total_inj, min_neff_cut=False)
        return r.log_likelihood, r.grad

    def close(self):
        self.eng.close()


def _finish(worst, failures):
    out = os.environ.get("GWI_TERMS_HP_REPORT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(worst.lines()) + "\n")
    U.report(failures, worst)


def _run(term, path, kernel_ok):
    worst, failures = U.Worst(), []
    for build, check in ((U.values_catalog, U.check_values), (U.catalog_a, U.check_gradients), (U.catalog_b, U.check_gradients)):
        cat = build(term, EngineEvaluator)
        name = cat.ev.eng.scan_kernel_name()
        assert kernel_ok(name), name
        check(cat, f"{path}/{build.__name__}", worst, failures)
        cat.close()
    _finish(worst, failures)


@pytest.mark.parametrize("name", TERMS)
def test_ahead_of_time_chains(fixture, name):
    _run(U.Term(fixture, name), "aot", lambda k: not k.startswith(("jit:", "generic")))


@pytest.mark.parametrize("name", ["plpeak_ratio", "plpeak_smooth"])
def test_generic_kernel(fixture, name, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    _run(U.Term(fixture, name), "generic", lambda k: k.startswith("generic"))


def test_chain_compiled_at_run_time(fixture, monkeypatch, tmp_path):
    """PL+Peak x PL q x truncated normal: a kind sequence without an ahead-of-time chain, so the engine compiles one (hipRTC) from
    the same headers; the reference is the sum of the two fixture terms."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    term = U.Product(U.Term(fixture, "plpeak_ratio"), U.Term(fixture, "truncnorm"))
    _run(term, "jit", lambda k: k.startswith("jit:"))


def _batch_points(term):
    want = ["beta-sweep+0", "beta-sweep+1e-10", "beta-sweep-1e-10", "beta-sweep+1e-06", "beta-sweep-1e-06", "beta-sweep+2.22e-16", "beta-sweep-2.22e-16", "alpha-sweep+0",
            "alpha-sweep-1e-10", "alpha-sweep-1e-06", "lam0.5"]
    pts = [term.tags.index(t) for t in want] + [h for h, t in enumerate(term.tags) if t == "ordinary"]
    assert len(pts) == 16, len(pts)
    return pts


@pytest.mark.parametrize("mode", ["rows-per-point", "pbatch"])
def test_batched_launch_mixing_exact_and_near_singular_points(fixture, mode, monkeypatch):
    """16 points in one launch: exact -1, +-2^-52, +-1e-10, +-1e-6 and ordinary exponents.  Every point is held to the fixture (same
    bars) and to its own single evaluation (1e-11 relative on the value, as tests/test_gpu_fuzz.py)."""
    if mode == "pbatch":
        monkeypatch.setenv("GWI_PBATCH", "1")
    term = U.Term(fixture, "plpeak_ratio")
    pts = _batch_points(term)
    worst, failures = U.Worst(), []
    for build in (U.catalog_a, U.catalog_b):
        cat = build(term, EngineEvaluator)
        eng = cat.ev.eng
        assert eng.batch_path(16) == mode, eng.batch_path(16)
        total = float(len(cat.inj_idx))
        batch = eng.evaluate_batch(np.stack([cat.theta(h) for h in pts]), total, min_neff_cut=False)
        U.check_gradients(cat, f"batch:{mode}/{build.__name__}", worst, failures, points=pts, results={h: (b.log_likelihood, b.grad) for h, b in zip(pts, batch)})
        for h, b in zip(pts, batch):
            one = eng.evaluate(cat.theta(h), total, min_neff_cut=False)
            if not abs(b.log_likelihood - one.log_likelihood) <= 1e-11 * abs(one.log_likelihood):
                failures.append(f"{term.tags[h]}: batched log_l {b.log_likelihood!r} vs single {one.log_likelihood!r}")
            e = U.grad_errors(term, b.grad, one.grad)
            if not np.all(e <= U.GRAD_RTOL):
                failures.append(f"{term.tags[h]}: batched gradient vs single evaluation: {e.max():.3e}")
        cat.close()
    _finish(worst, failures)


@pytest.mark.parametrize("name, param, tag", [("plpeak_ratio", "beta", "beta-sweep+0"), ("ratio", "beta", "sweep+0"), ("plpeak", "alpha", "sweep+0")])
def test_gradient_is_continuous_across_the_exact_point(fixture, name, param, tag):
    """Across 1 + exponent = -2^-52, 0, +2^-52 the engine's gradient moves by no more than the fixture's does, plus the bar."""
    term = U.Term(fixture, name)
    j = term.params.index(param)
    base = term.theta[term.tags.index(tag)]
    hs = []
    for e in (-(2.0**-52), 0.0, 2.0**-52):
        want = base.copy()
        want[j] = -1.0 + e
        hs.append(int(np.flatnonzero(np.all(term.theta == want, axis=1))[0]))
    failures = []
    for build in (U.catalog_a, U.catalog_b):
        cat = build(term, EngineEvaluator)
        total = float(len(cat.inj_idx))
        got = [np.asarray(cat.ev.evaluate(cat.theta(h), total)[1])[cat.slot] for h in hs]
        ref = [U.reference(cat, h)[1] for h in hs]
        for a, b in ((0, 1), (1, 2)):
            step, ref_step = np.abs(got[a] - got[b]), np.abs(ref[a] - ref[b])
            bar = U.GRAD_RTOL * np.maximum(1.0, np.abs(ref[b]))
            if not np.all(step <= ref_step + bar):
                failures.append(f"{name} {build.__name__}: gradient step {step.tolist()} across the exact point; the fixture's is {ref_step.tolist()}")
        cat.close()
    assert not failures, "\n".join(failures)
