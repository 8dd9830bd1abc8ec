"""CPU: the high-precision term fixture (tests/golden/terms_hp.npz) and the C oracle against it.

The fixture holds, for every closed-form term of the reference, the normalised log-density of a short sample vector and its
derivative with respect to every hyper-parameter at ~40 hyper-points, computed with mpmath at 80 digits straight from the
reference's definitions (tests/golden/make_terms_hp.py).  Its hyper-points include the sweep 1 + alpha, 1 + beta = 0, +-2^-52,
+-1e-14 ... +-0.1 through the removable singularity of the power-law normaliser, where a closed form shared by the engine and
its oracle cancels: the oracle is held here to the engine's own bars (tests/terms_hp_util.py) so that it can referee there.

A second fixture (tests/golden/spline_terms_hp_*.npz, tests/golden/make_spline_terms_hp.py) does the same for the 1-D B-spline
models on the four bases -- every coefficient's derivative, from the Cox-de Boor recursion on the reference's own knot vector, not
from the closed-form taps the engine and the oracle share -- and for the tabulated power-law redshift distribution."""
import importlib.util
import os

import numpy as np
import pytest
import terms_hp_util as U
from golden_util import GOLDEN_DIR

TERMS = ["powerlaw", "plpeak", "plpeak_ratio", "ratio", "plpeak_smooth", "tilt", "tilt_joint", "beta", "truncnorm"]


@pytest.fixture(scope="module")
def fixture():
    return U.load()


@pytest.fixture(scope="module")
def spline_fixture():
    return U.load_spline()


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN_DIR, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_what_its_generator_writes(fixture):
    pytest.importorskip("mpmath")
    gen = _generator("make_terms_hp")
    fresh = gen.generate(verify=False)  # (the doubled-precision pass is the generator's own assertion when the fixture is written)
    assert sorted(fresh) == sorted(fixture.files)
    for k, v in fresh.items():
        got = fixture[k]
        assert got.dtype == v.dtype and got.shape == v.shape, k
        assert got.tobytes() == v.tobytes(), k  # bit for bit (-0.0 and NaN payloads included)


def test_fixture_covers_the_sweep(fixture):
    t = U.Term(fixture, "plpeak_ratio")
    b1 = 1.0 + t.theta[:, t.params.index("beta")]
    for e in (0.0, 2.0**-52, -(2.0**-52), 1e-10, -1e-10, 1e-6, -1e-6):
        assert np.any(b1 == (-1.0 + e) + 1.0), e
    assert fixture["plpeak/dlogp"].shape[1] == 4 and os.path.getsize(os.path.join(GOLDEN_DIR, "terms_hp.npz")) < 256 * 1024


def test_spline_fixture_is_what_its_generator_writes():
    pytest.importorskip("mpmath")
    gen = _generator("make_spline_terms_hp")
    assert {k: (v["basis"], v["n"], tuple(v["xrange"]), v["float32"]) for k, v in gen.META.items()} == U.SPLINE_TERMS
    fresh = gen.generate(verify=False)  # (the doubled-precision pass, the shift invariance and the conditioning of the linear splines
    # are the generator's own assertions; the last two run here too)
    assert sorted(fresh) == [os.path.basename(p) for p in U.spline_files()]
    for fn, arrays in fresh.items():
        path = os.path.join(GOLDEN_DIR, fn)
        assert os.path.getsize(path) < 256 * 1024, fn
        with np.load(path) as z:
            assert sorted(arrays) == sorted(z.files), fn
            for k, v in arrays.items():
                got = z[k]
                assert got.dtype == v.dtype and got.shape == v.shape, k
                assert got.tobytes() == v.tobytes(), k


def test_spline_fixture_covers_what_it_is_for(spline_fixture):
    """Domain ends and their neighbours, samples outside, the shifted, the hole and the scale-40 points, float32 sample vectors, and
    the exact cases of the redshift exponent."""
    for name, (basis, n, (xmin, xmax), f32) in U.SPLINE_TERMS.items():
        t = U.Term(spline_fixture, name)
        x = t.cols[0]
        assert t.theta.shape[1] == n == t.dlogp.shape[1] and t.n <= 64 and len(t.theta) <= 16
        for v in (xmin, xmax, np.nextafter(xmin, np.inf), np.nextafter(xmax, -np.inf)):
            assert f32 or np.any(x == v), (name, v)
        assert np.any(x == xmin) and np.any(x == xmax) and np.any(x < xmin) and np.any(x > xmax)
        assert np.all(np.isneginf(t.logp[:, (x < xmin) | (x > xmax)])) and np.all(np.isfinite(t.logp[:, (x == xmin) | (x == xmax)]).any(axis=0))
        assert f32 == bool(np.array_equal(x.astype(np.float32).astype(np.float64), x)), name
        if "LogY" in basis:
            assert {"zeros", "5e0", f"5e{n - 1}", "normal40", "sawtooth10", "shift+300", "shift-300", "hole-300"} <= set(t.tags)
            h0, hp, hm = (t.tags.index(k) for k in ("normal1", "shift+300", "shift-300"))
            assert np.array_equal(t.theta[hp], t.theta[h0] + 300.0) and np.array_equal(t.theta[hm], t.theta[h0] - 300.0)
            assert np.array_equal(t.logp[hp], t.logp[h0]) and np.array_equal(t.logp[hm], t.logp[h0])  # the density does not move
        else:
            assert "mixed" in t.tags and np.any(t.theta[t.tags.index("mixed")] < 0) and np.all(t.theta[t.tags.index("pos0.01")] > 0)
    z = U.Term(spline_fixture, "powerlaw_redshift")
    assert set(z.theta[:, 0]) == {-4.0, -1.0, 0.0, 1.0, 1.0 + 2.0**-52, 1.0 - 2.0**-52, 2.7, 8.0}


class OracleEvaluator:
    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import bind
        from oracle.c_oracle import COracle

        self.bound = bind(d_pe, d_inj)
        self.orc = COracle(self.bound)

    def log_weights(self, theta):
        assert self.bound.n_pe == 1  # one sample per event: log BF = log weight + the sample-independent constants
        with np.errstate(all="ignore"):
            return self.orc.evaluate(theta, 1.0, min_neff_cut=False)["logBFs"].reshape(-1, 1)

    def evaluate(self, theta, total_inj, marginalize_selection=False):
        r = self.orc.evaluate(theta, total_inj, min_neff_cut=False, marginalize_selection=marginalize_selection)
        return r["log_likelihood"], r["grad"]


@pytest.mark.parametrize("name", TERMS)
def test_c_oracle_against_the_fixture(fixture, name):
    """Same assertions, same bars as the engine's (tests/test_gpu_terms_hp.py): values 1e-11, every gradient component 1e-8 of
    max(1, |ref|), log_l 1e-9 relative."""
    term = U.Term(fixture, name)
    worst, failures = U.Worst(), []
    U.check_values(U.values_catalog(term, OracleEvaluator), "oracle", worst, failures)
    U.check_gradients(U.catalog_a(term, OracleEvaluator), "oracle/A", worst, failures)
    U.check_gradients(U.catalog_b(term, OracleEvaluator), "oracle/B", worst, failures)
    print("\n".join(worst.lines()))
    U.report(failures, worst)


@pytest.mark.parametrize("name", U.SPLINE_FIXTURE_TERMS)
def test_c_oracle_against_the_spline_fixture(spline_fixture, name):
    """The same three catalogs, assertions and bars for the spline terms and the tabulated redshift term: every coefficient's
    component within 1e-8 of max(1, |ref_j|)."""
    term = U.Term(spline_fixture, name)
    worst, failures = U.Worst(), []
    U.check_values(U.values_catalog(term, OracleEvaluator), "oracle", worst, failures)
    U.check_gradients(U.catalog_a(term, OracleEvaluator), "oracle/A", worst, failures)
    U.check_gradients(U.catalog_b(term, OracleEvaluator), "oracle/B", worst, failures)
    print("\n".join(worst.lines()))
    U.report(failures, worst)


@pytest.mark.parametrize("name, fixture_name", [("logy17", "spline_fixture"), ("plpeak", "fixture")])
def test_c_oracle_with_marginalised_selection(request, name, fixture_name):
    """``reference_marginalised`` (catalog B) is what the engine's squared-weight pass is held to on the GPU; the oracle first."""
    term = U.Term(request.getfixturevalue(fixture_name), name)
    worst, failures = U.Worst(), []
    U.check_gradients(U.catalog_b(term, OracleEvaluator), "oracle/B/marginalised", worst, failures, points=U.marginalised_points(term), marginalised=True)
    U.report(failures, worst)
