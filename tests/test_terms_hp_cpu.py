"""CPU: the high-precision term fixture (tests/golden/terms_hp.npz) and the C oracle against it.

The fixture holds, for every closed-form term of the reference, the normalised log-density of a short sample vector and its
derivative with respect to every hyper-parameter at ~40 hyper-points, computed with mpmath at 80 digits straight from the
reference's definitions (tests/golden/make_terms_hp.py).  Its hyper-points include the sweep 1 + alpha, 1 + beta = 0, +-2^-52,
+-1e-14 ... +-0.1 through the removable singularity of the power-law normaliser, where a closed form shared by the engine and
its oracle cancels: the oracle is held here to the engine's own bars (tests/terms_hp_util.py) so that it can referee there."""
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


def test_fixture_is_what_its_generator_writes(fixture):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_terms_hp", os.path.join(GOLDEN_DIR, "make_terms_hp.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
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

    def evaluate(self, theta, total_inj):
        r = self.orc.evaluate(theta, total_inj, min_neff_cut=False)
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
