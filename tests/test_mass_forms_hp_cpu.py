"""CPU: the third high-precision fixture (tests/golden/mass_forms_hp.npz, mpmath at 80 digits; tests/golden/make_mass_forms_hp.py) and
the two host-side oracles against it, with the bars the engine faces in tests/test_gpu_mass_forms_hp.py -- so that the bars are known
to be attainable in float64 before a device is asked.

  plbounds                 Powerlaw.log_prob with SAMPLED minimum / maximum (GWI_TERM_POWERLAW_BOUNDS): a support that moves with theta,
                           intervals down to hi / lo - 1 = 1e-6, the reference's -log(hi / lo) at alpha == -1.0 exactly.
  pairing_iid / _indep     beta log(m2 / m1) of the component-mass models (GWI_TERM_POWERLAW, GWI_POWERLAW_UNNORMALISED), joined with the two
                           m1 / m2 splines that share one coefficient vector; q > 1 masked in the first, alive in the second.
  ratio_on_logxlogy20_*    powerlaw_pdf(q, beta, mmin / m1, 1) next to the m1 spline (BSplinePrimaryPowerlawRatio), where the binder folds
                           log m1 into the spline's column; bars conditioned on d log p / d log m1 (tests/terms_hp_util.py).

The C oracle is held to values, gradients and log_l; the NumPy evaluation of a bound model (tests/bound_eval.py, values only) to the
values."""
import importlib.util
import os

import numpy as np
import pytest
import terms_hp_util as U
from golden_util import GOLDEN_DIR


@pytest.fixture(scope="module")
def fixture():
    return U.load_mass_forms()


@pytest.fixture(scope="module")
def spline_fixture():
    return U.load_spline()


def _generator():
    spec = importlib.util.spec_from_file_location("make_mass_forms_hp", os.path.join(GOLDEN_DIR, "make_mass_forms_hp.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_what_its_generator_writes(fixture):
    pytest.importorskip("mpmath")
    gen = _generator()
    assert gen.TERM_NAMES == U.MASS_FORM_TERMS and {f"ratio_on_logxlogy20_{k}": v for k, v in gen.RATIO_MMINS} == U.RATIO_MMIN
    assert (gen.EPS_LM_OWN, gen.EPS_LM_FOLD, gen.COND_CAP) == (U.EPS_LM_OWN, U.EPS_LM_FOLD, U.COND_CAP) and gen.MAX_WAIVED == 2
    assert gen.SPLINE_RANGE == U.SPLINE_TERMS["logxlogy20"][2]
    fresh = gen.generate(verify=False)  # (the doubled-precision pass and the cap on waived samples are the generator's own assertions)
    assert sorted(fresh) == sorted(fixture)
    for k, v in fresh.items():
        got = fixture[k]
        assert got.dtype == np.asarray(v).dtype and got.shape == np.asarray(v).shape, k
        assert got.tobytes() == np.asarray(v).tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "mass_forms_hp.npz")) < 128 * 1024


def test_fixture_covers_what_it_is_for(fixture, spline_fixture):
    t = U.Term(fixture, "plbounds")
    x, (alpha, lo, hi) = t.cols[0], t.theta.T
    assert t.params == ["alpha", "lo", "hi"] and not np.any(alpha == 0.0)
    for b in np.unique(np.concatenate([lo, hi])):  # every bound and both neighbours
        assert all(np.any(x == v) for v in (b, np.nextafter(b, np.inf), np.nextafter(b, -np.inf))), b
    assert np.intersect1d(lo, hi).size >= 1  # one value is lo of one point and hi of another
    for w in (1e-1, 1e-3, 1e-6):
        narrow = np.abs(hi / lo - 1.0 - w) < 1e-3 * w
        assert {-1.0, -1.0 + 1e-6, -1.0 - 1e-6, -2.5} <= set(alpha[narrow]), w
    assert len({(a, b) for a, b in zip(lo[alpha == -1.0], hi[alpha == -1.0])}) >= 5
    for e in (0.0, 2.0**-52, -(2.0**-52), 1e-10, -1e-10, 1e-6, -1e-6):
        assert np.any((alpha == -1.0 + e) & (lo == 5.0) & (hi == 100.0)), e
    live = np.isfinite(t.logp)
    assert np.all(live == ((x >= lo[:, None]) & (x <= hi[:, None])))
    same_alpha = [(a, b) for a in range(len(alpha)) for b in range(a) if alpha[a] == alpha[b] and (lo[a] == lo[b]) != (hi[a] == hi[b])]
    assert sum(np.any(live[a] != live[b]) for a, b in same_alpha) >= 5  # a sample changes sides between points that differ in one bound
    h = t.tags.index("sweep+0")  # the reference's own expression at alpha == -1.0
    on = live[h]
    assert np.allclose(t.logp[h][on], -np.log(x[on]) - np.log(100.0 / 5.0), rtol=0, atol=1e-14)
    for name, masked in (("pairing_iid", True), ("pairing_indep", False)):
        p = U.Term(fixture, name)
        s = U.Term(spline_fixture, "logxlogy17")
        perm = fixture["pairing/perm"]
        assert np.array_equal(p.cols[0], s.cols[0]) and np.array_equal(p.cols[1], s.cols[0][perm]) and not np.any(p.cols[1] == 0.0)
        q = p.cols[1] / p.cols[0]
        assert np.sum(q < 1) >= p.n / 3 and np.sum(q > 1) >= p.n / 5 and np.sum(q == 1) >= 3 and np.any(q == 1.0 + 2.0**-52)
        assert [float(b) for b in p.theta[:, 0]] == [1.0, -1.0, 2.5, -3.5, 12.0, -8.0, 1e-12, 0.0]
        assert np.all(np.isneginf(p.logp[:, q > 1])) if masked else np.all(np.isfinite(p.logp))
        assert np.all(p.logp[p.tags.index("beta0")][q <= 1] == 0.0)
    for name, mmin in U.RATIO_MMIN.items():
        r = U.RatioTerm(fixture, name)
        s = U.Term(spline_fixture, "logxlogy20")
        m1, q = r.cols
        assert np.array_equal(m1, s.cols[0]) and r.mmin == mmin and r.theta.shape == (30, 1)
        low = mmin / m1
        assert np.any(q == low) and np.any(q == 1.0) and np.any(q == np.nextafter(low, 1.0)) and np.any(q == np.nextafter(low, 0.0)) and np.any(q == np.nextafter(1.0, 2.0))
        assert not np.isfinite(r.logp[:, m1 == mmin]).any()
        waived = (np.abs(r.cond) * U.EPS_LM_FOLD > U.COND_CAP).any(axis=0)
        assert waived.sum() == (1 if mmin == 3.0 else 0) and np.all(m1[waived] == np.nextafter(3.0, 4.0))
        if mmin == 5.0:  # live for the spline, excluded by the ratio
            assert np.sum(np.isfinite(s.logp[0]) & (m1 < mmin)) >= 5 and not np.isfinite(r.logp[:, m1 < mmin]).any()


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


class NumpyEvaluator:
    """tests/bound_eval.py: the flat description of the bound model evaluated in NumPy (values only)."""

    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import bind

        self.bound = bind(d_pe, d_inj)

    def log_weights(self, theta):
        import bound_eval

        return bound_eval.log_weights(self.bound, theta)[0].reshape(self.bound.n_ev, self.bound.n_pe)


def _run(term, make, path, groups=None, eps_lm=None, gradients=True):
    worst, failures = U.Worst(), []
    cat = U.values_catalog(term, make)
    U.check_values(cat, path, worst, failures, eps_lm=eps_lm)
    for points in (groups or [None]) if gradients else []:
        for build in (U.catalog_a, U.catalog_b):
            U.check_gradients(build(term, make, points), f"{path}/{build.__name__}", worst, failures, points=points, eps_lm=eps_lm)
    print("\n".join(worst.lines()))
    U.report(failures, worst)
    return cat


def test_c_oracle_plbounds(fixture):
    term = U.Term(fixture, "plbounds")
    _run(term, OracleEvaluator, "oracle", groups=[U.group_points(term, fixture, g) for g in (0, 1)])


def test_c_oracle_plbounds_product(fixture, spline_fixture):
    term = U.plbounds_product(fixture, spline_fixture)
    _run(term, OracleEvaluator, "oracle", groups=[U.group_points(term, fixture, 0)])


def test_c_oracle_plbounds_times_truncnorm(fixture):
    term = U.Product(U.plbounds_arranged(fixture, 32), U.Term(U.load(), "truncnorm"))
    _run(term, OracleEvaluator, "oracle", groups=[U.group_points(term, fixture, 0)])


@pytest.mark.parametrize("name", ["pairing_iid", "pairing_indep"])
def test_c_oracle_pairing(fixture, spline_fixture, name):
    """Through the component-mass model (two splines on one coefficient vector and the pairing factor), and the factor alone."""
    s = U.Term(spline_fixture, "logxlogy17")
    term = U.Joint(U.Shared(s, fixture["pairing/perm"]), U.Term(fixture, name))
    cat = _run(term, OracleEvaluator, "oracle")
    assert len(cat.ev.bound.terms) == 3 and cat.ev.bound.n_theta == 18
    _run(U.Term(fixture, name), OracleEvaluator, "oracle", gradients=False)


@pytest.mark.parametrize("name", list(U.RATIO_MMIN))
@pytest.mark.parametrize("fold", [True, False])
def test_c_oracle_ratio_next_to_the_m1_spline(fixture, spline_fixture, name, fold, monkeypatch):
    """The oracle is handed the host's columns, which hold log m1 itself under either binding: the bar of the own column."""
    from gwinferno_amd import _native as N

    if not fold:
        monkeypatch.setenv("GWI_FOLD_LOGM", "0")
    term = U.Joint(U.Term(spline_fixture, "logxlogy20"), U.RatioTerm(fixture, name))
    cat = _run(term, OracleEvaluator, "oracle:fold" if fold else "oracle:own", eps_lm=U.EPS_LM_OWN)
    ratio = [t for t in cat.ev.bound.terms if t["kind"] == N.TERM_POWERLAW_RATIO][0]
    assert bool(ratio["flags"] & N.RATIO_LOGM_FROM_SPLINE) == fold and len(cat.ev.bound.pe_exprs) == (3 if fold else 4)


def test_c_oracle_keeps_the_sample_one_ulp_above_mmin_alive(fixture, spline_fixture):
    """m1 = nextafter(3.0, +inf) with mmin = 3.0: fl(mmin / m1) = 1 - 2^-53 < 1, so the reference's density is finite (~1e16) and the
    fixture has the sample alive.  float64 log(m1) rounds to log(3.0), so the term's log(mmin / m1) is 0: the oracle (like the engine,
    which works from the same logarithm) once took that for m1 == mmin and excluded the sample at all 30 hyper-points.  m1 == mmin is
    now excluded by the model's mask, on the quotient, and a live sample with log(mmin / m1) == 0 is evaluated at r = 1 - 2^-53."""
    failures = []
    U.check_waived_liveness(U.values_catalog(U.Joint(U.Term(spline_fixture, "logxlogy20"), U.RatioTerm(fixture, "ratio_on_logxlogy20_mmin3")), OracleEvaluator), failures)
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:8])


def test_numpy_oracle_values(fixture, spline_fixture):
    worst, failures = U.Worst(), []
    U.check_values(U.values_catalog(U.Term(fixture, "plbounds"), NumpyEvaluator), "numpy", worst, failures)
    s17, s20 = U.Term(spline_fixture, "logxlogy17"), U.Term(spline_fixture, "logxlogy20")
    for name in ("pairing_iid", "pairing_indep"):
        U.check_values(U.values_catalog(U.Joint(U.Shared(s17, fixture["pairing/perm"]), U.Term(fixture, name)), NumpyEvaluator), "numpy", worst, failures)
    for name in U.RATIO_MMIN:
        U.check_values(U.values_catalog(U.Joint(s20, U.RatioTerm(fixture, name)), NumpyEvaluator), "numpy", worst, failures, eps_lm=U.EPS_LM_OWN)
    print("\n".join(worst.lines()))
    U.report(failures, worst)


def test_joint_refuses_disjoint_terms(fixture, spline_fixture):
    with pytest.raises(AssertionError, match="Product"):
        U.Joint(U.Term(spline_fixture, "logxlogy17"), U.Subset(U.Term(spline_fixture, "logy17"), np.arange(39), "other"))
