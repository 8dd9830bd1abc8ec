"""CPU: the high-precision term fixture (tests/golden/terms_hp.npz) and the C oracle against it.

The fixture holds, for every closed-form term of the reference, the normalised log-density of a short sample vector and its
derivative with respect to every hyper-parameter at ~40 hyper-points, computed with mpmath at 80 digits straight from the
reference's definitions (tests/golden/make_terms_hp.py).  Its hyper-points include the sweep 1 + alpha, 1 + beta = 0, +-2^-52,
+-1e-14 ... +-0.1 through the removable singularity of the power-law normaliser, where a closed form shared by the engine and
its oracle cancels: the oracle is held here to the engine's own bars (tests/terms_hp_util.py) so that it can referee there.

A second fixture (tests/golden/spline_terms_hp_*.npz, tests/golden/make_spline_terms_hp.py) does the same for the 1-D B-spline
models on the four bases -- every coefficient's derivative, from the Cox-de Boor recursion on the reference's own knot vector, not
from the closed-form taps the engine and the oracle share -- for the tabulated power-law redshift distribution, and for the two spline
redshift models (PowerlawSplineRedshiftModel: one grid normaliser over an exponent and a coefficient vector; BSplineRedshift: an
exponent block and a normaliser block, a spline domain inside the data range), whose catalogs pin the models' z grid to the
fixture's, and for BSplineDistribution.log_prob (a log-density tabulated on a grid that reaches beyond the basis domain, interpolated
linearly).  ``Shared`` reads one fixture term twice with one coefficient vector, as the IID spin models do."""
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
    assert {k: (v["model"], v["n"], v["xrange"], v["normalize"]) for k, v in gen.Z_META.items()} == U.Z_SPLINE_TERMS
    assert {k: (v["basis"], v["n"], tuple(v["xrange"]), tuple(v["grid"])) for k, v in gen.LERP_META.items()} == U.LERP_TERMS
    assert gen.names() == U.SPLINE_FIXTURE_TERMS
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


def test_redshift_spline_fixture_covers_what_it_is_for(spline_fixture):
    """The data ends exactly, the masked neighbour of zmax, the neighbours of each end of the spline domain, samples whose float64
    log is a knot's coordinate and one ulp either side, live samples and grid nodes outside the spline domain, lamb = 1 exactly, the
    hole and the scale-40 points; every file below 256 KiB."""
    zg, _, _ = U._z_table()
    zmin, zmax = zg[0], zg[-1]
    for name, (kind, n, xrange, normalize) in U.Z_SPLINE_TERMS.items():
        t = U.Term(spline_fixture, name)
        z = t.cols[0]
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"spline_terms_hp_{name}.npz")) < 256 * 1024
        assert t.columns == ["z", "dVcdz"] and 45 <= t.n <= 64 and 8 <= len(t.theta) <= 12 and np.all(z >= zmin)
        for v in (zmin, zmax, np.nextafter(zmin, np.inf), np.nextafter(zmax, -np.inf), np.nextafter(zmax, np.inf), 2.0):
            assert np.any(z == v), (name, v)
        lo, hi = np.log(xrange or (zmin, zmax))
        dx = np.diff(np.linspace(lo, hi, n - 2)[:2])[0]
        knots = np.linspace(lo - 3 * dx, hi + 3 * dx, n + 4)  # the reference's (interpolation.py:98-106)
        for k in ([lo, hi] if n == 4 else [lo, hi, knots[4], knots[n - 1]]):
            near = np.log(z)[np.abs(np.log(z) - k) <= 4 * np.spacing(abs(k))]
            # (lo and hi are logs of doubles and are met exactly; an interior knot only where some double's log is that number)
            assert (k in near or k not in (lo, hi)) and (np.any(near < k) or k == lo == np.log(zmin)) and (np.any(near > k) or k == hi == np.log(zmax)), (name, k)
        if kind == "PowerlawSplineRedshiftModel":
            assert t.params == ["lamb"] + [f"c{k}" for k in range(n)] and set(t.theta[:, 0]) == {-2.0, 0.0, 1.0, 2.7, 6.0}
            assert np.all(np.isneginf(t.logp[:, z > zmax])) and np.all(np.isfinite(t.logp[:, z <= zmax]))
            assert {"zeros/lamb1", "normal1/lamb1", "normal40/lamb-2", "hole-300/lamb0", "sawtooth10/lamb6", "shift+300/lamb1", "shift-300/lamb1"} <= set(t.tags)
            h0, hp = t.tags.index("normal1/lamb1"), t.tags.index("shift+300/lamb1")
            assert np.array_equal(t.theta[hp, 1:], t.theta[h0, 1:] + 300.0) and np.array_equal(t.logp[hp], t.logp[h0])
        else:
            assert np.all(np.isfinite(t.logp)) and t.theta.shape[1] == (2 * n if normalize else n)  # no sample is excluded
            for v in (xrange[0], xrange[1], np.nextafter(xrange[0], 0.0), np.nextafter(xrange[0], 1.0), np.nextafter(xrange[1], 0.0), np.nextafter(xrange[1], 9.0)):
                assert np.any(z == v), (name, v)
            outside = (z < xrange[0]) | (z > xrange[1])
            assert np.any(z < xrange[0]) and np.any((z > xrange[1]) & (z <= zmax)) and (not normalize or np.all(t.dlogp[:, :n][:, :, outside] == 0.0))
            assert np.any(zg < xrange[0]) and np.any(zg > xrange[1])  # live grid nodes outside the spline domain, on both sides
            assert {"normal40", "hole-300", "sawtooth10"} <= set(t.tags)


def test_lerp_fixture_covers_what_it_is_for(spline_fixture):
    """A sample on a node (f = 0) and one ulp either side, on grid[0] and grid[-1], outside the grid on both sides (live: the end values
    are held), one ulp below the end, on the last finite node next to a -inf one (live), inside the cell between them and on the
    -inf node (dead); a grid of at most 200 nodes that reaches beyond the basis domain; files below 256 KiB."""
    for name, (basis, n, (xmin, xmax), grid) in U.LERP_TERMS.items():
        t = U.Term(spline_fixture, name)
        g, x = spline_fixture[f"{name}/grid"], t.cols[0]
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"spline_terms_hp_{name}.npz")) < 256 * 1024
        assert np.array_equal(g, np.linspace(*grid)) and len(g) <= 200 and (g[0] < xmin or g[-1] > xmax) and 50 <= t.n <= 60 and 8 <= len(t.theta) <= 12
        on = np.flatnonzero(np.isin(x, g[1:-1]))
        assert len(on) >= 2 and all(np.any(x == np.nextafter(x[on[0]], s)) for s in (-np.inf, np.inf))
        for v in (g[0], g[-1], np.nextafter(g[-1], -np.inf)):
            assert np.any(x == v), (name, v)
        assert np.any(x < g[0]) and np.any(x > g[-1]) and {"zeros", "normal40", "sawtooth10", "hole-300"} <= set(t.tags)
        inside = (g >= xmin) & (g <= xmax)
        first, last = np.flatnonzero(inside)[[0, -1]]
        out_node = g[last + 1] if last + 1 < len(g) else g[first - 1]
        edge_node, (lo_c, hi_c) = (g[last], (g[last], g[last + 1])) if last + 1 < len(g) else (g[first], (g[first - 1], g[first]))
        between = (x > lo_c) & (x < hi_c)
        assert np.any(x == out_node) and np.any(x == edge_node) and np.any(between)
        if "LogY" in basis:
            assert np.all(np.isneginf(t.logp[:, (x == out_node) | between])) and np.all(np.isfinite(t.logp[:, x == edge_node]))
            held = (x > g[-1]) if inside[-1] else (x < g[0])  # beyond the end whose node is finite: that node's value is held
            assert np.any(held) and np.all(np.isfinite(t.logp[:, held]))
        else:
            assert np.all(np.isfinite(t.logp))  # a linear basis is 0 outside its domain: the log-density is 0 there, every sample is live
        assert np.all(np.isfinite(t.logp[:, (x > max(g[0], xmin)) & (x < min(g[-1], xmax))]))


@pytest.mark.parametrize("name", [k for k, v in U.Z_SPLINE_TERMS.items() if v[3]])
def test_host_scaling_of_the_exponent_coefficients(spline_fixture, name):
    """BSplineRedshift with normalize=True hands the engine e = c / (c . I), I_k the trapezoid integral of basis k over the basis's
    own grid: a theta-only matter of the host.  Held to I_k and e from the generator (e: the double nearest to the exact quotient);
    16 roundings of float64 over a sum conditioned to 1e-3 (the generator's CONDITION) stay below 1e-11 relative."""
    t = U.Term(spline_fixture, name)
    n = U.Z_SPLINE_TERMS[name][1]
    cat = U.catalog_a(t, OracleEvaluator)
    model = cat.models[0]
    ints = spline_fixture[f"{name}/I"]
    assert np.all(np.abs(model._basis_integrals - ints) <= 1e-14 * np.max(ints)), np.max(np.abs(model._basis_integrals - ints))
    for h, tag in enumerate(t.tags):
        e, c = t.theta[h, :n], t.theta[h, n:]
        got = model._exponent_coefs(c)
        assert np.all(np.abs(got - e) <= 1e-11 * np.max(np.abs(e))), (tag, np.max(np.abs(got - e)))
        layout = cat.ev.bound.theta_of(model(c, pe_samples=True))  # the drop-in call lays out (e, c)
        assert np.array_equal(layout[cat.slot[:n]], got) and np.array_equal(layout[cat.slot[n:]], c), tag


def test_cosmology_tables_are_checked_before_any_density(spline_fixture, monkeypatch):
    """Every catalog of a spline redshift model holds the model's z grid to the fixture's exactly and its dVc/dz tables to 1e-13
    relative (``check_tables``) when it is built; a table that is off, or a catalog that does not pin the range, is named."""
    from gwinferno_amd import cosmology as C

    t = U.Term(spline_fixture, "plzspline7")
    U.catalog_b(t, OracleEvaluator)  # passes as it stands
    idx = np.flatnonzero(t.cols[0] < 1.0)
    with pytest.raises(AssertionError, match="does not pin the redshift range"):
        U.Catalog(t, OracleEvaluator, idx.reshape(-1, 1), idx)
    cosmo = C.planck15_lvk()
    real = type(cosmo).dVc_dz
    monkeypatch.setattr(type(cosmo), "dVc_dz", lambda self, z: real(self, z) * (1.0 + 3e-13))
    with pytest.raises(AssertionError, match="dVc/dz on the z grid differs"):
        U.catalog_a(t, OracleEvaluator)


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


def shared_term(z, name):
    """``name`` read twice, the second time seven samples further on (samples near both domain ends meet interior ones)."""
    t = U.Term(z, name)
    return U.Shared(t, np.roll(np.arange(t.n), 7))


@pytest.mark.parametrize("name", ["logy7", "logy17"])
def test_c_oracle_with_one_coefficient_vector_read_by_two_terms(spline_fixture, name):
    """BSplineIIDSpinTilts on (-1, 1) with 7 coefficients, BSplineIIDSpinMagnitudes on (0, 1) with 17: two terms scatter into ONE
    block of gradient slots; the fixture's sum of the two parts, same bars."""
    term = shared_term(spline_fixture, name)
    worst, failures = U.Worst(), []
    cat = U.values_catalog(term, OracleEvaluator)
    assert cat.ev.bound.n_theta == len(term.params) and len(cat.ev.bound.terms) == 2
    U.check_values(cat, "oracle", worst, failures)
    U.check_gradients(U.catalog_a(term, OracleEvaluator), "oracle/A", worst, failures)
    U.check_gradients(U.catalog_b(term, OracleEvaluator), "oracle/B", worst, failures)
    print("\n".join(worst.lines()))
    U.report(failures, worst)


@pytest.mark.parametrize("name, fixture_name", [("logy17", "spline_fixture"), ("plpeak", "fixture"), ("plzspline7", "spline_fixture")])
def test_c_oracle_with_marginalised_selection(request, name, fixture_name):
    """``reference_marginalised`` (catalog B) is what the engine's squared-weight pass is held to on the GPU; the oracle first."""
    term = U.Term(request.getfixturevalue(fixture_name), name)
    worst, failures = U.Worst(), []
    U.check_gradients(U.catalog_b(term, OracleEvaluator), "oracle/B/marginalised", worst, failures, points=U.marginalised_points(term), marginalised=True)
    U.report(failures, worst)
