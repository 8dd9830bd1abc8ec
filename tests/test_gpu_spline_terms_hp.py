"""GPU (-m gpu): VALUES AND EVERY COEFFICIENT'S GRADIENT COMPONENT of the spline terms against the second high-precision fixture
(tests/golden/spline_terms_hp_*.npz: mpmath at 80 digits, Cox-de Boor recursion on the reference's own knot vector, analytic
derivatives; tests/golden/make_spline_terms_hp.py) -- not against the C oracle, which shares the closed-form taps, the ``x == hi``
convention and the grid normaliser with the engine -- and the tabulated power-law redshift distribution with them.

Bars (tests/terms_hp_util.py, unchanged): |log w - ref| < 1e-11 and -inf exactly where the fixture has it; every gradient COMPONENT
within 1e-8 max(1, |ref_j|); log_l within 1e-9.  Catalogs as in tests/test_gpu_terms_hp.py: one sample per event and one injection
(A), events of 3 samples with 5 injections (B).

Every test asserts the path it means to take (``scan_kernel_name()``, ``batch_path()``, the narrowed columns): the scan chain the
engine picks, the generic kernel, a chain compiled at run time for a product of two spline terms, the 4-tap batched kernel (K = 4, and
K = 16 on float32 columns), the matrix-core GEMM on full and ragged groups (K = 16, 17) and its rows variant, float32 coordinate
columns, replay mode, and the squared-weight pass of the marginalised selection.

The two spline redshift models (PowerlawSplineRedshiftModel: "plzspline*", BSplineRedshift: "zspline*") ride the same tests on
catalogs that pin the models' z grid to the fixture's (tests/terms_hp_util.pins; the dVc/dz tables are checked when a catalog is
built), the "lerp_*" terms are BSplineDistribution.log_prob (GWI_TERM_EXP_SPLINE_LERP) on grids that reach beyond the basis domain, and
``Shared`` holds the IID pair models, two terms scattering into one block of gradient slots.

The matrix-core kernel runs on the product redshift x LogY (17) x LogY (16), not on a one-term model.  For a model of ONE spline term
there is no ahead-of-time instantiation (gwi_engine.hip, kMfmaVariants: all carry the redshift term), and the one hipRTC makes under
GWI_BATCH_MFMA=1 spills 24 bytes per lane to scratch, which the engine refuses by rule (try_jit_mfma: "the instantiation spills
registers to scratch"): such a model keeps the 4-tap kernel, and GWI_BATCH_ROWS=1 needs an ahead-of-time variant in any case.  The
product matches the ahead-of-time "plz+spline2 (32,16)": its 17 coefficients fill one gradient tile and put one coefficient in a
second, its 16 fill exactly one, and every one of the 34 components faces the bar.  With GWI_TERMS_HP_REPORT=<file> the worst error per term, path and quantity is appended to that file
(profiles/spline_terms_hp/RESULTS.md keeps one such run)."""
import os

import numpy as np
import pytest
import terms_hp_util as U

pytestmark = pytest.mark.gpu

EXP_MIX = ["shift+300", "normal40", "hole-300", "zeros", "shift-300", "normal1", "normal10", "sawtooth10", "5e0"]  # the first four: one K = 4 launch
LINEAR_MIX = ["pos0.01", "pos10", "wide", "mixed", "ones", "pos0.1", "pos1"]


@pytest.fixture(scope="module")
def fixture():
    return U.load_spline()


@pytest.fixture(scope="module")
def parametric_fixture():
    return U.load()


class EngineEvaluator:
    narrow_columns = False

    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import NativePopulationLikelihood

        self.eng = NativePopulationLikelihood(d_pe, d_inj, narrow_columns=self.narrow_columns)
        self.bound = self.eng.bound

    def log_weights(self, theta):
        return self.eng.log_weights(theta)[0]

    def evaluate(self, theta, total_inj, marginalize_selection=False):
        r = self.eng.evaluate(theta, total_inj, min_neff_cut=False, marginalize_selection=marginalize_selection)
        return r.log_likelihood, r.grad

    def close(self):
        self.eng.close()


class NarrowEvaluator(EngineEvaluator):
    narrow_columns = "auto"


def _finish(worst, failures):
    out = os.environ.get("GWI_TERMS_HP_REPORT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(worst.lines()) + "\n")
    U.report(failures, worst)


def _run(term, path, kernel_ok, make=EngineEvaluator, engine_ok=None, repeat=False):
    """Values on the values catalog, gradients on A and B; ``repeat``: a second evaluation must give the same bits."""
    worst, failures = U.Worst(), []
    for build, check in ((U.values_catalog, U.check_values), (U.catalog_a, U.check_gradients), (U.catalog_b, U.check_gradients)):
        cat = build(term, make)
        name = cat.ev.eng.scan_kernel_name()
        assert kernel_ok(name), name
        if engine_ok:
            engine_ok(cat.ev.eng)
        check(cat, f"{path}/{build.__name__}", worst, failures)
        if repeat and check is U.check_gradients:
            total = float(len(cat.inj_idx))
            for h in range(len(term.theta)):
                (l1, g1), (l2, g2) = cat.ev.evaluate(cat.theta(h), total), cat.ev.evaluate(cat.theta(h), total)
                if not (l1 == l2 and np.array_equal(g1, g2)):
                    failures.append(f"{term.name} [{path}] {term.tags[h]}: a second evaluation differs")
        cat.close()
    _finish(worst, failures)


def _compiled_chain(k):
    return not k.startswith("generic")  # ahead of time, or "jit:..." where the kind sequence has no chain of its own


@pytest.mark.parametrize("name", U.SPLINE_FIXTURE_TERMS)
def test_single_evaluations_through_the_chain_the_engine_picks(fixture, name, monkeypatch, tmp_path):
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    _run(U.Term(fixture, name), "chain", _compiled_chain)


@pytest.mark.parametrize("name", ["logy7", "logy17"])
def test_one_coefficient_vector_read_by_two_terms(fixture, name, monkeypatch, tmp_path):
    """BSplineIIDSpinTilts (7 coefficients on (-1, 1)) and BSplineIIDSpinMagnitudes (17 on (0, 1)): both terms add into the same slots."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    t = U.Term(fixture, name)
    term = U.Shared(t, np.roll(np.arange(t.n), 7))
    _run(term, "chain", _compiled_chain, engine_ok=lambda e: len(e.bound.terms) == 2 and e.bound.n_theta == len(term.params) or pytest.fail("not one shared block"))


@pytest.mark.parametrize("name", ["logy17", "bspline7", "plzspline7", "zspline16", "lerp_logy7"])
def test_generic_kernel(fixture, name, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    _run(U.Term(fixture, name), "generic", lambda k: k.startswith("generic"))


def test_product_of_two_spline_terms_compiled_at_run_time(fixture, monkeypatch, tmp_path):
    """LogXLogY mass x LogY spin on disjoint columns.  Two exponentiated splines have an ahead-of-time chain ("spline2"), so
    GWI_FORCE_JIT=1 has hipRTC compile the chain from the same headers instead."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_FORCE_JIT", "1")
    term = U.Product(U.Term(fixture, "logxlogy17"), U.Term(fixture, "logy7"))
    _run(term, "jit", lambda k: k.startswith("jit:"))


def test_redshift_spline_times_spin_spline_compiled_at_run_time(fixture, monkeypatch, tmp_path):
    """PowerlawSplineRedshiftModel (17) x LogY (7): the normaliser over (lamb, c) next to a grid normaliser of the plain kind."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_FORCE_JIT", "1")
    term = U.Product(U.Term(fixture, "plzspline17"), U.Term(fixture, "logy7"))
    _run(term, "jit", lambda k: k.startswith("jit:"))


def _batch(term, mix, K, path, make, worst, failures, engine_ok=None, repeatable=False):
    """K points (``mix``, repeated to reach K) in one launch on catalogs A and B: every requested point against the fixture and against
    its own single evaluation (1e-11 relative on the value, the gradient bar per component)."""
    pts = [t if isinstance(t, int) else term.tags.index(t) for t in mix]
    pts = [pts[k % len(pts)] for k in range(K)]
    for build in (U.catalog_a, U.catalog_b):
        cat = build(term, make)
        eng = cat.ev.eng
        assert eng.batch_path(K) == path, (eng.batch_path(K), path)
        if engine_ok:
            engine_ok(eng)
        total = float(len(cat.inj_idx))
        thetas = np.stack([cat.theta(h) for h in pts])
        batch = eng.evaluate_batch(thetas, total, min_neff_cut=False)
        again = eng.evaluate_batch(thetas, total, min_neff_cut=False) if repeatable else batch
        singles = {}
        for k, (h, b) in enumerate(zip(pts, batch)):
            where = f"batch:{path}:K{K}/{build.__name__}"
            U.check_gradients(cat, where, worst, failures, points=[h], results={h: (b.log_likelihood, b.grad)})
            if h not in singles:
                singles[h] = eng.evaluate(cat.theta(h), total, min_neff_cut=False)
            one = singles[h]
            # (a flat density: log_l is the rounding of sums that cancel -- relative to those, as the bar against the fixture is)
            size = max(abs(one.log_likelihood), U.reference(cat, h)[2], 1.0) if U.is_cancelled(term, h, cat) else abs(one.log_likelihood)
            if not abs(b.log_likelihood - one.log_likelihood) <= 1e-11 * size:
                failures.append(f"{term.name} [{where}] {term.tags[h]} (slot {k}): batched log_l {b.log_likelihood!r} vs single {one.log_likelihood!r}")
            e = U.grad_errors(term, b.grad, one.grad)
            if not np.all(e <= U.GRAD_RTOL):
                failures.append(f"{term.name} [{where}] {term.tags[h]} (slot {k}): batched gradient vs single evaluation: {e.max():.3e}")
            if not (b.log_likelihood == again[k].log_likelihood and np.array_equal(b.grad, again[k].grad)):
                failures.append(f"{term.name} [{where}] {term.tags[h]} (slot {k}): a second launch differs")
        cat.close()


@pytest.mark.parametrize("name", ["logy16", "logy17", "logxlogy17", "bspline7", "logx17"])
def test_batch_of_4_on_the_4_tap_kernel(fixture, name):
    term = U.Term(fixture, name)
    worst, failures = U.Worst(), []
    _batch(term, (LINEAR_MIX if name in ("bspline7", "logx17") else EXP_MIX)[:4], 4, "taps", EngineEvaluator, worst, failures)
    _finish(worst, failures)


def test_batch_of_4_mixes_the_exact_exponent_the_hole_and_the_scale_40_point(fixture):
    """lamb = 1 (lamb - 1 = 0 exactly), hole-300 and normal40 in ONE launch of the 4-tap kernel."""
    worst, failures = U.Worst(), []
    _batch(U.Term(fixture, "plzspline17"), ["normal1/lamb1", "hole-300/lamb0", "normal40/lamb-2", "zeros/lamb1"], 4, "taps", EngineEvaluator, worst, failures)
    _batch(U.Term(fixture, "zspline17"), ["ones", "hole-300", "normal40", "sawtooth10"], 4, "taps", EngineEvaluator, worst, failures)
    _finish(worst, failures)


@pytest.mark.parametrize("K", [16, 17])
def test_batches_of_the_redshift_spline_product_without_the_rows_variant(fixture, K, monkeypatch, tmp_path):
    """PowerlawSplineRedshiftModel (17) x LogY (17) x LogY (16) on whichever batched kernel the engine reports when asked for the
    matrix cores: that kernel, or the 4-tap one with the reason named.  THE ROWS VARIANT IS NOT COVERED for this product: it exists
    for ahead-of-time instantiations only (tests/test_gpu_spline_terms_hp.py's matrix-core product has one), this kind sequence has
    none, and a matrix-core kernel compiled at run time has no rows form -- under GWI_BATCH_ROWS=1 the engine reports the 4-tap
    kernel, which ``test_batch_of_4...`` and the K = 16 float32 test already run."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_MAX_BATCH", "24")
    monkeypatch.setenv("GWI_BATCH_MFMA", "1")
    term = U.Product(U.Term(fixture, "plzspline17"), U.Term(fixture, "logy17"), U.Term(fixture, "logy16"))
    probe = U.catalog_a(term, EngineEvaluator)
    path, note = probe.ev.eng.batch_path(K), probe.ev.eng.batch_calibration()["matrix_core_kernel"]
    probe.close()
    assert path == "mfma" or (path == "taps" and note != ""), (path, note)
    worst, failures = U.Worst(), []
    _batch(term, range(len(term.theta)), K, path, EngineEvaluator, worst, failures, repeatable=True)
    _finish(worst, failures)


def _matrix_core_term(fixture):
    """(redshift x LogY 17 x LogY 16, its hyper-points whose spline parts are EXP_MIX): the +-300 shifts, the scale-40 vector, the hole
    and zeros share one launch, each with one of the redshift exponents."""
    term = U.Product(U.Term(fixture, "powerlaw_redshift"), U.Term(fixture, "logy17"), U.Term(fixture, "logy16"))
    tags = term.parts[1].tags
    assert len(term.theta) == len(tags) and all(term.parts[2].tags.index(t) == tags.index(t) for t in EXP_MIX)
    return term, [tags.index(t) for t in EXP_MIX]


@pytest.mark.parametrize("K", [16, 17])
def test_batches_on_the_matrix_cores(fixture, K, monkeypatch):
    """K = 16: one full group of points; K = 17: a ragged second group.  The results repeat bit for bit on a second launch."""
    monkeypatch.setenv("GWI_MAX_BATCH", "24")
    monkeypatch.setenv("GWI_BATCH_MFMA", "1")
    term, pts = _matrix_core_term(fixture)
    worst, failures = U.Worst(), []
    _batch(term, pts, K, "mfma", EngineEvaluator, worst, failures, engine_ok=lambda e: e.batch_path(4) == "taps" or pytest.fail("K = 4 off the 4-tap kernel"), repeatable=True)
    _finish(worst, failures)


def test_batch_of_16_on_the_rows_variant(fixture, monkeypatch):
    monkeypatch.setenv("GWI_MAX_BATCH", "24")
    monkeypatch.setenv("GWI_BATCH_ROWS", "1")
    term, pts = _matrix_core_term(fixture)
    worst, failures = U.Worst(), []
    _batch(term, pts, 16, "rows", EngineEvaluator, worst, failures)
    _finish(worst, failures)


def test_one_term_model_keeps_the_4_tap_kernel_and_says_why(fixture, monkeypatch, tmp_path):
    """Asked for the matrix cores, a model of one spline term either gets a run-time instantiation or names the reason it did not
    (today: register spills): never a silent third thing.  Held to the fixture on whichever of the two it reports."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_MAX_BATCH", "24")
    monkeypatch.setenv("GWI_BATCH_MFMA", "1")
    term = U.Term(fixture, "logy17")
    probe = U.catalog_a(term, EngineEvaluator)
    path, note = probe.ev.eng.batch_path(16), probe.ev.eng.batch_calibration()["matrix_core_kernel"]
    probe.close()
    assert (path == "mfma" and note.startswith("compiled jit-mfma:")) or (path == "taps" and note != ""), (path, note)
    worst, failures = U.Worst(), []
    _batch(term, EXP_MIX, 16, path, EngineEvaluator, worst, failures)
    _finish(worst, failures)


def _narrowed(eng):
    assert len(eng.bound.narrowed) == 1, eng.bound.narrowed


@pytest.mark.parametrize("name", ["logy7_f32", "bspline7_f32"])
def test_float32_columns(fixture, name, monkeypatch, tmp_path):
    """Sample vectors of float32 numbers: ``narrow_columns="auto"`` stores the coordinate at 4 bytes; same fixture, same bars."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_MAX_BATCH", "24")
    term = U.Term(fixture, name)
    assert U.SPLINE_TERMS[name][3]
    _run(term, "narrow", _compiled_chain, make=NarrowEvaluator, engine_ok=_narrowed)
    worst, failures = U.Worst(), []
    probe = U.catalog_a(term, NarrowEvaluator)
    path = probe.ev.eng.batch_path(16)
    probe.close()
    assert path == "taps", path
    _batch(term, EXP_MIX if name.startswith("logy") else LINEAR_MIX, 16, path, NarrowEvaluator, worst, failures, engine_ok=_narrowed)
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["logy20", "bspline17", "plzspline17", "zspline17"])
def test_replay_mode(fixture, name, monkeypatch, tmp_path):
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_DETERMINISTIC", "1")
    _run(U.Term(fixture, name), "deterministic", _compiled_chain, repeat=True)


@pytest.mark.parametrize("name, which", [("logy17", "fixture"), ("plpeak", "parametric_fixture"), ("plzspline7", "fixture")])
def test_marginalised_selection(request, name, which, monkeypatch, tmp_path):
    """The squared-weight pass (marginalize_selection=True) against ``reference_marginalised``, assembled from the fixture: catalog B,
    whose five injections give the correction real weight."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    term = U.Term(request.getfixturevalue(which), name)
    worst, failures = U.Worst(), []
    cat = U.catalog_b(term, EngineEvaluator)
    assert _compiled_chain(cat.ev.eng.scan_kernel_name())
    U.check_gradients(cat, "marginalised/catalog_b", worst, failures, points=U.marginalised_points(term), marginalised=True)
    cat.close()
    _finish(worst, failures)
