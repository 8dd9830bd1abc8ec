"""GPU (-m gpu): the engine against the third high-precision fixture (tests/golden/mass_forms_hp.npz, mpmath at 80 digits;
tests/golden/make_mass_forms_hp.py): the power law with SAMPLED bounds (GWI_TERM_POWERLAW_BOUNDS, the one term whose support moves
with theta), the unnormalised pairing factor of the component-mass models, and the mass-ratio power law that rebuilds log m1 from the
m1 spline's knot coordinate (GWI_RATIO_LOGM_FROM_SPLINE).  tests/test_mass_forms_hp_cpu.py holds the two host-side oracles to the
same fixture with the same bars.

Bars (tests/terms_hp_util.py, unchanged): |log w - ref| < 1e-11 and -inf exactly where the fixture has it; every gradient COMPONENT
within 1e-8 max(1, |ref_j|); log_l within 1e-9.  For the mass-ratio power law next to the spline the value bar at sample i is
1e-11 + |d log p / d log m1| eps_lm, eps_lm derived there from the arithmetic of the two bindings (EPS_LM_OWN, EPS_LM_FOLD).

Every test asserts the path it means to take (``scan_kernel_name()``, ``batch_path()``, the ratio term's flag).  With
GWI_TERMS_HP_REPORT=<file> the worst error per term, path and quantity is appended to that file (profiles/mass_forms_hp/RESULTS.md
keeps one such run)."""
import os

import numpy as np
import pytest
import terms_hp_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return U.load_mass_forms()


@pytest.fixture(scope="module")
def spline_fixture():
    return U.load_spline()


@pytest.fixture(scope="module")
def parametric_fixture():
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


def _finish(worst, failures, extra=()):
    out = os.environ.get("GWI_TERMS_HP_REPORT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(list(extra) + worst.lines()) + "\n")
    U.report(failures, worst)


def _run(term, path, kernel_ok, groups=None, eps_lm=None, engine_ok=None):
    """Values on the values catalog; gradients and log_l on catalogs A and B (per nest of intervals where ``groups`` names them)."""
    worst, failures = U.Worst(), []
    cat = U.values_catalog(term, EngineEvaluator)
    name = cat.ev.eng.scan_kernel_name()
    assert kernel_ok(name), name
    if engine_ok:
        engine_ok(cat.ev.eng)
    U.check_values(cat, f"{path}/values_catalog", worst, failures, eps_lm=eps_lm)
    cat.close()
    for points in groups or [None]:
        for build in (U.catalog_a, U.catalog_b):
            cat = build(term, EngineEvaluator, points)
            name = cat.ev.eng.scan_kernel_name()
            assert kernel_ok(name), name
            U.check_gradients(cat, f"{path}/{build.__name__}", worst, failures, points=points, eps_lm=eps_lm)
            cat.close()
    _finish(worst, failures)


def _batch(term, pts, path, worst, failures, points=None, eps_lm=None, path_ok=None):
    """``pts`` in ONE launch on catalogs A and B: every point against the fixture and against its own single evaluation (1e-11 relative
    on the value, the gradient bar per component).  Returns the batched path the engine took."""
    took = None
    for build in (U.catalog_a, U.catalog_b):
        cat = build(term, EngineEvaluator, points)
        eng = cat.ev.eng
        took = eng.batch_path(len(pts))
        assert path is None or took == path, (took, path)
        if path_ok:
            path_ok(eng)
        total = float(len(cat.inj_idx))
        batch = eng.evaluate_batch(np.stack([cat.theta(h) for h in pts]), total, min_neff_cut=False)
        where = f"batch:{took}:K{len(pts)}/{build.__name__}"
        U.check_gradients(cat, where, worst, failures, points=pts, results={h: (b.log_likelihood, b.grad) for h, b in zip(pts, batch)}, eps_lm=eps_lm)
        for h, b in zip(pts, batch):
            one = eng.evaluate(cat.theta(h), total, min_neff_cut=False)
            size = max(abs(one.log_likelihood), U.reference(cat, h)[2]) if U.is_cancelled(term, h, cat) else abs(one.log_likelihood)
            if not abs(b.log_likelihood - one.log_likelihood) <= 1e-11 * size:
                failures.append(f"{term.name} [{where}] {term.tags[h]}: batched log_l {b.log_likelihood!r} vs single {one.log_likelihood!r}")
            e = U.grad_errors(term, b.grad, one.grad)
            if not np.all(e <= U.GRAD_RTOL):
                failures.append(f"{term.name} [{where}] {term.tags[h]}: batched gradient vs single evaluation: {e.max():.3e}")
        cat.close()
    return took


# ---------------------------------------------------------------------------------------------------------------------
# plbounds
# ---------------------------------------------------------------------------------------------------------------------
def _groups(term, fixture, which=(0, 1)):
    return [U.group_points(term, fixture, g) for g in which]


def test_plbounds_ahead_of_time_chain(fixture):
    term = U.Term(fixture, "plbounds")
    _run(term, "aot:plb", lambda k: k == "plb", groups=_groups(term, fixture))


def test_plbounds_twice_next_to_the_redshift_power_law(fixture, spline_fixture):
    """powerlaw_redshift x plbounds x plbounds on a second arrangement of the samples: the ahead-of-time chain "plz+plb2"."""
    term = U.plbounds_product(fixture, spline_fixture)
    _run(term, "aot:plz+plb2", lambda k: k == "plz+plb2", groups=_groups(term, fixture, (0,)))


def test_plbounds_generic_kernel(fixture, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    term = U.Term(fixture, "plbounds")
    _run(term, "generic", lambda k: k.startswith("generic"), groups=_groups(term, fixture))


def test_plbounds_chain_compiled_at_run_time(fixture, parametric_fixture, monkeypatch, tmp_path):
    """plbounds x truncated normal: a kind sequence without an ahead-of-time chain."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    tn = U.Term(parametric_fixture, "truncnorm")
    term = U.Product(U.plbounds_arranged(fixture, tn.n), tn)
    _run(term, "jit", lambda k: k.startswith("jit:"), groups=_groups(term, fixture, (0,)))


BATCH_TAGS = ["sweep+0", "[2,50]/sweep+0", "[20,30]/sweep+1e-10", "sweep-1e-10", "[2,50]/sweep+1e-06", "[20,30]/sweep-1e-06", "sweep+2.22e-16", "sweep-2.22e-16",
              "ordinary-2.5", "ordinary-3.5", "ordinary-1.5", "wide/alpha12", "lo8", "hi60", "hi30", "lo+1ulp"]


@pytest.mark.parametrize("mode", ["rows-per-point", "pbatch"])
def test_plbounds_batch_mixing_exponents_and_bounds(fixture, mode, monkeypatch):
    """16 points in one launch: exact -1 on two intervals, +-2^-52, +-1e-10, +-1e-6 and ordinary exponents on EIGHT different
    (lo, hi): the same loaded sample is alive for some points of the launch and dead for others."""
    if mode == "pbatch":
        monkeypatch.setenv("GWI_PBATCH", "1")
    term = U.Term(fixture, "plbounds")
    pts = [term.tags.index(t) for t in BATCH_TAGS]
    assert len(pts) == 16 and len({tuple(term.theta[h, 1:]) for h in pts}) >= 4 and set(pts) <= set(U.group_points(term, fixture, 0))
    live = np.isfinite(term.logp[pts])
    assert np.any(live.any(axis=0) & ~live.all(axis=0))
    worst, failures = U.Worst(), []
    _batch(term, pts, mode, worst, failures, points=U.group_points(term, fixture, 0))
    _finish(worst, failures)


def test_plbounds_per_event_sites_at_the_exact_exponent(fixture):
    """log_bfs of one-sample events IS the log-density: at alpha == -1.0 the reference's -log x - log(hi / lo), on every interval that
    has the exact point; and the gradient slots of the two bounds are exactly 0."""
    term = U.Term(fixture, "plbounds")
    cat = U.values_catalog(term, EngineEvaluator)
    assert cat.ev.eng.scan_kernel_name() == "plb"
    exact = [h for h in range(len(term.theta)) if term.theta[h, 0] == -1.0]
    assert len(exact) >= 6
    failures = []
    for h in exact:
        got, ref = np.asarray(cat.ev.eng.evaluate(cat.theta(h), float(term.n), min_neff_cut=False).log_bfs), term.logp[h]
        dead = np.isneginf(ref)
        if not np.array_equal(np.isneginf(got), dead):
            failures.append(f"{term.tags[h]}: the support of log_bfs differs from the fixture's")
        elif not np.all(np.abs(got[~dead] - ref[~dead]) < U.VALUE_ATOL):
            failures.append(f"{term.tags[h]}: log_bfs differ from the fixture by {np.max(np.abs(got[~dead] - ref[~dead])):.3e}")
    cat.close()
    for g in (0, 1):
        points = U.group_points(term, fixture, g)
        for build in (U.catalog_a, U.catalog_b):
            cat = build(term, EngineEvaluator, points)
            for h in points:
                grad = np.asarray(cat.ev.evaluate(cat.theta(h), float(len(cat.inj_idx)))[1])[cat.slot]
                if not (grad[1] == 0.0 and grad[2] == 0.0):
                    failures.append(f"{build.__name__} {term.tags[h]}: d/dlo, d/dhi = {grad[1]!r}, {grad[2]!r}")
            cat.close()
    assert not failures, "\n".join(failures)


def test_plbounds_gradient_is_continuous_across_the_exact_point(fixture):
    """Across 1 + alpha = -2^-52, 0, +2^-52 the engine's gradient moves by no more than the fixture's does, plus the bar."""
    term = U.Term(fixture, "plbounds")
    hs = [term.tags.index(t) for t in ("sweep-2.22e-16", "sweep+0", "sweep+2.22e-16")]
    assert [term.theta[h, 0] for h in hs] == [-1.0 - 2.0**-52, -1.0, -1.0 + 2.0**-52]
    failures = []
    for build in (U.catalog_a, U.catalog_b):
        cat = build(term, EngineEvaluator, U.group_points(term, fixture, 0))
        total = float(len(cat.inj_idx))
        got = [np.asarray(cat.ev.evaluate(cat.theta(h), total)[1])[cat.slot] for h in hs]
        ref = [U.reference(cat, h)[1] for h in hs]
        for a, b in ((0, 1), (1, 2)):
            step, ref_step = np.abs(got[a] - got[b]), np.abs(ref[a] - ref[b])
            bar = U.GRAD_RTOL * np.maximum(1.0, np.abs(ref[b]))
            if not np.all(step <= ref_step + bar):
                failures.append(f"{build.__name__}: gradient step {step.tolist()} across the exact point; the fixture's is {ref_step.tolist()}")
        cat.close()
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------
# the pairing factor of the component-mass models
# ---------------------------------------------------------------------------------------------------------------------
def _component_masses(fixture, spline_fixture, name):
    s = U.Term(spline_fixture, "logxlogy17")
    return U.Joint(U.Shared(s, fixture["pairing/perm"]), U.Term(fixture, name))


def _three_terms_one_block(eng):
    assert len(eng.bound.terms) == 3 and eng.bound.n_theta == 18, (len(eng.bound.terms), eng.bound.n_theta)


@pytest.mark.parametrize("name", ["pairing_iid", "pairing_indep"])
def test_component_masses_on_the_chain_the_engine_picks(fixture, spline_fixture, name, monkeypatch, tmp_path):
    """BSplineIIDComponentMasses masks q > 1 (-inf exactly where the fixture has it); BSplineIndependentComponentMasses keeps it alive."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    term = _component_masses(fixture, spline_fixture, name)
    q = term.cols[1] / term.cols[0]
    inside = np.isfinite(term.parts[0].logp[0])
    assert np.all(np.isneginf(term.logp[:, q > 1])) if name == "pairing_iid" else np.all(np.isfinite(term.logp[:, inside & (q > 1)])) and np.any(inside & (q > 1))
    _run(term, "chain", lambda k: not k.startswith("generic"), engine_ok=_three_terms_one_block)


@pytest.mark.parametrize("name", ["pairing_iid", "pairing_indep"])
def test_component_masses_generic_kernel(fixture, spline_fixture, name, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    _run(_component_masses(fixture, spline_fixture, name), "generic", lambda k: k.startswith("generic"), engine_ok=_three_terms_one_block)


@pytest.mark.parametrize("name", ["pairing_iid", "pairing_indep"])
def test_component_masses_batch_of_16(fixture, spline_fixture, name, monkeypatch, tmp_path):
    """Every hyper-point (the eight beta, each with one of the spline's coefficient vectors), repeated to 16, on whatever batch_path(16)
    selects; the name goes into the report."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    term = _component_masses(fixture, spline_fixture, name)
    pts = [k % len(term.theta) for k in range(16)]
    worst, failures = U.Worst(), []
    took = _batch(term, pts, None, worst, failures)
    assert took in ("taps", "mfma", "rows", "rows-per-point", "pbatch"), took
    _finish(worst, failures, extra=[f"{term.name}: batch_path(16) = {took}"])


# ---------------------------------------------------------------------------------------------------------------------
# the mass-ratio power law next to the m1 spline
# ---------------------------------------------------------------------------------------------------------------------
def _primary_ratio(fixture, spline_fixture, name):
    return U.Joint(U.Term(spline_fixture, "logxlogy20"), U.RatioTerm(fixture, name))


def _folded(fold):
    def check(eng):
        from gwinferno_amd import _native as N

        ratio = [t for t in eng.bound.terms if t["kind"] == N.TERM_POWERLAW_RATIO][0]
        assert bool(ratio["flags"] & N.RATIO_LOGM_FROM_SPLINE) == fold and len(eng.bound.pe_exprs) == (3 if fold else 4), (ratio["flags"], len(eng.bound.pe_exprs))

    return check


@pytest.mark.parametrize("name", list(U.RATIO_MMIN))
def test_folded_ratio(fixture, spline_fixture, name, monkeypatch, tmp_path):
    """The default binding: the ratio term carries GWI_RATIO_LOGM_FROM_SPLINE and the engine has one column fewer."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.delenv("GWI_FOLD_LOGM", raising=False)
    _run(_primary_ratio(fixture, spline_fixture, name), "fold", lambda k: not k.startswith("generic"), eps_lm=U.EPS_LM_FOLD, engine_ok=_folded(True))


@pytest.mark.parametrize("fold", [True, False])
def test_ratio_keeps_the_sample_one_ulp_above_mmin_alive(fixture, spline_fixture, fold, monkeypatch, tmp_path):
    """m1 = nextafter(3.0, +inf) with mmin = 3.0: fl(mmin / m1) = 1 - 2^-53 < 1, so the reference's density is finite (~1e16) and the
    fixture has the sample alive.  float64 log(m1) rounds to log(3.0) and log(mmin / m1) is 0, which the term once took for
    m1 == mmin; that case is now the mask's (on the quotient), and the term evaluates such a live sample at r = 1 - 2^-53.  The
    sample m1 == mmin itself stays -inf (``test_folded_ratio`` and its siblings compare its support)."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_FOLD_LOGM", "1" if fold else "0")
    failures = []
    cat = U.values_catalog(_primary_ratio(fixture, spline_fixture, "ratio_on_logxlogy20_mmin3"), EngineEvaluator)
    _folded(fold)(cat.ev.eng)
    U.check_waived_liveness(cat, failures)
    cat.close()
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:8])


@pytest.mark.parametrize("name", list(U.RATIO_MMIN))
def test_ratio_with_its_own_log_m1_column(fixture, spline_fixture, name, monkeypatch, tmp_path):
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("GWI_FOLD_LOGM", "0")
    _run(_primary_ratio(fixture, spline_fixture, name), "own", lambda k: not k.startswith("generic"), eps_lm=U.EPS_LM_OWN, engine_ok=_folded(False))


@pytest.mark.parametrize("name", list(U.RATIO_MMIN))
def test_folded_ratio_generic_kernel(fixture, spline_fixture, name, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    monkeypatch.delenv("GWI_FOLD_LOGM", raising=False)
    _run(_primary_ratio(fixture, spline_fixture, name), "fold:generic", lambda k: k.startswith("generic"), eps_lm=U.EPS_LM_FOLD, engine_ok=_folded(True))


@pytest.mark.parametrize("name", list(U.RATIO_MMIN))
def test_folded_ratio_batch_of_16_mixing_the_sweep(fixture, spline_fixture, name, monkeypatch, tmp_path):
    """Exact -1, +-2^-52, +-1e-10, +-1e-6, +-1e-3 (inside the series branch), +-0.1 (outside it) and ordinary exponents in one launch."""
    monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    monkeypatch.delenv("GWI_FOLD_LOGM", raising=False)
    term = _primary_ratio(fixture, spline_fixture, name)
    want = ["sweep+0", "sweep+2.22e-16", "sweep-2.22e-16", "sweep+1e-10", "sweep-1e-10", "sweep+1e-06", "sweep-1e-06", "sweep+0.001", "sweep-0.001", "sweep+0.1", "sweep-0.1"]
    ratio_tags = term.parts[1].tags
    pts = [ratio_tags.index(t) for t in want] + [h for h, t in enumerate(ratio_tags) if t == "ordinary"][:5]
    assert len(pts) == 16 and len(term.theta) == len(ratio_tags)
    worst, failures = U.Worst(), []
    took = _batch(term, pts, None, worst, failures, eps_lm=U.EPS_LM_FOLD, path_ok=_folded(True))
    _finish(worst, failures, extra=[f"{term.name}: batch_path(16) = {took}"])
