"""CPU: the referee of tests/sites_hp_util.py (every site the tail of an evaluation outputs, the cuts and the gradient under them,
assembled in np.longdouble from the high-precision term fixtures) against the same assembly in mpmath at 50 digits; the conditions its
bars rest on (kappa <= 2, the share of live events, which comparison decides next to each threshold); and the C oracle and
oracle/numpy_oracle.py held to it with the assertions and bars the engine faces in tests/test_gpu_sites_hp.py, so that a disagreement
there can be attributed."""
import numpy as np
import pytest
import sites_hp_util as S
import terms_hp_util as U
from test_terms_hp_cpu import OracleEvaluator

CATALOGS = [S.sites_small, S.sites_tiles]
ALL_CATALOGS = [S.sites_small, S.sites_tiles, lambda t, m: S.sites_tiles(t, m, designed=False), lambda t, m: S.sites_tiles(t, m, designed=False, heavy=True)]


class NoEvaluator:
    """A catalog for the referee alone."""

    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import bind

        self.bound = bind(d_pe, d_inj)


@pytest.fixture(scope="module")
def terms():
    return {name: S.load_term((kind, name)) for kind, name in S.TERMS}


@pytest.mark.parametrize("name", ["plpeak_ratio", "logy17"])
def test_longdouble_referee_against_mpmath_at_50_digits(terms, name):
    """The same assembly (analysis.py:76-136, :259-317) from the same float64 log-densities with mpmath: 1e-17 relative on every site.
    Every site is a DIFFERENCE (log S1 - log N, 2 log S1 - log S2, 1 / n_eff - 1 / N), and a 64-bit mantissa (2^-64 = 5.4e-20 of
    each term) cannot hold 1e-17 of a difference that happens to come out 200 times smaller than its terms (logBF = 0.0056 from two
    logarithms of 1.1: 1.3e-17 of the value, 7e-20 of the terms): the bar is 1e-17 of the larger of the terms a site is the
    difference of, as for the variances (1 / n_eff and 1 / N) -- nine orders below the tightest bar the engine faces."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    term = terms[name]
    worst = 0.0
    for build in CATALOGS:
        cat = build(term, NoEvaluator)
        n_ev, n_pe = cat.pe_idx.shape
        n_tot = mp.mpf(cat.total_inj)
        for h in range(len(term.theta)):
            ref = S.sites_reference(cat, h)["raw"]

            def sums(idx):
                lp = [mp.mpf(float(v)) for v in term.logp[h][idx] if v > -np.inf]
                return (mp.fsum(mp.exp(v) for v in lp), mp.fsum(mp.exp(2 * v) for v in lp)) if lp else (mp.mpf(0), mp.mpf(0))

            def close(site, got, want, size=None):
                nonlocal worst
                err = abs(mp.mpf(float(got)) + mp.mpf(float(got - np.longdouble(float(got)))) - want) / (size if size is not None else abs(want) if want != 0 else 1)
                worst = max(worst, float(err))
                assert err <= 1e-17, (name, cat.cat_name, term.tags[h], site, float(err))

            total_var = mp.mpf(0)
            for e in range(n_ev):
                s1, s2 = sums(cat.pe_idx[e])
                if s1 == 0:
                    assert np.isneginf(ref["log_bfs"][e]) and np.isnan(ref["log_neffs"][e]) and np.isnan(ref["variances"][e])
                    total_var = mp.nan
                    continue
                log_neff = 2 * mp.log(s1) - mp.log(s2)
                close("logBF", ref["log_bfs"][e], mp.log(s1) - mp.log(n_pe), size=max(abs(mp.log(s1)), mp.log(n_pe)))
                close("log n_eff", ref["log_neffs"][e], log_neff, size=max(2 * abs(mp.log(s1)), abs(mp.log(s2)), mp.mpf(1)))
                close("variance", ref["variances"][e], 1 / mp.exp(log_neff) - mp.mpf(1) / n_pe, size=max(1 / mp.exp(log_neff), mp.mpf(1) / n_pe))
                total_var += 1 / mp.exp(log_neff) - mp.mpf(1) / n_pe
            S1, S2 = sums(cat.inj_idx)
            mu = S1 / n_tot
            var = S2 / n_tot**2 - mu**2 / n_tot
            log_neff_inj = 2 * mp.log(mu) - mp.log(var)
            var_mu = 1 / mp.exp(log_neff_inj) - 1 / n_tot
            close("log mu", ref["log_det_eff"], mp.log(mu), size=max(abs(mp.log(S1)), mp.log(n_tot)))
            close("log n_eff_inj", ref["log_nEff_inj"], log_neff_inj, size=max(2 * abs(mp.log(mu)), abs(mp.log(var))))
            close("variance of log mu", ref["variance_log_detection_efficiency"], var_mu, size=max(1 / mp.exp(log_neff_inj), 1 / n_tot))
            close("kappa", ref["kappa"], (S2 + S1**2 / n_tot) / (S2 - S1**2 / n_tot))
            if not mp.isnan(total_var):
                close("variance_log_likelihood", ref["variance_log_likelihood"], n_ev**2 * var_mu + total_var, size=max(n_ev**2 / mp.exp(log_neff_inj), mp.mpf(1)))
    print(f"{name}: worst relative difference longdouble - mpmath: {worst:.3e}")


def test_conditions_the_bars_and_the_decisions_rest_on(terms):
    """Asserted on the referee before any engine runs: kappa <= 2 wherever the injection total is live; at least 90 % of (term, point)
    pairs have every non-designed event live; the designed events are what they are meant to be; and over the five terms each of the
    three thresholds is approached somewhere, with the other comparison a factor 1 + 1e-6 away (``decisions`` asserts that)."""
    pairs = ok = 0
    kinds = {}
    for name, term in terms.items():
        for build in ALL_CATALOGS:
            cat = build(term, NoEvaluator)
            spread = {"event": 0.0, "injections": 0.0}
            for h in range(len(term.theta)):
                ref = S.sites_reference(cat, h)
                if cat.cat_name != "sites_small":
                    spread["event"] = max(spread["event"], S.tile_maxima_spread(cat, h, cat.pe_idx[S.GRADED_EVENT], 256))
                    spread["injections"] = max(spread["injections"], S.tile_maxima_spread(cat, h, cat.inj_idx, 256))
                if ref["inj_live"]:
                    assert ref["kappa"] <= 2.0, (name, cat.cat_name, term.tags[h], ref["kappa"])
                pairs += 1
                ok += bool(np.all(ref["live"][[e for e in range(len(ref["live"])) if e not in cat.designed]]))
                if cat.dead_event is not None:
                    assert not ref["live"][cat.dead_event] and ref["n_live"][cat.single_event] == 1 and cat.pe_idx[cat.single_event, 650] in U.core_samples(term)[0]
                if cat.uniform_event is not None:
                    assert ref["live"][cat.uniform_event] and len(set(cat.pe_idx[cat.uniform_event])) == 1
                for label, nobs, flags, expect in S.decisions(cat, h):
                    kinds[(name, cat.cat_name, label)] = kinds.get((name, cat.cat_name, label), 0) + 1
                    if label == "variance cut":
                        assert ref["sum_variances"] <= 0.5
            # live tiles of one group whose maxima differ: by more than 200 (f_t = exp(-200): the whole tile leaves the sums; the
            # fixtures' log-densities spread over 200 to 280, so no catalog drawn from them reaches further), 35 for plpeak_ratio
            if cat.cat_name != "sites_small":
                need = 35.0 if name == "plpeak_ratio" else 200.0
                assert spread["event"] > need and spread["injections"] > need, (name, cat.cat_name, spread)
    assert ok >= 0.9 * pairs, (ok, pairs)
    # every threshold is approached on every term, on the single-tile and on a multi-tile catalog, at two hyper-points or more
    # (2 entries per point); the variance comparison needs sum variances <= 0.5, which the heavy variant of plzspline7 never has
    for name in terms:
        for key in (("sites_small", "injection cut"), ("sites_tiles/plain", "injection cut"), ("sites_tiles/plain", "variance cut"), ("sites_tiles/heavy", "event cut")):
            assert kinds.get((name,) + key, 0) >= 4, (name, key, kinds.get((name,) + key, 0))
    assert sum(v for (n, c, label), v in kinds.items() if c == "sites_small" and label == "event cut") >= 4


def _oracle_evaluate(cat):
    def evaluate(theta, total_inj, nobs, flags):
        with np.errstate(all="ignore"):
            r = cat.ev.orc.evaluate(theta, total_inj, nobs=nobs, **flags)
        return S.Got(r["summary"], r["grad"], r["logBFs"], r["log_nEffs"], r["variance_log_BFs"])

    return evaluate


@pytest.mark.parametrize("name", [n for _, n in S.TERMS])
def test_c_oracle_sites_against_the_referee(terms, name):
    worst, failures = U.Worst(), []
    conv = {}
    for build in ALL_CATALOGS:
        cat = build(terms[name], OracleEvaluator)
        S.check_catalog(cat, "oracle", worst, failures, _oracle_evaluate(cat), conv=conv)
    print("\n".join(worst.lines()))
    U.report(failures, worst)


@pytest.mark.parametrize("name", ["plpeak_ratio", "plzspline7"])
def test_c_oracle_marginalised_sites_against_the_referee(terms, name):
    worst, failures = U.Worst(), []
    for build in (S.sites_small, lambda t, m: S.sites_tiles(t, m, designed=False)):
        cat = build(terms[name], OracleEvaluator)
        S.check_catalog(cat, "oracle/marginalised", worst, failures, _oracle_evaluate(cat), marginalised=True)
    U.report(failures, worst)


class NumpySummary:
    pass


class NumpyEvaluator(NoEvaluator):
    """oracle/numpy_oracle.py's restatement of the reference's assembly, fed the fixture's own float64 log-densities (the model
    functions of that file cover compositions, not single terms): sites only, it has no analytic gradient."""

    def attach(self, cat):
        self.cat = cat

    def evaluate(self, theta, total_inj, nobs, flags):
        from oracle import numpy_oracle as O

        cat, t = self.cat, self.cat.term
        h = [k for k in range(len(t.theta)) if np.array_equal(cat.theta(k), theta)][0]
        with np.errstate(all="ignore"):
            s = O.hierarchical_likelihood(t.logp[h][cat.pe_idx], t.logp[h][cat.inj_idx], total_inj, cat.pe_idx.shape[0] if nobs is None else nobs, 1.0, 1.0, log=True, **flags)
        out = NumpySummary()
        for k in S.SUMMARY_SITES + ("log_likelihood",):
            setattr(out, k, float(s[k]) if k in s else float("nan"))
        out.log_det_eff = float(np.log(s["detection_efficiency"]))
        out.min_log_nEff = float(np.min(np.nan_to_num(s["log_nEffs"])))
        return S.Got(out, None, s["logBFs"], s["log_nEffs"], s["variance_log_BFs"])


@pytest.mark.parametrize("name", ["truncnorm", "logxlogy17"])
def test_numpy_oracle_assembly_against_the_referee(terms, name):
    worst, failures = U.Worst(), []
    for build in ALL_CATALOGS:
        cat = build(terms[name], NumpyEvaluator)
        S.check_catalog(cat, "numpy_oracle", worst, failures, cat.ev.evaluate)
    print("\n".join(worst.lines()))
    U.report(failures, worst)
