"""Shared by tests/test_sites_hp_cpu.py (the C oracle and oracle/numpy_oracle.py) and tests/test_gpu_sites_hp.py (the engine, on every
tail it has): EVERYTHING the tail of an evaluation outputs -- the per-event sites, the selection summary, the two cuts and the
gradient under them -- against one referee assembled in np.longdouble from the high-precision term fixtures (tests/terms_hp_util.py),
on catalogs that reach the tail's shapes from a fixture of 30-60 samples.

Catalogs.  A catalog is a list of sample INDICES into a term's fixture, drawn with replacement with a fixed seed, so the referee stays
exact whatever the size (``total_inj`` is four times the found count: S1^2 / N_tot <= S2 / 4 by Cauchy-Schwarz, so V = S2 - S1^2 / N_tot
keeps three quarters of S2 and kappa = (S2 + S1^2/N_tot) / (S2 - S1^2/N_tot) <= 5/3):
  sites_small   5 events x 3 samples, 6 found injections, total_inj = 24, core samples only (live at every hyper-point): one tile per
                group, the host-final default.
  sites_tiles   7 events x 700 samples, 1500 found injections, total_inj = 6000; under GWI_SAMPLES_PER_BLOCK=256 several tiles per
                event, the last ragged.  Events 1, 2, 3 are DESIGNED: 1 draws only from dead samples, 2 has exactly one core sample
                (index 650, in the last tile) among dead ones, 3 repeats one core sample 700 times (uniform weights: n_eff = N_pe,
                variance 0).  ``designed=False`` makes them random draws too (the variant the threshold decisions run on).
                Event 4 and the injections are GRADED in every variant: consecutive runs of draws from three disjoint pools of core
                samples (``graded_pools``), so the tiles of one group have maxima that differ by 200 and more at some hyper-points
                (40 for plpeak_ratio, whose densities spread no further) and the rescaling f_t = exp(m_t - M) of the combine step
                and its square on S2 carry the result.  ``heavy=True`` makes event 5 ten live draws among 690 dead ones (n_eff <=
                10 < n_eff_inj / 4): the variant on which the EVENT comparison decides at every point.
The five terms this suite uses have NO sample that is dead at some hyper-points and live at others (``core_samples(term)[1]`` is empty
for each): the dead samples are the ones outside the support at EVERY point, so the designed events are dead (1) and single-sample (2)
at every point; ``truncnorm`` has no dead sample at all, and its events 1 and 2 are random draws.  For a spline redshift model both
sides carry the two end samples and no injection lies beyond zmax (``terms_hp_util.pins``).

Referee.  ``sites_reference`` follows the reference's analysis.py:76-136 (per-event Bayes factors, detection efficiency) and :259-317
(marginalised shift, the three comparisons, nan_to_num, the sites) line by line in np.longdouble from ``term.logp[h]`` and
``term.dlogp[h]`` alone, in the scale-free forms (weights relative to the side's maximum).  tests/test_sites_hp_cpu.py holds it to the
same assembly in mpmath at 50 digits.

Bars.  The engine's log-weights are within delta = VALUE_ATOL = 1e-11 of the fixture's (tests/test_gpu_terms_hp.py); with
w_i -> w_i e^(eps_i), |eps_i| <= delta, to first order (1.01 covers the second):
  logBF = log S1 - log N_pe            |d log S1| <= delta                                    delta
  log n_eff = 2 log S1 - log S2        |d log S2| <= 2 delta                                  4 delta
  variance = 1/n_eff - 1/N_pe          d(1/n_eff) = (1/n_eff) d log n_eff                     4 delta / n_eff + 2^-52 / N_pe (the subtraction)
  log mu = log S1 - log N_tot                                                                 delta
  log n_eff_inj = 2 log S1 - log V     |dV| <= 2 delta (S2 + S1^2/N_tot) = 2 delta kappa V    2 delta (1 + kappa)
  variance of log mu = 1/n_eff_inj - 1/N_tot                                                  2 delta (1 + kappa) / n_eff_inj
  variance_log_likelihood = N_obs^2 var_mu + sum variances                                    N_obs^2 bar(var_mu) + sum bar(variance)
  min_log_nEff                                                                                4 delta
  sum_logBFs, selection_factor, log_l  LOGL_RTOL relative, of the cancelled sums where ``is_cancelled`` says so (terms_hp_util)
  gradient                             GRAD_RTOL per component of max(1, |ref_j|)
Dead and degenerate segments are compared exactly: a dead event has logBF = -inf and NaN for log n_eff and the variance, the
single-live-sample event |log n_eff| <= 4 delta, the uniform event |variance| <= 4 delta / N_pe.

Decisions.  ``decisions`` chooses N_obs from the referee's own numbers, eta = 1e-9 either side of each threshold (the relative error of
an n_eff is at most 4 delta (1 + kappa) <= 1.2e-10: a factor 8).  The event comparison (min n_eff <= N_obs) and the injection
comparison (n_eff_inj >= 4 N_obs) cross at N_obs = n_eff_min and N_obs = n_eff_inj / 4: at a given point only the LOWER of the two can
be approached from both sides with the other one quiet, so each point tests the one that decides there, and ``decisions`` asserts in
the referee that the other stays a factor 1 + 1e-6 away: the injection comparison on sites_tiles/plain, the event comparison on
sites_tiles/heavy, both on sites_small.  At these points N_obs != n_ev, and the gradient is held to the convention of ``convention_shift``.  The variance cut needs sum variances <= 0.5 and is made where that holds."""
import numpy as np
import terms_hp_util as U

L = np.longdouble
DELTA = U.VALUE_ATOL
ETA = 1e-9
NEG_BIG = -1.7976931348623157e308
SECOND_ORDER = 1.01
TERMS = [("parametric", "plpeak_ratio"), ("parametric", "truncnorm"), ("spline", "logy17"), ("spline", "logxlogy17"), ("spline", "plzspline7")]
SUMMARY_SITES = ("log_l", "sum_logBFs", "selection_factor", "log_det_eff", "log_nEff_inj", "variance_log_detection_efficiency", "variance_log_likelihood", "min_log_nEff")
FLAGS_OFF = dict(marginalize_selection=False, min_neff_cut=False, max_variance_cut=False)


def load_term(kind_name):
    kind, name = kind_name
    return U.Term(U.load() if kind == "parametric" else U.load_spline(), name)


def _dead_pool(term):
    """Samples an event can be dead on: dead at some hyper-points where the term has such samples, else dead at every one."""
    core, some = U.core_samples(term)
    never = np.flatnonzero(~np.isfinite(term.logp).any(axis=0))
    return some if len(some) else never


class SitesCatalog(U.Catalog):
    def __init__(self, term, make, pe_idx, inj_idx, total_inj, name, dead_event=None, single_event=None, uniform_event=None):
        self.total_inj, self.cat_name = float(total_inj), name
        self.dead_event, self.single_event, self.uniform_event = dead_event, single_event, uniform_event
        super().__init__(term, make, pe_idx, inj_idx)
        attach = getattr(self.ev, "attach", None)
        if attach:
            attach(self)

    @property
    def designed(self):
        return [e for e in (self.dead_event, self.single_event, self.uniform_event) if e is not None]


def _injections(term, rng, n, pool):
    pin = U.pins(term)
    if pin is None:
        return rng.choice(pool, size=n)
    lo, hi, inside = pin
    inj = rng.choice(np.array([c for c in pool if inside[c]]), size=n)
    inj[0], inj[1] = lo, hi
    return inj


def sites_small(term, make):
    core, _ = U.core_samples(term)
    rng = np.random.default_rng(20250)
    pe = rng.choice(core, size=(5, 3))
    pin = U.pins(term)
    if pin is not None:
        pe[0, 0], pe[0, 1] = pin[0], pin[1]
    return SitesCatalog(term, make, pe, _injections(term, rng, 6, core), 24, "sites_small")


def graded_pools(term):
    """The core samples in three disjoint pools -- the three of lowest log-density, the next three, the rest -- ordered at the
    hyper-point where the core samples' log-densities spread the most (the hole, a narrow peak, a steep power law)."""
    core, _ = U.core_samples(term)
    pin = U.pins(term)
    if pin is not None:
        core = np.array([c for c in core if pin[2][c]])
    lp = term.logp[:, core]
    order = core[np.argsort(lp[int(np.argmax(lp.max(axis=1) - lp.min(axis=1)))], kind="stable")]
    return order[:3], order[3:6], order[6:]


GRADED_EVENT, HEAVY_EVENT = 4, 5


def sites_tiles(term, make, designed=True, heavy=False):
    core, _ = U.core_samples(term)
    dead = _dead_pool(term)
    rng = np.random.default_rng(20251)
    pool = np.concatenate([core, dead])  # random events carry dead samples among live ones
    pe = rng.choice(pool, size=(7, 700))
    low, mid, high = graded_pools(term)
    # the graded event and the injections: consecutive runs of samples from DISJOINT pools, so that the tiles of one group have
    # different maxima whatever the tile size (up to 500) and the combine's rescaling f_t = exp(m_t - M) is not 1
    pe[GRADED_EVENT] = np.concatenate([rng.choice(low, size=256), rng.choice(mid, size=256), rng.choice(high, size=188)])
    inj = np.concatenate([rng.choice(low, size=500), rng.choice(mid, size=500), rng.choice(high, size=500)])
    pin = U.pins(term)
    if pin is not None:
        pe[0, 0], pe[0, 1] = pin[0], pin[1]
        inj[-1], inj[-2] = pin[0], pin[1]  # (in the last run: the first two keep their low log-density)
    marks = {}
    if designed:
        if len(dead):
            pe[1] = rng.choice(dead, size=700)
            pe[2] = rng.choice(dead, size=700)
            pe[2, 650] = core[len(core) // 2]
            marks.update(dead_event=1, single_event=2)
        pe[3] = core[len(core) // 3]
        marks.update(uniform_event=3)
    if heavy:
        # an event whose n_eff stays below the injections' n_eff / 4: ten live draws among 690 dead samples (n_eff <= 10), or, for
        # a term without dead samples, among 690 copies of the sample of lowest median log-density
        filler = rng.choice(dead, size=690) if len(dead) else np.full(690, low[0])
        pe[HEAVY_EVENT] = np.concatenate([filler[:345], rng.choice(core, size=10), filler[345:]])
    name = "sites_tiles" if designed else ("sites_tiles/heavy" if heavy else "sites_tiles/plain")
    return SitesCatalog(term, make, pe, inj, 6000, name, **marks)


def tile_maxima_spread(cat, h, idx, chunk):
    """Largest difference between the maxima of two LIVE tiles of ``chunk`` samples of the index run ``idx`` at hyper-point ``h``."""
    lp = cat.term.logp[h][idx]
    m = np.array([np.max(lp[a:a + chunk]) for a in range(0, len(lp), chunk)])
    m = m[np.isfinite(m)]
    return float(m.max() - m.min()) if len(m) > 1 else 0.0


def _side(t, h, idx):
    """Scale-free sums of one side (..., n): maximum m, S1 = sum w, S2 = sum w^2 (w = exp(l - m)), weight-averaged derivatives
    sum w d and sum w^2 d, (P, ...)."""
    lp = t.logp[h][idx].astype(L)
    d = t.dlogp[h][:, idx].astype(L)
    m = np.max(lp, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        w = np.where(np.isneginf(lp), L(0), np.exp(lp - np.where(np.isneginf(m), L(0), m)))
        wd = np.where(w > 0, w * d, L(0))
        w2d = np.where(w > 0, w * w * d, L(0))
    return m[..., 0], np.sum(w, axis=-1), np.sum(w * w, axis=-1), np.sum(wd, axis=-1), np.sum(w2d, axis=-1)


def sites_reference(cat, h, nobs=None, flags=FLAGS_OFF):
    """Every site of the reference's hierarchical_likelihood on ``cat`` at hyper-point ``h`` with ``N_obs = nobs`` (default: the number
    of events) in np.longdouble; floats and float64 arrays out, plus ``kappa``, ``cut`` (which comparisons replaced the value),
    ``scale`` (the largest of the sums log_l is assembled from) and the bars of every site under ``bar``."""
    t = cat.term
    n_ev, n_pe = cat.pe_idx.shape
    nobs = L(n_ev if nobs is None else nobs)
    n_tot = L(cat.total_inj)
    marg, min_neff, max_var = (bool(flags[k]) for k in ("marginalize_selection", "min_neff_cut", "max_variance_cut"))
    with np.errstate(all="ignore"):
        # per_event_log_bayes_factors, log=True (analysis.py:76-88)
        m, s1, s2, swd, _ = _side(t, h, cat.pe_idx)
        lse = np.log(s1) + m                                  # :78 logsumexp(logweights, axis=1)
        log_neffs = 2 * np.log(s1) - np.log(s2)               # :79 (the maxima cancel)
        log_bfs = lse - np.log(L(n_pe))                       # :80
        variances = 1 / np.exp(log_neffs) - 1 / L(n_pe)       # :87
        # detection_efficiency (analysis.py:124-136)
        M, S1, S2, SWD, SW2D = _side(t, h, cat.inj_idx)
        log_mu = np.log(S1) + M - np.log(n_tot)               # :126
        V = S2 - S1 * S1 / n_tot                              # :128 in units of e^2M / N_tot^2
        log_neff_inj = 2 * np.log(S1) - np.log(V)             # :129
        var_mu = 1 / np.exp(log_neff_inj) - 1 / n_tot         # :135
        kappa = (S2 + S1 * S1 / n_tot) / V
        # hierarchical_likelihood (analysis.py:259-317)
        lde = log_mu
        if marg:
            lde = lde - (3 + nobs) / (2 * np.exp(log_neff_inj))                    # :271
        cut = []
        if min_neff and not (log_neff_inj >= np.log(4 * nobs)):                     # :273-277
            lde = L(np.inf)
            cut.append("injections")
        sel = float(NEG_BIG if np.isinf(lde) else -nobs * lde)                      # :278-281
        sum_log_bfs = np.sum(log_bfs)                                               # :282
        log_l = L(sel) + sum_log_bfs if sel != NEG_BIG else L(NEG_BIG)              # :283 (float64: -1.797e308 + x rounds back to it)
        if np.isnan(log_l) or np.isinf(log_l):                                      # :284-291
            log_l = L(NEG_BIG) if (np.isnan(log_l) or log_l < 0) else L(-NEG_BIG)
            cut.append("not finite")
        site_log_l = float(log_l)
        min_log_neff = np.min(np.where(np.isnan(log_neffs), L(0), log_neffs))       # :295 nan_to_num: NaN -> 0
        if min_neff and np.exp(min_log_neff) <= nobs:                               # :296-303
            log_l = L(NEG_BIG)
            cut.append("events")
        vll = nobs * nobs * var_mu + np.sum(variances)                              # :305-308
        if max_var and not (vll <= 1):                                              # :309-317
            log_l = L(NEG_BIG)
            cut.append("variance")
        # gradient: sum_e (sum w d / S1)_e - N_obs (sum w d / S1)_inj, the marginalised shift as terms_hp_util.reference_marginalised
        live = s1 > 0
        grad = np.sum(np.where(live, swd / np.where(live, s1, L(1)), L(0)), axis=-1) - nobs * SWD / S1
        if marg:
            grad = grad + nobs * (3 + nobs) / 2 * (2 * SW2D / S1**2 - 2 * S2 * SWD / S1**3)
        if cut:
            grad = np.zeros_like(grad)
        neffs, neff_inj = np.exp(log_neffs), np.exp(log_neff_inj)
        bar_var = SECOND_ORDER * (4 * DELTA / neffs + L(2.0) ** -52 / n_pe)
        bar_var_mu = SECOND_ORDER * 2 * DELTA * (1 + kappa) / neff_inj
        bar = {"log_bfs": SECOND_ORDER * DELTA, "log_neffs": SECOND_ORDER * 4 * DELTA, "variances": bar_var.astype(np.float64), "log_det_eff": SECOND_ORDER * DELTA,
               "log_nEff_inj": float(SECOND_ORDER * 2 * DELTA * (1 + kappa)), "variance_log_detection_efficiency": float(bar_var_mu),
               "variance_log_likelihood": float(nobs * nobs * bar_var_mu + np.sum(bar_var[live])), "min_log_nEff": SECOND_ORDER * 4 * DELTA}
        parts = [np.sum(lse[live]), n_ev * np.log(L(n_pe)), nobs * (np.log(S1) + M), nobs * np.log(n_tot)]
    f = np.float64
    return {"log_bfs": log_bfs.astype(f), "log_neffs": log_neffs.astype(f), "variances": variances.astype(f), "log_det_eff": float(log_mu), "log_nEff_inj": float(log_neff_inj),
            "variance_log_detection_efficiency": float(var_mu), "selection_factor": sel, "sum_logBFs": float(sum_log_bfs), "log_l": site_log_l,
            "min_log_nEff": float(min_log_neff), "variance_log_likelihood": float(vll), "log_likelihood": float(log_l), "grad": grad.astype(f), "kappa": float(kappa),
            "cut": cut, "scale": float(max(abs(p) for p in parts)), "bar": bar, "live": live, "n_live": np.sum(t.logp[h][cat.pe_idx] > -np.inf, axis=1),
            "raw": {"log_bfs": log_bfs, "log_neffs": log_neffs, "variances": variances, "log_det_eff": log_mu, "log_nEff_inj": log_neff_inj,
                    "variance_log_detection_efficiency": var_mu, "sum_logBFs": sum_log_bfs, "variance_log_likelihood": vll, "kappa": kappa},
            "neff_min": float(np.exp(min_log_neff)), "neff_inj": float(neff_inj), "sum_variances": float(np.sum(variances)), "inj_live": bool(S1 > 0)}


def all_live(ref):
    return bool(ref["inj_live"] and np.all(ref["live"]))


def decisions(cat, h):
    """[(label, nobs, flags, expected cut)] next to every threshold that can be approached at hyper-point ``h`` of a catalog whose sums
    are all live there (see the module docstring); asserts in the referee that only the comparison under test decides."""
    base = sites_reference(cat, h)
    if not all_live(base):
        return []
    out = []
    cut_on = dict(FLAGS_OFF, min_neff_cut=True)
    n_ev_cross, n_inj_cross = base["neff_min"], base["neff_inj"] / 4.0
    if n_ev_cross * (1 + 1e-6) < n_inj_cross:
        for nobs, expect in ((n_ev_cross * (1 + ETA), ["events"]), (n_ev_cross * (1 - ETA), [])):
            out.append(("event cut", nobs, cut_on, expect))
    elif n_inj_cross * (1 + 1e-6) < n_ev_cross:
        for nobs, expect in ((n_inj_cross * (1 + ETA), ["injections"]), (n_inj_cross * (1 - ETA), [])):
            out.append(("injection cut", nobs, cut_on, expect))
    if base["sum_variances"] <= 0.5 and base["variance_log_detection_efficiency"] > 0:
        var_on = dict(FLAGS_OFF, max_variance_cut=True)
        for s, expect in ((1 + ETA, ["variance"]), (1 - ETA, [])):
            out.append(("variance cut", float(np.sqrt(L(1 - base["sum_variances"]) * L(s) / L(base["variance_log_detection_efficiency"]))), var_on, expect))
    for label, nobs, flags, expect in out:
        ref = sites_reference(cat, h, nobs, flags)
        assert ref["cut"] == expect, f"{cat.term.name} {cat.cat_name} {cat.term.tags[h]}: {label} at N_obs = {nobs!r}: the referee cuts {ref['cut']}, expected {expect}"
    return out


class Got:
    """What an evaluator returned, by the referee's names; per-event arrays and the gradient may be None."""

    def __init__(self, summary, grad, log_bfs=None, log_neffs=None, variances=None):
        self.summary = {k: float(getattr(summary, k)) for k in SUMMARY_SITES + ("log_likelihood",)}
        self.grad = None if grad is None else np.asarray(grad, dtype=np.float64)
        self.log_bfs, self.log_neffs, self.variances = log_bfs, log_neffs, variances


def _same_special(got, ref):
    """Both NaN, or both the same infinity / the same bits."""
    return (np.isnan(got) and np.isnan(ref)) or got == ref


def check_point(cat, h, got, ref, path, label, worst, failures, values_only=False, nobs=None, conv=None):
    """``got`` (a ``Got``) against ``ref`` (``sites_reference`` with the same N_obs and flags) at hyper-point ``h``: every site its bar."""
    t = cat.term
    where = f"{t.name} [{path}] {cat.cat_name} {t.tags[h]} {label}"

    def miss(site, g, r, err, bar, unit=""):
        failures.append(f"{where}: {site} = {g!r} vs {r!r}: error {err:.3e} > bar {bar:.3e}{unit}")

    def scalar(site, g, r, bar):
        if not np.isfinite(r) or not np.isfinite(g):
            if not _same_special(g, r):
                failures.append(f"{where}: {site} = {g!r} vs {r!r}")
            return
        err = abs(g - r)
        worst.note((t.name, path, site), err / bar if bar > 0 else (0.0 if err == 0 else np.inf), f"{cat.cat_name} {t.tags[h]} {label}: error {err:.3e}, bar {bar:.3e}")
        if not err <= bar:
            miss(site, g, r, err, bar)

    live = ref["live"]
    if got.log_bfs is not None:
        for site, arr in (("log_bfs", got.log_bfs), ("log_neffs", got.log_neffs), ("variances", got.variances)):
            arr, r = np.asarray(arr), ref[site]
            bar = np.broadcast_to(ref["bar"][site], r.shape)
            for e in np.flatnonzero(~live):  # a dead event: -inf, NaN, NaN
                if not _same_special(arr[e], r[e]):
                    failures.append(f"{where}: dead event {e}: {site} = {arr[e]!r}, the reference has {r[e]!r}")
            err = np.abs(arr[live] - r[live])
            if not np.all(np.isfinite(arr[live])):
                failures.append(f"{where}: {site} is not finite at live events {np.flatnonzero(live)[~np.isfinite(arr[live])].tolist()}")
                continue
            if len(err):
                k = int(np.argmax(err / bar[live]))
                e = int(np.flatnonzero(live)[k])
                worst.note((t.name, path, site), err[k] / bar[live][k], f"{cat.cat_name} {t.tags[h]} {label} event {e}: error {err[k]:.3e}, bar {bar[live][k]:.3e}")
                if not err[k] <= bar[live][k]:
                    miss(f"{site}[{e}]", arr[e], r[e], err[k], bar[live][k])
        for e in range(len(live)):
            if live[e] and ref["n_live"][e] == 1 and not abs(got.log_neffs[e]) <= 4 * DELTA:
                failures.append(f"{where}: event {e} has ONE live sample: log n_eff = {got.log_neffs[e]!r}, |.| > {4 * DELTA:g}")
        if cat.uniform_event is not None and not abs(got.variances[cat.uniform_event]) <= 4 * DELTA / cat.pe_idx.shape[1]:
            failures.append(f"{where}: the uniform event's variance = {got.variances[cat.uniform_event]!r}, |.| > 4 delta / N_pe")
    s = got.summary
    if ref["inj_live"]:
        for site in ("log_det_eff", "log_nEff_inj", "variance_log_detection_efficiency", "variance_log_likelihood", "min_log_nEff"):
            scalar(site, s[site], ref[site], ref["bar"][site])
    cancelled = U.is_cancelled(t, h)
    floor = 1.0 if U.base_name(t) in U.SPLINE_TERMS else 0.0
    for site in ("sum_logBFs", "selection_factor", "log_l"):
        g, r = s[site], ref[site]
        if r == NEG_BIG or not np.isfinite(r) or not np.isfinite(g):
            if not _same_special(g, r):
                failures.append(f"{where}: {site} = {g!r} vs {r!r}")
            continue
        size = max(ref["scale"], abs(r), floor) if cancelled else (abs(r) or 1e-300)
        err = abs(g - r) / size
        worst.note((t.name, path, site + " (relative)"), err / U.LOGL_RTOL, f"{cat.cat_name} {t.tags[h]} {label}: relative error {err:.3e}, bar {U.LOGL_RTOL:g}")
        if not err <= U.LOGL_RTOL:
            miss(site, g, r, err, U.LOGL_RTOL, " relative" + (" (of the cancelled sums)" if cancelled else ""))
    # the value the sampler sees, and its gradient
    g, r = s["log_likelihood"], ref["log_likelihood"]
    if ref["cut"]:
        if g != NEG_BIG:
            failures.append(f"{where}: a cut ({', '.join(ref['cut'])}) is expected: log_likelihood = {g!r}, not {NEG_BIG!r}")
        if got.grad is not None and np.any(got.grad != 0.0):
            failures.append(f"{where}: a cut ({', '.join(ref['cut'])}) is expected: the gradient is not zero in every slot (max |g| = {np.max(np.abs(got.grad)):.3e})")
        return
    if g == NEG_BIG:
        failures.append(f"{where}: no cut is expected: log_likelihood = {g!r} (reference {r!r})")
        return
    if g != s["log_l"]:
        failures.append(f"{where}: no cut: log_likelihood {g!r} is not the site log_l {s['log_l']!r}")
    if got.grad is not None and not values_only:
        n_ev = cat.pe_idx.shape[0]
        off = 0.0 if nobs is None else float(nobs) - n_ev
        ref_g, slack = ref["grad"], 1.0
        if off != 0.0:
            if conv is None or h not in conv:
                failures.append(f"{where}: no convention shift is known for this hyper-point: the gradient at N_obs != n_ev cannot be compared")
                return
            ref_g, slack = ref_g + off * conv[h], 1.0 + abs(off) if np.any(conv[h] != 0.0) else 1.0
        e = U.grad_errors(t, got.grad[cat.slot], ref_g) / slack
        j = int(np.argmax(e))
        worst.note((t.name, path, "gradient"), e[j] / U.GRAD_RTOL, f"{cat.cat_name} {t.tags[h]} {label} d/d{t.params[j]}: error {e[j]:.3e} of max(1, |ref|), bar {U.GRAD_RTOL:g}")
        if not e[j] <= U.GRAD_RTOL:
            miss(f"d/d{t.params[j]}", got.grad[cat.slot][j], ref_g[j], e[j], U.GRAD_RTOL, " of max(1, |ref|)" + (f" x {slack:.3g} (convention shift)" if slack != 1.0 else ""))


# Terms whose normalisers sit inside the per-sample term: their gradient follows the reference at every N_obs, full bars.
CONVENTION_FREE = {"plpeak_ratio"}


def convention_shift(cat, h, evaluate):
    """DESIGN.md section 7, "N_obs and the gradient": the engine and the C oracle leave the theta-only normalisers log Z(theta) out of
    the gradient, so at N_obs != n_ev their gradient is the reference's plus (N_obs - n_ev) c with c = d log Z / d theta -- a vector
    that depends on the hyper-point ALONE: not on the catalog, N_obs, the flags or the path.  The fixtures hold derivatives of the
    normalised density only, so c is MEASURED once per (term, path, hyper-point), on sites_small without cuts at N_obs = n_ev + 1,
    and every other catalog, N_obs and flag set is then held to reference + (N_obs - n_ev) c: a gradient zeroed on the uncut side of
    a threshold, a wrong N_obs factor on the selection side (its shift would follow the catalog's injection sums) or in the
    marginalised term all miss.  c carries the bar of the evaluation that measured it, so the bar here is GRAD_RTOL (1 + |N_obs -
    n_ev|).  Terms in CONVENTION_FREE have c = 0 exactly and face the plain bar."""
    t = cat.term
    if t.name in CONVENTION_FREE:
        return np.zeros(len(t.params))
    n_ev = cat.pe_idx.shape[0]
    ref = sites_reference(cat, h, n_ev + 1.0)
    assert all_live(ref) and not ref["cut"]
    got = evaluate(cat.theta(h), cat.total_inj, n_ev + 1.0, FLAGS_OFF)
    if got.grad is None:  # an evaluator without a gradient: nothing will be compared
        return np.zeros(len(t.params))
    return got.grad[cat.slot] - ref["grad"]


def plan(cat, marginalised=False):
    """[(h, label, nobs or None, flags, values_only)]: every evaluation the checks ask of a catalog -- the uncut sites at every
    hyper-point, the decisions next to each threshold where all sums are live, and the dead-event rules where an event is dead."""
    t = cat.term
    out = []
    flat = set(range(len(t.theta))) - set(U.marginalised_points(t))
    for h in range(len(t.theta)):
        if marginalised:
            out.append((h, "marginalised", None, dict(FLAGS_OFF, marginalize_selection=True), h in flat))
            continue
        out.append((h, "no cuts", None, FLAGS_OFF, False))
        # (N_obs != number of events: the gradient is compared under the convention of ``convention_shift``)
        for label, nobs, flags, _ in decisions(cat, h):
            out.append((h, f"{label} N_obs={nobs!r}", nobs, flags, False))
        if cat.dead_event is not None:
            out.append((h, "dead event, min_neff_cut", None, dict(FLAGS_OFF, min_neff_cut=True), False))
            out.append((h, "dead event, min_neff_cut, N_obs=1", 1.0, dict(FLAGS_OFF, min_neff_cut=True), False))
            out.append((h, "dead event, max_variance_cut", None, dict(FLAGS_OFF, max_variance_cut=True), False))
    return out


def check_catalog(cat, path, worst, failures, evaluate, marginalised=False, conv=None):
    """``evaluate(theta, total_inj, nobs, flags) -> Got`` at every entry of ``plan(cat)``.  ``conv``: the dict of convention shifts of
    this (term, path), filled from the first catalog whose sums are all live (sites_small) and shared with the ones after it."""
    conv = {} if conv is None else conv
    if cat.cat_name == "sites_small" and not marginalised:
        for h in range(len(cat.term.theta)):
            conv.setdefault(h, convention_shift(cat, h, evaluate))
    for h, label, nobs, flags, values_only in plan(cat, marginalised):
        ref = sites_reference(cat, h, nobs, flags)
        if cat.dead_event is not None and label != "marginalised":
            assert "not finite" in ref["cut"] or "events" in ref["cut"], (label, ref["cut"])  # the referee's own statement of the dead-event rules
        check_point(cat, h, evaluate(cat.theta(h), cat.total_inj, nobs, flags), ref, path, label, worst, failures, values_only=values_only, nobs=nobs, conv=conv)
    return conv
