"""Posterior-predictive density curves on the engine, with the reference's
function names, arguments, grids and return values (gwinferno/postprocess/calculations.py:20-276: all eight functions).

For every posterior draw the reference evaluates the population density on an 800 x 800 (m1, q) mesh and
integrates it along each axis with the trapezoid rule (:44-52, :78-84).  That is the likelihood hot path
on a synthetic catalog: take the mesh rows as "events" and the trapezoid weights as the inverse sampling
prior, and the engine's per-event importance sums ARE the marginals --

    p_q(q_i) = trapz_m p(m, q_i)  =  N_pe * exp(logBF_i)        (rows = q, samples = m)
    p_m(m_j) = trapz_q p(m_j, q)  =  the same on the transposed mesh

so K draws are K hyper-parameter points of ``gwi_eval_batch``: no new kernels, no (N_draws, 800, 800)
temporaries, and the B-spline models never build their (N_basis, 640 000) design matrices.  The 1-D curves
(spin magnitudes, tilts) are the engine's per-sample log-weights (``gwi_log_weights``) on an 800-point grid, and so are
the merger-rate curves R(z) (:244-276) on the redshift model's own 1000-point grid ``z_model.zs``.

``rate`` / ``pop_frac`` scale the normalised curves exactly as the reference does (:50-51).
"""
import numpy as np

from . import _native as N
from . import models as M
from .engine import NativePopulationLikelihood
from .interpolation import LogYBSpline, trapezoid_weights
from .lazy import Column, Density, Factor, side_of

GRID = 800  # points per axis in every reference PPD function


def _ones(like, n):
    return np.ones(n) if like is None else np.asarray(like, dtype=np.float64)


class _MeshMarginals:
    """Two engines over one (ys x xs) mesh: per-row sums over x, and (transposed) per-column sums over y."""

    def __init__(self, xs, ys, weights_fn, placeholder, keep=None):
        self.xs, self.ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
        X, Y = np.meshgrid(self.xs, self.ys)  # X[i, j] = xs[j], Y[i, j] = ys[i]   (calculations.py:24)
        twx, twy = trapezoid_weights(self.xs), trapezoid_weights(self.ys)
        keep = np.ones_like(X) if keep is None else keep(X, Y).astype(np.float64)
        # orientation A: events = rows (y), samples = x -> integrates over x;  B: the transpose
        self.sides = []
        for Xa, Ya, tw in ((X, Y, twx[None, :] * keep), (np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T), twy[None, :] * keep.T)):
            fn = weights_fn(Xa, Ya, self.xs, self.ys)  # -> callable(draw, pe_samples) -> lazy density
            pe_w = lambda d, fn=fn, tw=np.ascontiguousarray(tw): fn(d, True) * tw  # noqa: E731
            eng = NativePopulationLikelihood(pe_w(placeholder), fn(placeholder, False))
            self.sides.append((pe_w, eng))

    def __call__(self, draws):
        """draws: list of parameter dicts -> (over_x[n, len(ys)], over_y[n, len(xs)])"""
        out = []
        for pe_w, eng in self.sides:
            thetas = np.stack([eng.bound.theta_of(pe_w(d)) for d in draws])
            rows = []
            kmax = 16
            for k0 in range(0, len(draws), kmax):
                res = eng.evaluate_batch(thetas[k0 : k0 + kmax], float(eng.n_inj), min_neff_cut=False, want_grad=False)
                rows.extend(np.exp(r.log_bfs) * eng.n_pe for r in res)
            out.append(np.array(rows))
        return out[0], out[1]

    def close(self):
        for _, eng in self.sides:
            eng.close()


def _normalise(p, grid, rate, frac):
    return rate[:, None] * p * frac[:, None] / np.trapezoid(p, grid, axis=1)[:, None]


def _mass_ppds(weights_fn, draws, placeholder, mmin, mmax, rate, pop_frac, keep=None):
    ms = np.linspace(mmin, mmax, GRID)
    qs = np.linspace(mmin / mmax, 1, GRID)
    keep = keep if keep is not None else (lambda Mg, Qg: Qg > mmin / Mg)  # calculations.py:46, 80
    mesh = _MeshMarginals(ms, qs, weights_fn, placeholder, keep=keep)
    p_q, p_m = mesh(draws)  # integrate over m (axis=1 of the mesh) / over q (axis=0)
    mesh.close()
    n = len(draws)
    rate, pop_frac = _ones(rate, n), _ones(pop_frac, n)
    return _normalise(p_m, ms, rate, pop_frac), ms, _normalise(p_q, qs, rate, pop_frac), qs


def calculate_powerlaw_peak_mass_ppds(alpha, beta, mu_peak, sig_peak, lamb, mmin, mmax, rate=None, pop_frac=None):
    """calculations.py:63-91 -> ``(mpdfs, ms, qpdfs, qs)``."""
    cols = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (alpha, beta, mu_peak, sig_peak, lamb)]
    draws = [dict(zip(("a", "b", "mp", "sp", "lam"), (float(c[i]) for c in cols))) for i in range(len(cols[0]))]

    def weights_fn(Mg, Qg, ms, qs):
        data = {True: (Mg, Qg), False: (ms, qs)}

        def w(d, pe_samples):
            m1, q = data[pe_samples]
            return M.plpeak_primary_ratio_pdf(m1, q, d["a"], d["b"], mmin, mmax, d["mp"], d["sp"], d["lam"])

        return w

    return _mass_ppds(weights_fn, draws, dict(a=-2.0, b=1.0, mp=30.0, sp=5.0, lam=0.1), mmin, mmax, rate, pop_frac)


def calculate_bspline_mass_ppds(m_cs, q_cs, nspline_dict, mmin, mmax, rate=None, pop_frac=None):
    """calculations.py:20-60 -> ``(mpdfs, ms, qpdfs, qs)``."""
    m_cs, q_cs = np.atleast_2d(np.asarray(m_cs, dtype=np.float64)), np.atleast_2d(np.asarray(q_cs, dtype=np.float64))
    draws = [dict(m=m_cs[i], q=q_cs[i]) for i in range(m_cs.shape[0])]

    def weights_fn(Mg, Qg, ms, qs):
        model = M.BSplinePrimaryBSplineRatio(nspline_dict["m1"], nspline_dict["q"], Mg, ms, Qg, qs, m1min=mmin, m2min=mmin, mmax=mmax)
        return lambda d, pe_samples: model(d["m"], d["q"], pe_samples=pe_samples)

    return _mass_ppds(weights_fn, draws, dict(m=np.zeros(nspline_dict["m1"]), q=np.zeros(nspline_dict["q"])), mmin, mmax, rate, pop_frac)


def calculate_peak_logm1_bspline_q_ppds(logmp, logsigp, q_cs, nspline_dict, mmin, mmax, rate=None, pop_frac=None):
    """calculations.py:94-130: log-normal primary-mass peak x LogY B-spline mass ratio -> ``(mpdfs, ms, qpdfs, qs)``."""
    logmp, logsigp = np.atleast_1d(np.asarray(logmp, dtype=np.float64)), np.atleast_1d(np.asarray(logsigp, dtype=np.float64))
    q_cs = np.atleast_2d(np.asarray(q_cs, dtype=np.float64))
    draws = [dict(mu=float(logmp[i]), sg=float(logsigp[i]), q=q_cs[i]) for i in range(q_cs.shape[0])]

    def weights_fn(Mg, Qg, ms, qs):
        q_model = M.BSplineRatio(nspline_dict["q"], Qg, qs, mmin / mmax, basis=LogYBSpline)
        data = {True: Mg, False: ms}
        return lambda d, pe_samples: q_model(d["q"], pe_samples=pe_samples) * M.truncnorm_pdf(data[pe_samples], d["mu"], d["sg"], mmin, mmax, log=True)

    keep = lambda Mg, Qg: ~((Mg < mmin) | (Mg * Qg < mmin))  # noqa: E731  (calculations.py:118)
    return _mass_ppds(weights_fn, draws, dict(mu=3.0, sg=0.5, q=np.zeros(nspline_dict["q"])), mmin, mmax, rate, pop_frac, keep=keep)


# ---- 1-D curves: per-sample log-weights of an 800-point grid -------------------------------------------
def _curves(grid, density_fn, draws, placeholder):
    """density_fn(x, draw) -> lazy density of x; returns pdf[n_draws, len(grid)] (unnormalised)."""
    grid = np.asarray(grid, dtype=np.float64)
    pe = np.ascontiguousarray(grid[None, :])
    eng = NativePopulationLikelihood(density_fn(pe, placeholder), density_fn(grid, placeholder))
    out = []
    for d in draws:
        _, logw = eng.log_weights(eng.bound.theta_of(density_fn(pe, d)))
        out.append(np.exp(logw))
    eng.close()
    return np.array(out)


def calculate_beta_spin_mag(alpha_a, beta_a, amax=1, rate=None, pop_frac=None):
    """calculations.py:133-154 -> ``(apdfs, aa)``."""
    aa = np.linspace(0, amax, GRID)
    alpha_a, beta_a = np.atleast_1d(np.asarray(alpha_a, dtype=np.float64)), np.atleast_1d(np.asarray(beta_a, dtype=np.float64))
    draws = list(zip(alpha_a, beta_a))
    p = _curves(aa, lambda x, d: M.betadist(x, d[0], d[1], scale=amax), draws, (2.0, 2.0))
    n = len(draws)
    return _normalise(p, aa, _ones(rate, n), _ones(pop_frac, n)), aa


def calculate_mixture_iso_aligned_spin_tilt(sig_ct, lambda_ct, rate=None, pop_frac=None):
    """calculations.py:157-178 -> ``(ctpdfs, ct)``."""
    ct = np.linspace(-1, 1, GRID)
    sig_ct, lambda_ct = np.atleast_1d(np.asarray(sig_ct, dtype=np.float64)), np.atleast_1d(np.asarray(lambda_ct, dtype=np.float64))
    draws = list(zip(sig_ct, lambda_ct))
    p = _curves(ct, lambda x, d: M.mixture_isoalign_spin_tilt(x, d[1], d[0]), draws, (1.0, 0.5))
    n = len(draws)
    return _normalise(p, ct, _ones(rate, n), _ones(pop_frac, n)), ct


def calculate_bspline_spin_ppds(a1_cs, tilt1_cs, nspline_dict, a2_cs=None, tilt2_cs=None, rate=None, pop_frac=None):
    """calculations.py:181-241: IID form -> ``(apdfs, aa, ctpdfs, cc)``; independent form ->
    ``(apdfs_1, apdfs_2, aa, ctpdfs_1, ctpdfs_2, cc)`` (LogYBSpline bases, normalised)."""
    aa, cc = np.linspace(0, 1, GRID), np.linspace(-1, 1, GRID)
    a1_cs, tilt1_cs = np.atleast_2d(np.asarray(a1_cs, dtype=np.float64)), np.atleast_2d(np.asarray(tilt1_cs, dtype=np.float64))
    n = a1_cs.shape[0]
    rate, pop_frac = _ones(rate, n), _ones(pop_frac, n)

    def spin_curves(grid, cls, n_splines, coefs):
        model = cls(n_splines, grid[None, :], grid, basis=LogYBSpline, normalize=True)
        dens = lambda x, c: model(c, pe_samples=np.ndim(x) == 2)  # noqa: E731
        return _normalise(_curves(grid, dens, list(coefs), np.zeros(n_splines)), grid, rate, pop_frac)

    if a2_cs is None:
        return (spin_curves(aa, M.BSplineSpinMagnitude, nspline_dict["a"], a1_cs), aa,
                spin_curves(cc, M.BSplineSpinTilt, nspline_dict["tilt"], tilt1_cs), cc)
    a2_cs, tilt2_cs = np.atleast_2d(np.asarray(a2_cs, dtype=np.float64)), np.atleast_2d(np.asarray(tilt2_cs, dtype=np.float64))
    return (spin_curves(aa, M.BSplineSpinMagnitude, nspline_dict["a1"], a1_cs), spin_curves(aa, M.BSplineSpinMagnitude, nspline_dict["a2"], a2_cs), aa,
            spin_curves(cc, M.BSplineSpinTilt, nspline_dict["tilt1"], tilt1_cs), spin_curves(cc, M.BSplineSpinTilt, nspline_dict["tilt2"], tilt2_cs), cc)


# ---- merger rate as a function of redshift: R(z) = rate * pop_frac * (1 + z)^lamb [* exp(spline(log z))] ----------------
def _rate_factor(z, lamb):
    """(1 + z)^lamb, no normaliser and no dVc/dz (calculations.py:253): the bare power law of the engine's term library on
    the column log(1 + z)."""
    side = side_of(z)
    return Factor(N.TERM_POWERLAW, side, [Column("log1p", z)], [lamb], consts=(0.0, 1.0), flags=N.POWERLAW_UNNORMALISED, tag="rate_of_z")


def calculate_powerlaw_rate_of_z_ppds(lamb, rate, z_model, pop_frac=None):
    """calculations.py:244-258 -> ``(rs, zs)``: ``rs[i] = rate[i] * pop_frac[i] * (1 + zs)^lamb[i]`` on ``z_model.zs``."""
    lamb = np.atleast_1d(np.asarray(lamb, dtype=np.float64))
    n = len(lamb)
    rate, pop_frac = _ones(rate, n), _ones(pop_frac, n)
    zs = np.asarray(z_model.zs, dtype=np.float64)
    p = _curves(zs, lambda z, la: Density([_rate_factor(z, la)], side_of(z)), list(lamb), 1.0)
    return rate[:, None] * pop_frac[:, None] * p, zs


def calculate_powerlaw_spline_rate_of_z_ppds(lamb, z_cs, rate, z_model, pop_frac=None):
    """calculations.py:261-276 -> ``(rs, zs)``: the power law times ``exp(sum_k c_k B_k(log z))`` with the redshift model's
    un-normalised LogXBSpline (spline_perturbation.py:317) and the first coefficient pinned to 0 (:269)."""
    lamb = np.atleast_1d(np.asarray(lamb, dtype=np.float64))
    z_cs = np.atleast_2d(np.asarray(z_cs, dtype=np.float64))
    n = len(lamb)
    rate, pop_frac = _ones(rate, n), _ones(pop_frac, n)
    zs = np.asarray(z_model.zs, dtype=np.float64)
    it = z_model.interpolator
    if z_cs.shape[1] != it.N - 1:
        raise ValueError(f"z_cs must hold {it.N - 1} coefficients per draw (the first of the model's {it.N} is pinned to 0)")

    def dens(z, d):
        side = side_of(z)
        sp = Factor(N.TERM_EXP_SPLINE, side, [Column("log", z)], coefs=d[1], consts=(it.lo, it.hi), n_basis=it.N, flags=N.SPLINE_OUTSIDE_ZERO_EXPONENT, tag="rate_of_z_spline")
        return Density([_rate_factor(z, d[0]), sp], side)

    draws = [(float(lamb[i]), np.concatenate([[0.0], z_cs[i]])) for i in range(n)]
    p = _curves(zs, dens, draws, (1.0, np.zeros(it.N)))
    return rate[:, None] * pop_frac[:, None] * p, zs


def posterior_predictive_draws(eng, thetas, n_draws, seed, pedata=None, injdata=None, param_names=None, m1min=None, m2min=None, mmax=None):
    """Population-informed posterior samples and predicted detections for K posterior hyper-parameter draws: per draw and
    event ``n_draws`` posterior samples drawn with probability proportional to their population weight ("reweighted"
    single-event posteriors), and ``n_draws`` found injections from the injection weights -- the draw of the reference's
    posterior-predictive branch (pipeline/analysis.py:321-355), made on the device (``eng.draw_indices``: only indices
    come back).

    ``thetas`` is ``(K, n_theta)`` in the engine's layout.  The uniforms come from ``numpy.random.default_rng(seed)``: the
    result is a function of ``(thetas, n_draws, seed)``.  With all of ``m1min, m2min, mmax`` given and both data
    dictionaries at hand the reference's mass cuts (:326-338) become the engine's draw mask (``eng.set_draw_mask``); otherwise
    the mask the engine already holds stays.

    Returns a dict: ``obs_idx (K, n_ev, n_draws)`` and ``pred_idx (K, n_draws)`` (int32; -1 where nothing has weight) and,
    when the data dictionaries are given, ``obs[p] (K, n_ev, n_draws)``, ``obs_pooled[p] (K, n_ev * n_draws)`` and
    ``pred[p] (K, n_draws)`` for every ``p`` of ``param_names`` (default: the keys both dictionaries share); NaN where the
    index is -1."""
    from .draws import mass_cut_masks

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    n_draws = int(n_draws)
    if n_draws < 1:
        raise ValueError("n_draws must be at least 1")
    cuts = (m1min, m2min, mmax)
    if pedata is not None and injdata is not None and all(c is not None for c in cuts):
        eng.set_draw_mask(*mass_cut_masks(pedata, injdata, m1min, m2min, mmax))
    elif any(c is not None for c in cuts) and not all(c is not None for c in cuts):
        raise ValueError("m1min, m2min and mmax are given together or not at all")
    rng = np.random.default_rng(seed)
    k = thetas.shape[0]
    u_pe, u_inj = rng.uniform(size=(k, eng.n_ev, n_draws)), rng.uniform(size=(k, n_draws))
    obs_idx, pred_idx = eng.draw_indices(thetas, u_pe, u_inj)
    out = {"obs_idx": obs_idx, "pred_idx": pred_idx}
    if pedata is not None and injdata is not None:
        names = list(param_names) if param_names is not None else [p for p in pedata if p in injdata]
        ev = np.arange(eng.n_ev)[None, :, None]
        out["obs"], out["obs_pooled"], out["pred"] = {}, {}, {}
        for p in names:
            a, b = np.asarray(pedata[p], dtype=np.float64), np.asarray(injdata[p], dtype=np.float64)
            obs = np.where(obs_idx >= 0, a[ev, np.maximum(obs_idx, 0)], np.nan)
            out["obs"][p] = obs
            out["obs_pooled"][p] = obs.reshape(k, -1)
            out["pred"][p] = np.where(pred_idx >= 0, b[np.maximum(pred_idx, 0)], np.nan)
    return out


def leave_one_out_weights(eng, thetas, total_inj, nobs=None, marginalize_selection=False):
    """Leave-one-out weights of the K hyper-posterior points ``thetas (K, n_theta)`` for every event, and the leave-one-out predictive
    score they give.  The points are draws from ``p(theta | all N events)``, which already contains event e: reweighting
    e's samples by ``p(x | theta_k)`` would use its data twice.  The posterior of e marginalises over ``p(theta | all events but e)``
    instead, and the same draws serve with the weight ``v_ke`` proportional to ``L_{-e}(theta_k) / L(theta_k) = exp(-l_ke)``, where
    ``l_ke = log L_N(theta_k) - log L_{N-1, without e}(theta_k)`` is the event's contribution to the log-likelihood.

    The likelihood is ``log L_n = sum_i logBF_i + f(n)`` over the n events of the catalog.  Without marginalised selection ``f(n) =
    -n log mu`` with ``mu`` the detection efficiency, so ``l_ke = logBF_e - log mu``.  With it (analysis.py:271) ``f(n) = -n (log mu
    - (3 + n) / (2 n_eff_inj)) = -n log mu + n (3 + n) / (2 n_eff_inj)``, and ``f(N) - f(N - 1) = -log mu + (N (3 + N) - (N - 1)(2 +
    N)) / (2 n_eff_inj) = -log mu + (N + 1) / n_eff_inj``: ``l_ke = logBF_e - log mu + (N + 1) / n_eff_inj``.  ``N`` is ``nobs``
    (default: the engine's events).  ``logBF``, ``log mu`` and ``n_eff_inj`` come from ``eng.evaluate_batch`` without gradients, in
    chunks of the batch limit; the ``min_neff`` and ``variance`` cuts are not applied (a cut replaces the likelihood by a constant and
    says nothing about one event).

    Returns :func:`gwinferno_amd.draws.leave_one_out_summary` of the table: ``log_l_event (K, n_ev)``; ``point_weights (K, n_ev +
    1)`` = ``exp(-l_ke + min_k l_ke)``, at most 1, the injection column all ones -- what ``Engine.marginal_weights_add`` and
    ``Engine.weighted_histograms`` take; ``elpd_loo (n_ev,)`` = ``-log mean_k exp(-l_ke)``; ``lpd (n_ev,)`` = ``log mean_k exp(l_ke)``;
    ``neff_points (n_ev,)`` = ``(sum_k v)^2 / sum_k v^2``; ``n_bad (n_ev,)``, the points whose ``l_ke`` is not finite (weight 0)."""
    from .draws import leave_one_out_summary

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    n_obs = float(eng.n_ev_global if nobs is None else nobs)
    ell = np.empty((k, eng.n_ev))
    step = int(eng.max_batch)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, k, step):
            res = eng.evaluate_batch(thetas[k0 : k0 + step], total_inj, nobs=nobs, marginalize_selection=marginalize_selection, min_neff_cut=False, max_variance_cut=False,
                                     want_grad=False)
            for i, r in enumerate(res):
                row = r.log_bfs - r.summary.log_det_eff
                if marginalize_selection:
                    row = row + (n_obs + 1.0) / np.exp(r.summary.log_nEff_inj)
                ell[k0 + i] = row
    return leave_one_out_summary(ell)


def _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection):
    """``(v (K, n_ev + 1) or None, the leave-one-out summary or None)`` of a post-processing call."""
    from .draws import point_weights_array

    if leave_one_out:
        if point_weights is not None:
            raise ValueError("leave_one_out=True makes the point weights itself: point_weights must be None")
        if total_inj is None:
            raise ValueError("leave_one_out=True needs total_inj")
        loo = leave_one_out_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)
        return loo["point_weights"], loo
    if point_weights is None:
        return None, None
    return point_weights_array(point_weights, thetas.shape[0], eng.n_ev + 1), None


def _point_weight_entries(out, loo, vsum):
    if vsum is not None:
        out["point_weight_sum"] = np.asarray(vsum).copy()
    if loo is not None:
        out["elpd_loo"], out["neff_points"] = loo["elpd_loo"], loo["neff_points"]


HISTOGRAM_CHUNK = 64  # points per gwi_weighted_histograms call of reweighted_event_posteriors (the sums do not depend on it)


def reweighted_event_posteriors(eng, thetas, pe_values, edges, inj_values=None, pedata=None, injdata=None, param_names=None, m1min=None, m2min=None, mmax=None,
                                backend="device", chunk=HISTOGRAM_CHUNK, point_weights=None, leave_one_out=False, total_inj=None, nobs=None, marginalize_selection=False):
    """The population-informed posterior of every event, marginalised over K posterior hyper-parameter draws, as binned densities,
    and the predicted detected distribution from the injections: per event, quantity and bin the mean over the draws of
    ``(sum of w_i in the bin) / (sum of w_i)`` with ``w_i = p(x_i | theta_k) / prior_i`` -- the exact sums whose Monte-Carlo
    estimate :func:`posterior_predictive_draws` gives with one index per draw (the reference's posterior-predictive branch,
    pipeline/analysis.py:321-355).  On the device (``eng.weighted_histograms``) the weights never leave HBM and
    ``(n_ev + 1) * len(names) * B`` doubles come back per chunk of points.

    ``thetas`` is ``(K, n_theta)`` in the engine's layout.  ``pe_values`` maps a name to the ``(n_ev, n_pe)`` array of the
    quantity to bin (any derived quantity, e.g. ``m2 = q * m1``), ``inj_values`` the same names to ``(n_inj,)`` arrays (``None``:
    no predicted distribution); ``edges`` maps each name to increasing bin edges, uniform or not, all with the same number of
    bins ``B <= 256`` (``np.histogram``'s rule: the last edge is inclusive).  ``param_names`` selects and orders the names
    (default: the keys of ``pe_values``; at most 8).  The mass cuts are :func:`posterior_predictive_draws`': with all of
    ``m1min, m2min, mmax`` given and both data dictionaries at hand they become the engine's draw mask, otherwise the mask the
    engine holds stays.  The values are digitised once on the host; the points go to the engine in chunks of at most
    ``chunk <= 64``, which does not change a bit of the result.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.weighted_histograms_reference`) on ``eng.log_weights`` under the masks given here (none without
    the cuts): the statement the kernels are tested against, not a fall-back.

    Returns a dict per name: ``events (n_ev, B)``, the mean normalised histogram divided by the bin widths (a density: ``events *
    widths`` sums to ``1 - outside``); ``predicted (B,)``, the same for the injection set (when ``inj_values`` is given);
    ``outside``, ``{"events": (n_ev,), "predicted": float}``, the weight fraction outside the edges; and ``n_points``, the same
    layout, the points at which the segment had weight (NaN densities where that is 0); beside them ``"edges"`` itself.

    ``point_weights`` -- ``(K, n_ev + 1)``, the injection set last, or ``(K,)`` -- gives every (point, segment) a linear weight in
    ``[0, 1]``, e.g. to move a finished run to another hyper-prior: the mean over the points becomes the weighted mean, the sums
    divided by the sum of the weights over the live points (returned as ``"point_weight_sum" (n_ev + 1,)``) instead of by their
    number.  ``leave_one_out=True`` (``total_inj`` is then required; ``nobs`` and ``marginalize_selection`` as in the likelihood)
    makes the weights with :func:`leave_one_out_weights`, so that no event's data is used twice, and adds ``"elpd_loo"`` and
    ``"neff_points"``.  The defaults leave every output as it was."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    chunk = int(chunk)
    if not 1 <= chunk <= HISTOGRAM_CHUNK:
        raise ValueError(f"chunk must be in 1 ... {HISTOGRAM_CHUNK}")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    names = list(param_names) if param_names is not None else list(pe_values)
    if not 1 <= len(names) <= 8:
        raise ValueError("between 1 and 8 quantities can be binned in one pass")
    n_ev, n_pe, n_inj = eng.n_ev, eng.n_pe, eng.n_inj
    grid = {p: np.asarray(edges[p], dtype=np.float64).ravel() for p in names}
    n_bins = grid[names[0]].size - 1
    if any(g.size - 1 != n_bins for g in grid.values()):
        raise ValueError("every quantity needs the same number of bins")
    if not 1 <= n_bins <= 256:
        raise ValueError("n_bins must be in 1 ... 256")
    pe_bins = np.empty((len(names), n_ev, n_pe), dtype=np.uint16)
    inj_bins = np.empty((len(names), n_inj), dtype=np.uint16) if inj_values is not None else None
    for c, p in enumerate(names):
        v = np.asarray(pe_values[p], dtype=np.float64)
        if v.shape != (n_ev, n_pe):
            raise ValueError(f"pe_values[{p!r}] has shape {v.shape}, the engine's sample set {(n_ev, n_pe)}")
        pe_bins[c] = D.digitize(v, grid[p])
        if inj_bins is not None:
            v = np.asarray(inj_values[p], dtype=np.float64)
            if v.shape != (n_inj,):
                raise ValueError(f"inj_values[{p!r}] has shape {v.shape}, the engine's injection set {(n_inj,)}")
            inj_bins[c] = D.digitize(v, grid[p])
    cuts = (m1min, m2min, mmax)
    masks = (None, None)
    if pedata is not None and injdata is not None and all(c is not None for c in cuts):
        masks = D.mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
        if backend == "device":
            eng.set_draw_mask(*masks)
    elif any(c is not None for c in cuts) and not all(c is not None for c in cuts):
        raise ValueError("m1min, m2min and mmax are given together or not at all")
    v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    vsum = None
    if backend == "device":
        eng.set_histogram_bins(pe_bins, inj_bins, n_bins=n_bins)
        out = None
        for i in range(0, k, chunk):
            out = eng.weighted_histograms(thetas[i : i + chunk], out=out, **({} if v is None else {"point_weights": v[i : i + chunk]}))
        hist_pe, hist_inj, dead = out[:3]
        vsum = out[3] if v is not None else None
    elif v is not None:
        hist_pe, hist_inj, dead = np.zeros((n_ev, len(names), n_bins)), (np.zeros((len(names), n_bins)) if inj_bins is not None else None), np.zeros(n_ev + 1, dtype=np.int32)
        vsum = np.zeros(n_ev + 1)
        for th, row in zip(thetas, v):
            lw_pe, lw_inj = eng.log_weights(th)
            h_pe, h_inj, d, vs = D.weighted_histograms_reference(lw_pe, lw_inj, masks[0], masks[1], pe_bins, inj_bins, n_bins, v=row)
            hist_pe += h_pe
            if hist_inj is not None:
                hist_inj += h_inj
            dead += d
            vsum += vs
    else:
        hist_pe, hist_inj, dead = np.zeros((n_ev, len(names), n_bins)), (np.zeros((len(names), n_bins)) if inj_bins is not None else None), np.zeros(n_ev + 1, dtype=np.int32)
        for th in thetas:
            lw_pe, lw_inj = eng.log_weights(th)
            h_pe, h_inj, d = D.weighted_histograms_reference(lw_pe, lw_inj, masks[0], masks[1], pe_bins, inj_bins, n_bins)
            hist_pe += h_pe
            if hist_inj is not None:
                hist_inj += h_inj
            dead += d
    live = (k - dead).astype(np.float64) if vsum is None else vsum
    result = {"edges": {p: grid[p] for p in names}}
    _point_weight_entries(result, loo, vsum)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c, p in enumerate(names):
            widths = np.diff(grid[p])
            mean_pe = hist_pe[:, c, :] / live[:n_ev, None]
            entry = {"events": mean_pe / widths, "outside": {"events": 1.0 - mean_pe.sum(axis=1)}, "n_points": {"events": (k - dead[:n_ev]).astype(np.int64)}}
            if hist_inj is not None:
                mean_inj = hist_inj[c] / live[n_ev]
                entry["predicted"] = mean_inj / widths
                entry["outside"]["predicted"] = float(1.0 - mean_inj.sum())
                entry["n_points"]["predicted"] = int(k - dead[n_ev])
            result[p] = entry
    return result


def _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names):
    """The quantities of a per-event summary as ``(names, x_pe (C, n_ev, n_pe), x_inj (C, n_inj) or None)``: from ``pe_values`` /
    ``inj_values`` (name -> array), or read from ``pedata`` / ``injdata`` by ``param_names``."""
    if pe_values is None:
        if pedata is None or param_names is None:
            raise ValueError("without pe_values, pedata and param_names name the quantities")
        pe_values = pedata
        if inj_values is None and injdata is not None:
            inj_values = injdata
    names = list(param_names) if param_names is not None else list(pe_values)
    if not 1 <= len(names) <= 8:
        raise ValueError("between 1 and 8 quantities can be summarised in one pass")
    n_ev, n_pe, n_inj = eng.n_ev, eng.n_pe, eng.n_inj
    x_pe = np.empty((len(names), n_ev, n_pe))
    x_inj = np.empty((len(names), n_inj)) if inj_values is not None else None
    for c, p in enumerate(names):
        v = np.asarray(pe_values[p], dtype=np.float64)
        if v.shape != (n_ev, n_pe):
            raise ValueError(f"pe_values[{p!r}] has shape {v.shape}, the engine's sample set {(n_ev, n_pe)}")
        x_pe[c] = v
        if x_inj is not None:
            v = np.asarray(inj_values[p], dtype=np.float64)
            if v.shape != (n_inj,):
                raise ValueError(f"inj_values[{p!r}] has shape {v.shape}, the engine's injection set {(n_inj,)}")
            x_inj[c] = v
    if not np.all(np.isfinite(x_pe)) or (x_inj is not None and not np.all(np.isfinite(x_inj))):
        raise ValueError("the quantities must be finite")
    return names, x_pe, x_inj


def _mass_cut_masks(pedata, injdata, m1min, m2min, mmax):
    """``(pe_mask, inj_mask)`` of the mass cuts when all three are given and both data dictionaries are at hand, else ``(None,
    None)``: the mask the engine holds stays."""
    from . import draws as D

    cuts = (m1min, m2min, mmax)
    if pedata is not None and injdata is not None and all(c is not None for c in cuts):
        return D.mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    if any(c is not None for c in cuts) and not all(c is not None for c in cuts):
        raise ValueError("m1min, m2min and mmax are given together or not at all")
    return None, None


def event_credible_intervals(eng, thetas, pe_values, levels=(0.05, 0.5, 0.95), inj_values=None, pedata=None, injdata=None, param_names=None, m1min=None, m2min=None,
                             mmax=None, backend="device", return_weights=False, point_weights=None, leave_one_out=False, total_inj=None, nobs=None,
                             marginalize_selection=False):
    """Credible intervals of the population-informed posterior of every event, marginalised over K posterior hyper-parameter draws:
    per event and quantity the weighted quantiles of ``levels`` (rule "inverted CDF": the value of a sample, never an interpolation),
    the mean and the standard deviation under the marginal posterior weight ``W_i = sum_k w_ki / S_k`` of the event's samples,
    ``w_i = p(x_i | theta_k) / prior_i`` -- the table population papers print for ``m1``, ``q`` and ``chi_eff`` -- and the same for the
    predicted detected distribution from the injections.  On the device (``eng.marginal_weights_add``, ``eng.weighted_quantiles``)
    the weights never leave HBM; only sample indices and two sums per quantity come back.

    ``thetas`` is ``(K, n_theta)`` in the engine's layout.  ``pe_values`` maps a name to the ``(n_ev, n_pe)`` array of the quantity
    (any derived quantity, e.g. ``m2 = q * m1``), ``inj_values`` the same names to ``(n_inj,)`` arrays (``None``: no predicted
    distribution); with ``pe_values=None`` the quantities are read from ``pedata`` / ``injdata`` by ``param_names``.  ``param_names``
    selects and orders the names (default: the keys of ``pe_values``; at most 8).  The mass cuts are
    :func:`reweighted_event_posteriors`': with all of ``m1min, m2min, mmax`` given and both data dictionaries at hand they become
    the engine's draw mask, otherwise the mask the engine holds stays.  The device backend resets the engine's marginal weights
    first.  ``backend="host"`` runs the NumPy statement (:func:`gwinferno_amd.draws.marginal_weights_reference`,
    :func:`gwinferno_amd.draws.weighted_quantiles_reference`) on ``eng.log_weights`` under the masks given here (none without the
    cuts): the statement the kernels are tested against, not a fall-back.

    Returns a dict: ``names``; ``levels``; ``quantiles (n_ev, C, Q)``, ``mean`` and ``sd (n_ev, C)``; ``dead (n_ev,)``, the points at
    which the event had no weight; ``n_points``; with ``inj_values`` also ``quantiles_inj (C, Q)``, ``mean_inj``, ``sd_inj (C,)``
    and ``dead_inj``; with ``return_weights=True`` also ``weights`` and ``weights_inj``, the ``W`` arrays.  A segment without weight
    gives NaN.

    ``point_weights``, ``leave_one_out``, ``total_inj``, ``nobs`` and ``marginalize_selection`` are
    :func:`reweighted_event_posteriors`': ``W_i = sum_k v_k w_ki / S_k``; with them the dict also holds ``point_weight_sum (n_ev +
    1,)`` and, for ``leave_one_out=True``, ``elpd_loo`` and ``neff_points``.  The defaults leave every output as it was."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or not 1 <= levels.size <= 32:
        raise ValueError("between 1 and 32 levels can be asked for in one query")
    if not np.all((levels >= 0.0) & (levels <= 1.0)):
        raise ValueError("levels must lie in [0, 1]")
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    if backend == "device" and masks[0] is not None:
        eng.set_draw_mask(*masks)
    n_cols, n_q, n_ev = len(names), levels.size, eng.n_ev
    v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    weighted = {} if v is None else {"point_weights": v}
    if backend == "device":
        eng.set_quantile_columns(x_pe, x_inj)
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas, **weighted)
        idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(levels)
        w_pe, w_inj, dead, n_points = eng.marginal_weights(weights=return_weights)
        vsum = eng.marginal_point_weights()[0] if v is not None else None
    else:
        lw = [eng.log_weights(th) for th in thetas]
        w_pe, w_inj, dead, n_points, *sums = D.marginal_weights_reference(np.stack([a for a, _ in lw]), np.stack([b for _, b in lw]), masks[0], masks[1], v=v)
        vsum = sums[0] if v is not None else None
        idx_pe, mom_pe, mass = np.full((n_ev, n_cols, n_q), -1, dtype=np.int32), np.zeros((n_ev, n_cols, 2)), np.zeros(n_ev + 1)
        idx_inj, mom_inj = (np.full((n_cols, n_q), -1, dtype=np.int32), np.zeros((n_cols, 2))) if x_inj is not None else (None, None)
        for c in range(n_cols):
            for ev in range(n_ev):
                idx_pe[ev, c], mom_pe[ev, c], mass[ev] = D.weighted_quantiles_reference(w_pe[ev], np.argsort(x_pe[c, ev], kind="stable"), x_pe[c, ev], levels)
            if x_inj is not None:
                idx_inj[c], mom_inj[c], mass[n_ev] = D.weighted_quantiles_reference(w_inj, np.argsort(x_inj[c], kind="stable"), x_inj[c], levels)

    def summary(idx, values, mom, m):
        """values (..., C, n) looked up at idx (..., C, Q); the mean and sd from the two sums and the mass m (...)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(idx >= 0, np.take_along_axis(values, np.maximum(idx, 0).astype(np.int64), axis=-1), np.nan)
            mean = mom[..., 0] / m[..., None]
            sd = np.sqrt(np.maximum(mom[..., 1] / m[..., None] - mean * mean, 0.0))
        nothing = ~(m > 0.0)
        mean[nothing], sd[nothing] = np.nan, np.nan
        return q, mean, sd

    out = {"names": names, "levels": levels, "n_points": n_points, "dead": np.asarray(dead[:n_ev]).copy()}
    _point_weight_entries(out, loo, vsum)
    out["quantiles"], out["mean"], out["sd"] = summary(idx_pe, np.moveaxis(x_pe, 0, 1), mom_pe, mass[:n_ev])
    if x_inj is not None:
        out["quantiles_inj"], out["mean_inj"], out["sd_inj"] = summary(idx_inj, x_inj, mom_inj, mass[n_ev : n_ev + 1].reshape(()))
        out["dead_inj"] = int(dead[n_ev])
    if return_weights:
        out["weights"], out["weights_inj"] = w_pe, w_inj
    return out


def event_posterior_densities(eng, thetas, pe_values, grid, pairs=None, grid2d=None, inj_values=None, bounds=None, rule="scott", scale=1.0, pedata=None, injdata=None,
                              param_names=None, m1min=None, m2min=None, mmax=None, backend="device", accumulate=True, point_weights=None, leave_one_out=False, total_inj=None,
                              nobs=None, marginalize_selection=False):
    """Smooth densities of the population-informed posterior of every event, marginalised over K posterior hyper-parameter draws: per
    event and quantity a weighted Gaussian kernel density estimate of the marginal posterior weights ``W_i = sum_k w_ki / S_k`` on
    the points of ``grid`` (the curves of a ridge or violin plot), per pair of quantities the same in two dimensions on a tensor grid
    (the map behind joint contours), and both for the predicted detected distribution from the injections.  The bandwidth rules are
    scipy.stats.gaussian_kde(weights=...)'s.  On the device (``eng.weighted_kde``, ``eng.weighted_kde2d``) the weights
    never leave HBM; only the curves come back.

    ``thetas``, ``pe_values`` / ``inj_values`` (or ``pedata`` / ``injdata`` with ``param_names``), the mass cuts and the masks are
    :func:`event_credible_intervals`'.  ``grid`` maps a name to its ``(G,)`` points, or is one ``(G,)`` or ``(C, G)`` array (all
    columns need the same G <= 1024).  ``pairs`` lists up to 4 pairs of names (or column indices) and ``grid2d = (gridx, gridy)``
    gives their axes, ``(n,)`` or ``(n_pairs, n)`` with n <= 128.  ``bounds`` maps a name to reflecting bounds ``(lo, hi)`` of its 1-D
    curve (``None`` for an open side); there is no reflection in 2-D.  ``rule`` is ``"scott"`` or ``"silverman"``, ``scale``
    multiplies the factor.  ``accumulate=False`` leaves the engine's marginal weights as they are -- those a preceding
    :func:`event_credible_intervals` call on the same ``thetas`` left, so that the table and the figure cost one pass over the
    points -- and sets no mask.  ``backend="host"`` runs the NumPy statement (:func:`gwinferno_amd.draws.weighted_kde_reference`,
    :func:`gwinferno_amd.draws.weighted_kde2d_reference`) on ``eng.marginal_weights()``: the statement the kernels are tested
    against, not a fall-back.

    Returns a dict: ``names``, ``grid (C, G)``, ``density (n_ev, C, G)``, ``bandwidth (n_ev, C)``, ``neff (n_ev,)``, ``degenerate
    (n_ev, C)``, ``dead (n_ev,)`` (the points at which the event had no weight) and ``n_points``; with ``inj_values`` also
    ``density_inj (C, G)``, ``bandwidth_inj``, ``neff_inj``, ``degenerate_inj`` and ``dead_inj``; with ``pairs`` also ``pairs``
    (column indices), ``density2d (n_ev, P, n_gx, n_gy)``, ``covariance (n_ev, P, 3)`` (``Hxx, Hxy, Hyy``), ``degenerate2d`` and their
    ``_inj`` counterparts.  A segment without a curve gives NaN.

    ``point_weights``, ``leave_one_out``, ``total_inj``, ``nobs`` and ``marginalize_selection`` are
    :func:`reweighted_event_posteriors`' and apply to the accumulation: with ``accumulate=False`` the weights the engine holds are
    reused whatever they were made with.  With them the dict also holds ``point_weight_sum (n_ev + 1,)`` (the engine's sum of the
    weights) and, for ``leave_one_out=True``, ``elpd_loo`` and ``neff_points``.  The defaults leave every output as it was."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    if thetas.shape[0] < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    D.kde_factor(1.0, 1, rule, scale)  # (checks both)
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    n_cols, n_ev = len(names), eng.n_ev
    grid = np.stack([np.asarray(grid[p], dtype=np.float64) for p in names]) if isinstance(grid, dict) else np.asarray(grid, dtype=np.float64)
    if grid.ndim not in (1, 2) or (grid.ndim == 2 and grid.shape[0] != n_cols) or not 1 <= grid.shape[-1] <= 1024:
        raise ValueError(f"grid has shape {grid.shape}; expected (G,) or ({n_cols}, G) with 1 <= G <= 1024")
    grid = np.ascontiguousarray(np.broadcast_to(grid, (n_cols, grid.shape[-1])))
    if not np.all(np.isfinite(grid)):
        raise ValueError("grid points must be finite")
    b = np.full((n_cols, 2), np.nan)
    for p, pair in (bounds or {}).items():
        if p not in names:
            raise ValueError(f"bounds name {p!r}, which is not one of the quantities")
        b[names.index(p)] = [np.nan if v is None else float(v) for v in pair]
    pair_idx = None
    if pairs is not None:
        if grid2d is None:
            raise ValueError("pairs need grid2d = (gridx, gridy)")
        pair_idx = np.array([[names.index(v) if isinstance(v, str) else int(v) for v in pair] for pair in pairs], dtype=np.int32).reshape(-1, 2)
        if not 1 <= pair_idx.shape[0] <= 4 or np.any(pair_idx < 0) or np.any(pair_idx >= n_cols):
            raise ValueError("between 1 and 4 pairs of the quantities can be asked for in one query")
        gridx, gridy = (np.ascontiguousarray(np.broadcast_to(np.asarray(g, dtype=np.float64), (pair_idx.shape[0], np.shape(g)[-1]))) for g in grid2d)
        if not (1 <= gridx.shape[1] <= 128 and 1 <= gridy.shape[1] <= 128) or not (np.all(np.isfinite(gridx)) and np.all(np.isfinite(gridy))):
            raise ValueError("grid2d holds one to 128 finite points per axis")
    v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    weighted = {} if v is None else {"point_weights": v}
    if accumulate:
        masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas, **weighted)
    n_segs = n_ev + 1
    if backend == "device":
        eng.set_kde_columns(x_pe, x_inj, b)
        rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid, rule, scale)
        if pair_idx is not None:
            rho2_pe, rho2_inj, cov, _, flags2 = eng.weighted_kde2d(pair_idx, gridx, gridy, rule, scale)
        _, _, dead, n_points = eng.marginal_weights(weights=False)
    else:
        w_pe, w_inj, dead, n_points = eng.marginal_weights()
        g = grid.shape[1]
        rho_pe, rho_inj = np.full((n_ev, n_cols, g), np.nan), (np.full((n_cols, g), np.nan) if x_inj is not None else None)
        bw, neff, flags = np.full((n_segs, n_cols), np.nan), np.zeros(n_segs), np.zeros((n_segs, n_cols), dtype=np.int32)
        for c in range(n_cols):
            for ev in range(n_ev):
                rho_pe[ev, c], bw[ev, c], neff[ev], flags[ev, c] = D.weighted_kde_reference(w_pe[ev], x_pe[c, ev], grid[c], rule, scale, b[c])
            if x_inj is not None:
                rho_inj[c], bw[n_ev, c], neff[n_ev], flags[n_ev, c] = D.weighted_kde_reference(w_inj, x_inj[c], grid[c], rule, scale, b[c])
        if pair_idx is not None:
            n_p, shape = pair_idx.shape[0], (gridx.shape[1], gridy.shape[1])
            rho2_pe, rho2_inj = np.full((n_ev, n_p) + shape, np.nan), (np.full((n_p,) + shape, np.nan) if x_inj is not None else None)
            cov, flags2 = np.full((n_segs, n_p, 3), np.nan), np.zeros((n_segs, n_p), dtype=np.int32)
            for t, (cx, cy) in enumerate(pair_idx):
                for ev in range(n_ev):
                    rho2_pe[ev, t], cov[ev, t], _, flags2[ev, t] = D.weighted_kde2d_reference(w_pe[ev], x_pe[cx, ev], x_pe[cy, ev], gridx[t], gridy[t], rule, scale)
                if x_inj is not None:
                    rho2_inj[t], cov[n_ev, t], _, flags2[n_ev, t] = D.weighted_kde2d_reference(w_inj, x_inj[cx], x_inj[cy], gridx[t], gridy[t], rule, scale)
    out = {"names": names, "grid": grid, "n_points": n_points, "dead": np.asarray(dead[:n_ev]).copy(), "density": rho_pe, "bandwidth": bw[:n_ev], "neff": neff[:n_ev],
           "degenerate": flags[:n_ev]}
    _point_weight_entries(out, loo, eng.marginal_point_weights()[0] if v is not None else None)
    if x_inj is not None:
        out.update(density_inj=rho_inj, bandwidth_inj=bw[n_ev], neff_inj=float(neff[n_ev]), degenerate_inj=flags[n_ev], dead_inj=int(dead[n_ev]))
    if pair_idx is not None:
        out.update(pairs=pair_idx, grid2d=(gridx, gridy), density2d=rho2_pe, covariance=cov[:n_ev], degenerate2d=flags2[:n_ev])
        if x_inj is not None:
            out.update(density2d_inj=rho2_inj, covariance_inj=cov[n_ev], degenerate2d_inj=flags2[n_ev])
    return out


def catalog_predictive_check(eng, thetas, pe_values, grid, inj_values=None, levels=(0.05, 0.5, 0.95), n_obs=None, point_weights=None, pedata=None, injdata=None,
                             param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """Catalog-level predictive checks over K posterior hyper-parameter draws: per quantity the cumulative distribution of
    the predicted detected population (from the injections) and the catalog's own population-informed one (the mean over the events
    of their CDFs), each as percentile bands over the draws, and the extreme-event test -- the CDF of the catalog's largest value,
    ``P(max_e x_e <= g | theta_k) = prod_e F_ke(g)``, and of its smallest, ``1 - prod_e (1 - F_ke(g))``, against those of a predicted
    catalog of ``n_obs`` detections, ``F_det,k(g)^n_obs`` and ``1 - (1 - F_det,k(g))^n_obs``.  Bands and products are not linear in
    the per-point distributions, so on the device (``eng.point_cdfs``) the curves of every point come back, ``4 C G`` doubles per
    point, and the weights never leave HBM.  A CDF at a grid point is an exact partition sum: it has no bin-width error.

    ``thetas`` is ``(K, n_theta)`` in the engine's layout.  ``pe_values`` / ``inj_values`` (or ``pedata`` / ``injdata`` with
    ``param_names``), the mass cuts and the masks are :func:`event_credible_intervals`'; without ``inj_values`` there is no predicted
    side (NaN).  ``grid`` maps a name to its strictly increasing ``(G,)`` points, or is one ``(G,)`` or ``(C, G)`` array; ``1 <= G
    <= 256``, the same for every quantity.  The device backend replaces the engine's histogram bins with the grid's cumulative
    codes (:func:`gwinferno_amd.draws.cdf_codes`).  ``n_obs`` is the size of the predicted catalog (default ``eng.n_ev``).
    ``point_weights (K,)`` -- finite, non-negative, not all 0; default equal -- weight the points in the bands (rule "inverted CDF",
    :func:`gwinferno_amd.draws.weighted_percentiles`) and in the means; they are applied here, to ``K C G`` numbers, and never go to
    the device.  With ``leave_one_out_weights(...)["point_weights"][:, e]`` the points stand for ``p(theta | all events but e)``:
    comparing event e's values with ``cdf_max_predicted`` (or ``cdf_min_predicted``) is then the leave-one-out outlier test of event
    e, whose own data no longer shapes the population it is held against.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.point_cdfs_reference`) on ``eng.log_weights`` under the masks given here (none without the cuts):
    the statement the kernels are tested against, not a fall-back.

    Returns a dict: ``names``; ``grid (C, G)``; ``levels``; the raw per-point arrays ``cdf_detected``, ``cdf_observed``,
    ``log_cdf_max_observed`` and ``log_sf_min_observed``, each ``(K, C, G)`` (``log_sf_min`` is the log of ``P(min > g)``);
    ``log_cdf_max_predicted = n_obs log cdf_detected`` and ``log_sf_min_predicted = n_obs log1p(-cdf_detected)``; ``bands_detected``
    and ``bands_observed (Q, C, G)``; ``cdf_max_observed``, ``cdf_max_predicted``, ``cdf_min_observed`` and ``cdf_min_predicted (C,
    G)``, the weighted means over the points of the exponentiated quantities, a point without a live event (observed) or without
    injection weight (predicted) left out; ``n_live (K,)``, the live events per point; ``dead_detected``, the points at which the
    injection set had no weight; ``n_points``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size < 1 or not np.all((levels >= 0.0) & (levels <= 1.0)):
        raise ValueError("levels must be numbers in [0, 1]")
    source = pe_values if pe_values is not None else pedata
    for p in param_names if param_names is not None and source is not None else ():
        if p not in source:
            raise ValueError(f"unknown quantity {p!r}")
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    n_cols, n_ev = len(names), eng.n_ev
    if isinstance(grid, dict):
        missing = [p for p in names if p not in grid]
        if missing:
            raise ValueError(f"grid names no points for {missing}")
        if len({np.size(grid[p]) for p in names}) != 1:
            raise ValueError("every quantity needs the same number of grid points")
        grid = np.stack([np.asarray(grid[p], dtype=np.float64).ravel() for p in names])
    else:
        grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim not in (1, 2) or (grid.ndim == 2 and grid.shape[0] != n_cols) or not 1 <= grid.shape[-1] <= D.MAX_CDF_GRID:
        raise ValueError(f"grid has shape {grid.shape}; expected (G,) or ({n_cols}, G) with 1 <= G <= {D.MAX_CDF_GRID}")
    grid = np.ascontiguousarray(np.broadcast_to(grid, (n_cols, grid.shape[-1])))
    n_grid = grid.shape[1]
    n_obs = float(n_ev if n_obs is None else n_obs)
    if not (n_obs > 0.0 and np.isfinite(n_obs)):
        raise ValueError("n_obs must be a positive number")
    if point_weights is None:
        v = np.ones(k)
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape != (k,) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.any(v > 0.0):
            raise ValueError(f"point_weights are ({k},) finite non-negative numbers, not all 0")
    pe_codes = np.stack([D.cdf_codes(x_pe[c], grid[c]) for c in range(n_cols)])
    inj_codes = np.stack([D.cdf_codes(x_inj[c], grid[c]) for c in range(n_cols)]) if x_inj is not None else None
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_histogram_bins(pe_codes, inj_codes, n_bins=n_grid)
        out, live = eng.point_cdfs(thetas)
    else:
        out, live = np.empty((k, 4, n_cols, n_grid)), np.empty((k, 2), dtype=np.int32)
        for i, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            out[i], live[i] = D.point_cdfs_reference(lw_pe, lw_inj, masks[0], masks[1], pe_codes, inj_codes, n_grid)
    det, obs, below, above = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        below_pred, above_pred = n_obs * np.log(det), n_obs * np.log1p(-np.minimum(det, 1.0))

    def mean(values, keep):
        """the weighted mean over the points of ``keep``; NaN where none has weight"""
        w = np.where(keep, v, 0.0)
        total = w.sum()
        if not total > 0.0:
            return np.full(values.shape[1:], np.nan)
        return np.tensordot(w, np.where(keep[:, None, None], values, 0.0), axes=1) / total

    has_obs, has_det = live[:, 0] > 0, live[:, 1] > 0
    return {"names": names, "grid": grid, "levels": levels, "cdf_detected": det, "cdf_observed": obs, "log_cdf_max_observed": below, "log_sf_min_observed": above,
            "log_cdf_max_predicted": below_pred, "log_sf_min_predicted": above_pred,
            "bands_detected": D.weighted_percentiles(det, v, levels), "bands_observed": D.weighted_percentiles(obs, v, levels),
            "cdf_max_observed": mean(np.exp(below), has_obs), "cdf_max_predicted": mean(np.exp(below_pred), has_det),
            "cdf_min_observed": mean(-np.expm1(above), has_obs), "cdf_min_predicted": mean(-np.expm1(above_pred), has_det),
            "n_live": live[:, 0].astype(np.int64), "dead_detected": int(np.count_nonzero(~has_det)) if x_inj is not None else k, "n_points": k}


def _ks_uniform(u):
    """The Kolmogorov distance of the sample ``u`` (no NaN) from the uniform distribution on [0, 1]: ``max_i max(i / n - u_(i), u_(i) -
    (i - 1) / n)`` over the sorted sample; NaN for an empty one."""
    u = np.sort(np.asarray(u, dtype=np.float64).ravel())
    n = u.size
    if n == 0:
        return np.nan
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - u), np.max(u - (i - 1.0) / n)))


def event_calibration(eng, thetas, pe_values, grid, inj_values=None, point_weights=None, leave_one_out=False, total_inj=None, nobs=None, marginalize_selection=False,
                      pedata=None, injdata=None, param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """Per-event calibration over K posterior hyper-parameter draws: the probability integral transform (PIT) of every event
    under the predicted detected distribution, ``PIT_kec = sum_i (w_ki / S_ke) F_det,k(x_i)``, averaged over the draws -- what a P-P plot
    is made of: flat when the population model describes the catalog, bent where it does not -- and with ``leave_one_out=True`` its
    leave-one-out form, LOO-PIT, in which event e is held against the population fitted without it.  The PIT is a product of the
    event's weights and the injection set's CDF at the same point, so on the device (``eng.point_pits``) a rigorous bracket ``[pit_lo,
    pit_hi]`` per (point, event, quantity) comes back, ``2 n_ev C + C G`` doubles per point, and the weights never leave HBM.  The
    bracket's width is the grid's resolution alone (at most the largest step of ``F_det`` between neighbouring grid points, plus the
    event's share above the grid); a finer grid narrows it.

    ``thetas`` is ``(K, n_theta)`` in the engine's layout.  ``pe_values`` / ``inj_values`` (or ``pedata`` / ``injdata`` with
    ``param_names``), ``grid``, the mass cuts and the masks are :func:`catalog_predictive_check`'s; the injections' values are needed.
    The device backend replaces the engine's histogram bins with the grid's cumulative codes.  The weights on the k axis are applied
    here, on the host: equal by default, ``point_weights (K,)`` or ``(K, n_ev + 1)`` (numbers in ``[0, 1]``; the last column is not
    used), or with ``leave_one_out=True`` those of :func:`leave_one_out_weights` (``total_inj`` is needed; ``nobs`` and
    ``marginalize_selection`` as there).  A (point, event) at which the event or the injection set has no weight is skipped and
    counted in ``n_dead``.  ``backend="host"`` runs the NumPy statement (:func:`gwinferno_amd.draws.point_pits_reference`) on
    ``eng.log_weights`` under the masks given here (none without the cuts): the statement the kernel is tested against, not a fall-back.

    Returns a dict: ``names``; ``grid (C, G)``; ``pit_lo``, ``pit_hi``, ``pit`` (the midpoint) and ``width``, each ``(n_ev, C)``, the
    weighted means over the points (NaN for an event without a live point of positive weight); ``neff_points (n_ev,)``, ``(sum_k v)^2
    / sum_k v^2`` over the points that count; ``n_dead (n_ev,)``; the sorted P-P curves ``pp_levels (n,) = (1 ... n) / n``, ``pp_lo``,
    ``pp_hi`` and ``pp (C, n)`` over the ``n`` events that have a PIT; ``ks_lo``, ``ks_hi`` and ``ks (C,)``, the Kolmogorov distance
    from uniform of the lower, upper and midpoint PITs; the raw per-point arrays ``point_pits (K, n_ev, C, 2)``, ``cdf_detected (K, C,
    G)`` and ``dead (K, n_ev + 1)``; ``n_points``; with ``leave_one_out=True`` also ``elpd_loo (n_ev,)``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    source = pe_values if pe_values is not None else pedata
    for p in param_names if param_names is not None and source is not None else ():
        if p not in source:
            raise ValueError(f"unknown quantity {p!r}")
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    if x_inj is None:
        raise ValueError("the PIT is taken under the predicted detected distribution: inj_values (or injdata) are needed")
    n_cols, n_ev = len(names), eng.n_ev
    if isinstance(grid, dict):
        missing = [p for p in names if p not in grid]
        if missing:
            raise ValueError(f"grid names no points for {missing}")
        if len({np.size(grid[p]) for p in names}) != 1:
            raise ValueError("every quantity needs the same number of grid points")
        grid = np.stack([np.asarray(grid[p], dtype=np.float64).ravel() for p in names])
    else:
        grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim not in (1, 2) or (grid.ndim == 2 and grid.shape[0] != n_cols) or not 1 <= grid.shape[-1] <= D.MAX_CDF_GRID:
        raise ValueError(f"grid has shape {grid.shape}; expected (G,) or ({n_cols}, G) with 1 <= G <= {D.MAX_CDF_GRID}")
    grid = np.ascontiguousarray(np.broadcast_to(grid, (n_cols, grid.shape[-1])))
    n_grid = grid.shape[1]
    pe_codes = np.stack([D.cdf_codes(x_pe[c], grid[c]) for c in range(n_cols)])
    inj_codes = np.stack([D.cdf_codes(x_inj[c], grid[c]) for c in range(n_cols)])
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    v = np.ones((k, n_ev)) if v is None else np.asarray(v, dtype=np.float64)[:, :n_ev]
    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_histogram_bins(pe_codes, inj_codes, n_bins=n_grid)
        raw, det, dead = eng.point_pits(thetas)
    else:
        raw, det, dead = np.empty((k, n_ev, n_cols, 2)), np.empty((k, n_cols, n_grid)), np.empty((k, n_ev + 1), dtype=np.int32)
        for i, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            raw[i], det[i], dead[i] = D.point_pits_reference(lw_pe, lw_inj, masks[0], masks[1], pe_codes, inj_codes, n_grid)
    gone = (dead[:, :n_ev] != 0) | (dead[:, n_ev:] != 0)  # (K, n_ev): the event or the injection set has no weight at the point
    w = np.where(gone, 0.0, v)
    wsum, wsq = w.sum(axis=0), (w * w).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (w[:, :, None, None] * np.where(gone[:, :, None, None], 0.0, raw)).sum(axis=0) / wsum[:, None, None]  # (n_ev, C, 2); NaN without weight
        neff = np.where(wsum > 0.0, wsum * wsum / wsq, 0.0)
    lo, hi = mean[..., 0], mean[..., 1]
    mid = 0.5 * (lo + hi)
    has = wsum > 0.0
    n_has = int(np.count_nonzero(has))
    curves = [np.sort(a[has], axis=0).T.reshape(n_cols, n_has) for a in (lo, hi, mid)]
    out = {"names": names, "grid": grid, "pit_lo": lo, "pit_hi": hi, "pit": mid, "width": hi - lo, "neff_points": neff, "n_dead": gone.sum(axis=0).astype(np.int64),
           "pp_levels": np.arange(1, n_has + 1, dtype=np.float64) / max(n_has, 1), "pp_lo": curves[0], "pp_hi": curves[1], "pp": curves[2],
           "ks_lo": np.array([_ks_uniform(c) for c in curves[0]]), "ks_hi": np.array([_ks_uniform(c) for c in curves[1]]),
           "ks": np.array([_ks_uniform(c) for c in curves[2]]), "point_pits": raw, "cdf_detected": det, "dead": dead, "n_points": k}
    if loo is not None:
        out["elpd_loo"] = loo["elpd_loo"]
    return out


def pareto_smoothed_loo_weights(eng, thetas, total_inj, nobs=None, marginalize_selection=False):
    """:func:`leave_one_out_weights` with every event's weights Pareto-smoothed on the point axis (Vehtari et al., *Pareto
    smoothed importance sampling*; :func:`gwinferno_amd.draws.pareto_smooth`): the raw weights ``exp(-l_ke)`` have a heavy right tail
    when a single point explains event e badly, and the largest ``M = min(K / 5, 3 sqrt K)`` of them are replaced by the quantiles of
    a generalised Pareto distribution fitted to them.  Takes what :func:`leave_one_out_weights` takes and returns the same dictionary
    with ``point_weights (K, n_ev + 1)`` the smoothed weights -- each event's largest exactly 1, the injection column all ones, every
    entry in ``[0, 1]``: they go straight into the ``point_weights=`` arguments of the weighted entries -- ``pareto_k (n_ev,)``, the
    fitted shape (below 0.5 good, up to 0.7 usable, above it unreliable; inf where fewer than 25 points leave no tail to fit; nothing
    is refitted), and ``elpd_loo`` and ``neff_points`` recomputed from the smoothed weights."""
    from .draws import pareto_smoothed_summary

    return pareto_smoothed_summary(leave_one_out_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)["log_l_event"])


def event_calibration_exact(eng, thetas, pe_values, inj_values=None, point_weights=None, leave_one_out=False, total_inj=None, nobs=None, marginalize_selection=False,
                            pedata=None, injdata=None, param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """:func:`event_calibration` without a grid: the un-gridded probability integral transform of every event under the
    predicted detected distribution, ``PIT_kec = sum_i (w_ki / S_ke) F_det,k(x_i)`` with ``F_det`` the weighted rank of the sample
    among the injections, averaged over the draws.  On the device (``eng.point_pits_exact``) ``2 n_ev C`` doubles come back per point
    and the weights never leave HBM; no bracket is left to the resolution of a grid, and values that tie between the two sets are
    treated exactly: ``pit_le`` counts the injections with ``x_inj <= x``, ``pit_lt`` those with ``x_inj < x``, and ``pit``, their
    midpoint, is the expectation of the randomised PIT.

    The arguments are :func:`event_calibration`'s without ``grid``.  The device backend replaces the engine's rank columns
    (``eng.set_rank_columns``).  ``leave_one_out="psis"`` takes the weights of :func:`pareto_smoothed_loo_weights` -- with the exact
    PIT, what ArviZ calls ``loo_pit`` -- and ``leave_one_out=True`` the raw ones.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.point_pits_exact_reference`) on ``eng.log_weights``: the statement the kernels are tested against, not
    a fall-back.

    Returns a dict: ``names``; ``pit_lt``, ``pit_le`` and ``pit``, each ``(n_ev, C)``, the weighted means over the points (NaN for an
    event without a live point of positive weight); ``neff_points (n_ev,)``; ``n_dead (n_ev,)``, the (point, event) pairs skipped
    because the event or the injection set had no weight; the sorted P-P curves ``pp_levels (n,)``, ``pp_lt``, ``pp_le`` and ``pp (C,
    n)``; the Kolmogorov distances ``ks_lt``, ``ks_le`` and ``ks (C,)``; the raw ``point_pits (K, n_ev, C, 2)`` and ``dead (K, n_ev +
    1)``; ``n_points``; with leave-one-out weights ``elpd_loo (n_ev,)``, and with ``"psis"`` also ``pareto_k (n_ev,)``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    if not (isinstance(leave_one_out, bool) or leave_one_out == "psis"):
        raise ValueError(f"leave_one_out must be False, True or 'psis', not {leave_one_out!r}")
    source = pe_values if pe_values is not None else pedata
    for p in param_names if param_names is not None and source is not None else ():
        if p not in source:
            raise ValueError(f"unknown quantity {p!r}")
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    if x_inj is None:
        raise ValueError("the PIT is taken under the predicted detected distribution: inj_values (or injdata) are needed")
    n_cols, n_ev = len(names), eng.n_ev
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    if leave_one_out == "psis":
        if point_weights is not None:
            raise ValueError("leave_one_out='psis' makes the point weights itself: point_weights must be None")
        if total_inj is None:
            raise ValueError("leave_one_out='psis' needs total_inj")
        loo = pareto_smoothed_loo_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)
        v = loo["point_weights"]
    else:
        v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    v = np.ones((k, n_ev)) if v is None else np.asarray(v, dtype=np.float64)[:, :n_ev]
    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_rank_columns(x_pe, x_inj)
        raw, dead = eng.point_pits_exact(thetas)
    else:
        order, lt, le = D.rank_codes(x_pe, x_inj)
        raw, dead = np.empty((k, n_ev, n_cols, 2)), np.empty((k, n_ev + 1), dtype=np.int32)
        for i, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            raw[i], dead[i] = D.point_pits_exact_reference(lw_pe, lw_inj, masks[0], masks[1], order, lt, le)
    gone = (dead[:, :n_ev] != 0) | (dead[:, n_ev:] != 0)  # (K, n_ev): the event or the injection set has no weight at the point
    w = np.where(gone, 0.0, v)
    wsum, wsq = w.sum(axis=0), (w * w).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (w[:, :, None, None] * np.where(gone[:, :, None, None], 0.0, raw)).sum(axis=0) / wsum[:, None, None]  # (n_ev, C, 2); NaN without weight
        neff = np.where(wsum > 0.0, wsum * wsum / wsq, 0.0)
    lt_mean, le_mean = mean[..., 0], mean[..., 1]
    mid = 0.5 * (lt_mean + le_mean)
    has = wsum > 0.0
    n_has = int(np.count_nonzero(has))
    curves = [np.sort(a[has], axis=0).T.reshape(n_cols, n_has) for a in (lt_mean, le_mean, mid)]
    out = {"names": names, "pit_lt": lt_mean, "pit_le": le_mean, "pit": mid, "neff_points": neff, "n_dead": gone.sum(axis=0).astype(np.int64),
           "pp_levels": np.arange(1, n_has + 1, dtype=np.float64) / max(n_has, 1), "pp_lt": curves[0], "pp_le": curves[1], "pp": curves[2],
           "ks_lt": np.array([_ks_uniform(c) for c in curves[0]]), "ks_le": np.array([_ks_uniform(c) for c in curves[1]]),
           "ks": np.array([_ks_uniform(c) for c in curves[2]]), "point_pits": raw, "dead": dead, "n_points": k}
    if loo is not None:
        out["elpd_loo"] = loo["elpd_loo"]
        if "pareto_k" in loo:
            out["pareto_k"] = loo["pareto_k"]
    return out


def _moment_points(eng, thetas, x_pe, x_inj, masks, backend):
    """``(mean (K, n_ev + 1, C), cov (K, n_ev + 1, C, C), dead (K, n_ev + 1))`` of the points on either backend."""
    from . import draws as D

    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_kde_columns(x_pe, x_inj)
        return eng.point_moments(thetas)
    k, n_cols, n_segs = thetas.shape[0], x_pe.shape[0], eng.n_ev + 1
    mean, cov, dead = np.empty((k, n_segs, n_cols)), np.empty((k, n_segs, n_cols, n_cols)), np.empty((k, n_segs), dtype=np.int32)
    for i, th in enumerate(thetas):
        lw_pe, lw_inj = eng.log_weights(th)
        mean[i], cov[i], dead[i] = D.point_moments_reference(lw_pe, lw_inj, x_pe, x_inj, masks[0], masks[1])
    return mean, cov, dead


def _checked_names(pe_values, pedata, param_names):
    source = pe_values if pe_values is not None else pedata
    for p in param_names if param_names is not None and source is not None else ():
        if p not in source:
            raise ValueError(f"unknown quantity {p!r}")


def catalog_correlation_check(eng, thetas, pe_values, inj_values=None, pairs=None, levels=(0.05, 0.5, 0.95), point_weights=None, pedata=None, injdata=None,
                              param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """Does the catalog's correlation between two quantities agree with the one the fitted population predicts for detected sources?
      Every model the engine evaluates is a product of one-dimensional densities, and the checks of one coordinate at a
    time cannot see a correlation the data demand.  Per hyper-posterior point k the observed catalog is the equal-weight mixture of its
    live events' population-informed posteriors, with mean and covariance

    ``mu_obs = mean_e m_ke``        ``Sigma_obs = mean_e [V_ke + (m_ke - mu_obs)(m_ke - mu_obs)^T]``

    from the events' per-point means ``m_ke`` and covariances ``V_ke``; the prediction is the injection segment's ``V_det,k``.  A
    correlation is a ratio of centred second moments and has to be taken point by point: on the device (``eng.point_moments``) ``(n_ev
    + 1)(C + C (C + 1) / 2)`` doubles come back per point and the weights never leave HBM.

    ``thetas`` is ``(K, n_theta)``.  ``pe_values`` / ``inj_values`` (or ``pedata`` / ``injdata`` with ``param_names``), the mass cuts
    and the masks are :func:`catalog_predictive_check`'s; without ``inj_values`` there is no predicted side (NaN).  ``pairs`` holds
    pairs of names or of column indices (default: every pair ``c < d``).  ``point_weights (K,)`` -- finite, non-negative, not all 0;
    default equal -- weight the points in the bands (:func:`gwinferno_amd.draws.weighted_percentiles`) and in the shares; they are
    applied here and never go to the device.  The device backend replaces the engine's KDE columns.  ``backend="host"`` runs the NumPy
    statement (:func:`gwinferno_amd.draws.point_moments_reference`) on ``eng.log_weights``: the statement the kernels are tested
    against, not a fall-back.

    Returns a dict: ``names``; ``pairs (n_pairs, 2)`` column indices; ``levels``; per point and pair ``rho_obs``, ``rho_det`` and
    ``delta = rho_obs - rho_det``, each ``(K, n_pairs)``; ``bands_rho_obs``, ``bands_rho_det`` and ``bands_delta (Q, n_pairs)``;
    ``p_delta_positive (n_pairs,)``, the weighted share of the points with ``delta > 0`` among those where it is a number, and
    ``p_two_sided = 2 min(p, 1 - p)``, the tail probability of "no difference"; the same for the covariances themselves, which need no
    division: ``cov_obs``, ``cov_det``, ``delta_cov``, ``bands_cov_obs``, ``bands_cov_det``, ``bands_delta_cov``,
    ``p_delta_cov_positive`` and ``p_cov_two_sided``.  A correlation is the covariance standardised by the two variances: where a
    variance is 0 within rounding (at most ``(64 * 2^-52 mu)^2``) or not finite nothing is divided, the correlation is NaN and ``degenerate_obs`` / ``degenerate_det
    (K, n_pairs)`` flag it.  Also ``mu_obs (K, C)``, ``sigma_obs (K, C, C)``, ``mu_det``, ``sigma_det``; ``n_live (K,)``, the live
    events per point; ``dead_detected``, the points at which the injection set had no weight; the raw ``point_mean``, ``point_cov``
    and ``dead`` of ``eng.point_moments``; ``n_points``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size < 1 or not np.all((levels >= 0.0) & (levels <= 1.0)):
        raise ValueError("levels must be numbers in [0, 1]")
    _checked_names(pe_values, pedata, param_names)
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    n_cols, n_ev = len(names), eng.n_ev
    if pairs is None:
        pairs = [(c, d) for c in range(n_cols) for d in range(c + 1, n_cols)]
    pairs = [tuple(names.index(p) if isinstance(p, str) else int(p) for p in pair) for pair in pairs]
    if not pairs or any(len(p) != 2 or not all(0 <= c < n_cols for c in p) for p in pairs):
        raise ValueError(f"pairs are pairs of names or of column indices below {n_cols}, at least one")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if point_weights is None:
        v = np.ones(k)
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape != (k,) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.any(v > 0.0):
            raise ValueError(f"point_weights are ({k},) finite non-negative numbers, not all 0")
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    mean, cov, dead = _moment_points(eng, thetas, x_pe, x_inj, masks, backend)
    live = dead[:, :n_ev] == 0                                    # (K, n_ev)
    n_live = live.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = live / n_live[:, None]                            # NaN rows where no event is live
        m = np.where(live[:, :, None], mean[:, :n_ev], 0.0)
        mu_obs = np.einsum("ke,kec->kc", share, m)
        dm = np.where(live[:, :, None], mean[:, :n_ev] - mu_obs[:, None, :], 0.0)
        spread = np.where(live[:, :, None, None], cov[:, :n_ev], 0.0) + dm[:, :, :, None] * dm[:, :, None, :]
        sigma_obs = np.einsum("ke,kecd->kcd", share, spread)
    mu_det, sigma_det = mean[:, n_ev], cov[:, n_ev]

    def standardised(sigma, mu):
        """``(covariance, correlation, flag)`` per point and pair: nothing is divided where a variance is not finite or does not exceed
        ``(64 * 2^-52 |mu|)^2`` -- a constant column's mean carries a rounding of its own, so its centred values are a few ulps of
        the mean, not 0, and a standard deviation of that size is what the arithmetic cannot tell from none"""
        c, d = pairs[:, 0], pairs[:, 1]
        s_cd, s_cc, s_dd = sigma[:, c, d], sigma[:, c, c], sigma[:, d, d]
        floor = (64.0 * 2.0**-52 * np.abs(mu)) ** 2
        with np.errstate(invalid="ignore"):
            ok = (s_cc > floor[:, c]) & (s_dd > floor[:, d]) & np.isfinite(s_cc) & np.isfinite(s_dd)
        rho = np.full(s_cd.shape, np.nan)
        rho[ok] = s_cd[ok] / np.sqrt(s_cc[ok] * s_dd[ok])
        return s_cd, rho, (~ok & ~np.isnan(s_cc) & ~np.isnan(s_dd)).astype(np.int32)

    def shares(delta):
        """the weighted share of the points with delta > 0 among those where delta is a number, and the two-sided tail"""
        has = ~np.isnan(delta)
        den = (v[:, None] * has).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (v[:, None] * (has & (np.where(has, delta, 0.0) > 0.0))).sum(axis=0) / den
        return p, 2.0 * np.minimum(p, 1.0 - p)

    cov_obs, rho_obs, flag_obs = standardised(sigma_obs, mu_obs)
    cov_det, rho_det, flag_det = standardised(sigma_det, mu_det)
    delta, delta_cov = rho_obs - rho_det, cov_obs - cov_det
    p_rho, p_cov = shares(delta), shares(delta_cov)
    out = {"names": names, "pairs": pairs, "levels": levels, "rho_obs": rho_obs, "rho_det": rho_det, "delta": delta, "cov_obs": cov_obs, "cov_det": cov_det,
           "delta_cov": delta_cov, "p_delta_positive": p_rho[0], "p_two_sided": p_rho[1], "p_delta_cov_positive": p_cov[0], "p_cov_two_sided": p_cov[1],
           "degenerate_obs": flag_obs, "degenerate_det": flag_det, "mu_obs": mu_obs, "sigma_obs": sigma_obs, "mu_det": mu_det, "sigma_det": sigma_det,
           "n_live": n_live.astype(np.int64), "dead_detected": int(np.count_nonzero(dead[:, n_ev])) if x_inj is not None else k, "point_mean": mean, "point_cov": cov,
           "dead": dead, "n_points": k}
    for key in ("rho_obs", "rho_det", "delta", "cov_obs", "cov_det", "delta_cov"):
        out["bands_" + key] = D.weighted_percentiles(out[key], v, levels)
    return out


def _rankcorr_points(eng, thetas, x_pe, x_inj, masks, backend):
    """``(total (K, 2), mean_rank (K, 2, C), cov (K, 2, C, C), dead (K, n_ev + 1), dead_set (K, 2))`` of the points on either backend
    (DESIGN 8l)."""
    from . import draws as D

    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_rankcorr_columns(x_pe, x_inj)
        return eng.point_rank_correlations(thetas)
    k, n_cols, n_ev = thetas.shape[0], x_pe.shape[0], eng.n_ev
    codes_obs, codes_det = D.rankcorr_codes(x_pe.reshape(n_cols, -1)), D.rankcorr_codes(x_inj)
    raw, dead = np.empty((k, 2, 1 + n_cols + n_cols * (n_cols + 1) // 2)), np.empty((k, n_ev + 2), dtype=np.int32)
    for i, th in enumerate(thetas):
        lw_pe, lw_inj = eng.log_weights(th)
        raw[i], dead[i] = D.point_rank_correlations_reference(lw_pe, lw_inj, codes_obs, codes_det, masks[0], masks[1])
    total, mean_rank, cov = D.rankcorr_matrix(raw, n_cols)
    return total, mean_rank, cov, np.ascontiguousarray(dead[:, : n_ev + 1]), np.ascontiguousarray(dead[:, [n_ev + 1, n_ev]])


def catalog_rank_correlation_check(eng, thetas, pe_values, inj_values=None, pairs=None, levels=(0.05, 0.5, 0.95), point_weights=None, pedata=None, injdata=None,
                                   param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """Does the catalog's RANK correlation between two quantities agree with the one the fitted population predicts for detected
    sources?    :func:`catalog_correlation_check` asks the same of Pearson's correlation, which changes with the coordinate
    (``m1`` or ``log m1``, ``q`` or ``1 / q``) and is set by the tail of a heavy-tailed quantity.  Spearman's correlation is that of the
    weighted mid-ranks: no monotone map of either quantity changes it, and it sees any monotone dependence.  Per hyper-posterior point
    the observed catalog is the equal-weight mixture of its live events' population-informed posteriors -- all PE samples pooled, sample
    ``i`` of event ``e`` weighing ``w_i / S_e`` -- and the prediction the injection set under the point's weights; a member's rank is the
    weighted CDF of its own set at the member, so it changes with every point, and on the device (``eng.point_rank_correlations``) ``2
    (1 + C + C (C + 1) / 2)`` doubles come back per point while the weights never leave HBM.

    The arguments are :func:`catalog_correlation_check`'s, with ``inj_values`` (or ``injdata``) needed.  ``point_weights`` -- ``(K,)``, or
    ``(K, n_ev + 1)`` as the leave-one-out and Pareto-smoothed weights come, of which the last column (the injection set's, which no
    event's removal touches) is taken; finite, non-negative, not all 0; default equal -- weight the points in the bands and shares; they
    are applied here and never go to the device.  The device backend replaces the engine's rank-correlation columns.
    ``backend="host"`` runs the NumPy statement (:func:`gwinferno_amd.draws.point_rank_correlations_reference`) on
    ``eng.log_weights``: the statement the kernels are tested against, not a fall-back.

    Returns a dict: ``names``; ``pairs (n_pairs, 2)``; ``levels``; per point and pair ``rho_obs``, ``rho_det`` and ``delta = rho_obs -
    rho_det``, each ``(K, n_pairs)``; ``bands_rho_obs``, ``bands_rho_det``, ``bands_delta (Q, n_pairs)``
    (:func:`gwinferno_amd.draws.weighted_percentiles`); ``p_delta_positive (n_pairs,)``, the weighted share of the points with ``delta >
    0`` among those where it is a number, and ``p_two_sided = 2 min(p, 1 - p)``.  A (point, pair) with a dead set is skipped (NaN) and
    counted in ``n_skipped (n_pairs,)``.  Where a rank variance ``R_cc`` does not exceed ``variance_floor (2,)`` -- the derived bound on
    its rounding, :func:`gwinferno_amd.draws.rankcorr_error_bound`; a column whose members all tie has exactly 0 -- nothing is divided,
    the correlation is NaN and ``degenerate_obs`` / ``degenerate_det (K, n_pairs)`` flag it.  ``rank_mean_error``: the largest ``|m_c -
    1/2|`` over the live (point, set, column), which exact arithmetic makes 0.  Also the raw ``total``, ``mean_rank``, ``rank_cov``,
    ``dead`` and ``dead_set`` of ``eng.point_rank_correlations``, and ``n_points``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size < 1 or not np.all((levels >= 0.0) & (levels <= 1.0)):
        raise ValueError("levels must be numbers in [0, 1]")
    _checked_names(pe_values, pedata, param_names)
    names, x_pe, x_inj = _summary_columns(eng, pe_values, inj_values, pedata, injdata, param_names)
    if x_inj is None:
        raise ValueError("the predicted side ranks the injections: inj_values (or injdata) are needed")
    n_cols, n_ev = len(names), eng.n_ev
    if pairs is None:
        pairs = [(c, d) for c in range(n_cols) for d in range(c + 1, n_cols)]
    pairs = [tuple(names.index(p) if isinstance(p, str) else int(p) for p in pair) for pair in pairs]
    if not pairs or any(len(p) != 2 or not all(0 <= c < n_cols for c in p) for p in pairs):
        raise ValueError(f"pairs are pairs of names or of column indices below {n_cols}, at least one")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if point_weights is None:
        v = np.ones(k)
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape == (k, n_ev + 1):
            v = v[:, -1]
        if v.shape != (k,) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.any(v > 0.0):
            raise ValueError(f"point_weights are ({k},) or ({k}, {n_ev + 1}) finite non-negative numbers, not all 0")
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    total, mean_rank, cov, dead, dead_set = _rankcorr_points(eng, thetas, x_pe, x_inj, masks, backend)
    tile = D.RANKCORR_TILE
    sample_tiles = (n_ev * -(-eng.n_pe // tile), -(-eng.n_inj // tile))
    floor = np.array([D.rankcorr_error_bound(eng.n_pe, -(-(n_ev * eng.n_pe) // tile), sample_tiles[0], True),
                      D.rankcorr_error_bound(eng.n_inj, sample_tiles[1], sample_tiles[1], False)])
    c, d = pairs[:, 0], pairs[:, 1]
    rho, flags = [], []
    for s in range(2):
        r_cd, r_cc, r_dd = cov[:, s, c, d], cov[:, s, c, c], cov[:, s, d, d]
        alive = (dead_set[:, s] == 0)[:, None] & np.ones(r_cd.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            ok = alive & (r_cc > floor[s]) & (r_dd > floor[s])
        one = np.full(r_cd.shape, np.nan)
        one[ok] = r_cd[ok] / np.sqrt(r_cc[ok] * r_dd[ok])
        rho.append(one)
        flags.append((alive & ~ok).astype(np.int32))
    rho_obs, rho_det = rho
    delta = rho_obs - rho_det
    skipped = ((dead_set[:, 0] != 0) | (dead_set[:, 1] != 0))[:, None] & np.ones(delta.shape, dtype=bool)
    has = ~np.isnan(delta)
    den = (v[:, None] * has).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (v[:, None] * (has & (np.where(has, delta, 0.0) > 0.0))).sum(axis=0) / den
    live_means = mean_rank[dead_set == 0]
    out = {"names": names, "pairs": pairs, "levels": levels, "rho_obs": rho_obs, "rho_det": rho_det, "delta": delta, "p_delta_positive": p,
           "p_two_sided": 2.0 * np.minimum(p, 1.0 - p), "n_skipped": skipped.sum(axis=0).astype(np.int64), "degenerate_obs": flags[0], "degenerate_det": flags[1],
           "variance_floor": floor, "rank_mean_error": float(np.max(np.abs(live_means - 0.5))) if live_means.size else float("nan"), "total": total,
           "mean_rank": mean_rank, "rank_cov": cov, "dead": dead, "dead_set": dead_set, "n_points": k}
    for key in ("rho_obs", "rho_det", "delta"):
        out["bands_" + key] = D.weighted_percentiles(out[key], v, levels)
    return out


def event_variance_split(eng, thetas, pe_values, point_weights=None, leave_one_out=False, total_inj=None, nobs=None, marginalize_selection=False, pedata=None,
                         injdata=None, param_names=None, m1min=None, m2min=None, mmax=None, backend="device"):
    """How much of an event's population-informed variance is hyper-posterior uncertainty and how much its own measurement?  (DESIGN
    8j.)  :func:`event_credible_intervals` reports the standard deviation under the marginal weights, which is the total.  With the
    per-point means ``m_k`` and variances ``V_cc,k`` of the event (``eng.point_moments``) and normalised point weights ``v_k``, the law
    of total variance splits it:

    ``within = sum_k v_k V_cc,k``    ``between = sum_k v_k (m_k - mbar)^2``, ``mbar = sum_k v_k m_k``    ``total = within + between``

    ``within`` is the event's measurement under a fixed population, ``between`` what moving the population moves.

    ``thetas`` is ``(K, n_theta)``.  ``pe_values`` (or ``pedata`` with ``param_names``), the mass cuts and the masks are
    :func:`event_credible_intervals`'.  The weights on the k axis are applied here, on the host: equal by default, ``point_weights
    (K,)`` or ``(K, n_ev + 1)`` (the last column is not used), with ``leave_one_out=True`` those of :func:`leave_one_out_weights` and
    with ``leave_one_out="psis"`` those of :func:`pareto_smoothed_loo_weights` (``total_inj`` is needed; ``nobs`` and
    ``marginalize_selection`` as there).  A (point, event) at which the event has no weight is skipped and counted in ``n_dead``.  The
    device backend replaces the engine's KDE columns.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.point_moments_reference`) on ``eng.log_weights``: the statement the kernels are tested against, not a
    fall-back.

    Returns a dict: ``names``; ``mean``, ``within``, ``between``, ``total`` and ``fraction_between = between / total``, each ``(n_ev,
    C)`` (NaN for an event without a live point of positive weight; ``fraction_between`` also where ``total`` is 0); ``neff_points
    (n_ev,)``, ``(sum_k v)^2 / sum_k v^2`` over the points that count; ``n_dead (n_ev,)``; the raw ``point_mean (K, n_ev + 1, C)``,
    ``point_cov (K, n_ev + 1, C, C)`` and ``dead (K, n_ev + 1)``; ``n_points``; with leave-one-out weights ``elpd_loo (n_ev,)``, and
    with ``"psis"`` also ``pareto_k (n_ev,)``."""
    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    if not (isinstance(leave_one_out, bool) or leave_one_out == "psis"):
        raise ValueError(f"leave_one_out must be False, True or 'psis', not {leave_one_out!r}")
    _checked_names(pe_values, pedata, param_names)
    names, x_pe, _ = _summary_columns(eng, pe_values, None, pedata, None, param_names)
    n_cols, n_ev = len(names), eng.n_ev
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    if leave_one_out == "psis":
        if point_weights is not None:
            raise ValueError("leave_one_out='psis' makes the point weights itself: point_weights must be None")
        if total_inj is None:
            raise ValueError("leave_one_out='psis' needs total_inj")
        loo = pareto_smoothed_loo_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)
        v = loo["point_weights"]
    else:
        v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    v = np.ones((k, n_ev)) if v is None else np.asarray(v, dtype=np.float64)[:, :n_ev]
    mean, cov, dead = _moment_points(eng, thetas, x_pe, None, masks, backend)
    gone = dead[:, :n_ev] != 0                                    # (K, n_ev): the event has no weight at the point
    w = np.where(gone, 0.0, v)
    wsum, wsq = w.sum(axis=0), (w * w).sum(axis=0)
    diag = np.arange(n_cols)
    m = np.where(gone[:, :, None], 0.0, mean[:, :n_ev])          # (K, n_ev, C)
    var = np.where(gone[:, :, None], 0.0, cov[:, :n_ev][..., diag, diag])
    with np.errstate(divide="ignore", invalid="ignore"):
        vn = w / wsum                                             # NaN columns where an event has no point that counts
        mbar = (vn[:, :, None] * m).sum(axis=0)
        within = (vn[:, :, None] * var).sum(axis=0)
        between = (vn[:, :, None] * np.where(gone[:, :, None], 0.0, m - mbar) ** 2).sum(axis=0)
        total = within + between
        fraction = np.where(total > 0.0, between / total, np.nan)
        neff = np.where(wsum > 0.0, wsum * wsum / wsq, 0.0)
    out = {"names": names, "mean": mbar, "within": within, "between": between, "total": total, "fraction_between": fraction, "neff_points": neff,
           "n_dead": gone.sum(axis=0).astype(np.int64), "point_mean": mean, "point_cov": cov, "dead": dead, "n_points": k}
    if loo is not None:
        out["elpd_loo"] = loo["elpd_loo"]
        if "pareto_k" in loo:
            out["pareto_k"] = loo["pareto_k"]
    return out


def _conditional_points(eng, thetas, x, y, edges, pe_values, inj_values, backend):
    """``(share, mean, var (K, n_ev + 1, B), dead (K, n_ev + 1), edges (B + 1,))`` of ``y`` given the bin of ``x`` on either backend
    (DESIGN 8k): ``x`` is binned with ``np.histogram``'s rule (:func:`gwinferno_amd.draws.digitize`)."""
    from . import draws as D

    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    for name in (x, y):
        if name not in pe_values or (inj_values is not None and name not in inj_values):
            raise ValueError(f"unknown quantity {name!r}")
    edges = np.asarray(edges, dtype=np.float64).ravel()
    n_bins = edges.size - 1
    if not 1 <= n_bins <= min(D.MAX_CDF_GRID, D.MAX_CONDITIONAL_ITEMS):
        raise ValueError("edges are between 2 and 257 increasing numbers")
    _, v_pe, v_inj = _summary_columns(eng, pe_values, inj_values, None, None, [x, y])
    codes_pe, codes_inj = D.digitize(v_pe[0], edges)[None], (None if v_inj is None else D.digitize(v_inj[0], edges)[None])
    y_pe, y_inj = np.ascontiguousarray(v_pe[1:]), (None if v_inj is None else np.ascontiguousarray(v_inj[1:]))
    if backend == "device":
        eng.set_histogram_bins(codes_pe, codes_inj, n_bins=n_bins)
        eng.set_kde_columns(y_pe, y_inj)
        share, mean, var, dead = eng.point_conditionals(thetas, [(0, 0)])
        return share[:, :, 0], mean[:, :, 0], var[:, :, 0], dead, edges
    k, n_segs = thetas.shape[0], eng.n_ev + 1
    out, dead = np.empty((k, n_segs, 3, n_bins)), np.empty((k, n_segs), dtype=np.int32)
    for i, th in enumerate(thetas):
        lw_pe, lw_inj = eng.log_weights(th)
        one, dead[i] = D.point_conditionals_reference(lw_pe, lw_inj, codes_pe, codes_inj, y_pe, y_inj, [(0, 0)], n_bins)
        out[i] = one[:, 0]
    return out[:, :, 0], out[:, :, 1], out[:, :, 2], dead, edges


def catalog_conditional_check(eng, thetas, x, y, edges, *, pe_values, inj_values, point_weights=None, backend="device", levels=(5, 50, 95)):
    """Do the catalog's conditional mean and width of ``y`` given ``x`` agree with what the fitted population predicts for detected
    sources?    A covariance (:func:`catalog_correlation_check`) sees the linear part of a dependence only; the known
    departures from a separable model are a mean of ``chi_eff`` that drifts with mass ratio and a width that grows with redshift or mass:
    statements about ``E[y | x]`` and ``Var[y | x]`` as functions of ``x``.  Per hyper-posterior point k and bin b of ``x`` the device
    (``eng.point_conditionals``) returns every segment's share ``a``, conditional mean ``m`` and conditional variance ``v``; the observed
    catalog is the equal-weight mixture of its live events e:

    ``A_b = mean_e a_eb``    ``mu_b = sum_e a_eb m_eb / sum_e a_eb``    ``sigma2_b = sum_e a_eb [v_eb + (m_eb - mu_b)^2] / sum_e a_eb``

    (events with ``a_eb = 0`` are left out of a bin's sums), held against the injection segment's ``m_b`` and ``v_b``.

    ``thetas`` is ``(K, n_theta)``.  ``x`` and ``y`` name quantities of ``pe_values`` (name -> ``(n_ev, n_pe)``) and ``inj_values``
    (name -> ``(n_inj,)``; ``None``: no predicted side, NaN); ``edges`` are the ``B + 1 <= 257`` increasing bin edges of ``x``
    (``np.histogram``'s rule).  ``point_weights (K,)`` -- finite, non-negative, not all 0; default equal -- weight the points in the bands
    and in the shares; they are applied here and never go to the device.  ``levels`` are percentiles in ``[0, 100]``.  The device
    backend replaces the engine's histogram bins and KDE columns; the draw mask the engine holds stays.  ``backend="host"`` runs the NumPy
    statement (:func:`gwinferno_amd.draws.point_conditionals_reference`) on ``eng.log_weights``, without a mask: the statement the
    kernels are tested against, not a fall-back.

    Returns a dict: ``x``, ``y``, ``edges``, ``levels``; per point and bin ``share_obs``, ``mean_obs``, ``var_obs``, ``std_obs``,
    ``share_det``, ``mean_det``, ``var_det``, ``std_det``, ``delta_mean = mean_obs - mean_det`` and ``delta_std = std_obs - std_det``,
    each ``(K, B)``; ``bands_<key> (Q, B)`` of each, the weighted percentiles over the points
    (:func:`gwinferno_amd.draws.weighted_percentiles`); ``p_delta_mean_positive`` and ``p_delta_std_positive (B,)``, the weighted share
    of the points with ``delta > 0`` among those where it is a number, and ``p_mean_two_sided``, ``p_std_two_sided = 2 min(p, 1 - p)``.
    A (point, bin) with no observed or no predicted weight is skipped (NaN) and counted in ``n_skipped (B,)``.  Also ``n_live (K,)``, the
    live events per point; the raw ``point_share``, ``point_mean``, ``point_var (K, n_ev + 1, B)`` and ``dead``; ``n_points``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k, n_ev = thetas.shape[0], eng.n_ev
    if k < 1:
        raise ValueError("thetas holds no point")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size < 1 or not np.all((levels >= 0.0) & (levels <= 100.0)):
        raise ValueError("levels must be percentiles in [0, 100]")
    if point_weights is None:
        v = np.ones(k)
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape != (k,) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.any(v > 0.0):
            raise ValueError(f"point_weights are ({k},) finite non-negative numbers, not all 0")
    share, mean, var, dead, edges = _conditional_points(eng, thetas, x, y, edges, pe_values, inj_values, backend)
    live = dead[:, :n_ev] == 0                                    # (K, n_ev)
    n_live = live.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(live[:, :, None], share[:, :n_ev], 0.0)      # (K, n_ev, B); NaN nowhere
        has = a > 0.0
        den = a.sum(axis=1)                                       # (K, B)
        share_obs = den / n_live[:, None]
        m = np.where(has, mean[:, :n_ev], 0.0)
        mean_obs = (a * m).sum(axis=1) / den                      # NaN where no event has weight in the bin
        dm = np.where(has, m - mean_obs[:, None, :], 0.0)
        var_obs = (a * (np.where(has, var[:, :n_ev], 0.0) + dm * dm)).sum(axis=1) / den
        std_obs = np.sqrt(var_obs)
        share_det, mean_det, var_det = share[:, n_ev], mean[:, n_ev], var[:, n_ev]
        std_det = np.sqrt(var_det)
        delta_mean, delta_std = mean_obs - mean_det, std_obs - std_det

    def shares(delta):
        has_delta = ~np.isnan(delta)
        total = (v[:, None] * has_delta).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (v[:, None] * (has_delta & (np.where(has_delta, delta, 0.0) > 0.0))).sum(axis=0) / total
        return p, 2.0 * np.minimum(p, 1.0 - p)

    p_mean, p_std = shares(delta_mean), shares(delta_std)
    out = {"x": x, "y": y, "edges": edges, "levels": levels, "share_obs": share_obs, "mean_obs": mean_obs, "var_obs": var_obs, "std_obs": std_obs,
           "share_det": share_det, "mean_det": mean_det, "var_det": var_det, "std_det": std_det, "delta_mean": delta_mean, "delta_std": delta_std,
           "p_delta_mean_positive": p_mean[0], "p_mean_two_sided": p_mean[1], "p_delta_std_positive": p_std[0], "p_std_two_sided": p_std[1],
           "n_skipped": np.isnan(delta_mean).sum(axis=0).astype(np.int64), "n_live": n_live.astype(np.int64), "point_share": share, "point_mean": mean,
           "point_var": var, "dead": dead, "n_points": k}
    for key in ("share_obs", "mean_obs", "std_obs", "share_det", "mean_det", "std_det", "delta_mean", "delta_std"):
        out["bands_" + key] = D.weighted_percentiles(out[key], v, levels / 100.0)
    return out


def event_conditional_moments(eng, thetas, x, y, edges, *, pe_values, inj_values=None, point_weights=None, leave_one_out=False, total_inj=None, nobs=None,
                              marginalize_selection=False, backend="device"):
    """Every event's population-informed conditional mean and variance of ``y`` per bin of ``x``, marginalised over the hyper-posterior
    points, with the variance split as in :func:`event_variance_split`.  With the per-point shares ``a_kb``, conditional
    means ``m_kb`` and variances ``v_kb`` of the event (``eng.point_conditionals``) and normalised point weights ``v_k``, the weight of
    point k in bin b is ``u_kb = v_k a_kb / sum_k v_k a_kb`` and

    ``share_b = sum_k v_k a_kb``   ``mean_b = sum_k u_kb m_kb``   ``within_b = sum_k u_kb v_kb``   ``between_b = sum_k u_kb (m_kb - mean_b)^2``

    ``total = within + between`` is the variance of ``y`` under the marginal weights restricted to the bin (the law of total variance).

    The arguments are :func:`catalog_conditional_check`'s (``inj_values`` is not needed).  The weights on the k axis are applied here, on the
    host: equal by default, ``point_weights (K,)`` or ``(K, n_ev + 1)`` (the last column is not used), with ``leave_one_out=True`` those of
    :func:`leave_one_out_weights` and with ``leave_one_out="psis"`` those of :func:`pareto_smoothed_loo_weights` (``total_inj`` is needed;
    ``nobs`` and ``marginalize_selection`` as there).  A (point, event, bin) without weight -- the event dead at the point or the bin
    empty -- is skipped and counted in ``n_skipped``.

    Returns a dict: ``x``, ``y``, ``edges``; ``share``, ``mean``, ``within``, ``between`` and ``total``, each ``(n_ev, B)`` (NaN mean
    and variances for a bin no point gives weight; NaN shares too for an event without a live point of positive weight); ``neff_points
    (n_ev,)``, ``(sum_k v)^2 / sum_k v^2`` over the points at which the event is live; ``n_skipped (n_ev, B)``; ``n_dead (n_ev,)``; the
    raw ``point_share``, ``point_mean``, ``point_var (K, n_ev + 1, B)`` and ``dead``; ``n_points``; with leave-one-out weights ``elpd_loo
    (n_ev,)``, and with ``"psis"`` also ``pareto_k (n_ev,)``."""
    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k, n_ev = thetas.shape[0], eng.n_ev
    if k < 1:
        raise ValueError("thetas holds no point")
    if not (isinstance(leave_one_out, bool) or leave_one_out == "psis"):
        raise ValueError(f"leave_one_out must be False, True or 'psis', not {leave_one_out!r}")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    if leave_one_out == "psis":
        if point_weights is not None:
            raise ValueError("leave_one_out='psis' makes the point weights itself: point_weights must be None")
        if total_inj is None:
            raise ValueError("leave_one_out='psis' needs total_inj")
        loo = pareto_smoothed_loo_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)
        v = loo["point_weights"]
    else:
        v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    v = np.ones((k, n_ev)) if v is None else np.asarray(v, dtype=np.float64)[:, :n_ev]
    share, mean, var, dead, edges = _conditional_points(eng, thetas, x, y, edges, pe_values, inj_values, backend)
    gone = dead[:, :n_ev] != 0                                    # (K, n_ev): the event has no weight at the point
    w = np.where(gone, 0.0, v)
    wsum, wsq = w.sum(axis=0), (w * w).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        vn = w / wsum                                             # NaN columns where an event has no point that counts
        a = np.where(gone[:, :, None], 0.0, share[:, :n_ev])     # (K, n_ev, B)
        has = (a > 0.0) & (w[:, :, None] > 0.0)
        mass = vn[:, :, None] * a
        share_e = mass.sum(axis=0)                                # (n_ev, B)
        u = np.where(has, mass, 0.0) / np.where(has, mass, 0.0).sum(axis=0)
        m = np.where(has, mean[:, :n_ev], 0.0)
        mbar = (u * m).sum(axis=0)
        mbar = np.where(has.any(axis=0), mbar, np.nan)
        within = np.where(has.any(axis=0), (u * np.where(has, var[:, :n_ev], 0.0)).sum(axis=0), np.nan)
        between = np.where(has.any(axis=0), (u * np.where(has, m - mbar, 0.0) ** 2).sum(axis=0), np.nan)
        neff = np.where(wsum > 0.0, wsum * wsum / wsq, 0.0)
    out = {"x": x, "y": y, "edges": edges, "share": share_e, "mean": mbar, "within": within, "between": between, "total": within + between, "neff_points": neff,
           "n_skipped": (~has).sum(axis=0).astype(np.int64), "n_dead": gone.sum(axis=0).astype(np.int64), "point_share": share, "point_mean": mean, "point_var": var,
           "dead": dead, "n_points": k}
    if loo is not None:
        out["elpd_loo"] = loo["elpd_loo"]
        if "pareto_k" in loo:
            out["pareto_k"] = loo["pareto_k"]
    return out


def _tail_points(eng, thetas, m_pe, m_inj, masks, backend):
    """``(tail_pe (K, n_ev, m_pe), tail_inj (K, m_inj), stats (K, n_ev + 1, 4), counts (K, n_ev + 1, 4))`` of the points on either backend
    (DESIGN 8m)."""
    from . import draws as D

    if backend == "device":
        if masks[0] is not None:
            eng.set_draw_mask(*masks)
        eng.set_tail_sizes(m_pe, m_inj)
        return eng.point_tails(thetas)
    k, n_ev = thetas.shape[0], eng.n_ev
    tail_pe, tail_inj = np.empty((k, n_ev, m_pe)), np.empty((k, m_inj))
    stats, counts = np.empty((k, n_ev + 1, 4)), np.empty((k, n_ev + 1, 4), dtype=np.int32)
    for i, th in enumerate(thetas):
        lw_pe, lw_inj = eng.log_weights(th)
        tail_pe[i], tail_inj[i], stats[i], counts[i] = D.point_tails_reference(lw_pe, lw_inj, masks[0], masks[1], m_pe, m_inj)
    return tail_pe, tail_inj, stats, counts


def importance_sum_diagnostics(eng, thetas, m_pe=None, m_inj=None, point_weights=None, backend="device", pedata=None, injdata=None, m1min=None, m2min=None, mmax=None):
    """Can the inner importance sums be trusted?    Every number the engine returns is a self-normalised sum of ``w = p(x |
    theta) / prior`` over an event's PE samples or over the found injections.  ``log_nEffs`` and the variance site are made of the same
    weights and stay finite when a handful of samples carry the sum; the Pareto shape ``khat`` of the largest weights (Vehtari et al.,
    *Pareto smoothed importance sampling*) says when that is so: below 0.5 good, up to 0.7 usable, above it unreliable.  Per
    hyper-posterior point and segment -- the events, then the injection set -- ``eng.point_tails`` returns the ``m`` largest live
    log-weights and the sum of the rest, about 0.1 MB per point where the weights themselves are megabytes and never leave HBM; the fit
    (:func:`gwinferno_amd.draws.pareto_tail_fit`) is made here.

    ``m_pe`` / ``m_inj``: the tail sizes, ``None`` for ``min(floor(n / 5), ceil(3 sqrt(n)))`` capped at 4096.  ``point_weights`` -- ``(K,)``
    or ``(K, n_ev + 1)``, finite, non-negative, not all 0 in a column; default equal -- weight the points in the shares; they are applied
    here and never go to the device.  ``pedata``, ``injdata``, ``m1min``, ``m2min``, ``mmax``: the mass cuts of
    :func:`posterior_predictive_draws` as masks; without them the mask the engine holds stays (device backend).  The device backend
    replaces the engine's tail sizes.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.point_tails_reference`) on ``eng.log_weights``: the statement the kernels are tested against, not a
    fall-back.

    A (point, segment) is SKIPPED -- counted, never fitted -- when the segment is dead there or has ``n_live <= m``: nothing lies outside
    the tail.  Returns a dict.  Per point and segment, ``(K, n_ev + 1)``: ``pareto_k`` (NaN where skipped; inf where the fit has nothing
    to work on: ``m < 5``, a constant tail, a lowest quarter that ties with the cut-off); ``n_live``; ``skipped``; ``log_sum_raw = max +
    log S``; ``log_sum_psis = max + log(rest + sum exp(smoothed tail))`` with the tail's weights replaced by the fitted quantiles and
    ``rest`` the sum outside the tail (:func:`gwinferno_amd.draws.tail_cutoff_and_rest`); ``log_sum_diff``, their difference; ``neff``, a
    LOWER bound of the engine's ``n_eff = S^2 / sum w^2`` from what came back: the tail's and the ties' squares exactly, the samples below
    the cut-off counted as ``w_below body >= sum w^2`` of them (exact for ``n_live <= m``; with a heavy tail, where it matters, the tail's
    squares dominate); on the host backend also ``neff_exact``.  NaN for a dead segment.  Per segment over the points, ``(n_ev + 1,)``:
    ``share_above_0.5`` and ``share_above_0.7``, the weighted share of the fitted points with ``khat`` above the level (NaN: none
    fitted); ``worst_point`` (-1: none fitted) and ``worst_k``; ``n_skipped``.  Also ``m_pe``, ``m_inj``, ``n_points`` and the raw
    ``tail_pe``, ``tail_inj``, ``stats``, ``counts``."""
    import math

    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k, n_ev = thetas.shape[0], eng.n_ev
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    m_pe = min(D.psis_tail_size(eng.n_pe), D.MAX_TAIL) if m_pe is None else int(m_pe)
    m_inj = min(D.psis_tail_size(eng.n_inj), D.MAX_TAIL) if m_inj is None else int(m_inj)
    if point_weights is None:
        v = np.ones((k, n_ev + 1))
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape == (k,):
            v = np.repeat(v[:, None], n_ev + 1, axis=1)
        if v.shape != (k, n_ev + 1) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.all(np.any(v > 0.0, axis=0)):
            raise ValueError(f"point_weights are ({k},) or ({k}, {n_ev + 1}) finite non-negative numbers, not all 0 in a column")
    masks = _mass_cut_masks(pedata, injdata, m1min, m2min, mmax)
    tail_pe, tail_inj, stats, counts = _tail_points(eng, thetas, m_pe, m_inj, masks, backend)
    shape = (k, n_ev + 1)
    khat, psis, neff = np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape, np.nan)
    dead = counts[..., 3] != 0
    n_live = counts[..., 0].astype(np.int64)
    sizes = np.array([m_pe] * n_ev + [m_inj])
    skipped = dead | (n_live <= sizes[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.where(dead, np.nan, stats[..., 0] + np.log(stats[..., 1]))
    for p in range(k):
        for s in range(n_ev + 1):
            if dead[p, s]:
                continue
            tail = tail_pe[p, s] if s < n_ev else tail_inj[p]
            top, total, body, below_max = stats[p, s]
            cutoff, rest = D.tail_cutoff_and_rest(tail, stats[p, s], counts[p, s])
            w_tail = np.exp(tail - top)
            extra = max(int(counts[p, s, 1]) + int(counts[p, s, 2]) - tail.size, 0)
            squares = math.fsum((w_tail * w_tail).tolist()) + extra * w_tail[0] * w_tail[0] + (math.exp(below_max - top) * body if body > 0.0 else 0.0)
            neff[p, s] = total * total / squares
            if skipped[p, s]:
                continue
            khat[p, s], smoothed = D.pareto_tail_fit(tail, float(cutoff), top)
            psis[p, s] = top + math.log(float(rest) + math.fsum(np.exp(smoothed).tolist()))
    fitted = ~skipped
    share, worst_point, worst_k = {}, np.full(n_ev + 1, -1, dtype=np.int64), np.full(n_ev + 1, np.nan)
    den = (v * fitted).sum(axis=0)
    for level in (0.5, 0.7):
        with np.errstate(divide="ignore", invalid="ignore"):
            share[level] = (v * (fitted & (np.where(fitted, khat, 0.0) > level))).sum(axis=0) / den
    for s in range(n_ev + 1):
        if fitted[:, s].any():
            worst_point[s] = int(np.argmax(np.where(fitted[:, s], khat[:, s], -np.inf)))
            worst_k[s] = khat[worst_point[s], s]
    out = {"pareto_k": khat, "n_live": n_live, "skipped": skipped, "neff": neff, "log_sum_raw": raw, "log_sum_psis": psis, "log_sum_diff": psis - raw,
           "share_above_0.5": share[0.5], "share_above_0.7": share[0.7], "worst_point": worst_point, "worst_k": worst_k, "n_skipped": skipped.sum(axis=0).astype(np.int64),
           "m_pe": m_pe, "m_inj": m_inj, "n_points": k, "tail_pe": tail_pe, "tail_inj": tail_inj, "stats": stats, "counts": counts}
    if backend == "host":
        exact = np.full(shape, np.nan)
        for p, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            for s in range(n_ev + 1):
                w = D.draw_weights(lw_pe[s], None if masks[0] is None else np.asarray(masks[0]).reshape(n_ev, -1)[s]) if s < n_ev else D.draw_weights(lw_inj, masks[1])
                if not dead[p, s]:
                    exact[p, s] = math.fsum(w.tolist()) ** 2 / math.fsum((w * w).tolist())
        out["neff_exact"] = exact
    return out


BOOTSTRAP_CHUNK = 64  # points per gwi_point_bootstrap call of likelihood_bootstrap (the sums do not depend on it)


def _bootstrap_points(eng, thetas, seed, n_replicates, masks, backend, chunk):
    """``(sums (K, n_ev + 1, B), stats (K, n_ev + 1, 2), dead (K, n_ev + 1), counts (n_ev + 1, B))`` of the points on either backend
    (DESIGN 8n); more replicates than one call takes are split over ``first_replicate``."""
    from . import draws as D

    k, n_ev = thetas.shape[0], eng.n_ev
    sums, counts = np.empty((k, n_ev + 1, n_replicates)), np.empty((n_ev + 1, n_replicates), dtype=np.int64)
    stats, dead = np.empty((k, n_ev + 1, 2)), np.empty((k, n_ev + 1), dtype=np.int32)
    if backend == "device":
        eng.set_draw_mask(*masks)
        for b0 in range(0, n_replicates, D.MAX_BOOTSTRAP_REPLICATES):
            b1 = min(n_replicates, b0 + D.MAX_BOOTSTRAP_REPLICATES)
            eng.set_bootstrap(seed, b1 - b0, b0)
            for k0 in range(0, k, chunk):
                sums[k0 : k0 + chunk, :, b0:b1], stats[k0 : k0 + chunk], dead[k0 : k0 + chunk], counts[:, b0:b1] = eng.point_bootstrap(thetas[k0 : k0 + chunk])
        return sums, stats, dead, counts
    # the statement, one segment's counts at a time: they serve every point
    lw = [eng.log_weights(th) for th in thetas]
    for seg in range(n_ev + 1):
        n = eng.n_pe if seg < n_ev else eng.n_inj
        c = D.bootstrap_counts(seed, seg * eng.n_pe, n, n_replicates)
        mask = None if masks[0 if seg < n_ev else 1] is None else (np.asarray(masks[0]).reshape(n_ev, -1)[seg] if seg < n_ev else masks[1])
        for p in range(k):
            sums[p, seg], stats[p, seg], dead[p, seg], counts[seg] = D.bootstrap_segment(lw[p][0][seg] if seg < n_ev else lw[p][1], mask, c)
    return sums, stats, dead, counts


def likelihood_bootstrap(eng, thetas, total_inj, n_replicates=128, seed=0, nobs=None, backend="device", chunk=BOOTSTRAP_CHUNK, masks=None):
    """How much of ``log L(theta_a) - log L(theta_b)`` is sampling noise of the catalog?    Every number the engine returns
    is a Monte-Carlo sum over a finite set of PE samples and found injections.  ``log_nEffs``, the delta-method
    ``variance_log_likelihood`` and the Pareto ``khat`` (:func:`importance_sum_diagnostics`) speak of one point; the errors at two points
    of a chain are made of the same samples and largely cancel in the difference, and the delta method says nothing about the bias of
    the logarithm of a noisy mean.  This is the non-parametric answer: a Poisson bootstrap with common random numbers.  Every event's
    PE samples and the injection set are resampled ``n_replicates`` times -- sample ``i`` is taken ``c_ib ~ Poisson(1)`` times in
    replicate ``b``, the same at every point (:func:`gwinferno_amd.draws.bootstrap_counts`) --, ``eng.point_bootstrap`` returns the
    resampled sums, ``(n_ev + 1) B`` doubles per point while the weights never leave HBM, and
    :func:`gwinferno_amd.draws.bootstrap_likelihood` forms ``log L_b = sum_e logBF_eb - N_obs log mu_b`` here.  The injections that were
    not found are resampled as well (a Poisson number of them per replicate, from ``total_inj``).  NO cuts (``min_neff``, variance) and
    NO marginalised-selection term are applied: the replicates are those of the plain ``sum logBF - N_obs log mu``.

    ``thetas (K, n_theta)``; ``total_inj`` the injections made; ``nobs`` the events of the likelihood (default: the engine's);
    ``n_replicates`` any number up to 2^20, split over calls of at most 1 024; ``chunk`` the points per call (the sums do not depend on
    either split).  ``masks = (pe_mask, inj_mask)`` as :meth:`Engine.set_draw_mask` takes them (None: every sample; a masked found
    injection counts as one that was not found).  The device backend replaces the engine's draw mask and bootstrap setting.  ``backend="host"``
    runs the NumPy statement on ``eng.log_weights``: the statement the kernels are tested against, not a fall-back.

    Returns a dict: ``log_l (K,)``, the uncut value from the entry's own ``M`` and ``S``; ``log_l_rep (K, B)``; ``std_log_l (K,)``;
    ``bias_log_l (K,)`` = the mean over the replicates minus ``log_l``; ``std_log_bf (K, n_ev)``; ``std_log_mu (K,)``; ``delta_std (K,
    K)``, the standard deviation over the replicates of ``log_l_rep[a] - log_l_rep[b]`` -- the noise of the difference; ``corr (K, K)``,
    the correlation of the replicates of two points; ``variance_log_likelihood (K,)`` from ``eng.evaluate_batch`` for the side-by-side
    with ``std_log_l ** 2``; ``n_dead``, the (point, segment) pairs without weight, whose replicates are NaN -- counted, never divided;
    ``n_nan_replicates (K,)``, the replicates of a point that are NaN (a dead segment: all; a replicate that drew nothing from a
    segment, ``C_eb = 0``, possible only for tiny segments), left out of the moments of that point and of its pairs; ``counts (n_ev + 1,
    B)``; ``c_miss (B,)``; ``log_bf (K, n_ev)``, ``log_mu (K,)``; ``n_replicates``, ``seed``.  Standard deviations divide by the
    replicates used minus one."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k, n_ev = thetas.shape[0], eng.n_ev
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    n_replicates, chunk = int(n_replicates), int(chunk)
    if not 1 <= n_replicates <= D.MAX_BOOTSTRAP_REPLICATE:
        raise ValueError(f"n_replicates = {n_replicates} is not in 1 ... {D.MAX_BOOTSTRAP_REPLICATE}")
    if chunk < 1:
        raise ValueError("chunk is at least 1")
    n_obs = float(getattr(eng, "n_ev_global", n_ev) if nobs is None else nobs)
    pe_mask, inj_mask = (None, None) if masks is None else masks
    held = (pe_mask, inj_mask)
    sums, stats, dead, counts = _bootstrap_points(eng, thetas, seed, n_replicates, held, backend, chunk)
    n_live = np.array([eng.n_pe if held[0] is None else int(np.count_nonzero(np.asarray(held[0]).reshape(n_ev, -1)[e])) for e in range(n_ev)]
                      + [eng.n_inj if held[1] is None else int(np.count_nonzero(held[1]))])
    out = D.bootstrap_likelihood(sums, stats, dead, counts, n_live, total_inj, n_obs, seed)
    rep = out["log_l_rep"]

    def spread(x):  # over the last axis, NaN replicates left out
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = np.isfinite(x)
            n = ok.sum(axis=-1)
            mean = np.where(ok, x, 0.0).sum(axis=-1) / n
            var = np.where(ok, (x - mean[..., None]) ** 2, 0.0).sum(axis=-1) / (n - 1)
            return mean, np.sqrt(np.where(n > 1, var, np.nan))

    mean_l, std_l = spread(rep)
    delta, corr = np.empty((k, k)), np.empty((k, k))
    for a in range(k):
        _, delta[a] = spread(rep[a][None, :] - rep)
        for b in range(k):
            ok = np.isfinite(rep[a]) & np.isfinite(rep[b])
            if ok.sum() > 1:
                xa, xb = rep[a][ok] - rep[a][ok].mean(), rep[b][ok] - rep[b][ok].mean()
                with np.errstate(invalid="ignore", divide="ignore"):
                    corr[a, b] = 1.0 if a == b and np.any(xa != 0.0) else float(np.dot(xa, xb) / np.sqrt(np.dot(xa, xa) * np.dot(xb, xb)))
            else:
                corr[a, b] = np.nan
    var_site = np.empty(k)
    step = int(eng.max_batch)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, k, step):
            res = eng.evaluate_batch(thetas[k0 : k0 + step], total_inj, nobs=nobs, marginalize_selection=False, min_neff_cut=False, max_variance_cut=False, want_grad=False)
            var_site[k0 : k0 + len(res)] = [r.summary.variance_log_likelihood for r in res]
    out.update(std_log_l=std_l, bias_log_l=mean_l - out["log_l"], std_log_bf=spread(out["log_bf_rep"])[1], std_log_mu=spread(out["log_mu_rep"])[1], delta_std=delta, corr=corr,
               variance_log_likelihood=var_site, n_nan_replicates=(~np.isfinite(rep)).sum(axis=1).astype(np.int64), counts=counts, sums=sums, stats=stats, dead=dead,
               n_replicates=n_replicates, seed=int(seed))
    return out


def _joint_setup(eng, pe_values, inj_values, edges, pairs, param_names):
    """``(names, pair names, pairs (R, 2), grid, n_bins, pe_bins (C, n_ev, n_pe), inj_bins (C, n_inj) or None)`` of a joint-table call:
    the quantities digitised once with ``np.histogram``'s rule (:func:`gwinferno_amd.draws.digitize`)."""
    from . import draws as D

    names = list(param_names) if param_names is not None else list(pe_values)
    if not 1 <= len(names) <= 8:
        raise ValueError("between 1 and 8 quantities can be binned in one pass")
    grid = {p: np.asarray(edges[p], dtype=np.float64).ravel() for p in names}
    n_bins = grid[names[0]].size - 1
    if any(g.size - 1 != n_bins for g in grid.values()):
        raise ValueError("every quantity needs the same number of bins")
    if not 1 <= n_bins <= D.MAX_HIST2D_BINS:
        raise ValueError(f"n_bins must be in 1 ... {D.MAX_HIST2D_BINS}")
    if pairs is None:
        pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
    pair_names = [tuple(p) for p in pairs]
    if not 1 <= len(pair_names) <= D.MAX_HIST2D_PAIRS:
        raise ValueError(f"{len(pair_names)} pairs: between 1 and {D.MAX_HIST2D_PAIRS} can be asked for in one call")
    for p in pair_names:
        if len(p) != 2 or p[0] not in names or p[1] not in names:
            raise ValueError(f"unknown pair {p!r}: a pair is two of {names}")
    index = np.array([[names.index(x), names.index(y)] for x, y in pair_names], dtype=np.int32)
    _, v_pe, v_inj = _summary_columns(eng, pe_values, inj_values, None, None, names)
    pe_bins = np.stack([D.digitize(v_pe[c], grid[p]) for c, p in enumerate(names)])
    inj_bins = None if v_inj is None else np.stack([D.digitize(v_inj[c], grid[p]) for c, p in enumerate(names)])
    return names, pair_names, index, grid, n_bins, pe_bins, inj_bins


def event_joint_posteriors(eng, thetas, pe_values, edges, pairs=None, inj_values=None, param_names=None, point_weights=None, leave_one_out=False, total_inj=None, nobs=None,
                           marginalize_selection=False, backend="device", chunk=HISTOGRAM_CHUNK):
    """The two-dimensional panels of the corner plot of every event's population-informed posterior, marginalised over K hyper-posterior
    draws, at histogram cost: per event, pair of quantities ``(x, y)`` and cell the mean over the draws of ``(sum of w_i in
    the cell) / (sum of w_i)`` with ``w_i = p(x_i | theta_k) / prior_i`` -- the joint counterpart of :func:`reweighted_event_posteriors`
    -- and the same table for the injection set, the predicted detected distribution.  On the device (``eng.point_histograms2d``) the
    weights never leave HBM.

    ``thetas`` is ``(K, n_theta)``.  ``pe_values`` maps a name to ``(n_ev, n_pe)``, ``inj_values`` the same names to ``(n_inj,)`` (``None``:
    no predicted table); ``edges`` maps each name to increasing bin edges, all with the same number of bins ``B <= 64``
    (``np.histogram``'s rule).  ``param_names`` selects and orders the names (at most 8); ``pairs`` is a list of ``(x name, y name)``, at
    most 8, default every pair ``i < j`` of the names.  The point weights are :func:`reweighted_event_posteriors`': equal by default,
    ``point_weights (K, n_ev + 1)`` or ``(K,)`` in ``[0, 1]``, ``leave_one_out=True`` for :func:`leave_one_out_weights` and
    ``leave_one_out="psis"`` for :func:`pareto_smoothed_loo_weights` (``total_inj`` is then needed); they go to the device with the
    points.  The device backend replaces the engine's histogram bins; the draw mask the engine holds stays.  ``backend="host"`` runs
    the NumPy statement (:func:`gwinferno_amd.draws.point_histograms2d_reference`) on ``eng.log_weights``, without a mask: the statement
    the kernels are tested against, not a fall-back.

    Returns a dict: ``pairs`` (the name pairs), ``edges``; ``events (n_ev, R, B, B)``, the mean share per cell, indexed ``[x bin, y
    bin]``, and ``events_density``, the same divided by the cell areas -- ``pcolormesh(edges[x], edges[y], events_density[e, r].T)``;
    ``predicted (R, B, B)`` and ``predicted_density`` (with ``inj_values``); ``outside``, ``{"events": (n_ev, R), "predicted": (R,)}``,
    the weight share outside the edges in either coordinate; ``n_points``, the same layout per segment, the points at which it had
    weight (NaN tables where that is 0); with weights ``point_weight_sum (n_ev + 1,)``, and with leave-one-out weights ``elpd_loo``,
    ``neff_points`` and for ``"psis"`` ``pareto_k``."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k, n_ev = thetas.shape[0], eng.n_ev
    if k < 1:
        raise ValueError("thetas holds no point")
    chunk = int(chunk)
    if not 1 <= chunk <= HISTOGRAM_CHUNK:
        raise ValueError(f"chunk must be in 1 ... {HISTOGRAM_CHUNK}")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    if not (isinstance(leave_one_out, bool) or leave_one_out == "psis"):
        raise ValueError(f"leave_one_out must be False, True or 'psis', not {leave_one_out!r}")
    names, pair_names, index, grid, n_bins, pe_bins, inj_bins = _joint_setup(eng, pe_values, inj_values, edges, pairs, param_names)
    if leave_one_out == "psis":
        if point_weights is not None:
            raise ValueError("leave_one_out='psis' makes the point weights itself: point_weights must be None")
        if total_inj is None:
            raise ValueError("leave_one_out='psis' needs total_inj")
        loo = pareto_smoothed_loo_weights(eng, thetas, total_inj, nobs=nobs, marginalize_selection=marginalize_selection)
        v = loo["point_weights"]
    else:
        v, loo = _resolve_point_weights(eng, thetas, point_weights, leave_one_out, total_inj, nobs, marginalize_selection)
    n_pairs = len(pair_names)
    if backend == "device":
        eng.set_histogram_bins(pe_bins, inj_bins, n_bins=n_bins)
        out = None
        for i in range(0, k, chunk):
            out = eng.point_histograms2d(thetas[i : i + chunk], index, out=out, **({} if v is None else {"point_weights": v[i : i + chunk]}))
        hist_pe, hist_inj, dead, vsum = out["hist_pe"], out["hist_inj"], out["n_dead"], out["vsum"]
    else:
        hist_pe, hist_inj = np.zeros((n_ev, n_pairs, n_bins, n_bins)), (None if inj_bins is None else np.zeros((n_pairs, n_bins, n_bins)))
        dead, vsum = np.zeros(n_ev + 1, dtype=np.int32), (None if v is None else np.zeros(n_ev + 1))
        for p, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            one = D.point_histograms2d_reference(lw_pe, lw_inj, None, None, pe_bins, inj_bins, n_bins, index, v=None if v is None else v[p])
            hist_pe += one["hist_pe"]
            if hist_inj is not None:
                hist_inj += one["hist_inj"]
            dead += one["n_dead"]
            if v is not None:
                vsum += one["vsum"]
    live = (k - dead).astype(np.float64) if vsum is None else vsum
    area = np.stack([np.outer(np.diff(grid[x]), np.diff(grid[y])) for x, y in pair_names])
    result = {"pairs": pair_names, "edges": {p: grid[p] for p in names}}
    _point_weight_entries(result, loo, vsum)
    if loo is not None and "pareto_k" in loo:
        result["pareto_k"] = loo["pareto_k"]
    with np.errstate(invalid="ignore", divide="ignore"):
        events = hist_pe / live[:n_ev, None, None, None]
        result.update(events=events, events_density=events / area, outside={"events": 1.0 - events.sum(axis=(-2, -1))},
                      n_points={"events": (k - dead[:n_ev]).astype(np.int64)})
        if hist_inj is not None:
            predicted = hist_inj / live[n_ev]
            result.update(predicted=predicted, predicted_density=predicted / area)
            result["outside"]["predicted"] = 1.0 - predicted.sum(axis=(-2, -1))
            result["n_points"]["predicted"] = int(k - dead[n_ev])
    return result


def joint_check_summaries(obs, pred, live, point_weights=None, levels=(5, 50, 95)):
    """The host half of :func:`catalog_joint_check` on per-point tables ``obs``, ``pred (K, R, B, B)`` and ``live (K, 2)`` as
    ``Engine.point_histograms2d`` returns them.  A point without a live event or with a dead injection set is SKIPPED -- counted, never
    divided: its rows are NaN in every per-point output and it is left out of the bands and shares."""
    from . import draws as D

    obs, pred, live = np.asarray(obs, dtype=np.float64), np.asarray(pred, dtype=np.float64), np.asarray(live)
    k = obs.shape[0]
    if obs.ndim != 4 or pred.shape != obs.shape or live.shape != (k, 2) or k < 1:
        raise ValueError("obs and pred are (K, R, B, B) and live is (K, 2)")
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size < 1 or not np.all((levels >= 0.0) & (levels <= 100.0)):
        raise ValueError("levels must be percentiles in [0, 100]")
    if point_weights is None:
        v = np.ones(k)
    else:
        v = np.asarray(point_weights, dtype=np.float64)
        if v.shape != (k,) or not np.all(np.isfinite(v)) or np.any(v < 0.0) or not np.any(v > 0.0):
            raise ValueError(f"point_weights are ({k},) finite non-negative numbers, not all 0")
    no_event, no_inj = live[:, 0] == 0, live[:, 1] == 0
    used = ~(no_event | no_inj)
    hole = np.full(obs.shape[1:], np.nan)
    obs_u, pred_u = np.where(used[:, None, None, None], obs, hole), np.where(used[:, None, None, None], pred, hole)
    delta = obs_u - pred_u
    s_obs, s_pred = D.joint_table_summaries(obs_u), D.joint_table_summaries(pred_u)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = 0.5 * np.abs(obs_u / s_obs["total"][..., None, None] - pred_u / s_pred["total"][..., None, None]).sum(axis=(-2, -1))
        tv = np.where(used[:, None] & (s_obs["total"] > 0.0) & (s_pred["total"] > 0.0), tv, np.nan)
        has = ~np.isnan(delta)
        den = (v[:, None, None, None] * has).sum(axis=0)
        p_pos = (v[:, None, None, None] * (has & (np.where(has, delta, 0.0) > 0.0))).sum(axis=0) / den
    delta_mi = s_obs["mi"] - s_pred["mi"]
    q = levels / 100.0
    return {"levels": levels, "obs": obs_u, "pred": pred_u, "delta": delta, "bands_delta": D.weighted_percentiles(delta, v, q), "p_delta_positive": p_pos,
            "p_two_sided": 2.0 * np.minimum(p_pos, 1.0 - p_pos), "tv": tv, "bands_tv": D.weighted_percentiles(tv, v, q), "mi_obs": s_obs["mi"], "mi_pred": s_pred["mi"],
            "delta_mi": delta_mi, "bands_mi_obs": D.weighted_percentiles(s_obs["mi"], v, q), "bands_mi_pred": D.weighted_percentiles(s_pred["mi"], v, q),
            "bands_delta_mi": D.weighted_percentiles(delta_mi, v, q), "outside_obs": s_obs["outside"], "outside_pred": s_pred["outside"], "live": live,
            "n_skipped": int(np.count_nonzero(~used)), "n_skipped_no_event": int(np.count_nonzero(no_event)), "n_skipped_dead_injections": int(np.count_nonzero(no_inj)),
            "n_points": k}


def catalog_joint_check(eng, thetas, pe_values, edges, inj_values, pairs=None, param_names=None, point_weights=None, levels=(5, 50, 95), backend="device", total_inj=None):
    """Does the observed catalog fill the plane of two quantities the way the fitted population predicts for detected sources?  (DESIGN
    8o.)  Pearson's rho (:func:`catalog_correlation_check`), the conditional moments (:func:`catalog_conditional_check`) and Spearman's
    rho (:func:`catalog_rank_correlation_check`) compress the joint distribution to a number or two per pair; a dependence that is
    neither linear nor monotone -- a sub-population in one corner of the ``q``-``chi_eff`` plane -- shows only in the table itself.  Per
    hyper-posterior point k the device (``eng.point_histograms2d``) returns the observed table ``obs``, the equal-weight mixture of the
    live events' population-informed tables, and ``pred``, the injection set's table.

    ``thetas`` is ``(K, n_theta)``; ``pe_values``, ``inj_values`` (needed), ``edges``, ``param_names`` and ``pairs`` are
    :func:`event_joint_posteriors`'.  ``point_weights (K,)`` -- finite, non-negative, not all 0; default equal -- weight the points in the
    bands and shares; they are applied here and never go to the device.  ``levels`` are percentiles in ``[0, 100]``.  The device backend
    replaces the engine's histogram bins; the draw mask stays.  ``backend="host"`` runs the NumPy statement
    (:func:`gwinferno_amd.draws.point_histograms2d_reference`) on ``eng.log_weights``, without a mask: the statement the kernels are
    tested against, not a fall-back.

    Returns :func:`joint_check_summaries` of the tables with ``pairs`` and ``edges``: per point ``obs``, ``pred`` and ``delta = obs - pred
    (K, R, B, B)``; per cell ``bands_delta (Q, R, B, B)``, ``p_delta_positive`` and ``p_two_sided = 2 min(p, 1 - p) (R, B, B)``; per point
    and pair the total-variation distance of the tables renormalised to their in-range totals, ``tv = sum |obs / t_o - pred / t_p| / 2``,
    and the mutual informations ``mi_obs``, ``mi_pred``, ``delta_mi`` (:func:`gwinferno_amd.draws.joint_table_summaries`), each ``(K, R)``
    with ``bands_<key> (Q, R)``; ``outside_obs`` / ``outside_pred (K, R)``; the counts ``n_skipped``, ``n_skipped_no_event``,
    ``n_skipped_dead_injections`` of points without a live event or with a dead injection set, which are skipped (NaN rows), never
    divided; ``live (K, 2)`` and ``n_points``.

    The plug-in mutual information is biased UPWARD by roughly ``(cells - 1) / (2 n_eff)``, and the two sides have different ``n_eff``:
    the observed table rests on the events' PE samples, the predicted one on the found injections.  No correction is applied;
    ``log_nEffs (K, n_ev + 1)``, the engine's own log effective sample sizes per point -- the events, then the injection set, without
    the draw mask -- are returned beside it so that the size of the bias on either side can be judged (``total_inj`` is passed to
    ``eng.evaluate_batch``; the effective sizes do not depend on it)."""
    from . import draws as D

    thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, eng.n_theta)
    k = thetas.shape[0]
    if k < 1:
        raise ValueError("thetas holds no point")
    if backend not in ("device", "host"):
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    if inj_values is None:
        raise ValueError("the predicted table is the injection set's: inj_values is needed")
    names, pair_names, index, grid, n_bins, pe_bins, inj_bins = _joint_setup(eng, pe_values, inj_values, edges, pairs, param_names)
    if backend == "device":
        eng.set_histogram_bins(pe_bins, inj_bins, n_bins=n_bins)
        got = eng.point_histograms2d(thetas, index, accumulate=False)
        obs, pred, live = got["obs"], got["pred"], got["live"]
    else:
        shape = (k, len(pair_names), n_bins, n_bins)
        obs, pred, live = np.empty(shape), np.empty(shape), np.empty((k, 2), dtype=np.int32)
        for p, th in enumerate(thetas):
            lw_pe, lw_inj = eng.log_weights(th)
            one = D.point_histograms2d_reference(lw_pe, lw_inj, None, None, pe_bins, inj_bins, n_bins, index)
            obs[p], pred[p], live[p] = one["obs"], one["pred"], one["live"]
    out = joint_check_summaries(obs, pred, live, point_weights=point_weights, levels=levels)
    out.update(pairs=pair_names, edges={p: grid[p] for p in names})
    log_neffs = np.empty((k, eng.n_ev + 1))
    step = int(eng.max_batch)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, k, step):
            res = eng.evaluate_batch(thetas[k0 : k0 + step], float(eng.n_inj if total_inj is None else total_inj), min_neff_cut=False, max_variance_cut=False, want_grad=False)
            for i, r in enumerate(res):
                log_neffs[k0 + i, : eng.n_ev], log_neffs[k0 + i, eng.n_ev] = r.log_neffs, r.summary.log_nEff_inj
    out["log_nEffs"] = log_neffs
    return out
