"""CPU: Pareto smoothing of importance weights on the point axis (gwinferno_amd/draws.py: pareto_smooth, pareto_smoothed_summary;
gwinferno_amd/postprocess.py: pareto_smoothed_loo_weights) -- the fitted shape on samples whose shape is known, and the
structural properties of the smoothed weights."""
import math
import types

import numpy as np
import pytest

# twice the largest |khat - target| found on the cases of the first test (0.0176, at K = 1 000 and k = 0.9; the table is in
# profiles/point_ranks/RESULTS.md): a fit that drifts past it has changed.  Far below 0.05, at which the fit would count as wrong.
KHAT_DEVIATION = 2 * 0.0177


def _tail_size(k_points):
    return min(k_points // 5, int(math.ceil(3.0 * math.sqrt(k_points))))


def _gpd_quantiles(k_points, shape):
    p = (np.arange(1, k_points + 1, dtype=np.float64) - 0.5) / k_points
    return ((1.0 - p) ** (-shape) - 1.0) / shape


@pytest.mark.parametrize("k_points", (1000, 4000))
@pytest.mark.parametrize("shape", (0.2, 0.6, 0.9))
def test_khat_of_generalised_pareto_quantiles(k_points, shape):
    """Ratios that ARE the quantiles of a generalised Pareto distribution of known shape k (its tail above any threshold has the same
    shape): khat lands in the diagnostic class of the ANALYTIC target (M k + 5) / (M + 10), the fit pulled towards 0.5 by its weakly
    informative prior, which leaves at least 0.09 of room to either class boundary; and within KHAT_DEVIATION of it."""
    from gwinferno_amd.draws import pareto_smooth

    m = _tail_size(k_points)
    target = (m * shape + 5.0) / (m + 10.0)
    edges = (0.5, 0.7)
    assert min(abs(target - e) for e in edges) >= 0.09
    ratios = _gpd_quantiles(k_points, shape)
    lw, khat = pareto_smooth(np.log(ratios)[:, None])
    print(f"K = {k_points}, k = {shape}: M = {m}, khat = {khat[0]:.4f}, target = {target:.4f}, deviation = {khat[0] - target:+.4f}")
    assert lw.shape == (k_points, 1) and khat.shape == (1,)
    assert np.searchsorted(edges, khat[0]) == np.searchsorted(edges, target)
    assert abs(khat[0] - target) <= KHAT_DEVIATION < 0.05


def test_structure_of_the_smoothed_weights():
    """Entries outside the tail keep the bits of the shifted input; the smoothed tail does not decrease along the raw order and stays at
    or below the raw maximum (0 after the shift); a constant added to a column moves khat by rounding only and the weights not at all
    beyond it; columns are treated one by one; fewer than five tail points (K < 25) or a constant tail give khat = inf and untouched
    weights; non-finite input is refused."""
    from gwinferno_amd.draws import pareto_smooth

    rng = np.random.default_rng(6)
    k_points = 400
    m = _tail_size(k_points)
    lr = np.stack([np.log(_gpd_quantiles(k_points, 0.7))[rng.permutation(k_points)], rng.normal(0.0, 1.0, k_points), rng.standard_cauchy(k_points)], axis=1)
    lw, khat = pareto_smooth(lr)
    assert lw.shape == lr.shape and khat.shape == (3,) and np.all(np.isfinite(khat)) and khat[1] < 0.5 < khat[2]
    for c in range(3):
        shifted = lr[:, c] - lr[:, c].max()
        order = np.argsort(shifted, kind="stable")
        body, tail = order[: k_points - m], order[k_points - m :]
        assert np.array_equal(lw[body, c], shifted[body])
        assert np.all(np.diff(lw[tail, c]) >= 0.0) and lw[tail, c].max() <= 0.0 and lw[tail[0], c] >= shifted[body[-1]]
        assert not np.array_equal(lw[tail, c], shifted[tail])
        alone, k_alone = pareto_smooth(lr[:, c : c + 1])
        assert np.array_equal(alone[:, 0], lw[:, c]) and k_alone[0] == khat[c]
    moved, k_moved = pareto_smooth(lr + np.array([1e3, -40.0, 0.125]))
    assert np.allclose(k_moved, khat, rtol=0.0, atol=1e-9) and np.allclose(moved, lw, rtol=0.0, atol=1e-9)
    small = rng.normal(0.0, 1.0, (24, 2))
    lw_s, k_s = pareto_smooth(small)
    assert np.all(np.isinf(k_s)) and np.array_equal(lw_s, small - small.max(axis=0))
    flat = np.concatenate([rng.normal(-3.0, 0.1, 400 - m), np.zeros(m)])[:, None]
    lw_f, k_f = pareto_smooth(flat)
    assert np.isinf(k_f[0]) and np.array_equal(lw_f, flat)
    for bad in (np.zeros(5), np.zeros((0, 2)), np.array([[0.0], [np.inf]]), np.array([[0.0], [np.nan]])):
        with pytest.raises(ValueError):
            pareto_smooth(bad)


class _TableEngine:
    """What leave_one_out_weights needs of an engine: per-event log Bayes factors and the detection efficiency of evaluate_batch."""

    def __init__(self, log_bfs, log_mu):
        self.log_bfs, self.log_mu = log_bfs, log_mu
        self.n_ev = self.n_ev_global = log_bfs.shape[1]
        self.n_theta, self.max_batch = 1, 64

    def evaluate_batch(self, thetas, total_inj, **kw):
        assert kw["want_grad"] is False and kw["min_neff_cut"] is False
        return [types.SimpleNamespace(log_bfs=self.log_bfs[int(t[0])], summary=types.SimpleNamespace(log_det_eff=self.log_mu[int(t[0])], log_nEff_inj=np.log(50.0))) for t in thetas]


def test_pareto_smoothed_loo_weights():
    """K = 300 points, four events whose l_ke have tails of different weight and one point at which an event's l is not finite: the
    weights lie in [0, 1] with each event's maximum exactly 1 and the injection column all ones, so point_weights_array takes them;
    pareto_k is finite, below 0.5 for the two narrow tables and above 0.7 for the widest; the body of every event's weights is leave_one_out_weights' up to the common
    scale; elpd_loo and neff_points are those of the smoothed weights; lpd, n_bad and log_l_event are unchanged."""
    from gwinferno_amd import postprocess as P
    from gwinferno_amd.draws import point_weights_array

    rng = np.random.default_rng(9)
    k_points, n_ev = 300, 4
    ell = np.stack([rng.normal(0.0, s, k_points) for s in (0.1, 0.5, 1.5, 3.0)], axis=1)
    ell[7, 2] = -np.inf
    eng = _TableEngine(ell + 2.0, np.full(k_points, 2.0))  # l = logBF - log mu
    thetas = np.arange(k_points, dtype=np.float64)[:, None]
    raw, out = P.leave_one_out_weights(eng, thetas, 1000.0), P.pareto_smoothed_loo_weights(eng, thetas, 1000.0)
    v = out["point_weights"]
    assert v.shape == (k_points, n_ev + 1) and np.all((v >= 0.0) & (v <= 1.0)) and np.array_equal(v.max(axis=0), np.ones(n_ev + 1)) and np.all(v[:, n_ev] == 1.0)
    assert np.array_equal(point_weights_array(v, k_points, n_ev + 1), v) and v[7, 2] == 0.0
    assert out["pareto_k"].shape == (n_ev,) and np.all(np.isfinite(out["pareto_k"])) and np.all(out["pareto_k"][:2] < 0.5) and out["pareto_k"][3] > 0.7
    assert np.array_equal(out["log_l_event"], raw["log_l_event"]) and np.array_equal(out["lpd"], raw["lpd"]) and np.array_equal(out["n_bad"], [0, 0, 1, 0])
    for e in range(n_ev):
        good = np.isfinite(ell[:, e])
        body = np.argsort(-ell[good, e], kind="stable")[: good.sum() - _tail_size(int(good.sum()))]
        ratio = v[good, e][body] / raw["point_weights"][good, e][body]
        assert np.allclose(ratio, ratio[0], rtol=1e-12, atol=0.0) and ratio[0] >= 1.0 - 1e-12  # (the smoothed maximum is at or below the raw one)
        ve, le = v[good, e], ell[good, e]
        assert out["elpd_loo"][e] == pytest.approx(math.log(np.sum(ve * np.exp(le)) / np.sum(ve)), rel=1e-12, abs=1e-12)
        assert out["neff_points"][e] == pytest.approx(np.sum(ve) ** 2 / np.sum(ve * ve), rel=1e-12)
    assert abs(out["elpd_loo"][0] - raw["elpd_loo"][0]) < 1e-3 and abs(out["elpd_loo"][3] - raw["elpd_loo"][3]) > 1e-6
