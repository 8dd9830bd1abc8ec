"""CPU: linear weights per (point, segment) in the marginal weights and the weighted histograms, and the leave-one-out summary made of
them (include/gwi_engine.h: gwi_marginal_weights_add_weighted, gwi_weighted_histograms_weighted) -- the NumPy statements
(gwinferno_amd/draws.py: marginal_weights_reference, weighted_histograms_reference, leave_one_out_summary) alone: weights of 1, of
1/2 and of 0, the scores against a direct log-sum-exp, points that are not finite, the refusals of the Python layer, and the inputs
of tests/test_gpu_loo.py, which are vetted here."""
import math

import loo_util as LU
import numpy as np
import pytest

N_EV, N_PE, N_INJ, K, N_BINS = 2, 300, 500, 4, 5


def _inputs():
    """Log-weights of moderate spread (no weight near the subnormal range, where halving would round), one dead (point, event)."""
    rng = np.random.default_rng(8)
    lw_pe, lw_inj = rng.normal(0.0, 3.0, (K, N_EV, N_PE)), rng.normal(0.0, 3.0, (K, N_INJ))
    lw_pe[2, 1] = -np.inf
    pb, ib = rng.integers(0, N_BINS, (2, N_EV, N_PE)).astype(np.uint16), rng.integers(0, N_BINS, (2, N_INJ)).astype(np.uint16)
    pb[0, 0, ::7] = 0xFFFF
    pm, im = (rng.uniform(size=(N_EV, N_PE)) < 0.8).astype(np.uint8), (rng.uniform(size=N_INJ) < 0.8).astype(np.uint8)
    return lw_pe, lw_inj, pb, ib, pm, im


def _histograms(lw_pe, lw_inj, pm, im, pb, ib, v=None):
    """The statement of one point, summed over the points in order: (hist_pe, hist_inj, dead[, vsum])."""
    from gwinferno_amd.draws import weighted_histograms_reference

    total = None
    for p in range(lw_pe.shape[0]):
        one = weighted_histograms_reference(lw_pe[p], lw_inj[p], pm, im, pb, ib, N_BINS, v=None if v is None else v[p])
        total = list(one) if total is None else [a + b for a, b in zip(total, one)]
    return total


def _quantile_indices(W_pe, x):
    from gwinferno_amd.draws import weighted_quantiles_reference

    return np.stack([weighted_quantiles_reference(W_pe[ev], np.argsort(x[ev], kind="stable"), x[ev], LU.LEVELS)[0] for ev in range(W_pe.shape[0])])


@pytest.mark.parametrize("masked", (False, True))
def test_weights_of_one_are_the_statement_without_weights(masked):
    from gwinferno_amd.draws import marginal_weights_reference

    lw_pe, lw_inj, pb, ib, pm, im = _inputs()
    pm, im = (pm, im) if masked else (None, None)
    plain = marginal_weights_reference(lw_pe, lw_inj, pm, im)
    assert len(plain) == 4  # the return shape without v is today's
    for ones in (np.ones((K, N_EV + 1)), np.ones(K)):
        got = marginal_weights_reference(lw_pe, lw_inj, pm, im, v=ones)
        assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(plain, got[:4]))
        assert np.array_equal(got[4], plain[3] - plain[2]) and np.array_equal(got[5], got[4]) and plain[2][1] == 1  # vsum = n_points - dead
    h_plain, h_ones = _histograms(lw_pe, lw_inj, pm, im, pb, ib), _histograms(lw_pe, lw_inj, pm, im, pb, ib, np.ones((K, N_EV + 1)))
    assert len(h_plain) == 3 and len(h_ones) == 4 and all(np.array_equal(a, b) for a, b in zip(h_plain, h_ones[:3]))
    assert np.array_equal(h_ones[3], K - h_plain[2])


def test_weights_of_one_half_halve_every_sum():
    from gwinferno_amd.draws import marginal_weights_reference

    lw_pe, lw_inj, pb, ib, pm, im = _inputs()
    x = np.random.default_rng(9).normal(size=(N_EV, N_PE))
    plain = marginal_weights_reference(lw_pe, lw_inj, pm, im)
    half = marginal_weights_reference(lw_pe, lw_inj, pm, im, v=np.full((K, N_EV + 1), 0.5))
    assert np.array_equal(half[0], 0.5 * plain[0]) and np.array_equal(half[1], 0.5 * plain[1]) and np.array_equal(half[2], plain[2]) and half[3] == K
    assert np.array_equal(half[4], 0.5 * (K - plain[2])) and np.array_equal(half[5], 0.25 * (K - plain[2]))
    assert np.array_equal(_quantile_indices(half[0], x), _quantile_indices(plain[0], x))
    h_plain, h_half = _histograms(lw_pe, lw_inj, pm, im, pb, ib), _histograms(lw_pe, lw_inj, pm, im, pb, ib, np.full((K, N_EV + 1), 0.5))
    assert np.array_equal(h_half[0], 0.5 * h_plain[0]) and np.array_equal(h_half[1], 0.5 * h_plain[1]) and np.array_equal(h_half[2], h_plain[2])
    assert np.array_equal(h_half[3], 0.5 * (K - h_plain[2]))


def test_a_point_of_weight_zero_is_the_run_without_it():
    from gwinferno_amd.draws import marginal_weights_reference

    lw_pe, lw_inj, pb, ib, pm, im = _inputs()
    rng = np.random.default_rng(10)
    v = rng.uniform(0.1, 1.0, (K, N_EV + 1))
    for gone in (0, 2, K - 1):  # (at point 2 event 1 is dead: with weight 0 it is not counted)
        v0 = v.copy()
        v0[gone] = 0.0
        keep = [p for p in range(K) if p != gone]
        with_zero = marginal_weights_reference(lw_pe, lw_inj, pm, im, v=v0)
        without = marginal_weights_reference(lw_pe[keep], lw_inj[keep], pm, im, v=v[keep])
        assert all(np.array_equal(with_zero[i], without[i]) for i in (0, 1, 2, 4, 5)) and with_zero[3] == without[3] + 1 == K
        h_zero, h_without = _histograms(lw_pe, lw_inj, pm, im, pb, ib, v0), _histograms(lw_pe[keep], lw_inj[keep], pm, im, pb, ib, v[keep])
        assert all(np.array_equal(a, b) for a, b in zip(h_zero, h_without))
    # one segment's weight alone set to 0: that segment as without the point, the others as with it
    v0 = v.copy()
    v0[2, 1] = 0.0
    got, full = marginal_weights_reference(lw_pe, lw_inj, pm, im, v=v0), marginal_weights_reference(lw_pe, lw_inj, pm, im, v=v)
    assert full[2][1] == 1 and got[2][1] == 0 and np.array_equal(got[0], full[0]) and np.array_equal(got[4], full[4])


@pytest.mark.parametrize("k", (1, 5, 64, 1000))
def test_scores_against_a_direct_logsumexp(k):
    """elpd_loo = -log mean exp(-l) and lpd = log mean exp(l) on a table spread over +-300, where exp(l) itself overflows: within (K +
    8) 2^-52 relative of a direct log-sum-exp in extended precision (the summation bound for K positive terms); the weights are
    exp(-l + min l), at most 1 with the largest exactly 1, the last column all ones; neff_points = (sum v)^2 / sum v^2."""
    from gwinferno_amd.draws import leave_one_out_summary

    n_ev = 6
    ell = np.random.default_rng(100 + k).uniform(-300.0, 300.0, (k, n_ev))
    out = leave_one_out_summary(ell)
    v = out["point_weights"]
    assert v.shape == (k, n_ev + 1) and np.all(v[:, n_ev] == 1.0) and np.all(v >= 0.0) and np.all(v <= 1.0) and np.all(v[:, :n_ev].max(axis=0) == 1.0)
    assert np.array_equal(v[:, :n_ev], np.exp(-ell + ell.min(axis=0))) and out["log_l_event"].shape == (k, n_ev) and not out["n_bad"].any()
    tol = (k + 8) * 2.0**-52
    for e in range(n_ev):
        elpd, lpd = -(LU.logsumexp(-ell[:, e]) - math.log(k)), LU.logsumexp(ell[:, e]) - math.log(k)
        print(f"K = {k} event {e}: elpd_loo {out['elpd_loo'][e]!r} against {elpd!r}, lpd {out['lpd'][e]!r} against {lpd!r}, bound {tol:.2e} relative")
        assert abs(out["elpd_loo"][e] - elpd) <= tol * abs(elpd) and abs(out["lpd"][e] - lpd) <= tol * abs(lpd)
        assert out["elpd_loo"][e] <= out["lpd"][e] + tol * abs(lpd)  # (the harmonic mean lies below the arithmetic one)
        s1, s2 = v[:, e].astype(np.longdouble).sum(), (v[:, e].astype(np.longdouble) ** 2).sum()
        assert abs(out["neff_points"][e] - float(s1 * s1 / s2)) <= tol * float(s1 * s1 / s2) and 1.0 <= out["neff_points"][e] <= k * (1.0 + tol)


def test_points_that_are_not_finite_get_weight_zero():
    from gwinferno_amd.draws import leave_one_out_summary

    ell = np.random.default_rng(3).normal(0.0, 2.0, (6, 3))
    ell[1, 0], ell[4, 0], ell[2, 1] = np.nan, np.inf, -np.inf
    ell[:, 2] = np.nan
    out = leave_one_out_summary(ell)
    assert np.array_equal(out["n_bad"], [2, 1, 6])
    v = out["point_weights"]
    assert v[1, 0] == v[4, 0] == v[2, 1] == 0.0 and not v[:, 2].any() and np.all(v[:, 3] == 1.0) and np.all(np.isfinite(v))
    good = np.isfinite(ell)
    for e in (0, 1):  # the means run over the finite points
        col = ell[good[:, e], e]
        assert np.array_equal(v[good[:, e], e], leave_one_out_summary(col[:, None])["point_weights"][:, 0])
        assert out["elpd_loo"][e] == leave_one_out_summary(col[:, None])["elpd_loo"][0] and out["lpd"][e] == leave_one_out_summary(col[:, None])["lpd"][0]
    assert np.isnan(out["elpd_loo"][2]) and np.isnan(out["lpd"][2]) and out["neff_points"][2] == 0.0
    with pytest.raises(ValueError):
        leave_one_out_summary(np.zeros(3))


def test_refusals_of_the_python_layer():
    from gwinferno_amd.draws import marginal_weights_reference, point_weights_array, weighted_histograms_reference

    lw_pe, lw_inj, pb, ib, pm, im = _inputs()
    for bad in (np.ones((K, N_EV)), np.ones((K + 1, N_EV + 1)), np.ones(K + 1), np.ones((K, N_EV + 1, 1))):
        with pytest.raises(ValueError, match="shape"):
            marginal_weights_reference(lw_pe, lw_inj, None, None, v=bad)
    for wrong in (np.nan, -1e-300, np.nextafter(1.0, 2.0), np.inf, -np.inf):
        v = np.ones((K, N_EV + 1))
        v[1, 2] = wrong
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            marginal_weights_reference(lw_pe, lw_inj, None, None, v=v)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            weighted_histograms_reference(lw_pe[0], lw_inj[0], None, None, pb, ib, N_BINS, v=v[1])
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            point_weights_array(v[:, 2], K, N_EV + 1)
    with pytest.raises(ValueError, match="shape"):
        weighted_histograms_reference(lw_pe[0], lw_inj[0], None, None, pb, ib, N_BINS, v=np.ones(N_EV))
    got = point_weights_array([0.0, 0.25, 1.0, 0.5], K, N_EV + 1)
    assert got.shape == (K, N_EV + 1) and got.flags.c_contiguous and got.dtype == np.float64 and np.array_equal(got[:, 0], got[:, N_EV]) and got[1, 1] == 0.25


def test_postprocess_refuses_inconsistent_requests():
    """leave_one_out=True needs total_inj and makes its own weights: both refusals come before the engine is touched."""
    from gwinferno_amd import postprocess as P

    class Shape:
        n_theta, n_ev, n_pe, n_inj = 2, 1, 4, 4

    x = {"a": np.arange(4.0)[None]}
    for call in (lambda **kw: P.event_credible_intervals(Shape(), np.zeros((2, 2)), x, **kw),
                 lambda **kw: P.event_posterior_densities(Shape(), np.zeros((2, 2)), x, np.linspace(0.0, 1.0, 3), **kw),
                 lambda **kw: P.reweighted_event_posteriors(Shape(), np.zeros((2, 2)), x, {"a": np.linspace(0.0, 4.0, 3)}, **kw)):
        with pytest.raises(ValueError, match="total_inj"):
            call(leave_one_out=True)
        with pytest.raises(ValueError, match="point_weights must be None"):
            call(leave_one_out=True, total_inj=10.0, point_weights=np.ones(2))
        with pytest.raises(ValueError, match="shape"):
            call(point_weights=np.ones(3))
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            call(point_weights=np.array([0.5, 1.5]))


def test_new_symbols_in_binding_and_header():
    import os

    from gwinferno_amd import _native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gwi_engine.h")).read()
    for sym in ("gwi_marginal_weights_add_weighted", "gwi_marginal_point_weights", "gwi_weighted_histograms_weighted"):
        assert sym in _native.EXPORTED_SYMBOLS and sym + "(gwi_handle h" in hdr


def test_inputs_of_the_gpu_tests():
    """The catalog, the weights and the bins of tests/test_gpu_loo.py: the shapes; every leave-one-out catalog builds the redshift
    model of the full one (the same range and grid: loo_util.catalog); the weights lie in [2^-20, 1] or are 0; samples lie outside the
    edges and inside."""
    from gwinferno_amd.draws import OUTSIDE_BIN

    pe, inj, total = LU.catalog()
    assert pe["mass_1"].shape == (LU.N_EV, LU.N_PE) == (3, 1500) and inj["mass_1"].shape == (LU.N_INJ,) == (2500,) and LU.K == 5 and total > LU.N_INJ
    assert LU.N_PE > 1024 and LU.N_PE % 1024 and LU.N_PE % 4 == 0 and LU.N_INJ % 1024
    for name in LU.COMPS:
        full = LU.composition(name, engine=False).z_model
        for e in range(LU.N_EV):
            part = LU.composition(name, without=e, engine=False).z_model
            assert part.zmin == full.zmin and part.zmax == full.zmax and np.array_equal(part.zs, full.zs), (name, e)
    v = LU.point_weights()
    assert v.shape == (LU.K, LU.N_EV + 1) and np.count_nonzero(v == 0.0) == 3 and v.max() == 1.0 and v[v > 0].min() == 2.0**-20
    assert v[1, 0] == 0.0 and v[2, LU.DEAD_EVENT] == 0.0 and v[3, LU.N_EV] == 0.0
    pb, ib = LU.bins()
    for b in (pb, ib):
        assert np.any(b == OUTSIDE_BIN) and set(np.unique(b)) == set(range(LU.N_BINS)) | {OUTSIDE_BIN}
    pm, im = LU.dead_mask()
    assert not pm[LU.DEAD_EVENT].any() and pm.sum() == (LU.N_EV - 1) * LU.N_PE and im.all()
