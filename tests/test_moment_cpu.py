"""CPU: per-point moments (include/gwi_engine.h: gwi_point_moments; gwinferno_amd/csrc/gwi_moment.h) -- the NumPy statement
alone (gwinferno_amd/draws.py: moments_segment, point_moments_reference) against np.average / np.cov, its exact cases, the digits a
two-pass covariance keeps, the derived device tolerance, the host backend of postprocess.catalog_correlation_check and
postprocess.event_variance_split on a stub engine, and the header, the exports and the refusals that need no device."""
import os
import re

import moment_util as MU
import numpy as np
import pytest
import test_pit_cpu as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segments(seed=3, n_ev=3, n_pe=300, n_inj=500, n_cols=4):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(2.0, 1.5, (n_cols, n_ev, n_pe)), rng.normal(-1.0, 0.7, (n_cols, n_inj))
    x_pe[1] += 0.6 * x_pe[0]  # (correlated columns)
    x_inj[1] -= 0.4 * x_inj[0]
    return rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj), x_pe, x_inj


def test_the_statement_against_numpy():
    """Seeded inputs, with and without masks: per segment the mean is np.average and the covariance np.cov(x, aweights=w, ddof=0), to 1e-12
    of sum w^ |x_c| and of sum w^ |x_c - m_c||x_d - m_d|; the covariance is symmetric to the bit; nothing is dead."""
    from gwinferno_amd import draws as D

    lw_pe, lw_inj, x_pe, x_inj = _segments()
    rng = np.random.default_rng(5)
    pm, im = (rng.uniform(size=lw_pe.shape) < 0.7).astype(np.uint8), (rng.uniform(size=lw_inj.shape) < 0.5).astype(np.uint8)
    for masks in ((None, None), (pm, im)):
        mean, cov, dead = D.point_moments_reference(lw_pe, lw_inj, x_pe, x_inj, *masks)
        assert mean.shape == (4, 4) and cov.shape == (4, 4, 4) and dead.shape == (4,) and dead.dtype == np.int32 and not dead.any()
        assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
        for seg in range(4):
            w = D.draw_weights(lw_pe[seg], None if masks[0] is None else masks[0][seg]) if seg < 3 else D.draw_weights(lw_inj, masks[1])
            x = x_pe[:, seg] if seg < 3 else x_inj
            share = w / w.sum()
            want_mean, want_cov = np.average(x, axis=1, weights=w), np.cov(x, aweights=w, ddof=0)
            d = np.abs(x - want_mean[:, None])
            assert np.all(np.abs(mean[seg] - want_mean) <= 1e-12 * (share * np.abs(x)).sum(axis=1))
            assert np.all(np.abs(cov[seg] - want_cov) <= 1e-12 * np.einsum("i,ci,di->cd", share, d, d))


def test_exact_cases():
    """One live sample: the mean is the sample and the covariance exactly 0, whatever its log-weight and wherever it sits.  A segment
    without weight (masked, -inf, NaN) gives NaN and is counted; the others do not move.  A set without columns gives NaN and its flags
    still tell the weight."""
    from gwinferno_amd import draws as D

    lw_pe, lw_inj, x_pe, x_inj = _segments()
    pm = np.ones(lw_pe.shape, dtype=np.uint8)
    pm[0] = 0
    pm[0, 217] = 1
    lw = lw_pe.copy()
    lw[1, ::2], lw[1, 1::2] = -np.inf, np.nan
    mean, cov, dead = D.point_moments_reference(lw, lw_inj, x_pe, x_inj, pm, None)
    assert np.array_equal(dead, [0, 1, 0, 0])
    assert np.array_equal(mean[0], x_pe[:, 0, 217]) and np.array_equal(cov[0], np.zeros((4, 4)))
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(cov[1]))
    free = D.point_moments_reference(lw_pe, lw_inj, x_pe, x_inj)
    assert np.array_equal(mean[2:], free[0][2:]) and np.array_equal(cov[2:], free[1][2:])
    only = D.point_moments_reference(lw, lw_inj, None, x_inj, pm, None)
    assert np.all(np.isnan(only[0][:3])) and np.array_equal(only[0][3], free[0][3]) and np.array_equal(only[2], dead)
    m, v, alive = D.moments_segment(np.zeros(5), np.ones((2, 5)))
    assert not alive and np.all(np.isnan(m)) and np.all(np.isnan(v))
    with pytest.raises(ValueError, match="both None"):
        D.point_moments_reference(lw, lw_inj, None, None)


def test_two_passes_keep_the_digits_of_a_column_far_from_zero():
    """x_n = 1e6 + 1e-3 n, n = 0 ... 1999, equal weights: the variance is 1e-6 (N^2 - 1) / 12 and the two-pass statement keeps it to 1e-9
    relative (the spacing of the doubles near 1e6 is 1.2e-10, a relative 1.2e-7 of the step, which averages out).  The one-pass formula
    E[x^2] - E[x]^2 subtracts two numbers near 1e12 whose spacing is 1.2e-4: nothing of the variance of 0.33 survives to 1e-9, and this
    test says so -- the reason gwi_moment.h centres on a first-pass mean."""
    from gwinferno_amd import draws as D

    n = 2000
    x = (1.0e6 + 1.0e-3 * np.arange(n))[None, :]
    exact = 1.0e-6 * (n * n - 1.0) / 12.0
    mean, cov, alive = D.moments_segment(np.ones(n), x)
    assert alive and abs(cov[0, 0] - exact) <= 1e-9 * exact and abs(mean[0] - (1.0e6 + 1.0e-3 * (n - 1) / 2.0)) <= 1e-9
    one_pass = np.mean(x[0] * x[0]) - np.mean(x[0]) ** 2
    assert abs(one_pass - exact) > 1e-6 * exact  # (measured: off by more than a part in a thousand)


def test_the_device_tolerance_is_a_rounding_bound():
    """moment_util's bounds are counts of roundings: the sums' depth is 3 + 6 + 3 + n_tiles, one more tile adds half a unit, one more live
    sample one unit, and with every sample of the GPU tests' largest segment live the relative bound stays below 1e-12 -- nothing can
    hide under it."""
    assert MU.sum_depth(2) == 14 and MU.sum_depth(3) == 15
    assert MU.mean_units(10, 3) - MU.mean_units(10, 2) == 0.5 and MU.mean_units(11, 2) - MU.mean_units(10, 2) == 1.0
    assert MU.cov_units(10, 2) - MU.mean_units(10, 2) == 3.0
    assert (MU.N_INJ + 8) < MU.cov_units(MU.N_INJ, 3) < MU.N_INJ + 30 and 1.01 * MU.cov_units(MU.N_INJ, 3) * MU.U < 1e-12
    pm, im = MU.masks("masked")
    assert not pm[MU.DEAD_EVENT].any() and pm[MU.SINGLE_EVENT].sum() == 1 and pm[MU.SINGLE_EVENT, MU.SINGLE_SAMPLE] == 1 and MU.SINGLE_SAMPLE >= MU.TILE
    assert 0 < MU.N_PE % MU.TILE and -(-MU.N_PE // MU.TILE) == 2 and 0 < MU.N_INJ % MU.TILE and -(-MU.N_INJ // MU.TILE) == 3
    x_pe, x_inj = MU.columns(8)
    assert x_pe.shape == (8, MU.N_EV, MU.N_PE) and x_inj.shape == (8, MU.N_INJ) and x_pe[0].min() > MU.OFFSET and np.array_equal(MU.columns(3)[0], x_pe[:3])


def _stub(k=6, seed=9, n_ev=4, n_pe=50, n_inj=80):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(0.0, 1.0, (3, n_ev, n_pe)), rng.normal(0.0, 1.2, (3, n_inj))
    lw_pe, lw_inj = rng.normal(0.0, 1.0, (k, n_ev, n_pe)), rng.normal(0.0, 1.0, (k, n_inj))
    eng = TP._StubEngine(lw_pe, lw_inj, rng.normal(0.0, 1.0, (k, n_ev)), rng.normal(-3.0, 0.2, k))
    names = ("a", "b", "c")
    return eng, np.arange(k, dtype=np.float64)[:, None], {n: x_pe[i] for i, n in enumerate(names)}, {n: x_inj[i] for i, n in enumerate(names)}


def test_catalog_correlation_check_on_the_host():
    """Shapes and what the entries say on the stub engine; the raw arrays are the statement's; mu_obs and Sigma_obs are the moments of
    the pooled sample of the live events with weight w_i / (S_e n_live); named and indexed pairs agree; a point of weight 0 leaves the
    shares as without it; a dead event is left out of the mixture; a zero-variance column is flagged and not divided; without
    inj_values the predicted side is NaN."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values = _stub()
    k, n_ev = thetas.shape[0], eng.n_ev
    r = P.catalog_correlation_check(eng, thetas, pe_values, inj_values=inj_values, backend="host")
    assert r["names"] == ["a", "b", "c"] and np.array_equal(r["pairs"], [[0, 1], [0, 2], [1, 2]]) and r["n_points"] == k and r["dead_detected"] == 0
    for key in ("rho_obs", "rho_det", "delta", "cov_obs", "cov_det", "delta_cov", "degenerate_obs", "degenerate_det"):
        assert r[key].shape == (k, 3), key
    for key in ("bands_rho_obs", "bands_rho_det", "bands_delta", "bands_cov_obs", "bands_cov_det", "bands_delta_cov"):
        assert r[key].shape == (3, 3) and np.all(np.diff(r[key], axis=0) >= 0.0), key
    assert np.array_equal(r["delta"], r["rho_obs"] - r["rho_det"]) and np.all(np.abs(r["rho_obs"]) <= 1.0) and not r["degenerate_obs"].any()
    assert np.array_equal(r["n_live"], np.full(k, n_ev)) and np.array_equal(r["p_two_sided"], 2.0 * np.minimum(r["p_delta_positive"], 1.0 - r["p_delta_positive"]))
    assert np.array_equal(r["p_delta_positive"], (r["delta"] > 0.0).mean(axis=0))
    x_pe, x_inj = np.stack([pe_values[n] for n in "abc"]), np.stack([inj_values[n] for n in "abc"])
    for i in range(k):
        mean, cov, dead = D.point_moments_reference(eng.lw_pe[i], eng.lw_inj[i], x_pe, x_inj)
        assert np.array_equal(mean, r["point_mean"][i]) and np.array_equal(cov, r["point_cov"][i]) and np.array_equal(dead, r["dead"][i])
        w = np.concatenate([D.draw_weights(eng.lw_pe[i, e]) / D.draw_weights(eng.lw_pe[i, e]).sum() / n_ev for e in range(n_ev)])
        pooled = x_pe.reshape(3, -1)
        assert np.allclose(r["mu_obs"][i], np.average(pooled, axis=1, weights=w), rtol=1e-12, atol=1e-14)
        assert np.allclose(r["sigma_obs"][i], np.cov(pooled, aweights=w, ddof=0), rtol=1e-11, atol=1e-14)
        s = np.cov(x_inj, aweights=D.draw_weights(eng.lw_inj[i]), ddof=0)
        assert np.allclose(r["sigma_det"][i], s, rtol=1e-11, atol=1e-14)
        assert np.allclose(r["rho_det"][i], (s / np.sqrt(np.outer(np.diag(s), np.diag(s))))[[0, 0, 1], [1, 2, 2]], rtol=1e-11, atol=1e-13)
    named = P.catalog_correlation_check(eng, thetas, pe_values, inj_values=inj_values, pairs=[("a", "c"), (2, 1)], backend="host")
    assert np.array_equal(named["pairs"], [[0, 2], [2, 1]]) and np.array_equal(named["rho_obs"][:, 0], r["rho_obs"][:, 1]) and np.array_equal(named["rho_obs"][:, 1], r["rho_obs"][:, 2])
    v = np.ones(k)
    v[2] = 0.0
    weighted = P.catalog_correlation_check(eng, thetas, pe_values, inj_values=inj_values, point_weights=v, backend="host")
    keep = np.arange(k) != 2
    assert np.array_equal(weighted["p_delta_positive"], (r["delta"][keep] > 0.0).mean(axis=0)) and np.array_equal(weighted["rho_obs"], r["rho_obs"])
    assert np.array_equal(weighted["bands_delta"], D.weighted_percentiles(r["delta"][keep], np.ones(k - 1), r["levels"]))
    # a dead event at one point is left out of that point's mixture; a constant column is flagged, not divided
    eng.lw_pe[1, 0] = -np.inf
    flat = dict(pe_values, c=np.full_like(pe_values["c"], 3.0))
    d = P.catalog_correlation_check(eng, thetas, flat, backend="host")
    assert np.array_equal(d["n_live"], [n_ev, n_ev - 1] + [n_ev] * (k - 2)) and d["dead"][1, 0] == 1 and np.all(np.isnan(d["rho_det"])) and d["dead_detected"] == k
    assert np.all(d["degenerate_obs"][:, 1:] == 1) and not d["degenerate_obs"][:, 0].any() and np.all(np.isnan(d["rho_obs"][:, 1:])) and np.all(np.abs(d["cov_obs"][:, 1:]) < 1e-15)
    others = [e for e in range(1, n_ev)]
    w = np.concatenate([D.draw_weights(eng.lw_pe[1, e]) / D.draw_weights(eng.lw_pe[1, e]).sum() for e in others])
    assert np.allclose(d["mu_obs"][1, :2], np.average(np.stack([flat[n][others].ravel() for n in "ab"]), axis=1, weights=w), rtol=1e-12)
    for bad in (dict(pairs=[(0, 3)]), dict(pairs=[]), dict(point_weights=np.zeros(k)), dict(levels=(1.5,)), dict(backend="cuda"), dict(param_names=["a", "zz"])):
        with pytest.raises(ValueError):
            P.catalog_correlation_check(eng, thetas, pe_values, **bad)


def test_catalog_correlation_check_recovers_a_known_correlation():
    """20 events of 400 samples and 4 000 injections drawn from ONE bivariate normal with rho = -0.6, flat log-weights (the population
    does not reweight): rho_obs and rho_det are the sample correlations, both within 4 standard errors (1 - rho^2) / sqrt(n) of -0.6,
    and delta is 0 within their combined error, so neither tail probability is reported as extreme from a shared truth: delta's sign is
    the same at every point (the points do not differ), and the third, independent column is uncorrelated with both."""
    from gwinferno_amd import postprocess as P

    rng = np.random.default_rng(21)
    rho, n_ev, n_pe, n_inj, k = -0.6, 20, 400, 4000, 4
    chol = np.linalg.cholesky(np.array([[1.0, rho, 0.0], [rho, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    pe, inj = np.einsum("cd,dep->cep", chol, rng.normal(size=(3, n_ev, n_pe))), chol @ rng.normal(size=(3, n_inj))
    eng = TP._StubEngine(np.zeros((k, n_ev, n_pe)), np.zeros((k, n_inj)))
    r = P.catalog_correlation_check(eng, np.arange(k, dtype=np.float64)[:, None], {n: pe[i] for i, n in enumerate("xyz")}, inj_values={n: inj[i] for i, n in enumerate("xyz")},
                                    backend="host")
    se_obs, se_det = (1.0 - rho * rho) / np.sqrt(n_ev * n_pe), (1.0 - rho * rho) / np.sqrt(n_inj)
    assert np.all(np.abs(r["rho_obs"][:, 0] - rho) <= 4.0 * se_obs) and np.all(np.abs(r["rho_det"][:, 0] - rho) <= 4.0 * se_det)
    assert np.all(np.abs(r["delta"][:, 0]) <= 4.0 * np.hypot(se_obs, se_det))
    assert np.all(np.abs(r["rho_obs"][:, 1:]) <= 4.0 / np.sqrt(n_ev * n_pe)) and np.all(np.abs(r["rho_det"][:, 1:]) <= 4.0 / np.sqrt(n_inj))
    assert np.allclose(r["rho_obs"][:, 0], np.corrcoef(pe[0].ravel(), pe[1].ravel())[0, 1], rtol=1e-12)
    assert np.all(np.isin(r["p_delta_positive"], (0.0, 1.0))) and np.array_equal(r["bands_delta"][0], r["bands_delta"][-1])


def test_event_variance_split_on_the_host():
    """within + between == total to the bit; total and mean are the variance and mean of the pooled weighted sample with weights v_k w_ki
    / S_ke (the law of total variance), for equal, (K,), (K, n_ev + 1), leave-one-out and Pareto-smoothed weights; a dead (point, event)
    is skipped and counted; one point alone has no between part; the refusals of the user-facing function."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, _ = _stub()
    k, n_ev = thetas.shape[0], eng.n_ev
    x_pe = np.stack([pe_values[n] for n in "abc"])
    rng = np.random.default_rng(13)
    loo = D.leave_one_out_summary(eng.log_bfs - eng.log_mu[:, None])["point_weights"]
    psis = D.pareto_smoothed_summary(eng.log_bfs - eng.log_mu[:, None])
    cases = ((dict(), np.ones((k, n_ev))), (dict(point_weights=np.linspace(0.2, 1.0, k)), np.tile(np.linspace(0.2, 1.0, k)[:, None], (1, n_ev))),
             (dict(leave_one_out=True, total_inj=1000.0), loo[:, :n_ev]), (dict(leave_one_out="psis", total_inj=1000.0), psis["point_weights"][:, :n_ev]))
    full = rng.uniform(0.1, 1.0, (k, n_ev + 1))
    cases += ((dict(point_weights=full), full[:, :n_ev]),)
    for kw, v in cases:
        r = P.event_variance_split(eng, thetas, pe_values, backend="host", **kw)
        assert r["names"] == ["a", "b", "c"] and r["n_points"] == k and not r["n_dead"].any() and ("elpd_loo" in r) == ("leave_one_out" in kw)
        assert ("pareto_k" in r) == (kw.get("leave_one_out") == "psis")
        assert np.array_equal(r["within"] + r["between"], r["total"]) and np.all(r["within"] > 0.0) and np.all(r["between"] >= 0.0)
        assert np.allclose(r["fraction_between"], r["between"] / r["total"], rtol=1e-15) and np.allclose(r["neff_points"], v.sum(axis=0) ** 2 / (v * v).sum(axis=0), rtol=1e-13)
        for e in range(n_ev):
            w = np.concatenate([v[i, e] * D.draw_weights(eng.lw_pe[i, e]) / D.draw_weights(eng.lw_pe[i, e]).sum() for i in range(k)])
            pooled = np.tile(x_pe[:, e], (1, k))
            assert np.allclose(r["mean"][e], np.average(pooled, axis=1, weights=w), rtol=1e-12, atol=1e-14)
            assert np.allclose(r["total"][e], np.diag(np.atleast_2d(np.cov(pooled, aweights=w, ddof=0))), rtol=1e-11)
    one = P.event_variance_split(eng, thetas[:1], pe_values, backend="host")
    assert np.all(one["between"] == 0.0) and np.array_equal(one["total"], one["within"]) and np.all(one["fraction_between"] == 0.0)
    eng.lw_pe[2, 1] = np.nan
    d = P.event_variance_split(eng, thetas, pe_values, backend="host")
    assert np.array_equal(d["n_dead"], [0, 1, 0, 0]) and np.isclose(d["neff_points"][1], k - 1) and np.all(np.isfinite(d["total"]))
    rest = P.event_variance_split(eng, thetas[np.arange(k) != 2], pe_values, backend="host")
    assert np.allclose(d["total"][1], rest["total"][1], rtol=1e-13) and np.allclose(d["between"][1], rest["between"][1], rtol=1e-12, atol=1e-16)
    for bad in (dict(leave_one_out="loo"), dict(leave_one_out=True), dict(leave_one_out="psis", total_inj=1.0, point_weights=np.ones(k)), dict(backend="gpu"),
                dict(point_weights=np.ones(k + 1))):
        with pytest.raises(ValueError):
            P.event_variance_split(eng, thetas, pe_values, **bad)


def test_header_library_and_refusals_without_a_device():
    """The two exports are declared, bound and listed, with their argument counts; the ABI version stays 3; a null handle and a host-only
    handle answer GWI_ERR_INVALID, the latter with a message, and write nothing; the Python layer refuses an engine that holds a shard in
    the words of its neighbours, and a call before columns are set."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_point_moments", 5), ("gwi_point_moment_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_moments.restype is C.c_int32 and lib.gwi_point_moment_times.restype is None
    assert "DESIGN 8j" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_moments(None, None, 1, None, None) == -1
    eng = MU.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    try:
        i32 = C.POINTER(C.c_int32)
        out, dead = np.full((1, MU.N_EV + 1, 2), 7.0), np.full((1, MU.N_EV + 1), 7, dtype=np.int32)
        assert lib.gwi_point_moments(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(out), dead.ctypes.data_as(i32)) == -1
        assert "gwi_point_moments: host-only handle: no device to sum on" in lib.gwi_last_error(eng.handle).decode() and np.all(out == 7.0) and np.all(dead == 7)
        with pytest.raises(ValueError, match="thetas has shape"):
            eng.point_moments(np.zeros(eng.n_theta + 1))
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_moments: this engine holds one shard of the catalog; the injection moments need the global set"):
        shard.point_moments(np.zeros(3))
