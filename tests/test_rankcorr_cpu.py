"""CPU: per-point rank correlations (include/gwi_engine.h: gwi_set_rankcorr_columns, gwi_point_rank_correlations; gwinferno_amd/csrc/
gwi_rankcorr.h) -- the NumPy statement alone (gwinferno_amd/draws.py: rankcorr_codes, rankcorr_set,
point_rank_correlations_reference) against scipy.stats.spearmanr, against a dataset with every sample repeated its weight's number of
times, its exact cases, monotone maps, pooling, the host backend of postprocess.catalog_rank_correlation_check on a stub engine, the
derived bounds, and the header, the exports and the refusals that need no device."""
import os
import re

import numpy as np
import pytest
import rankcorr_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rho(out, n_cols):
    from gwinferno_amd.draws import rankcorr_matrix

    _, _, r = rankcorr_matrix(out, n_cols)
    s = np.sqrt(np.diagonal(r, axis1=-2, axis2=-1))
    return r / (s[..., :, None] * s[..., None, :])


def _data(seed=2, n=900, heavy=False):
    """three columns: the second depends on the first (not linearly), the third on neither; ``heavy``: every column rounded so that a
    value is shared by dozens of members"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (3, n))
    x[1] = np.exp(0.8 * x[0]) + 0.5 * rng.normal(size=n)
    return np.round(2.0 * x) / 2.0 if heavy else x


@pytest.mark.parametrize("heavy", (False, True))
def test_equal_weights_against_scipy(heavy):
    """With equal weights the weighted mid-rank is (average rank - 1/2) / n, a linear function of scipy's average rank, so rho is
    scipy.stats.spearmanr's, to 1e-12: without ties and with heavy ones."""
    from gwinferno_amd import draws as D
    from scipy.stats import spearmanr

    x = _data(heavy=heavy)
    out, alive = D.rankcorr_set(np.ones(x.shape[1]), *D.rankcorr_codes(x))
    assert alive and out[0] == x.shape[1]
    assert heavy == bool(np.unique(x[0]).size < x.shape[1] // 10)
    want = spearmanr(x.T).statistic
    assert np.all(np.abs(_rho(out, 3) - want) <= 1e-12), np.max(np.abs(_rho(out, 3) - want))
    assert abs(want[0, 1]) > 0.5 and abs(want[0, 2]) < 0.2


@pytest.mark.parametrize("heavy", (False, True))
def test_integer_weights_repeat_the_samples(heavy):
    """Integer weights give the rho of the dataset with every sample repeated its weight's number of times (a weight of 0: left out),
    to 1e-12, and the same U, mean ranks and R to 1e-12: the repeated samples tie, and tied members share the mid-rank."""
    from gwinferno_amd import draws as D
    from scipy.stats import spearmanr

    x = _data(seed=4, n=400, heavy=heavy)
    w = np.random.default_rng(9).integers(0, 5, x.shape[1])
    out, _ = D.rankcorr_set(w.astype(np.float64), *D.rankcorr_codes(x))
    rep = np.repeat(x, w, axis=1)
    flat, _ = D.rankcorr_set(np.ones(rep.shape[1]), *D.rankcorr_codes(rep))
    assert out[0] == flat[0] == w.sum() and np.all(np.abs(out - flat) <= 1e-12)
    assert np.all(np.abs(_rho(out, 3) - spearmanr(rep.T).statistic) <= 1e-12)


def test_mean_rank_and_the_all_tied_column():
    """m_c = 1/2 to a few ulps under random weights (exact arithmetic gives 1/2: sum_g W_g (2 B_g + W_g) = T^2 over the groups of tied
    members); a column whose members all tie has d = 0, so r = 0.5 and R_cc = 0 and every R_cd with it exactly -- whatever the
    weights' total is -- and postprocess flags it without dividing; a set without weight is NaN and not alive."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(6)
    x = _data(seed=7, n=700)
    x[2] = 3.25
    for trial in range(8):
        u = rng.lognormal(0.0, 2.0, x.shape[1]) * (rng.uniform(size=x.shape[1]) < 0.8)
        out, alive = D.rankcorr_set(u, *D.rankcorr_codes(x))
        assert alive and np.all(np.abs(out[1:4] - 0.5) <= RU.STATEMENT_MEAN_ROUNDING), out[1:4] - 0.5
        assert out[3] == 0.5 or abs(out[3] - 0.5) <= 2.0 * RU.U  # (sum u 0.5 / U: two roundings)
        _, _, r = D.rankcorr_matrix(out, 3)
        assert np.array_equal(r[2], np.zeros(3)) and np.array_equal(r[:, 2], np.zeros(3)) and r[0, 0] > 0.05 and r[1, 1] > 0.05
    dead, alive = D.rankcorr_set(np.zeros(x.shape[1]), *D.rankcorr_codes(x))
    assert not alive and dead[0] == 0.0 and np.all(np.isnan(dead[1:]))


def test_monotone_maps():
    """rankcorr_codes(x) and rankcorr_codes(f(x)) are identical arrays for the strictly increasing exp and cube.  For a decreasing map
    the codes mirror (lt' = n - le, le' = n - lt) and, with weights whose sums are exact (integers), every d changes sign exactly:
    R_cd of a mapped and an unmapped column changes sign to the bit, and so does rho; R_cc does not move."""
    from gwinferno_amd import draws as D

    x = _data(seed=11, n=600)
    x[2] = np.round(3.0 * x[2]) / 3.0  # ties in one column
    base = D.rankcorr_codes(x)
    for f in (np.exp, lambda v: v**3):
        assert np.unique(f(x[0])).size == np.unique(x[0]).size  # (the map is strictly increasing on these doubles too)
        assert all(np.array_equal(a, b) for a, b in zip(base, D.rankcorr_codes(f(x))))
    n = x.shape[1]
    y = x.copy()
    y[2] = -y[2]
    mirrored = D.rankcorr_codes(y)
    assert np.array_equal(mirrored[1][2], n - base[2][2]) and np.array_equal(mirrored[2][2], n - base[1][2])
    w = np.random.default_rng(12).integers(1, 6, n).astype(np.float64)
    out, flipped = D.rankcorr_set(w, *base)[0], D.rankcorr_set(w, *mirrored)[0]
    _, _, r = D.rankcorr_matrix(out, 3)
    _, _, s = D.rankcorr_matrix(flipped, 3)
    assert np.array_equal(s[2, :2], -r[2, :2]) and np.array_equal(s[2, 2], r[2, 2]) and np.array_equal(s[:2, :2], r[:2, :2]) and np.all(r[2, :2] != 0.0)
    assert np.array_equal(_rho(flipped, 3)[2, :2], -_rho(out, 3)[2, :2])
    both, _ = D.rankcorr_set(w, *D.rankcorr_codes(np.stack([x[0], -x[0]])))
    assert _rho(both, 2)[0, 1] == -1.0


def test_pooling_and_flags():
    """The pooled statement equals rankcorr_set on ONE artificial event holding all PE samples with the weights w_i / S_e, to the bit;
    a dead event (masked, or -inf everywhere) has u = 0, is flagged and leaves the statement that of the live events; with no live
    event the observed set is dead, with no live injection the detected one."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(13)
    n_ev, n_pe, n_inj = 4, 150, 333
    x_pe, x_inj = rng.normal(size=(2, n_ev, n_pe)), rng.normal(size=(2, n_inj))
    lw_pe, lw_inj = rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj)
    codes_obs, codes_det = RU.codes(x_pe, x_inj)
    out, dead = D.point_rank_correlations_reference(lw_pe, lw_inj, codes_obs, codes_det)
    assert out.shape == (2, 6) and dead.shape == (n_ev + 2,) and dead.dtype == np.int32 and not dead.any()
    u = np.concatenate([D.draw_weights(lw_pe[e]) / np.float64(__import__("math").fsum(D.draw_weights(lw_pe[e]).tolist())) for e in range(n_ev)])
    assert np.array_equal(out[0], D.rankcorr_set(u, *codes_obs)[0]) and np.array_equal(out[1], D.rankcorr_set(D.draw_weights(lw_inj), *codes_det)[0])
    assert abs(out[0, 0] - n_ev) <= 4 * n_ev * RU.U
    pm = np.ones((n_ev, n_pe), dtype=np.uint8)
    pm[2] = 0
    lw = lw_pe.copy()
    lw[0] = -np.inf
    masked, dead = D.point_rank_correlations_reference(lw, lw_inj, codes_obs, codes_det, pm, None)
    assert np.array_equal(dead, [1, 0, 1, 0, 0, 0])
    u_live = u.reshape(n_ev, n_pe).copy()
    u_live[[0, 2]] = 0.0
    assert np.array_equal(masked[0], D.rankcorr_set(u_live.ravel(), *codes_obs)[0]) and np.array_equal(masked[1], out[1])
    # ... which is the statement on the two live events alone
    keep = [1, 3]
    alone, _ = D.point_rank_correlations_reference(lw_pe[keep], lw_inj, *RU.codes(x_pe[:, keep], x_inj))
    assert np.all(np.abs(_rho(masked[0], 2) - _rho(alone[0], 2)) <= 1e-12) and abs(masked[0, 0] - 2.0) <= 8 * RU.U
    none, dead = D.point_rank_correlations_reference(np.full((n_ev, n_pe), -np.inf), lw_inj, codes_obs, codes_det, None, np.zeros(n_inj, dtype=np.uint8))
    assert np.array_equal(dead, [1, 1, 1, 1, 1, 1]) and np.all(np.isnan(none[:, 1:])) and np.array_equal(none[:, 0], [0.0, 0.0])


def _stub(k=4, seed=21, n_ev=5, n_pe=700, n_inj=2500):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(size=(3, n_ev, n_pe)), rng.normal(size=(3, n_inj))
    x_pe[1] += 0.7 * x_pe[0]
    x_inj[1] -= 0.3 * x_inj[0]
    eng = RU.StubEngine(rng.normal(0.0, 1.0, (k, n_ev, n_pe)), rng.normal(0.0, 1.0, (k, n_inj)))
    return eng, np.arange(k, dtype=np.float64)[:, None], {n: x_pe[i] for i, n in enumerate("abc")}, {n: x_inj[i] for i, n in enumerate("abc")}


def test_catalog_rank_correlation_check_on_the_host():
    """On the shape of the GPU tests (5 x 700 PE samples, 2 500 injections) the statement alone skips and flags NO (point, pair): the
    counts are 0, not capped.  Shapes; rho is R_cd / sqrt(R_cc R_dd) of the raw arrays; delta, the shares and the bands are what they
    say; the mean ranks sit at 1/2; a monotone map of a quantity changes nothing, to the bit; point weights (K,) and (K, n_ev + 1) are
    applied on the host; a constant quantity is flagged and NaN; a dead set is skipped and counted."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values = _stub()
    k = thetas.shape[0]
    r = P.catalog_rank_correlation_check(eng, thetas, pe_values, inj_values=inj_values, backend="host")
    assert int(r["n_skipped"].sum()) == 0 and int(r["degenerate_obs"].sum()) == 0 and int(r["degenerate_det"].sum()) == 0
    assert r["rho_obs"].shape == (k, 3) and r["bands_delta"].shape == (3, 3) and np.array_equal(r["pairs"], [[0, 1], [0, 2], [1, 2]]) and r["n_points"] == k
    assert np.all(np.isfinite(r["delta"])) and np.array_equal(r["delta"], r["rho_obs"] - r["rho_det"])
    cov = r["rank_cov"]
    assert np.array_equal(r["rho_obs"][:, 0], cov[:, 0, 0, 1] / np.sqrt(cov[:, 0, 0, 0] * cov[:, 0, 1, 1]))
    assert np.all(r["rho_obs"][:, 0] > 0.3) and np.all(r["rho_det"][:, 0] < -0.1) and np.all(np.abs(r["rho_obs"][:, 1]) < 0.1)
    assert np.array_equal(r["p_delta_positive"], (r["delta"] > 0).mean(axis=0)) and np.array_equal(r["p_two_sided"], 2 * np.minimum(r["p_delta_positive"], 1 - r["p_delta_positive"]))
    assert np.array_equal(r["bands_rho_obs"], D.weighted_percentiles(r["rho_obs"], np.ones(k), r["levels"]))
    assert 0.0 <= r["rank_mean_error"] <= RU.STATEMENT_MEAN_ROUNDING and np.all(r["variance_floor"] < 1e-9)
    mapped = dict(pe_values, a=np.exp(pe_values["a"])), dict(inj_values, a=np.exp(inj_values["a"]))
    m = P.catalog_rank_correlation_check(eng, thetas, mapped[0], inj_values=mapped[1], backend="host")
    assert all(np.array_equal(m[key], r[key]) for key in ("rho_obs", "rho_det", "delta", "rank_cov", "mean_rank", "total"))
    v = np.array([0.0, 1.0, 0.25, 1.0])
    w = P.catalog_rank_correlation_check(eng, thetas, pe_values, inj_values=inj_values, point_weights=v, backend="host")
    wide = P.catalog_rank_correlation_check(eng, thetas, pe_values, inj_values=inj_values, point_weights=np.column_stack([np.ones((k, eng.n_ev)), v]), backend="host")
    assert np.array_equal(w["rho_obs"], r["rho_obs"]) and np.array_equal(w["bands_delta"], D.weighted_percentiles(r["delta"], v, r["levels"]))
    assert np.array_equal(w["p_delta_positive"], (v[:, None] * (r["delta"] > 0)).sum(axis=0) / v.sum()) and np.array_equal(wide["bands_delta"], w["bands_delta"])
    flat = dict(pe_values, c=np.full_like(pe_values["c"], 1.5))
    f = P.catalog_rank_correlation_check(eng, thetas, flat, inj_values=inj_values, pairs=[("a", "c"), ("a", "b")], backend="host")
    assert np.array_equal(f["degenerate_obs"], np.tile([1, 0], (k, 1))) and not f["degenerate_det"].any() and np.all(np.isnan(f["rho_obs"][:, 0])) and not f["n_skipped"].any()
    assert np.array_equal(f["rho_obs"][:, 1], r["rho_obs"][:, 0]) and np.all(f["rank_cov"][:, 0, 2, 2] == 0.0)
    gone = RU.StubEngine(eng.lw_pe, np.where(np.arange(k)[:, None] == 2, -np.inf, eng.lw_inj))
    g = P.catalog_rank_correlation_check(gone, thetas, pe_values, inj_values=inj_values, backend="host")
    assert np.array_equal(g["n_skipped"], [1, 1, 1]) and np.all(np.isnan(g["delta"][2])) and np.array_equal(g["dead_set"][2], [0, 1]) and np.array_equal(g["rho_obs"], r["rho_obs"])
    with pytest.raises(ValueError, match="inj_values"):
        P.catalog_rank_correlation_check(eng, thetas, pe_values, backend="host")


def test_the_derived_bounds():
    """The tolerance of the GPU tests is a count of roundings: far below the rank variance of any column that is not constant (1/12 for
    a continuous one), growing with the live samples of an event and with the tiles; the floor below which the library does not divide
    (draws.rankcorr_error_bound, with every sample of an event live) is never below the tests' bound for the same shape."""
    from gwinferno_amd import draws as D

    for shape, (n_ev, n_pe, n_inj) in RU.SHAPES.items():
        obs = (n_pe, -(-(n_ev * n_pe) // RU.TILE), n_ev * -(-n_pe // RU.TILE))
        det = (n_inj, -(-n_inj // RU.TILE), -(-n_inj // RU.TILE))
        t_obs, t_det = RU.r_tolerance(*obs, True), RU.r_tolerance(0, *det[1:], False)
        assert 2e-13 < t_obs < 2e-12 and 5e-15 < t_det < 5e-14, (shape, t_obs, t_det)
        assert D.rankcorr_error_bound(*obs, True) >= t_obs and D.rankcorr_error_bound(*det, False) >= t_det
        assert RU.r_tolerance(obs[0] // 2, *obs[1:], True) < t_obs < RU.r_tolerance(obs[0], obs[1] + 1, obs[2] + 1, True)
        assert RU.mean_tolerance(*obs, True) < 1e-11
    tol = RU.rho_tolerance(np.float64(1e-12), 0.04, 1 / 12, 1 / 12)
    assert 1e-11 < tol < 3e-11


def test_header_library_and_refusals_without_a_device():
    """The three exports are declared, bound and listed, with their argument counts; the ABI version stays 3; a null handle and a
    host-only handle answer GWI_ERR_INVALID, the latter with a message, and write nothing; the Python layer refuses an engine that holds
    a shard in the words of its neighbours, a call before columns are set, and columns of the wrong shape."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_set_rankcorr_columns", 8), ("gwi_point_rank_correlations", 5), ("gwi_point_rankcorr_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_rank_correlations.restype is C.c_int32 and lib.gwi_set_rankcorr_columns.restype is C.c_int32 and lib.gwi_point_rankcorr_times.restype is None
    assert "DESIGN 8l" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_rank_correlations(None, None, 1, None, None) == -1 and lib.gwi_set_rankcorr_columns(None, 1, None, None, None, None, None, None) == -1
    comp = RU.composition("ragged", device=N.DEVICE_HOST_ONLY)
    eng = comp.engine()
    try:
        i32 = C.POINTER(C.c_int32)
        out, dead = np.full((1, 2, 3), 7.0), np.full((1, eng.n_ev + 2), 7, dtype=np.int32)
        assert lib.gwi_point_rank_correlations(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(out), dead.ctypes.data_as(i32)) == -1
        assert "gwi_point_rank_correlations: host-only handle: no device to sum on" in lib.gwi_last_error(eng.handle).decode() and np.all(out == 7.0) and np.all(dead == 7)
        ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
        lib.gwi_point_rankcorr_times(*[C.byref(m) for m in ms], C.byref(n_launch))
        assert n_launch.value == 0 and all(m.value == 0.0 for m in ms)
        x_pe, x_inj = RU.columns(1)
        with pytest.raises(N.NativeEngineError, match="gwi_set_rankcorr_columns: host-only handle: no device to keep the columns on"):
            eng.set_rankcorr_columns(x_pe, x_inj)
        with pytest.raises(ValueError, match="both needed"):
            eng.set_rankcorr_columns(x_pe, None)
        with pytest.raises(ValueError, match="pe_values has shape"):
            eng.set_rankcorr_columns(x_pe[:, :2], x_inj)
        with pytest.raises(ValueError, match="thetas has shape"):
            eng.point_rank_correlations(np.zeros(eng.n_theta + 1))
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_rank_correlations: this engine holds one shard of the catalog; the rank sets need the global set"):
        shard.point_rank_correlations(np.zeros(3))
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: set_rankcorr_columns: this engine holds one shard"):
        shard.set_rankcorr_columns(None, None)
