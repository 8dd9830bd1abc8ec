"""CPU: per-point conditional moments (include/gwi_engine.h: gwi_point_conditionals; gwinferno_amd/csrc/gwi_cond.h) -- the
NumPy statement alone (gwinferno_amd/draws.py: conditionals_segment, point_conditionals_reference) against an independent brute-force
loop, its exact cases, the digits a two-pass variance keeps, the derived device tolerance, the vetted inputs of the GPU file, the host
backend of postprocess.catalog_conditional_check and postprocess.event_conditional_moments on a stub engine against pooled samples, and
the header, the exports and the refusals that need no device."""
import os
import re

import conditional_util as CU
import moment_util as MU
import numpy as np
import pytest
import test_pit_cpu as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segments(seed=3, n_ev=3, n_pe=300, n_inj=500, n_bins=7):
    from gwinferno_amd.draws import digitize

    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(2.0, 1.5, (3, n_ev, n_pe)), rng.normal(2.0, 1.5, (3, n_inj))
    x_pe[1] += 0.6 * x_pe[0] ** 2  # (a dependence no covariance sees in full)
    x_inj[1] += 0.6 * x_inj[0] ** 2
    e = np.linspace(-1.0, 5.0, n_bins + 1)  # (samples lie outside on both sides)
    codes_pe, codes_inj = np.stack([digitize(x_pe[0], e), digitize(x_pe[2], e)]), np.stack([digitize(x_inj[0], e), digitize(x_inj[2], e)])
    return rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj), codes_pe, codes_inj, x_pe, x_inj


def test_the_statement_against_a_brute_force_loop():
    """Seeded inputs, with and without masks, three pairs: per segment, pair and bin a plain Python loop over the samples (sums in sample
    order, np.exp of lw - max) gives the share, the mean and the centred variance to 1e-12 of sum w^ |y| and sum w^ |y - m|^2; the shares
    of a pair sum to 1 minus the weight outside; nothing is dead."""
    from gwinferno_amd import draws as D

    lw_pe, lw_inj, cp, ci, x_pe, x_inj = _segments()
    rng = np.random.default_rng(5)
    pm, im = (rng.uniform(size=lw_pe.shape) < 0.7).astype(np.uint8), (rng.uniform(size=lw_inj.shape) < 0.5).astype(np.uint8)
    pairs, n_bins = ((0, 1), (1, 0), (0, 2)), 7
    for masks in ((None, None), (pm, im)):
        out, dead = D.point_conditionals_reference(lw_pe, lw_inj, cp, ci, x_pe, x_inj, pairs, n_bins, *masks)
        assert out.shape == (4, 3, 3, n_bins) and dead.shape == (4,) and dead.dtype == np.int32 and not dead.any()
        for seg in range(4):
            lw, mask = (lw_pe[seg], None if masks[0] is None else masks[0][seg]) if seg < 3 else (lw_inj, masks[1])
            on = np.ones(lw.size, dtype=bool) if mask is None else mask != 0
            big = lw[on].max()
            for r, (cx, cy) in enumerate(pairs):
                code, y = (cp[cx, seg], x_pe[cy, seg]) if seg < 3 else (ci[cx], x_inj[cy])
                total, inside = 0.0, 0.0
                sums = np.zeros((n_bins, 3))
                for i in range(lw.size):
                    if not on[i]:
                        continue
                    w = float(np.exp(lw[i] - big))
                    total += w
                    if code[i] < n_bins:
                        inside += w
                        sums[code[i]] += (w, w * y[i], w * abs(y[i]))
                for b in range(n_bins):
                    m = sums[b, 1] / sums[b, 0]
                    sq = sum(float(np.exp(lw[i] - big)) * (y[i] - m) ** 2 for i in range(lw.size) if on[i] and code[i] == b)
                    assert abs(out[seg, r, 0, b] - sums[b, 0] / total) <= 1e-12 * sums[b, 0] / total
                    assert abs(out[seg, r, 1, b] - m) <= 1e-12 * sums[b, 2] / sums[b, 0]
                    assert abs(out[seg, r, 2, b] - sq / sums[b, 0]) <= 1e-12 * sq / sums[b, 0]
                assert abs(out[seg, r, 0].sum() - inside / total) <= 1e-12 and inside < total
        assert np.array_equal(out[:, 0, 0], out[:, 2, 0])  # (the same cx: the same shares)


def test_exact_cases():
    """One live sample: share exactly 1 in its bin and 0 elsewhere, the mean the sample, the variance exactly 0, NaN in the other bins.  A
    bin without weight has share +0.0 and NaN mean and variance and is no error.  A segment without weight gives NaN and is counted; a set
    that lacks codes or values gives NaN and its flag still tells the weight; codes for one set and values for the other are refused."""
    from gwinferno_amd import draws as D

    lw_pe, lw_inj, cp, ci, x_pe, x_inj = _segments()
    pm = np.ones(lw_pe.shape, dtype=np.uint8)
    pm[0] = 0
    pm[0, 217] = 1
    lw = lw_pe.copy()
    lw[1, ::2], lw[1, 1::2] = -np.inf, np.nan
    cp = cp.copy()
    cp[0, 0, 217] = 3
    out, dead = D.point_conditionals_reference(lw, lw_inj, cp, ci, x_pe, x_inj, [(0, 1)], 7, pm, None)
    assert np.array_equal(dead, [0, 1, 0, 0]) and np.all(np.isnan(out[1]))
    assert np.array_equal(out[0, 0, 0], [0, 0, 0, 1, 0, 0, 0]) and not np.any(np.signbit(out[0, 0, 0]))
    assert out[0, 0, 1, 3] == x_pe[1, 0, 217] and out[0, 0, 2, 3] == 0.0 and np.all(np.isnan(np.delete(out[0, 0, 1:], 3, axis=1)))
    free, _ = D.point_conditionals_reference(lw_pe, lw_inj, cp, ci, x_pe, x_inj, [(0, 1)], 7)
    assert np.array_equal(out[2:], free[2:])
    only, d2 = D.point_conditionals_reference(lw, lw_inj, None, ci, x_pe, x_inj, [(0, 1)], 7, pm, None)
    assert np.all(np.isnan(only[:3])) and np.array_equal(only[3], free[3]) and np.array_equal(d2, dead)
    seg, alive = D.conditionals_segment(np.zeros(5), np.zeros(5, dtype=np.uint16), np.ones(5), 2)
    assert not alive and np.all(np.isnan(seg))
    for bad, word in ((dict(codes_pe=None, x_inj=None), "both codes and values"), (dict(pairs=[(2, 0)]), "a pair is"), (dict(pairs=[(0, 3)]), "a pair is"),
                      (dict(pairs=[(0, 0)] * 9), "pairs"), (dict(pairs=[(0, 0)] * 3, n_bins=171), "n_pairs n_bins")):
        kw = dict(codes_pe=cp, codes_inj=ci, x_pe=x_pe, x_inj=x_inj, pairs=[(0, 1)], n_bins=7)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            D.point_conditionals_reference(lw, lw_inj, **kw)
    assert D.MAX_CONDITIONAL_PAIRS == 8 and D.MAX_CONDITIONAL_ITEMS == 512


def test_two_passes_keep_the_digits_of_a_column_far_from_zero():
    """y_n = 1e6 + 1e-3 n, n = 0 ... 1999, equal weights, all in one bin of two: the conditional variance is 1e-6 (N^2 - 1) / 12 and the
    two-pass statement keeps it to 1e-9 relative.  The one-pass formula E[y^2 | b] - E[y | b]^2 subtracts two numbers near 1e12 whose
    spacing is 1.2e-4 and loses it -- the reason gwi_cond.h centres on the first pass's own mean, as gwi_moment.h does."""
    from gwinferno_amd import draws as D

    n = 2000
    y = 1.0e6 + 1.0e-3 * np.arange(n)
    exact = 1.0e-6 * (n * n - 1.0) / 12.0
    out, alive = D.conditionals_segment(np.ones(n), np.ones(n, dtype=np.uint16), y, 2)
    assert alive and out[0, 1] == 1.0 and abs(out[2, 1] - exact) <= 1e-9 * exact and abs(out[1, 1] - (1.0e6 + 1.0e-3 * (n - 1) / 2.0)) <= 1e-9
    assert out[0, 0] == 0.0 and np.isnan(out[1, 0]) and np.isnan(out[2, 0])
    one_pass = np.mean(y * y) - np.mean(y) ** 2
    assert abs(one_pass - exact) > 1e-6 * exact


def test_the_device_tolerance_is_a_rounding_bound_and_the_inputs_are_vetted():
    """conditional_util's bounds are counts of roundings: one more live sample in the bin adds one unit, one more tile one unit, the variance
    three more than the mean; with a whole segment in one bin the relative bound stays below 1e-12.  The inputs of the GPU file: at
    setting 5 every (segment, mass_ratio bin) cell of the unmasked catalog holds at least 50 samples, the designed-empty sixth bin none
    in any segment and bin column, and exactly the pushed samples are coded outside; at setting 256 at least half of all (segment, bin)
    cells over the two bin columns are non-empty; the pair lists meet the limits, 512 items exactly at setting 256."""
    assert CU.mean_units(11, 2) - CU.mean_units(10, 2) == 1.0 and CU.mean_units(10, 3) - CU.mean_units(10, 2) == 1.0 and CU.var_units(10, 2) - CU.mean_units(10, 2) == 3.0
    assert CU.mean_units(10, 2) == 10 + 2 + 7 and 1.01 * CU.var_units(MU.N_INJ, 3) * CU.U < 1e-12
    n_segs = MU.N_EV + 1
    cp, ci = CU.codes(5)
    assert cp.shape == (2, MU.N_EV, MU.N_PE) and ci.shape == (2, MU.N_INJ) and cp.dtype == np.uint16
    cells = np.array([[np.count_nonzero(c == b) for b in range(5)] for c in list(cp[0]) + [ci[0]]])
    print("setting 5: smallest (segment, mass_ratio bin) cell holds", cells.min(), "samples")
    assert cells.shape == (n_segs, 5) and cells.min() >= 50
    assert not np.any(cp == CU.EMPTY_BIN) and not np.any(ci == CU.EMPTY_BIN)
    assert np.array_equal(np.nonzero(cp[1, 2] == CU.OUTSIDE)[0], CU.OUTSIDE_PE) and np.array_equal(np.nonzero(ci[0] == CU.OUTSIDE)[0], CU.OUTSIDE_INJ)
    assert MU.SINGLE_SAMPLE not in CU.OUTSIDE_PE and CU.OUTSIDE_PE[0] < MU.TILE <= CU.OUTSIDE_PE[1]
    free = CU.codes(5, outside=False)
    assert not np.any(free[0] == CU.OUTSIDE) and not np.any(free[1] == CU.OUTSIDE)
    cp, ci = CU.codes(256)
    filled = np.mean([[np.bincount(c, minlength=256) > 0 for c in list(cp[col]) + [ci[col]]] for col in range(2)])
    print(f"setting 256: {100 * filled:.0f} % of the (segment, bin) cells are non-empty")
    assert filled >= 0.5 and int(cp.max()) == 255 and not np.any(cp == CU.OUTSIDE)
    for s in CU.SETTINGS:
        assert 1 <= len(CU.PAIRS[s]) <= 8 and len(CU.PAIRS[s]) * CU.N_BINS[s] <= 512 and all(cx < 2 and cy < CU.N_VALUE_COLUMNS for cx, cy in CU.PAIRS[s])
    assert len(CU.PAIRS[256]) * CU.N_BINS[256] == 512 and MU.columns(3)[0][0].min() > MU.OFFSET


def _stub(k=6, seed=9, n_ev=4, n_pe=60, n_inj=90):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(0.0, 1.0, (2, n_ev, n_pe)), rng.normal(0.0, 1.2, (2, n_inj))
    x_pe[1] += 0.5 * np.abs(x_pe[0])
    lw_pe, lw_inj = rng.normal(0.0, 1.0, (k, n_ev, n_pe)), rng.normal(0.0, 1.0, (k, n_inj))
    eng = TP._StubEngine(lw_pe, lw_inj, rng.normal(0.0, 1.0, (k, n_ev)), rng.normal(-3.0, 0.2, k))
    return eng, np.arange(k, dtype=np.float64)[:, None], {"x": x_pe[0], "y": x_pe[1]}, {"x": x_inj[0], "y": x_inj[1]}, np.array([-1.5, -0.5, 0.0, 0.5, 1.5])


def test_catalog_conditional_check_against_pooled_samples():
    """On the stub engine: the raw arrays are the statement's; A_b, mu_b and sigma2_b are the share, mean and variance, within the bin, of
    the pooled sample of the live events with weight w_i / (S_e n_live); the predicted side is the injection segment's; the deltas, the
    shares of the points and the bands are what they say; a point of weight 0 drops out; a dead event is left out of its point's mixture;
    a bin no sample falls into is skipped and counted; the refusals."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, edges = _stub()
    k, n_ev, n_bins = thetas.shape[0], eng.n_ev, edges.size - 1
    r = P.catalog_conditional_check(eng, thetas, "x", "y", edges, pe_values=pe_values, inj_values=inj_values, backend="host")
    assert r["n_points"] == k and np.array_equal(r["edges"], edges) and not r["n_skipped"].any() and np.array_equal(r["n_live"], np.full(k, n_ev))
    for key in ("share_obs", "mean_obs", "var_obs", "std_obs", "share_det", "mean_det", "std_det", "delta_mean", "delta_std"):
        assert r[key].shape == (k, n_bins) and np.all(np.isfinite(r[key])), key
    for key in ("bands_mean_obs", "bands_std_det", "bands_delta_mean", "bands_delta_std"):
        assert r[key].shape == (3, n_bins) and np.all(np.diff(r[key], axis=0) >= 0.0), key
    assert np.array_equal(r["delta_mean"], r["mean_obs"] - r["mean_det"]) and np.array_equal(r["delta_std"], r["std_obs"] - r["std_det"])
    assert np.array_equal(r["p_delta_mean_positive"], (r["delta_mean"] > 0.0).mean(axis=0))
    assert np.array_equal(r["p_std_two_sided"], 2.0 * np.minimum(r["p_delta_std_positive"], 1.0 - r["p_delta_std_positive"]))
    assert np.array_equal(r["bands_delta_mean"], D.weighted_percentiles(r["delta_mean"], np.ones(k), [0.05, 0.5, 0.95]))
    code_pe, code_inj = D.digitize(pe_values["x"], edges), D.digitize(inj_values["x"], edges)
    for i in range(k):
        out, dead = D.point_conditionals_reference(eng.lw_pe[i], eng.lw_inj[i], code_pe[None], code_inj[None], pe_values["y"][None], inj_values["y"][None], [(0, 0)], n_bins)
        assert np.array_equal(out[:, 0, 0], r["point_share"][i]) and np.array_equal(out[:, 0, 1], r["point_mean"][i]) and np.array_equal(out[:, 0, 2], r["point_var"][i])
        w = np.concatenate([D.draw_weights(eng.lw_pe[i, e]) / D.draw_weights(eng.lw_pe[i, e]).sum() / n_ev for e in range(n_ev)])
        wd = D.draw_weights(eng.lw_inj[i])
        for b in range(n_bins):
            sel = code_pe.ravel() == b
            wb, yb = w[sel], pe_values["y"].ravel()[sel]
            mu = np.average(yb, weights=wb)
            assert np.isclose(r["share_obs"][i, b], wb.sum(), rtol=1e-12) and np.isclose(r["mean_obs"][i, b], mu, rtol=1e-12, atol=1e-14)
            assert np.isclose(r["var_obs"][i, b], np.average((yb - mu) ** 2, weights=wb), rtol=1e-11)
            sel = code_inj == b
            md = np.average(inj_values["y"][sel], weights=wd[sel])
            assert np.isclose(r["mean_det"][i, b], md, rtol=1e-12, atol=1e-14) and np.isclose(r["std_det"][i, b] ** 2, np.average((inj_values["y"][sel] - md) ** 2, weights=wd[sel]), rtol=1e-11)
    v = np.ones(k)
    v[2] = 0.0
    weighted = P.catalog_conditional_check(eng, thetas, "x", "y", edges, pe_values=pe_values, inj_values=inj_values, point_weights=v, backend="host")
    keep = np.arange(k) != 2
    assert np.array_equal(weighted["p_delta_mean_positive"], (r["delta_mean"][keep] > 0.0).mean(axis=0)) and np.array_equal(weighted["mean_obs"], r["mean_obs"])
    # a dead event at one point is left out of that point's mixture; a bin above every sample is skipped and counted at every point
    eng.lw_pe[1, 0] = -np.inf
    wide = np.append(edges, [50.0, 60.0])
    d = P.catalog_conditional_check(eng, thetas, "x", "y", wide, pe_values=pe_values, inj_values=None, backend="host")
    assert np.array_equal(d["n_live"], [n_ev, n_ev - 1] + [n_ev] * (k - 2)) and d["dead"][1, 0] == 1 and np.all(np.isnan(d["mean_det"])) and np.array_equal(d["n_skipped"], [k] * (n_bins + 2))
    assert np.all(d["share_obs"][:, -1] == 0.0) and np.all(np.isnan(d["mean_obs"][:, -1])) and np.all(np.isfinite(d["mean_obs"][:, :-1]))
    others = list(range(1, n_ev))
    w = np.concatenate([D.draw_weights(eng.lw_pe[1, e]) / D.draw_weights(eng.lw_pe[1, e]).sum() for e in others])
    sel = code_pe[others].ravel() == 1
    assert np.isclose(d["mean_obs"][1, 1], np.average(pe_values["y"][others].ravel()[sel], weights=w[sel]), rtol=1e-12)
    for bad in (dict(point_weights=np.zeros(k)), dict(levels=(150,)), dict(backend="cuda")):
        with pytest.raises(ValueError):
            P.catalog_conditional_check(eng, thetas, "x", "y", edges, pe_values=pe_values, inj_values=inj_values, **bad)
    for args in (("x", "zz", edges), ("x", "y", edges[::-1]), ("x", "y", edges[:1])):
        with pytest.raises(ValueError):
            P.catalog_conditional_check(eng, thetas, *args, pe_values=pe_values, inj_values=inj_values, backend="host")


def test_event_conditional_moments_on_the_host():
    """within + between == total to the bit; share, mean and total are the share, mean and variance, within the bin, of the pooled weighted
    sample with weights v_k w_ki / S_ke (the law of total variance), for equal, (K,), (K, n_ev + 1), leave-one-out and Pareto-smoothed
    weights; a dead (point, event) is skipped and counted in every bin; one point alone has no between part; the refusals."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, _, edges = _stub()
    k, n_ev, n_bins = thetas.shape[0], eng.n_ev, edges.size - 1
    code = D.digitize(pe_values["x"], edges)
    rng = np.random.default_rng(13)
    loo = D.leave_one_out_summary(eng.log_bfs - eng.log_mu[:, None])["point_weights"]
    psis = D.pareto_smoothed_summary(eng.log_bfs - eng.log_mu[:, None])
    full = rng.uniform(0.1, 1.0, (k, n_ev + 1))
    cases = ((dict(), np.ones((k, n_ev))), (dict(point_weights=np.linspace(0.2, 1.0, k)), np.tile(np.linspace(0.2, 1.0, k)[:, None], (1, n_ev))),
             (dict(leave_one_out=True, total_inj=1000.0), loo[:, :n_ev]), (dict(leave_one_out="psis", total_inj=1000.0), psis["point_weights"][:, :n_ev]),
             (dict(point_weights=full), full[:, :n_ev]))
    for kw, v in cases:
        r = P.event_conditional_moments(eng, thetas, "x", "y", edges, pe_values=pe_values, backend="host", **kw)
        assert r["n_points"] == k and not r["n_dead"].any() and not r["n_skipped"].any() and ("elpd_loo" in r) == ("leave_one_out" in kw)
        assert ("pareto_k" in r) == (kw.get("leave_one_out") == "psis") and r["share"].shape == (n_ev, n_bins)
        assert np.array_equal(r["within"] + r["between"], r["total"]) and np.all(r["within"] > 0.0) and np.all(r["between"] >= 0.0)
        assert np.allclose(r["neff_points"], v.sum(axis=0) ** 2 / (v * v).sum(axis=0), rtol=1e-13)
        for e in range(n_ev):
            w = np.concatenate([v[i, e] * D.draw_weights(eng.lw_pe[i, e]) / D.draw_weights(eng.lw_pe[i, e]).sum() for i in range(k)]) / v[:, e].sum()
            pooled, pooled_code = np.tile(pe_values["y"][e], k), np.tile(code[e], k)
            for b in range(n_bins):
                sel = pooled_code == b
                mu = np.average(pooled[sel], weights=w[sel])
                assert np.isclose(r["share"][e, b], w[sel].sum(), rtol=1e-12) and np.isclose(r["mean"][e, b], mu, rtol=1e-12, atol=1e-14)
                assert np.isclose(r["total"][e, b], np.average((pooled[sel] - mu) ** 2, weights=w[sel]), rtol=1e-11)
    one = P.event_conditional_moments(eng, thetas[:1], "x", "y", edges, pe_values=pe_values, backend="host")
    assert np.all(one["between"] == 0.0) and np.array_equal(one["total"], one["within"])
    eng.lw_pe[2, 1] = np.nan
    d = P.event_conditional_moments(eng, thetas, "x", "y", edges, pe_values=pe_values, backend="host")
    assert np.array_equal(d["n_dead"], [0, 1, 0, 0]) and np.array_equal(d["n_skipped"][1], [1] * n_bins) and not d["n_skipped"][[0, 2, 3]].any()
    rest = P.event_conditional_moments(eng, thetas[np.arange(k) != 2], "x", "y", edges, pe_values=pe_values, backend="host")
    assert np.isclose(d["neff_points"][1], k - 1) and np.allclose(d["total"][1], rest["total"][1], rtol=1e-12) and np.allclose(d["mean"][1], rest["mean"][1], rtol=1e-13)
    for bad in (dict(leave_one_out="loo"), dict(leave_one_out=True), dict(leave_one_out="psis", total_inj=1.0, point_weights=np.ones(k)), dict(backend="gpu"),
                dict(point_weights=np.ones(k + 1))):
        with pytest.raises(ValueError):
            P.event_conditional_moments(eng, thetas, "x", "y", edges, pe_values=pe_values, **bad)


def test_header_library_and_refusals_without_a_device():
    """The two exports are declared, bound and listed, with their argument counts; the header cites DESIGN 8k; the ABI version stays 3; a
    null handle and a host-only handle answer GWI_ERR_INVALID, the latter with a message, and write nothing; the Python layer refuses
    an engine that holds a shard in the words of its neighbours, and a bad pair list before any call."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_point_conditionals", 7), ("gwi_point_conditional_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_conditionals.restype is C.c_int32 and lib.gwi_point_conditional_times.restype is None
    assert "DESIGN 8k" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert "DESIGN 8k" in open(os.path.join(ROOT, "gwinferno_amd", "csrc", "gwi_cond.h")).read()
    assert lib.gwi_point_conditionals(None, None, 1, 1, None, None, None) == -1
    eng = MU.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    try:
        i32 = C.POINTER(C.c_int32)
        out, dead, pairs = np.full((1, MU.N_EV + 1, 1, 3, 4), 7.0), np.full((1, MU.N_EV + 1), 7, dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
        assert lib.gwi_point_conditionals(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, 1, pairs.ctypes.data_as(i32), N.as_dp(out), dead.ctypes.data_as(i32)) == -1
        assert "gwi_point_conditionals: host-only handle: no device to sum on" in lib.gwi_last_error(eng.handle).decode() and np.all(out == 7.0) and np.all(dead == 7)
        with pytest.raises(ValueError, match="thetas has shape"):
            eng.point_conditionals(np.zeros(eng.n_theta + 1), [(0, 0)])
        with pytest.raises(ValueError, match="between 1 and 8"):
            eng.point_conditionals(np.zeros(eng.n_theta), [(0, 0)] * 9)
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_conditionals: this engine holds one shard of the catalog; the injection moments need the global set"):
        shard.point_conditionals(np.zeros(3), [(0, 0)])
