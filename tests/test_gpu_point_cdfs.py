"""GPU: per-point CDFs on the device (include/gwi_engine.h: gwi_point_cdfs; gwinferno_amd/csrc/gwi_cdf.h): bit equality with
the running sums of gwi_weighted_histograms, the logarithmic slots against the NumPy statement (gwinferno_amd/draws.py:
point_cdfs_reference) fed with the engine's own log-weights, liveness and masks, determinism over calls, splits, handles and the staging
chunk, the absence of side effects, the refusals, and postprocess.catalog_predictive_check on both backends.

Shapes (tests/cdf_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 500 injections (three tiles, the last ragged),
two columns, 5 and 256 grid points, three points of a PL+Peak model.  The inputs are vetted without a device in tests/test_cdf_cpu.py:
test_inputs_of_the_gpu_tests -- no entry is left out of any comparison here."""
import ctypes as C

import cdf_util as U
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CASE = {}


def _case():
    """The engine with its three points and their log-weights from the device: made once, shared, never changed."""
    if not _CASE:
        comp = U.composition()
        eng = comp.engine()
        thetas = U.points(comp)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas]
        for pair in lw:
            for a in pair:
                a.setflags(write=False)
        _CASE.update(comp=comp, eng=eng, thetas=thetas, lw=lw)
    return _CASE


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    if _CASE:
        _CASE["eng"].close()
    _CASE.clear()


def _set(eng, n_grid, case="free", pe=True, inj=True):
    pc, ic = U.codes(n_grid)
    eng.set_draw_mask(*U.masks(case))
    eng.set_histogram_bins(pc if pe else None, ic if inj else None, n_bins=n_grid)


def _same(a, b):
    """equal bits, NaN in the same places"""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("n_grid", U.N_GRID)
def test_bit_equality_with_the_histogram_entry(n_grid, case):
    """For every point alone: slot 0 is np.cumsum of the injection histogram gwi_weighted_histograms returns for that point, to the
    bit; the events' np.cumsum(hist_pe[e]) added in event order and divided by n_live is slot 1, to the bit.  No tolerance: this pins
    the quotient, the order of the prefix and the order of the events."""
    c = _case()
    eng = c["eng"]
    try:
        _set(eng, n_grid, case)
        out, live = eng.point_cdfs(c["thetas"])
        assert out.shape == (U.N_POINTS, 4, 2, n_grid) and live.shape == (U.N_POINTS, 2) and live.dtype == np.int32
        for k, theta in enumerate(c["thetas"]):
            hp, hi, dead = eng.weighted_histograms(theta)
            assert np.array_equal(out[k, 0], np.cumsum(hi, axis=-1))
            acc, n_live = np.zeros((2, n_grid)), 0
            for e in range(U.N_EV):
                if dead[e]:
                    continue
                acc += np.cumsum(hp[e], axis=-1)
                n_live += 1
            assert np.array_equal(live[k], [n_live, 1 - dead[U.N_EV]]) and n_live == (U.N_EV - 1 if case == "masked" else U.N_EV)
            assert np.array_equal(out[k, 1], acc / n_live)
            assert np.all(np.diff(out[k, :2], axis=-1) >= 0.0) and np.all(out[k, 0] > 0.0) and np.all(out[k, :2] < 1.0)
    finally:
        eng.set_draw_mask()


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("n_grid", U.N_GRID)
def test_log_slots_against_the_statement(n_grid, case):
    """Slots 2 and 3 of every point against point_cdfs_reference on eng.log_weights under the DERIVED bound of cdf_util.log_sum_bounds
    (per live event the F error -- hist_util's bound plus G roundings -- over F, resp. over 1 - F, plus the documented ulp bound of the
    HIP maths library's log / log1p and one ulp of the host's, plus the rounding of the sum over the events).  Where the statement
    gives -inf the device gives -inf: the whole mass_1 column of slot 2, where the heavy events have no weight on the grid.  Slots 0
    and 1 are held to the F bound against the statement as well.  The largest deviation is printed in units of the bound."""
    from gwinferno_amd.draws import point_cdfs_reference

    c = _case()
    eng = c["eng"]
    pm, im = U.masks(case)
    pc, ic = U.codes(n_grid)
    try:
        _set(eng, n_grid, case)
        out, live = eng.point_cdfs(c["thetas"])
    finally:
        eng.set_draw_mask()
    worst = [0.0, 0.0]
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_live = point_cdfs_reference(lw_pe, lw_inj, pm, im, pc, ic, n_grid)
        assert np.array_equal(live[k], want_live)
        f, lives = U.statement_event_cdfs(lw_pe, pm, pc, n_grid)
        tols = U.log_sum_bounds(f, lives, n_grid)
        assert np.all(np.isfinite(tols[0])) and np.all(np.isfinite(tols[1]))  # (nothing is left out)
        r_pe, r_inj = max(U.f_rel_bound(n, n_grid) for n in lives), U.f_rel_bound(U.HU.n_live(lw_inj, im), n_grid)
        assert np.all(np.abs(out[k, 0] - want[0]) <= r_inj * want[0]) and np.all(np.abs(out[k, 1] - want[1]) <= (r_pe + 4 * U.U) * want[1])
        for slot, tol in ((2, tols[0]), (3, tols[1])):
            inf = np.isneginf(want[slot])
            assert np.array_equal(np.isneginf(out[k, slot]), inf) and np.all(np.isfinite(out[k, slot][~inf])) and not np.any(np.isnan(out[k, slot]))
            dev = np.abs(out[k, slot][~inf] - want[slot][~inf])
            assert np.all(dev <= tol[~inf]), (slot, k, float(np.max(dev / tol[~inf])))
            worst[slot - 2] = max(worst[slot - 2], float(np.max(dev / tol[~inf])))
        assert np.all(np.isneginf(want[2][1])) and np.all(np.isfinite(want[2][0])) and np.all(np.isfinite(want[3])) and np.all(want[3] < 0.0)
    print(f"G = {n_grid} {case}: largest |device - statement| of log_all_below = {worst[0]:.3f}, of log_all_above = {worst[1]:.3f} of the derived bound")


def test_liveness_and_masks():
    """An event masked out entirely through set_draw_mask: live[k, 0] = n_ev - 1 and slots 1-3 are those of the catalog without it
    (slot 1 to the bit from the other events' histograms; slots 2 and 3 under the derived bound against the statement on the arrays
    with the event deleted).  An injection mask that removes everything: slot 0 all NaN, live[k, 1] = 0, slots 1-3 keep their bits."""
    from gwinferno_amd.draws import point_cdfs_reference

    c = _case()
    eng, n_grid = c["eng"], 5
    pc, ic = U.codes(n_grid)
    try:
        _set(eng, n_grid, "masked")
        out, live = eng.point_cdfs(c["thetas"])
        _set(eng, n_grid, "no_inj")
        out_no, live_no = eng.point_cdfs(c["thetas"])
    finally:
        eng.set_draw_mask()
    assert np.array_equal(live, [[U.N_EV - 1, 1]] * U.N_POINTS) and np.array_equal(live_no, [[U.N_EV - 1, 0]] * U.N_POINTS)
    assert np.all(np.isnan(out_no[:, 0])) and np.array_equal(out_no[:, 1:], out[:, 1:]) and not np.any(np.isnan(out[:, 0]))
    pm, im = U.masks("masked")
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        less = [np.delete(a, U.DEAD_EVENT, axis=ax) for a, ax in ((lw_pe, 0), (pm, 0), (pc, 1))]
        want, want_live = point_cdfs_reference(less[0], lw_inj, less[1], im, less[2], ic, n_grid)
        assert np.array_equal(want_live, live[k])
        f, lives = U.statement_event_cdfs(less[0], less[1], less[2], n_grid)
        tols = U.log_sum_bounds(f, lives, n_grid)
        for slot, tol in ((2, tols[0]), (3, tols[1])):
            inf = np.isneginf(want[slot])
            assert np.array_equal(np.isneginf(out[k, slot]), inf) and np.all(np.abs(out[k, slot][~inf] - want[slot][~inf]) <= tol[~inf])
        assert np.all(np.abs(out[k, 1] - want[1]) <= (max(U.f_rel_bound(n, n_grid) for n in lives) + 4 * U.U) * want[1])


def test_bits_are_a_function_of_the_arguments():
    """K = 3 in one call, as 2 + 1 and as 1 + 1 + 1 concatenate to the same bits; the same call twice; a second handle on the same
    catalog; a call of K = 70 crosses the 64-point staging chunk: its rows 0-2 are those of the K = 3 call and rows 64-69 those of the
    points they repeat; the diagnostic reports five launches per point."""
    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 256
    _set(eng, n_grid)
    whole = eng.point_cdfs(thetas)
    again = eng.point_cdfs(thetas)
    assert _same(whole[0], again[0]) and np.array_equal(whole[1], again[1])
    assert not np.array_equal(whole[0][0], whole[0][1])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_cdf_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 15 and all(m.value > 0.0 for m in ms)
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        parts, at = [], 0
        for n in split:
            parts.append(eng.point_cdfs(thetas[at : at + n]))
            at += n
        assert _same(np.concatenate([p[0] for p in parts]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in parts]), whole[1]), split
    single = eng.point_cdfs(thetas[1])  # one point given as (n_theta,)
    assert single[0].shape == (1, 4, 2, n_grid) and _same(single[0][0], whole[0][1])
    many = np.tile(thetas, (24, 1))[:70]
    out, live = eng.point_cdfs(many)
    assert out.shape == (70, 4, 2, n_grid) and _same(out[:3], whole[0]) and np.array_equal(live[:3], whole[1])
    for k in range(70):
        assert _same(out[k], whole[0][k % 3]) and np.array_equal(live[k], whole[1][k % 3]), k
    eng2 = U.composition().engine()
    try:
        pc, ic = U.codes(n_grid)
        eng2.set_histogram_bins(pc, ic, n_bins=n_grid)
        other = eng2.point_cdfs(thetas)
        assert _same(other[0], whole[0]) and np.array_equal(other[1], whole[1])
    finally:
        eng2.close()


def test_no_side_effects():
    """A weighted_histograms call before and after a point_cdfs call returns identical bits; a marginal_weights_add /
    weighted_quantiles sequence with point_cdfs calls in between returns what it returns without them."""
    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 5
    _set(eng, n_grid)
    pe_values, inj_values = U.values()
    x_pe, x_inj = np.stack([pe_values[k] for k in U.COLUMNS]), np.stack([inj_values[k] for k in U.COLUMNS])
    eng.set_quantile_columns(x_pe, x_inj)

    def quantiles(interleave):
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas[:2])
        if interleave:
            eng.point_cdfs(thetas)
        eng.marginal_weights_add(thetas[2:])
        if interleave:
            eng.point_cdfs(thetas[1])
        return eng.weighted_quantiles(np.array([0.05, 0.5, 0.95])), eng.marginal_weights()

    before = eng.weighted_histograms(thetas)
    plain = quantiles(False)
    cdfs = eng.point_cdfs(thetas)
    after = eng.weighted_histograms(thetas)
    mixed = quantiles(True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    for a, b in zip(tuple(plain[0]) + tuple(plain[1][:3]), tuple(mixed[0]) + tuple(mixed[1][:3])):
        assert np.array_equal(a, b)
    assert plain[1][3] == mixed[1][3] == 3
    assert _same(eng.point_cdfs(thetas)[0], cdfs[0])


def test_errors_and_single_sets():
    """Before set_histogram_bins the call answers GWI_ERR_INVALID with a message; null pointers and k < 1 likewise, and nothing is
    written; PE-only bins give slot 0 NaN and injection-only bins slots 1-3 NaN, the other slots keeping their bits; an engine that
    holds a shard is refused with UNSUPPORTED at the Python guard (test_gpu_hist.py builds no world > 1 engine either)."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    comp = U.composition()
    eng = comp.engine()
    try:
        theta, n_grid = _case()["thetas"][0], 5
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):
            eng.point_cdfs(theta)
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th, out, live = N.f64(theta), np.full((1, 4, 2, n_grid), 7.0), np.full((1, 2), 7, dtype=np.int32)
        assert lib.gwi_point_cdfs(eng.handle, N.as_dp(th), 1, N.as_dp(out), live.ctypes.data_as(i32)) == -1
        assert "gwi_point_cdfs: no bins are set" in lib.gwi_last_error(eng.handle).decode()
        pc, ic = U.codes(n_grid)
        eng.set_histogram_bins(pc, ic, n_bins=n_grid)
        for args, word in (((None, 1, N.as_dp(out), live.ctypes.data_as(i32)), "thetas"), ((N.as_dp(th), 0, N.as_dp(out), live.ctypes.data_as(i32)), "k < 1"),
                           ((N.as_dp(th), 1, None, live.ctypes.data_as(i32)), "out is null"), ((N.as_dp(th), 1, N.as_dp(out), None), "live is null")):
            assert lib.gwi_point_cdfs(eng.handle, *args) == -1
            assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
        assert np.all(out == 7.0) and np.all(live == 7)
        both = eng.point_cdfs(theta)
        assert np.array_equal(both[1], [[U.N_EV, 1]]) and not np.any(np.isnan(both[0]))
        eng.set_histogram_bins(pc, None, n_bins=n_grid)
        only_pe = eng.point_cdfs(theta)
        eng.set_histogram_bins(None, ic, n_bins=n_grid)
        only_inj = eng.point_cdfs(theta)
        assert np.all(np.isnan(only_pe[0][:, 0])) and np.array_equal(only_pe[0][:, 1:], both[0][:, 1:]) and np.array_equal(only_pe[1], [[U.N_EV, 0]])
        assert np.all(np.isnan(only_inj[0][:, 1:])) and np.array_equal(only_inj[0][:, 0], both[0][:, 0]) and np.array_equal(only_inj[1], [[0, 1]])
        shared = _case()["eng"]
        _set(shared, n_grid)
        assert _same(shared.point_cdfs(theta)[0], both[0])  # the refused calls left nothing behind
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_cdfs"):
        shard.point_cdfs(np.zeros(3))


def test_catalog_predictive_check_device_against_host():
    """postprocess.catalog_predictive_check on both backends with the leave-one-out weights of event 0 on the k axis: the raw arrays
    agree within the bounds of the first two tests; the bands are values of the raw arrays, so they agree within the same bounds (and
    to the bit wherever the raw arrays do); the means of the exponentiated quantities likewise."""
    from gwinferno_amd import postprocess as P

    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 5
    _, _, total = U.catalog()
    v = P.leave_one_out_weights(eng, thetas, total)["point_weights"][:, 0]
    assert v.shape == (U.N_POINTS,) and v.max() == 1.0 and np.all(v > 0.0)
    pe_values, inj_values = U.values()
    kw = dict(inj_values=inj_values, point_weights=v, param_names=list(U.COLUMNS))
    dev = P.catalog_predictive_check(eng, thetas, pe_values, U.grid(n_grid), **kw)
    host = P.catalog_predictive_check(eng, thetas, pe_values, U.grid(n_grid), backend="host", **kw)
    assert dev["names"] == list(U.COLUMNS) and np.array_equal(dev["n_live"], host["n_live"]) and dev["dead_detected"] == host["dead_detected"] == 0
    pc, _ = U.codes(n_grid)
    r_f = max(U.f_rel_bound(U.N_PE, n_grid), U.f_rel_bound(U.N_INJ, n_grid)) + 4 * U.U  # (the mean over the events: two additions and a division on either side)
    tol_below, tol_above = np.zeros((U.N_POINTS, 2, n_grid)), np.zeros((U.N_POINTS, 2, n_grid))
    for k, (lw_pe, _) in enumerate(c["lw"]):
        f, lives = U.statement_event_cdfs(lw_pe, None, pc, n_grid)
        tol_below[k], tol_above[k] = U.log_sum_bounds(f, lives, n_grid)
    for key in ("cdf_detected", "cdf_observed"):
        assert np.all(np.abs(dev[key] - host[key]) <= r_f * host[key]), key
    for key, tol in (("log_cdf_max_observed", tol_below), ("log_sf_min_observed", tol_above)):
        inf = np.isneginf(host[key])
        assert np.array_equal(np.isneginf(dev[key]), inf) and np.all(np.abs(dev[key][~inf] - host[key][~inf]) <= tol[~inf]), key
    # n_obs log F and n_obs log1p(-F) of the detected CDF, computed by the same host code on both sides from F within r_f
    n_obs = float(U.N_EV)
    move = r_f * host["cdf_detected"] / (1.0 - host["cdf_detected"])
    tol_below_pred = n_obs * (1.01 * r_f + 2 * U.U * np.abs(np.log(host["cdf_detected"])))
    tol_above_pred = n_obs * (1.01 * move + 2 * U.U * np.abs(np.log1p(-host["cdf_detected"])))
    assert np.all(np.abs(dev["log_cdf_max_predicted"] - host["log_cdf_max_predicted"]) <= tol_below_pred)
    assert np.all(np.abs(dev["log_sf_min_predicted"] - host["log_sf_min_predicted"]) <= tol_above_pred)
    for key in ("bands_detected", "bands_observed"):  # a band is one of the K values: within the bound of the raw array at the same entry
        assert np.all(np.abs(dev[key] - host[key]) <= r_f * host[key]) and np.all(np.diff(dev[key], axis=0) >= 0.0), key
        raw = dev["cdf_" + key[6:]]
        assert np.all((dev[key][:, None] == raw[None]).any(axis=1))
    # exp of a quantity within t of another is within expm1(t) relative; the weighted mean keeps that (non-negative terms)
    for key, tol in (("cdf_max_observed", tol_below.max(axis=0)), ("cdf_max_predicted", tol_below_pred.max(axis=0))):
        assert np.all(np.abs(dev[key] - host[key]) <= (np.expm1(tol) + 4 * U.U) * host[key]), key
    assert np.array_equal(dev["cdf_max_observed"][1], np.zeros(n_grid)) and np.all(dev["cdf_max_observed"][0] > 0.0)
    for key, log_key, tol in (("cdf_min_observed", "log_sf_min_observed", tol_above.max(axis=0)), ("cdf_min_predicted", "log_sf_min_predicted", tol_above_pred.max(axis=0))):
        sf = np.exp(host[log_key]).max(axis=0)  # 1 - cdf_min: the survival function moves by expm1(t) of itself at most
        assert np.all(np.abs(dev[key] - host[key]) <= (np.expm1(tol) + 4 * U.U) * sf + 4 * U.U), key


def test_mock_catalog_sanity():
    """The smallest mock catalog of the suite (tests/mock_util.py; 8 events x 256 samples as in test_gpu_hist.py) at the true
    hyper-parameters repeated with small perturbations, on a grid over the whole mass range: cdf_max_predicted and cdf_max_observed
    both rise from 0 to 1 across the grid, and the observed median band lies inside [0, 1] and does not decrease.  No statistical
    assertion."""
    import mock_util as MU

    from gwinferno_amd import mock_catalog as MC
    from gwinferno_amd import postprocess as P
    from gwinferno_amd.compositions import COMPOSITIONS

    model = MU.catalog_model(MC)
    pe, inj, total, _ = MC.make_mock_catalog(MU.population(MC, on_host=False), MU.injection_tables(model), model, 8, 256, 20_000, 3)
    inj = {k: v for k, v in inj.items() if k != "snr"}
    comp = COMPOSITIONS["plpeak"](pe, inj, mmin=MU.MMIN, mmax=MU.MMAX)
    eng = comp.engine()
    try:
        base = {k: MU.THETA[k] for k in comp.PARAMS}
        rng = np.random.default_rng(4)
        thetas = np.stack([comp.theta({k: v * (1.0 + (0.02 * rng.standard_normal() if i else 0.0)) for k, v in base.items()}) for i in range(6)])
        grid = np.geomspace(MU.MMIN * 0.9, MU.MMAX * 1.1, 64)
        r = P.catalog_predictive_check(eng, thetas, {"mass_1": pe["mass_1"]}, grid, inj_values={"mass_1": inj["mass_1"]})
        assert np.array_equal(r["n_live"], np.full(6, 8)) and r["dead_detected"] == 0
        for key in ("cdf_max_predicted", "cdf_max_observed"):
            curve = r[key][0]
            assert curve[0] == 0.0 and abs(curve[-1] - 1.0) <= 1e-9 and np.all(np.diff(curve) >= -1e-12) and np.all((curve >= 0.0) & (curve <= 1.0 + 1e-12)), key
        median = r["bands_observed"][1, 0]
        assert np.all((median >= 0.0) & (median <= 1.0 + 1e-12)) and np.all(np.diff(median) >= -1e-12) and median[0] == 0.0 and abs(median[-1] - 1.0) <= 1e-9
    finally:
        eng.close()
