"""GPU: marginal weights and weighted quantiles on the device (include/gwi_engine.h: gwi_marginal_weights_add,
gwi_weighted_quantiles; gwinferno_amd/csrc/gwi_quant.h) against their NumPy statement (gwinferno_amd/draws.py:
marginal_weights_reference, weighted_quantiles_reference), their determinism across calls, handles and the split of a request, dead
segments and underflowing weights, their agreement with the weighted histograms, the user-facing function, the refusals and the
lifetime of the handle's state.

Shapes (tests/hist_util.py, tests/quant_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 600 injections
(three tiles), 1 and 8 columns, 5 and 32 levels, K = 3 points, a PL+Peak and a B-spline model.  The inputs are vetted without a
device in tests/test_quant_cpu.py: test_inputs_of_the_gpu_tests."""
import ctypes as C
import gc
import os

import hist_util as U
import numpy as np
import pytest
import quant_util as QU

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """One engine per composition with its three points and their log-weights from the device: made once, shared, never changed."""
    if name not in _CASES:
        comp = U.composition(name)
        eng = comp.engine()
        thetas = U.points(comp, name, QU.K)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas]
        lw_pe, lw_inj = np.stack([a for a, _ in lw]), np.stack([b for _, b in lw])
        lw_pe.setflags(write=False)
        lw_inj.setflags(write=False)
        _CASES[name] = dict(comp=comp, eng=eng, thetas=thetas, lw=(lw_pe, lw_inj))
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
    _CASES.clear()


def _accumulate(eng, thetas, masks=(None, None)):
    try:
        eng.set_draw_mask(*masks)
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas)
    finally:
        eng.set_draw_mask()
    return eng.marginal_weights()


def _mass(W, order, x, mass, col):
    """What check_segment holds against the statement's C_last: the device's mass for column 0, whose order it is summed in; for
    another column (the same W summed in another order: equal but for rounding) the statement's own."""
    from gwinferno_amd.draws import weighted_quantiles_reference

    return mass if col == 0 else weighted_quantiles_reference(W, order, x, [0.5])[2]


def _same(a, b):
    """Equal bits, entry by entry (arrays, None for a set that is left out, and the integer n_points)."""
    return len(a) == len(b) and all((x is None and y is None) or (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y))
                                    or (isinstance(x, int) and x == y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", U.MASK_CASES)
@pytest.mark.parametrize("name", U.COMPS)
def test_marginal_weights_against_statement(name, case):
    """W, dead and n_points after K = 3 points against marginal_weights_reference on eng.log_weights of the same points, with and
    without masks.  The bound is DERIVED (quant_util.weight_bound): (n_live + 8 + K) 2^-52 relative; a sample the statement leaves at
    0 must be 0.  Then W against the independent host evaluation (tests/bound_eval.py) at the project's 1e-9, and a reset: zeros."""
    from gwinferno_amd.draws import marginal_weights_reference

    c = _case(name)
    eng, thetas, (lw_pe, lw_inj) = c["eng"], c["thetas"], c["lw"]
    pm, im = U.masks(case)
    W_pe, W_inj, dead, n_points = _accumulate(eng, thetas, (pm, im))
    want_pe, want_inj, want_dead, want_n = marginal_weights_reference(lw_pe, lw_inj, pm, im)
    assert W_pe.shape == (U.N_EV, U.N_PE) and W_inj.shape == (U.N_INJ,) and dead.dtype == np.int32 and n_points == want_n == QU.K
    assert np.array_equal(dead, want_dead) and dead[U.DEAD_EVENT] == (QU.K if case == "masked" else 0)
    worst = 0.0
    for seg in range(U.N_EV + 1):
        g, w = (W_pe[seg], want_pe[seg]) if seg < U.N_EV else (W_inj, want_inj)
        live = max(U.n_live(lw_pe[p, seg] if seg < U.N_EV else lw_inj[p], None if (pm if seg < U.N_EV else im) is None else (pm[seg] if seg < U.N_EV else im)) for p in range(QU.K))
        tol = QU.weight_bound(live)
        assert np.all(np.isfinite(g)) and np.array_equal(g == 0.0, w == 0.0), (name, case, seg)
        dev = np.abs(g - w)
        assert np.all(dev <= tol * w), (name, case, seg, float(np.max(dev[w > 0] / w[w > 0])), tol)
        if np.any(w > 0):
            worst = max(worst, float(np.max(dev[w > 0] / w[w > 0])) / tol)
            assert abs(g.sum() - QU.K) <= 1e-9
    print(f"{name} {case}: largest |device - statement| / statement of W = {worst:.3f} of the derived bound")
    host = [U.host_log_weights(eng.bound, th) for th in thetas]
    h_pe, h_inj, h_dead, _ = marginal_weights_reference(np.stack([a for a, _ in host]), np.stack([b for _, b in host]), pm, im)
    assert np.array_equal(dead, h_dead) and np.allclose(W_pe, h_pe, rtol=1e-9, atol=1e-300) and np.allclose(W_inj, h_inj, rtol=1e-9, atol=1e-300)
    eng.marginal_weights_reset()
    z_pe, z_inj, z_dead, z_n = eng.marginal_weights()
    assert not z_pe.any() and not z_inj.any() and not z_dead.any() and z_n == 0


@pytest.mark.parametrize("levels", (QU.LEVELS, QU.LEVELS_32), ids=("5 levels", "32 levels"))
@pytest.mark.parametrize("n_cols", (1, 8))
@pytest.mark.parametrize("name", U.COMPS)
def test_quantiles_and_moments_against_statement(name, n_cols, levels):
    """Indices, moments and mass of every (segment, column) against weighted_quantiles_reference on the W read back from the device,
    with and without masks (quant_util.check_segment: the index equals the statement's, but for a level whose target lies within the
    derived band of a prefix value; at most 1 case in 100 may); p = 0 gives the smallest value with weight and p = 1 the largest."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp, vi = QU.columns(n_cols)
    op, oi = QU.orders(n_cols)
    eng.set_quantile_columns(vp, vi)
    cases, in_band = 0, 0
    for case in U.MASK_CASES:
        W_pe, W_inj, dead, _ = _accumulate(eng, thetas, U.masks(case))
        idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(levels)
        assert idx_pe.shape == (U.N_EV, n_cols, len(levels)) and idx_inj.shape == (n_cols, len(levels)) and idx_pe.dtype == idx_inj.dtype == np.int32
        assert mom_pe.shape == (U.N_EV, n_cols, 2) and mom_inj.shape == (n_cols, 2) and mass.shape == (U.N_EV + 1,)
        for seg in range(U.N_EV + 1):
            W = W_pe[seg] if seg < U.N_EV else W_inj
            for col in range(n_cols):
                x, order, gi, gm = (vp[col, seg], op[col, seg], idx_pe[seg, col], mom_pe[seg, col]) if seg < U.N_EV else (vi[col], oi[col], idx_inj[col], mom_inj[col])
                in_band += QU.check_segment(W, order, x, levels, gi, gm, _mass(W, order, x, mass[seg], col), (name, case, seg, col))
                cases += len(levels)
                if W.any():
                    live_x = x[W > 0]
                    assert x[gi[0]] == live_x.min() and x[gi[-1]] == live_x.max() and levels[0] == 0.0 and levels[-1] == 1.0
                else:
                    assert seg == U.DEAD_EVENT and case == "masked" and np.all(gi == -1)
    print(f"{name} C = {n_cols} Q = {len(levels)}: {cases} (mask case, segment, column, level) cases, {in_band} in the band")
    assert in_band * 100 <= cases


@pytest.mark.parametrize("name", U.COMPS)
def test_determinism(name):
    """The bits of W, of the indices and of the moments: one call of 3 points equals 2 + 1 and 1 + 1 + 1; a second identical call
    after a reset; a second handle of the same model; a query repeated; a query after the columns were replaced and set back."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp, vi = QU.columns(8)
    eng.set_quantile_columns(vp, vi)
    whole = _accumulate(eng, thetas)
    q_whole = eng.weighted_quantiles(QU.LEVELS)
    assert _same(q_whole, eng.weighted_quantiles(QU.LEVELS))  # repeated
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        eng.marginal_weights_reset()
        at = 0
        for n in split:
            eng.marginal_weights_add(thetas[at : at + n])
            at += n
        assert _same(whole, eng.marginal_weights()), split
        assert _same(q_whole, eng.weighted_quantiles(QU.LEVELS)), split
    assert _same(whole, _accumulate(eng, thetas))  # a second identical call after a reset
    eng.marginal_weights_add(np.zeros((0, eng.n_theta)))  # no point: nothing changes
    assert _same(whole, eng.marginal_weights())
    eng.set_quantile_columns(vp[:1], None)  # replaced (one column, PE only) ...
    one = eng.weighted_quantiles(QU.LEVELS)
    assert one[1] is None and one[3] is None and np.array_equal(one[0][:, 0], q_whole[0][:, 0]) and np.array_equal(one[2][:, 0], q_whole[2][:, 0])
    assert np.array_equal(one[4][: U.N_EV], q_whole[4][: U.N_EV]) and one[4][U.N_EV] == 0.0
    eng.set_quantile_columns(None, vi[:2])
    two = eng.weighted_quantiles(QU.LEVELS)
    assert two[0] is None and np.array_equal(two[1], q_whole[1][:2]) and np.array_equal(two[3], q_whole[3][:2]) and two[4][U.N_EV] == q_whole[4][U.N_EV] and not two[4][: U.N_EV].any()
    eng.set_quantile_columns(vp, vi)        # ... and set back: the accumulation does not depend on the columns
    assert _same(q_whole, eng.weighted_quantiles(QU.LEVELS)) and _same(whole, eng.marginal_weights())
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_quantile_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 3 and ms[2].value > 0.0
    comp2 = U.composition(name)
    eng2 = comp2.engine()
    try:
        eng2.set_quantile_columns(vp, vi)
        assert _same(whole, _accumulate(eng2, thetas)) and _same(q_whole, eng2.weighted_quantiles(QU.LEVELS))
        eng2.lib.gwi_quantile_times(*[C.byref(m) for m in ms], C.byref(n_launch))
        assert ms[0].value > 0.0 and ms[1].value > 0.0
    finally:
        eng2.close()


def test_dead_event_and_wide_spread():
    """A theta that sends one event's weights to -inf: index -1, NaN mean, dead incremented, the other events as without it.  A
    log-weight spread above 800 within one event: the quantiles lie among the few samples with weight."""
    from gwinferno_amd import postprocess as P

    c = _case("plpeak")
    eng, comp, thetas = c["eng"], c["comp"], c["thetas"]
    vp, vi = QU.columns(8)
    eng.set_quantile_columns(vp, vi)
    theta = comp.theta(U.dead_event_params())
    finite = np.isfinite(eng.log_weights(theta)[0]).sum(axis=1)
    assert finite.min() == 0 and finite.max() >= 200
    gone = np.nonzero(finite == 0)[0]
    alone = _accumulate(eng, thetas[:1])
    q_alone = eng.weighted_quantiles(QU.LEVELS)
    both = _accumulate(eng, np.stack([theta, thetas[0]]))
    q_both = eng.weighted_quantiles(QU.LEVELS)
    assert both[3] == 2 and np.array_equal(both[2][: U.N_EV], (finite == 0).astype(np.int32))
    for ev in gone:  # the dead point added nothing: the sums are the second point's
        assert np.array_equal(both[0][ev], alone[0][ev]) and np.array_equal(q_both[0][ev], q_alone[0][ev]) and np.array_equal(q_both[2][ev], q_alone[2][ev])
    only = _accumulate(eng, theta)
    idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(QU.LEVELS)
    assert np.array_equal(only[2][: U.N_EV], (finite == 0).astype(np.int32)) and np.all(np.isfinite(mom_pe)) and np.all(np.isfinite(mass))
    for ev in range(U.N_EV):
        if ev in gone:
            assert np.all(idx_pe[ev] == -1) and mass[ev] == 0.0 and not mom_pe[ev].any() and not only[0][ev].any()
        else:
            assert np.all(idx_pe[ev] >= 0) and abs(mass[ev] - 1.0) <= 1e-12
            for col in range(8):
                order = QU.orders(8)[0][col, ev]
                QU.check_segment(only[0][ev], order, vp[col, ev], QU.LEVELS, idx_pe[ev, col], mom_pe[ev, col], _mass(only[0][ev], order, vp[col, ev], mass[ev], col), ("dead-event point", ev, col))
    pe, inj, _ = U.catalog()
    out = P.event_credible_intervals(eng, theta[None], {"mass_1": pe["mass_1"]})
    for ev in range(U.N_EV):
        assert (np.all(np.isnan(out["quantiles"][ev])) and np.isnan(out["mean"][ev, 0]) and np.isnan(out["sd"][ev, 0]) and out["dead"][ev] == 1) == (ev in gone)
    # a spread above 800 within one event
    theta = comp.theta(U.wide_spread_params())
    lw_pe, lw_inj = eng.log_weights(theta)
    spread = [float(np.ptp(r[np.isfinite(r)])) if np.isfinite(r).any() else 0.0 for r in lw_pe]
    assert max(spread) > 800.0
    eng.set_quantile_columns(vp, vi)
    W_pe, W_inj, dead, _ = _accumulate(eng, theta)
    idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(QU.LEVELS)
    assert np.all(np.isfinite(W_pe)) and np.all(W_pe >= 0.0) and np.all(np.isfinite(mom_pe)) and not dead.any()
    n_with = (W_pe > 0).sum(axis=1)
    print("samples with weight per event at the wide-spread point:", n_with, "of", U.N_PE)
    assert n_with.min() < U.N_PE  # some weights underflow to 0
    for ev in range(U.N_EV):
        assert np.all(idx_pe[ev] >= 0) and np.all(W_pe[ev][idx_pe[ev]] > 0.0)  # among the samples with weight
        for col in range(8):
            x = vp[col, ev]
            assert x[idx_pe[ev, col, 0]] == x[W_pe[ev] > 0].min() and x[idx_pe[ev, col, -1]] == x[W_pe[ev] > 0].max() and np.all(np.diff(x[idx_pe[ev, col]]) >= 0)


@pytest.mark.parametrize("name", U.COMPS)
def test_cross_check_against_the_histogram_kernels(name):
    """Edges that span every sample, so that nothing is outside: the cumulative weighted_histograms up to and including the bin that
    holds a quantile's value is >= p (K - dead) minus the two bounds, and strictly below that bin it is <= p (K - dead) plus the two
    bounds (hist_util.bound for every bin sum, quant_util.weight_bound for W: both relative, of a total of at most K)."""
    from gwinferno_amd.draws import digitize

    c = _case(name)
    eng, thetas, (lw_pe, lw_inj) = c["eng"], c["thetas"], c["lw"]
    vp, vi = QU.columns(1)
    n_bins = 64
    lo, hi = min(vp.min(), vi.min()), max(vp.max(), vi.max())
    edges = np.linspace(lo, hi, n_bins + 1)
    pb, ib = digitize(vp, edges), digitize(vi, edges)
    assert np.all(pb < n_bins) and np.all(ib < n_bins)
    eng.set_histogram_bins(pb, ib, n_bins=n_bins)
    hp, hi_, hdead = eng.weighted_histograms(thetas)
    eng.set_quantile_columns(vp, vi)
    _, _, dead, n_points = _accumulate(eng, thetas)
    idx_pe, idx_inj, _, _, _ = eng.weighted_quantiles(QU.LEVELS)
    assert np.array_equal(dead, hdead) and n_points == QU.K
    for seg in range(U.N_EV + 1):
        h, idx, code = (hp[seg, 0], idx_pe[seg, 0], pb[0, seg]) if seg < U.N_EV else (hi_[0], idx_inj[0], ib[0])
        live = max(U.n_live(lw_pe[p, seg] if seg < U.N_EV else lw_inj[p], None) for p in range(QU.K))
        total = float(QU.K - dead[seg])
        tol = (U.bound(live) + QU.weight_bound(live)) * total
        cum = np.cumsum(h)
        for q, p in enumerate(QU.LEVELS):
            b = int(code[idx[q]])
            assert cum[b] >= p * total - tol and (cum[b - 1] if b else 0.0) <= p * total + tol, (name, seg, p, b, cum[b], p * total)


def test_event_credible_intervals():
    """The user-facing function on the device against backend="host" (the statement on eng.log_weights): the same quantiles but for
    levels in the band, the mean and sd to the derived bounds' scale; with and without mass cuts; with pedata / param_names and with
    arrays."""
    from gwinferno_amd import postprocess as P

    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    pe, inj, _ = U.catalog()
    names = ["mass_1", "mass_2", "mass_ratio"]
    pe_values, inj_values = {k: pe[k] for k in names}, {k: inj[k] for k in names}
    for cuts in ({}, dict(pedata=pe, injdata=inj, m1min=6.0, m2min=4.0, mmax=70.0)):
        try:
            dev = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, return_weights=True, **cuts)
            host = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, backend="host", return_weights=True, **cuts)
        finally:
            eng.set_draw_mask()
        assert dev["names"] == host["names"] == names and dev["n_points"] == host["n_points"] == QU.K
        assert dev["quantiles"].shape == (U.N_EV, 3, 3) and dev["quantiles_inj"].shape == (3, 3) and dev["mean"].shape == (U.N_EV, 3) and dev["sd_inj"].shape == (3,)
        assert np.array_equal(dev["dead"], host["dead"]) and dev["dead_inj"] == host["dead_inj"] == 0 and not dev["dead"].any()
        assert np.array_equal(dev["quantiles"], host["quantiles"]) and np.array_equal(dev["quantiles_inj"], host["quantiles_inj"])
        for k in ("mean", "sd", "mean_inj", "sd_inj", "weights", "weights_inj"):
            assert np.allclose(dev[k], host[k], rtol=1e-9, atol=1e-300), k
        assert np.all(dev["quantiles"][:, :, 0] <= dev["quantiles"][:, :, 1]) and np.all(dev["quantiles"][:, :, 1] <= dev["quantiles"][:, :, 2])
        assert np.all(dev["quantiles"][:, :, 0] <= dev["mean"] + 3 * dev["sd"]) and np.all(dev["sd"] > 0)
        if cuts:  # the cuts leave no sample outside them with weight
            from gwinferno_amd.draws import mass_cut_masks

            pm, im = mass_cut_masks(pe, inj, 6.0, 4.0, 70.0)
            assert pm.min() == 0 and not dev["weights"][pm == 0].any() and not dev["weights_inj"][im == 0].any()
            assert np.all(dev["quantiles"][:, 0, :] >= 6.0) and np.all(dev["quantiles"][:, 0, :] <= 70.0)
    arrays = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, param_names=["mass_2"], levels=[0.5])
    named = P.event_credible_intervals(eng, thetas, None, pedata=pe, injdata=inj, param_names=["mass_2"], levels=[0.5])
    assert "weights" not in named and np.array_equal(arrays["quantiles"], named["quantiles"]) and np.array_equal(arrays["mean_inj"], named["mean_inj"])


def test_refusals():
    """Every refusal of the C ABI with its message and without a launch; the handle keeps working afterwards."""
    from gwinferno_amd import _native as N

    comp = U.composition("plpeak")
    eng = comp.engine()
    try:
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        theta = comp.theta(U.params("plpeak"))
        vp, vi = QU.columns(1)
        op, oi = QU.orders(1)
        ip = lambda a: a.ctypes.data_as(i32)  # noqa: E731
        err = lambda: lib.gwi_last_error(eng.handle).decode()  # noqa: E731
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no columns are set"):
            eng.weighted_quantiles([0.5])
        # nothing accumulated is valid: every index -1, mass 0
        eng.set_quantile_columns(vp, vi)
        idx_pe, idx_inj, mom_pe, mom_inj, mass = eng.weighted_quantiles(QU.LEVELS)
        assert np.all(idx_pe == -1) and np.all(idx_inj == -1) and not mass.any() and not mom_pe.any() and not mom_inj.any()
        assert eng.marginal_weights()[3] == 0
        th, dead, n, mass = N.f64(theta), np.zeros(U.N_EV + 1, dtype=np.int32), C.c_int64(0), np.zeros(U.N_EV + 1)
        assert lib.gwi_marginal_weights_add(eng.handle, None, 1) == -1 and "thetas is null" in err()
        assert lib.gwi_marginal_weights_add(eng.handle, N.as_dp(th), -1) == -1 and "k < 0" in err()
        assert lib.gwi_marginal_weights_read(eng.handle, None, None, None, C.byref(n)) == -1 and "dead or n_points is null" in err()
        assert lib.gwi_marginal_weights_read(eng.handle, None, None, ip(dead), None) == -1 and "dead or n_points is null" in err()
        cols = lambda n_cols, xp, o_p, xi, o_i: lib.gwi_set_quantile_columns(eng.handle, n_cols, N.as_dp(xp), None if o_p is None else ip(o_p), N.as_dp(xi), None if o_i is None else ip(o_i))  # noqa: E731
        eight_p, eight_i = QU.columns(8), QU.orders(8)
        nine = (np.concatenate([eight_p[0], eight_p[0][:1]]), np.concatenate([eight_i[0], eight_i[0][:1]]), np.concatenate([eight_p[1], eight_p[1][:1]]), np.concatenate([eight_i[1], eight_i[1][:1]]))
        assert cols(9, *[np.ascontiguousarray(a) for a in nine]) == -1 and "n_cols = 9 is not in 1 ... 8" in err()
        assert cols(0, vp, op, vi, oi) == -1 and "n_cols = 0" in err()
        assert cols(1, None, None, None, None) == -1 and "both null" in err()
        assert cols(1, vp, None, vi, oi) == -1 and "x_pe and order_pe are given together" in err()
        assert cols(1, vp, op, vi, None) == -1 and "x_inj and order_inj are given together" in err()
        bad = oi.copy()
        bad[0, 7] = bad[0, 8]
        assert cols(1, vp, op, vi, bad) == -1 and "order_inj column 0: rank 8 holds" in err() and "not a permutation" in err()
        bad = op.copy()
        bad[0, 2, 0] = U.N_PE
        assert cols(1, vp, bad, vi, oi) == -1 and f"order_pe column 0, event 2: rank 0 holds {U.N_PE}" in err()
        bad = op.copy()
        bad[0, 1, [10, 900]] = bad[0, 1, [900, 10]]
        assert cols(1, vp, bad, vi, oi) == -1 and "x_pe column 0, event 1: the values decrease along the order at rank" in err()
        bad = vi.copy()
        bad[0, 11] = np.inf
        assert cols(1, vp, op, bad, oi) == -1 and "x_inj column 0: sample 11 is not finite" in err()
        # none of the refused calls replaced the columns
        quant = lambda lv, n_lv, a, b, m_p, m_i, ms: lib.gwi_weighted_quantiles(eng.handle, N.as_dp(lv), n_lv, None if a is None else ip(a), None if b is None else ip(b), N.as_dp(m_p), N.as_dp(m_i), N.as_dp(ms))  # noqa: E731
        lv = np.array(QU.LEVELS)
        a, b, m_p, m_i = np.zeros((U.N_EV, 1, 5), dtype=np.int32), np.zeros((1, 5), dtype=np.int32), np.zeros((U.N_EV, 1, 2)), np.zeros((1, 2))
        assert quant(lv, 5, a, b, m_p, m_i, mass) == 0
        assert quant(lv, 0, a, b, m_p, m_i, mass) == -1 and "n_levels = 0 is not in 1 ... 32" in err()
        assert quant(np.zeros(33), 33, a, b, m_p, m_i, mass) == -1 and "n_levels = 33" in err()
        assert quant(None, 5, a, b, m_p, m_i, mass) == -1 and "levels is null" in err()
        for wrong in (np.nan, -0.01, 1.01, np.inf):
            assert quant(np.array([0.5, wrong]), 2, a, b, m_p, m_i, mass) == -1 and "level 1 is" in err() and "not in [0, 1]" in err()
        assert quant(lv, 5, None, b, m_p, m_i, mass) == -1 and "idx_pe and moments_pe are needed" in err()
        assert quant(lv, 5, a, b, None, m_i, mass) == -1 and "idx_pe and moments_pe are needed" in err()
        assert quant(lv, 5, a, None, m_p, m_i, mass) == -1 and "idx_inj and moments_inj are needed" in err()
        assert quant(lv, 5, a, b, m_p, m_i, None) == -1 and "mass is null" in err()
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*level 0 is"):
            eng.weighted_quantiles([1.5])
        # a handle that holds a shard: GWI_ERR_UNSUPPORTED from Python and from the library itself
        from gwinferno_amd.engine import NativePopulationLikelihood

        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
            shards[0].marginal_weights_add(theta)
        seg = f"/gwi_quant_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            sp, si = np.zeros((1, shards[0].n_ev, shards[0].n_pe)), np.zeros((1, shards[0].n_inj))
            so_p, so_i = np.argsort(sp, axis=-1, kind="stable").astype(np.int32), np.argsort(si, axis=-1, kind="stable").astype(np.int32)
            sdead = np.zeros(shards[0].n_ev + 1, dtype=np.int32)
            for st in (lib.gwi_marginal_weights_reset(hs), lib.gwi_marginal_weights_add(hs, N.as_dp(th), 1), lib.gwi_marginal_weights_read(hs, None, None, ip(sdead), C.byref(n)),
                       lib.gwi_set_quantile_columns(hs, 1, N.as_dp(sp), ip(so_p), N.as_dp(si), ip(so_i))):
                assert st == -4 and "this handle holds one shard of the catalog" in lib.gwi_last_error(hs).decode()  # GWI_ERR_UNSUPPORTED
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        # usable after all of it, with the bits of the shared engine
        eng.set_quantile_columns(vp, vi)
        got = _accumulate(eng, theta)
        q = eng.weighted_quantiles(QU.LEVELS)
        ref = _case("plpeak")["eng"]
        ref.set_quantile_columns(vp, vi)
        assert _same(got, _accumulate(ref, theta)) and _same(q, ref.weighted_quantiles(QU.LEVELS)) and got[3] == 1
    finally:
        eng.close()


def test_lifetime():
    """create / set / add / quantiles / destroy over a few handles: every handle gives the first one's bits and device memory returns
    to its starting level (the state is released with the handle)."""
    import torch

    from gwinferno_amd import likelihood

    likelihood.clear_engine_cache()
    gc.collect()
    vp, vi = QU.columns(8)
    free, first = [], None
    for it in range(6):
        comp = U.composition("plpeak")
        eng = comp.engine()
        try:
            thetas = U.points(comp, "plpeak", 2)
            eng.set_quantile_columns(vp, vi)
            if it % 2:  # the columns replaced once, the state reset once: the buffers of either are dropped and made anew
                eng.set_quantile_columns(vp[:2], None)
                eng.set_quantile_columns(vp, vi)
                eng.marginal_weights_add(thetas[:1])
                eng.marginal_weights_reset()
            eng.marginal_weights_add(thetas)
            got = (*eng.marginal_weights(), *eng.weighted_quantiles(QU.LEVELS))
        finally:
            eng.close()
        first = got if first is None else first
        assert all(np.array_equal(a, b) for a, b in zip(first, got)), it
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert abs(free[-1] - free[1]) <= 8 << 20, free  # (the runtime's own pools settle with the first handle)
