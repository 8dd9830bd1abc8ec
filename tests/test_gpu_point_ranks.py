"""GPU: exact per-event calibration on the device (include/gwi_engine.h: gwi_set_rank_columns, gwi_point_pits_exact;
gwinferno_amd/csrc/gwi_rank.h): the full statement (draws.point_pits_exact_reference on the engine's own log-weights) under the
derived bound of tests/rank_util.py, the independent gridded entry (point_pits) on the same handle, determinism over calls, splits,
handles and the staging chunk, the absence of side effects, liveness, the refusals, and postprocess.event_calibration_exact on both
backends.

Shapes (tests/cdf_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 500 injections (three tiles, the last ragged),
three points of a PL+Peak model, two columns: mass_ratio, continuous, and mass_1 rounded to whole solar masses, which ties between the
two sets.  The inputs are vetted without a device in tests/test_rank_cpu.py."""
import ctypes as C
import re

import numpy as np
import pytest
import rank_util as RU

U, PU = RU.CU, RU.PU

pytestmark = pytest.mark.gpu

_CASE = {}


def _case():
    """The engine with its rank columns, its three points and their log-weights from the device: made once, shared."""
    if not _CASE:
        comp = U.composition()
        eng = comp.engine()
        thetas = U.points(comp)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas]
        for pair in lw:
            for a in pair:
                a.setflags(write=False)
        eng.set_rank_columns(*RU.columns())
        _CASE.update(comp=comp, eng=eng, thetas=thetas, lw=lw)
    return _CASE


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    if _CASE:
        _CASE["eng"].close()
    _CASE.clear()


def _same(a, b):
    """equal bits, NaN in the same places"""
    return np.array_equal(a, b, equal_nan=True)


def _exact(eng, thetas, case="free"):
    try:
        eng.set_draw_mask(*U.masks(case))
        return eng.point_pits_exact(thetas)
    finally:
        eng.set_draw_mask()


@pytest.mark.parametrize("case", ("free", "masked"))
def test_against_the_full_statement(case):
    """Every pit of every point against point_pits_exact_reference on eng.log_weights under the DERIVED bound of
    rank_util.device_tolerance.  Flags and NaN positions agree exactly; the masked case's dead event gives NaN rows and dead = 1.  The
    largest deviation is printed in units of the bound."""
    c = _case()
    pm, im = U.masks(case)
    pit, dead = _exact(c["eng"], c["thetas"], case)
    assert pit.shape == (U.N_POINTS, U.N_EV, 2, 2) and dead.shape == (U.N_POINTS, U.N_EV + 1) and dead.dtype == np.int32
    worst = 0.0
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_dead, tol = RU.statement_point(lw_pe, lw_inj, pm, im)
        assert np.array_equal(dead[k], want_dead) and np.array_equal(np.isnan(pit[k]), np.isnan(want))
        assert np.array_equal(np.nonzero(dead[k])[0], [U.DEAD_EVENT] if case == "masked" else [])
        ok = ~np.isnan(want)
        assert ok.sum() == (U.N_EV - (case == "masked")) * 4 and np.all(tol[ok] > 0.0) and tol[ok].max() < 1e-11  # (nothing is left out; a rounding bound)
        dev = np.abs(pit[k][ok] - want[ok])
        print(f"{case}, point {k}: largest |device - statement| = {float(np.max(dev / tol[ok])):.3f} of the derived bound")
        assert np.all(dev <= tol[ok]), (k, float(np.max(dev / tol[ok])))
        worst = max(worst, float(np.max(dev / tol[ok])))
    live = pit[:, [e for e in range(U.N_EV) if case == "free" or e != U.DEAD_EVENT]]
    assert np.all(live >= 0.0) and np.all(live <= 1.0 + 1e-12) and np.array_equal(live[:, :, 0, 0], live[:, :, 0, 1]) and np.all(live[:, :, 1, 0] < live[:, :, 1, 1])
    print(f"{case}: largest |device - statement| of a pit = {worst:.3f} of the derived bound")


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("n_grid", RU.N_GRID + (0,))
def test_against_the_gridded_entry(n_grid, case):
    """The independent existing entry on the same handle: pit_lo - tol <= pit_lt <= pit_le <= pit_hi + tol against point_pits for G = 1, 5
    and 256, with tol the two entries' derived bounds (pit_util.device_tolerance and rank_util.device_tolerance) and the derived
    rounding of the two statements (pit_util.statement_rounding, rank_util.statement_rounding): in exact arithmetic the bracket holds the
    exact value (tests/test_rank_cpu.py).  n_grid = 0 stands for the grid of ALL distinct values of the rounded column: every sample
    sits on a grid point, so pit_lt = pit_lo and pit_le = pit_hi within the same tolerance -- this pins the < / <= ranks and the ties."""
    c = _case()
    eng = c["eng"]
    grid = RU.distinct_grid() if n_grid == 0 else U.grid(n_grid)
    n_bins = grid.shape[1]
    pc, ic = RU.codes(grid)
    pm, im = U.masks(case)
    try:
        eng.set_draw_mask(pm, im)
        eng.set_histogram_bins(pc, ic, n_bins=n_bins)
        bracket, _, b_dead = eng.point_pits(c["thetas"])
        pit, dead = eng.point_pits_exact(c["thetas"])
    finally:
        eng.set_draw_mask()
    assert np.array_equal(dead, b_dead) and np.array_equal(np.isnan(pit), np.isnan(bracket))
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        _, _, _, b_tol = PU.statement_point(lw_pe, lw_inj, pm, im, pc, ic, n_bins)
        _, _, e_tol = RU.statement_point(lw_pe, lw_inj, pm, im)
        n_inj_live = U.HU.n_live(lw_inj, im)
        for e in range(U.N_EV):
            if dead[k, e]:
                continue
            rel, absolute = PU.statement_rounding(U.HU.n_live(lw_pe[e], None if pm is None else pm[e]), n_inj_live, n_bins)
            for col in range(2):
                lo, hi = bracket[k, e, col]
                lt, le = pit[k, e, col]
                slack = rel * hi + absolute + RU.statement_rounding() * le
                tol_lo, tol_hi = b_tol[e, col, 0] + e_tol[e, col, 0] + slack, b_tol[e, col, 1] + e_tol[e, col, 1] + slack
                assert tol_lo < 1e-11 and tol_hi < 1e-11
                assert lo - tol_lo <= lt <= le <= hi + tol_hi, (k, e, col, lo, lt, le, hi)
                if n_grid == 0 and col == RU.ROUNDED:
                    assert abs(lt - lo) <= tol_lo and abs(le - hi) <= tol_hi and le - lt > 1e-4, (k, e, lo, lt, le, hi)


def test_bits_are_a_function_of_the_arguments():
    """K = 3 in one call, as 2 + 1 and as 1 + 1 + 1 concatenate to the same bits; the same call twice; one point given as (n_theta,); a call
    of K = 70 crosses the 64-point staging chunk: row k is that of the point it repeats; a second handle on the same catalog; the
    diagnostic reports seven launches per point."""
    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    whole = eng.point_pits_exact(thetas)
    again = eng.point_pits_exact(thetas)
    assert all(_same(a, b) for a, b in zip(whole, again)) and not np.any(np.isnan(whole[0])) and not whole[1].any()
    assert not np.array_equal(whole[0][0], whole[0][1])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_rank_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 21 and all(m.value > 0.0 for m in ms)
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        parts, at = [], 0
        for n in split:
            parts.append(eng.point_pits_exact(thetas[at : at + n]))
            at += n
        assert all(_same(np.concatenate([p[i] for p in parts]), whole[i]) for i in range(2)), split
    single = eng.point_pits_exact(thetas[1])
    assert single[0].shape == (1, U.N_EV, 2, 2) and _same(single[0][0], whole[0][1])
    out = eng.point_pits_exact(np.tile(thetas, (24, 1))[:70])
    assert out[0].shape == (70, U.N_EV, 2, 2) and out[1].shape == (70, U.N_EV + 1)
    for k in range(70):
        assert all(_same(out[i][k], whole[i][k % 3]) for i in range(2)), k
    eng2 = U.composition().engine()
    try:
        eng2.set_rank_columns(*RU.columns())
        assert all(_same(a, b) for a, b in zip(eng2.point_pits_exact(thetas), whole))
    finally:
        eng2.close()


def test_no_side_effects():
    """weighted_histograms split over two calls, point_pits, a marginal_weights_add / weighted_quantiles sequence with
    marginal_weights (the read-back) each return the bits they return without the new entry when point_pits_exact calls and a
    set_rank_columns call sit in between; point_pits_exact itself repeats after all of them."""
    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 5
    pc, ic = RU.codes(U.grid(n_grid))
    eng.set_histogram_bins(pc, ic, n_bins=n_grid)
    x_pe, x_inj = RU.columns()
    eng.set_quantile_columns(x_pe, x_inj)

    def between(interleave, reset=False):
        if interleave:
            eng.point_pits_exact(thetas)
        if reset:
            eng.set_rank_columns(x_pe, x_inj)

    def histograms(interleave):
        out = eng.weighted_histograms(thetas[:2])
        between(interleave)
        return eng.weighted_histograms(thetas[2:], out=out)

    def quantiles(interleave):
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas[:2])
        between(interleave, reset=interleave)
        eng.marginal_weights_add(thetas[2:])
        between(interleave)
        return eng.weighted_quantiles(np.array([0.05, 0.5, 0.95])), eng.marginal_weights()

    plain_h, plain_q, brackets = histograms(False), quantiles(False), eng.point_pits(thetas)
    exact = eng.point_pits_exact(thetas)
    mixed_h, mixed_q, brackets_after = histograms(True), quantiles(True), eng.point_pits(thetas)
    assert all(np.array_equal(a, b) for a, b in zip(plain_h, mixed_h))
    for a, b in zip(tuple(plain_q[0]) + tuple(plain_q[1][:3]), tuple(mixed_q[0]) + tuple(mixed_q[1][:3])):
        assert np.array_equal(a, b)
    assert plain_q[1][3] == mixed_q[1][3] == 3
    assert all(_same(a, b) for a, b in zip(brackets, brackets_after))
    assert all(_same(a, b) for a, b in zip(eng.point_pits_exact(thetas), exact))


def test_liveness_and_refusals():
    """An injection mask that removes everything gives NaN everywhere and the injection flag beside the dead event's.  On a fresh handle:
    a call before set_rank_columns, k = 0 and k < 0, null pointers through raw ctypes, an order that is no permutation, a rank above
    n_inj and rank_lt > rank_le each answer GWI_ERR_INVALID with a message, without a GPU fault, and write nothing; a refused
    set_rank_columns leaves the entry refusing; afterwards the handle gives the shared engine's bits."""
    from gwinferno_amd import _native as N

    c = _case()
    thetas = c["thetas"]
    free = c["eng"].point_pits_exact(thetas)
    none = _exact(c["eng"], thetas, "no_inj")
    assert np.array_equal(none[1], [[1 if e == U.DEAD_EVENT else 0 for e in range(U.N_EV)] + [1]] * U.N_POINTS) and np.all(np.isnan(none[0]))
    eng = U.composition().engine()
    try:
        theta = thetas[0]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no rank columns are set"):
            eng.point_pits_exact(theta)
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th, pit, dead = N.f64(theta), np.full((1, U.N_EV, 2, 2), 7.0), np.full((1, U.N_EV + 1), 7, dtype=np.int32)
        full = (N.as_dp(th), 1, N.as_dp(pit), dead.ctypes.data_as(i32))
        assert lib.gwi_point_pits_exact(eng.handle, *full) == -1
        assert "gwi_point_pits_exact: no rank columns are set" in lib.gwi_last_error(eng.handle).decode()
        order, lt, le = (np.array(a) for a in RU.ranks())
        ptr = lambda a: a.ctypes.data_as(i32)  # noqa: E731
        twice, high, crossed = order.copy(), le.copy(), lt.copy()
        twice[1, 5] = twice[1, 6]
        high[0, 1, 7] = U.N_INJ + 1
        crossed[1, 2, 3] = le[1, 2, 3] + 1
        for args, word in (((2, ptr(twice), ptr(lt), ptr(le)), "order_inj column 1: rank 6 holds .* not a permutation"),
                           ((2, ptr(order), ptr(lt), ptr(high)), "rank_le_pe column 0, sample 1507: 2501 is not in 0 ... n_inj = 2500"),
                           ((2, ptr(order), ptr(crossed), ptr(le)), "rank_lt_pe column 1, sample 3003: .* exceeds rank_le_pe"),
                           ((0, ptr(order), ptr(lt), ptr(le)), "n_cols = 0 is not in 1 ... 8"), ((9, ptr(order), ptr(lt), ptr(le)), "n_cols = 9"),
                           ((2, None, ptr(lt), ptr(le)), "is null"), ((2, ptr(order), None, ptr(le)), "is null"), ((2, ptr(order), ptr(lt), None), "is null")):
            assert lib.gwi_set_rank_columns(eng.handle, *args) == -1
            message = lib.gwi_last_error(eng.handle).decode()
            assert message.startswith("gwi_set_rank_columns: ") and re.search(word, message), (word, message)
            assert lib.gwi_point_pits_exact(eng.handle, *full) == -1 and "no rank columns are set" in lib.gwi_last_error(eng.handle).decode()
        assert lib.gwi_set_rank_columns(eng.handle, 2, ptr(order), ptr(lt), ptr(le)) == 0
        for args, word in (((None,) + full[1:], "thetas"), ((full[0], 0) + full[2:], "k < 1"), ((full[0], -1) + full[2:], "k < 1"),
                           (full[:2] + (None,) + full[3:], "pit is null"), (full[:3] + (None,), "dead is null")):
            assert lib.gwi_point_pits_exact(eng.handle, *args) == -1
            assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
        assert np.all(pit == 7.0) and np.all(dead == 7)
        assert lib.gwi_point_pits_exact(eng.handle, *full) == 0
        assert _same(pit, free[0][:1]) and np.array_equal(dead, free[1][:1])  # a second handle; the refused calls left nothing behind
    finally:
        eng.close()


def test_event_calibration_exact_device_against_host():
    """postprocess.event_calibration_exact on both backends, with leave_one_out="psis" and with leave_one_out=True: the raw arrays agree
    within the derived bound of the first test, the flags exactly; the weights are the same numbers on both sides (the same engine
    evaluates them), so a weighted mean of non-negative pits moves by at most the weighted mean of their bounds plus the rounding of the
    mean itself ((K + 2) 2^-52 relative); the P-P curves are those means sorted and the Kolmogorov distance moves by at most the
    largest of them.  K = 25 points, seeded convex mixtures of the three (every parameter stays between values at which the model is
    live): 5 tail points are smoothed, pareto_k is finite for every event, and the smoothed run differs from the unsmoothed one through the
    weights alone: the raw arrays are the same bits.  The bound of a pit is rank_util.device_tolerance with every sample live (no mask is
    set), relative to the host's value."""
    from gwinferno_amd import postprocess as P

    c = _case()
    eng = c["eng"]
    k = 25
    thetas = np.random.default_rng(12).dirichlet(np.ones(U.N_POINTS), k) @ c["thetas"]
    _, _, total = U.catalog()
    pe_values, inj_values = RU.values()
    kw = dict(inj_values=inj_values, total_inj=total, param_names=list(U.COLUMNS))
    dev = P.event_calibration_exact(eng, thetas, pe_values, leave_one_out="psis", **kw)
    host = P.event_calibration_exact(eng, thetas, pe_values, leave_one_out="psis", backend="host", **kw)
    plain = P.event_calibration_exact(eng, thetas, pe_values, leave_one_out=True, **kw)
    assert dev["names"] == list(U.COLUMNS) and np.array_equal(dev["dead"], host["dead"]) and not dev["n_dead"].any() and not host["n_dead"].any()
    for key in ("neff_points", "elpd_loo", "pareto_k"):
        assert np.array_equal(dev[key], host[key]), key
    assert not P.leave_one_out_weights(eng, thetas, total)["n_bad"].any()  # (the inputs: every l_ke is finite)
    assert dev["pareto_k"].shape == (U.N_EV,) and np.all(np.isfinite(dev["pareto_k"])) and "pareto_k" not in plain
    assert _same(dev["point_pits"], plain["point_pits"]) and np.array_equal(dev["dead"], plain["dead"])
    tol = RU.device_tolerance(U.N_PE) * host["point_pits"]  # (K, n_ev, C, 2)
    assert np.all(np.abs(dev["point_pits"] - host["point_pits"]) <= tol)
    v_psis = P.pareto_smoothed_loo_weights(eng, thetas, total)["point_weights"][:, : U.N_EV]
    v_raw = P.leave_one_out_weights(eng, thetas, total)["point_weights"][:, : U.N_EV]
    assert not np.array_equal(v_psis, v_raw)
    round_tol = (k + 2) * RU.U
    for run, v in ((dev, v_psis), (plain, v_raw)):  # the run's means are those of its own weights on the shared raw arrays
        want = (v[:, :, None, None] * run["point_pits"]).sum(axis=0) / v.sum(axis=0)[:, None, None]
        assert np.all(np.abs(run["pit_lt"] - want[..., 0]) <= round_tol * want[..., 0]) and np.all(np.abs(run["pit_le"] - want[..., 1]) <= round_tol * want[..., 1])
    mean_tol = (v_psis[:, :, None, None] * tol).sum(axis=0) / v_psis.sum(axis=0)[:, None, None]
    for i, key in enumerate(("pit_lt", "pit_le")):
        bound = mean_tol[..., i] * (1.0 + round_tol) + round_tol * host[key]
        assert np.all(np.abs(dev[key] - host[key]) <= bound), key
        pp = "pp_" + key[4:]
        assert np.all(np.abs(dev[pp] - host[pp]) <= bound.max(axis=0)[:, None]) and np.all(np.diff(dev[pp], axis=1) >= 0.0), pp
        ks = "ks_" + key[4:]
        assert np.all(np.abs(dev[ks] - host[ks]) <= bound.max(axis=0) + 2 * RU.U), ks
    assert np.all(dev["pit_lt"] <= dev["pit"]) and np.all(dev["pit"] <= dev["pit_le"]) and np.all(np.diff(dev["pp"], axis=1) >= 0.0)
