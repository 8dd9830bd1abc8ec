"""GPU: per-event calibration on the device (include/gwi_engine.h: gwi_point_pits; gwinferno_amd/csrc/gwi_pit.h): bit equality
with the NumPy loop (gwinferno_amd/draws.py: pit_bracket) fed with the device's own single-point histograms and detected CDF, the full
statement (point_pits_reference on the engine's own log-weights) under the derived bound of tests/pit_util.py, liveness and masks,
determinism over calls, splits, handles and the staging chunk, the absence of side effects, the refusals, and
postprocess.event_calibration on both backends.

Shapes (tests/cdf_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 500 injections (three tiles, the last ragged),
two columns, 1, 5 and 256 grid points, three points of a PL+Peak model.  The inputs are vetted without a device in
tests/test_cdf_cpu.py: test_inputs_of_the_gpu_tests and the brackets in tests/test_pit_cpu.py."""
import ctypes as C

import numpy as np
import pit_util as PU
import pytest

U = PU.CU

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
@pytest.mark.parametrize("n_grid", PU.N_GRID)
def test_bit_equality_with_the_numpy_loop(n_grid, case):
    """For every point alone: cdf_det is point_cdfs slot 0 to the bit, and draws.pit_bracket fed with the event's bins as
    gwi_weighted_histograms returns them for that point and with that slot has exactly the bits of point_pits.  No tolerance: this pins
    the quotient, the outside share, the order of the walk and the absence of a fused multiply-add."""
    from gwinferno_amd.draws import pit_bracket

    c = _case()
    eng = c["eng"]
    try:
        _set(eng, n_grid, case)
        pit, det, dead = eng.point_pits(c["thetas"])
        assert pit.shape == (U.N_POINTS, U.N_EV, 2, 2) and det.shape == (U.N_POINTS, 2, n_grid) and dead.shape == (U.N_POINTS, U.N_EV + 1) and dead.dtype == np.int32
        cdfs, _ = eng.point_cdfs(c["thetas"])
        assert np.array_equal(det, cdfs[:, 0]) and not np.any(np.isnan(det))
        for k, theta in enumerate(c["thetas"]):
            hp, _, h_dead = eng.weighted_histograms(theta)
            assert np.array_equal(dead[k], h_dead) and np.array_equal(np.nonzero(h_dead)[0], [U.DEAD_EVENT] if case == "masked" else [])
            for e in range(U.N_EV):
                if h_dead[e]:
                    assert np.all(np.isnan(pit[k, e]))
                    continue
                for col in range(2):
                    assert tuple(pit[k, e, col]) == pit_bracket(hp[e, col], det[k, col]), (k, e, col)
        live = pit[:, [e for e in range(U.N_EV) if case == "free" or e != U.DEAD_EVENT]]
        assert np.all(live[..., 0] <= live[..., 1]) and np.all(live >= 0.0) and np.all(live <= 1.0 + 1e-12) and np.any(live[..., 0] < live[..., 1])
    finally:
        eng.set_draw_mask()


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("n_grid", PU.N_GRID)
def test_against_the_full_statement(n_grid, case):
    """Every bracket end of every point against point_pits_reference on eng.log_weights under the DERIVED bound of
    pit_util.device_tolerance (hist_util.bound(n_live_e) for q, cdf_util.f_rel_bound(n_live_inj, G) for D, (G + 2) 2^-52 for the walk,
    and the absolute bound of the outside share).  The flags agree exactly.  The largest deviation is printed in units of the bound."""
    c = _case()
    eng = c["eng"]
    pm, im = U.masks(case)
    pc, ic = U.codes(n_grid)
    try:
        _set(eng, n_grid, case)
        pit, det, dead = eng.point_pits(c["thetas"])
    finally:
        eng.set_draw_mask()
    worst = 0.0
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_det, want_dead, tol = PU.statement_point(lw_pe, lw_inj, pm, im, pc, ic, n_grid)
        assert np.array_equal(dead[k], want_dead) and np.array_equal(np.isnan(pit[k]), np.isnan(want))
        assert np.all(np.abs(det[k] - want_det) <= U.f_rel_bound(U.HU.n_live(lw_inj, im), n_grid) * want_det)
        ok = ~np.isnan(want)
        assert np.all(np.isfinite(tol[ok])) and tol[ok].max() < 1e-11  # (nothing is left out, and the bound is a rounding bound)
        dev = np.abs(pit[k][ok] - want[ok])
        assert np.all(dev <= tol[ok]), (k, float(np.max(dev / tol[ok])))
        worst = max(worst, float(np.max(dev / tol[ok])))
    print(f"G = {n_grid} {case}: largest |device - statement| of a bracket end = {worst:.3f} of the derived bound")


def test_liveness_and_refusals():
    """The dead event gives NaN and its flag, the others keep their bits; an injection mask that removes everything gives all NaN (cdf_det
    included) and the injection flag; before set_histogram_bins, and while either set has no bins, the call answers GWI_ERR_INVALID with
    a message; null pointers and k < 1 likewise, and nothing is written; cdf_det may be NULL; an engine that holds a shard is refused
    with UNSUPPORTED at the Python guard (test_gpu_point_cdfs.py builds no world > 1 engine either)."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    c = _case()
    shared, thetas, n_grid = c["eng"], c["thetas"], 5
    try:
        _set(shared, n_grid)
        free = shared.point_pits(thetas)
        _set(shared, n_grid, "masked")
        masked = shared.point_pits(thetas)
        _set(shared, n_grid, "no_inj")
        none = shared.point_pits(thetas)
    finally:
        shared.set_draw_mask()
    keep = [e for e in range(U.N_EV) if e != U.DEAD_EVENT]
    assert not free[2].any() and not np.any(np.isnan(free[0])) and not np.any(np.isnan(free[1]))
    assert np.array_equal(masked[2], [[1 if e == U.DEAD_EVENT else 0 for e in range(U.N_EV)] + [0]] * U.N_POINTS)
    assert np.all(np.isnan(masked[0][:, U.DEAD_EVENT])) and not np.any(np.isnan(masked[0][:, keep])) and not np.any(np.isnan(masked[1]))
    assert not np.array_equal(masked[0][:, -1], free[0][:, -1])  # (the last event keeps its own weights, but the injection mask changed D)
    assert np.array_equal(none[2], [[1 if e == U.DEAD_EVENT else 0 for e in range(U.N_EV)] + [1]] * U.N_POINTS)
    assert np.all(np.isnan(none[0])) and np.all(np.isnan(none[1]))
    eng = U.composition().engine()
    try:
        theta = thetas[0]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):
            eng.point_pits(theta)
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th, pit, det, dead = N.f64(theta), np.full((1, U.N_EV, 2, 2), 7.0), np.full((1, 2, n_grid), 7.0), np.full((1, U.N_EV + 1), 7, dtype=np.int32)
        full = (N.as_dp(th), 1, N.as_dp(pit), N.as_dp(det), dead.ctypes.data_as(i32))
        assert lib.gwi_point_pits(eng.handle, *full) == -1
        assert "gwi_point_pits: no bins are set" in lib.gwi_last_error(eng.handle).decode()
        pc, ic = U.codes(n_grid)
        for sets, word in (((pc, None), "no injection bins are set"), ((None, ic), "no PE bins are set")):
            eng.set_histogram_bins(*sets, n_bins=n_grid)
            assert lib.gwi_point_pits(eng.handle, *full) == -1
            assert "gwi_point_pits: " + word in lib.gwi_last_error(eng.handle).decode()
            with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*" + word):
                eng.point_pits(theta)
        eng.set_histogram_bins(pc, ic, n_bins=n_grid)
        for args, word in (((None,) + full[1:], "thetas"), ((full[0], 0) + full[2:], "k < 1"), ((full[0], -1) + full[2:], "k < 1"),
                           (full[:2] + (None,) + full[3:], "pit is null"), (full[:4] + (None,), "dead is null")):
            assert lib.gwi_point_pits(eng.handle, *args) == -1
            assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
        assert np.all(pit == 7.0) and np.all(det == 7.0) and np.all(dead == 7)
        assert lib.gwi_point_pits(eng.handle, *(full[:3] + (None,) + full[4:])) == 0  # cdf_det is optional
        assert _same(pit, free[0][:1]) and np.all(det == 7.0) and np.array_equal(dead, free[2][:1])
        both = eng.point_pits(theta)
        assert all(_same(a, b[:1]) for a, b in zip(both, free))  # a second handle; the refused calls left nothing behind
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_pits"):
        shard.point_pits(np.zeros(3))


def test_bits_are_a_function_of_the_arguments():
    """K = 3 in one call, as 2 + 1 and as 1 + 1 + 1 concatenate to the same bits; the same call twice; a second handle on the same
    catalog; a call of K = 70 crosses the 64-point staging chunk: row k is that of the point it repeats; the diagnostic reports five
    launches per point."""
    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 256
    _set(eng, n_grid)
    whole = eng.point_pits(thetas)
    again = eng.point_pits(thetas)
    assert all(_same(a, b) for a, b in zip(whole, again))
    assert not np.array_equal(whole[0][0], whole[0][1])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_pit_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 15 and all(m.value > 0.0 for m in ms)
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        parts, at = [], 0
        for n in split:
            parts.append(eng.point_pits(thetas[at : at + n]))
            at += n
        assert all(_same(np.concatenate([p[i] for p in parts]), whole[i]) for i in range(3)), split
    single = eng.point_pits(thetas[1])  # one point given as (n_theta,)
    assert single[0].shape == (1, U.N_EV, 2, 2) and _same(single[0][0], whole[0][1])
    many = np.tile(thetas, (24, 1))[:70]
    out = eng.point_pits(many)
    assert out[0].shape == (70, U.N_EV, 2, 2) and out[1].shape == (70, 2, n_grid) and out[2].shape == (70, U.N_EV + 1)
    for k in range(70):
        assert all(_same(out[i][k], whole[i][k % 3]) for i in range(3)), k
    eng2 = U.composition().engine()
    try:
        pc, ic = U.codes(n_grid)
        eng2.set_histogram_bins(pc, ic, n_bins=n_grid)
        other = eng2.point_pits(thetas)
        assert all(_same(a, b) for a, b in zip(other, whole))
    finally:
        eng2.close()


def test_no_side_effects():
    """A weighted_histograms accumulation split over two calls with a point_pits call in between, a marginal_weights_add /
    weighted_quantiles sequence with point_pits calls in between, and point_cdfs before and after point_pits each return the bits they
    return without it; point_pits itself repeats after all of them."""
    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 5
    _set(eng, n_grid)
    pe_values, inj_values = U.values()
    x_pe, x_inj = np.stack([pe_values[k] for k in U.COLUMNS]), np.stack([inj_values[k] for k in U.COLUMNS])
    eng.set_quantile_columns(x_pe, x_inj)

    def histograms(interleave):
        out = eng.weighted_histograms(thetas[:2])
        if interleave:
            eng.point_pits(thetas)
        return eng.weighted_histograms(thetas[2:], out=out)

    def quantiles(interleave):
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas[:2])
        if interleave:
            eng.point_pits(thetas)
        eng.marginal_weights_add(thetas[2:])
        if interleave:
            eng.point_pits(thetas[1])
        return eng.weighted_quantiles(np.array([0.05, 0.5, 0.95])), eng.marginal_weights()

    plain_h, plain_q, cdfs = histograms(False), quantiles(False), eng.point_cdfs(thetas)
    pits = eng.point_pits(thetas)
    mixed_h, mixed_q, cdfs_after = histograms(True), quantiles(True), eng.point_cdfs(thetas)
    assert all(np.array_equal(a, b) for a, b in zip(plain_h, mixed_h)) and np.array_equal(plain_h[0], eng.weighted_histograms(thetas)[0])
    for a, b in zip(tuple(plain_q[0]) + tuple(plain_q[1][:3]), tuple(mixed_q[0]) + tuple(mixed_q[1][:3])):
        assert np.array_equal(a, b)
    assert plain_q[1][3] == mixed_q[1][3] == 3
    assert _same(cdfs[0], cdfs_after[0]) and np.array_equal(cdfs[1], cdfs_after[1])
    assert all(_same(a, b) for a, b in zip(eng.point_pits(thetas), pits))


def test_event_calibration_device_against_host():
    """postprocess.event_calibration on both backends with leave_one_out=True: the raw arrays agree within the derived bound of the
    second test, the flags exactly; the leave-one-out weights are the same numbers on both sides (the same engine evaluates them), so a
    weighted mean of non-negative brackets moves by at most the weighted mean of their bounds, plus the rounding of the mean itself
    ((K + 2) 2^-52 relative: K products, K - 1 additions and a division on either side); the P-P curves are those means sorted and the
    Kolmogorov distance moves by at most the largest of them."""
    from gwinferno_amd import postprocess as P

    c = _case()
    eng, thetas, n_grid = c["eng"], c["thetas"], 5
    _, _, total = U.catalog()
    pe_values, inj_values = U.values()
    kw = dict(inj_values=inj_values, leave_one_out=True, total_inj=total, param_names=list(U.COLUMNS))
    dev = P.event_calibration(eng, thetas, pe_values, U.grid(n_grid), **kw)
    host = P.event_calibration(eng, thetas, pe_values, U.grid(n_grid), backend="host", **kw)
    assert dev["names"] == list(U.COLUMNS) and np.array_equal(dev["dead"], host["dead"]) and not dev["n_dead"].any() and not host["n_dead"].any()
    assert np.array_equal(dev["neff_points"], host["neff_points"]) and np.array_equal(dev["elpd_loo"], host["elpd_loo"]) and np.all(dev["neff_points"] <= U.N_POINTS)
    pc, ic = U.codes(n_grid)
    tol = np.stack([PU.statement_point(lw_pe, lw_inj, None, None, pc, ic, n_grid)[3] for lw_pe, lw_inj in c["lw"]])  # (K, n_ev, C, 2)
    assert np.all(np.abs(dev["point_pits"] - host["point_pits"]) <= tol)
    v = P.leave_one_out_weights(eng, thetas, total)["point_weights"][:, : U.N_EV]
    mean_tol = (v[:, :, None, None] * tol).sum(axis=0) / v.sum(axis=0)[:, None, None]
    round_tol = (U.N_POINTS + 2) * PU.U
    for i, key in enumerate(("pit_lo", "pit_hi")):
        bound = mean_tol[..., i] * (1.0 + round_tol) + round_tol * host[key]
        assert np.all(np.abs(dev[key] - host[key]) <= bound), key
        pp = "pp_" + key[4:]
        assert np.all(np.abs(dev[pp] - host[pp]) <= bound.max(axis=0)[:, None]) and np.all(np.diff(dev[pp], axis=1) >= 0.0), pp
        ks = "ks_" + key[4:]
        assert np.all(np.abs(dev[ks] - host[ks]) <= bound.max(axis=0) + 2 * PU.U), ks
    assert np.all(dev["pit_lo"] <= dev["pit"]) and np.all(dev["pit"] <= dev["pit_hi"]) and np.array_equal(dev["width"], dev["pit_hi"] - dev["pit_lo"])
