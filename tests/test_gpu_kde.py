"""GPU: weighted kernel density estimates of the marginal weights on the device (include/gwi_engine.h: gwi_set_kde_columns,
gwi_weighted_kde, gwi_weighted_kde2d; gwinferno_amd/csrc/gwi_kde.h) against their NumPy statement (gwinferno_amd/draws.py:
weighted_kde_reference, weighted_kde2d_reference) under derived bounds (tests/kde_util.py), their bits across calls, handles, splits
of the grid and of the points, masked, dead and degenerate segments, reflection, their agreement with the weighted quantiles' moments,
the user-facing function, the refusals and the lifetime of the handle's buffers.

Shapes (tests/hist_util.py, tests/quant_util.py, tests/kde_util.py): 3 events x 1 500 PE samples (two sample chunks, the second
ragged), 2 600 injections (three chunks), 1 and 8 columns, 5 and 300 grid points, one pair at 7 x 5 and two at 33 x 20, K = 3 points, a
PL+Peak and a B-spline model.  The inputs are vetted without a device in tests/test_kde_cpu.py: test_inputs_of_the_gpu_tests."""
import ctypes as C
import gc
import os

import hist_util as U
import kde_util as KU
import numpy as np
import pytest
import quant_util as QU

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """One engine per composition with its three points: made once, shared, never changed."""
    if name not in _CASES:
        comp = U.composition(name)
        thetas = U.points(comp, name, KU.K)
        thetas.setflags(write=False)
        _CASES[name] = dict(comp=comp, eng=comp.engine(), thetas=thetas)
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


def _same(a, b):
    """Equal bits, entry by entry (NaN equal to NaN)."""
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def _one_sample_mask():
    """hist_util's "masked" case with the last event masked down to one sample."""
    pm, im = U.masks("masked")
    pm = pm.copy()
    pm[2] = 0
    pm[2, 777] = 1
    return pm, im


@pytest.mark.parametrize("n_grid", KU.N_GRID)
@pytest.mark.parametrize("n_cols", (1, 8))
@pytest.mark.parametrize("name", U.COMPS)
def test_curves_against_statement(name, n_cols, n_grid):
    """Every (segment, column, grid point) of the 1-D estimate against weighted_kde_reference on the W read back from the same
    handle, with and without masks, Scott and a scaled Silverman: under kde_util.bound_1d (DERIVED); h and n_eff to 1e-12 relative."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp, vi = QU.columns(n_cols)
    grid = KU.grid(n_cols, n_grid)
    eng.set_kde_columns(vp, vi)
    worst = 0.0
    for case in U.MASK_CASES:
        W_pe, W_inj, dead, _ = _accumulate(eng, thetas, U.masks(case))
        for rule, scale in (("scott", 1.0), ("silverman", 0.7)):
            rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid, rule, scale)
            assert rho_pe.shape == (U.N_EV, n_cols, n_grid) and rho_inj.shape == (n_cols, n_grid) and bw.shape == flags.shape == (U.N_EV + 1, n_cols) and flags.dtype == np.int32
            for seg in range(U.N_EV + 1):
                W = W_pe[seg] if seg < U.N_EV else W_inj
                for col in range(n_cols):
                    x, got = (vp[col, seg], rho_pe[seg, col]) if seg < U.N_EV else (vi[col], rho_inj[col])
                    worst = max(worst, KU.check_1d(W, x, grid[col], rule, scale, None, got, bw[seg, col], neff[seg], flags[seg, col], (name, case, rule, seg, col)))
                if dead[seg]:
                    assert seg == U.DEAD_EVENT and case == "masked" and neff[seg] == 0.0 and not flags[seg].any()
    print(f"{name} C = {n_cols} G = {n_grid}: the worst |device - statement| is {worst:.3f} of the derived bound")


@pytest.mark.parametrize("pairs,shape", ((KU.PAIRS_1, KU.SHAPE_1), (KU.PAIRS_2, KU.SHAPE_2)), ids=("1 pair 7x5", "2 pairs 33x20"))
@pytest.mark.parametrize("name", U.COMPS)
def test_maps_against_statement(name, pairs, shape):
    """Every (segment, pair, grid point) of the 2-D estimate against weighted_kde2d_reference on the W read back, with and without
    masks: under kde_util.bound_2d (DERIVED); H and n_eff to 1e-12 relative."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp, vi = QU.columns(8)
    gx, gy = KU.grid2d(pairs, shape)
    eng.set_kde_columns(vp, vi)
    worst = 0.0
    for case in U.MASK_CASES:
        W_pe, W_inj, dead, _ = _accumulate(eng, thetas, U.masks(case))
        rule, scale = ("scott", 1.0) if case == "free" else ("silverman", 1.3)
        rho_pe, rho_inj, cov, neff, flags = eng.weighted_kde2d(pairs, gx, gy, rule, scale)
        assert rho_pe.shape == (U.N_EV, len(pairs)) + shape and rho_inj.shape == (len(pairs),) + shape and cov.shape == (U.N_EV + 1, len(pairs), 3)
        for seg in range(U.N_EV + 1):
            W = W_pe[seg] if seg < U.N_EV else W_inj
            for t, (cx, cy) in enumerate(pairs):
                x, y, got = (vp[cx, seg], vp[cy, seg], rho_pe[seg, t]) if seg < U.N_EV else (vi[cx], vi[cy], rho_inj[t])
                worst = max(worst, KU.check_2d(W, x, y, gx[t], gy[t], rule, scale, got, cov[seg, t], neff[seg], flags[seg, t], (name, case, seg, t)))
    print(f"{name} {len(pairs)} pair(s) at {shape}: the worst |device - statement| is {worst:.3f} of the derived bound")


@pytest.mark.parametrize("name", U.COMPS)
def test_same_bits(name):
    """Two calls; two handles; a grid split 2 + 3 and 150 + 150 (1-D) and a map split along either axis against one call, point by
    point; W accumulated as 3, 2 + 1 and 1 + 1 + 1 points."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp, vi = QU.columns(8)
    gx, gy = KU.grid2d(KU.PAIRS_2, KU.SHAPE_2)
    eng.set_kde_columns(vp, vi)
    _accumulate(eng, thetas)
    whole = {g: eng.weighted_kde(KU.grid(8, g)) for g in KU.N_GRID}
    whole2 = eng.weighted_kde2d(KU.PAIRS_2, gx, gy)
    for g, cut in ((5, 2), (300, 150)):
        grid = KU.grid(8, g)
        assert _same(whole[g], eng.weighted_kde(grid))
        a, b = eng.weighted_kde(grid[:, :cut]), eng.weighted_kde(grid[:, cut:])
        assert _same(whole[g], (np.concatenate([a[0], b[0]], axis=-1), np.concatenate([a[1], b[1]], axis=-1), a[2], a[3], a[4])) and _same(a[2:], b[2:])
    assert _same(whole2, eng.weighted_kde2d(KU.PAIRS_2, gx, gy))
    a, b = eng.weighted_kde2d(KU.PAIRS_2, gx[:, :13], gy), eng.weighted_kde2d(KU.PAIRS_2, gx[:, 13:], gy)
    assert _same(whole2[:2], (np.concatenate([a[0], b[0]], axis=2), np.concatenate([a[1], b[1]], axis=1))) and _same(whole2[2:], a[2:])
    a, b = eng.weighted_kde2d(KU.PAIRS_2, gx, gy[:, :7]), eng.weighted_kde2d(KU.PAIRS_2, gx, gy[:, 7:])
    assert _same(whole2[:2], (np.concatenate([a[0], b[0]], axis=3), np.concatenate([a[1], b[1]], axis=2)))
    for split in ((2, 1), (1, 1, 1)):
        eng.marginal_weights_reset()
        at = 0
        for m in split:
            eng.marginal_weights_add(thetas[at : at + m])
            at += m
        assert _same(whole[300], eng.weighted_kde(KU.grid(8, 300))) and _same(whole2, eng.weighted_kde2d(KU.PAIRS_2, gx, gy)), split
    other = U.composition(name).engine()
    try:
        other.set_kde_columns(vp, vi)
        _accumulate(other, thetas)
        assert _same(whole[300], other.weighted_kde(KU.grid(8, 300))) and _same(whole2, other.weighted_kde2d(KU.PAIRS_2, gx, gy))
    finally:
        other.close()


def test_masked_dead_and_degenerate_segments():
    """hist_util's dead event (the mask; and, with PL+Peak, the point whose weights underflow for the heaviest event) and an event
    masked down to one sample: NaN, dead and degenerate as in the statement; the other segments are unchanged to the bit."""
    c = _case("plpeak")
    eng, comp, thetas = c["eng"], c["comp"], c["thetas"]
    vp, vi = QU.columns(8)
    grid = KU.grid(8, 300)
    gx, gy = KU.grid2d(KU.PAIRS_2, KU.SHAPE_2)
    eng.set_kde_columns(vp, vi)
    _accumulate(eng, thetas, U.masks("masked"))
    ref, ref2 = eng.weighted_kde(grid), eng.weighted_kde2d(KU.PAIRS_2, gx, gy)
    W_pe, W_inj, dead, _ = _accumulate(eng, thetas, _one_sample_mask())
    rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid)
    rho2_pe, rho2_inj, cov, neff2, flags2 = eng.weighted_kde2d(KU.PAIRS_2, gx, gy)
    assert np.count_nonzero(W_pe[2]) == 1 and dead[U.DEAD_EVENT] == KU.K and dead[2] == 0
    assert np.all(np.isnan(rho_pe[U.DEAD_EVENT])) and np.all(np.isnan(bw[U.DEAD_EVENT])) and neff[U.DEAD_EVENT] == 0.0 and not flags[U.DEAD_EVENT].any() and not flags2[U.DEAD_EVENT].any()
    assert np.all(np.isnan(rho_pe[2])) and np.all(np.isnan(bw[2])) and neff[2] == 1.0 and np.all(flags[2] == 1)
    assert np.all(np.isnan(rho2_pe[2])) and np.all(np.isnan(cov[2])) and np.all(flags2[2] == 1) and np.all(np.isnan(rho2_pe[U.DEAD_EVENT]))
    for seg in (0, U.N_EV):  # the segments the change of the mask does not touch
        assert np.array_equal(rho_pe[0], ref[0][0]) and np.array_equal(rho_inj, ref[1]) and np.array_equal(bw[seg], ref[2][seg]) and neff[seg] == ref[3][seg] and not flags[seg].any()
        assert np.array_equal(rho2_pe[0], ref2[0][0]) and np.array_equal(rho2_inj, ref2[1]) and np.array_equal(cov[seg], ref2[2][seg]) and not flags2[seg].any()
    for seg in range(U.N_EV + 1):  # ... and all of it as the statement has it
        W = W_pe[seg] if seg < U.N_EV else W_inj
        x, got = (vp[3, seg], rho_pe[seg, 3]) if seg < U.N_EV else (vi[3], rho_inj[3])
        KU.check_1d(W, x, grid[3], "scott", 1.0, None, got, bw[seg, 3], neff[seg], flags[seg, 3], ("one sample", seg))
    # a point at which the heaviest event's weights underflow: dead by the model, not by a mask
    theta = comp.theta(U.dead_event_params())
    W_pe, W_inj, dead, _ = _accumulate(eng, theta)
    rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid)
    assert dead.any() and not dead.all()
    for seg in range(U.N_EV):
        assert bool(dead[seg]) == (neff[seg] == 0.0) and (not dead[seg] or (np.all(np.isnan(rho_pe[seg])) and not flags[seg].any()))
        for col in (0, 4):
            KU.check_1d(W_pe[seg], vp[col, seg], grid[col], "scott", 1.0, None, rho_pe[seg, col], bw[seg, col], neff[seg], flags[seg, col], ("steep", seg, col))


@pytest.mark.parametrize("name", U.COMPS)
def test_reflection(name):
    """mass_ratio reflected at [0, 1], at one bound only and not at all, beside an unreflected column: against the statement,
    including grid points exactly on a bound and outside; the bandwidth is the unreflected one."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    vp8, vi8 = QU.columns(8)
    vp, vi = np.ascontiguousarray(vp8[[0, KU.Q_COLUMN]]), np.ascontiguousarray(vi8[[0, KU.Q_COLUMN]])
    rg = KU.reflection_grid()
    grid = np.stack([np.linspace(vp[0].min(), vp[0].max(), rg.size), rg])
    W_pe, W_inj, _, _ = _accumulate(eng, thetas)
    eng.set_kde_columns(vp, vi)
    plain = eng.weighted_kde(grid)
    worst = 0.0
    for bounds in (KU.Q_BOUNDS, (None, 1.0), (0.0, None)):
        eng.set_kde_columns(vp, vi, bounds=[(None, None), bounds])
        rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid)
        assert np.array_equal(bw, plain[2]) and np.array_equal(neff, plain[3]) and not flags.any()
        assert np.array_equal(rho_pe[:, 0], plain[0][:, 0]) and np.array_equal(rho_inj[0], plain[1][0])  # the column without bounds
        for seg in range(U.N_EV + 1):
            W, x, got = (W_pe[seg], vp[1, seg], rho_pe[seg, 1]) if seg < U.N_EV else (W_inj, vi[1], rho_inj[1])
            worst = max(worst, KU.check_1d(W, x, rg, "scott", 1.0, bounds, got, bw[seg, 1], neff[seg], flags[seg, 1], (name, bounds, seg)))
            lo, hi = (-np.inf if bounds[0] is None else bounds[0]), (np.inf if bounds[1] is None else bounds[1])
            inside, unreflected = (rg >= lo) & (rg <= hi), plain[0][seg, 1] if seg < U.N_EV else plain[1][1]
            assert not got[~inside].any() and np.all(got[inside] >= unreflected[inside])
    print(f"{name}: reflection: the worst |device - statement| is {worst:.3f} of the derived bound")


def test_consistency_with_the_quantile_moments():
    """On a wide uniform grid the trapezoid mean of the 1-D curve agrees with weighted_quantiles' mean, and the 2-D map summed over
    gy (trapezoid) with the 1-D curve of Hxx's bandwidth.  The bound: the grid reaches 8 h beyond the samples on either side, where
    a Gaussian's tail mass is below 1e-15, and the trapezoid rule on a sum of Gaussians of width h at spacing d errs by a relative
    2 exp(-2 pi^2 h^2 / d^2) (the first alias of the Gaussian's Fourier transform); the grids are made with d <= h / 1.5, where that
    is 2e-19 -- so the quadrature is exact to rounding, and 1e-9 (the project's parity bar) is asked for, of the range of the grid for
    the mean and of the curve's peak for the marginal."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    vp8, vi8 = QU.columns(8)
    cols = [0, KU.Q_COLUMN]
    vp, vi = np.ascontiguousarray(vp8[cols]), np.ascontiguousarray(vi8[cols])
    _accumulate(eng, thetas)
    eng.set_quantile_columns(vp, vi)
    _, _, mom_pe, mom_inj, mass = eng.weighted_quantiles([0.5])
    eng.set_kde_columns(vp, vi)
    g0 = np.stack([np.linspace(vp[k].min(), vp[k].max(), 5) for k in range(2)])
    bw = eng.weighted_kde(g0)[2]
    seg, lo, hi = U.N_EV, vi.min(axis=1), vi.max(axis=1)  # the injection set: the widest segment
    h = bw[seg]
    assert np.all((hi - lo + 16 * h) / 1023 <= h / 1.5)
    grid = np.stack([np.linspace(lo[k] - 8 * h[k], hi[k] + 8 * h[k], 1024) for k in range(2)])
    rho_inj = eng.weighted_kde(grid)[1]
    for k in range(2):
        d = grid[k, 1] - grid[k, 0]
        total, mean = float(np.sum(rho_inj[k]) * d), float(np.sum(rho_inj[k] * grid[k]) * d)  # (the ends are below 1e-15 of the peak: trapezoid = plain sum)
        assert abs(total - 1.0) <= 1e-9 and abs(mean - mom_inj[k, 0] / mass[seg]) <= 1e-9 * (grid[k, -1] - grid[k, 0]), (k, total, mean)
    # the map of (mass_1, mass_ratio) summed over gy is the Gaussian sum in mass_1 of variance Hxx
    gy = np.linspace(lo[1] - 1.0, hi[1] + 1.0, 128)
    rho2_inj, cov = eng.weighted_kde2d([(0, 1)], np.linspace(lo[0], hi[0], 16), gy)[1:3]
    hx, hy = np.sqrt(cov[seg, 0, 0]), np.sqrt(cov[seg, 0, 2])
    assert gy[1] - gy[0] <= np.sqrt(cov[seg, 0, 2] - cov[seg, 0, 1] ** 2 / cov[seg, 0, 0]) / 1.5 and 1.0 >= 8 * hy  # (the conditional width sets the alias)
    marginal = np.sum(rho2_inj[0], axis=1) * (gy[1] - gy[0])
    eng.set_kde_columns(vp[:1], vi[:1])
    want = eng.weighted_kde(np.linspace(lo[0], hi[0], 16), scale=hx / bw[seg, 0])[1][0]
    assert np.all(np.abs(marginal - want) <= 1e-9 * want.max()), float(np.max(np.abs(marginal - want)) / want.max())


def test_event_posterior_densities():
    """backend="device" against backend="host" (the statement on the handle's W: under the derived bounds); accumulate=False after
    event_credible_intervals against a fresh accumulation: the same bits; names against arrays; the mass cuts become the mask."""
    from gwinferno_amd import postprocess as P

    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    pe, inj, _ = U.catalog()
    names = ["mass_1", "mass_ratio"]
    pe_values, inj_values = {k: pe[k] for k in names}, {k: inj[k] for k in names}
    grid = {"mass_1": np.linspace(3.0, 90.0, 64), "mass_ratio": np.linspace(-0.1, 1.1, 64)}
    kw = dict(pairs=[("mass_1", "mass_ratio")], grid2d=(np.linspace(5.0, 80.0, 12), np.linspace(0.1, 1.0, 9)), bounds={"mass_ratio": (0.0, 1.0)})
    dev = P.event_posterior_densities(eng, thetas, pe_values, grid, inj_values=inj_values, **kw)
    host = P.event_posterior_densities(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host", **kw)
    W_pe, W_inj, _, n_points = eng.marginal_weights()
    assert dev["names"] == names and dev["n_points"] == n_points == KU.K and not dev["dead"].any() and not dev["degenerate"].any() and not dev["degenerate2d"].any()
    assert np.allclose(dev["bandwidth"], host["bandwidth"], rtol=1e-12, atol=0) and np.allclose(dev["neff"], host["neff"], rtol=1e-12, atol=0)
    assert np.allclose(dev["covariance"], host["covariance"], rtol=1e-12, atol=0) and np.allclose(dev["covariance_inj"], host["covariance_inj"], rtol=1e-12, atol=0)
    for seg in range(U.N_EV + 1):
        W = W_pe[seg] if seg < U.N_EV else W_inj
        for k, p in enumerate(names):
            x, got, want, h = (pe[p][seg], dev["density"][seg, k], host["density"][seg, k], host["bandwidth"][seg, k]) if seg < U.N_EV else (
                inj[p], dev["density_inj"][k], host["density_inj"][k], host["bandwidth_inj"][k])
            KU.compare(got, want, KU.bound_1d(W, x, grid[p], h, kw["bounds"].get(p)), ("densities", seg, p))
        x, y, got, want, H = (pe[names[0]][seg], pe[names[1]][seg], dev["density2d"][seg, 0], host["density2d"][seg, 0], host["covariance"][seg, 0]) if seg < U.N_EV else (
            inj[names[0]], inj[names[1]], dev["density2d_inj"][0], host["density2d_inj"][0], host["covariance_inj"][0])
        KU.compare(got, want, KU.bound_2d(W, x, y, kw["grid2d"][0], kw["grid2d"][1], H), ("densities 2-D", seg))
    # the table, then the figure from the weights the table left
    P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values)
    reused = P.event_posterior_densities(eng, thetas, pe_values, grid, inj_values=inj_values, accumulate=False, **kw)
    named = P.event_posterior_densities(eng, thetas, None, grid, pedata=pe, injdata=inj, param_names=names, **kw)
    for key in ("density", "density_inj", "density2d", "density2d_inj", "bandwidth", "neff", "covariance", "dead"):
        assert np.array_equal(dev[key], reused[key]) and np.array_equal(dev[key], named[key]), key
    assert reused["n_points"] == named["n_points"] == KU.K
    try:
        cut = P.event_posterior_densities(eng, thetas, None, grid, pedata=pe, injdata=inj, param_names=names, m1min=6.0, m2min=5.0, mmax=70.0)
        assert not np.array_equal(cut["density"], dev["density"]) and np.all(np.isfinite(cut["density"]))
    finally:
        eng.set_draw_mask()


def test_refusals():
    """Every refusal of the C ABI that needs a device, with its message and without a launch; nothing accumulated is valid; the handle
    keeps working afterwards."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    comp = U.composition("plpeak")
    eng = comp.engine()
    try:
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        ip = lambda a: None if a is None else a.ctypes.data_as(i32)  # noqa: E731
        err = lambda: lib.gwi_last_error(eng.handle).decode()  # noqa: E731
        vp, vi = QU.columns(8)
        grid = np.ascontiguousarray(KU.grid(8, 5))
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no columns are set"):
            eng.weighted_kde(grid[0])
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no columns are set"):
            eng.weighted_kde2d([(0, 1)], grid[0], grid[1])
        cols = lambda n, xp, xi, b: lib.gwi_set_kde_columns(eng.handle, n, N.as_dp(xp), N.as_dp(xi), N.as_dp(b))  # noqa: E731
        assert cols(0, vp, vi, None) == -1 and "n_cols = 0 is not in 1 ... 8" in err()
        assert cols(9, vp, vi, None) == -1 and "n_cols = 9" in err()
        assert cols(8, None, None, None) == -1 and "both null" in err()
        bad = vi.copy()
        bad[2, 11] = np.inf
        assert cols(8, vp, bad, None) == -1 and f"x_inj: value {2 * U.N_INJ + 11} is not finite" in err()
        b = np.full((8, 2), np.nan)
        b[3] = [1.0, 1.0]
        assert cols(8, vp, vi, b) == -1 and "bounds of column 3: lo is not below hi" in err()
        b[3] = [-np.inf, 1.0]
        assert cols(8, vp, vi, b) == -1 and "bounds of column 3" in err()
        # nothing accumulated is valid: everything NaN, neff 0, nothing flagged
        eng.set_kde_columns(vp, vi)
        rho_pe, rho_inj, bw, neff, flags = eng.weighted_kde(grid)
        rho2_pe, rho2_inj, cov, neff2, flags2 = eng.weighted_kde2d(KU.PAIRS_1, *KU.grid2d(KU.PAIRS_1, KU.SHAPE_1))
        assert np.all(np.isnan(rho_pe)) and np.all(np.isnan(rho_inj)) and np.all(np.isnan(bw)) and not neff.any() and not flags.any()
        assert np.all(np.isnan(rho2_pe)) and np.all(np.isnan(rho2_inj)) and np.all(np.isnan(cov)) and not neff2.any() and not flags2.any()
        r_pe, r_inj, o_bw, o_neff, o_flag = np.zeros((U.N_EV, 8, 5)), np.zeros((8, 5)), np.zeros((U.N_EV + 1, 8, 3)), np.zeros(U.N_EV + 1), np.zeros((U.N_EV + 1, 8), dtype=np.int32)
        kde = lambda g=grid, n=5, rule=0, scale=1.0, a=r_pe, b=r_inj, w=o_bw, e=o_neff, f=o_flag: lib.gwi_weighted_kde(  # noqa: E731
            eng.handle, N.as_dp(g), n, rule, scale, N.as_dp(a), N.as_dp(b), N.as_dp(w), N.as_dp(e), ip(f))
        assert kde() == 0
        assert kde(n=0) == -1 and "n_grid = 0 is not in 1 ... 1024" in err()
        assert kde(n=1025) == -1 and "n_grid = 1025" in err()
        assert kde(rule=2) == -1 and "rule = 2 is neither" in err()
        for scale in (0.0, -1.0, np.nan, np.inf):
            assert kde(scale=scale) == -1 and "is not a positive finite number" in err()
        assert kde(g=None) == -1 and "grid is null" in err()
        bad = grid.copy()
        bad[1, 2] = np.nan
        assert kde(g=bad) == -1 and "grid: point 7 is not finite" in err()
        assert kde(a=None) == -1 and "rho_pe is needed" in err()
        assert kde(b=None) == -1 and "rho_inj is needed" in err()
        assert kde(w=None) == -1 and kde(e=None) == -1 and kde(f=None) == -1 and "output is null" in err()
        pairs, gx, gy = np.array([[0, 4]], dtype=np.int32), np.ascontiguousarray(grid[:1]), np.ascontiguousarray(grid[4:5])
        m_pe, m_inj = np.zeros((U.N_EV, 1, 5, 5)), np.zeros((1, 5, 5))
        kde2 = lambda p=pairs, n_p=1, x=gx, nx=5, y=gy, ny=5, rule=0, scale=1.0: lib.gwi_weighted_kde2d(  # noqa: E731
            eng.handle, ip(p), n_p, N.as_dp(x), nx, N.as_dp(y), ny, rule, scale, N.as_dp(m_pe), N.as_dp(m_inj), N.as_dp(o_bw), N.as_dp(o_neff), ip(o_flag))
        assert kde2() == 0
        assert kde2(n_p=0) == -1 and "n_pairs = 0 is not in 1 ... 4" in err() and kde2(n_p=5) == -1 and "n_pairs = 5" in err()
        assert kde2(nx=0) == -1 and "not in 1 ... 128" in err() and kde2(ny=129) == -1 and "n_gy = 129" in err()
        assert kde2(rule=-1) == -1 and "rule = -1" in err() and kde2(scale=0.0) == -1 and "positive finite" in err()
        assert kde2(p=None) == -1 and "is null" in err() and kde2(x=None) == -1 and kde2(y=None) == -1
        for wrong in (8, -1):
            assert kde2(p=np.array([[0, wrong]], dtype=np.int32)) == -1 and f"pair 0 names column {wrong}: not in 0 ... 7" in err()
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*pair 0 names column 8"):
            eng.weighted_kde2d([(8, 0)], grid[0], grid[1])
        bad = gy.copy()
        bad[0, 4] = np.inf
        assert kde2(y=bad) == -1 and "gridy: point 4 is not finite" in err()
        # a handle that holds a shard: GWI_ERR_UNSUPPORTED from Python and from the library itself
        theta = comp.theta(U.params("plpeak"))
        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
            shards[0].weighted_kde(grid[0])
        seg = f"/gwi_kde_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            sp, si = np.zeros((1, shards[0].n_ev, shards[0].n_pe)), np.zeros((1, shards[0].n_inj))
            for st in (lib.gwi_set_kde_columns(hs, 1, N.as_dp(sp), N.as_dp(si), None),
                       lib.gwi_weighted_kde(hs, N.as_dp(grid), 5, 0, 1.0, N.as_dp(r_pe), N.as_dp(r_inj), N.as_dp(o_bw), N.as_dp(o_neff), ip(o_flag)),
                       lib.gwi_weighted_kde2d(hs, ip(pairs), 1, N.as_dp(gx), 5, N.as_dp(gy), 5, 0, 1.0, N.as_dp(m_pe), N.as_dp(m_inj), N.as_dp(o_bw), N.as_dp(o_neff), ip(o_flag))):
                assert st == -4 and "this handle holds one shard of the catalog" in lib.gwi_last_error(hs).decode()  # GWI_ERR_UNSUPPORTED
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        # usable after all of it, with the bits of the shared engine
        _accumulate(eng, theta)
        ref = _case("plpeak")["eng"]
        ref.set_kde_columns(vp, vi)
        _accumulate(ref, theta)
        assert _same(eng.weighted_kde(grid), ref.weighted_kde(grid))
        # one set alone: the other's outputs are left out
        eng.set_kde_columns(None, vi)
        only = eng.weighted_kde(grid)
        assert only[0] is None and np.array_equal(only[1], ref.weighted_kde(grid)[1]) and np.all(np.isnan(only[2][: U.N_EV])) and not only[3][: U.N_EV].any()
    finally:
        eng.close()


def test_lifetime():
    """create / set / add / densities / destroy over a few handles, the columns replaced on every other one and the handle closed
    with its buffers live: every handle gives the first one's bits and device memory returns to its starting level."""
    import torch

    from gwinferno_amd import likelihood

    likelihood.clear_engine_cache()
    gc.collect()
    vp, vi = QU.columns(8)
    grid = KU.grid(8, 300)
    gx, gy = KU.grid2d(KU.PAIRS_2, KU.SHAPE_2)
    free, first = [], None
    for it in range(6):
        comp = U.composition("plpeak")
        eng = comp.engine()
        try:
            thetas = U.points(comp, "plpeak", 2)
            eng.set_kde_columns(vp, vi)
            if it % 2:  # the columns replaced: the buffers are dropped and made anew
                eng.marginal_weights_add(thetas[:1])
                eng.set_kde_columns(vp[:2], None)
                eng.weighted_kde(grid[:2, :7])
                eng.set_kde_columns(vp, vi)
                eng.marginal_weights_reset()
            eng.marginal_weights_add(thetas)
            got = (*eng.weighted_kde(grid), *eng.weighted_kde2d(KU.PAIRS_2, gx, gy))
        finally:
            eng.close()
        del eng, comp
        gc.collect()
        first = got if first is None else first
        assert _same(first, got), it
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert abs(free[-1] - free[1]) <= 8 << 20, free  # (the runtime's own pools settle with the first handle)
