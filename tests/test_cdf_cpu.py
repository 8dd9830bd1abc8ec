"""CPU: per-point CDFs and the catalog predictive check (include/gwi_engine.h: gwi_point_cdfs; gwinferno_amd/csrc/gwi_cdf.h)
-- the NumPy statements alone (gwinferno_amd/draws.py: cdf_codes, point_cdfs_reference, weighted_percentiles), the host backend of
postprocess.catalog_predictive_check on a stub engine, the header, the library's exports and the refusals that need no device, and the
inputs of tests/test_gpu_point_cdfs.py, which are vetted here."""
import os
import re

import cdf_util as U
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cdf_codes_against_a_brute_force_count():
    """The code is the number of grid points below the value: values equal to a grid point (x == g_j gets j), below g_0, above
    g_{G-1}, NaN and infinities; grids that do not increase or are not finite are refused."""
    from gwinferno_amd import draws as D

    g = np.array([1.0, 1.5, 4.0, 4.5, 10.0])
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(0.0, 11.0, 500), g, [0.5, np.nextafter(1.0, 0.0), np.nextafter(10.0, 11.0), 11.0, np.nan, np.inf, -np.inf]])
    code = D.cdf_codes(x, g)
    assert code.dtype == np.uint16 and code.shape == x.shape
    brute = np.array([sum(1 for p in g if p < v) for v in x])
    want = np.where((brute < g.size) & ~np.isnan(x), brute, D.OUTSIDE_BIN)
    assert np.array_equal(code, want)
    assert np.array_equal(D.cdf_codes(g, g), np.arange(5))
    assert np.array_equal(D.cdf_codes([0.5, np.nextafter(1.0, 0.0), -np.inf], g), [0, 0, 0])
    assert np.all(D.cdf_codes([np.nextafter(10.0, 11.0), 11.0, np.nan, np.inf], g) == D.OUTSIDE_BIN)
    for j in range(g.size):  # the bins up to j hold exactly the values <= g_j
        assert np.array_equal(code <= j, x <= g[j])
    assert D.cdf_codes(np.ones((2, 3)), g).shape == (2, 3) and np.array_equal(D.cdf_codes([3.0], [3.0]), [0])
    for bad in ([1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [1.0, np.inf], [-np.inf, 1.0]):
        with pytest.raises(ValueError, match="finite and strictly increasing"):
            D.cdf_codes(x, bad)
    with pytest.raises(ValueError, match="1 ... 256"):
        D.cdf_codes(x, np.arange(257.0))
    with pytest.raises(ValueError, match="1 ... 256"):
        D.cdf_codes(x, [])


def _small_case(seed=5, n_ev=3, n_pe=40, n_inj=60, n_grid=6):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(0.0, 1.0, (2, n_ev, n_pe)), rng.normal(0.0, 1.2, (2, n_inj))
    lw_pe, lw_inj = rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj)
    lw_pe[0, 3], lw_inj[7] = -np.inf, np.nan
    grid = np.stack([np.linspace(-1.0, 1.0, n_grid), np.sort(rng.uniform(-1.5, 1.5, n_grid))])
    return x_pe, x_inj, lw_pe, lw_inj, grid


def _codes(x_pe, x_inj, grid):
    from gwinferno_amd.draws import cdf_codes

    return np.stack([cdf_codes(x_pe[c], grid[c]) for c in range(grid.shape[0])]), np.stack([cdf_codes(x_inj[c], grid[c]) for c in range(grid.shape[0])])


def _brute_cdf(lw, mask, x, grid):
    """sum of w over x <= g, over the sum of w, from the raw values: no codes, no bins, no cumsum"""
    ok = np.isfinite(lw) & (np.ones(lw.shape, bool) if mask is None else np.asarray(mask).astype(bool))
    w = np.where(ok, np.exp(np.where(ok, lw, 0.0) - lw[ok].max()), 0.0)
    return np.array([w[x <= g].sum() for g in grid]) / w.sum()


def test_statement_against_an_independent_brute_force():
    """Every F of the statement against sum w [x <= g] / sum w from the raw values, to (n + G) 2^-52 relative (n additions in the
    numerator and total on either side in another order, G in the running sum); F does not decrease in b; the slots are the plain
    reductions of the events' F; shapes and dtypes."""
    from gwinferno_amd import draws as D

    x_pe, x_inj, lw_pe, lw_inj, grid = _small_case()
    n_ev, n_pe = lw_pe.shape
    n_grid = grid.shape[1]
    pc, ic = _codes(x_pe, x_inj, grid)
    out, live = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert out.shape == (4, 2, n_grid) and live.shape == (2,) and live.dtype == np.int32 and np.array_equal(live, [n_ev, 1])
    f_ev = np.array([[_brute_cdf(lw_pe[e], None, x_pe[c, e], grid[c]) for c in range(2)] for e in range(n_ev)])
    f_inj = np.array([_brute_cdf(lw_inj, None, x_inj[c], grid[c]) for c in range(2)])
    assert np.all(np.abs(out[0] - f_inj) <= (lw_inj.size + n_grid) * 2.0**-52 * f_inj)
    tol = (n_pe + n_grid) * 2.0**-52
    assert np.all(np.abs(out[1] - f_ev.mean(axis=0)) <= tol * f_ev.mean(axis=0))
    assert np.all(np.diff(out[0], axis=-1) >= 0.0) and np.all(np.diff(out[1], axis=-1) >= 0.0) and np.all(out[0] <= 1.0 + tol)
    assert np.all(np.diff(out[2], axis=-1) >= -n_ev * tol) and np.all(np.diff(out[3], axis=-1) <= n_ev * tol)
    # slot 2 is the log of the PRODUCT of the events' CDFs, slot 3 of the product of their complements: small enough to multiply
    assert np.allclose(np.exp(out[2]), np.prod(f_ev, axis=0), rtol=1e-13, atol=0.0)
    assert np.allclose(np.exp(out[3]), np.prod(1.0 - f_ev, axis=0), rtol=1e-12, atol=0.0)
    # one set at a time
    only_pe, lp = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, None, n_grid)
    only_inj, li = D.point_cdfs_reference(lw_pe, lw_inj, None, None, None, ic, n_grid)
    assert np.all(np.isnan(only_pe[0])) and np.array_equal(only_pe[1:], out[1:]) and np.array_equal(lp, [n_ev, 0])
    assert np.all(np.isnan(only_inj[1:])) and np.array_equal(only_inj[0], out[0]) and np.array_equal(li, [0, 1])


def test_masked_event_is_not_live_and_dead_segments():
    """An event masked out entirely is not live and does not enter slots 1-3: they are those of the catalog without it, to the bit; a
    dead injection set gives NaN in slot 0 and nothing else changes; no live event gives NaN in slot 1 and empty sums in slots 2, 3."""
    from gwinferno_amd import draws as D

    x_pe, x_inj, lw_pe, lw_inj, grid = _small_case()
    n_ev, n_pe = lw_pe.shape
    n_grid = grid.shape[1]
    pc, ic = _codes(x_pe, x_inj, grid)
    full, _ = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    mask = np.ones((n_ev, n_pe), dtype=np.uint8)
    mask[1] = 0
    out, live = D.point_cdfs_reference(lw_pe, lw_inj, mask, None, pc, ic, n_grid)
    less, live_less = D.point_cdfs_reference(np.delete(lw_pe, 1, axis=0), lw_inj, None, None, np.delete(pc, 1, axis=1), ic, n_grid)
    assert np.array_equal(live, [n_ev - 1, 1]) and np.array_equal(live_less, [n_ev - 1, 1])
    assert np.array_equal(out, less) and not np.array_equal(out[1:], full[1:]) and np.array_equal(out[0], full[0])
    dead_inj, live = D.point_cdfs_reference(lw_pe, lw_inj, None, np.zeros(lw_inj.size, dtype=np.uint8), pc, ic, n_grid)
    assert np.all(np.isnan(dead_inj[0])) and np.array_equal(dead_inj[1:], full[1:]) and np.array_equal(live, [n_ev, 0])
    nothing, live = D.point_cdfs_reference(np.full((n_ev, n_pe), -np.inf), lw_inj, None, None, pc, ic, n_grid)
    assert np.array_equal(live, [0, 1]) and np.all(np.isnan(nothing[1])) and np.array_equal(nothing[2:], np.zeros((2, 2, n_grid))) and np.array_equal(nothing[0], full[0])


def test_all_samples_above_the_grid():
    """A column whose samples all lie above the grid (every code 0xFFFF) has F = 0: log_all_below is -inf, log_all_above 0 and cdf_obs
    0; one event without weight below a grid point is enough for -inf there.  Samples all below g_0 give F = 1: log_all_above -inf."""
    from gwinferno_amd import draws as D

    x_pe, x_inj, lw_pe, lw_inj, grid = _small_case()
    n_grid = grid.shape[1]
    x_pe = x_pe.copy()
    x_pe[1] += 100.0
    pc, ic = _codes(x_pe, x_inj, grid)
    assert np.all(pc[1] == D.OUTSIDE_BIN)
    out, live = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert np.array_equal(live, [3, 1]) and np.all(out[2, 1] == -np.inf) and np.array_equal(out[3, 1], np.zeros(n_grid)) and np.array_equal(out[1, 1], np.zeros(n_grid))
    assert np.all(np.isfinite(out[2, 0, -1]))
    x_one = x_pe.copy()
    x_one[0, 2] = 100.0  # one event of column 0
    pc, _ = _codes(x_one, x_inj, grid)
    out, _ = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert np.all(out[2, 0] == -np.inf) and np.all(out[1, 0] > 0.0) and np.all(np.isfinite(out[3, 0]))
    x_low = x_pe.copy()
    x_low[0] -= 100.0
    pc, _ = _codes(x_low, x_inj, grid)
    out, _ = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert np.all(out[3, 0] == -np.inf) and np.all(np.abs(out[2, 0]) <= 3 * 50 * 2.0**-52) and np.all(np.abs(out[1, 0] - 1.0) <= 50 * 2.0**-52)


def test_weighted_percentiles():
    """Inverted-CDF percentiles over the first axis: equal weights, a one-hot weight, NaN entries and zero weights left out, ties."""
    from gwinferno_amd.draws import weighted_percentiles

    v = np.array([[3.0, 1.0], [1.0, np.nan], [2.0, 5.0], [4.0, 5.0]])
    q = weighted_percentiles(v, np.ones(4), [0.0, 0.25, 0.5, 0.75, 1.0])
    assert q.shape == (5, 2) and np.array_equal(q[:, 0], [1.0, 1.0, 2.0, 3.0, 4.0]) and np.array_equal(q[:, 1], [1.0, 1.0, 5.0, 5.0, 5.0])
    assert np.array_equal(weighted_percentiles(v, [0.0, 0.0, 1.0, 0.0], [0.05, 0.5, 0.95]), np.broadcast_to(v[2], (3, 2)))
    assert np.array_equal(weighted_percentiles(v[:, 0], [1.0, 1.0, 1.0, 7.0], [0.5]), [4.0])
    assert np.all(np.isnan(weighted_percentiles(np.full((2, 3), np.nan), np.ones(2), [0.5])))
    for w, lv in (([1.0, -1.0, 1.0, 1.0], [0.5]), (np.ones(3), [0.5]), (np.ones(4), [1.5]), ([1.0, np.nan, 1.0, 1.0], [0.5])):
        with pytest.raises(ValueError):
            weighted_percentiles(v, w, lv)


class _StubEngine:
    """What catalog_predictive_check(backend="host") needs of an engine: the shapes and log_weights."""

    def __init__(self, lw_pe, lw_inj):
        self.lw_pe, self.lw_inj = lw_pe, lw_inj
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe[0].shape, lw_inj[0].size, 1

    def log_weights(self, theta):
        k = int(theta[0])
        return self.lw_pe[k].copy(), self.lw_inj[k].copy()


def _stub(k=5, seed=8):
    x_pe, x_inj, _, _, grid = _small_case()
    rng = np.random.default_rng(seed)
    lw_pe, lw_inj = rng.normal(0.0, 1.5, (k,) + x_pe.shape[1:]), rng.normal(0.0, 1.5, (k, x_inj.shape[1]))
    return _StubEngine(lw_pe, lw_inj), np.arange(k, dtype=np.float64)[:, None], {"a": x_pe[0], "b": x_pe[1]}, {"a": x_inj[0], "b": x_inj[1]}, {"a": grid[0], "b": grid[1]}


def test_catalog_predictive_check_on_the_host():
    """Shapes; the raw arrays are the statement's; the predicted extremes are n_obs times the logarithms of the detected CDF; the
    bands are ordered and made of the points' own values; a one-hot weight on point j returns point j's curves; the means are the
    means of the exponentiated quantities; a dead point is left out; validation errors."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, grid = _stub()
    k, n_grid = thetas.shape[0], 6
    r = P.catalog_predictive_check(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    assert r["names"] == ["a", "b"] and r["grid"].shape == (2, n_grid) and r["n_points"] == k and r["dead_detected"] == 0 and np.array_equal(r["n_live"], np.full(k, 3))
    for key in ("cdf_detected", "cdf_observed", "log_cdf_max_observed", "log_sf_min_observed", "log_cdf_max_predicted", "log_sf_min_predicted"):
        assert r[key].shape == (k, 2, n_grid), key
    for key in ("bands_detected", "bands_observed"):
        assert r[key].shape == (3, 2, n_grid) and np.all(np.diff(r[key], axis=0) >= 0.0), key
    for key in ("cdf_max_observed", "cdf_max_predicted", "cdf_min_observed", "cdf_min_predicted"):
        assert r[key].shape == (2, n_grid) and np.all((r[key] >= 0.0) & (r[key] <= 1.0)) and np.all(np.diff(r[key], axis=-1) >= -1e-15), key
    pc, ic = _codes(np.stack([pe_values["a"], pe_values["b"]]), np.stack([inj_values["a"], inj_values["b"]]), r["grid"])
    for i in range(k):
        out, _ = D.point_cdfs_reference(eng.lw_pe[i], eng.lw_inj[i], None, None, pc, ic, n_grid)
        assert np.array_equal(out, np.stack([r["cdf_detected"][i], r["cdf_observed"][i], r["log_cdf_max_observed"][i], r["log_sf_min_observed"][i]]))
    assert np.array_equal(r["log_cdf_max_predicted"], 3.0 * np.log(r["cdf_detected"])) and np.array_equal(r["log_sf_min_predicted"], 3.0 * np.log1p(-r["cdf_detected"]))
    assert np.array_equal(r["bands_observed"][1], np.sort(r["cdf_observed"], axis=0)[2])  # the median of five equal weights is the third value
    assert np.allclose(r["cdf_max_observed"], np.exp(r["log_cdf_max_observed"]).mean(axis=0), rtol=1e-14) and np.allclose(r["cdf_min_predicted"], 1.0 - np.exp(r["log_sf_min_predicted"]).mean(axis=0), rtol=1e-13)
    # n_obs, and a one-hot weight
    j = 3
    one = P.catalog_predictive_check(eng, thetas, pe_values, grid, inj_values=inj_values, n_obs=7, point_weights=np.eye(k)[j], param_names=["b", "a"], backend="host")
    assert one["names"] == ["b", "a"] and np.array_equal(one["log_cdf_max_predicted"], 7.0 * np.log(one["cdf_detected"]))
    for q in range(3):
        assert np.array_equal(one["bands_detected"][q], r["cdf_detected"][j, ::-1]) and np.array_equal(one["bands_observed"][q], r["cdf_observed"][j, ::-1])
    assert np.array_equal(one["cdf_max_observed"], np.exp(r["log_cdf_max_observed"][j, ::-1])) and np.array_equal(one["cdf_min_observed"], -np.expm1(r["log_sf_min_observed"][j, ::-1]))
    # a grid given as one array; no injections: no predicted side
    alone = P.catalog_predictive_check(eng, thetas, pe_values, np.linspace(-1.0, 1.0, 4), backend="host")
    assert alone["grid"].shape == (2, 4) and np.all(np.isnan(alone["cdf_detected"])) and np.all(np.isnan(alone["cdf_max_predicted"])) and alone["dead_detected"] == k
    assert np.all(np.isfinite(alone["cdf_observed"]))
    # a point at which nothing has weight is left out of the means and the bands
    eng.lw_pe[1][:] = -np.inf
    eng.lw_inj[1][:] = -np.inf
    gap = P.catalog_predictive_check(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    keep = [0, 2, 3, 4]
    assert np.array_equal(gap["n_live"], [3, 0, 3, 3, 3]) and gap["dead_detected"] == 1 and np.all(np.isnan(gap["cdf_observed"][1])) and np.all(np.isnan(gap["cdf_detected"][1]))
    assert np.allclose(gap["cdf_max_observed"], np.exp(r["log_cdf_max_observed"][keep]).mean(axis=0), rtol=1e-14)
    assert np.allclose(gap["cdf_max_predicted"], np.exp(r["log_cdf_max_predicted"][keep]).mean(axis=0), rtol=1e-14)
    assert np.array_equal(gap["bands_observed"], D.weighted_percentiles(r["cdf_observed"][keep], np.ones(4), [0.05, 0.5, 0.95]))


def test_validation_of_the_user_facing_function():
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, grid = _stub(k=2)
    call = lambda **kw: P.catalog_predictive_check(eng, thetas, pe_values, kw.pop("grid", grid), **{"inj_values": inj_values, "backend": "host", **kw})  # noqa: E731
    with pytest.raises(ValueError, match="1 <= G <= 256"):
        call(grid=np.arange(257.0))
    with pytest.raises(ValueError, match="unknown quantity 'c'"):
        call(param_names=["a", "c"])
    with pytest.raises(ValueError, match="strictly increasing"):
        call(grid={"a": [0.0, 0.0], "b": [0.0, 1.0]})
    with pytest.raises(ValueError, match="same number of grid points"):
        call(grid={"a": [0.0, 0.5, 1.0], "b": [0.0, 1.0]})
    with pytest.raises(ValueError, match="no points for"):
        call(grid={"a": [0.0, 1.0]})
    with pytest.raises(ValueError, match="point_weights"):
        call(point_weights=[1.0, -1.0])
    with pytest.raises(ValueError, match="point_weights"):
        call(point_weights=[0.0, 0.0])
    with pytest.raises(ValueError, match="point_weights"):
        call(point_weights=np.ones(3))
    with pytest.raises(ValueError, match="levels"):
        call(levels=[0.5, 1.5])
    with pytest.raises(ValueError, match="n_obs"):
        call(n_obs=0)
    with pytest.raises(ValueError, match="backend"):
        call(backend="cpu")
    with pytest.raises(ValueError, match="between 1 and 8"):
        P.catalog_predictive_check(eng, thetas, {str(i): pe_values["a"] for i in range(9)}, [0.0, 1.0], backend="host")


def test_header_library_and_refusals_without_a_device():
    """The two exports are declared, bound and listed; a null handle and a host-only handle answer GWI_ERR_INVALID, the latter with a
    message; the Python layer checks the thetas first and refuses an engine that holds a shard."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_point_cdfs", 5), ("gwi_point_cdf_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert "DESIGN 8g" in hdr and "more than 256 grid points" in hdr
    assert lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_cdfs(None, None, 1, None, None) == -1
    eng = U.composition(device=N.DEVICE_HOST_ONLY).engine()
    out, live = np.zeros((1, 4, 2, 5)), np.zeros((1, 2), dtype=np.int32)
    assert lib.gwi_point_cdfs(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(out), live.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert "gwi_point_cdfs: host-only" in lib.gwi_last_error(eng.handle).decode()
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.point_cdfs(np.zeros(eng.n_theta))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.point_cdfs(np.zeros(eng.n_theta + 1))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.point_cdfs(np.zeros((0, eng.n_theta)))
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_cdfs: this engine holds one shard of the catalog"):
        shard.point_cdfs(np.zeros(3))


def test_inputs_of_the_gpu_tests():
    """Every case tests/test_gpu_point_cdfs.py compares, from the host evaluation of the bound model: the shapes (two tiles per event
    and three of injections, the last of each ragged); every segment meant to be live has at least 150 samples with weight, all above
    hist_util.LOG_FLOOR relative to the segment's maximum (no weight can round to 0 on one side only); at every grid point every live
    segment has weight above (F <= 1 - 1e-4) and, in the mass_ratio column, below (F >= 1e-4), while on the mass_1 grid the heavy events
    have F = 0 exactly and the lightest one F >= 1e-4: the derived bounds of slots 2 and 3 are finite everywhere, no entry is left out
    of any comparison, and every -inf of slot 2 is an exact zero of F; the masked case has exactly one dead event; the codes use the full range and 0xFFFF."""
    import hist_util as HU

    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import OUTSIDE_BIN, draw_weights, point_cdfs_reference

    assert (U.N_EV, U.N_PE, U.N_INJ) == (3, 1500, 2500) and U.N_PE % HU.TILE not in (0,) and -(-U.N_PE // HU.TILE) == 2 and -(-U.N_INJ // HU.TILE) == 3 and U.N_INJ % HU.TILE
    comp = U.composition(device=N.DEVICE_HOST_ONLY)
    thetas = U.points(comp)
    assert thetas.shape == (U.N_POINTS, comp.engine().n_theta) and len({t.tobytes() for t in thetas}) == U.N_POINTS
    for n_grid in U.N_GRID:
        g = U.grid(n_grid)
        pc, ic = U.codes(n_grid)
        assert g.shape == (2, n_grid) and np.all(np.diff(g, axis=1) > 0) and pc.shape == (2, U.N_EV, U.N_PE) and ic.shape == (2, U.N_INJ)
        for c in (pc, ic):
            assert np.any(c == OUTSIDE_BIN) and np.any(c == 0) and np.any(c == n_grid - 1) and np.all((c < n_grid) | (c == OUTSIDE_BIN))
        for theta in thetas:
            lw_pe, lw_inj = HU.host_log_weights(comp.engine().bound, theta)
            for case in ("free", "masked"):
                pm, im = U.masks(case)
                dead = 0
                for seg, (lw, mask) in enumerate(HU.segments(lw_pe, lw_inj, pm, im)):
                    w = draw_weights(lw, mask)
                    if not w.any():
                        dead += 1
                        continue
                    assert np.count_nonzero(w) >= 150 and np.log(w[w > 0]).min() > HU.LOG_FLOOR
                assert dead == (1 if case == "masked" else 0)
                f, lives = U.statement_event_cdfs(lw_pe, pm, pc, n_grid)
                assert f.shape[0] == U.N_EV - dead and np.all(f[:, 0] >= 1e-4) and np.all((f[:, 1] >= 1e-4) | (f[:, 1] == 0.0)) and np.all(f <= 1.0 - 1e-4)
                assert np.all(f[-1, 1] > 0.0) and np.all(f[0, 1] == 0.0)  # the lightest event alone has weight on the mass_1 grid
                out, live = point_cdfs_reference(lw_pe, lw_inj, pm, im, pc, ic, n_grid)
                assert np.array_equal(live, [U.N_EV - dead, 1]) and np.all(out[0] >= 1e-4) and np.all(out[0] <= 1.0 - 1e-4)
                tol_below, tol_above = U.log_sum_bounds(f, lives, n_grid)
                assert np.all(np.isfinite(tol_below)) and np.all(np.isfinite(tol_above)) and tol_below.max() < 1e-11 and tol_above.max() < 1e-8
    pm, im = U.masks("no_inj")
    assert not im.any() and not pm[U.DEAD_EVENT].any() and pm[2].all()
