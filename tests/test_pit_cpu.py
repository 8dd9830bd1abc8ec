"""CPU: per-event calibration (include/gwi_engine.h: gwi_point_pits; gwinferno_amd/csrc/gwi_pit.h) -- the NumPy statements
alone (gwinferno_amd/draws.py: pit_bracket, point_pits_reference), the validity of the bracket against the exact un-gridded PIT on the
catalog of tests/test_gpu_point_pits.py, the host backend of postprocess.event_calibration on a stub engine, the header, the library's
exports and the refusals that need no device, and a sanity check on a small mock catalog."""
import os
import re
import types

import numpy as np
import pit_util as PU
import pytest

CU, HU = PU.CU, PU.HU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pit_bracket_on_exact_binary_fractions():
    """Hand-made q and D whose products and sums are exact in float64: the expected numbers come out exactly.  G = 1 (the lower end is
    the outside term alone), all weight outside the grid ([D[G-1], 1]), all weight in bin 0 ([0, D[0]]), a general case, and bins that
    sum past 1 (o is clamped to 0)."""
    from gwinferno_amd.draws import pit_bracket

    assert pit_bracket([0.5], [0.25]) == (0.125, 0.625)  # o = 0.5: lo = o D[0]; hi = q[0] D[0] + o
    assert pit_bracket([0.0, 0.0, 0.0], [0.25, 0.5, 0.75]) == (0.75, 1.0)
    assert pit_bracket([1.0, 0.0, 0.0], [0.25, 0.5, 0.75]) == (0.0, 0.25)
    assert pit_bracket([0.0, 0.0, 1.0], [0.25, 0.5, 0.75]) == (0.5, 0.75)
    # o = 0.125: lo = 0.5 0.125 + 0.125 0.5 + 0.125 0.75; hi = 0.25 0.125 + 0.5 0.5 + 0.125 0.75 + 0.125
    assert pit_bracket([0.25, 0.5, 0.125], [0.125, 0.5, 0.75]) == (0.21875, 0.5)
    assert pit_bracket([0.75, 0.5], [0.5, 1.0]) == (0.25, 0.875)  # 1 - 1.25 < 0: o = 0
    lo, hi = pit_bracket(np.array([0.25, 0.25]), np.array([0.5, 1.0]))
    assert isinstance(lo, float) and isinstance(hi, float) and (lo, hi) == (0.125 + 0.5, 0.125 + 0.25 + 0.5)
    for q, d in (([], []), ([0.5], [0.5, 1.0])):
        with pytest.raises(ValueError, match="same number"):
            pit_bracket(q, d)


def test_statement_layout_and_liveness():
    """Shapes and dtypes; every entry is pit_bracket of the segment's own normalised bins and the injection set's cumsum; a dead
    event gives NaN and its flag and nothing else changes; a dead injection set gives NaN everywhere and its flag; both sets of bins
    are needed."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(5)
    n_ev, n_pe, n_inj, n_grid = 3, 40, 60, 6
    x_pe, x_inj = rng.normal(0.0, 1.0, (2, n_ev, n_pe)), rng.normal(0.0, 1.2, (2, n_inj))
    lw_pe, lw_inj = rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj)
    lw_pe[0, 3], lw_inj[7] = -np.inf, np.nan
    grid = np.stack([np.linspace(-1.0, 1.0, n_grid), np.sort(rng.uniform(-1.5, 1.5, n_grid))])
    pc, ic = (np.stack([D.cdf_codes(x[c], grid[c]) for c in range(2)]) for x in (x_pe, x_inj))
    pit, det, dead = D.point_pits_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert pit.shape == (n_ev, 2, 2) and det.shape == (2, n_grid) and dead.shape == (n_ev + 1,) and dead.dtype == np.int32 and not dead.any()
    out, _ = D.point_cdfs_reference(lw_pe, lw_inj, None, None, pc, ic, n_grid)
    assert np.array_equal(det, out[0])
    for e in range(n_ev):
        q, _ = D.weighted_histogram_segment(lw_pe[e], None, pc[:, e], n_grid)
        for c in range(2):
            assert tuple(pit[e, c]) == D.pit_bracket(q[c], det[c])
    assert np.all(pit[..., 0] <= pit[..., 1]) and np.all(pit >= 0.0) and np.all(pit <= 1.0 + 1e-14)
    mask = np.ones((n_ev, n_pe), dtype=np.uint8)
    mask[1] = 0
    p2, d2, dead2 = D.point_pits_reference(lw_pe, lw_inj, mask, None, pc, ic, n_grid)
    assert np.array_equal(dead2, [0, 1, 0, 0]) and np.all(np.isnan(p2[1])) and np.array_equal(p2[[0, 2]], pit[[0, 2]]) and np.array_equal(d2, det)
    p3, d3, dead3 = D.point_pits_reference(lw_pe, lw_inj, mask, np.zeros(n_inj, dtype=np.uint8), pc, ic, n_grid)
    assert np.array_equal(dead3, [0, 1, 0, 1]) and np.all(np.isnan(p3)) and np.all(np.isnan(d3))
    for a, b in ((None, ic), (pc, None)):
        with pytest.raises(ValueError, match="both sets"):
            D.point_pits_reference(lw_pe, lw_inj, None, None, a, b, n_grid)


def test_the_bracket_holds_the_exact_pit_on_the_test_catalog():
    """On the catalog, grids (G = 1, 5, 256), masks and three points of tests/test_gpu_point_pits.py, from the host evaluation of the
    bound model: the exact un-gridded PIT of every live event and quantity (pit_util.exact_pit: the weighted rank of each PE sample
    among the injections, with <=, in integer arithmetic on the statement's weights) lies in the statement's bracket up to the DERIVED
    rounding of the statement itself (pit_util.statement_rounding, about 1e-12), and the width is at most max_j (D[j] - D[j-1]) + o.
    The brackets are not trivial: at G = 256 the mass_ratio column's are narrower than 0.02 beside the share above the grid.  The dead
    event of the masked case is NaN and flagged."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import point_pits_reference, weighted_histogram_segment

    comp = CU.composition(device=N.DEVICE_HOST_ONLY)
    thetas = CU.points(comp)
    pe_values, inj_values = CU.values()
    for theta in thetas:
        lw_pe, lw_inj = HU.host_log_weights(comp.engine().bound, theta)
        for case in ("free", "masked"):
            pm, im = CU.masks(case)
            n_inj = HU.n_live(lw_inj, im)
            live = [e for e in range(CU.N_EV) if case == "free" or e != CU.DEAD_EVENT]
            exact = {(e, c): float(PU.exact_pit(lw_pe[e], None if pm is None else pm[e], pe_values[name][e], lw_inj, im, inj_values[name]))
                     for e in live for c, name in enumerate(CU.COLUMNS)}  # (a Fraction rounded once: half an ulp)
            for n_grid in PU.N_GRID:
                pc, ic = CU.codes(n_grid)
                pit, det, dead = point_pits_reference(lw_pe, lw_inj, pm, im, pc, ic, n_grid)
                assert np.array_equal(np.nonzero(dead)[0], [] if case == "free" else [CU.DEAD_EVENT])
                for e in range(CU.N_EV):
                    if e not in live:
                        assert np.all(np.isnan(pit[e]))
                        continue
                    mask = None if pm is None else pm[e]
                    rel, absolute = PU.statement_rounding(HU.n_live(lw_pe[e], mask), n_inj, n_grid)
                    q, _ = weighted_histogram_segment(lw_pe[e], mask, pc[:, e], n_grid)
                    for c in range(len(CU.COLUMNS)):
                        lo, hi = pit[e, c]
                        tol = rel * hi + absolute + PU.U
                        assert lo - tol <= exact[e, c] <= hi + tol, (n_grid, case, e, c, lo, exact[e, c], hi)
                        o = max(0.0, 1.0 - np.cumsum(q[c])[-1])
                        step = np.max(np.diff(np.concatenate([[0.0], det[c]])))
                        assert 0.0 <= hi - lo <= step + o + tol, (n_grid, case, e, c, hi - lo, step, o)
                        if n_grid == 256 and c == 0:
                            assert hi - lo < 0.02 + o


class _StubEngine:
    """What event_calibration(backend="host") needs of an engine: the shapes, log_weights, and for leave_one_out=True the per-event
    log Bayes factors and the detection efficiency of evaluate_batch."""

    def __init__(self, lw_pe, lw_inj, log_bfs=None, log_mu=None):
        self.lw_pe, self.lw_inj, self.log_bfs, self.log_mu = lw_pe, lw_inj, log_bfs, log_mu
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe[0].shape, lw_inj[0].size, 1
        self.n_ev_global, self.max_batch = self.n_ev, 2

    def log_weights(self, theta):
        k = int(theta[0])
        return self.lw_pe[k].copy(), self.lw_inj[k].copy()

    def evaluate_batch(self, thetas, total_inj, **kw):
        assert kw["want_grad"] is False and kw["min_neff_cut"] is False
        return [types.SimpleNamespace(log_bfs=self.log_bfs[int(t[0])], summary=types.SimpleNamespace(log_det_eff=self.log_mu[int(t[0])], log_nEff_inj=np.log(50.0))) for t in thetas]


def _stub(k=5, seed=8, n_ev=4, n_pe=40, n_inj=60, n_grid=6):
    rng = np.random.default_rng(seed)
    x_pe, x_inj = rng.normal(0.0, 1.0, (2, n_ev, n_pe)), rng.normal(0.0, 1.2, (2, n_inj))
    lw_pe, lw_inj = rng.normal(0.0, 1.5, (k, n_ev, n_pe)), rng.normal(0.0, 1.5, (k, n_inj))
    grid = {"a": np.linspace(-1.0, 1.0, n_grid), "b": np.sort(rng.uniform(-1.5, 1.5, n_grid))}
    eng = _StubEngine(lw_pe, lw_inj, rng.normal(0.0, 1.0, (k, n_ev)), rng.normal(-3.0, 0.2, k))
    return eng, np.arange(k, dtype=np.float64)[:, None], {"a": x_pe[0], "b": x_pe[1]}, {"a": x_inj[0], "b": x_inj[1]}, grid


def _ks(u):
    u = np.sort(u)
    n = u.size
    return max(max((i + 1) / n - u[i], u[i] - i / n) for i in range(n))


def test_event_calibration_on_the_host():
    """Shapes; the raw arrays are the statement's; equal weights reproduce the plain mean over the points; the midpoint, the width,
    the sorted P-P curves and the Kolmogorov distances are what they say; a point of weight 0 is the run without it, to the bit; the
    (K, n_ev + 1) path and the leave-one-out path agree with a direct NumPy evaluation; a dead (point, event) is skipped and counted.
    The weighted means are sums of K = 5 non-negative terms over a sum of 5 weights: (K + 2) 2^-52 relative covers both sides."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, grid = _stub()
    k, n_ev, n_grid, rtol = thetas.shape[0], eng.n_ev, 6, 7 * 2.0**-52
    r = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    assert r["names"] == ["a", "b"] and r["grid"].shape == (2, n_grid) and r["n_points"] == k and not r["n_dead"].any() and "elpd_loo" not in r
    assert r["point_pits"].shape == (k, n_ev, 2, 2) and r["cdf_detected"].shape == (k, 2, n_grid) and r["dead"].shape == (k, n_ev + 1)
    for key in ("pit_lo", "pit_hi", "pit", "width"):
        assert r[key].shape == (n_ev, 2), key
    pc, ic = (np.stack([D.cdf_codes(v[name], grid[name]) for name in ("a", "b")]) for v in (pe_values, inj_values))
    for i in range(k):
        pit, det, dead = D.point_pits_reference(eng.lw_pe[i], eng.lw_inj[i], None, None, pc, ic, n_grid)
        assert np.array_equal(pit, r["point_pits"][i]) and np.array_equal(det, r["cdf_detected"][i]) and np.array_equal(dead, r["dead"][i])
    raw = r["point_pits"]
    assert np.allclose(r["pit_lo"], raw[..., 0].mean(axis=0), rtol=rtol, atol=0.0) and np.allclose(r["pit_hi"], raw[..., 1].mean(axis=0), rtol=rtol, atol=0.0)
    assert np.array_equal(r["pit"], 0.5 * (r["pit_lo"] + r["pit_hi"])) and np.array_equal(r["width"], r["pit_hi"] - r["pit_lo"]) and np.all(r["width"] > 0.0)
    assert np.allclose(r["neff_points"], k, rtol=rtol)
    assert np.array_equal(r["pp_levels"], np.arange(1, n_ev + 1) / n_ev)
    for key, src in (("pp_lo", "pit_lo"), ("pp_hi", "pit_hi"), ("pp", "pit")):
        assert r[key].shape == (2, n_ev) and np.array_equal(r[key], np.sort(r[src], axis=0).T), key
    for key, src in (("ks_lo", "pit_lo"), ("ks_hi", "pit_hi"), ("ks", "pit")):
        assert r[key].shape == (2,) and np.allclose(r[key], [_ks(r[src][:, c]) for c in range(2)], rtol=1e-15, atol=0.0), key
    # a point of weight 0 is the run without it
    zero = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, point_weights=[1.0, 1.0, 0.0, 1.0, 1.0], backend="host")
    less = P.event_calibration(eng, thetas[[0, 1, 3, 4]], pe_values, grid, inj_values=inj_values, backend="host")
    for key in ("pit_lo", "pit_hi", "pit", "width", "neff_points", "pp_lo", "pp_hi", "ks_lo", "ks_hi", "ks"):
        assert np.array_equal(zero[key], less[key]), key
    # one weight per (point, segment); the quantities in another order
    v = np.random.default_rng(3).uniform(0.1, 1.0, (k, n_ev + 1))
    got = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, point_weights=v, param_names=["b", "a"], backend="host")
    want = (v[:, :n_ev, None, None] * raw).sum(axis=0) / v[:, :n_ev].sum(axis=0)[:, None, None]
    assert got["names"] == ["b", "a"] and np.allclose(got["pit_lo"], want[:, ::-1, 0], rtol=rtol, atol=0.0) and np.allclose(got["pit_hi"], want[:, ::-1, 1], rtol=rtol, atol=0.0)
    assert np.allclose(got["neff_points"], v[:, :n_ev].sum(axis=0) ** 2 / (v[:, :n_ev] ** 2).sum(axis=0), rtol=rtol)
    # leave-one-out: v_ke = exp(-l_ke + min_k l_ke) with l_ke = logBF_ke - log mu_k
    loo = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, leave_one_out=True, total_inj=1000.0, backend="host")
    ell = eng.log_bfs - eng.log_mu[:, None]
    v = np.exp(ell.min(axis=0) - ell)
    want = (v[:, :, None, None] * raw).sum(axis=0) / v.sum(axis=0)[:, None, None]
    assert np.allclose(loo["pit_lo"], want[..., 0], rtol=rtol, atol=0.0) and np.allclose(loo["pit_hi"], want[..., 1], rtol=rtol, atol=0.0)
    assert np.allclose(loo["neff_points"], v.sum(axis=0) ** 2 / (v * v).sum(axis=0), rtol=rtol) and np.all(loo["neff_points"] < k)
    assert np.allclose(loo["elpd_loo"], -np.log(np.mean(np.exp(-ell), axis=0)), rtol=1e-13)
    assert not np.allclose(loo["pit_lo"], r["pit_lo"], rtol=1e-6)
    # a dead (point, event) and a dead injection set at another point
    eng.lw_pe[1][0] = -np.inf
    eng.lw_inj[3][:] = -np.inf
    gap = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    assert np.array_equal(gap["n_dead"], [2, 1, 1, 1]) and np.array_equal(gap["dead"][:, 0], [0, 1, 0, 0, 0]) and np.array_equal(gap["dead"][:, n_ev], [0, 0, 0, 1, 0])
    assert np.allclose(gap["pit_lo"][0], raw[[0, 2, 4], 0, :, 0].mean(axis=0), rtol=rtol, atol=0.0) and np.allclose(gap["pit_hi"][1], raw[[0, 1, 2, 4], 1, :, 1].mean(axis=0), rtol=rtol, atol=0.0)
    assert np.allclose(gap["neff_points"], [3, 4, 4, 4], rtol=rtol) and np.all(np.isfinite(gap["pit"]))
    # an event that is dead at every point has no PIT and is left out of the curves
    for i in range(k):
        eng.lw_pe[i][2] = -np.inf
    none = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    assert np.all(np.isnan(none["pit"][2])) and none["n_dead"][2] == k and none["neff_points"][2] == 0.0 and none["pp_lo"].shape == (2, n_ev - 1)
    assert np.array_equal(none["pp_levels"], np.arange(1, n_ev) / (n_ev - 1)) and np.all(np.isfinite(none["ks"]))


def test_validation_of_the_user_facing_function():
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, grid = _stub(k=2)
    call = lambda **kw: P.event_calibration(eng, thetas, pe_values, kw.pop("grid", grid), **{"inj_values": inj_values, "backend": "host", **kw})  # noqa: E731
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
    with pytest.raises(ValueError, match="point weights"):
        call(point_weights=[1.0, -1.0])
    with pytest.raises(ValueError, match="point weights"):
        call(point_weights=np.ones(3))
    with pytest.raises(ValueError, match="point_weights must be None"):
        call(point_weights=np.ones(2), leave_one_out=True, total_inj=10.0)
    with pytest.raises(ValueError, match="needs total_inj"):
        call(leave_one_out=True)
    with pytest.raises(ValueError, match="backend"):
        call(backend="cpu")
    with pytest.raises(ValueError, match="inj_values"):
        call(inj_values=None)
    with pytest.raises(ValueError, match="holds no point"):
        P.event_calibration(eng, np.zeros((0, 1)), pe_values, grid, inj_values=inj_values, backend="host")
    with pytest.raises(ValueError, match="between 1 and 8"):
        P.event_calibration(eng, thetas, {str(i): pe_values["a"] for i in range(9)}, [0.0, 1.0], inj_values={str(i): inj_values["a"] for i in range(9)}, backend="host")


def test_header_library_and_refusals_without_a_device():
    """The two exports are declared, bound and listed; a null handle and a host-only handle answer GWI_ERR_INVALID, the latter with a
    message; the Python layer checks the thetas first and refuses an engine that holds a shard."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_point_pits", 6), ("gwi_point_pit_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_pits.restype is C.c_int32 and lib.gwi_point_pit_times.restype is None
    assert "DESIGN 8h" in hdr and "the exact un-gridded PIT" in hdr
    assert lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_pits(None, None, 1, None, None, None) == -1
    eng = CU.composition(device=N.DEVICE_HOST_ONLY).engine()
    pit, dead = np.full((1, CU.N_EV, 2, 2), 7.0), np.full((1, CU.N_EV + 1), 7, dtype=np.int32)
    assert lib.gwi_point_pits(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(pit), None, dead.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert "gwi_point_pits: host-only" in lib.gwi_last_error(eng.handle).decode() and np.all(pit == 7.0) and np.all(dead == 7)
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    lib.gwi_point_pit_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 0 and all(m.value == 0.0 for m in ms)  # the refused call launched nothing
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.point_pits(np.zeros(eng.n_theta))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.point_pits(np.zeros(eng.n_theta + 1))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.point_pits(np.zeros((0, eng.n_theta)))
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_pits: this engine holds one shard of the catalog"):
        shard.point_pits(np.zeros(3))


class _HostEngine:
    """event_calibration(backend="host") on a host-only handle: the shapes, and log_weights from the independent host evaluation of
    the bound model (tests/bound_eval.py)."""

    def __init__(self, comp):
        eng = comp.engine()
        self.bound, self.n_ev, self.n_pe, self.n_inj, self.n_theta = eng.bound, eng.n_ev, eng.n_pe, eng.n_inj, eng.n_theta

    def log_weights(self, theta):
        from bound_eval import log_weights

        lpe, linj, _ = log_weights(self.bound, np.asarray(theta, dtype=np.float64), include_consts=True)
        return np.asarray(lpe, dtype=np.float64).reshape(self.n_ev, self.n_pe), np.asarray(linj, dtype=np.float64)


def test_mock_catalog_sanity():
    """A small mock catalog made on the host (tests/mock_util.py: 48 events x 128 samples, 20 000 generated injections, seed 3) from a
    PL+Peak population: the Kolmogorov distance from uniform of the events' midpoint mass_1 PITs at the TRUE hyper-parameters is
    smaller than at a deliberately wrong point, the primary-mass slope alpha shifted from -2.5 to -0.5 (a far too heavy population:
    the events pile up at low PIT).  A comparison, not a threshold; it was checked to hold for seeds 3, 4 and 5 (0.08 against 0.43, 0.23
    against 0.42, 0.19 against 0.56) before seed 3 was committed.  The brackets are narrow beside either distance."""
    import mock_util as MU

    from gwinferno_amd import _native as N
    from gwinferno_amd import mock_catalog as MC
    from gwinferno_amd import postprocess as P
    from gwinferno_amd.compositions import COMPOSITIONS

    model = MU.catalog_model(MC)
    pe, inj, _, _ = MC.make_mock_catalog(MU.population(MC), MU.injection_tables(model), model, 48, 128, 20_000, 3, backend="host")
    inj = {k: v for k, v in inj.items() if k != "snr"}
    comp = COMPOSITIONS["plpeak"](pe, inj, mmin=MU.MMIN, mmax=MU.MMAX)
    comp.engine(device=N.DEVICE_HOST_ONLY)
    eng = _HostEngine(comp)
    grid = np.geomspace(MU.MMIN * 0.9, MU.MMAX * 1.1, 128)
    ks = {}
    for label, shift in (("true", {}), ("wrong", {"alpha": -0.5})):
        theta = comp.theta({**{k: MU.THETA[k] for k in comp.PARAMS}, **shift})
        r = P.event_calibration(eng, theta[None], {"mass_1": pe["mass_1"]}, grid, inj_values={"mass_1": inj["mass_1"]}, backend="host")
        assert r["pit"].shape == (48, 1) and not r["n_dead"].any() and np.all((r["pit_lo"] >= 0.0) & (r["pit_hi"] <= 1.0 + 1e-12)) and r["width"].max() < 0.05
        assert abs(r["ks_lo"][0] - r["ks"][0]) <= r["width"].max() and abs(r["ks_hi"][0] - r["ks"][0]) <= r["width"].max()
        ks[label] = float(r["ks"][0])
    print(f"Kolmogorov distance of the midpoint PITs: {ks['true']:.3f} at the true point, {ks['wrong']:.3f} with alpha = -0.5")
    assert ks["true"] < ks["wrong"]
