"""CPU: exact per-event calibration (include/gwi_engine.h: gwi_set_rank_columns, gwi_point_pits_exact; gwinferno_amd/csrc/gwi_rank.h;
DESIGN 8i) -- the NumPy statements alone (gwinferno_amd/draws.py: rank_codes, point_pits_exact_reference) against brute force, the exact
PIT inside the gridded bracket of draws.point_pits_reference on the inputs of tests/test_gpu_point_ranks.py, those inputs themselves,
the derived device tolerance, the host backend of postprocess.event_calibration_exact, and the header, the exports and the refusals
that need no device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import rank_util as RU
import test_pit_cpu as TP

CU, HU, PU = RU.CU, RU.HU, RU.PU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_codes_against_a_brute_force_count():
    """40 x 60 values drawn from eleven distinct numbers, so that most samples tie with injections and injections tie with each other:
    the ranks are the O(n m) counts, the order is a stable argsort, the dtypes and ranges are the contract's."""
    from gwinferno_amd.draws import rank_codes

    rng = np.random.default_rng(2)
    pe, inj = rng.integers(0, 11, (2, 2, 20)).astype(np.float64) / 4.0, rng.integers(1, 10, (2, 60)).astype(np.float64) / 4.0
    order, lt, le = rank_codes(pe, inj)
    assert order.dtype == lt.dtype == le.dtype == np.int32 and order.shape == (2, 60) and lt.shape == le.shape == (2, 2, 20)
    for c in range(2):
        assert np.array_equal(order[c], np.argsort(inj[c], kind="stable")) and np.array_equal(np.sort(order[c]), np.arange(60))
        for e in range(2):
            for i in range(20):
                assert lt[c, e, i] == sum(1 for y in inj[c] if y < pe[c, e, i]) and le[c, e, i] == sum(1 for y in inj[c] if y <= pe[c, e, i])
    assert lt.min() == 0 and le.max() == 60 and np.all(lt <= le) and np.any(lt < le) and np.any(lt == le)
    for bad, word in (((pe[0], inj), "n_cols"), ((np.where(pe == pe[0, 0, 0], np.nan, pe), inj), "finite"), ((pe, np.where(inj == inj[0, 0], np.inf, inj)), "finite"),
                      ((np.zeros((9, 1, 2)), np.zeros((9, 3))), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            rank_codes(*bad)


def test_the_statement_against_a_double_loop_in_fractions():
    """Tiny inputs with ties, a masked sample, a -inf and a NaN log-weight: pit_lt and pit_le are the double loop over (sample,
    injection) in fractions.Fraction on the statement's own weights, up to the statement's DERIVED rounding (rank_util.statement_rounding: 4
    2^-52 relative); a dead event gives NaN and its flag and nothing else changes; a dead injection set gives NaN everywhere."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(4)
    n_ev, n_pe, n_inj = 3, 12, 17
    x_pe, x_inj = rng.integers(0, 7, (2, n_ev, n_pe)).astype(np.float64), rng.integers(1, 6, (2, n_inj)).astype(np.float64)
    lw_pe, lw_inj = rng.normal(0.0, 2.0, (n_ev, n_pe)), rng.normal(0.0, 2.0, n_inj)
    lw_pe[0, 3], lw_inj[5] = -np.inf, np.nan
    pe_mask, inj_mask = np.ones((n_ev, n_pe), dtype=np.uint8), np.ones(n_inj, dtype=np.uint8)
    pe_mask[1, 2], inj_mask[9] = 0, 0
    codes = D.rank_codes(x_pe, x_inj)
    pit, dead = D.point_pits_exact_reference(lw_pe, lw_inj, pe_mask, inj_mask, *codes)
    assert pit.shape == (n_ev, 2, 2) and dead.shape == (n_ev + 1,) and dead.dtype == np.int32 and not dead.any()
    u = [Fraction(float(v)) for v in D.draw_weights(lw_inj, inj_mask)]
    for e in range(n_ev):
        w = [Fraction(float(v)) for v in D.draw_weights(lw_pe[e], pe_mask[e])]
        for c in range(2):
            below = sum(wi * sum(uj for uj, y in zip(u, x_inj[c]) if y < x) for wi, x in zip(w, x_pe[c, e])) / (sum(w) * sum(u))
            upto = sum(wi * sum(uj for uj, y in zip(u, x_inj[c]) if y <= x) for wi, x in zip(w, x_pe[c, e])) / (sum(w) * sum(u))
            assert below < upto  # (the integers tie)
            for got, want in zip(pit[e, c], (below, upto)):
                assert abs(Fraction(float(got)) - want) <= Fraction(RU.statement_rounding()) * want, (e, c)
    assert np.all(pit[..., 0] < pit[..., 1]) and np.all(pit > 0.0) and np.all(pit < 1.0)
    pe_mask[1] = 0
    p2, dead2 = D.point_pits_exact_reference(lw_pe, lw_inj, pe_mask, inj_mask, *codes)
    assert np.array_equal(dead2, [0, 1, 0, 0]) and np.all(np.isnan(p2[1])) and np.array_equal(p2[[0, 2]], pit[[0, 2]])
    p3, dead3 = D.point_pits_exact_reference(lw_pe, lw_inj, pe_mask, np.zeros(n_inj), *codes)
    assert np.array_equal(dead3, [0, 1, 0, 1]) and np.all(np.isnan(p3))
    with pytest.raises(ValueError, match="rank_lt <= rank_le"):
        D.point_pits_exact_reference(lw_pe, lw_inj, None, None, codes[0], codes[2] + 1, codes[2])


def _host_points():
    from gwinferno_amd import _native as N

    comp = CU.composition(device=N.DEVICE_HOST_ONLY)
    return [HU.host_log_weights(comp.engine().bound, theta) for theta in CU.points(comp)]


def test_inputs_of_the_gpu_tests_and_the_bracket_around_the_exact_pit():
    """The inputs of tests/test_gpu_point_ranks.py, from the host evaluation of the bound model.  Shapes: two PE tiles per event, the
    second ragged, three injection tiles, the last ragged.  The continuous column has no tie at all, the rounded one at most 200 distinct
    values and ties between the two sets on more than half of the PE samples.  Liveness: every segment is live in the free case, the
    masked case kills DEAD_EVENT alone, and every live weight lies above hist_util.LOG_FLOOR.  In exact arithmetic (pit_util.exact_pit's
    integers, imported: rank_util.exact_pits; its <= value IS pit_util.exact_pit's) pit_lo <= pit_lt <= pit_le <= pit_hi against
    draws.point_pits_reference for G = 1, 5 and 256, up to the bracket statement's own derived rounding (pit_util.statement_rounding);
    on the grid of ALL distinct values of the rounded column the bracket's ends ARE pit_lt and pit_le; and the float statement is within
    rank_util.statement_rounding of the exact value."""
    from gwinferno_amd.draws import point_pits_reference

    x_pe, x_inj = RU.columns()
    order, lt, le = RU.ranks()
    assert x_pe.shape == (2, CU.N_EV, CU.N_PE) and x_inj.shape == (2, CU.N_INJ) and CU.N_PE % RU.TILE != 0 and CU.N_INJ % RU.TILE != 0
    assert -(-CU.N_PE // RU.TILE) == 2 and -(-CU.N_INJ // RU.TILE) == 3 and CU.N_PE % 4 == 0
    assert np.array_equal(lt[0], le[0]) and np.unique(x_inj[0]).size == CU.N_INJ
    distinct = RU.distinct_grid()
    assert distinct.shape[1] <= 200 and np.mean(lt[RU.ROUNDED] < le[RU.ROUNDED]) > 0.5 and np.unique(x_inj[RU.ROUNDED]).size < CU.N_INJ
    for lw_pe, lw_inj in _host_points():
        for case in ("free", "masked"):
            pm, im = CU.masks(case)
            pit, dead, tol = RU.statement_point(lw_pe, lw_inj, pm, im)
            live = [e for e in range(CU.N_EV) if case == "free" or e != CU.DEAD_EVENT]
            assert np.array_equal(np.nonzero(dead)[0], [] if case == "free" else [CU.DEAD_EVENT])
            for lw, mask in HU.segments(lw_pe, lw_inj, pm, im):
                on = np.isfinite(lw) if mask is None else np.isfinite(lw) & (np.asarray(mask) != 0)
                assert not on.any() or np.all(lw[on] - lw[on].max() > HU.LOG_FLOOR)
            n_inj_live = HU.n_live(lw_inj, im)
            exact = {}
            for e in live:
                mask = None if pm is None else pm[e]
                for c in range(2):
                    exact[e, c] = RU.exact_pits(lw_pe[e], mask, x_pe[c, e], lw_inj, im, x_inj[c])
                    assert exact[e, c][1] == PU.exact_pit(lw_pe[e], mask, x_pe[c, e], lw_inj, im, x_inj[c])
                    assert exact[e, c][0] <= exact[e, c][1] and (exact[e, c][0] < exact[e, c][1]) == (c == RU.ROUNDED)
                    for got, want in zip(pit[e, c], exact[e, c]):
                        assert abs(Fraction(float(got)) - want) <= Fraction(RU.statement_rounding()) * want
            for grid in [CU.grid(g) for g in RU.N_GRID] + [distinct]:
                n_grid = grid.shape[1]
                pc, ic = RU.codes(grid)
                bracket, _, _ = point_pits_reference(lw_pe, lw_inj, pm, im, pc, ic, n_grid)
                for (e, c), (below, upto) in exact.items():
                    rel, absolute = PU.statement_rounding(HU.n_live(lw_pe[e], None if pm is None else pm[e]), n_inj_live, n_grid)
                    slack = rel * bracket[e, c, 1] + absolute + PU.U
                    assert bracket[e, c, 0] - slack <= below <= upto <= bracket[e, c, 1] + slack, (n_grid, case, e, c)
                    if grid is distinct and c == RU.ROUNDED:
                        assert abs(bracket[e, c, 0] - below) <= slack and abs(bracket[e, c, 1] - upto) <= slack
                        assert bracket[e, c, 1] - bracket[e, c, 0] > 1e-4  # (the ties carry weight: < and <= are told apart)


def test_the_device_tolerance_is_a_rounding_bound():
    """rank_util.device_tolerance is built from the sums' shapes -- the in-tile scan depth, n_inj_tiles and tiles_per_event additions, one
    product per term, two divisions and n_live terms in S -- in units of 2^-52, and stays below 1e-11 for the shapes of the GPU tests
    with every sample live: nothing can hide under it."""
    assert RU.SCAN_DEPTH == 3 + 6 + 3 + 1 + 4 + 1
    tol = RU.device_tolerance(CU.N_PE)
    assert tol == RU.device_tolerance(CU.N_PE, 3, 2) and 1.01 * (CU.N_PE + 8) * RU.U < tol < 1e-11
    assert RU.device_tolerance(CU.N_PE, 4, 2) - tol == pytest.approx(1.01 * RU.U) and RU.device_tolerance(CU.N_PE, 3, 4) - tol == pytest.approx(1.01 * RU.U)
    assert RU.device_tolerance(10) < RU.device_tolerance(11)


def test_event_calibration_exact_on_the_host():
    """On test_pit_cpu's stub engine: the raw arrays are the statement's; equal weights give the plain mean over the points; the
    midpoint, the sorted P-P curves and the Kolmogorov distances are what they say; the exact values lie inside event_calibration's
    brackets on the same inputs; (K,), (K, n_ev + 1), leave_one_out=True and leave_one_out="psis" weights; a dead (point, event) is
    skipped and counted; the refusals of the user-facing function."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    eng, thetas, pe_values, inj_values, grid = TP._stub()
    k, n_ev, rtol = thetas.shape[0], eng.n_ev, 7 * 2.0**-52
    r = P.event_calibration_exact(eng, thetas, pe_values, inj_values=inj_values, backend="host")
    assert r["names"] == ["a", "b"] and r["n_points"] == k and not r["n_dead"].any() and "elpd_loo" not in r and "pareto_k" not in r
    codes = D.rank_codes(np.stack([pe_values["a"], pe_values["b"]]), np.stack([inj_values["a"], inj_values["b"]]))
    for i in range(k):
        pit, dead = D.point_pits_exact_reference(eng.lw_pe[i], eng.lw_inj[i], None, None, *codes)
        assert np.array_equal(pit, r["point_pits"][i]) and np.array_equal(dead, r["dead"][i])
    raw = r["point_pits"]
    assert np.allclose(r["pit_lt"], raw[..., 0].mean(axis=0), rtol=rtol, atol=0.0) and np.allclose(r["pit_le"], raw[..., 1].mean(axis=0), rtol=rtol, atol=0.0)
    assert np.array_equal(r["pit"], 0.5 * (r["pit_lt"] + r["pit_le"])) and np.array_equal(r["pit_lt"], r["pit_le"])  # (continuous values: no tie)
    for key, src in (("pp_lt", "pit_lt"), ("pp_le", "pit_le"), ("pp", "pit")):
        assert r[key].shape == (2, n_ev) and np.array_equal(r[key], np.sort(r[src], axis=0).T) and np.all(np.diff(r[key], axis=1) >= 0.0), key
    for key, src in (("ks_lt", "pit_lt"), ("ks_le", "pit_le"), ("ks", "pit")):
        assert np.allclose(r[key], [TP._ks(r[src][:, c]) for c in range(2)], rtol=1e-15, atol=0.0), key
    gridded = P.event_calibration(eng, thetas, pe_values, grid, inj_values=inj_values, backend="host")
    assert np.all(gridded["point_pits"][..., 0] - 1e-13 <= raw[..., 0]) and np.all(raw[..., 1] <= gridded["point_pits"][..., 1] + 1e-13)
    v = np.random.default_rng(3).uniform(0.1, 1.0, (k, n_ev + 1))
    got = P.event_calibration_exact(eng, thetas, pe_values, inj_values=inj_values, point_weights=v, param_names=["b", "a"], backend="host")
    want = (v[:, :n_ev, None, None] * raw).sum(axis=0) / v[:, :n_ev].sum(axis=0)[:, None, None]
    assert got["names"] == ["b", "a"] and np.allclose(got["pit_lt"], want[:, ::-1, 0], rtol=rtol, atol=0.0)
    assert np.allclose(got["neff_points"], v[:, :n_ev].sum(axis=0) ** 2 / (v[:, :n_ev] ** 2).sum(axis=0), rtol=rtol)
    one = P.event_calibration_exact(eng, thetas, pe_values, inj_values=inj_values, point_weights=v[:, 0], backend="host")
    assert np.allclose(one["pit_le"], (v[:, 0, None, None] * raw[..., 1]).sum(axis=0) / v[:, 0].sum(), rtol=rtol, atol=0.0)
    ell = eng.log_bfs - eng.log_mu[:, None]
    for mode in (True, "psis"):  # (K = 5 leaves no tail to fit: the smoothed weights are the raw ones, and pareto_k says so)
        loo = P.event_calibration_exact(eng, thetas, pe_values, inj_values=inj_values, leave_one_out=mode, total_inj=1000.0, backend="host")
        vv = np.exp(ell.min(axis=0) - ell)
        want = (vv[:, :, None, None] * raw).sum(axis=0) / vv.sum(axis=0)[:, None, None]
        assert np.allclose(loo["pit_lt"], want[..., 0], rtol=rtol, atol=0.0) and np.allclose(loo["elpd_loo"], -np.log(np.mean(np.exp(-ell), axis=0)), rtol=1e-13)
        assert ("pareto_k" in loo) == (mode == "psis") and (mode is True or np.all(np.isinf(loo["pareto_k"])))
    eng.lw_pe[1][0] = -np.inf
    eng.lw_inj[3][:] = -np.inf
    gap = P.event_calibration_exact(eng, thetas, pe_values, inj_values=inj_values, backend="host")
    assert np.array_equal(gap["n_dead"], [2, 1, 1, 1]) and np.array_equal(gap["dead"][:, 0], [0, 1, 0, 0, 0]) and np.array_equal(gap["dead"][:, n_ev], [0, 0, 0, 1, 0])
    assert np.allclose(gap["pit_lt"][0], raw[[0, 2, 4], 0, :, 0].mean(axis=0), rtol=rtol, atol=0.0) and np.all(np.isfinite(gap["pit"]))
    call = lambda **kw: P.event_calibration_exact(eng, thetas, pe_values, **{"inj_values": inj_values, "backend": "host", **kw})  # noqa: E731
    for kw, word in ((dict(param_names=["a", "c"]), "unknown quantity 'c'"), (dict(point_weights=-np.ones(k)), "point weights"), (dict(leave_one_out="psis"), "needs total_inj"),
                     (dict(leave_one_out="psis", total_inj=1.0, point_weights=np.ones(k)), "point_weights must be None"), (dict(leave_one_out="loo"), "leave_one_out must be"),
                     (dict(backend="cpu"), "backend"), (dict(inj_values=None), "inj_values")):
        with pytest.raises(ValueError, match=word):
            call(**kw)


def test_header_library_and_refusals_without_a_device():
    """The three exports are declared, bound and listed; a null handle and a host-only handle answer GWI_ERR_INVALID, the latter with a
    message, and write nothing; the Python layer checks its arguments first and refuses an engine that holds a shard."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_set_rank_columns", 5), ("gwi_point_pits_exact", 5), ("gwi_point_rank_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_pits_exact.restype is C.c_int32 and lib.gwi_set_rank_columns.restype is C.c_int32 and lib.gwi_point_rank_times.restype is None
    assert "DESIGN 8i" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_pits_exact(None, None, 1, None, None) == -1 and lib.gwi_set_rank_columns(None, 1, None, None, None) == -1
    eng = CU.composition(device=N.DEVICE_HOST_ONLY).engine()
    i32 = C.POINTER(C.c_int32)
    pit, dead = np.full((1, CU.N_EV, 2, 2), 7.0), np.full((1, CU.N_EV + 1), 7, dtype=np.int32)
    assert lib.gwi_point_pits_exact(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(pit), dead.ctypes.data_as(i32)) == -1
    assert "gwi_point_pits_exact: host-only" in lib.gwi_last_error(eng.handle).decode() and np.all(pit == 7.0) and np.all(dead == 7)
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    lib.gwi_point_rank_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 0 and all(m.value == 0.0 for m in ms)  # the refused call launched nothing
    order, lt, le = RU.ranks()
    assert lib.gwi_set_rank_columns(eng.handle, 2, order.ctypes.data_as(i32), lt.ctypes.data_as(i32), le.ctypes.data_as(i32)) == -1
    assert "gwi_set_rank_columns: host-only" in lib.gwi_last_error(eng.handle).decode()
    x_pe, x_inj = RU.columns()
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.set_rank_columns(x_pe, x_inj)
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.point_pits_exact(np.zeros(eng.n_theta))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.point_pits_exact(np.zeros((0, eng.n_theta)))
    with pytest.raises(ValueError, match="both needed"):
        eng.set_rank_columns(x_pe, None)
    with pytest.raises(ValueError, match="pe_values has shape"):
        eng.set_rank_columns(x_pe[:, :, :-1], x_inj)
    with pytest.raises(ValueError, match="holds 2 columns, inj_values 1"):
        eng.set_rank_columns(x_pe, x_inj[:1])
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    for call in (lambda: shard.point_pits_exact(np.zeros(3)), lambda: shard.set_rank_columns(x_pe, x_inj)):
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: .*this engine holds one shard of the catalog"):
            call()
