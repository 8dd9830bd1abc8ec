"""CPU: marginal weights and weighted quantiles (include/gwi_engine.h: gwi_marginal_weights_add, gwi_weighted_quantiles;
gwinferno_amd/csrc/gwi_quant.h) -- the NumPy statement (gwinferno_amd/draws.py: marginal_weights_reference,
weighted_quantiles_reference) against NumPy's own inverted-CDF quantile and on cases worked by hand, its invariance under the split
of the points, postprocess.event_credible_intervals(backend="host"), the header, the library's exports and the refusals that need no
device, and the inputs of tests/test_gpu_quant.py, which are vetted here."""
import ctypes as C
import os
import re

import hist_util as U
import numpy as np
import pytest
import quant_util as QU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_with_equal_weights_is_numpys_inverted_cdf():
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(5)
    levels = np.concatenate([[0.0, 1.0, 0.05, 0.5, 0.95, 0.25, 1.0 / 3.0], rng.uniform(size=20)])
    # (sizes at which no p n is an integer but for the dyadic levels: the statement takes the double p exactly -- 0.05 is a little
    # above 1 / 20 -- where NumPy rounds the product p n)
    for n in (1, 2, 7, 101, 1501):
        x = np.round(rng.normal(size=n), 1) if n == 101 else rng.normal(size=n)  # (n = 101: ties)
        order = np.argsort(x, kind="stable")
        idx, (m1, m2), mass = D.weighted_quantiles_reference(np.ones(n), order, x, levels)
        assert idx.dtype == np.int32 and idx.shape == levels.shape and mass == float(n)
        try:
            want = np.quantile(x, levels, method="inverted_cdf")
        except TypeError:  # a NumPy without the method
            want = np.sort(x)[np.maximum(np.ceil(levels * n).astype(int) - 1, 0)]
        assert np.array_equal(x[idx], want), n
        assert abs(m1 - x.sum()) <= 1e-12 * np.abs(x).sum() and abs(m2 - (x * x).sum()) <= 1e-12 * (x * x).sum()
        assert x[idx[0]] == x.min() and x[idx[1]] == x.max()


def test_ties_masks_and_dead_segments():
    """Worked by hand: W = (1, 0, 2, 1) on x = (3, 1, 2, 2): the order (stable) is samples 1, 2, 3, 0; prefixes 0, 2, 3, 4."""
    from gwinferno_amd import draws as D

    W, x = np.array([1.0, 0.0, 2.0, 1.0]), np.array([3.0, 1.0, 2.0, 2.0])
    order = np.argsort(x, kind="stable")
    assert np.array_equal(order, [1, 2, 3, 0])
    idx, (m1, m2), mass = D.weighted_quantiles_reference(W, order, x, [0.0, 0.25, 0.5, 0.500001, 0.75, 0.76, 1.0])
    # p = 0: the smallest value WITH weight (sample 1 has none); targets 1, 2 -> prefix 2 (sample 2); 2.000004, 3 -> sample 3; above 3 -> sample 0
    assert np.array_equal(idx, [2, 2, 2, 3, 3, 0, 0]) and mass == 4.0 and m1 == 3.0 + 4.0 + 2.0 and m2 == 9.0 + 8.0 + 4.0
    # ties are in the caller's order: with samples 3 and 2 swapped in the order the median moves to sample 3
    idx2, _, _ = D.weighted_quantiles_reference(W, np.array([1, 3, 2, 0]), x, [0.25, 0.5])
    assert np.array_equal(idx2, [3, 2])
    # a weight far below the others still is the largest value at p = 1, and never at p < 1 by rounding
    W3 = np.array([1.0, 1.0, 1e-300])
    idx3, _, mass3 = D.weighted_quantiles_reference(W3, np.arange(3), np.array([1.0, 2.0, 3.0]), [1.0, np.nextafter(1.0, 0.0)])
    assert np.array_equal(idx3, [2, 1]) and mass3 == 2.0
    # nothing with weight: -1, zeros
    idx4, mom4, mass4 = D.weighted_quantiles_reference(np.zeros(4), order, x, [0.0, 0.5, 1.0])
    assert np.array_equal(idx4, [-1, -1, -1]) and mom4 == (0.0, 0.0) and mass4 == 0.0
    for bad in (dict(order=[0, 0, 1, 2]), dict(order=[0, 1, 2, 3]), dict(levels=[1.5]), dict(levels=[np.nan]), dict(W=[1.0, -1.0, 0.0, 0.0])):
        kw = dict(W=W, order=order, x=x, levels=[0.5])
        kw.update(bad)
        with pytest.raises(ValueError):
            D.weighted_quantiles_reference(**kw)
    # marginal weights: masks leave numerator and total; a dead segment adds nothing and is counted
    lw_pe = np.log(np.array([[[1.0, 3.0, 4.0], [1.0, 1.0, 2.0]], [[1.0, 1.0, 2.0], [1.0, 1.0, 1.0]]]))  # (K = 2, 2 events, 3 samples)
    lw_pe[1, 1] = [-np.inf, np.nan, np.inf]
    lw_inj = np.log(np.array([[1.0, 1.0], [1.0, 3.0]]))
    wp, wi, dead, n_points = D.marginal_weights_reference(lw_pe, lw_inj, None, None)
    assert n_points == 2 and dead.dtype == np.int32 and np.array_equal(dead, [0, 1, 0])
    assert np.allclose(wp[0], [1 / 8 + 1 / 4, 3 / 8 + 1 / 4, 1 / 2 + 1 / 2], rtol=1e-15, atol=0) and np.allclose(wp[1], [0.25, 0.25, 0.5], rtol=1e-15, atol=0)
    assert np.allclose(wi, [0.5 + 0.25, 0.5 + 0.75], rtol=1e-15, atol=0)
    wp, wi, dead, _ = D.marginal_weights_reference(lw_pe, lw_inj, np.array([[1, 1, 0], [0, 0, 0]]), np.array([0, 1]))
    assert np.array_equal(dead, [0, 2, 0]) and np.allclose(wp[0], [0.25 + 0.5, 0.75 + 0.5, 0.0], rtol=1e-15, atol=0) and not wp[1].any() and np.array_equal(wi, [0.0, 2.0])


def test_statement_is_invariant_under_the_split_of_the_points():
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(6)
    lw_pe, lw_inj = rng.normal(0.0, 3.0, (3, 2, 300)), rng.normal(0.0, 3.0, (3, 500))
    lw_pe[1, 0] = -np.inf
    whole = D.marginal_weights_reference(lw_pe, lw_inj, None, None)
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        wp, wi, dead, n, at = np.zeros((2, 300)), np.zeros(500), np.zeros(3, dtype=np.int32), 0, 0
        for m in split:
            # (adding a part's sum onto the running sum is the running sum of the parts only for parts of ONE point: the statement adds
            # point by point, as the device does)
            for p in range(at, at + m):
                a, b, d, one = D.marginal_weights_reference(lw_pe[p : p + 1], lw_inj[p : p + 1], None, None)
                wp, wi, dead, n = wp + a, wi + b, dead + d, n + one
            at += m
        assert np.array_equal(wp, whole[0]) and np.array_equal(wi, whole[1]) and np.array_equal(dead, whole[2]) and n == whole[3] == 3
    assert np.array_equal(whole[2], [1, 0, 0])


def test_new_symbols_in_binding_header_and_library():
    from gwinferno_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    want = {"gwi_marginal_weights_reset": 1, "gwi_marginal_weights_add": 3, "gwi_marginal_weights_read": 5, "gwi_set_quantile_columns": 6, "gwi_weighted_quantiles": 8,
            "gwi_quantile_times": 4}
    for sym, n_args in want.items():
        assert sym in _native.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args, sym
    assert lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_marginal_weights_reset(None) == -1 and lib.gwi_marginal_weights_add(None, None, 1) == -1 and lib.gwi_marginal_weights_read(None, None, None, None, None) == -1
    assert lib.gwi_set_quantile_columns(None, 1, None, None, None, None) == -1 and lib.gwi_weighted_quantiles(None, None, 1, None, None, None, None, None) == -1


def test_host_only_handle_and_validation():
    """A host-only handle answers GWI_ERR_INVALID with a message from every entry; the Python layer checks shapes and values before
    the library is asked."""
    from gwinferno_amd import _native as N

    eng = U.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    vp, vi = QU.columns(1)
    for call in (lambda: eng.marginal_weights_reset(), lambda: eng.marginal_weights_add(np.zeros(eng.n_theta)), lambda: eng.marginal_weights(),
                 lambda: eng.set_quantile_columns(vp, vi), lambda: eng.weighted_quantiles([0.5])):
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
            call()
    lib, i32 = eng.lib, C.POINTER(C.c_int32)
    op, oi = QU.orders(1)
    th, dead, n, mass = np.zeros(eng.n_theta), np.zeros(U.N_EV + 1, dtype=np.int32), C.c_int64(0), np.zeros(U.N_EV + 1)
    for st in (lib.gwi_marginal_weights_reset(eng.handle), lib.gwi_marginal_weights_add(eng.handle, N.as_dp(th), 1),
               lib.gwi_marginal_weights_read(eng.handle, None, None, dead.ctypes.data_as(i32), C.byref(n)),
               lib.gwi_set_quantile_columns(eng.handle, 1, N.as_dp(vp), op.ctypes.data_as(i32), N.as_dp(vi), oi.ctypes.data_as(i32)),
               lib.gwi_weighted_quantiles(eng.handle, N.as_dp(np.array([0.5])), 1, None, None, None, None, N.as_dp(mass))):
        assert st == -1 and "host-only" in lib.gwi_last_error(eng.handle).decode()
    with pytest.raises(ValueError, match="both None"):
        eng.set_quantile_columns()
    with pytest.raises(ValueError, match="pe_values has shape"):
        eng.set_quantile_columns(vp[:, :, :-1], vi)
    with pytest.raises(ValueError, match="pe_values has shape"):
        eng.set_quantile_columns(vp[0], vi)
    with pytest.raises(ValueError, match="inj_values has shape"):
        eng.set_quantile_columns(vp, vi[:, :-1])
    with pytest.raises(ValueError, match="columns"):
        eng.set_quantile_columns(np.concatenate([vp, vp]), vi)
    bad = vi.copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="inj_values holds values that are not finite"):
        eng.set_quantile_columns(vp, bad)
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.marginal_weights_add(np.zeros(eng.n_theta + 1))
    with pytest.raises(ValueError, match="levels has shape"):
        eng.weighted_quantiles(np.zeros((2, 2)))


def test_world_above_one_is_refused_in_python():
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    eng = object.__new__(NativePopulationLikelihood)
    eng.world = 2
    for call, name in ((lambda: eng.marginal_weights_reset(), "marginal_weights_reset"), (lambda: eng.marginal_weights_add(np.zeros(3)), "marginal_weights_add"),
                       (lambda: eng.marginal_weights(), "marginal_weights"), (lambda: eng.set_quantile_columns(np.zeros((1, 1, 1))), "set_quantile_columns"),
                       (lambda: eng.weighted_quantiles([0.5]), "weighted_quantiles")):
        with pytest.raises(N.NativeEngineError, match=f"GWI_ERR_UNSUPPORTED: {name}: this engine holds one shard of the catalog"):
            call()


class _StubEngine:
    """What event_credible_intervals(backend="host") needs of an engine: the shapes and log_weights."""

    def __init__(self, lw_pe, lw_inj):
        self.lw_pe, self.lw_inj = lw_pe, lw_inj
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe[0].shape, lw_inj[0].size, 1

    def log_weights(self, theta):
        k = int(theta[0])
        return self.lw_pe[k].copy(), self.lw_inj[k].copy()


def test_event_credible_intervals_on_the_host():
    """The host backend is the statement; the mean and sd are those of the weights; a segment without weight gives NaN; the argument
    checks."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    rng = np.random.default_rng(8)
    k, n_ev, n_pe, n_inj = 4, 3, 200, 350
    lw_pe, lw_inj = rng.normal(0.0, 2.0, (k, n_ev, n_pe)), rng.normal(0.0, 2.0, (k, n_inj))
    lw_pe[:, 1] = -np.inf  # event 1 never has weight
    lw_pe[2, 0] = np.nan   # event 0 is dead at point 2
    eng = _StubEngine(lw_pe, lw_inj)
    pe_values = {"a": rng.normal(0.0, 1.0, (n_ev, n_pe)), "b": rng.lognormal(0.0, 1.0, (n_ev, n_pe))}
    inj_values = {"a": rng.normal(0.0, 1.0, n_inj), "b": rng.lognormal(0.0, 1.0, n_inj)}
    thetas = np.arange(k, dtype=np.float64)[:, None]
    out = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, backend="host", return_weights=True)
    assert out["names"] == ["a", "b"] and out["quantiles"].shape == (n_ev, 2, 3) and out["mean"].shape == out["sd"].shape == (n_ev, 2)
    assert out["quantiles_inj"].shape == (2, 3) and out["mean_inj"].shape == out["sd_inj"].shape == (2,)
    assert np.array_equal(out["dead"], [1, k, 0]) and out["dead_inj"] == 0 and out["n_points"] == k
    assert np.all(np.isnan(out["quantiles"][1])) and np.all(np.isnan(out["mean"][1])) and np.all(np.isnan(out["sd"][1]))
    W, Wi = out["weights"], out["weights_inj"]
    want = D.marginal_weights_reference(lw_pe, lw_inj, None, None)
    assert np.array_equal(W, want[0]) and np.array_equal(Wi, want[1]) and abs(W[0].sum() - (k - 1)) <= 1e-12 and abs(Wi.sum() - k) <= 1e-12
    for ev in (0, 2):
        for c, name in enumerate(("a", "b")):
            x = pe_values[name][ev]
            mean = (W[ev] * x).sum() / W[ev].sum()
            assert abs(out["mean"][ev, c] - mean) <= 1e-12 * np.abs(x).max()
            assert abs(out["sd"][ev, c] - np.sqrt((W[ev] * (x - mean) ** 2).sum() / W[ev].sum())) <= 1e-9 * np.abs(x).max()
            o = np.argsort(x, kind="stable")
            cdf = np.cumsum(W[ev][o]) / W[ev].sum()
            for q, p in enumerate((0.05, 0.5, 0.95)):  # the inverted CDF: the first value at which the weighted CDF reaches p
                assert out["quantiles"][ev, c, q] == x[o][np.searchsorted(cdf, p)]
            assert out["quantiles"][ev, c, 0] <= out["quantiles"][ev, c, 1] <= out["quantiles"][ev, c, 2]
    named = P.event_credible_intervals(eng, thetas, None, pedata=pe_values, injdata=inj_values, param_names=["b"], levels=[0.5], backend="host")
    assert named["names"] == ["b"] and np.array_equal(named["quantiles"][:, 0, 0], out["quantiles"][:, 1, 1], equal_nan=True)
    assert np.array_equal(named["quantiles_inj"][0, 0], out["quantiles_inj"][1, 1])
    only_pe = P.event_credible_intervals(eng, thetas, pe_values, backend="host")
    assert "quantiles_inj" not in only_pe and "weights" not in only_pe and np.array_equal(only_pe["quantiles"], out["quantiles"], equal_nan=True)
    with pytest.raises(ValueError, match="pe_values\\['a'\\] has shape"):
        P.event_credible_intervals(eng, thetas, {"a": np.zeros(3)}, backend="host")
    with pytest.raises(ValueError, match="inj_values\\['a'\\] has shape"):
        P.event_credible_intervals(eng, thetas, pe_values, inj_values={"a": np.zeros(3), "b": inj_values["b"]}, backend="host")
    with pytest.raises(ValueError, match="together or not at all"):
        P.event_credible_intervals(eng, thetas, pe_values, m1min=5.0, backend="host")
    with pytest.raises(ValueError, match="backend"):
        P.event_credible_intervals(eng, thetas, pe_values, backend="eager")
    with pytest.raises(ValueError, match="between 1 and 32 levels"):
        P.event_credible_intervals(eng, thetas, pe_values, levels=np.linspace(0, 1, 33), backend="host")
    with pytest.raises(ValueError, match="levels must lie"):
        P.event_credible_intervals(eng, thetas, pe_values, levels=[0.5, 1.5], backend="host")
    with pytest.raises(ValueError, match="between 1 and 8 quantities"):
        P.event_credible_intervals(eng, thetas, {str(i): pe_values["a"] for i in range(9)}, backend="host")
    with pytest.raises(ValueError, match="must be finite"):
        P.event_credible_intervals(eng, thetas, {"a": np.full((n_ev, n_pe), np.inf)}, backend="host")
    with pytest.raises(ValueError, match="no point"):
        P.event_credible_intervals(eng, np.zeros((0, 1)), pe_values, backend="host")
    with pytest.raises(ValueError, match="pedata and param_names"):
        P.event_credible_intervals(eng, thetas, None, backend="host")


@pytest.mark.parametrize("name", U.COMPS)
def test_inputs_of_the_gpu_tests(name):
    """CONDITION, not measurement.  Every case tests/test_gpu_quant.py compares (composition, mask case, column, level), from the
    host evaluation of the bound model: every column is finite and has ties where it is meant to (the rounded columns) and both
    signs where it is meant to; every segment meant to be live has at least 200 samples with weight; and no level other than 0 and
    1 has its target p C_last within quant_util.band of one of the statement's prefix values -- so the device's index must EQUAL the
    statement's wherever its weights agree with these to the derived bound, and the GPU test's allowance of 1 case in 100 is for the
    difference between the device's weights and the host's, not for this fixture."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import marginal_weights_reference, weighted_quantiles_reference

    vp, vi = QU.columns(8)
    op, oi = QU.orders(8)
    assert vp.shape == (8, U.N_EV, U.N_PE) and vi.shape == (8, U.N_INJ) and np.all(np.isfinite(vp)) and np.all(np.isfinite(vi))
    assert np.array_equal(QU.columns(1)[0][0], vp[0]) and np.array_equal(vp[1], vp[0] * vp[4])  # mass_2 = q m1
    assert all(np.unique(vp[2, ev]).size < U.N_PE // 10 for ev in range(U.N_EV)) and np.unique(vi[2]).size < U.N_INJ // 10  # many ties
    assert np.any(vp[3] < 0) and np.any(vp[3] > 0) and np.any(vi[3] < 0) and np.any(vi[3] > 0)                             # both signs
    comp = U.composition(name, device=N.DEVICE_HOST_ONLY)
    thetas = U.points(comp, name, QU.K)
    lw = [U.host_log_weights(comp.engine().bound, th) for th in thetas]
    lw_pe, lw_inj = np.stack([a for a, _ in lw]), np.stack([b for _, b in lw])
    checked, closest = 0, np.inf
    for case in U.MASK_CASES:
        pm, im = U.masks(case)
        W_pe, W_inj, dead, n_points = marginal_weights_reference(lw_pe, lw_inj, pm, im)
        assert n_points == QU.K and np.array_equal(dead, [0, QU.K if case == "masked" else 0, 0, 0])
        for seg in range(U.N_EV + 1):
            W = W_pe[seg] if seg < U.N_EV else W_inj
            live = int(np.count_nonzero(W > 0))
            if dead[seg]:
                assert live == 0
                continue
            assert live >= 200 and abs(W.sum() - QU.K) <= 1e-9
            for c in range(8):
                x, order = (vp[c, seg], op[c, seg]) if seg < U.N_EV else (vi[c], oi[c])
                prefix = np.cumsum(W[order].astype(np.longdouble))
                prefix = prefix[W[order] > 0]
                for levels in (QU.LEVELS, QU.LEVELS_32):
                    idx, _, mass = weighted_quantiles_reference(W, order, x, levels)
                    assert np.all(idx >= 0) and abs(mass - QU.K) <= 1e-9
                    live_x = x[W > 0]
                    assert x[idx[0]] == live_x.min() and x[idx[-1]] == live_x.max() and np.all(np.diff(x[idx]) >= 0)
                    for p in levels:
                        if p in (0.0, 1.0):
                            continue
                        near = float(np.min(np.abs(prefix - np.longdouble(p) * prefix[-1])) / prefix[-1])
                        closest = min(closest, near / QU.band(live))
                        assert near > QU.band(live), (name, case, seg, c, p, near, QU.band(live))
                        checked += 1
    print(f"{name}: {checked} (mask case, segment, column, level) targets; the closest lies {closest:.3g} bands from a prefix value")
    assert checked == (4 + 3) * 8 * (3 + 30)
