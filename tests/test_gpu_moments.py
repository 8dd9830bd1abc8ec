"""GPU: per-point moments on the device (include/gwi_engine.h: gwi_point_moments; gwinferno_amd/csrc/gwi_moment.h): the
statement (draws.point_moments_reference on the engine's own log-weights) under the derived bound of tests/moment_util.py, determinism
over calls, splits and handles, the absence of side effects on the existing entries, the law of total variance against
event_credible_intervals, and the refusals.

Shapes (tests/moment_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 500 injections (three tiles, the last ragged),
three points of a PL+Peak and of a B-spline model, 1, 3 and 8 columns, the first offset by 1e6.  The masked case removes one event, leaves
one sample of another and thins the third.  The inputs are vetted without a device in tests/test_moment_cpu.py."""
import ctypes as C
import os

import moment_util as MU
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """One engine per composition with its three points and their log-weights from the device: made once, shared."""
    if name not in _CASES:
        comp = MU.composition(name)
        eng = comp.engine()
        thetas = MU.points(comp, name)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas]
        for pair in lw:
            for a in pair:
                a.setflags(write=False)
        _CASES[name] = dict(comp=comp, eng=eng, thetas=thetas, lw=lw)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
    _CASES.clear()


def _same(a, b):
    """equal bits, NaN in the same places"""
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def _moments(eng, thetas, n_cols, case="free"):
    try:
        eng.set_draw_mask(*MU.masks(case))
        eng.set_kde_columns(*MU.columns(n_cols))
        return eng.point_moments(thetas)
    finally:
        eng.set_draw_mask()


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("n_cols", MU.N_COLS)
@pytest.mark.parametrize("name", MU.COMPS)
def test_against_the_statement(name, n_cols, case):
    """Every mean and every covariance entry of every point against point_moments_reference on eng.log_weights under the DERIVED bounds
    of moment_util.tolerances: a count of roundings times 2^-52 applied to sum w^ |x_c| and to sum w^ |x_c - m_c||x_d - m_d| (plus the
    second-order centring term written down there).  Flags and NaN positions agree exactly; the masked case's dead event gives NaN and
    dead = 1, its single-sample event the sample itself and a covariance of exactly 0; the covariance is symmetric.  The largest
    deviations are printed as fractions of the bound."""
    c = _case(name)
    pm, im = MU.masks(case)
    x_pe, x_inj = MU.columns(n_cols)
    mean, cov, dead = _moments(c["eng"], c["thetas"], n_cols, case)
    n_segs = MU.N_EV + 1
    assert mean.shape == (MU.N_POINTS, n_segs, n_cols) and cov.shape == (MU.N_POINTS, n_segs, n_cols, n_cols) and dead.shape == (MU.N_POINTS, n_segs) and dead.dtype == np.int32
    assert np.array_equal(cov, np.swapaxes(cov, 2, 3), equal_nan=True)
    worst_m = worst_v = 0.0
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want_m, want_v, want_dead, tol_m, tol_v = MU.statement_point(lw_pe, lw_inj, x_pe, x_inj, pm, im)
        assert np.array_equal(dead[k], want_dead) and np.array_equal(np.isnan(mean[k]), np.isnan(want_m)) and np.array_equal(np.isnan(cov[k]), np.isnan(want_v))
        assert np.array_equal(np.nonzero(dead[k])[0], [MU.DEAD_EVENT] if case == "masked" else [])
        live = [s for s in range(n_segs) if not want_dead[s]]
        assert len(live) == n_segs - (case == "masked") and np.all(tol_m[live] > 0.0) and np.all(tol_v[live] >= 0.0)
        dev_m, dev_v = np.abs(mean[k][live] - want_m[live]), np.abs(cov[k][live] - want_v[live])
        assert np.all(dev_m <= tol_m[live]), (k, float(np.max(dev_m / tol_m[live])))
        assert np.all(dev_v <= tol_v[live]), (k, float(np.max(dev_v - tol_v[live])))
        pos = tol_v[live] > 0.0
        worst_m, worst_v = max(worst_m, float(np.max(dev_m / tol_m[live]))), max(worst_v, float(np.max(dev_v[pos] / tol_v[live][pos])))
        if case == "masked":
            assert np.array_equal(mean[k, MU.SINGLE_EVENT], x_pe[:, MU.SINGLE_EVENT, MU.SINGLE_SAMPLE]) and np.array_equal(cov[k, MU.SINGLE_EVENT], np.zeros((n_cols, n_cols)))
    diag = np.arange(n_cols)
    assert np.all(cov[:, -1][:, diag, diag] > 0.0)
    print(f"{name}, C = {n_cols}, {case}: largest |device - statement| = {worst_m:.4f} (mean), {worst_v:.4f} (covariance) of the derived bound")


def test_bits_are_a_function_of_the_arguments():
    """K = 3 in one call, as 1 + 2 and as 1 + 1 + 1 concatenate to the same bits; the same call twice; one point given as (n_theta,); a call
    of K = 70 crosses the 64-point staging chunk; a second handle on the same catalog; the diagnostic reports six launches per point."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    whole = _moments(eng, thetas, 3, "masked")
    again = eng.point_moments(thetas)  # (the mask is off now: another input)
    assert not _same(whole, again) and _same(again, eng.point_moments(thetas)) and not np.any(np.isnan(again[0])) and not again[2].any()
    assert not np.array_equal(again[0][0], again[0][1])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_moment_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 18 and all(m.value > 0.0 for m in ms)
    whole = again
    for split in ((1, 2), (2, 1), (1, 1, 1)):
        parts, at = [], 0
        for n in split:
            parts.append(eng.point_moments(thetas[at : at + n]))
            at += n
        assert _same([np.concatenate([p[i] for p in parts]) for i in range(3)], whole), split
    single = eng.point_moments(thetas[1])
    assert single[0].shape == (1, MU.N_EV + 1, 3) and _same([s[0] for s in single], [w[1] for w in whole])
    out = eng.point_moments(np.tile(thetas, (24, 1))[:70])
    assert out[0].shape == (70, MU.N_EV + 1, 3) and out[2].shape == (70, MU.N_EV + 1)
    for k in range(70):
        assert _same([o[k] for o in out], [w[k % 3] for w in whole]), k
    eng2 = MU.composition("plpeak").engine()
    try:
        eng2.set_kde_columns(*MU.columns(3))
        assert _same(eng2.point_moments(thetas), whole)
        # one set alone: the other's segments come back NaN, its own with the same bits, the flags unchanged
        eng2.set_kde_columns(None, MU.columns(3)[1])
        only = eng2.point_moments(thetas)
        assert np.all(np.isnan(only[0][:, : MU.N_EV])) and np.all(np.isnan(only[1][:, : MU.N_EV])) and _same([o[:, -1] for o in only], [w[:, -1] for w in whole])
        eng2.set_kde_columns(MU.columns(3)[0], None)
        only = eng2.point_moments(thetas)
        assert np.all(np.isnan(only[0][:, -1])) and _same([o[:, : MU.N_EV] for o in only[:2]], [w[:, : MU.N_EV] for w in whole[:2]]) and np.array_equal(only[2], whole[2])
    finally:
        eng2.close()


def test_no_existing_entry_moves():
    """weighted_kde (on marginal weights added before and after), weighted_histograms split over two calls and point_cdfs on the same
    handle return the bits they return without the new entry when point_moments calls sit in between; point_moments itself repeats
    after all of them."""
    import cdf_util as CU

    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = MU.columns(3)
    eng.set_kde_columns(x_pe, x_inj)
    pe, inj, _ = MU.catalog()
    g = CU.grid(5)
    from gwinferno_amd.draws import cdf_codes

    pc = np.stack([cdf_codes(pe[n], g[i]) for i, n in enumerate(CU.COLUMNS)])
    ic = np.stack([cdf_codes(inj[n], g[i]) for i, n in enumerate(CU.COLUMNS)])
    eng.set_histogram_bins(pc, ic, n_bins=5)
    grid = np.stack([np.linspace(x_inj[i].min(), x_inj[i].max(), 7) for i in range(3)])

    def run(interleave):
        between = (lambda: eng.point_moments(thetas)) if interleave else (lambda: None)
        eng.marginal_weights_reset()
        eng.marginal_weights_add(thetas[:2])
        between()
        eng.marginal_weights_add(thetas[2:])
        between()
        kde = eng.weighted_kde(grid)
        hist = eng.weighted_histograms(thetas[:2])
        between()
        hist = eng.weighted_histograms(thetas[2:], out=hist)
        between()
        return tuple(a for a in kde) + tuple(hist) + tuple(eng.point_cdfs(thetas))

    plain = run(False)
    moments = eng.point_moments(thetas)
    assert _same(run(True), plain) and _same(eng.point_moments(thetas), moments)


def test_total_variance_against_the_credible_intervals():
    """The law of total variance against the marginal-weight moments: event_variance_split(...)["total"] equals the square of
    event_credible_intervals' standard deviation on the same points, within the two entries' stated bounds.  The interval entry forms
    E[x^2] - E[x]^2 from sums that are each within r = quant_util.weight_bound + 2 quant_util.moment_bound (relative, of the sums of
    absolute terms), so its variance is within 1.01 r (E[x^2] + 2 E|x|^2); the split's total moves by at most the weighted mean of
    tol_cov plus 4 tol_mean (|m_k - mbar| + tol_mean) for the between part, and (K + 4) 2^-52 of within + between for the host's own
    sums.  For the offset column the first bound is of order 1 (the one-pass formula has lost the variance: test_moment_cpu says so) and
    the comparison says nothing; for the other two columns it is below 1e-10 of the variance and does."""
    import quant_util as QU
    from gwinferno_amd import postprocess as P

    c = _case("plpeak")
    eng, thetas, k = c["eng"], c["thetas"], MU.N_POINTS
    pe_values, _ = MU.values(3)
    x_pe = MU.columns(3)[0]
    split = P.event_variance_split(eng, thetas, pe_values)
    eci = P.event_credible_intervals(eng, thetas, pe_values)
    host = P.event_variance_split(eng, thetas, pe_values, backend="host")
    assert np.array_equal(split["within"] + split["between"], split["total"]) and not split["n_dead"].any() and np.allclose(split["neff_points"], k)
    assert np.all(split["between"] > 0.0) and np.all(split["fraction_between"] > 0.0) and np.all(split["fraction_between"] < 1.0)
    r = QU.weight_bound(MU.N_PE, k) + 2.0 * QU.moment_bound(MU.N_PE)
    W = eci_w = P.event_credible_intervals(eng, thetas, pe_values, return_weights=True)["weights"]
    share = W / W.sum(axis=1, keepdims=True)
    e_abs, e_sq = np.einsum("ep,cep->ec", share, np.abs(x_pe)), np.einsum("ep,cep->ec", share, x_pe * x_pe)
    tol_eci = 1.01 * r * (e_sq + 2.0 * e_abs * e_abs)
    tol_m, tol_v = np.empty((k, MU.N_EV, 3)), np.empty((k, MU.N_EV, 3))
    for i, (lw_pe, lw_inj) in enumerate(c["lw"]):
        _, _, _, tm, tv = MU.statement_point(lw_pe, lw_inj, x_pe, None, None, None)
        tol_m[i], tol_v[i] = tm[: MU.N_EV], tv[: MU.N_EV][:, np.arange(3), np.arange(3)]
    spread = np.abs(split["point_mean"][:, : MU.N_EV] - split["mean"][None])
    tol_split = tol_v.mean(axis=0) + (4.0 * tol_m * (spread + tol_m)).mean(axis=0) + (k + 4) * MU.U * split["total"]
    dev = np.abs(split["total"] - eci["sd"] ** 2)
    print("largest |total - sd^2| as a fraction of the two bounds, per column:", np.max(dev / (tol_eci + tol_split), axis=0))
    assert np.all(dev <= tol_eci + tol_split) and np.all((tol_eci + tol_split)[:, 1:] < 1e-10 * split["total"][:, 1:])
    assert eci_w.shape == (MU.N_EV, MU.N_PE) and np.all(np.abs(split["total"] - host["total"]) <= 2.0 * tol_split)


def test_catalog_correlation_check_device_against_host():
    """postprocess.catalog_correlation_check on both backends: the raw arrays agree within the derived bounds of the first test, the
    flags exactly, and the correlations -- smooth functions of them with variances far above the bounds -- to 1e-9."""
    from gwinferno_amd import postprocess as P

    c = _case("bspline_iid")
    pe_values, inj_values = MU.values(3)
    dev = P.catalog_correlation_check(c["eng"], c["thetas"], pe_values, inj_values=inj_values)
    host = P.catalog_correlation_check(c["eng"], c["thetas"], pe_values, inj_values=inj_values, backend="host")
    assert np.array_equal(dev["dead"], host["dead"]) and np.array_equal(dev["n_live"], host["n_live"]) and not dev["degenerate_obs"].any() and not dev["degenerate_det"].any()
    for key in ("rho_obs", "rho_det", "delta"):
        assert np.all(np.isfinite(dev[key])) and np.all(np.abs(dev[key] - host[key]) <= 1e-9), key
    assert np.allclose(dev["point_cov"], host["point_cov"], rtol=1e-9, atol=1e-12) and np.allclose(dev["point_mean"], host["point_mean"], rtol=1e-12, atol=0.0)


def test_refusals():
    """On a fresh handle: a call before set_kde_columns, then null thetas, k = 0, k < 0, null out and null dead through raw ctypes each
    answer GWI_ERR_INVALID with a message and write nothing; afterwards the handle gives the shared engine's bits.  A shard is refused
    from Python, and from the library itself on a world-2 shared-memory handle."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    c = _case("plpeak")
    thetas = c["thetas"]
    c["eng"].set_kde_columns(*MU.columns(3))
    free = c["eng"].point_moments(thetas)
    comp = MU.composition("plpeak")
    eng = comp.engine()
    try:
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no columns are set"):
            eng.point_moments(thetas[0])
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th, out, dead = N.f64(thetas[0]), np.full((1, MU.N_EV + 1, 9), 7.0), np.full((1, MU.N_EV + 1), 7, dtype=np.int32)
        full = (N.as_dp(th), 1, N.as_dp(out), dead.ctypes.data_as(i32))
        assert lib.gwi_point_moments(eng.handle, *full) == -1
        assert "gwi_point_moments: no columns are set (gwi_set_kde_columns)" in lib.gwi_last_error(eng.handle).decode()
        eng.set_kde_columns(*MU.columns(3))
        for args, word in (((None,) + full[1:], "thetas"), ((full[0], 0) + full[2:], "k < 1"), ((full[0], -1) + full[2:], "k < 1"),
                           (full[:2] + (None,) + full[3:], "out is null"), (full[:3] + (None,), "dead is null")):
            assert lib.gwi_point_moments(eng.handle, *args) == -1
            message = lib.gwi_last_error(eng.handle).decode()
            assert message.startswith("gwi_point_moments: ") and word in message, (word, message)
        assert np.all(out == 7.0) and np.all(dead == 7)
        assert _same(eng.point_moments(thetas), free)  # a second handle; the refused calls left nothing behind
        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_moments: this engine holds one shard of the catalog"):
            shards[0].point_moments(thetas[0])
        seg = f"/gwi_moment_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            assert lib.gwi_point_moments(hs, *full) == -4  # GWI_ERR_UNSUPPORTED
            assert "gwi_point_moments: this handle holds one shard of the catalog; the injection moments need the global set" in lib.gwi_last_error(hs).decode()
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        assert _same(eng.point_moments(thetas), free)
    finally:
        eng.close()
