"""GPU: linear weights per (point, segment) in the device sums and the leave-one-out event posteriors made of them
(include/gwi_engine.h: gwi_marginal_weights_add_weighted, gwi_marginal_point_weights, gwi_weighted_histograms_weighted;
gwinferno_amd/csrc/gwi_quant.h, gwi_hist.h): weights of 1 against the entries without weights, to the bit; the kernels
against the NumPy statement; the split of a request and two handles; a dead segment; the leave-one-out identity against engines on
the catalogs without one event; the three user-facing functions, device against host; the refusals.

Shapes (tests/loo_util.py): 3 events x 1 500 PE samples (a full tile and a ragged one), 2 500 injections (three tiles, the last
ragged), K = 5 points, 2 columns, 7 bins, a PL+Peak and a B-spline model.  The inputs are vetted without a device in
tests/test_loo_cpu.py: test_inputs_of_the_gpu_tests."""
import ctypes as C
import os

import hist_util as U
import kde_util as KU
import loo_util as LU
import numpy as np
import pytest
import quant_util as QU

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """One engine per composition with its five points and their log-weights from the device: made once, shared, never changed."""
    if name not in _CASES:
        comp = LU.composition(name)
        eng = comp.engine()
        thetas = LU.points(comp, name)
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


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True))
                                    or (isinstance(x, int) and x == y) for x, y in zip(a, b))


def _accumulate(eng, thetas, v=None, masks=(None, None), split=None):
    """(W_pe, W_inj, dead, n_points, vsum, vsum2) after a reset and the points, in calls of the sizes of ``split``."""
    try:
        eng.set_draw_mask(*masks)
        eng.marginal_weights_reset()
        at = 0
        for n in split or (len(thetas),):
            eng.marginal_weights_add(thetas[at : at + n], **({} if v is None else {"point_weights": v[at : at + n]}))
            at += n
    finally:
        eng.set_draw_mask()
    return (*eng.marginal_weights(), *eng.marginal_point_weights())


def _histograms(eng, thetas, v=None, masks=(None, None), split=None):
    try:
        eng.set_draw_mask(*masks)
        out, at = None, 0
        for n in split or (len(thetas),):
            out = eng.weighted_histograms(thetas[at : at + n], out=out, **({} if v is None else {"point_weights": v[at : at + n]}))
            at += n
    finally:
        eng.set_draw_mask()
    return out


def _setup(eng):
    pb, ib = LU.bins()
    eng.set_histogram_bins(pb, ib, n_bins=LU.N_BINS)
    eng.set_quantile_columns(*LU.columns())


@pytest.mark.parametrize("name", LU.COMPS)
def test_weights_of_one_give_the_unweighted_bits(name):
    """point_weights = 1, as (K, n_ev + 1) and as (K,): W, dead, n_points, the quantile indices, the moments, the mass and the
    histograms are those of the entries without weights, bit for bit; vsum = vsum2 = n_points - dead, also after unweighted adds and
    after a mix of both."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    _setup(eng)
    plain = _accumulate(eng, thetas)
    q_plain = eng.weighted_quantiles(LU.LEVELS)
    h_plain = _histograms(eng, thetas)
    assert plain[3] == LU.K and np.array_equal(plain[4], LU.K - plain[2]) and np.array_equal(plain[5], plain[4]) and len(h_plain) == 3
    for ones in (np.ones((LU.K, LU.N_EV + 1)), np.ones(LU.K)):
        got = _accumulate(eng, thetas, ones)
        assert _same(plain, got) and _same(q_plain, eng.weighted_quantiles(LU.LEVELS))
        h = _histograms(eng, thetas, ones)
        assert len(h) == 4 and _same(h_plain, h[:3]) and np.array_equal(h[3], LU.K - h_plain[2])
    eng.marginal_weights_reset()
    eng.marginal_weights_add(thetas[:2])
    eng.marginal_weights_add(thetas[2:], point_weights=np.ones(3))
    assert _same(plain, (*eng.marginal_weights(), *eng.marginal_point_weights()))
    eng.marginal_weights_reset()
    assert not any(a.any() for a in eng.marginal_point_weights())


@pytest.mark.parametrize("masked", (False, True), ids=("free", "masked"))
@pytest.mark.parametrize("name", LU.COMPS)
def test_kernels_against_statement(name, masked):
    """v in [2^-20, 1] with exact zeros: W and H against the statements on eng.log_weights of the same points under the derived
    bounds of one more rounding than without weights (loo_util.weight_bound, hist_bound); a sample or bin the statement leaves at 0
    is 0; dead and n_points equal; vsum and vsum2 to (K + 2) 2^-52 relative."""
    from gwinferno_amd.draws import marginal_weights_reference, weighted_histograms_reference

    c = _case(name)
    eng, thetas, (lw_pe, lw_inj) = c["eng"], c["thetas"], c["lw"]
    _setup(eng)
    v = LU.point_weights()
    pm, im = U_masks(masked)
    pb, ib = LU.bins()
    got = _accumulate(eng, thetas, v, (pm, im))
    want = marginal_weights_reference(lw_pe, lw_inj, pm, im, v=v)
    hist = _histograms(eng, thetas, v, (pm, im))
    h_want = None
    for p in range(LU.K):
        one = weighted_histograms_reference(lw_pe[p], lw_inj[p], pm, im, pb, ib, LU.N_BINS, v=v[p])
        h_want = list(one) if h_want is None else [a + b for a, b in zip(h_want, one)]
    assert got[3] == want[3] == LU.K and np.array_equal(got[2], want[2]) and np.array_equal(hist[2], h_want[2]) and np.array_equal(hist[2], got[2])
    zeros = (v == 0.0).sum(axis=0)
    assert np.array_equal(got[2] == 0, [not (masked and seg == LU.DEAD_EVENT) for seg in range(LU.N_EV + 1)])
    if masked:  # the dead event: every point but the one of weight 0 is counted
        assert got[2][LU.DEAD_EVENT] == LU.K - zeros[LU.DEAD_EVENT] == LU.K - 1 and got[4][LU.DEAD_EVENT] == 0.0 and hist[3][LU.DEAD_EVENT] == 0.0
    worst_w = worst_h = 0.0
    for seg in range(LU.N_EV + 1):
        mask = None if pm is None else (pm[seg] if seg < LU.N_EV else im)
        live = max(U.n_live(lw_pe[p, seg] if seg < LU.N_EV else lw_inj[p], mask) for p in range(LU.K))
        for what, g, w, tol in (("W", got[0][seg] if seg < LU.N_EV else got[1], want[0][seg] if seg < LU.N_EV else want[1], LU.weight_bound(live)),
                                ("H", hist[0][seg] if seg < LU.N_EV else hist[1], h_want[0][seg] if seg < LU.N_EV else h_want[1], LU.hist_bound(live))):
            assert np.all(np.isfinite(g)) and np.array_equal(g == 0.0, w == 0.0), (name, masked, what, seg)
            dev = np.abs(g - w)
            ratio = float(np.max(dev[w > 0] / w[w > 0])) / tol if np.any(w > 0) else 0.0
            print(f"{name} masked={masked} segment {seg}: largest |device - statement| / statement of {what} = {ratio:.3f} of the derived bound {tol:.3e}")
            assert np.all(dev <= tol * w), (name, masked, what, seg, ratio)
            worst_w, worst_h = (max(worst_w, ratio), worst_h) if what == "W" else (worst_w, max(worst_h, ratio))
    for what, g, w in (("vsum", got[4], want[4]), ("vsum2", got[5], want[5]), ("vsum of the histograms", hist[3], h_want[3])):
        print(f"{name} masked={masked} {what}: device {g!r} statement {w!r}")
        assert np.all(np.abs(g - w) <= LU.vsum_bound() * w), (name, masked, what)
    print(f"{name} masked={masked}: worst W {worst_w:.3f}, worst H {worst_h:.3f} of their bounds")


def U_masks(masked):
    return LU.dead_mask() if masked else (None, None)


@pytest.mark.parametrize("name", LU.COMPS)
def test_split_invariance_and_two_handles(name):
    """One call of 5 points, calls of 2 + 3 and five calls of 1: identical bits of W, dead, n_points, vsum, vsum2, the quantiles and
    H (through the in/out convention); a second handle of the same model gives the same bits."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    _setup(eng)
    v = LU.point_weights()
    whole = _accumulate(eng, thetas, v)
    q_whole = eng.weighted_quantiles(LU.LEVELS)
    h_whole = _histograms(eng, thetas, v)
    assert whole[0].any() and whole[4].all() and h_whole[0].any()
    for split in ((2, 3), (1, 1, 1, 1, 1)):
        assert _same(whole, _accumulate(eng, thetas, v, split=split)), split
        assert _same(q_whole, eng.weighted_quantiles(LU.LEVELS)), split
        assert _same(h_whole, _histograms(eng, thetas, v, split=split)), split
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_histogram_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 4 and all(m.value > 0.0 for m in ms)  # the last weighted call: one point, four launches
    eng.marginal_weights_reset()
    eng.marginal_weights_add(thetas, point_weights=v)
    eng.lib.gwi_quantile_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 3 * LU.K and ms[0].value > 0.0 and ms[1].value > 0.0
    eng2 = LU.composition(name).engine()
    try:
        _setup(eng2)
        assert _same(whole, _accumulate(eng2, thetas, v)) and _same(q_whole, eng2.weighted_quantiles(LU.LEVELS)) and _same(h_whole, _histograms(eng2, thetas, v))
    finally:
        eng2.close()


@pytest.mark.parametrize("name", LU.COMPS)
def test_dead_segment(name):
    """Every sample of one event masked: dead counts the points (not the one of weight 0), vsum of the event stays 0, its quantiles
    and densities are NaN, and the other events and the injection set are those of the run without the mask, bit for bit."""
    from gwinferno_amd import postprocess as P

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    _setup(eng)
    v, d = LU.point_weights(), LU.DEAD_EVENT
    free, h_free = _accumulate(eng, thetas, v), _histograms(eng, thetas, v)
    q_free = eng.weighted_quantiles(LU.LEVELS)
    got, h = _accumulate(eng, thetas, v, LU.dead_mask()), _histograms(eng, thetas, v, LU.dead_mask())
    q = eng.weighted_quantiles(LU.LEVELS)
    want_dead = np.zeros(LU.N_EV + 1, dtype=np.int32)
    want_dead[d] = LU.K - 1  # (the event's weight is 0 at one point)
    assert np.array_equal(got[2], want_dead) and np.array_equal(h[2], want_dead) and got[3] == LU.K
    assert got[4][d] == 0.0 and got[5][d] == 0.0 and h[3][d] == 0.0 and not got[0][d].any() and not h[0][d].any()
    assert np.all(q[0][d] == -1) and q[4][d] == 0.0
    others = [e for e in range(LU.N_EV) if e != d]
    assert np.array_equal(got[0][others], free[0][others]) and np.array_equal(got[1], free[1]) and np.array_equal(h[0][others], h_free[0][others]) and np.array_equal(h[1], h_free[1])
    for i in (4, 5):
        assert np.array_equal(np.delete(got[i], d), np.delete(free[i], d))
    assert np.array_equal(np.delete(h[3], d), np.delete(h_free[3], d))
    assert np.array_equal(q[0][others], q_free[0][others]) and np.array_equal(q[2][others], q_free[2][others]) and np.array_equal(q[1], q_free[1])
    # the user-facing functions on the weights the masked accumulation left, and with the mask as mass cuts of their own
    pe, inj, _ = LU.catalog()
    pe_values, inj_values = {k: pe[k] for k in LU.COLUMNS}, {k: inj[k] for k in LU.COLUMNS}
    dens = P.event_posterior_densities(eng, thetas, pe_values, np.linspace(0.0, 1.0, 16), inj_values=inj_values, accumulate=False)
    assert np.all(np.isnan(dens["density"][d])) and np.all(np.isfinite(dens["density"][others])) and dens["dead"][d] == LU.K - 1
    try:
        eng.set_draw_mask(*LU.dead_mask())
        table = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, point_weights=v)
    finally:
        eng.set_draw_mask()
    assert np.all(np.isnan(table["quantiles"][d])) and np.all(np.isnan(table["mean"][d])) and np.all(np.isfinite(table["quantiles"][others]))
    assert np.array_equal(table["point_weight_sum"], got[4]) and table["dead"][d] == LU.K - 1


@pytest.mark.parametrize("marginalize", (False, True), ids=("plain", "marginalized selection"))
@pytest.mark.parametrize("name", LU.COMPS)
def test_leave_one_out_identity(name, marginalize):
    """For every event e an engine on the catalog without e: log v_ke - (log L_{-e}(theta_k) - log L(theta_k)) is the same constant
    for all k, within 1e-9 max_k |log L| (the project's parity bound on a likelihood value); nobs = N - 1 there, no cuts."""
    from gwinferno_amd import postprocess as P

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    total = LU.catalog()[2]
    loo = P.leave_one_out_weights(eng, thetas, total, marginalize_selection=marginalize)
    v = loo["point_weights"]
    assert v.shape == (LU.K, LU.N_EV + 1) and np.all(v[:, LU.N_EV] == 1.0) and np.all(v[:, : LU.N_EV].max(axis=0) == 1.0) and np.all(v > 0.0) and not loo["n_bad"].any()
    kw = dict(marginalize_selection=marginalize, min_neff_cut=False, max_variance_cut=False, want_grad=False)
    log_l = np.array([r.log_likelihood for r in eng.evaluate_batch(thetas, total, **kw)])
    tol = 1e-9 * float(np.max(np.abs(log_l)))
    for e in range(LU.N_EV):
        part = LU.composition(name, without=e).engine()
        try:
            assert part.n_ev == LU.N_EV - 1 and part.n_theta == eng.n_theta
            log_l_part = np.array([r.log_likelihood for r in part.evaluate_batch(thetas, total, nobs=LU.N_EV - 1, **kw)])
        finally:
            part.close()
        const = np.log(v[:, e]) - (log_l_part - log_l)
        print(f"{name} marginalize={marginalize} event {e}: log v - (log L_-e - log L) = {const!r}; spread {np.ptp(const):.3e}, bound {tol:.3e}")
        assert np.all(np.isfinite(const)) and np.ptp(const) <= tol, (name, marginalize, e, float(np.ptp(const)), tol)
        assert np.allclose(loo["log_l_event"][:, e], log_l - log_l_part, rtol=0.0, atol=tol)
    assert np.all(loo["elpd_loo"] <= loo["lpd"] + 1e-12 * np.abs(loo["lpd"])) and np.all(loo["neff_points"] >= 1.0) and np.all(loo["neff_points"] <= LU.K + 1e-9)


@pytest.mark.parametrize("name", LU.COMPS)
def test_postprocess_leave_one_out_device_against_host(name):
    """The three user-facing functions with leave_one_out=True, backend="device" against backend="host", compared as
    tests/test_gpu_quant.py, test_gpu_hist.py and test_gpu_kde.py compare their backends; elpd_loo and neff_points are identical
    (the same evaluate_batch), point_weight_sum to the summation bound; the defaults are untouched by the new keywords."""
    from gwinferno_amd import postprocess as P

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    pe, inj, total = LU.catalog()
    names = list(LU.COLUMNS)
    pe_values, inj_values = {k: pe[k] for k in names}, {k: inj[k] for k in names}
    loo = P.leave_one_out_weights(eng, thetas, total)
    kw = dict(inj_values=inj_values, leave_one_out=True, total_inj=total)

    def shared(dev, host):
        assert np.array_equal(dev["elpd_loo"], loo["elpd_loo"]) and np.array_equal(host["elpd_loo"], loo["elpd_loo"])
        assert np.array_equal(dev["neff_points"], loo["neff_points"]) and np.array_equal(host["neff_points"], loo["neff_points"])
        want = loo["point_weights"].sum(axis=0)
        for got in (dev["point_weight_sum"], host["point_weight_sum"]):
            assert got.shape == (LU.N_EV + 1,) and np.all(np.abs(got - want) <= LU.vsum_bound() * want) and got[LU.N_EV] == LU.K

    # credible intervals (tests/test_gpu_quant.py: test_event_credible_intervals)
    dev = P.event_credible_intervals(eng, thetas, pe_values, return_weights=True, **kw)
    host = P.event_credible_intervals(eng, thetas, pe_values, backend="host", return_weights=True, **kw)
    shared(dev, host)
    assert dev["n_points"] == host["n_points"] == LU.K and np.array_equal(dev["dead"], host["dead"]) and not dev["dead"].any()
    assert np.array_equal(dev["quantiles"], host["quantiles"]) and np.array_equal(dev["quantiles_inj"], host["quantiles_inj"])
    for k in ("mean", "sd", "mean_inj", "sd_inj", "weights", "weights_inj"):
        assert np.allclose(dev[k], host[k], rtol=1e-9, atol=1e-300), k
    plain = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, return_weights=True)
    assert "elpd_loo" not in plain and "point_weight_sum" not in plain and not np.array_equal(plain["weights"], dev["weights"])
    assert np.array_equal(plain["weights_inj"], dev["weights_inj"])  # the injection set has no event of its own: its weights are 1
    given = P.event_credible_intervals(eng, thetas, pe_values, inj_values=inj_values, return_weights=True, point_weights=loo["point_weights"])
    assert np.array_equal(given["weights"], dev["weights"]) and np.array_equal(given["quantiles"], dev["quantiles"]) and "elpd_loo" not in given
    # densities (tests/test_gpu_kde.py: test_event_posterior_densities)
    grid = {"mass_1": np.linspace(3.0, 90.0, 64), "mass_ratio": np.linspace(-0.1, 1.1, 64)}
    dkw = dict(pairs=[("mass_1", "mass_ratio")], grid2d=(np.linspace(5.0, 80.0, 12), np.linspace(0.1, 1.0, 9)), bounds={"mass_ratio": (0.0, 1.0)})
    dev = P.event_posterior_densities(eng, thetas, pe_values, grid, **dkw, **kw)
    host = P.event_posterior_densities(eng, thetas, pe_values, grid, backend="host", **dkw, **kw)
    shared(dev, host)
    W_pe, W_inj, _, n_points = eng.marginal_weights()
    assert np.array_equal(W_pe, given["weights"]) and dev["n_points"] == n_points == LU.K and not dev["dead"].any() and not dev["degenerate"].any() and not dev["degenerate2d"].any()
    assert np.allclose(dev["bandwidth"], host["bandwidth"], rtol=1e-12, atol=0) and np.allclose(dev["neff"], host["neff"], rtol=1e-12, atol=0)
    assert np.allclose(dev["covariance"], host["covariance"], rtol=1e-12, atol=0) and np.allclose(dev["covariance_inj"], host["covariance_inj"], rtol=1e-12, atol=0)
    for seg in range(LU.N_EV + 1):
        W = W_pe[seg] if seg < LU.N_EV else W_inj
        for k, p in enumerate(names):
            x, got, want, h = (pe[p][seg], dev["density"][seg, k], host["density"][seg, k], host["bandwidth"][seg, k]) if seg < LU.N_EV else (
                inj[p], dev["density_inj"][k], host["density_inj"][k], host["bandwidth_inj"][k])
            KU.compare(got, want, KU.bound_1d(W, x, grid[p], h, dkw["bounds"].get(p)), ("densities", seg, p))
        x, y, got, want, H = (pe[names[0]][seg], pe[names[1]][seg], dev["density2d"][seg, 0], host["density2d"][seg, 0], host["covariance"][seg, 0]) if seg < LU.N_EV else (
            inj[names[0]], inj[names[1]], dev["density2d_inj"][0], host["density2d_inj"][0], host["covariance_inj"][0])
        KU.compare(got, want, KU.bound_2d(W, x, y, dkw["grid2d"][0], dkw["grid2d"][1], H), ("densities 2-D", seg))
    reused = P.event_posterior_densities(eng, thetas, pe_values, grid, inj_values=inj_values, accumulate=False, **dkw)
    assert np.array_equal(reused["density"], dev["density"]) and "elpd_loo" not in reused  # whatever W is there
    # binned densities (tests/test_gpu_hist.py: test_determinism)
    e = LU.edges()
    r1 = P.reweighted_event_posteriors(eng, thetas, pe_values, e, chunk=1, **kw)
    r64 = P.reweighted_event_posteriors(eng, thetas, pe_values, e, chunk=64, **kw)
    host = P.reweighted_event_posteriors(eng, thetas, pe_values, e, backend="host", **kw)
    shared(r64, host)
    assert np.array_equal(r1["point_weight_sum"], r64["point_weight_sum"])
    pb, ib = LU.bins()
    eng.set_histogram_bins(pb, ib, n_bins=LU.N_BINS)
    whole = eng.weighted_histograms(thetas, point_weights=loo["point_weights"])
    assert np.array_equal(whole[3], r64["point_weight_sum"])
    for i, k in enumerate(names):
        assert np.array_equal(r1[k]["events"], r64[k]["events"]) and np.array_equal(r1[k]["predicted"], r64[k]["predicted"])
        assert np.array_equal(r64[k]["events"], whole[0][:, i] / whole[3][: LU.N_EV, None] / np.diff(e[k])) and np.array_equal(r64[k]["n_points"]["events"], [LU.K] * LU.N_EV)
        assert np.allclose(r64[k]["events"], host[k]["events"], rtol=1e-12, atol=0.0) and np.allclose(r64[k]["predicted"], host[k]["predicted"], rtol=1e-12, atol=0.0)
        assert np.all(np.abs((r64[k]["events"] * np.diff(e[k])).sum(axis=1) - (1.0 - r64[k]["outside"]["events"])) <= 1e-15)
    plain = P.reweighted_event_posteriors(eng, thetas, pe_values, e, inj_values=inj_values)
    assert "elpd_loo" not in plain and not np.array_equal(plain[names[0]]["events"], r64[names[0]]["events"])


def test_refusals():
    """Every refusal of the new entries with its status and message and without a launch: a NaN, a negative and an above-1 entry of
    v, a null v, k < 0, null outputs, a sharded handle (GWI_ERR_UNSUPPORTED); the handle keeps working afterwards, with the bits of
    the shared engine."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    comp = LU.composition("plpeak")
    eng = comp.engine()
    try:
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        thetas = N.f64(LU.points(comp, "plpeak", 2))
        err = lambda: lib.gwi_last_error(eng.handle).decode()  # noqa: E731
        pb, ib = LU.bins()
        eng.set_histogram_bins(pb, ib, n_bins=LU.N_BINS)
        hp, hi, dead, vsum = np.zeros((LU.N_EV, 2, LU.N_BINS)), np.zeros((2, LU.N_BINS)), np.zeros(LU.N_EV + 1, dtype=np.int32), np.zeros(LU.N_EV + 1)
        add = lambda k, v: lib.gwi_marginal_weights_add_weighted(eng.handle, N.as_dp(thetas), k, N.as_dp(v))  # noqa: E731
        hist = lambda k, v, vs=vsum: lib.gwi_weighted_histograms_weighted(eng.handle, N.as_dp(thetas), k, N.as_dp(v), N.as_dp(hp), N.as_dp(hi), dead.ctypes.data_as(i32), N.as_dp(vs))  # noqa: E731
        ones = np.ones((2, LU.N_EV + 1))
        for wrong in (np.nan, -0.25, 1.5, np.inf):
            v = ones.copy()
            v[1, 2] = wrong
            assert add(2, v) == -1 and "point 1, segment 2" in err() and "not in [0, 1]" in err()
            assert hist(2, v) == -1 and "point 1, segment 2" in err() and "not in [0, 1]" in err()
        assert add(2, None) == -1 and "v is null" in err() and hist(2, None) == -1 and "v is null" in err()
        assert add(-1, ones) == -1 and "k < 0" in err() and hist(-1, ones) == -1 and "k < 0" in err()
        assert hist(2, ones, None) == -1 and "vsum is null" in err()
        assert lib.gwi_marginal_weights_add_weighted(eng.handle, None, 2, N.as_dp(ones)) == -1 and "thetas is null" in err()
        assert lib.gwi_marginal_point_weights(eng.handle, None, N.as_dp(vsum)) == -1 and "vsum or vsum2 is null" in err()
        assert lib.gwi_marginal_weights_add_weighted(None, None, 1, None) == -1 and lib.gwi_marginal_point_weights(None, None, None) == -1
        assert lib.gwi_weighted_histograms_weighted(None, None, 1, None, None, None, None, None) == -1
        # none of it launched or changed the state
        assert not hp.any() and not hi.any() and not dead.any() and not vsum.any() and eng.marginal_weights()[3] == 0 and not eng.marginal_point_weights()[0].any()
        for bad in (np.ones(3), np.ones((2, LU.N_EV)), np.array([0.5, 1.5])):
            with pytest.raises(ValueError):
                eng.marginal_weights_add(thetas, point_weights=bad)
            with pytest.raises(ValueError):
                eng.weighted_histograms(thetas, point_weights=bad)
        with pytest.raises(ValueError, match="out is"):
            eng.weighted_histograms(thetas, out=(hp, hi, dead), point_weights=ones)
        # a handle that holds a shard: GWI_ERR_UNSUPPORTED from Python and from the library itself
        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
            shards[0].marginal_weights_add(thetas, point_weights=np.ones(2))
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
            shards[0].marginal_point_weights()
        seg = f"/gwi_loo_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs, n_seg = shards[0].handle, shards[0].n_ev + 1
            sv, sdead, svs = np.ones((2, n_seg)), np.zeros(n_seg, dtype=np.int32), np.zeros(n_seg)
            shp, shi = np.zeros((shards[0].n_ev, 2, LU.N_BINS)), np.zeros((2, LU.N_BINS))
            for st in (lib.gwi_marginal_weights_add_weighted(hs, N.as_dp(thetas), 2, N.as_dp(sv)), lib.gwi_marginal_point_weights(hs, N.as_dp(svs), N.as_dp(svs.copy())),
                       lib.gwi_weighted_histograms_weighted(hs, N.as_dp(thetas), 2, N.as_dp(sv), N.as_dp(shp), N.as_dp(shi), sdead.ctypes.data_as(i32), N.as_dp(svs))):
                assert st == -4 and "this handle holds one shard of the catalog" in lib.gwi_last_error(hs).decode()  # GWI_ERR_UNSUPPORTED
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        # usable after all of it, with the bits of the shared engine
        v = LU.point_weights()[:2]
        ref = _case("plpeak")["eng"]
        ref.set_histogram_bins(pb, ib, n_bins=LU.N_BINS)
        assert _same(_accumulate(eng, thetas, v), _accumulate(ref, thetas, v)) and _same(_histograms(eng, thetas, v), _histograms(ref, thetas, v))
    finally:
        eng.close()
