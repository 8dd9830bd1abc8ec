"""GPU: weighted histograms on the device (include/gwi_engine.h: gwi_weighted_histograms; gwinferno_amd/csrc/gwi_hist.h) against
their NumPy statement (gwinferno_amd/draws.py: weighted_histograms_reference) fed with the engine's own log-weights, their
determinism across calls and across the split of a request, masks / dead segments / outside samples, the limits, and their meaning:
the histogram of many index draws of gwi_draw_indices.

Shapes (tests/hist_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 600 injections (three tiles), two columns,
7 and 256 bins, a PL+Peak and a B-spline model.  The inputs are vetted without a device in tests/test_hist_cpu.py:
test_inputs_of_the_gpu_tests -- no bin and no segment is left out of any comparison here."""
import ctypes as C

import hist_util as U
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """One engine per composition with its three points and their log-weights from the device: made once, shared, never changed."""
    if name not in _CASES:
        comp = U.composition(name)
        eng = comp.engine()
        thetas = U.points(comp, name, 3)
        thetas.setflags(write=False)
        lw = eng.log_weights(thetas[0])
        for a in lw:
            a.setflags(write=False)
        _CASES[name] = dict(comp=comp, eng=eng, thetas=thetas, lw=lw)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
    _CASES.clear()


def _compare(got, want, lw_pe, lw_inj, pm, im, what):
    """Every bin of every segment under the segment's derived bound; returns the largest deviation in units of the bound."""
    worst = 0.0
    hp, hi, dead = got
    wp, wi, wdead = want
    assert np.array_equal(dead, wdead), (what, dead, wdead)
    for seg, (lw, mask) in enumerate(U.segments(lw_pe, lw_inj, pm, im)):
        g, w = (hp[seg], wp[seg]) if seg < U.N_EV else (hi, wi)
        tol = U.bound(U.n_live(lw, mask))
        assert np.all(np.isfinite(g)) and np.array_equal(g == 0.0, w == 0.0), (what, seg)
        dev = np.abs(g - w)
        assert np.all(dev <= tol * w), (what, seg, float(np.max(dev[w > 0] / w[w > 0])), tol)
        if np.any(w > 0):
            worst = max(worst, float(np.max(dev[w > 0] / w[w > 0])) / tol)
    return worst


@pytest.mark.parametrize("case", U.MASK_CASES)
@pytest.mark.parametrize("n_bins", U.N_BINS)
@pytest.mark.parametrize("name", U.COMPS)
def test_kernel_against_statement(name, n_bins, case):
    """K = 1: every bin of every segment against weighted_histograms_reference on eng.log_weights(theta), with and without masks
    (the masked case has a partial mask, a wholly masked event and a half-masked injection set).  The bound is DERIVED, not
    measured (hist_util.bound): all terms are non-negative, so each bin sum and S carry a relative error of at most
    (n_live + 8) 2^-52 -- summation, two exp roundings, the division -- and a bin may deviate from the statement's by that much of
    the statement's value; a bin the statement leaves at 0 must be 0.  The largest deviation seen is printed in units of the bound
    and recorded in profiles/weighted_histograms/RESULTS.md."""
    from gwinferno_amd.draws import weighted_histograms_reference

    c = _case(name)
    eng, theta, (lw_pe, lw_inj) = c["eng"], c["thetas"][0], c["lw"]
    pb, ib = U.bins(n_bins)
    pm, im = U.masks(case)
    try:
        eng.set_draw_mask(pm, im)
        eng.set_histogram_bins(pb, ib, n_bins=n_bins)
        got = eng.weighted_histograms(theta)
    finally:
        eng.set_draw_mask()
    assert got[0].shape == (U.N_EV, 2, n_bins) and got[1].shape == (2, n_bins) and got[2].dtype == np.int32 and got[2].shape == (U.N_EV + 1,)
    want = weighted_histograms_reference(lw_pe, lw_inj, pm, im, pb, ib, n_bins)
    worst = _compare(got, want, lw_pe, lw_inj, pm, im, (name, n_bins, case))
    print(f"{name} B = {n_bins} {case}: largest |device - statement| / statement = {worst:.3f} of the derived bound")
    if case == "masked":
        assert got[2][U.DEAD_EVENT] == 1 and np.array_equal(got[0][U.DEAD_EVENT], np.zeros((2, n_bins)))
    if case == "free":  # one set at a time: the other is left out, the sums are the same bits
        eng.set_histogram_bins(pb, None, n_bins=n_bins)
        only_pe = eng.weighted_histograms(theta)
        eng.set_histogram_bins(None, ib, n_bins=n_bins)
        only_inj = eng.weighted_histograms(theta)
        assert only_pe[1] is None and np.array_equal(only_pe[0], got[0]) and np.array_equal(only_pe[2], [0, 0, 0, 0])
        assert only_inj[0] is None and np.array_equal(only_inj[1], got[1]) and np.array_equal(only_inj[2], [0, 0, 0, 0])


@pytest.mark.parametrize("name", U.COMPS)
def test_determinism(name):
    """The same call twice gives equal bits; K = 3 in one call equals 2 + 1 and 1 + 1 + 1 through the in/out accumulation, to the
    bit; a second handle of the same model gives the same; the postprocess function with chunk sizes 1 and 64 gives equal bits."""
    from gwinferno_amd import postprocess as P

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    pb, ib = U.bins(7)
    eng.set_histogram_bins(pb, ib, n_bins=7)
    whole = eng.weighted_histograms(thetas)
    again = eng.weighted_histograms(thetas)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again)) and np.all(whole[2] == 0)
    assert np.all(whole[0].sum(axis=2) > 0.0) and np.all(whole[0].sum(axis=2) <= 3.0 + 1e-12)  # sums over three points, not means
    for split in ((2, 1), (1, 2), (1, 1, 1)):
        out, at = None, 0
        for n in split:
            out = eng.weighted_histograms(thetas[at : at + n], out=out)
            at += n
        assert all(np.array_equal(a, b) for a, b in zip(whole, out)), split
    single = eng.weighted_histograms(thetas[1])  # one point given as (n_theta,)
    assert not np.array_equal(single[0], eng.weighted_histograms(thetas[0])[0])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.weighted_histograms(thetas)
    eng.lib.gwi_histogram_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 12 and all(m.value > 0.0 for m in ms)  # the calling thread's last call: three points, four launches each
    comp2 = U.composition(name)
    eng2 = comp2.engine()
    try:
        eng2.set_histogram_bins(pb, ib, n_bins=7)
        assert all(np.array_equal(a, b) for a, b in zip(whole, eng2.weighted_histograms(thetas)))
    finally:
        eng2.close()
    pe, inj, _ = U.catalog()
    e = U.edges(7)
    pe_values, inj_values = {k: pe[k] for k in U.COLUMNS}, {k: inj[k] for k in U.COLUMNS}
    r1 = P.reweighted_event_posteriors(eng, thetas, pe_values, e, inj_values=inj_values, chunk=1)
    r64 = P.reweighted_event_posteriors(eng, thetas, pe_values, e, inj_values=inj_values, chunk=64)
    host = P.reweighted_event_posteriors(eng, thetas, pe_values, e, inj_values=inj_values, backend="host")
    for i, k in enumerate(U.COLUMNS):
        assert np.array_equal(r1[k]["events"], r64[k]["events"]) and np.array_equal(r1[k]["predicted"], r64[k]["predicted"])
        assert np.array_equal(r1[k]["outside"]["events"], r64[k]["outside"]["events"]) and r1[k]["outside"]["predicted"] == r64[k]["outside"]["predicted"]
        assert np.array_equal(r64[k]["events"], whole[0][:, i] / 3.0 / np.diff(e[k])) and np.array_equal(r64[k]["n_points"]["events"], [3, 3, 3])
        assert np.allclose(r64[k]["events"], host[k]["events"], rtol=1e-12, atol=0.0) and np.allclose(r64[k]["predicted"], host[k]["predicted"], rtol=1e-12, atol=0.0)
        assert np.all(np.abs((r64[k]["events"] * np.diff(e[k])).sum(axis=1) - (1.0 - r64[k]["outside"]["events"])) <= 1e-15)


def test_mask_dead_and_outside():
    """One event masked entirely: dead incremented, its H rows zero (also in test_kernel_against_statement); a partial mask equals
    the statement (there).  Here: a theta that sends one event's weights to -inf is counted dead, not NaN; samples coded 0xFFFF
    reduce the row sum by exactly their weight share; a log-weight spread above 800 within one event gives no NaN or inf."""
    from gwinferno_amd.draws import OUTSIDE_BIN, draw_weights, weighted_histograms_reference

    c = _case("plpeak")
    eng, comp = c["eng"], c["comp"]
    pb, ib = U.bins(7)
    eng.set_histogram_bins(pb, ib, n_bins=7)
    # a dead event through theta
    theta = comp.theta(U.dead_event_params())
    lw_pe, lw_inj = eng.log_weights(theta)
    finite = np.isfinite(lw_pe).sum(axis=1)
    print("finite log-weights per event at the dead-event point:", finite)
    assert finite.min() == 0 and finite.max() >= 200
    hp, hi, dead = eng.weighted_histograms(np.stack([theta, c["thetas"][0]]))
    want_dead = np.array([0 if n else 1 for n in finite] + [0 if np.isfinite(lw_inj).any() else 1], dtype=np.int32)
    assert np.array_equal(dead, want_dead) and np.all(np.isfinite(hp)) and np.all(np.isfinite(hi))
    alone = eng.weighted_histograms(c["thetas"][0])
    for ev in np.nonzero(finite == 0)[0]:  # the dead point added nothing: the sum over both points is the second point's
        assert np.array_equal(hp[ev], alone[0][ev])
    # outside samples: the deficit of a row is their weight share
    theta0, (lw_pe, lw_inj) = c["thetas"][0], c["lw"]
    got = eng.weighted_histograms(theta0)
    for seg, (lw, _) in enumerate(U.segments(lw_pe, lw_inj, None, None)):
        w = draw_weights(lw, None)
        for col in range(2):
            code = pb[col, seg] if seg < U.N_EV else ib[col]
            row = got[0][seg, col] if seg < U.N_EV else got[1][col]
            share = w[code == OUTSIDE_BIN].sum() / w.sum()
            assert abs((1.0 - row.sum()) - share) <= 2.0 * U.bound(U.n_live(lw, None)), (seg, col, 1.0 - row.sum(), share)
    # ... and with every sample of one column outside, that column's rows are 0 while the other column's stay as they were
    pb_out = pb.copy()
    pb_out[1] = OUTSIDE_BIN
    eng.set_histogram_bins(pb_out, ib, n_bins=7)
    moved = eng.weighted_histograms(theta0)
    assert np.array_equal(moved[0][:, 1], np.zeros((U.N_EV, 7))) and np.array_equal(moved[0][:, 0], got[0][:, 0]) and np.array_equal(moved[1], got[1])
    assert np.all(moved[2] == 0)  # outside is not dead
    # a spread above 800 within one event
    eng.set_histogram_bins(pb, ib, n_bins=7)
    theta = comp.theta(U.wide_spread_params())
    lw_pe, lw_inj = eng.log_weights(theta)
    spread = [float(np.ptp(r[np.isfinite(r)])) if np.isfinite(r).any() else 0.0 for r in lw_pe]
    print("spread of the finite log-weights per event at the wide-spread point:", spread)
    assert max(spread) > 800.0
    hp, hi, dead = eng.weighted_histograms(theta)
    assert np.all(np.isfinite(hp)) and np.all(np.isfinite(hi)) and np.all(hp >= 0.0) and np.all(hp.sum(axis=2) <= 1.0 + 1e-12)
    want = weighted_histograms_reference(lw_pe, lw_inj, None, None, pb, ib, 7)
    assert np.array_equal(dead, want[2]) and np.allclose(hp, want[0], rtol=1e-9, atol=1e-300) and np.allclose(hi, want[1], rtol=1e-9, atol=1e-300)


def test_limits():
    """B = 257, C = 9, a bin code that is neither a bin nor 0xFFFF, null pointers and a call before set_histogram_bins return
    GWI_ERR_INVALID with a message and without a launch; the engine keeps working afterwards."""
    from gwinferno_amd import _native as N

    comp = U.composition("plpeak")
    eng = comp.engine()
    try:
        theta = comp.theta(U.params("plpeak"))
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):
            eng.weighted_histograms(theta)
        pb, ib = U.bins(7)
        lib, u16, i32 = eng.lib, C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
        th, dead = N.f64(theta), np.zeros(U.N_EV + 1, dtype=np.int32)
        hp, hi = np.zeros((U.N_EV, 2, 7)), np.zeros((2, 7))
        assert lib.gwi_weighted_histograms(eng.handle, N.as_dp(th), 1, N.as_dp(hp), N.as_dp(hi), dead.ctypes.data_as(i32)) == -1
        assert "no bins are set" in lib.gwi_last_error(eng.handle).decode()
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*n_bins = 257"):
            eng.set_histogram_bins(pb, ib, n_bins=257)
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*n_bins = 0"):
            eng.set_histogram_bins(pb, ib, n_bins=0)
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*n_cols = 9"):
            eng.set_histogram_bins(np.zeros((9, U.N_EV, U.N_PE), dtype=np.uint16), np.zeros((9, U.N_INJ), dtype=np.uint16), n_bins=7)
        bad = ib.copy()
        bad[1, 5] = 7
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*inj_bins entry 2605 is 7"):
            eng.set_histogram_bins(pb, bad, n_bins=7)
        assert lib.gwi_set_histogram_bins(eng.handle, 2, 7, None, None) == -1 and "both null" in lib.gwi_last_error(eng.handle).decode()
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):  # none of the refused calls left bins behind
            eng.weighted_histograms(theta)
        eng.set_histogram_bins(pb, ib, n_bins=7)
        for args, word in (((None, 1, N.as_dp(hp), N.as_dp(hi), dead.ctypes.data_as(i32)), "thetas"), ((N.as_dp(th), 0, N.as_dp(hp), N.as_dp(hi), dead.ctypes.data_as(i32)), "k < 1"),
                           ((N.as_dp(th), 1, None, N.as_dp(hi), dead.ctypes.data_as(i32)), "hist_pe"), ((N.as_dp(th), 1, N.as_dp(hp), None, dead.ctypes.data_as(i32)), "hist_inj"),
                           ((N.as_dp(th), 1, N.as_dp(hp), N.as_dp(hi), None), "dead")):
            assert lib.gwi_weighted_histograms(eng.handle, *args) == -1
            assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
        assert not hp.any() and not hi.any() and not dead.any()
        with pytest.raises(ValueError, match="out: hist_pe"):
            eng.weighted_histograms(theta, out=(np.zeros((U.N_EV, 2, 8)), hi, dead))
        with pytest.raises(ValueError, match="out: dead"):
            eng.weighted_histograms(theta, out=(hp, hi, dead.astype(np.int64)))
        good = eng.weighted_histograms(theta)
        c = _case("plpeak")
        c["eng"].set_histogram_bins(pb, ib, n_bins=7)
        assert all(np.array_equal(a, b) for a, b in zip(good, c["eng"].weighted_histograms(theta)))
    finally:
        eng.close()


def test_meaning_histogram_of_index_draws():
    """The catalog make_mock_catalog produces at the settings of tests/test_gpu_mock_catalog.py (8 events x 256 samples, 20 000
    generated injections, seed 3), a single theta: the indices gwi_draw_indices draws for 20 000 uniforms per event (and as many from
    the injection set), binned, agree with H within 5 standard deviations of the multinomial count per bin: |n_b - n H_b| <=
    5 sqrt(n H_b (1 - H_b)).  The bins of a segment are quantiles of its own samples (the codes are per sample: every segment may
    have edges of its own), so no bin's expected count is small."""
    import mock_util as MU

    from gwinferno_amd import mock_catalog as MC
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.draws import OUTSIDE_BIN, digitize

    model = MU.catalog_model(MC)
    pe, inj, total, _ = MC.make_mock_catalog(MU.population(MC, on_host=False), MU.injection_tables(model), model, 8, 256, 20_000, 3)
    inj = {k: v for k, v in inj.items() if k != "snr"}
    comp = COMPOSITIONS["plpeak"](pe, inj, mmin=MU.MMIN, mmax=MU.MMAX)
    eng = comp.engine()
    try:
        theta = comp.theta({k: MU.THETA[k] for k in comp.PARAMS})
        n_bins, n_draw = 7, 20_000
        names = ("mass_1", "mass_ratio")
        own = lambda v: digitize(v, np.quantile(v, np.linspace(0.03, 0.97, n_bins + 1)))  # noqa: E731
        pb, ib = np.stack([np.stack([own(row) for row in pe[k]]) for k in names]), np.stack([own(inj[k]) for k in names])
        eng.set_histogram_bins(pb, ib, n_bins=n_bins)
        hp, hi, dead = eng.weighted_histograms(theta)
        assert np.all(dead == 0)
        rng = np.random.default_rng(9)
        idx_pe, idx_inj = eng.draw_indices(theta, rng.uniform(size=(eng.n_ev, n_draw)), rng.uniform(size=n_draw))
        assert np.all(idx_pe >= 0) and np.all(idx_inj >= 0)
        checked = 0
        for seg in range(eng.n_ev + 1):
            for c in range(2):
                code = pb[c, seg][idx_pe[seg]] if seg < eng.n_ev else ib[c][idx_inj]
                h = hp[seg, c] if seg < eng.n_ev else hi[c]
                counts = np.bincount(code[code != OUTSIDE_BIN], minlength=n_bins)
                sd = np.sqrt(n_draw * h * (1.0 - h))
                assert np.all(np.abs(counts - n_draw * h) <= 5.0 * sd), (seg, c, counts, n_draw * h)
                assert abs(np.count_nonzero(code == OUTSIDE_BIN) - n_draw * (1.0 - h.sum())) <= 5.0 * np.sqrt(n_draw * h.sum() * max(1.0 - h.sum(), 0.0))
                checked += int(np.count_nonzero(h > 0))
        print(f"{checked} bins with weight compared with {n_draw} draws per segment")
        assert checked >= 2 * (eng.n_ev + 1)
    finally:
        eng.close()
