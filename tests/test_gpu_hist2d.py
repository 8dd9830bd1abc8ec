"""GPU: per-point joint histograms on the device (include/gwi_engine.h: gwi_point_histograms2d; gwinferno_amd/csrc/gwi_hist2d.h)
against their NumPy statement (gwinferno_amd/draws.py: point_histograms2d_reference) fed with the engine's own log-weights, against
gwi_weighted_histograms (a pair (c, c); the marginals), their purity across calls, handles, splits and pair lists, point weights, dead
and extreme segments, sets left out, the refusals, and postprocess on the device against its host backend.

Shapes (tests/hist2d_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 600 injections (three tiles, the last
ragged), three columns, B = 7 and 64, a PL+Peak and a B-spline model.  The inputs are vetted without a device in
tests/test_hist2d_cpu.py: test_inputs_of_the_gpu_tests."""
import ctypes as C
import os

import hist2d_util as HU
import hist_util as U
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CASES = {}
SUM_KEYS = ("hist_pe", "hist_inj", "n_dead", "vsum")
ALL_KEYS = ("obs", "pred", "live") + SUM_KEYS


def _case(name):
    """One engine per composition with its points and their log-weights from the device: made once, shared, never changed."""
    if name not in _CASES:
        comp = U.composition(name)
        eng = comp.engine()
        thetas = U.points(comp, name, 4)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas[: HU.K_POINTS]]
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


def _same(a, b, keys=ALL_KEYS):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _within(got, want, tol, what):
    """Cells of the device within tol (relative to the statement's value) of the statement's; an empty cell of the statement is exactly
    0.  Returns the largest deviation in units of the bound."""
    assert np.all(np.isfinite(got)) and np.array_equal(got == 0.0, want == 0.0), what
    dev = np.abs(got - want)
    assert np.all(dev <= tol * want), (what, float(np.max(dev[want > 0] / want[want > 0])), tol)
    return float(np.max(dev[want > 0] / want[want > 0])) / tol if np.any(want > 0) else 0.0


@pytest.mark.parametrize("case", U.MASK_CASES)
@pytest.mark.parametrize("n_bins", HU.N_BINS)
@pytest.mark.parametrize("name", U.COMPS)
def test_kernels_against_statement(name, n_bins, case):
    """K = 3 points, two pairs: hist_pe, hist_inj (each point's contribution to zeroed sums), obs and pred against
    point_histograms2d_reference on eng.log_weights(theta).  The bounds are DERIVED, not measured: a cell of a segment is held to
    hist_util.bound = (n_live + 8) 2^-52 relative (the same exp on both sides, non-negative terms, one quotient); obs gets n_ev + 1 more
    half-units for the event sum and its quotient (hist2d_util.obs_bound).  live and n_dead are equal; a cell the statement leaves
    empty is exactly 0.  One call with all three points returns the single calls' rows to the bit.  The largest deviation seen is
    printed in units of the bound and recorded in profiles/point_hist2d/RESULTS.md."""
    from gwinferno_amd.draws import point_histograms2d_reference

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"][: HU.K_POINTS]
    pb, ib = HU.bins(n_bins)
    pm, im = U.masks(case)
    try:
        eng.set_draw_mask(pm, im)
        eng.set_histogram_bins(pb, ib, n_bins=n_bins)
        singles = [eng.point_histograms2d(t, HU.PAIRS) for t in thetas]
        whole = eng.point_histograms2d(thetas, HU.PAIRS)
    finally:
        eng.set_draw_mask()
    worst = 0.0
    for p, got in enumerate(singles):
        lw_pe, lw_inj = c["lw"][p]
        want = point_histograms2d_reference(lw_pe, lw_inj, pm, im, pb, ib, n_bins, HU.PAIRS)
        live = HU.live_counts(lw_pe, lw_inj, pm, im)
        assert got["obs"].shape == (1, 2, n_bins, n_bins) and got["hist_pe"].shape == (U.N_EV, 2, n_bins, n_bins) and got["hist_inj"].shape == (2, n_bins, n_bins)
        assert got["live"].dtype == np.int32 and np.array_equal(got["live"][0], want["live"]) and np.array_equal(got["n_dead"], want["n_dead"]) and got["vsum"] is None
        for seg in range(U.N_EV):
            if live[seg] == 0:
                assert not got["hist_pe"][seg].any() and want["n_dead"][seg] == 1
            else:
                worst = max(worst, _within(got["hist_pe"][seg], want["hist_pe"][seg], HU.cell_bound(live[seg]), (name, n_bins, case, p, seg)))
        worst = max(worst, _within(got["hist_inj"], want["hist_inj"], HU.cell_bound(live[U.N_EV]), (name, n_bins, case, p, "inj")))
        assert np.array_equal(got["pred"][0], got["hist_inj"])  # the injection set's table itself
        worst = max(worst, _within(got["obs"][0], want["obs"], HU.obs_bound([n for n in live[: U.N_EV] if n]), (name, n_bins, case, p, "obs")))
        assert np.array_equal(whole["obs"][p], got["obs"][0]) and np.array_equal(whole["pred"][p], got["pred"][0]) and np.array_equal(whole["live"][p], got["live"][0])
    print(f"{name} B = {n_bins} {case}: largest |device - statement| / statement = {worst:.3f} of the derived bound")
    if case == "masked":
        assert whole["n_dead"][U.DEAD_EVENT] == HU.K_POINTS and not whole["hist_pe"][U.DEAD_EVENT].any() and np.all(whole["live"][:, 0] == U.N_EV - 1)


@pytest.mark.parametrize("n_bins", HU.N_BINS)
@pytest.mark.parametrize("name", U.COMPS)
def test_diagonal_pair_and_marginals(name, n_bins):
    """A pair (c, c): every off-diagonal cell is exactly 0 and the diagonal has the BITS gwi_weighted_histograms adds for column c at the
    same single point -- the summation shapes coincide.  A pair (cx, cy): the row and column sums of a segment's table, plus the share of
    the row's samples that the OTHER column codes outside (from the statement's weights), agree with weighted_histograms of cx and cy.
    The bound is the issue's: B more half-units (the row sum of B cells) on top of the cell bound, (n_live + 8) 2^-52 + B 2^-53, relative to
    the 1-D bin."""
    from gwinferno_amd.draws import OUTSIDE_BIN, draw_weights

    c = _case(name)
    eng, theta = c["eng"], c["thetas"][0]
    lw_pe, lw_inj = c["lw"][0]
    pb, ib = HU.bins(n_bins)
    eng.set_histogram_bins(pb, ib, n_bins=n_bins)
    hp, hi, dead = eng.weighted_histograms(theta)
    assert not dead.any()
    got = eng.point_histograms2d(theta, [(0, 0), (2, 2), (0, 2)])
    off = ~np.eye(n_bins, dtype=bool)
    for r, col in ((0, 0), (1, 2)):
        assert not got["hist_pe"][:, r][:, off].any() and not got["hist_inj"][r][off].any()
        assert np.array_equal(np.diagonal(got["hist_pe"][:, r], axis1=1, axis2=2), hp[:, col]) and np.array_equal(np.diagonal(got["hist_inj"][r]), hi[col])
    worst = 0.0
    live = HU.live_counts(lw_pe, lw_inj, None, None)
    for seg, (lw, _) in enumerate(U.segments(lw_pe, lw_inj, None, None)):
        table = got["hist_pe"][seg, 2] if seg < U.N_EV else got["hist_inj"][2]
        h1 = (hp[seg, 0], hp[seg, 2]) if seg < U.N_EV else (hi[0], hi[2])
        codes = (pb[0, seg], pb[2, seg]) if seg < U.N_EV else (ib[0], ib[2])
        w = draw_weights(lw, None)
        s = w.sum()
        tol = HU.cell_bound(live[seg]) + n_bins * 2.0**-53
        for axis, (mine, other) in enumerate(((0, 1), (1, 0))):
            # the part of the 1-D bin whose samples the other column codes outside, from the statement's weights
            lost = np.bincount(codes[mine][(codes[other] == OUTSIDE_BIN) & (codes[mine] != OUTSIDE_BIN)].astype(np.int64),
                               weights=w[(codes[other] == OUTSIDE_BIN) & (codes[mine] != OUTSIDE_BIN)], minlength=n_bins) / s
            marginal = table.sum(axis=1 - axis) + lost
            assert np.array_equal(marginal == 0.0, h1[axis] == 0.0) and np.all(np.abs(marginal - h1[axis]) <= tol * h1[axis]), (seg, axis)
            worst = max(worst, float(np.max(np.abs(marginal - h1[axis])[h1[axis] > 0] / h1[axis][h1[axis] > 0])) / tol)
    print(f"{name} B = {n_bins}: largest |marginal of the table - weighted_histograms| = {worst:.3f} of the bound")


@pytest.mark.parametrize("name", U.COMPS)
def test_purity(name):
    """Bit equality: K = 4 in one call against 1 + 3 and 2 + 2 through the in/out sums; a repeated call; a second handle; the same pair
    alone and as the last of several pairs; accumulate=False leaves obs / pred / live unchanged; the timing report counts 2 + 3 R
    launches per point."""
    c = _case(name)
    eng, thetas = c["eng"], c["thetas"]
    pb, ib = HU.bins(7)
    eng.set_histogram_bins(pb, ib, n_bins=7)
    whole = eng.point_histograms2d(thetas, HU.PAIRS)
    assert _same(whole, eng.point_histograms2d(thetas, HU.PAIRS)) and not whole["n_dead"].any()
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_hist2d_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 4 * (2 + 3 * len(HU.PAIRS)) and all(m.value > 0.0 for m in ms)
    for split in ((1, 3), (2, 2)):
        out, at, rows = None, 0, []
        for n in split:
            out = eng.point_histograms2d(thetas[at : at + n], HU.PAIRS, out=out)
            rows.append(out)
            at += n
        assert _same(whole, out, SUM_KEYS), split
        for key in ("obs", "pred", "live"):
            assert np.array_equal(np.concatenate([r[key] for r in rows]), whole[key]), (split, key)
    bare = eng.point_histograms2d(thetas, HU.PAIRS, accumulate=False)
    assert _same(whole, bare, ("obs", "pred", "live")) and all(bare[k] is None for k in SUM_KEYS)
    alone = eng.point_histograms2d(thetas, [HU.PAIRS[1]])
    last = eng.point_histograms2d(thetas, [(2, 1), (0, 0), HU.PAIRS[1]])
    for key in ("obs", "pred"):
        assert np.array_equal(alone[key][:, 0], whole[key][:, 1]) and np.array_equal(last[key][:, 2], whole[key][:, 1])
    assert np.array_equal(alone["hist_pe"][:, 0], last["hist_pe"][:, 2]) and np.array_equal(alone["hist_inj"][0], last["hist_inj"][2])
    assert np.array_equal(alone["hist_pe"][:, 0], whole["hist_pe"][:, 1]) and np.array_equal(alone["live"], last["live"])
    eng2 = U.composition(name).engine()
    try:
        eng2.set_histogram_bins(pb, ib, n_bins=7)
        assert _same(whole, eng2.point_histograms2d(thetas, HU.PAIRS))
    finally:
        eng2.close()


def test_point_weights():
    """v = 1 everywhere gives the bits of v = None; a point with v = 0 gives the call without that point, n_dead and vsum included (the
    masked case has a dead event: it is not counted at that point); a fractional v agrees with the statement: one more product per
    side, a half-unit each, on top of the cell bound."""
    from gwinferno_amd.draws import point_histograms2d_reference

    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"][: HU.K_POINTS]
    pb, ib = HU.bins(7)
    pm, im = U.masks("masked")
    try:
        eng.set_draw_mask(pm, im)
        eng.set_histogram_bins(pb, ib, n_bins=7)
        plain = eng.point_histograms2d(thetas, HU.PAIRS)
        ones = eng.point_histograms2d(thetas, HU.PAIRS, point_weights=np.ones((HU.K_POINTS, U.N_EV + 1)))
        assert _same(plain, ones, ("obs", "pred", "live", "hist_pe", "hist_inj", "n_dead"))
        assert np.array_equal(ones["vsum"], [3.0, 0.0, 3.0, 3.0]) and np.array_equal(plain["n_dead"], [0, 3, 0, 0])
        v = np.ones((HU.K_POINTS, U.N_EV + 1))
        v[1] = 0.0
        skipped, without = eng.point_histograms2d(thetas, HU.PAIRS, point_weights=v), eng.point_histograms2d(thetas[[0, 2]], HU.PAIRS, point_weights=np.ones(2))
        assert _same(skipped, without, SUM_KEYS) and np.array_equal(skipped["n_dead"], [0, 2, 0, 0]) and np.array_equal(skipped["vsum"], [2.0, 0.0, 2.0, 2.0])
        assert _same(skipped, plain, ("obs", "pred", "live"))  # the point's own rows do not depend on v
        frac = np.array([[0.25, 0.5, 1.0, 0.125]])
        got = eng.point_histograms2d(thetas[0], HU.PAIRS, point_weights=frac)
    finally:
        eng.set_draw_mask()
    lw_pe, lw_inj = c["lw"][0]
    want = point_histograms2d_reference(lw_pe, lw_inj, pm, im, pb, ib, 7, HU.PAIRS, v=frac[0])
    live = HU.live_counts(lw_pe, lw_inj, pm, im)
    assert np.array_equal(got["n_dead"], want["n_dead"]) and np.array_equal(got["vsum"], want["vsum"]) and np.array_equal(got["vsum"], [0.25, 0.0, 1.0, 0.125])
    for seg in (0, 2):
        _within(got["hist_pe"][seg], want["hist_pe"][seg], HU.cell_bound(live[seg]) + 2.0**-52, seg)
    _within(got["hist_inj"], want["hist_inj"], HU.cell_bound(live[U.N_EV]) + 2.0**-52, "inj")


def test_extreme_points():
    """hist_util's dead-event point: the dead event is counted, contributes nothing, obs is the mean over the live events and live says
    so; the wide-spread point (log-weight spread above 800 within an event): no NaN or inf in live cells."""
    from gwinferno_amd.draws import point_histograms2d_reference

    c = _case("plpeak")
    eng, comp = c["eng"], c["comp"]
    pb, ib = HU.bins(7)
    eng.set_histogram_bins(pb, ib, n_bins=7)
    theta = comp.theta(U.dead_event_params())
    lw_pe, lw_inj = eng.log_weights(theta)
    finite = np.isfinite(lw_pe).sum(axis=1)
    assert finite.min() == 0 and finite.max() >= 200
    got = eng.point_histograms2d(np.stack([theta, c["thetas"][0]]), HU.PAIRS)
    want = point_histograms2d_reference(lw_pe, lw_inj, None, None, pb, ib, 7, HU.PAIRS)
    n_dead_events = int(np.count_nonzero(finite == 0))
    assert np.array_equal(got["n_dead"][: U.N_EV], (finite == 0).astype(np.int32)) and np.array_equal(got["live"][0], want["live"]) and got["live"][0, 0] == U.N_EV - n_dead_events
    assert got["live"][1, 0] == U.N_EV and np.all(np.isfinite(got["obs"])) and np.all(np.isfinite(got["hist_pe"]))
    alone = eng.point_histograms2d(c["thetas"][0], HU.PAIRS)
    for ev in np.nonzero(finite == 0)[0]:  # the dead point added nothing: the sum over both points is the second point's
        assert np.array_equal(got["hist_pe"][ev], alone["hist_pe"][ev])
    live = HU.live_counts(lw_pe, lw_inj, None, None)
    _within(got["obs"][0], want["obs"], HU.obs_bound([n for n in live[: U.N_EV] if n]), "obs at the dead-event point")
    theta = comp.theta(U.wide_spread_params())
    lw_pe, lw_inj = eng.log_weights(theta)
    assert max(float(np.ptp(r[np.isfinite(r)])) for r in lw_pe if np.isfinite(r).any()) > 800.0
    wide = eng.point_histograms2d(theta, HU.PAIRS)
    want = point_histograms2d_reference(lw_pe, lw_inj, None, None, pb, ib, 7, HU.PAIRS)
    assert np.array_equal(wide["live"][0], want["live"]) and np.array_equal(wide["n_dead"], want["n_dead"])
    for key in ("obs", "pred", "hist_pe", "hist_inj"):
        assert np.all(np.isfinite(wide[key])) and np.all(wide[key] >= 0.0)
    assert np.all(wide["hist_pe"].sum(axis=(-2, -1)) <= 1.0 + 1e-12) and np.allclose(wide["obs"][0], want["obs"], rtol=1e-9, atol=1e-300)


def _raw_call_leaves_alone(eng, thetas, untouched):
    """A raw library call with non-null hist_pe and hist_inj full of a sentinel while only one set has bins: the buffer of the set that
    is left out comes back as it went in, the other one holds sums."""
    from gwinferno_amd import _native as N

    i32, k = C.POINTER(C.c_int32), len(thetas)
    pairs = np.ascontiguousarray(HU.PAIRS, dtype=np.int32)
    bufs = dict(hist_pe=np.full((U.N_EV, 2, 7, 7), 7.0), hist_inj=np.full((2, 7, 7), 7.0))
    obs, pred, live, n_dead = np.empty((k, 2, 7, 7)), np.empty((k, 2, 7, 7)), np.empty((k, 2), dtype=np.int32), np.zeros(U.N_EV + 1, dtype=np.int32)
    th = N.f64(thetas)
    assert eng.lib.gwi_point_histograms2d(eng.handle, N.as_dp(th), k, 2, pairs.ctypes.data_as(i32), None, N.as_dp(bufs["hist_pe"]), N.as_dp(bufs["hist_inj"]), N.as_dp(obs),
                                          N.as_dp(pred), live.ctypes.data_as(i32), n_dead.ctypes.data_as(i32), None) == 0
    other = "hist_pe" if untouched == "hist_inj" else "hist_inj"
    assert np.all(bufs[untouched] == 7.0) and np.all(bufs[other] >= 7.0) and np.any(bufs[other] > 7.0) and not n_dead.any()


def test_a_set_left_out_and_no_existing_entry_moves():
    """PE bins only: pred is NaN, live[:, 1] = 0, hist_inj is None and a caller's hist_inj buffer is left untouched; injection bins only
    (the same for hist_pe): obs is NaN and live[:, 0] = 0; the covered side
    has the bits of the call with both.  On one handle weighted_histograms, point_cdfs and point_conditionals return the same bits
    before and after a point_histograms2d call."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"][:2]
    pb, ib = HU.bins(7)
    pe_values, inj_values = HU.values()
    eng.set_histogram_bins(pb, ib, n_bins=7)
    eng.set_kde_columns(np.stack([pe_values[k] for k in HU.COLUMNS]), np.stack([inj_values[k] for k in HU.COLUMNS]))
    before = (eng.weighted_histograms(thetas), eng.point_cdfs(thetas), eng.point_conditionals(thetas, [(0, 1)]))
    both = eng.point_histograms2d(thetas, HU.PAIRS)
    after = (eng.weighted_histograms(thetas), eng.point_cdfs(thetas), eng.point_conditionals(thetas, [(0, 1)]))
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(b, a))
    eng.set_histogram_bins(pb, None, n_bins=7)
    only_pe = eng.point_histograms2d(thetas, HU.PAIRS)
    assert only_pe["hist_inj"] is None and np.all(np.isnan(only_pe["pred"])) and np.all(only_pe["live"][:, 1] == 0)
    assert np.array_equal(only_pe["obs"], both["obs"]) and np.array_equal(only_pe["hist_pe"], both["hist_pe"]) and np.array_equal(only_pe["live"][:, 0], both["live"][:, 0])
    _raw_call_leaves_alone(eng, thetas, "hist_inj")
    eng.set_histogram_bins(None, ib, n_bins=7)
    _raw_call_leaves_alone(eng, thetas, "hist_pe")
    only_inj = eng.point_histograms2d(thetas, HU.PAIRS)
    assert only_inj["hist_pe"] is None and np.all(np.isnan(only_inj["obs"])) and np.all(only_inj["live"][:, 0] == 0) and not only_inj["n_dead"].any()
    assert np.array_equal(only_inj["pred"], both["pred"]) and np.array_equal(only_inj["hist_inj"], both["hist_inj"]) and np.all(only_inj["live"][:, 1] == 1)


def test_refusals():
    """No bins set, bins set with 65 bins, n_pairs 0 and 9, a column index out of range, null outputs, k < 1, v outside [0, 1] or NaN and
    a host-only handle return GWI_ERR_INVALID with a message that names the cause; a handle that holds a shard (two ranks on this GPU joined
    through shared memory) is refused by the Python layer in its neighbours' words and by the library with GWI_ERR_UNSUPPORTED and its
    message, nothing written; the handle still works afterwards."""
    from gwinferno_amd import _native as N

    comp = U.composition("plpeak")
    eng = comp.engine()
    try:
        theta = comp.theta(U.params("plpeak"))
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):
            eng.point_histograms2d(theta, HU.PAIRS)
        pe_values, inj_values = HU.values()
        e65 = np.linspace(pe_values["mass_ratio"].min(), 1.0, 66)
        from gwinferno_amd.draws import digitize

        eng.set_histogram_bins(digitize(pe_values["mass_ratio"], e65)[None], digitize(inj_values["mass_ratio"], e65)[None], n_bins=65)
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*n_bins = 65.*at most 64"):
            eng.point_histograms2d(theta, [(0, 0)])
        assert not eng.weighted_histograms(theta)[2].any()  # the other entries keep their 256
        pb, ib = HU.bins(7)
        eng.set_histogram_bins(pb, ib, n_bins=7)
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th = N.f64(theta)
        obs, pred, live = np.full((1, 1, 7, 7), 7.0), np.full((1, 1, 7, 7), 7.0), np.full((1, 2), 7, dtype=np.int32)
        pairs = np.array([[0, 2]], dtype=np.int32)
        good = dict(thetas=N.as_dp(th), k=1, n_pairs=1, pairs=pairs.ctypes.data_as(i32), v=None, hist_pe=None, hist_inj=None, obs=N.as_dp(obs), pred=N.as_dp(pred),
                    live=live.ctypes.data_as(i32), n_dead=None, vsum=None)
        bad_pairs, nine = np.array([[0, 3]], dtype=np.int32), np.zeros((9, 2), dtype=np.int32)
        for change, word in ((dict(thetas=None), "thetas"), (dict(k=0), "k < 1"), (dict(pairs=None), "pairs is null"), (dict(obs=None), "obs is null"),
                             (dict(pred=None), "pred is null"), (dict(live=None), "live is null"), (dict(n_pairs=0), "n_pairs = 0"),
                             (dict(n_pairs=9, pairs=nine.ctypes.data_as(i32)), "n_pairs = 9"), (dict(pairs=bad_pairs.ctypes.data_as(i32)), "bin column 3 is not in 0 ... 2"),
                             (dict(v=N.as_dp(np.array([1.0, 1.5, 1.0, 1.0]))), "not in [0, 1]"), (dict(v=N.as_dp(np.array([1.0, 1.0, np.nan, 1.0]))), "not in [0, 1]"),
                             (dict(v=N.as_dp(np.array([-0.5, 1.0, 1.0, 1.0]))), "not in [0, 1]")):
            args = dict(good)
            args.update(change)
            assert lib.gwi_point_histograms2d(eng.handle, *args.values()) == -1, word
            assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
        assert np.all(obs == 7.0) and np.all(pred == 7.0) and np.all(live == 7)
        with pytest.raises(ValueError, match="point weights"):
            eng.point_histograms2d(theta, HU.PAIRS, point_weights=np.full(1, 2.0))
        with pytest.raises(ValueError, match="out: hist_pe"):
            eng.point_histograms2d(theta, HU.PAIRS, out=dict(hist_pe=np.zeros((U.N_EV, 2, 7, 8)), hist_inj=np.zeros((2, 7, 7)), n_dead=np.zeros(U.N_EV + 1, dtype=np.int32)))
        with pytest.raises(ValueError, match="accumulate=False"):
            eng.point_histograms2d(theta, HU.PAIRS, accumulate=False, out={})
        assert lib.gwi_point_histograms2d(eng.handle, *good.values()) == 0 and np.all(np.isfinite(obs)) and np.array_equal(live[0], [U.N_EV, 1])
        host = U.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
        try:
            assert lib.gwi_point_histograms2d(host.handle, *good.values()) == -1 and "host-only handle" in lib.gwi_last_error(host.handle).decode()
        finally:
            host.close()
        from gwinferno_amd.engine import NativePopulationLikelihood

        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_histograms2d: this engine holds one shard of the catalog"):
            shards[0].point_histograms2d(theta, HU.PAIRS)
        seg = f"/gwi_hist2d_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            obs[:], pred[:], live[:] = 7.0, 7.0, 7
            assert lib.gwi_point_histograms2d(hs, *good.values()) == -4  # GWI_ERR_UNSUPPORTED
            assert "gwi_point_histograms2d: this handle holds one shard of the catalog; the injection table needs the global set" in lib.gwi_last_error(hs).decode()
            assert np.all(obs == 7.0) and np.all(pred == 7.0) and np.all(live == 7)
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        c = _case("plpeak")
        c["eng"].set_histogram_bins(pb, ib, n_bins=7)
        assert _same(eng.point_histograms2d(theta, HU.PAIRS), c["eng"].point_histograms2d(theta, HU.PAIRS))  # after the refusals the handle still works
    finally:
        eng.close()


@pytest.mark.parametrize("name", U.COMPS)
def test_postprocess_device_against_host(name):
    """event_joint_posteriors with equal and leave-one-out weights and catalog_joint_check on the device against backend="host" (the
    statement on eng.log_weights), B = 7, K = 3.  The tables are held to the bounds of test_kernels_against_statement carried through the
    mean over the points (hist2d_util.mean_bound); delta, tv, the mutual informations and the bands to the bounds propagated from them
    (hist2d_util.tv_bound, mi_bound: derivations there); a band is an order statistic of the points' values, so it moves by at most the
    largest per-point bound of its cell; the share of points with delta > 0 may differ only through points whose delta lies within its
    bound of 0.  A mutual information is compared only where every occupied cell of the statement's table exceeds 2^-30 of its total;
    at most 5 % of the items may be left out (vetted in tests/test_hist2d_cpu.py: none is)."""
    from gwinferno_amd import postprocess as P

    c = _case(name)
    eng, thetas = c["eng"], c["thetas"][: HU.K_POINTS]
    _, _, total = U.catalog()
    pe_values, inj_values = HU.values()
    n_bins, k = 7, HU.K_POINTS
    e = HU.edges(n_bins)
    pairs = [(HU.COLUMNS[a], HU.COLUMNS[b]) for a, b in HU.PAIRS]
    live = np.array([HU.live_counts(*c["lw"][p], None, None) for p in range(k)])
    eps_seg = np.array([HU.cell_bound(n) for n in live.max(axis=0)])
    for kw in ({}, dict(leave_one_out=True, total_inj=total)):
        dev = P.event_joint_posteriors(eng, thetas, pe_values, e, pairs=pairs, inj_values=inj_values, **kw)
        host = P.event_joint_posteriors(eng, thetas, pe_values, e, pairs=pairs, inj_values=inj_values, backend="host", **kw)
        assert dev["pairs"] == pairs and dev["events"].shape == (U.N_EV, 2, n_bins, n_bins) and dev["predicted"].shape == (2, n_bins, n_bins)
        for seg in range(U.N_EV):
            _within(dev["events"][seg], host["events"][seg], HU.mean_bound(eps_seg[seg], k, bool(kw)), (name, seg, kw))
        _within(dev["predicted"], host["predicted"], HU.mean_bound(eps_seg[U.N_EV], k, bool(kw)), (name, "predicted", kw))
        assert np.array_equal(dev["n_points"]["events"], host["n_points"]["events"]) and np.array_equal(dev["events_density"] > 0, host["events_density"] > 0)
        if kw:
            assert np.array_equal(dev["point_weight_sum"], host["point_weight_sum"]) and np.array_equal(dev["elpd_loo"], host["elpd_loo"])
    dev = P.catalog_joint_check(eng, thetas, pe_values, e, inj_values, pairs=pairs, total_inj=total)
    host = P.catalog_joint_check(eng, thetas, pe_values, e, inj_values, pairs=pairs, total_inj=total, backend="host")
    assert dev["n_skipped"] == host["n_skipped"] == 0 and np.array_equal(dev["live"], host["live"]) and np.array_equal(dev["log_nEffs"], host["log_nEffs"])
    assert dev["log_nEffs"].shape == (k, U.N_EV + 1) and np.all(np.isfinite(dev["log_nEffs"]))
    eps_obs = np.array([HU.obs_bound(list(live[p, : U.N_EV])) for p in range(k)])
    eps_pred = np.array([HU.cell_bound(live[p, U.N_EV]) for p in range(k)])
    tol_delta = eps_obs[:, None, None, None] * host["obs"] + eps_pred[:, None, None, None] * host["pred"] + 2.0**-53 * np.abs(host["delta"])
    for p in range(k):
        _within(dev["obs"][p], host["obs"][p], eps_obs[p], (name, p, "obs"))
        _within(dev["pred"][p], host["pred"][p], eps_pred[p], (name, p, "pred"))
    assert np.all(np.abs(dev["delta"] - host["delta"]) <= tol_delta)
    assert np.all(np.abs(dev["bands_delta"] - host["bands_delta"]) <= tol_delta.max(axis=0)[None])
    unsure = (np.abs(host["delta"]) <= tol_delta).sum(axis=0)
    assert np.all(np.abs(dev["p_delta_positive"] - host["p_delta_positive"]) <= unsure / k + 1e-15)
    assert np.all(np.abs(dev["tv"] - host["tv"]) <= HU.tv_bound(eps_obs, eps_pred, n_bins)[:, None])
    assert np.all(np.abs(dev["bands_tv"] - host["bands_tv"]) <= HU.tv_bound(eps_obs, eps_pred, n_bins).max())
    left_out = 0
    tol_mi = {}
    for side, eps in (("obs", eps_obs), ("pred", eps_pred)):
        ok = HU.mi_comparable(host[side])
        left_out += int(np.count_nonzero(~ok))
        tol_mi[side] = HU.mi_bound(eps[:, None], n_bins, HU.abs_log_sum(host[side]))
        assert np.all(np.abs(dev["mi_" + side] - host["mi_" + side])[ok] <= tol_mi[side][ok]), side
    assert left_out <= 0.05 * 2 * k * len(pairs)
    both = HU.mi_comparable(host["obs"]) & HU.mi_comparable(host["pred"])
    assert np.all(np.abs(dev["delta_mi"] - host["delta_mi"])[both] <= (tol_mi["obs"] + tol_mi["pred"] + 2.0**-52)[both])
    print(f"{name}: tv {host['tv'].ravel()}, mi_obs {host['mi_obs'].ravel()}, mi_pred {host['mi_pred'].ravel()}; {left_out} tables left out of the mi comparison")
