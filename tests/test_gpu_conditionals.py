"""GPU: per-point conditional moments on the device (include/gwi_engine.h: gwi_point_conditionals; gwinferno_amd/csrc/gwi_cond.h; DESIGN
8k): the statement (draws.point_conditionals_reference on the engine's own log-weights) under the derived bounds of
tests/conditional_util.py, slot 0 against the bits of weighted_histograms, consistency with point_moments, determinism over calls, splits
and handles, the absence of side effects on the existing entries, a set left out, the refusals, and the two host functions.

Shapes (tests/moment_util.py, tests/conditional_util.py): 3 events x 1 500 PE samples (two tiles, the second ragged), 2 500 injections (three
tiles, the last ragged), three points of a PL+Peak and of a B-spline model; value columns mass_1 + 1e6, mass_ratio, chi_eff; bin columns
mass_ratio and redshift at 5 (+ 1 designed-empty) bins with two samples per segment coded outside, and at 256 bins with two pairs (512
items); pair lists with three and with eight distinct value columns for the two larger LDS layouts of the tile kernel.  The masked case
removes one event, leaves one sample of another and thins the third.  The case in which the bin column and the value column name the
same quantity is not exercised.  The inputs are vetted without a device in tests/test_conditional_cpu.py."""
import ctypes as C
import os

import conditional_util as CU
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


def _setup(eng, setting, outside=True, n_cols=CU.N_VALUE_COLUMNS):
    eng.set_histogram_bins(*CU.codes(setting, outside), n_bins=CU.N_BINS[setting])
    eng.set_kde_columns(*MU.columns(n_cols))


def _conditionals(eng, thetas, setting, case="free", outside=True):
    try:
        eng.set_draw_mask(*MU.masks(case))
        _setup(eng, setting, outside)
        return eng.point_conditionals(thetas, CU.PAIRS[setting])
    finally:
        eng.set_draw_mask()


@pytest.mark.parametrize("case", ("free", "masked"))
@pytest.mark.parametrize("setting", CU.SETTINGS)
@pytest.mark.parametrize("name", MU.COMPS)
def test_against_the_statement(name, setting, case):
    """Every share, mean and variance of every point against point_conditionals_reference on eng.log_weights under the DERIVED bounds of
    conditional_util.tolerances: counts of roundings times 2^-52 applied to the statement's share, to sum w^ |y| and to sum w^ |y - m|^2
    of the bin (plus the second-order centring term written down there).  Flags and NaN positions agree exactly and no cell is excluded
    other than by that agreement; the designed-empty bin is a = +0.0, m = v = NaN in every live segment; the masked case's dead event gives
    NaN and dead = 1, its single-sample event exactly one non-empty bin per pair with a = 1, the sample as the mean and a variance of
    exactly 0.  The largest deviations are printed as fractions of the bound."""
    c = _case(name)
    pm, im = MU.masks(case)
    x_pe, x_inj = MU.columns(CU.N_VALUE_COLUMNS)
    cp, ci = CU.codes(setting)
    pairs, n_bins = CU.PAIRS[setting], CU.N_BINS[setting]
    share, mean, var, dead = _conditionals(c["eng"], c["thetas"], setting, case)
    n_segs = MU.N_EV + 1
    assert share.shape == mean.shape == var.shape == (MU.N_POINTS, n_segs, len(pairs), n_bins) and dead.shape == (MU.N_POINTS, n_segs) and dead.dtype == np.int32
    got = np.stack([share, mean, var], axis=3)
    worst = np.zeros(3)
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_dead, tol = CU.statement_point(lw_pe, lw_inj, cp, ci, x_pe, x_inj, pairs, n_bins, pm, im)
        assert np.array_equal(dead[k], want_dead) and np.array_equal(np.isnan(got[k]), np.isnan(want))
        assert np.array_equal(np.nonzero(dead[k])[0], [MU.DEAD_EVENT] if case == "masked" else [])
        live = [s for s in range(n_segs) if not want_dead[s]]
        assert len(live) == n_segs - (case == "masked") and np.all(np.isnan(got[k][[s for s in range(n_segs) if want_dead[s]]]))
        assert not np.any(np.isnan(got[k][live][:, :, 0])) and np.array_equal(np.isnan(tol), np.isnan(want))
        cell = ~np.isnan(want)
        dev = np.abs(got[k][cell] - want[cell])
        assert np.all(dev <= tol[cell]), (k, float(np.max(dev - tol[cell])))
        for slot in range(3):
            sel = cell[:, :, slot] & (tol[:, :, slot] > 0.0)
            if sel.any():
                worst[slot] = max(worst[slot], float(np.max(np.abs(got[k][:, :, slot][sel] - want[:, :, slot][sel]) / tol[:, :, slot][sel])))
        if setting == 5:
            e = got[k][live][:, :, :, CU.EMPTY_BIN]
            assert np.all(e[:, :, 0] == 0.0) and not np.any(np.signbit(e[:, :, 0])) and np.all(np.isnan(e[:, :, 1:]))
        if case == "masked":
            one = got[k, MU.SINGLE_EVENT]
            for r, (cx, cy) in enumerate(pairs):
                b = int(cp[cx, MU.SINGLE_EVENT, MU.SINGLE_SAMPLE])
                assert b < n_bins and one[r, 0, b] == 1.0 and np.count_nonzero(one[r, 0]) == 1 and one[r, 1, b] == x_pe[cy, MU.SINGLE_EVENT, MU.SINGLE_SAMPLE] and one[r, 2, b] == 0.0
                assert np.all(np.isnan(np.delete(one[r, 1:], b, axis=1)))
    assert np.any(var[:, -1] > 0.0)
    print(f"{name}, setting {setting}, {case}: largest |device - statement| = {worst[0]:.4f} (share), {worst[1]:.4f} (mean), {worst[2]:.4f} (variance) of the derived bound")


@pytest.mark.parametrize("n_cols", sorted(CU.WIDE_PAIRS))
def test_more_distinct_columns_against_the_statement(n_cols):
    """The pair lists above name two distinct bin columns and two distinct value columns: cond_tile_kernel<2>.  With three distinct value
    columns the launch takes cond_tile_kernel<4> (48 / 52 KB of LDS), with eight cond_tile_kernel<8> (88 / 92 KB, one workgroup per CU):
    the masked case at setting 5 under the same derived bounds, NaN positions and flags exactly, and the pairs the lists share with PAIRS[5]
    have the bits of that call."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    pairs, n_bins = CU.WIDE_PAIRS[n_cols], CU.N_BINS[5]
    assert len({cy for _, cy in pairs}) == n_cols and len(pairs) * n_bins <= 512
    pm, im = MU.masks("masked")
    x_pe, x_inj = MU.columns(n_cols)
    cp, ci = CU.codes(5)
    narrow = _conditionals(eng, thetas, 5, "masked")
    try:
        eng.set_draw_mask(pm, im)
        _setup(eng, 5, n_cols=n_cols)
        share, mean, var, dead = eng.point_conditionals(thetas, pairs)
    finally:
        eng.set_draw_mask()
    got = np.stack([share, mean, var], axis=3)
    worst = 0.0
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_dead, tol = CU.statement_point(lw_pe, lw_inj, cp, ci, x_pe, x_inj, pairs, n_bins, pm, im)
        assert np.array_equal(dead[k], want_dead) and np.array_equal(np.isnan(got[k]), np.isnan(want)) and np.array_equal(np.isnan(tol), np.isnan(want))
        cell = ~np.isnan(want)
        gap = np.abs(got[k][cell] - want[cell])
        assert np.all(gap <= tol[cell]), (k, float(np.max(gap - tol[cell])))
        pos = tol[cell] > 0.0
        worst = max(worst, float(np.max(gap[pos] / tol[cell][pos])))
    for r, pair in enumerate(pairs):
        if pair in CU.PAIRS[5]:
            assert _same([o[:, :, r] for o in (share, mean, var)], [o[:, :, CU.PAIRS[5].index(pair)] for o in narrow[:3]]), pair
    print(f"{n_cols} distinct value columns: largest |device - statement| = {worst:.4f} of the derived bound")


@pytest.mark.parametrize("setting", CU.SETTINGS)
def test_slot_0_has_the_bits_of_weighted_histograms(setting):
    """For every point on its own, every pair and both settings, masked and free: slot 0 is bit for bit what weighted_histograms adds for
    that single point onto a fresh (zeroed) accumulation, for the pair's bin column; a dead segment is NaN here and adds nothing there."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    for case in ("free", "masked"):
        share, _, _, dead = _conditionals(eng, thetas, setting, case)
        try:
            eng.set_draw_mask(*MU.masks(case))
            for k in range(MU.N_POINTS):
                hist_pe, hist_inj, hdead = eng.weighted_histograms(thetas[k])
                assert np.array_equal(hdead, dead[k])
                h = np.concatenate([hist_pe, hist_inj[None]])  # (n_ev + 1, 2, B)
                for r, (cx, _) in enumerate(CU.PAIRS[setting]):
                    for s in range(MU.N_EV + 1):
                        if dead[k, s]:
                            assert np.all(np.isnan(share[k, s, r])) and not h[s, cx].any()
                        else:
                            assert np.array_equal(share[k, s, r], h[s, cx]), (case, k, s, r)
        finally:
            eng.set_draw_mask()


def test_consistent_with_point_moments():
    """Where no sample lies outside the edges the bins partition a segment: sum_b a_b m_b is point_moments' mean and sum_b a_b (v_b + (m_b -
    m)^2) its variance, under the sum of the two entries' derived bounds -- the conditional side's propagated through the sums (a_b tol_m +
    |m_b| tol_a, and a_b (tol_v + 2 |m_b - m| (tol_m + tol_mean)) + (v_b + (m_b - m)^2) tol_a), the moment side's own tolerance, and (B + 4)
    2^-52 of the sums of absolute terms for the host's additions.  Setting 5 without the pushed samples, all three pairs, free and masked."""
    c = _case("bspline_iid")
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = MU.columns(CU.N_VALUE_COLUMNS)
    cp, ci = CU.codes(5, outside=False)
    pairs, n_bins = CU.PAIRS[5], CU.N_BINS[5]
    for case in ("free", "masked"):
        pm, im = MU.masks(case)
        share, mean, var, dead = _conditionals(eng, thetas, 5, case, outside=False)
        try:
            eng.set_draw_mask(pm, im)
            mom_mean, mom_cov, mom_dead = eng.point_moments(thetas)
        finally:
            eng.set_draw_mask()
        assert np.array_equal(dead, mom_dead)
        worst = 0.0
        for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
            _, _, _, tol_mm, tol_mv = MU.statement_point(lw_pe, lw_inj, x_pe, x_inj, pm, im)
            _, _, tol = CU.statement_point(lw_pe, lw_inj, cp, ci, x_pe, x_inj, pairs, n_bins, pm, im)
            for s in range(MU.N_EV + 1):
                if dead[k, s]:
                    continue
                for r, (_, cy) in enumerate(pairs):
                    has = share[k, s, r] > 0.0
                    a, m, v = share[k, s, r][has], mean[k, s, r][has], var[k, s, r][has]
                    ta, tm, tv = (tol[s, r, i][has] for i in range(3))
                    m_all, v_all = mom_mean[k, s, cy], mom_cov[k, s, cy, cy]
                    d = m - m_all
                    tol_1 = (a * tm + np.abs(m) * ta).sum() + tol_mm[s, cy] + (n_bins + 4) * MU.U * (a * np.abs(m)).sum()
                    tol_2 = ((a * (tv + 2.0 * np.abs(d) * (tm + tol_mm[s, cy])) + (v + d * d) * ta).sum() + tol_mv[s, cy, cy] + (n_bins + 4) * MU.U * (a * (v + d * d)).sum())
                    dev_1, dev_2 = abs((a * m).sum() - m_all), abs((a * (v + d * d)).sum() - v_all)
                    assert dev_1 <= tol_1 and dev_2 <= tol_2, (case, k, s, r, dev_1 / tol_1, dev_2 / tol_2)
                    worst = max(worst, dev_1 / tol_1, dev_2 / tol_2)
        print(f"{case}: largest deviation from point_moments = {worst:.4f} of the two entries' bounds")


def test_bits_are_a_function_of_the_arguments():
    """K = 3 in one call, as 1 + 2, 2 + 1 and 1 + 1 + 1 concatenate to the same bits; the same call twice; one point given as (n_theta,);
    calls of K = 64, 65 and 70 against the cyclic reference rows (the stage's edge); a second handle on the same catalog; the diagnostic
    reports six launches per point."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    pairs = CU.PAIRS[5]
    masked = _conditionals(eng, thetas, 5, "masked")
    whole = eng.point_conditionals(thetas, pairs)  # (the mask is off now: another input)
    assert not _same(masked, whole) and _same(whole, eng.point_conditionals(thetas, pairs)) and not whole[3].any()
    assert not np.array_equal(whole[1][0], whole[1][1])
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_conditional_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 6 * MU.N_POINTS and all(m.value > 0.0 for m in ms)
    for split in ((1, 2), (2, 1), (1, 1, 1)):
        parts, at = [], 0
        for n in split:
            parts.append(eng.point_conditionals(thetas[at : at + n], pairs))
            at += n
        assert _same([np.concatenate([p[i] for p in parts]) for i in range(4)], whole), split
    single = eng.point_conditionals(thetas[1], pairs)
    assert single[0].shape == (1, MU.N_EV + 1, len(pairs), CU.N_BINS[5]) and _same([s[0] for s in single], [w[1] for w in whole])
    for n in (64, 65, 70):
        out = eng.point_conditionals(np.tile(thetas, (24, 1))[:n], pairs)
        assert out[0].shape == (n, MU.N_EV + 1, len(pairs), CU.N_BINS[5]) and out[3].shape == (n, MU.N_EV + 1)
        for k in range(n):
            assert _same([o[k] for o in out], [w[k % 3] for w in whole]), (n, k)
    eng2 = MU.composition("plpeak").engine()
    try:
        _setup(eng2, 5)
        assert _same(eng2.point_conditionals(thetas, pairs), whole)
    finally:
        eng2.close()


def test_a_set_left_out():
    """Bins or columns given for one set only: the other set's segments come back NaN, its own with the same bits, the flags unchanged.  Bins
    for PE only together with columns for injections only is refused with a message."""
    from gwinferno_amd import _native as N

    c = _case("plpeak")
    thetas, pairs = c["thetas"], CU.PAIRS[5]
    whole = _conditionals(c["eng"], thetas, 5)
    cp, ci = CU.codes(5)
    x_pe, x_inj = MU.columns(CU.N_VALUE_COLUMNS)
    eng = MU.composition("plpeak").engine()
    try:
        for bins, cols, kept in (((cp, None), (x_pe, x_inj), "pe"), ((cp, ci), (x_pe, None), "pe"), ((None, ci), (x_pe, x_inj), "inj"), ((cp, ci), (None, x_inj), "inj")):
            eng.set_histogram_bins(*bins, n_bins=CU.N_BINS[5])
            eng.set_kde_columns(*cols)
            only = eng.point_conditionals(thetas, pairs)
            mine, other = (slice(0, MU.N_EV), slice(MU.N_EV, None)) if kept == "pe" else (slice(MU.N_EV, None), slice(0, MU.N_EV))
            assert all(np.all(np.isnan(o[:, other])) for o in only[:3]) and _same([o[:, mine] for o in only[:3]], [w[:, mine] for w in whole[:3]])
            assert np.array_equal(only[3], whole[3])
        eng.set_histogram_bins(cp, None, n_bins=CU.N_BINS[5])
        eng.set_kde_columns(None, x_inj)
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no sample set has both bins and columns"):
            eng.point_conditionals(thetas, pairs)
    finally:
        eng.close()


def test_no_existing_entry_moves():
    """weighted_histograms (its running sums split over two calls), point_cdfs, point_moments and weighted_kde (on marginal weights added
    before and after) return the bits they return without the new entry when point_conditionals calls sit in between; point_conditionals
    itself repeats after all of them."""
    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    _setup(eng, 5)
    x_inj = MU.columns(CU.N_VALUE_COLUMNS)[1]
    grid = np.stack([np.linspace(x_inj[i].min(), x_inj[i].max(), 7) for i in range(CU.N_VALUE_COLUMNS)])

    def run(interleave):
        between = (lambda: eng.point_conditionals(thetas, CU.PAIRS[5])) if interleave else (lambda: None)
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
        cdfs = eng.point_cdfs(thetas)
        between()
        return tuple(kde) + tuple(hist) + tuple(cdfs) + tuple(eng.point_moments(thetas))

    plain = run(False)
    own = eng.point_conditionals(thetas, CU.PAIRS[5])
    assert _same(run(True), plain) and _same(eng.point_conditionals(thetas, CU.PAIRS[5]), own)


def test_refusals():
    """On a fresh handle: a call before set_histogram_bins, then before set_kde_columns, then null thetas, k = 0, k < 0, null pairs, out and
    dead, n_pairs = 0 and 9, an index outside the bin columns and outside the value columns, and n_pairs n_bins > 512 through raw ctypes
    each answer GWI_ERR_INVALID with a message and write nothing; afterwards the handle gives the shared engine's bits.  A shard is refused
    from Python, and from the library itself on a world-2 shared-memory handle, before any column check."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    c = _case("plpeak")
    thetas = c["thetas"]
    free = _conditionals(c["eng"], thetas, 5)
    comp = MU.composition("plpeak")
    eng = comp.engine()
    try:
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no bins are set"):
            eng.point_conditionals(thetas[0], CU.PAIRS[5])
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        pairs = np.ascontiguousarray(CU.PAIRS[5], dtype=np.int32)
        many = np.zeros((9, 2), dtype=np.int32)
        th, out, dead = N.f64(thetas[0]), np.full((1, MU.N_EV + 1, 9, 3, 256), 7.0), np.full((1, MU.N_EV + 1), 7, dtype=np.int32)
        full = (N.as_dp(th), 1, 3, pairs.ctypes.data_as(i32), N.as_dp(out), dead.ctypes.data_as(i32))
        assert lib.gwi_point_conditionals(eng.handle, *full) == -1
        assert "gwi_point_conditionals: no bins are set (gwi_set_histogram_bins)" in lib.gwi_last_error(eng.handle).decode()
        eng.set_histogram_bins(*CU.codes(5), n_bins=CU.N_BINS[5])
        assert lib.gwi_point_conditionals(eng.handle, *full) == -1
        assert "gwi_point_conditionals: no columns are set (gwi_set_kde_columns)" in lib.gwi_last_error(eng.handle).decode()
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no columns are set"):
            eng.point_conditionals(thetas[0], CU.PAIRS[5])
        eng.set_kde_columns(*MU.columns(CU.N_VALUE_COLUMNS))

        alive = []  # (the arrays behind the pointers)

        def with_pairs(p):
            alive.append(np.ascontiguousarray(p, dtype=np.int32))
            return full[:2] + (len(p), alive[-1].ctypes.data_as(i32)) + full[4:]

        cases = [((None,) + full[1:], "thetas"), ((full[0], 0) + full[2:], "k < 1"), ((full[0], -1) + full[2:], "k < 1"), (full[:3] + (None,) + full[4:], "pairs is null"),
                 (full[:4] + (None,) + full[5:], "out is null"), (full[:5] + (None,), "dead is null"), (full[:2] + (0,) + full[3:], "n_pairs = 0 is not in 1 ... 8"),
                 (full[:2] + (9, many.ctypes.data_as(i32)) + full[4:], "n_pairs = 9 is not in 1 ... 8"), (with_pairs([(0, 0), (2, 0)]), "pair 1: bin column 2 is not in 0 ... 1"),
                 (with_pairs([(-1, 0)]), "bin column -1"), (with_pairs([(1, 3)]), "pair 0: value column 3 is not in 0 ... 2"), (with_pairs([(0, -1)]), "value column -1")]
        for args, word in cases:
            assert lib.gwi_point_conditionals(eng.handle, *args) == -1, word
            message = lib.gwi_last_error(eng.handle).decode()
            assert message.startswith("gwi_point_conditionals: ") and word in message, (word, message)
        eng.set_histogram_bins(*CU.codes(256), n_bins=256)
        assert lib.gwi_point_conditionals(eng.handle, *with_pairs([(0, 0), (1, 1), (0, 2)])) == -1
        assert "gwi_point_conditionals: n_pairs n_bins = 768 exceeds 512" in lib.gwi_last_error(eng.handle).decode()
        assert np.all(out == 7.0) and np.all(dead == 7)
        _setup(eng, 5)
        assert _same(eng.point_conditionals(thetas, CU.PAIRS[5]), free)  # a second handle; the refused calls left nothing behind
        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_conditionals: this engine holds one shard of the catalog"):
            shards[0].point_conditionals(thetas[0], CU.PAIRS[5])
        seg = f"/gwi_conditional_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            assert lib.gwi_point_conditionals(hs, *full) == -4  # GWI_ERR_UNSUPPORTED
            assert "gwi_point_conditionals: this handle holds one shard of the catalog; the injection moments need the global set" in lib.gwi_last_error(hs).decode()
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        assert _same(eng.point_conditionals(thetas, CU.PAIRS[5]), free)
    finally:
        eng.close()


def _values():
    pe, inj, _ = MU.catalog()
    return ({n: np.asarray(pe[n], dtype=np.float64) for n in ("mass_ratio", "chi_eff")}, {n: np.asarray(inj[n], dtype=np.float64) for n in ("mass_ratio", "chi_eff")},
            CU.edges(5)["mass_ratio"])


def test_catalog_conditional_check_device_against_host():
    """postprocess.catalog_conditional_check on both backends, chi_eff given the mass-ratio bin at setting 5: the raw arrays agree within
    the derived bounds of the first test, the flags and the skipped counts exactly (the designed-empty bin is skipped at every point), and
    the derived per-point arrays under the bounds propagated through the mixture: every event's share, mean and variance enter with
    weights a_eb / sum_e a_eb that sum to 1, so mu_b moves by at most tol_mu = max_e tol_m + 2 max_e |m_eb| max_e (tol_a / a_eb) and, with
    spread_e = v_eb + (m_eb - mu_b)^2, sigma2_b by at most max_e tol_v + 4 max_e |m_eb - mu_b| tol_mu + 4 tol_mu^2 + 2 max_e spread_e max_e
    (tol_a / a_eb); (n_ev + 4) 2^-52 of the largest term is added to each for the host's own sums."""
    from gwinferno_amd import postprocess as P

    c = _case("bspline_iid")
    eng, thetas = c["eng"], c["thetas"]
    pe_values, inj_values, edges = _values()
    dev = P.catalog_conditional_check(eng, thetas, "mass_ratio", "chi_eff", edges, pe_values=pe_values, inj_values=inj_values)
    host = P.catalog_conditional_check(eng, thetas, "mass_ratio", "chi_eff", edges, pe_values=pe_values, inj_values=inj_values, backend="host")
    n_ev, n_bins = MU.N_EV, CU.N_BINS[5]
    assert np.array_equal(dev["dead"], host["dead"]) and np.array_equal(dev["n_live"], host["n_live"]) and np.array_equal(dev["n_skipped"], host["n_skipped"])
    assert np.array_equal(dev["n_skipped"], [0] * 5 + [MU.N_POINTS]) and dev["delta_mean"].shape == (MU.N_POINTS, n_bins) and dev["bands_delta_std"].shape == (3, n_bins)
    from gwinferno_amd.draws import digitize

    cp, ci = digitize(pe_values["mass_ratio"], edges)[None], digitize(inj_values["mass_ratio"], edges)[None]
    worst = 0.0
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, _, tol = CU.statement_point(lw_pe, lw_inj, cp, ci, pe_values["chi_eff"][None], inj_values["chi_eff"][None], [(0, 0)], n_bins, None, None)
        for i, key in enumerate(("point_share", "point_mean", "point_var")):
            assert np.array_equal(host[key][k], want[:, 0, i], equal_nan=True) and np.array_equal(np.isnan(dev[key][k]), np.isnan(want[:, 0, i]))
            cell = ~np.isnan(want[:, 0, i])
            assert np.all(np.abs(dev[key][k][cell] - want[:, 0, i][cell]) <= tol[:, 0, i][cell]), key
        a, m, v = (want[:n_ev, 0, i, :5] for i in range(3))
        ta, tm, tv = (tol[:n_ev, 0, i, :5] for i in range(3))
        mu, s2 = host["mean_obs"][k, :5], host["var_obs"][k, :5]
        rel_a = np.max(ta / a, axis=0)
        tol_mu = np.max(tm, axis=0) + 2.0 * np.max(np.abs(m), axis=0) * rel_a + (n_ev + 4) * MU.U * np.max(np.abs(m), axis=0)
        spread = v + (m - mu) ** 2
        tol_s2 = (np.max(tv, axis=0) + 4.0 * np.max(np.abs(m - mu), axis=0) * tol_mu + 4.0 * tol_mu * tol_mu + 2.0 * np.max(spread, axis=0) * rel_a
                  + (n_ev + 4) * MU.U * np.max(spread, axis=0))
        dev_mu, dev_s2 = np.abs(dev["mean_obs"][k, :5] - mu), np.abs(dev["var_obs"][k, :5] - s2)
        assert np.all(dev_mu <= tol_mu) and np.all(dev_s2 <= tol_s2), (k, dev_mu / tol_mu, dev_s2 / tol_s2)
        assert np.all(np.abs(dev["mean_det"][k, :5] - host["mean_det"][k, :5]) <= tol[n_ev, 0, 1, :5]) and np.all(np.abs(dev["var_det"][k, :5] - host["var_det"][k, :5]) <= tol[n_ev, 0, 2, :5])
        worst = max(worst, float(np.max(dev_mu / tol_mu)), float(np.max(dev_s2 / tol_s2)))
    assert np.array_equal(dev["p_delta_mean_positive"][:5], host["p_delta_mean_positive"][:5]) and np.all(np.isnan(dev["p_delta_mean_positive"][5:]))
    print(f"largest |device - host| of the mixture's mean and variance = {worst:.4f} of the propagated bound")


def test_event_conditional_moments_against_the_marginal_weights():
    """postprocess.event_conditional_moments on both backends under the PROPAGATED bounds, and its share, mean and within + between against
    the moments of the pooled marginal weights restricted to the bin.

    Device against host.  The raw per-point arrays are held to conditional_util.tolerances as in the first test (the host's are the
    statement's bits).  With equal point weights the weight of point k in bin b is u_k = a_k / sum_k a_k, and with tol_a, tol_m, tol_v the
    bounds of the point's share, mean and variance: the u_k move by at most ru = 2 sum_k tol_a / sum_k a_k together, and they sum to 1 on
    both sides, so
      share   = sum_k a_k / K          moves by at most  sum_k tol_a / K
      mean    = sum_k u_k m_k                            max_k tol_m + ru max_k |m_k - mean|                       =: tol_mean
      within  = sum_k u_k v_k                            max_k tol_v + ru max_k v_k
      between = sum_k u_k (m_k - mean)^2                 max_k (2 |d_k| t_k + t_k^2) + ru max_k d_k^2,  d_k = m_k - mean, t_k = tol_m,k + tol_mean
      total   = within + between                         the sum of the two
    and each carries (K + 4) 2^-52 of its largest term for the host's own sums on the two sides.  The worst fraction is printed.

    Against the marginal weights.  marginal_weights_add leaves W_i = sum_k w_ki / S_k on the device, within quant_util.weight_bound(n_pe, K)
    =: r_w relative of the statement's; with equal point weights share_b = sum_{i in b} W_i / K, and mean_b and total_b are the mean and the
    variance of y under W within the bin, the same numbers as the split's in exact arithmetic (the law of total variance).  NumPy's sums
    over the n_b samples of the bin add (n_b + 4) 2^-52 of their absolute terms, so the share is within tol_share + (r_w + (n_b + 4) 2^-52)
    share, the mean within tol_mean + 2 (r_w + (n_b + 4) 2^-52) E_W|y| =: t_mu, and the variance within tol_total + 2 (r_w + (n_b + 4)
    2^-52) Var_W + t_mu^2 (a ratio moves by at most twice the relative error of its weights; centring on a mean off by t_mu adds its
    square)."""
    import quant_util as QU
    from gwinferno_amd import postprocess as P
    from gwinferno_amd.draws import digitize

    c = _case("plpeak")
    eng, thetas = c["eng"], c["thetas"]
    pe_values, inj_values, edges = _values()
    dev = P.event_conditional_moments(eng, thetas, "mass_ratio", "chi_eff", edges, pe_values=pe_values, inj_values=inj_values)
    host = P.event_conditional_moments(eng, thetas, "mass_ratio", "chi_eff", edges, pe_values=pe_values, inj_values=inj_values, backend="host")
    n_ev, n_k, n_bins = MU.N_EV, MU.N_POINTS, CU.N_BINS[5]
    assert np.array_equal(dev["within"] + dev["between"], dev["total"], equal_nan=True) and not dev["n_dead"].any() and np.allclose(dev["neff_points"], n_k)
    assert np.array_equal(dev["n_skipped"], np.tile([0] * 5 + [n_k], (n_ev, 1))) and np.array_equal(dev["n_skipped"], host["n_skipped"])
    cp, ci = digitize(pe_values["mass_ratio"], edges)[None], digitize(inj_values["mass_ratio"], edges)[None]
    want, tol = np.empty((n_k, n_ev, 3, 5)), np.empty((n_k, n_ev, 3, 5))
    for k, (lw_pe, lw_inj) in enumerate(c["lw"]):
        w_k, _, t_k = CU.statement_point(lw_pe, lw_inj, cp, ci, pe_values["chi_eff"][None], inj_values["chi_eff"][None], [(0, 0)], n_bins, None, None)
        for i, key in enumerate(("point_share", "point_mean", "point_var")):
            assert np.array_equal(host[key][k], w_k[:, 0, i], equal_nan=True) and np.array_equal(np.isnan(dev[key][k]), np.isnan(w_k[:, 0, i]))
            cell = ~np.isnan(w_k[:, 0, i])
            assert np.all(np.abs(dev[key][k][cell] - w_k[:, 0, i][cell]) <= t_k[:, 0, i][cell]), key
        want[k], tol[k] = w_k[:n_ev, 0, :, :5], t_k[:n_ev, 0, :, :5]
    (a, m, v), (ta, tm, tv) = (want[:, :, i] for i in range(3)), (tol[:, :, i] for i in range(3))  # each (K, n_ev, 5)
    own = (n_k + 4) * MU.U
    ru = 2.0 * ta.sum(axis=0) / a.sum(axis=0)
    d = m - host["mean"][None, :, :5]
    tol_mean = tm.max(axis=0) + ru * np.abs(d).max(axis=0) + own * np.abs(m).max(axis=0)
    t = tm + tol_mean[None]
    bound = {"share": ta.sum(axis=0) / n_k + own * host["share"][:, :5], "mean": tol_mean,
             "within": tv.max(axis=0) + ru * v.max(axis=0) + own * v.max(axis=0),
             "between": (2.0 * np.abs(d) * t + t * t).max(axis=0) + ru * (d * d).max(axis=0) + own * (d * d).max(axis=0)}
    bound["total"] = bound["within"] + bound["between"] + MU.U * host["total"][:, :5]
    worst = {}
    for key in ("share", "mean", "within", "between", "total"):
        assert np.array_equal(np.isnan(dev[key]), np.isnan(host[key])) and np.all(np.isnan(dev[key][:, 5]) | (key == "share")), key
        gap = np.abs(dev[key][:, :5] - host[key][:, :5])
        assert np.all(bound[key] > 0.0) and np.all(gap <= bound[key]), (key, float(np.max(gap / bound[key])))
        worst[key] = float(np.max(gap / bound[key]))
    print("largest |device - host| as a fraction of the propagated bound:", ", ".join(f"{k} {x:.4f}" for k, x in worst.items()))
    assert np.all(bound["total"] < 1e-11 * host["total"][:, :5])  # (the bounds bind: far below the numbers compared)
    assert np.all(dev["between"][:, :5] > 0.0) and np.all(dev["within"][:, :5] > dev["between"][:, :5])
    eng.marginal_weights_reset()
    eng.marginal_weights_add(thetas)
    W = eng.marginal_weights()[0]
    code = digitize(pe_values["mass_ratio"], edges)
    r_w, worst_w = QU.weight_bound(MU.N_PE, n_k), 0.0
    for e in range(n_ev):
        for b in range(5):
            sel = code[e] == b
            w, y = W[e][sel], pe_values["chi_eff"][e][sel]
            r = r_w + (int(np.count_nonzero(sel)) + 4) * MU.U
            mu = np.average(y, weights=w)
            var = np.average((y - mu) ** 2, weights=w)
            t_share = bound["share"][e, b] + r * w.sum() / n_k
            t_mu = bound["mean"][e, b] + 2.0 * r * np.average(np.abs(y), weights=w)
            t_var = bound["total"][e, b] + 2.0 * r * var + t_mu * t_mu
            gaps = (abs(dev["share"][e, b] - w.sum() / n_k) / t_share, abs(dev["mean"][e, b] - mu) / t_mu, abs(dev["total"][e, b] - var) / t_var)
            assert max(gaps) <= 1.0, (e, b, gaps)
            worst_w = max(worst_w, *gaps)
    print(f"largest deviation from the moments under the marginal weights = {worst_w:.4f} of the bound")
