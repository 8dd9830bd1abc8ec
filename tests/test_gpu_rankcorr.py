"""GPU: per-point rank correlations on the device (include/gwi_engine.h: gwi_set_rankcorr_columns, gwi_point_rank_correlations;
gwinferno_amd/csrc/gwi_rankcorr.h): the statement (draws.point_rank_correlations_reference on the engine's own log-weights)
under the derived bounds of tests/rankcorr_util.py, ties, monotone maps in bits, masks and dead sets, determinism over calls, splits
and handles, the absence of side effects on the existing entries, the refusals, and postprocess.catalog_rank_correlation_check on both
backends.

Shapes (tests/rankcorr_util.py), PL+Peak x PL-q x PL-z on a seeded synthetic catalog: 5 events x 700 PE samples (the pooled 3 500 make
four tiles along an order, the last ragged, mixing events; an event's sample tile is ragged) with 2 500 injections (three tiles, the last
ragged), and 2 x 1 024 with 2 048 injections (every tile full); three points; 1, 3 and 8 columns.  The statement and the bounds are
vetted without a device in tests/test_rankcorr_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import rankcorr_util as RU

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(shape="ragged"):
    """One engine per shape with its three points and their log-weights from the device: made once, shared."""
    if shape not in _CASES:
        comp = RU.composition(shape)
        eng = comp.engine()
        thetas = RU.points(comp)
        thetas.setflags(write=False)
        lw = [eng.log_weights(t) for t in thetas]
        for pair in lw:
            for a in pair:
                a.setflags(write=False)
        _CASES[shape] = dict(comp=comp, eng=eng, thetas=thetas, lw=lw)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
    _CASES.clear()


def _same(a, b):
    """equal bits, NaN in the same places"""
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def _run(eng, thetas, x_pe, x_inj, masks=(None, None)):
    try:
        eng.set_draw_mask(*masks)
        eng.set_rankcorr_columns(x_pe, x_inj)
        return eng.point_rank_correlations(thetas)
    finally:
        eng.set_draw_mask()


def _rho(cov):
    s = np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return cov / (s[..., :, None] * s[..., None, :])


def _against_the_statement(c, x_pe, x_inj, masks, constant=()):
    """every number of every point against the statement under the derived bounds; returns the largest deviations as fractions of them"""
    from gwinferno_amd import draws as D

    n_cols, n_ev = x_pe.shape[0], x_pe.shape[1]
    total, mean_rank, cov, dead, dead_set = _run(c["eng"], c["thetas"], x_pe, x_inj, masks)
    k = len(c["lw"])
    assert total.shape == (k, 2) and mean_rank.shape == (k, 2, n_cols) and cov.shape == (k, 2, n_cols, n_cols) and dead.shape == (k, n_ev + 1) and dead_set.shape == (k, 2)
    assert dead.dtype == np.int32 and dead_set.dtype == np.int32 and np.array_equal(cov, np.swapaxes(cov, 2, 3), equal_nan=True)
    codes_obs, codes_det = RU.codes(x_pe, x_inj)
    varying = [i for i in range(n_cols) if i not in constant]
    worst = dict(U=0.0, mean=0.0, R=0.0, rho=0.0)
    for p, (lw_pe, lw_inj) in enumerate(c["lw"]):
        want, want_dead = D.point_rank_correlations_reference(lw_pe, lw_inj, codes_obs, codes_det, *masks)
        w_total, w_mean, w_cov = D.rankcorr_matrix(want, n_cols)
        assert np.array_equal(dead[p], want_dead[: n_ev + 1]) and np.array_equal(dead_set[p], want_dead[[n_ev + 1, n_ev]])
        tol_r, tol_m = RU.set_tolerances(lw_pe, lw_inj, *masks)
        for s in range(2):
            if dead_set[p, s]:
                assert total[p, s] == 0.0 and np.all(np.isnan(mean_rank[p, s])) and np.all(np.isnan(cov[p, s])) and np.all(np.isnan(w_cov[s]))
                continue
            n_live = max(RU.HU.n_live(lw_pe[e], None if masks[0] is None else masks[0][e]) for e in range(n_ev)) if s == 0 else 0
            tol_u = 1.01 * RU.U * (RU.weight_units(n_live, s == 0) + 0.5 * (RU.sum_depth(n_ev * -(-x_pe.shape[2] // RU.TILE) if s == 0 else -(-lw_inj.size // RU.TILE)) + 1)) * w_total[s]
            dev_u, dev_m, dev_r = abs(total[p, s] - w_total[s]), np.abs(mean_rank[p, s] - w_mean[s]), np.abs(cov[p, s] - w_cov[s])
            print(f"point {p}, set {s}: |device - statement| / bound: U {dev_u / tol_u:.4f}, mean rank {dev_m.max() / tol_m[s]:.4f}, R {dev_r.max() / tol_r[s]:.4f}")
            assert dev_u <= tol_u and np.all(dev_m <= tol_m[s]) and np.all(dev_r <= tol_r[s])
            assert np.all(np.abs(mean_rank[p, s] - 0.5) <= tol_m[s] + RU.STATEMENT_MEAN_ROUNDING)
            for i in constant:
                assert np.array_equal(cov[p, s, i], np.zeros(n_cols)) and np.array_equal(w_cov[s][i], np.zeros(n_cols))
            worst.update(U=max(worst["U"], dev_u / tol_u), mean=max(worst["mean"], dev_m.max() / tol_m[s]), R=max(worst["R"], dev_r.max() / tol_r[s]))
            if len(varying) > 1:
                sub = np.ix_(varying, varying)
                got, ref = _rho(cov[p, s])[sub], _rho(w_cov[s])[sub]
                diag = np.diagonal(w_cov[s])[varying]
                tol_rho = RU.rho_tolerance(tol_r[s], w_cov[s][sub], diag[:, None] * np.ones(len(varying)), diag[None, :] * np.ones((len(varying), 1)))
                assert np.all(np.abs(got - ref) <= tol_rho)
                worst["rho"] = max(worst["rho"], float(np.max(np.abs(got - ref) / tol_rho)))
    return worst, (total, mean_rank, cov, dead, dead_set)


@pytest.mark.parametrize("shape,n_cols,case", [("ragged", 1, "free"), ("ragged", 3, "free"), ("ragged", 8, "free"), ("ragged", 3, "masked"), ("ragged", 8, "masked"),
                                               ("full", 3, "free"), ("full", 8, "masked")])
def test_against_the_statement(shape, n_cols, case):
    """U, every mean rank, every R_cd and every rho of every point and set against point_rank_correlations_reference on eng.log_weights
    under the DERIVED bounds of rankcorr_util (absolute on R, since |d| <= 1/2, and propagated to rho).  Flags and NaN positions agree
    exactly; the mean ranks sit at 1/2 within the bound.  C = 1, 3 and 8 are the template's ends and a middle.  The largest deviations
    are printed as fractions of the bound."""
    c = _case(shape)
    worst, out = _against_the_statement(c, *RU.columns(n_cols, shape), RU.masks(case, shape))
    dead, dead_set = out[3], out[4]
    assert not dead_set.any() and np.array_equal(np.nonzero(dead.any(axis=0))[0], [RU.DEAD_EVENT] if case == "masked" else [])
    n_live_events = RU.SHAPES[shape][0] - (case == "masked")
    assert np.all(np.abs(out[0][:, 0] - n_live_events) < 1e-9)  # (each live event weighs 1)
    diag = np.arange(n_cols)
    assert np.all(out[2][:, :, diag, diag] > 0.01)
    print(f"{shape}, C = {n_cols}, {case}: largest |device - statement| as a fraction of the derived bound: " + ", ".join(f"{key} {v:.4f}" for key, v in worst.items()))


def test_ties():
    """One column rounded to two decimals (hundreds of members share a value), one held in float32, one constant: against the statement
    under the same bounds; the constant column has R = 0 exactly in its row on the device, and catalog_rank_correlation_check flags its
    pairs, gives NaN and divides nothing, while the pair without it is a number."""
    from gwinferno_amd import postprocess as P

    c = _case()
    x_pe, x_inj = RU.columns(3, "ragged", True)
    assert np.unique(x_pe[0]).size < 200 and np.unique(x_inj[0]).size < 200 and np.unique(x_pe[2]).size == 1
    worst, out = _against_the_statement(c, x_pe, x_inj, (None, None), constant=(2,))
    assert np.all(out[2][:, :, 0, 0] > 0.01) and np.all(out[2][:, :, 1, 1] > 0.01)
    print("ties: largest fractions of the bound: " + ", ".join(f"{key} {v:.4f}" for key, v in worst.items()))
    names = ("rounded", "narrow", "constant")
    r = P.catalog_rank_correlation_check(c["eng"], c["thetas"], {n: x_pe[i] for i, n in enumerate(names)}, inj_values={n: x_inj[i] for i, n in enumerate(names)})
    k = len(c["lw"])
    assert np.array_equal(r["pairs"], [[0, 1], [0, 2], [1, 2]]) and np.array_equal(r["degenerate_obs"], np.tile([0, 1, 1], (k, 1))) and np.array_equal(r["degenerate_det"], r["degenerate_obs"])
    assert np.all(np.isfinite(r["delta"][:, 0])) and np.all(np.isnan(r["delta"][:, 1:])) and not r["n_skipped"].any()


def test_monotone_map_in_bits():
    """A handle given x and a second handle given exp(x) return identical bits: only the codes reach the device, and a strictly
    increasing map does not change them.  (x, -x) gives rho = -1 within the propagated bound."""
    c = _case()
    x_pe, x_inj = RU.columns(3)
    plain = _run(c["eng"], c["thetas"], x_pe, x_inj)
    eng2 = RU.composition().engine()
    try:
        assert _same(_run(eng2, c["thetas"], np.exp(x_pe), np.exp(x_inj)), plain)
    finally:
        eng2.close()
    both = _run(c["eng"], c["thetas"], np.stack([x_pe[0], -x_pe[0]]), np.stack([x_inj[0], -x_inj[0]]))
    for p, (lw_pe, lw_inj) in enumerate(c["lw"]):
        tol_r, _ = RU.set_tolerances(lw_pe, lw_inj, None, None)
        for s in range(2):
            r = both[2][p, s]
            tol = RU.rho_tolerance(tol_r[s], r[0, 1], r[0, 0], r[1, 1])
            assert abs(r[0, 1] / np.sqrt(r[0, 0] * r[1, 1]) + 1.0) <= tol, (p, s)


def test_masks_and_dead_sets():
    """set_draw_mask thins one event and removes another: the dead event is flagged, its members weigh 0, and the observed set is the
    statement over the live events ALONE (a catalog without the event: rho within the propagated bound, U = 4).  With no injection
    left the detected set gives NaN rows and its flag, and the observed rows keep their bits; with no PE sample left the observed set
    does, and the detected rows keep theirs."""
    from gwinferno_amd import draws as D

    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = RU.columns(3)
    pm, im = RU.masks("masked")
    total, mean_rank, cov, dead, dead_set = _run(eng, thetas, x_pe, x_inj, (pm, im))
    n_ev = x_pe.shape[1]
    keep = [e for e in range(n_ev) if e != RU.DEAD_EVENT]
    assert np.array_equal(dead, np.tile(np.eye(n_ev + 1, dtype=np.int32)[RU.DEAD_EVENT], (len(thetas), 1))) and not dead_set.any()
    for p, (lw_pe, lw_inj) in enumerate(c["lw"]):
        alone, _ = D.point_rank_correlations_reference(lw_pe[keep], lw_inj, *RU.codes(x_pe[:, keep], x_inj), pm[keep], im)
        _, _, want = D.rankcorr_matrix(alone, 3)
        tol_r, _ = RU.set_tolerances(lw_pe, lw_inj, pm, im)
        iu = np.triu_indices(3, 1)
        got, ref = _rho(cov[p, 0])[iu], _rho(want[0])[iu]
        tol = RU.rho_tolerance(tol_r[0], want[0][iu], np.diagonal(want[0])[iu[0]], np.diagonal(want[0])[iu[1]])
        assert np.all(np.abs(got - ref) <= tol) and abs(total[p, 0] - len(keep)) < 1e-9
    none = _run(eng, thetas, x_pe, x_inj, RU.masks("no_inj"))
    assert np.all(none[4] == [0, 1]) and np.all(none[3][:, n_ev] == 1) and np.all(np.isnan(none[1][:, 1])) and np.all(np.isnan(none[2][:, 1])) and np.all(none[0][:, 1] == 0.0)
    assert _same([a[:, 0] for a in none[:3]], [a[:, 0] for a in (total, mean_rank, cov)])
    gone = _run(eng, thetas, x_pe, x_inj, (np.zeros_like(pm), im))
    assert np.all(gone[4] == [1, 0]) and np.all(gone[3][:, :n_ev] == 1) and np.all(np.isnan(gone[2][:, 0])) and _same([a[:, 1] for a in gone[:3]], [a[:, 1] for a in (total, mean_rank, cov)])


def test_bits_are_a_function_of_the_arguments():
    """K = 65 crosses the 64-point stage; it equals the calls of 40 + 25 concatenated, itself repeated, and a second handle on the same
    catalog; the diagnostic reports seven launches per point.  point_moments, point_pits_exact and weighted_histograms called before
    and after the new entry return identical bits: no foreign state is touched.  Calling the setter again with another C works and
    replaces the columns."""
    import hist_util as HU
    from gwinferno_amd.draws import digitize

    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = RU.columns(8)
    pe, inj, _ = RU.catalog()
    many = np.tile(thetas, (22, 1))[:65]
    eng.set_kde_columns(x_pe[:3], x_inj[:3])
    eng.set_rank_columns(x_pe[:2], x_inj[:2])
    edges = np.linspace(5.0, 100.0, 9)
    eng.set_histogram_bins(np.stack([digitize(pe["mass_1"], edges)]), np.stack([digitize(inj["mass_1"], edges)]), n_bins=8)

    def others():
        return tuple(eng.point_moments(thetas)) + tuple(eng.point_pits_exact(thetas)) + tuple(eng.weighted_histograms(thetas))

    before = others()
    eng.set_rankcorr_columns(x_pe[:3], x_inj[:3])
    whole = eng.point_rank_correlations(many)
    assert whole[0].shape == (65, 2) and whole[2].shape == (65, 2, 3, 3) and whole[3].shape == (65, x_pe.shape[1] + 1)
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_point_rankcorr_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 7 * 65 and all(m.value > 0.0 for m in ms)
    assert _same(others(), before)
    parts = [eng.point_rank_correlations(many[:40]), eng.point_rank_correlations(many[40:])]
    assert _same([np.concatenate([p[i] for p in parts]) for i in range(5)], whole) and _same(eng.point_rank_correlations(many), whole)
    for k in range(65):
        assert _same([w[k] for w in whole], [w[k % 3] for w in whole]), k
    assert not np.array_equal(whole[2][0], whole[2][1])
    single = eng.point_rank_correlations(thetas[1])
    assert single[0].shape == (1, 2) and _same([s[0] for s in single], [w[1] for w in whole])
    eng.set_rankcorr_columns(x_pe, x_inj)
    wide = eng.point_rank_correlations(thetas)
    assert wide[2].shape == (3, 2, 8, 8) and np.array_equal(wide[2][:, :, :3, :3], whole[2][:3]) and np.array_equal(wide[0], whole[0][:3])
    eng.set_rankcorr_columns(x_pe[:1], x_inj[:1])
    narrow = eng.point_rank_correlations(thetas)
    assert narrow[2].shape == (3, 2, 1, 1) and np.array_equal(narrow[2][:, :, 0, 0], whole[2][:3, :, 0, 0])
    assert _same(others(), before)
    eng2 = RU.composition().engine()
    try:
        eng2.set_rankcorr_columns(x_pe[:3], x_inj[:3])
        assert _same(eng2.point_rank_correlations(many), whole)
    finally:
        eng2.close()
    assert HU.TILE == RU.TILE


def test_refusals():
    """On a fresh handle: a call before set_rankcorr_columns; every violation of the setter's contract (n_cols outside 1 ... 8, a null
    array, an order that is no permutation, a rank out of range, lt above le, a member's position outside lt ... le - 1), after each
    of which the entry still refuses; then null thetas, k = 0, k < 0, null out and null dead -- each GWI_ERR_INVALID with a message,
    nothing written; afterwards the handle gives the shared engine's bits.  A shard is refused from Python, and from the library itself
    on a world-2 shared-memory handle with GWI_ERR_UNSUPPORTED, before its arguments are looked at."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    c = _case()
    thetas = c["thetas"]
    x_pe, x_inj = RU.columns(2)
    free = _run(c["eng"], thetas, x_pe, x_inj)
    comp = RU.composition()
    eng = comp.engine()
    try:
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*no rank-correlation columns are set"):
            eng.point_rank_correlations(thetas[0])
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        th, out, dead = N.f64(thetas[0]), np.full((1, 2, 6), 7.0), np.full((1, eng.n_ev + 2), 7, dtype=np.int32)
        full = (N.as_dp(th), 1, N.as_dp(out), dead.ctypes.data_as(i32))
        assert lib.gwi_point_rank_correlations(eng.handle, *full) == -1
        assert "gwi_point_rank_correlations: no rank-correlation columns are set (gwi_set_rankcorr_columns)" in lib.gwi_last_error(eng.handle).decode()
        good = [np.array(a) for a in RU.codes(x_pe, x_inj)[0] + RU.codes(x_pe, x_inj)[1]]
        n_obs, n_det = good[0].shape[1], good[3].shape[1]

        def changed(i, at, value):
            arrays = [a.copy() for a in good]
            arrays[i][at] = value
            return arrays

        first = int(good[3][1][0])   # the member at position 0 of the detected order of column 1: lt = 0, le >= 1
        tenth = int(good[0][0][10])  # the member at position 10 of the observed order of column 0: le = its lt puts the position outside
        bad = [((0, good), "n_cols = 0 is not in 1 ... 8"), ((9, good), "n_cols = 9 is not in 1 ... 8"), ((2, good[:2] + [None] + good[3:]), "is null"),
               ((2, changed(0, (1, 5), good[0][1, 6])), "order_obs column 1: position .* not a permutation of the set's 3500 members"),
               ((2, changed(3, (0, 0), n_det)), "order_det column 0: position 0 holds 2500: not a permutation"),
               ((2, changed(1, (0, 7), -1)), "lt_obs column 0, member 7: -1 is not in 0 ... n = 3500"),
               ((2, changed(5, (1, 3), n_det + 1)), "le_det column 1, member 3: 2501 is not in 0 ... n = 2500"),
               ((2, changed(4, (1, first), 1)), f"lt_det column 1, member {first}: the member's position 0 along the order is not in lt = 1"),
               ((2, changed(2, (0, tenth), int(good[1][0][tenth]))), f"lt_obs column 0, member {tenth}: the member's position 10 along the order is not in")]
        assert n_obs == 3500
        for (n_cols, arrays), word in bad:
            ptrs = [None if a is None else a.ctypes.data_as(i32) for a in arrays]
            assert lib.gwi_set_rankcorr_columns(eng.handle, n_cols, *ptrs) == -1, word
            message = lib.gwi_last_error(eng.handle).decode()
            assert message.startswith("gwi_set_rankcorr_columns: ") and re.search(word, message), (word, message)
            assert lib.gwi_point_rank_correlations(eng.handle, *full) == -1 and "no rank-correlation columns are set" in lib.gwi_last_error(eng.handle).decode()
        assert lib.gwi_set_rankcorr_columns(eng.handle, 2, *[a.ctypes.data_as(i32) for a in good]) == 0
        for args, word in (((None,) + full[1:], "thetas"), ((full[0], 0) + full[2:], "k < 1"), ((full[0], -1) + full[2:], "k < 1"),
                           (full[:2] + (None,) + full[3:], "out is null"), (full[:3] + (None,), "dead is null")):
            assert lib.gwi_point_rank_correlations(eng.handle, *args) == -1
            message = lib.gwi_last_error(eng.handle).decode()
            assert message.startswith("gwi_point_rank_correlations: ") and word in message, (word, message)
        assert np.all(out == 7.0) and np.all(dead == 7)
        assert lib.gwi_point_rank_correlations(eng.handle, *full) == 0 and np.array_equal(out[0, :, 0], free[0][0])
        eng._rankcorr_shape = (2,)
        assert _same(eng.point_rank_correlations(thetas), free)  # a second handle; the refused calls left nothing behind
        p = comp.placeholder()
        shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_rank_correlations: this engine holds one shard of the catalog"):
            shards[0].point_rank_correlations(thetas[0])
        seg = f"/gwi_rankcorr_test_{os.getpid()}"
        try:
            for r, sh in enumerate(shards):
                sh.shm_comm_init(seg, r, 2)
            hs = shards[0].handle
            for args in (full, (None, 0, None, None)):
                assert lib.gwi_point_rank_correlations(hs, *args) == -4  # GWI_ERR_UNSUPPORTED
                assert "gwi_point_rank_correlations: this handle holds one shard of the catalog; the rank sets need the global set" in lib.gwi_last_error(hs).decode()
            assert lib.gwi_set_rankcorr_columns(hs, 0, None, None, None, None, None, None) == -4
            assert "gwi_set_rankcorr_columns: this handle holds one shard of the catalog; the rank sets need the global set" in lib.gwi_last_error(hs).decode()
        finally:
            lib.gwi_shm_comm_unlink(seg.encode())
            for sh in shards:
                sh.close()
        assert _same(eng.point_rank_correlations(thetas), free)
    finally:
        eng.close()


def test_catalog_rank_correlation_check_device_against_host():
    """postprocess.catalog_rank_correlation_check on both backends: flags and counts agree exactly and are all 0, every rho and delta
    within the propagated bound (twice it for delta), the raw R within the bound on R, and rank_mean_error of the device below the
    bound on a mean rank (plus the statement's own rounding)."""
    from gwinferno_amd import postprocess as P

    c = _case()
    pe_values, inj_values = RU.values(3)
    dev = P.catalog_rank_correlation_check(c["eng"], c["thetas"], pe_values, inj_values=inj_values)
    host = P.catalog_rank_correlation_check(c["eng"], c["thetas"], pe_values, inj_values=inj_values, backend="host")
    for key in ("dead", "dead_set", "degenerate_obs", "degenerate_det", "n_skipped", "pairs"):
        assert np.array_equal(dev[key], host[key]), key
    assert not dev["n_skipped"].any() and not dev["degenerate_obs"].any() and not dev["degenerate_det"].any() and not dev["dead_set"].any()
    ci, di = dev["pairs"][:, 0], dev["pairs"][:, 1]
    worst = 0.0
    for p, (lw_pe, lw_inj) in enumerate(c["lw"]):
        tol_r, tol_m = RU.set_tolerances(lw_pe, lw_inj, None, None)
        tol_rho = []
        for s, key in enumerate(("rho_obs", "rho_det")):
            r = host["rank_cov"][p, s]
            assert np.all(np.abs(dev["rank_cov"][p, s] - r) <= tol_r[s])
            tol_rho.append(RU.rho_tolerance(tol_r[s], r[ci, di], r[ci, ci], r[di, di]))
            assert np.all(np.abs(dev[key][p] - host[key][p]) <= tol_rho[s]), (p, key)
            worst = max(worst, float(np.max(np.abs(dev[key][p] - host[key][p]) / tol_rho[s])))
        assert np.all(np.abs(dev["delta"][p] - host["delta"][p]) <= tol_rho[0] + tol_rho[1])
        assert np.all(np.abs(dev["mean_rank"][p] - 0.5) <= (tol_m + RU.STATEMENT_MEAN_ROUNDING)[:, None])
    tol_m_all = max(RU.set_tolerances(lw_pe, lw_inj, None, None)[1].max() for lw_pe, lw_inj in c["lw"])
    assert dev["rank_mean_error"] <= tol_m_all + RU.STATEMENT_MEAN_ROUNDING and host["rank_mean_error"] <= RU.STATEMENT_MEAN_ROUNDING
    assert np.all(dev["variance_floor"] >= RU.set_tolerances(*c["lw"][0], None, None)[0])
    print(f"catalog_rank_correlation_check: largest |device - host| of a rho = {worst:.4f} of the propagated bound; rank_mean_error = {dev['rank_mean_error']:.3e} (device), "
          f"{host['rank_mean_error']:.3e} (host)")
