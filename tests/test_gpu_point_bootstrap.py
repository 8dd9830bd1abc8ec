"""GPU: bootstrap replicates of the inner importance sums on the device (include/gwi_engine.h: gwi_set_bootstrap, gwi_point_bootstrap;
gwinferno_amd/csrc/gwi_boot.h): counts and dead EQUAL to the statement (draws.point_bootstrap_reference on the engine's own
log-weights), (M, S) EQUAL to point_tails', the sums under the derived bound of tests/boot_util.py, the purity of the sums over splits of
the points and of the replicates, handles and the stage of 64 points, the absence of side effects on two existing entries, and
postprocess.likelihood_bootstrap on both backends.

Shapes (tests/tail_util.py), PL+Peak x PL-q x PL-z on seeded synthetic catalogs: 5 x 700 with 2 500 injections (every last tile ragged, the
last slice partly empty, three injection tiles) and 2 x 1 024 with 2 048 (every tile and slice full).  Two points under the default mass
bounds and one under an upper bound that cuts through every event and the injection set.  The statement is vetted without a device in
tests/test_boot_cpu.py.

The file's name keeps it behind tests/test_gpu_c_abi.py in the suite's order.  That file starts a plain C program that uses the GPU and,
two tests later, compares the device's free memory over a loop of engines; the memory of the finished program comes back a moment after
it has exited, and what has so far separated the two is the start-up of the GPU runtime in the test process itself, which a GPU test
module that runs earlier would take away."""
import re

import boot_util as BU
import numpy as np
import pytest
import tail_util as TU

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(shape="ragged"):
    """Per shape two engines, made once and shared: the default mass bounds with two points and the cut upper bound with one; their
    log-weights from the device, read-only."""
    if shape not in _CASES:
        comp, comp_cut = TU.composition(shape), TU.composition(shape, cut=True)
        eng, eng_cut = comp.engine(), comp_cut.engine()
        thetas, theta_cut = TU.points(comp, TU.N_FREE_POINTS), TU.points(comp_cut, 1)
        lw, lw_cut = [eng.log_weights(t) for t in thetas], [eng_cut.log_weights(t) for t in theta_cut]
        for a in [thetas, theta_cut] + [x for pair in lw + lw_cut for x in pair]:
            a.setflags(write=False)
        _CASES[shape] = dict(eng=eng, thetas=thetas, lw=lw, eng_cut=eng_cut, theta_cut=theta_cut, lw_cut=lw_cut, total=TU.catalog(shape)[2])
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
        c["eng_cut"].close()
    _CASES.clear()


def _same(a, b):
    """equal bits, NaN in the same places"""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def _boot(eng, thetas, n_rep, first=0, masks=(None, None), seed=BU.SEED):
    try:
        eng.set_draw_mask(*masks)
        eng.set_bootstrap(seed, n_rep, first)
        return eng.point_bootstrap(thetas)
    finally:
        eng.set_draw_mask()


def _ms_of_tails(eng, thetas, masks):
    try:
        eng.set_draw_mask(*masks)
        eng.set_tail_sizes(5, 7)
        return eng.point_tails(thetas)[2][..., :2]
    finally:
        eng.set_draw_mask()


def _against_the_statement(eng, thetas, lws, n_rep, masks):
    """counts and dead EQUAL to the statement on the engine's own log-weights, (M, S) EQUAL to point_tails', the sums under the derived
    bound.  Returns the largest deviation of a sum as a fraction of the bound."""
    from gwinferno_amd import draws as D

    sums, stats, dead, counts = _boot(eng, thetas, n_rep, masks=masks)
    k, n_ev = len(lws), eng.n_ev
    assert sums.shape == (k, n_ev + 1, n_rep) and stats.shape == (k, n_ev + 1, 2) and dead.shape == (k, n_ev + 1) and dead.dtype == np.int32
    assert counts.shape == (n_ev + 1, n_rep) and counts.dtype == np.int64
    assert np.array_equal(stats, _ms_of_tails(eng, thetas, masks))
    worst = 0.0
    for p, (lw_pe, lw_inj) in enumerate(lws):
        w_sums, w_stats, w_dead, w_counts = D.point_bootstrap_reference(lw_pe, lw_inj, masks, BU.SEED, n_rep)
        assert np.array_equal(counts, w_counts) and np.array_equal(dead[p], w_dead) and np.array_equal(stats[p][:, 0], w_stats[:, 0])
        for s in range(n_ev + 1):
            if w_dead[s]:
                assert np.all(np.isnan(sums[p, s])) and np.all(np.isnan(w_sums[s])) and dead[p, s] == 1
                continue
            tol = BU.sums_bound(TU.n_tiles_of(eng.n_pe if s < n_ev else eng.n_inj)) * w_sums[s]
            dev = np.abs(sums[p, s] - w_sums[s])
            frac = float(np.max(np.where(tol > 0.0, dev / np.where(tol > 0.0, tol, 1.0), np.where(dev > 0.0, np.inf, 0.0))))
            print(f"point {p}, segment {s}, B = {n_rep}: largest |device - statement| of a sum is {frac:.4f} of the bound; S {stats[p, s, 1]!r} vs {w_stats[s, 1]!r}")
            assert frac <= 1.0 and abs(stats[p, s, 1] - w_stats[s, 1]) <= TU.total_bound(int(np.count_nonzero(np.isfinite(lw_pe[s] if s < n_ev else lw_inj)))) * w_stats[s, 1]
            worst = max(worst, frac)
    return worst, dead


@pytest.mark.parametrize("case", ["free", "masked"])
@pytest.mark.parametrize("n_rep", BU.REPLICATES)
@pytest.mark.parametrize("shape", BU.SHAPES)
def test_device_against_the_statement(shape, n_rep, case):
    """Every shape, with and without masks (one event dead), B in (1, 5, 128, 260), K = 1 and the three points (the third under
    cut_mmax, on its engine): counts, dead and M equal in every bit, (M, S) the bits of point_tails, the sums within
    (1024 / 8 + 8 + n_tiles + 2) 2^-52 relative (boot_util.sums_bound), NaN sums and flag 1 for the dead segment."""
    c = _case(shape)
    masks = TU.masks(case, shape)
    w1, _ = _against_the_statement(c["eng"], c["thetas"][:1], c["lw"][:1], n_rep, masks)
    w2, dead = _against_the_statement(c["eng"], c["thetas"], c["lw"], n_rep, masks)
    w3, dead_cut = _against_the_statement(c["eng_cut"], c["theta_cut"], c["lw_cut"], n_rep, masks)
    n_ev, n_pe, n_inj = TU.SHAPES[shape]
    for lw_pe, lw_inj in c["lw_cut"]:
        assert all(0 < np.isfinite(lw_pe[e]).sum() < n_pe for e in range(n_ev)) and 0 < np.isfinite(lw_inj).sum() < n_inj
    want_dead = np.zeros(n_ev + 1, dtype=np.int32)
    if case == "masked":
        want_dead[TU.DEAD_EVENT] = 1
    assert np.all(dead == want_dead) and np.all(dead_cut == want_dead)
    print(f"{shape}, B = {n_rep}, {case}: largest fraction of the bound: {max(w1, w2, w3):.4f}")


def test_purity_over_points_replicates_handles_and_the_stage():
    """The bits of the sums (and of every other output) are the same for K = 3 in one call or in three; for B = 260 in one call or as
    first_replicate = 0 / 128 / 256 with 128 / 128 / 4 replicates (and for a first replicate inside a group of four); on two handles of
    one composition; and for one point before and after a 65-point call, which crosses the stage of 64 points."""
    c = _case()
    eng, masks = c["eng"], TU.masks("masked")
    thetas = np.concatenate([c["thetas"], c["thetas"][:1] * (1.0 + 1e-3)])
    for mk in ((None, None), masks):
        whole = _boot(eng, thetas, 260, masks=mk)
        assert _same(whole, _boot(eng, thetas, 260, masks=mk))
        parts = [_boot(eng, thetas[p : p + 1], 260, masks=mk) for p in range(3)]
        assert _same(whole[:3], [np.concatenate([q[i] for q in parts]) for i in range(3)]) and all(np.array_equal(q[3], whole[3]) for q in parts)
        split = [_boot(eng, thetas, n, first, masks=mk) for first, n in ((0, 128), (128, 128), (256, 4))]
        assert np.array_equal(whole[0], np.concatenate([q[0] for q in split], axis=2), equal_nan=True) and np.array_equal(whole[3], np.concatenate([q[3] for q in split], axis=1))
        assert all(_same(whole[1:3], q[1:3]) for q in split)
        odd = _boot(eng, thetas, 7, 253, masks=mk)
        assert np.array_equal(odd[0], whole[0][..., 253:260], equal_nan=True) and np.array_equal(odd[3], whole[3][:, 253:260])
    free = _boot(eng, thetas, 260)
    assert not np.array_equal(free[0][0], free[0][2])  # (the third point is another point)
    eng2 = TU.composition().engine()
    try:
        assert _same(free, _boot(eng2, thetas, 260))
    finally:
        eng2.close()
    before = _boot(eng, thetas[:1], 128)
    rows = np.repeat(np.arange(3), 22)[:65]
    many, ref = _boot(eng, thetas[rows], 128), _boot(eng, thetas, 128)
    assert _same(many[:3], [x[rows] for x in ref[:3]]) and np.array_equal(many[3], ref[3])
    assert _same(before, _boot(eng, thetas[:1], 128)) and np.array_equal(before[0][0], many[0][0])
    assert not np.array_equal(_boot(eng, thetas[:1], 128, seed=BU.SEED + 1)[3], before[3])  # another seed, other counts


def test_nothing_else_moved():
    """weighted_histograms and point_tails return the same bits before and after a point_bootstrap call on the same handle."""
    from gwinferno_amd import draws as D

    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = TU.RU.columns(3)
    edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.02, 0.98, 17)) for p, i in zip(x_pe, x_inj)]
    eng.set_histogram_bins(np.stack([D.digitize(p, e) for p, e in zip(x_pe, edges)]), np.stack([D.digitize(i, e) for i, e in zip(x_inj, edges)]), n_bins=16)
    eng.set_tail_sizes(37, 671)

    def existing():
        return list(eng.weighted_histograms(thetas)) + list(eng.point_tails(thetas))

    before = existing()
    boot = _boot(eng, thetas, 128)
    assert _same(before, existing()) and _same(boot, _boot(eng, thetas, 128))


def test_likelihood_bootstrap_on_both_backends():
    """likelihood_bootstrap on the device and on the host (the statement on eng.log_weights), B = 64, free and with the masks that leave
    one event dead: every returned array within the bound of the sums carried through the logarithms (2 bounds per logBF replicate --
    A and S --, summed over the events and N_obs times for log mu), n_dead and the NaN pattern equal, and log_l within 1e-10 relative of
    evaluate_batch's uncut sum logBF - N_obs log mu."""
    from gwinferno_amd import postprocess as P

    c = _case()
    eng, thetas, total = c["eng"], c["thetas"], c["total"]
    n_ev, n_pe, n_inj = TU.SHAPES["ragged"]
    for mk in (None, TU.masks("masked")):
        try:
            dev = P.likelihood_bootstrap(eng, thetas, total, n_replicates=64, seed=BU.SEED, backend="device", masks=mk)
        finally:
            eng.set_draw_mask()
        host = P.likelihood_bootstrap(eng, thetas, total, n_replicates=64, seed=BU.SEED, backend="host", masks=mk)
        assert dev["n_dead"] == host["n_dead"] == (0 if mk is None else len(thetas)) and np.array_equal(dev["counts"], host["counts"]) and np.array_equal(dev["c_miss"], host["c_miss"])
        per_bf = 2.0 * BU.log_bound(max(BU.sums_bound(TU.n_tiles_of(n_pe)), TU.total_bound(n_pe)))
        per_mu = 2.0 * BU.log_bound(max(BU.sums_bound(TU.n_tiles_of(n_inj)), TU.total_bound(n_inj)))
        tol_l = n_ev * per_bf + n_ev * per_mu  # (N_obs = n_ev)
        scale = {"log_bf_rep": per_bf, "log_mu_rep": per_mu, "log_l_rep": tol_l, "log_bf": per_bf, "log_mu": per_mu, "log_l": tol_l}
        for key, tol in scale.items():
            a, b = dev[key], host[key]
            assert np.array_equal(np.isnan(a), np.isnan(b)), key
            ok = ~np.isnan(b)
            worst = float(np.max(np.abs(a[ok] - b[ok]) - U_ABS * np.abs(b[ok]))) if ok.any() else 0.0
            print(f"masks {'free' if mk is None else 'masked'}: {key}: largest |device - host| beyond the rounding of the value itself {worst:.3e}, bound {tol:.3e}")
            assert worst <= tol, key
        # the moments over B replicates of values within tol of each other: a standard deviation moves by at most 2 tol, a mean by tol
        for key, tol in (("std_log_l", 2 * tol_l), ("bias_log_l", 2 * tol_l), ("std_log_bf", 2 * per_bf), ("std_log_mu", 2 * per_mu), ("delta_std", 4 * tol_l)):
            a, b = dev[key], host[key]
            assert np.array_equal(np.isnan(a), np.isnan(b)), key
            ok = ~np.isnan(b)
            if ok.any():
                assert float(np.max(np.abs(a[ok] - b[ok]))) <= tol + 64 * BU.U * float(np.max(np.abs(host["log_l"][~np.isnan(host["log_l"])]), initial=1.0)), key
        if mk is None:
            assert np.allclose(dev["corr"], host["corr"], rtol=0.0, atol=1e-6) and np.all(np.isfinite(dev["std_log_l"])) and np.all(dev["delta_std"].diagonal() == 0.0)
            res = eng.evaluate_batch(thetas, total, min_neff_cut=False, max_variance_cut=False, want_grad=False)
            want = np.array([np.sum(r.log_bfs) - n_ev * r.summary.log_det_eff for r in res])
            print(f"log_l {dev['log_l']!r} against evaluate_batch {want!r}")
            assert np.all(np.abs(dev["log_l"] - want) <= 1e-10 * np.abs(want))
            assert np.array_equal(dev["variance_log_likelihood"], [r.summary.variance_log_likelihood for r in res])
        else:
            assert np.all(np.isnan(dev["log_l_rep"])) and np.all(dev["n_nan_replicates"] == 64) and np.all(np.isfinite(np.delete(dev["std_log_bf"], TU.DEAD_EVENT, axis=1)))


U_ABS = 4.0 * BU.U  # the additions that assemble a value (M + log, the sum over the events) round relative to the value itself


def test_refusals_on_the_device():
    """A call before the setting, settings out of range, null outputs and k < 1: GWI_ERR_INVALID in the words of bad_point_args and of the
    setter, and nothing is written."""
    import ctypes as C

    from gwinferno_amd import _native as N

    eng = TU.composition().engine()
    try:
        theta = _case()["thetas"][0]
        with pytest.raises(N.NativeEngineError, match=r"gwi_point_bootstrap: no replicates are set \(gwi_set_bootstrap\)"):
            eng.point_bootstrap(theta)
        lib = eng.lib
        for (n, first), why in (((0, 0), "n_replicates = 0 is not in 1 ... 1024"), ((1025, 0), "n_replicates = 1025 is not in 1 ... 1024"), ((4, -1), "first_replicate = -1 is negative"),
                                ((4, (1 << 20) - 3), "first_replicate \\+ n_replicates exceeds 1048576")):
            assert lib.gwi_set_bootstrap(eng.handle, 1, n, first) == -1
            assert re.search("gwi_set_bootstrap: .*" + why, lib.gwi_last_error(eng.handle).decode())
        with pytest.raises(N.NativeEngineError, match="no replicates are set"):  # (a refused setting sets nothing)
            eng.point_bootstrap(theta)
        eng.set_bootstrap(3, 4, (1 << 20) - 4)
        n = eng.n_ev + 1
        sums, stats, dead, counts = np.full((1, n, 4), 7.0), np.full((1, n, 2), 7.0), np.full((1, n), 7, dtype=np.int32), np.full((n, 4), 7, dtype=np.int64)
        args = [N.as_dp(sums), N.as_dp(stats), dead.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_int64))]
        for i, name in enumerate(("sums", "stats", "dead", "counts")):
            assert lib.gwi_point_bootstrap(eng.handle, N.as_dp(theta), 1, *[None if j == i else a for j, a in enumerate(args)]) == -1
            assert f"gwi_point_bootstrap: {name} is null" in lib.gwi_last_error(eng.handle).decode()
        for th, k in ((N.as_dp(theta), 0), (None, 1)):
            assert lib.gwi_point_bootstrap(eng.handle, th, k, *args) == -1 and "gwi_point_bootstrap: thetas is null or k < 1" in lib.gwi_last_error(eng.handle).decode()
        assert np.all(sums == 7.0) and np.all(stats == 7.0) and np.all(dead == 7) and np.all(counts == 7)
        assert lib.gwi_point_bootstrap(eng.handle, N.as_dp(theta), 1, *args) == 0 and np.all(sums > 0.0) and np.all(dead == 0) and np.all(counts > 0)
    finally:
        eng.close()
