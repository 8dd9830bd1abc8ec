"""No device: the NumPy statement of the per-point tails (gwinferno_amd/draws.py: tails_segment, point_tails_reference,
tail_cutoff_and_rest, pareto_tail_fit) against a brute-force loop, the fit against pareto_smooth in bits, the bookkeeping of
postprocess.importance_sum_diagnostics(backend="host"), the derived bounds of tests/tail_util.py and the exports."""
import math
import os
import re

import numpy as np
import pytest
import tail_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_segment(lw, mask, m):
    from gwinferno_amd import draws as D

    tail, stats, counts = D.tails_segment(lw, mask, m)
    b_tail, b_stats, b_counts = TU.brute_segment(lw, mask, m)
    assert tail.shape == (m,) and np.array_equal(tail, np.array(b_tail)) and np.array_equal(counts, np.array(b_counts, dtype=np.int32)) and counts.dtype == np.int32
    assert np.array_equal(stats[[0, 3]], np.array(b_stats)[[0, 3]])
    for got, want in zip(stats[1:3], b_stats[1:3]):  # (two exact sums of the same weights, each rounded once)
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 2.0 * TU.U * abs(want)
    return tail, stats, counts


def test_statement_against_a_loop():
    """tails_segment against repeated removal of the maximum: random values of both signs with NaN, +inf and -inf among them, with and
    without a mask, at m = 1, a few, and n - 1; the sum outside the tail and the cut-off derived from the rows."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(5)
    lw = rng.normal(size=120) * 40.0
    lw[[3, 50]], lw[[7, 90]], lw[[11, 12, 13]] = np.nan, np.inf, -np.inf
    assert (lw[np.isfinite(lw)] > 0).any() and (lw[np.isfinite(lw)] < 0).any()
    mask = (rng.uniform(size=120) < 0.7).astype(np.uint8)
    for m in (1, 5, 37, 119):
        for mk in (None, mask):
            tail, stats, counts = _check_segment(lw, mk, m)
            live = np.sort(lw[np.isfinite(lw) & (np.ones(120, bool) if mk is None else mk.astype(bool))])
            cutoff, rest = D.tail_cutoff_and_rest(tail, stats, counts)
            if live.size > m:
                assert cutoff == live[-m - 1]
                want = math.fsum(np.exp(live[:-m] - live[-1]).tolist())
                assert abs(rest - want) <= 4.0 * TU.U * want
            else:
                assert counts[1] == live.size and counts[2] == 0 and rest == 0.0 and cutoff == -np.inf and np.all(tail[: m - live.size] == -np.inf)


def test_ties_short_and_dead_segments():
    """Ties straddling the cut-off: the tail holds m - n_gt copies of v*, n_gt + n_eq > m and the derived cut-off is v*.  A segment with
    exactly m and with fewer live samples; a dead one (all masked; all -inf); -0.0 and +0.0 tie."""
    from gwinferno_amd import draws as D

    lw = np.repeat(np.array([-3.5, 2.0, 0.25, -1.0, 7.0, 0.25, 0.25]), 2)  # three pairs tie at 0.25
    tail, stats, counts = _check_segment(lw, None, 5)
    assert np.array_equal(tail, [0.25, 2.0, 2.0, 7.0, 7.0]) and tuple(counts) == (14, 4, 6, 0) and stats[3] == -1.0
    cutoff, rest = D.tail_cutoff_and_rest(tail, stats, counts)
    assert cutoff == 0.25 and abs(rest - (2 * math.exp(-10.5) + 2 * math.exp(-8.0) + 5 * math.exp(0.25 - 7.0))) < 1e-15
    tail, stats, counts = _check_segment(lw, None, 3)  # the tie at 7 and one of the two 2s: v* = 2 with one copy outside
    assert np.array_equal(tail, [2.0, 7.0, 7.0]) and tuple(counts) == (14, 2, 2, 0) and D.tail_cutoff_and_rest(tail, stats, counts)[0] == 2.0
    for n_keep in (5, 2):
        mask = np.zeros(14, dtype=np.uint8)
        mask[:n_keep] = 1
        tail, stats, counts = _check_segment(lw, mask, 5)
        assert counts[0] == n_keep and np.all(tail[: 5 - n_keep] == -np.inf) and np.all(np.isfinite(tail[5 - n_keep:])) and counts[3] == 0
        assert D.tail_cutoff_and_rest(tail, stats, counts)[1] == 0.0
    for dead_lw, mk in ((lw, np.zeros(14, dtype=np.uint8)), (np.full(14, -np.inf), None), (np.full(14, np.nan), None)):
        tail, stats, counts = _check_segment(dead_lw, mk, 4)
        assert np.all(tail == -np.inf) and tuple(counts) == (0, 0, 0, 1) and math.isnan(stats[2]) and stats[3] == -np.inf
        assert math.isnan(D.tail_cutoff_and_rest(tail, stats, counts)[1])
    tail, stats, counts = _check_segment(np.array([-0.0, 0.0, -1.0, -0.0]), None, 2)
    assert np.array_equal(tail, [0.0, 0.0]) and tuple(counts) == (4, 0, 3, 0)


def test_point_layout_and_refusals():
    """point_tails_reference lays the segments out as the device does and refuses sizes the device refuses."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(6)
    lw_pe, lw_inj = rng.normal(size=(3, 40)), rng.normal(size=90)
    mask_pe, mask_inj = np.ones((3, 40), dtype=np.uint8), (np.arange(90) % 2).astype(np.uint8)
    mask_pe[1] = 0
    tail_pe, tail_inj, stats, counts = D.point_tails_reference(lw_pe, lw_inj, mask_pe, mask_inj, 7, 11)
    assert tail_pe.shape == (3, 7) and tail_inj.shape == (11,) and stats.shape == (4, 4) and counts.shape == (4, 4) and counts.dtype == np.int32
    assert np.array_equal(tail_pe[2], np.sort(lw_pe[2])[-7:]) and np.array_equal(tail_inj, np.sort(lw_inj[1::2])[-11:]) and np.array_equal(counts[:, 3], [0, 1, 0, 0])
    for bad in ((0, 5), (5, 0), (40, 5), (5, 90), (D.MAX_TAIL + 1, 5)):
        with pytest.raises(ValueError, match="tail size"):
            D.point_tails_reference(lw_pe, lw_inj, None, None, *bad)
    assert D.psis_tail_size(5000) == 213 and D.psis_tail_size(50_000) == 671 and D.psis_tail_size(20) == 4


@pytest.mark.parametrize("n,df", [(400, 2.0), (1000, 5.0), (5000, 4.0), (64, 3.0)])
def test_fit_has_the_bits_of_pareto_smooth(n, df):
    """pareto_tail_fit on a column's own tail (m by the rule), cut-off and maximum: khat and the smoothed values are pareto_smooth's in
    every bit, and the entries outside the tail keep theirs."""
    from gwinferno_amd import draws as D

    col = np.random.default_rng(n).standard_t(df, size=n) * 1.7 + 3.0
    want, khat = D.pareto_smooth(col[:, None])
    m = D.psis_tail_size(n)
    order = np.argsort(col, kind="stable")
    got_k, smoothed = D.pareto_tail_fit(col[order[n - m:]], col[order[n - m - 1]], col.max())
    assert np.isfinite(got_k) and got_k == khat[0] and np.array_equal(smoothed, want[order[n - m:], 0])
    assert np.array_equal(want[order[: n - m], 0], col[order[: n - m]] - col.max())


def test_fit_gives_inf_where_nothing_is_smoothed():
    """m < 5, a constant tail, a lowest quarter that ties with the cut-off: khat = inf and the tail comes back shifted, not smoothed."""
    from gwinferno_amd import draws as D

    for tail, cutoff in ((np.array([1.0, 2.0, 3.0, 4.0]), 0.5), (np.full(8, 2.0), 1.0), (np.array([1.0, 1.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), 1.0)):
        khat, smoothed = D.pareto_tail_fit(tail, cutoff, tail[-1])
        assert khat == np.inf and np.array_equal(smoothed, tail - tail[-1])
    khat, _ = D.pareto_tail_fit(np.array([1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0, 9.0]), 0.5, 9.0)
    assert np.isfinite(khat)


def test_diagnostics_bookkeeping_on_the_host():
    """importance_sum_diagnostics(backend="host") on a hand-made case of three points: a heavy-tailed event, a light-tailed one, an event
    that is dead at one point and short (n_live <= m) at another.  Skipped segments are counted and never fitted; the shares are weighted;
    the worst point is the one with the largest khat; neff is a lower bound of the exact one and exact where nothing lies below the tail;
    log_sum_raw is the log of the plain sum."""
    from gwinferno_amd import postprocess as P

    rng = np.random.default_rng(8)
    k, n_pe, n_inj = 3, 400, 900
    lw_pe = [np.stack([rng.standard_cauchy(n_pe) * 3.0, rng.normal(size=n_pe) * 0.3, rng.normal(size=n_pe)]) for _ in range(k)]
    lw_inj = [rng.normal(size=n_inj) for _ in range(k)]
    lw_pe[1][2] = -np.inf
    lw_pe[2][2, 30:] = np.nan  # 30 live samples <= m_pe = 60
    eng = TU.RU.StubEngine(lw_pe, lw_inj)
    thetas = np.arange(k, dtype=np.float64)[:, None]
    r = P.importance_sum_diagnostics(eng, thetas, backend="host")
    assert r["m_pe"] == 60 and r["m_inj"] == 90 and r["n_points"] == 3 and r["pareto_k"].shape == (3, 4)
    assert np.array_equal(r["skipped"], [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]]) and np.array_equal(r["n_skipped"], [0, 0, 2, 0])
    assert np.array_equal(np.isnan(r["pareto_k"]), r["skipped"]) and np.array_equal(np.isnan(r["log_sum_psis"]), r["skipped"])
    assert np.array_equal(r["n_live"], [[400, 400, 400, 900], [400, 400, 0, 900], [400, 400, 30, 900]])
    assert np.all(r["pareto_k"][:, 0] > 0.7) and np.all(r["pareto_k"][:, 1] < 0.5)  # Cauchy log-weights; a narrow normal
    assert np.array_equal(r["share_above_0.7"][:2], [1.0, 0.0]) and np.array_equal(r["share_above_0.5"][:2], [1.0, 0.0])
    assert r["worst_point"][0] == int(np.argmax(r["pareto_k"][:, 0])) and r["worst_k"][0] == r["pareto_k"][:, 0].max() and r["worst_point"][2] == 0
    assert math.isnan(r["neff"][1, 2]) and math.isnan(r["log_sum_raw"][1, 2]) and r["neff"][2, 2] == pytest.approx(r["neff_exact"][2, 2], rel=1e-13)
    ok = ~np.isnan(r["neff_exact"])
    assert np.all(r["neff"][ok] <= r["neff_exact"][ok] * (1 + 1e-12)) and np.all(r["neff"][ok] >= 1.0)
    assert np.allclose(r["neff"][:, 0], r["neff_exact"][:, 0], rtol=1e-6, atol=0.0)  # (the heavy tail holds the squares)
    for p in range(k):
        for s in range(4):
            lw = lw_pe[p][s] if s < 3 else lw_inj[p]
            lw = lw[np.isfinite(lw)]
            if lw.size:
                assert r["log_sum_raw"][p, s] == pytest.approx(lw.max() + math.log(math.fsum(np.exp(lw - lw.max()).tolist())), abs=1e-12)
    assert np.all(np.abs(r["log_sum_diff"][:, 1]) < 0.05) and np.array_equal(r["log_sum_diff"], r["log_sum_psis"] - r["log_sum_raw"], equal_nan=True)
    # weights: a point with weight 0 does not count in the shares
    w = np.array([1.0, 0.0, 3.0])
    above = r["pareto_k"][:, 3] > 0.5
    rw = P.importance_sum_diagnostics(eng, thetas, point_weights=w, backend="host")
    assert rw["share_above_0.5"][3] == pytest.approx((w * above).sum() / w.sum()) and rw["share_above_0.5"][2] == pytest.approx(float(r["pareto_k"][0, 2] > 0.5))
    with pytest.raises(ValueError, match="point_weights"):
        P.importance_sum_diagnostics(eng, thetas, point_weights=np.zeros(3), backend="host")
    with pytest.raises(ValueError, match="backend"):
        P.importance_sum_diagnostics(eng, thetas, backend="eager")
    # explicit sizes; the tail's own values come back
    r5 = P.importance_sum_diagnostics(eng, thetas[:1], m_pe=5, m_inj=7, backend="host")
    assert r5["tail_pe"].shape == (1, 3, 5) and np.array_equal(r5["tail_inj"][0], np.sort(lw_inj[0])[-7:])


def test_the_catalogs_and_the_bounds():
    """The seeds give what the GPU file relies on: an upper mass bound inside every event's samples; the tie catalog's pairs are copies;
    the bounds are the derived ones, far below any tolerance a fit would pick."""
    for shape, (n_ev, n_pe, n_inj) in TU.SHAPES.items():
        pe, inj, _ = TU.catalog(shape)
        cut = TU.cut_mmax(shape)
        above = (pe["mass_1"] > cut).mean(axis=1)
        assert pe["mass_1"].shape == (n_ev, n_pe) and np.all(above > 0.09) and np.all(above < 0.91) and 0.0 < (inj["mass_1"] > cut).mean() < 1.0
        assert max(TU.M_PE) < n_pe and (max(TU.M_INJ) < n_inj or shape == "full") and n_pe % 2 == 0 and n_inj % 2 == 0
    assert TU.SHAPES["long"][2] > TU.M_LONG and TU.n_tiles_of(2500) == 3 and TU.n_tiles_of(700) == 1 and TU.n_tiles_of(2048) == 2
    pe, inj, _ = TU.catalog("ragged", True)
    assert all(np.array_equal(d[key][..., 0::2], d[key][..., 1::2]) for d in (pe, inj) for key in d)
    assert TU.body_bound(3) == 1.01 * TU.U * (2.0 + 0.5 * 16) and TU.body_bound(5) < 3e-15 and TU.total_bound(700) == 708 * TU.U
    assert TU.log_sum_bound(1e-15, 2.0, 10.0) < 1e-14


def test_header_library_and_refusals_without_a_device():
    """The three exports are declared, bound and listed, with their argument counts; a null handle and a host-only handle answer
    GWI_ERR_INVALID, the latter with a message, and write nothing; the Python layer refuses an engine that holds a shard in the words of
    its neighbours and a call before the sizes are set."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym, n_args in (("gwi_set_tail_sizes", 3), ("gwi_point_tails", 6), ("gwi_point_tail_times", 4)):
        assert sym in N.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n_args
    assert lib.gwi_point_tails.restype is C.c_int32 and lib.gwi_set_tail_sizes.restype is C.c_int32 and lib.gwi_point_tail_times.restype is None
    assert "DESIGN 8m" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_point_tails(None, None, 1, None, None, None) == -1 and lib.gwi_set_tail_sizes(None, 1, 1) == -1
    comp = TU.composition("ragged", device=N.DEVICE_HOST_ONLY)
    eng = comp.engine()
    try:
        i32 = C.POINTER(C.c_int32)
        tail, stats, counts = np.full((1, 12), 7.0), np.full((1, eng.n_ev + 1, 4), 7.0), np.full((1, eng.n_ev + 1, 4), 7, dtype=np.int32)
        assert lib.gwi_point_tails(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, N.as_dp(tail), N.as_dp(stats), counts.ctypes.data_as(i32)) == -1
        assert "gwi_point_tails: host-only handle: no device to select on" in lib.gwi_last_error(eng.handle).decode()
        assert np.all(tail == 7.0) and np.all(stats == 7.0) and np.all(counts == 7)
        ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
        lib.gwi_point_tail_times(*[C.byref(m) for m in ms], C.byref(n_launch))
        assert n_launch.value == 0 and all(m.value == 0.0 for m in ms)
        with pytest.raises(N.NativeEngineError, match="gwi_set_tail_sizes: host-only handle: no device to keep a tail on"):
            eng.set_tail_sizes()
        with pytest.raises(ValueError, match="thetas has shape"):
            eng.point_tails(np.zeros(eng.n_theta + 1))
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_tails: this engine holds one shard of the catalog; the injection tail needs the global set"):
        shard.point_tails(np.zeros(3))
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: set_tail_sizes: this engine holds one shard"):
        shard.set_tail_sizes()
