"""CPU: per-point joint histograms (include/gwi_engine.h: gwi_point_histograms2d; gwinferno_amd/csrc/gwi_hist2d.h) -- the NumPy
statement (gwinferno_amd/draws.py: point_histograms2d_reference, joint_table_summaries) against a plain double loop and against
np.histogram2d on the raw values, the band and tail logic of postprocess.joint_check_summaries on hand-made tables, the inputs of
tests/test_gpu_hist2d.py vetted from the host evaluation, and the header / binding / refusals that need no device."""
import os
import re

import hist2d_util as HU
import hist_util as U
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_point(seed):
    rng = np.random.default_rng(seed)
    lw_pe, lw_inj = rng.normal(0.0, 3.0, (U.N_EV, U.N_PE)), rng.normal(0.0, 3.0, U.N_INJ)
    lw_pe[0, 5], lw_pe[2, 7], lw_inj[3] = -np.inf, np.nan, np.inf  # samples without weight
    return lw_pe, lw_inj


@pytest.mark.parametrize("case", U.MASK_CASES)
@pytest.mark.parametrize("n_bins", HU.N_BINS)
def test_statement_against_a_double_loop_and_histogram2d(n_bins, case):
    """Every cell of every segment: membership (which cells hold anything) equal to a plain loop over the samples and to
    np.histogram2d(weights=) on the raw values; the sums under hist_util.bound; a sample outside in either coordinate is in no cell but
    in S; obs is the mean over the live events, pred the injection set's table, dead segments counted."""
    from gwinferno_amd.draws import OUTSIDE_BIN, draw_weights, point_histograms2d_reference

    lw_pe, lw_inj = _random_point(5)
    pb, ib = HU.bins(n_bins)
    pm, im = U.masks(case)
    e = HU.edges(n_bins)
    pe, inj, _ = U.catalog()
    got = point_histograms2d_reference(lw_pe, lw_inj, pm, im, pb, ib, n_bins, HU.PAIRS)
    assert got["hist_pe"].shape == (U.N_EV, 2, n_bins, n_bins) and got["hist_inj"].shape == (2, n_bins, n_bins) and got["vsum"] is None
    n_live_events = 0
    total_obs = np.zeros((2, n_bins, n_bins))
    for seg, (lw, mask) in enumerate(U.segments(lw_pe, lw_inj, pm, im)):
        w = draw_weights(lw, mask)
        live = int(np.count_nonzero(w > 0.0))
        table = got["hist_pe"][seg] if seg < U.N_EV else got["hist_inj"]
        if live == 0:
            assert got["n_dead"][seg] == 1 and not table.any()
            continue
        assert got["n_dead"][seg] == 0
        n_live_events += seg < U.N_EV
        s = float(np.sum(w))
        for r, (cx, cy) in enumerate(HU.PAIRS):
            codes = (pb[cx, seg], pb[cy, seg]) if seg < U.N_EV else (ib[cx], ib[cy])
            raw = [(pe if seg < U.N_EV else inj)[HU.COLUMNS[c]] for c in (cx, cy)]
            raw = [v[seg] if seg < U.N_EV else v for v in raw]
            loop, outside = np.zeros((n_bins, n_bins)), 0.0
            for i in range(w.size):
                if codes[0][i] == OUTSIDE_BIN or codes[1][i] == OUTSIDE_BIN:
                    outside += w[i]
                else:
                    loop[codes[0][i], codes[1][i]] += w[i]
            h2d = np.histogram2d(raw[0], raw[1], bins=[e[HU.COLUMNS[cx]], e[HU.COLUMNS[cy]]], weights=w)[0]
            tol = U.bound(live)
            assert np.array_equal(table[r] > 0.0, loop > 0.0) and np.array_equal(table[r] > 0.0, h2d > 0.0)
            assert np.all(np.abs(table[r] - loop / s) <= tol * (loop / s)) and np.all(np.abs(table[r] - h2d / s) <= tol * (h2d / s))
            # outside every cell, inside S (an event's samples cluster and the pooled edges may hold them all; the injections spread out)
            assert (outside > 0.0 or seg < U.N_EV) and abs((1.0 - table[r].sum()) - outside / s) <= 2.0 * tol
        if seg < U.N_EV:
            total_obs += table
    assert np.array_equal(got["live"], [n_live_events, 1]) and n_live_events == (2 if case == "masked" else 3)
    assert np.allclose(got["obs"], total_obs / n_live_events, rtol=1e-15, atol=0.0) and np.array_equal(got["pred"], got["hist_inj"])


def test_statement_weights_and_sets_left_out():
    """v = 1 gives the bits of v = None; v = 0 adds nothing and is not counted dead; a fractional v scales the sums and leaves obs / pred;
    a set without bins gives None sums and NaN rows; bad arguments are refused."""
    from gwinferno_amd.draws import point_histograms2d_reference as ref

    lw_pe, lw_inj = _random_point(6)
    pb, ib = HU.bins(7)
    pm, im = U.masks("masked")
    plain = ref(lw_pe, lw_inj, pm, im, pb, ib, 7, HU.PAIRS)
    ones = ref(lw_pe, lw_inj, pm, im, pb, ib, 7, HU.PAIRS, v=np.ones(U.N_EV + 1))
    for key in ("hist_pe", "hist_inj", "obs", "pred", "live", "n_dead"):
        assert np.array_equal(plain[key], ones[key], equal_nan=True), key
    assert np.array_equal(ones["vsum"], [1.0, 0.0, 1.0, 1.0]) and np.array_equal(plain["n_dead"], [0, 1, 0, 0])
    v = np.array([0.25, 0.0, 0.0, 0.5])
    part = ref(lw_pe, lw_inj, pm, im, pb, ib, 7, HU.PAIRS, v=v)
    assert np.array_equal(part["hist_pe"][0], 0.25 * plain["hist_pe"][0]) and not part["hist_pe"][1:].any() and np.array_equal(part["hist_inj"], 0.5 * plain["hist_inj"])
    assert np.array_equal(part["n_dead"], [0, 0, 0, 0]) and np.array_equal(part["vsum"], [0.25, 0.0, 0.0, 0.5])
    assert np.array_equal(part["obs"], plain["obs"]) and np.array_equal(part["pred"], plain["pred"]) and np.array_equal(part["live"], plain["live"])
    only_pe, only_inj = ref(lw_pe, lw_inj, pm, im, pb, None, 7, HU.PAIRS), ref(lw_pe, lw_inj, pm, im, None, ib, 7, HU.PAIRS)
    assert only_pe["hist_inj"] is None and np.all(np.isnan(only_pe["pred"])) and np.array_equal(only_pe["obs"], plain["obs"]) and np.array_equal(only_pe["live"], [2, 0])
    assert only_inj["hist_pe"] is None and np.all(np.isnan(only_inj["obs"])) and np.array_equal(only_inj["pred"], plain["pred"]) and np.array_equal(only_inj["live"], [0, 1])
    assert not only_inj["n_dead"].any()  # a set that is left out is not counted
    for bad in (dict(pairs=[(0, 3)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 1)] * 9), dict(pairs=np.zeros((0, 2))), dict(n_bins=65), dict(v=[2.0, 0, 0, 0])):
        kw = dict(pairs=HU.PAIRS, n_bins=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            ref(lw_pe, lw_inj, pm, im, pb, ib, kw.pop("n_bins"), kw.pop("pairs"), **kw)
    with pytest.raises(ValueError):
        ref(lw_pe, lw_inj, pm, im, None, None, 7, HU.PAIRS)


@pytest.mark.parametrize("n_bins", (2, 7, 64))
def test_joint_table_summaries(n_bins):
    """A product table has no mutual information (below 1e-15 B^2); a diagonal table of B equal cells has log B (to 4 2^-52 B); an all-zero
    table gives NaN; the marginals and the outside share are those of the renormalised table."""
    from gwinferno_amd.draws import joint_table_summaries

    rng = np.random.default_rng(n_bins)
    px, py = rng.dirichlet(np.ones(n_bins)), rng.dirichlet(np.ones(n_bins))
    product = 0.8 * np.outer(px, py)
    s = joint_table_summaries(product)
    assert abs(s["mi"]) < 1e-15 * n_bins**2 and abs(s["outside"] - 0.2) < 1e-15 * n_bins**2 and np.allclose(s["px"], px, rtol=1e-14) and np.allclose(s["py"], py, rtol=1e-14)
    diagonal = np.diag(np.full(n_bins, 0.5 / n_bins))
    s = joint_table_summaries(diagonal)
    assert abs(s["mi"] - np.log(n_bins)) <= 4 * 2.0**-52 * n_bins and abs(s["total"] - 0.5) < 1e-15
    stack = joint_table_summaries(np.stack([product, np.zeros((n_bins, n_bins)), diagonal]))
    assert stack["mi"].shape == (3,) and np.isnan(stack["mi"][1]) and np.all(np.isnan(stack["px"][1])) and stack["outside"][1] == 1.0
    assert stack["mi"][2] == s["mi"]
    with pytest.raises(ValueError):
        joint_table_summaries(np.zeros((3, 4)))


def test_band_and_tail_logic_on_hand_made_tables():
    """joint_check_summaries on five points of one pair with B = 2: delta, its bands (values of the input: the inverted-CDF rule), the
    share of points with delta > 0 and its two-sided form, tv and the mutual informations; a point without a live event and one with a
    dead injection set are skipped and counted, never divided; point weights move the shares."""
    from gwinferno_amd import postprocess as P
    from gwinferno_amd.draws import joint_table_summaries

    k = 5
    obs, pred = np.empty((k, 1, 2, 2)), np.empty((k, 1, 2, 2))
    for p in range(k):
        obs[p, 0] = [[0.1 + 0.05 * p, 0.2], [0.3, 0.1]]
        pred[p, 0] = [[0.2, 0.2 - 0.01 * p], [0.25, 0.15]]
    live = np.array([[3, 1]] * k, dtype=np.int32)
    live[1], live[3] = (0, 1), (3, 0)
    obs[1], pred[3] = np.nan, np.nan
    out = P.joint_check_summaries(obs, pred, live)
    used = [0, 2, 4]
    assert out["n_skipped"] == 2 and out["n_skipped_no_event"] == 1 and out["n_skipped_dead_injections"] == 1 and out["n_points"] == k
    assert np.all(np.isnan(out["delta"][[1, 3]])) and np.all(np.isnan(out["tv"][[1, 3]])) and np.all(np.isnan(out["mi_obs"][[1, 3]])) and np.all(np.isnan(out["pred"][1]))
    assert np.array_equal(out["delta"][used], obs[used] - pred[used])
    # cell [0, 0]: delta = -0.1, 0.0, 0.1 at the used points; [0, 1]: 0, 0.02, 0.04; [1, 0]: 0.05 each; [1, 1]: -0.05 each
    assert np.allclose(out["p_delta_positive"][0], [[1 / 3, 2 / 3], [1.0, 0.0]]) and np.allclose(out["p_two_sided"][0], [[2 / 3, 2 / 3], [0.0, 0.0]])
    assert np.array_equal(out["bands_delta"][:, 0, 0, 0], [out["delta"][0, 0, 0, 0], out["delta"][2, 0, 0, 0], out["delta"][4, 0, 0, 0]])
    for p in used:
        o, q = obs[p, 0] / obs[p, 0].sum(), pred[p, 0] / pred[p, 0].sum()
        assert abs(out["tv"][p, 0] - 0.5 * np.abs(o - q).sum()) < 1e-15
        assert out["mi_obs"][p, 0] == joint_table_summaries(obs[p, 0])["mi"] and out["delta_mi"][p, 0] == out["mi_obs"][p, 0] - out["mi_pred"][p, 0]
    assert out["bands_tv"].shape == (3, 1) and out["bands_delta_mi"].shape == (3, 1) and np.all(np.isfinite(out["bands_tv"]))
    weighted = P.joint_check_summaries(obs, pred, live, point_weights=[1.0, 5.0, 0.0, 5.0, 3.0])  # points 0 and 4 count, 1 : 3
    assert np.allclose(weighted["p_delta_positive"][0], [[0.75, 0.75], [1.0, 0.0]])
    for bad in (dict(point_weights=np.ones(k + 1)), dict(point_weights=-np.ones(k)), dict(levels=(101,))):
        with pytest.raises(ValueError):
            P.joint_check_summaries(obs, pred, live, **bad)
    with pytest.raises(ValueError):
        P.joint_check_summaries(obs, pred[:, :, :1], live)


@pytest.mark.parametrize("name", U.COMPS)
def test_inputs_of_the_gpu_tests(name):
    """From the host evaluation of the bound model, for the points, masks and bin counts tests/test_gpu_hist2d.py uses: every pair's
    table of every live segment has weight inside and outside the edges; and the rule that leaves a table's mutual information out of
    the comparison (an occupied cell at or below 2^-30 of the total) leaves out at most 5 % of the (point, pair) items of the observed
    and of the predicted side at the bin count the postprocess test uses."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import point_histograms2d_reference

    comp = U.composition(name, device=N.DEVICE_HOST_ONLY)
    thetas = U.points(comp, name, HU.K_POINTS)
    left_out = total = 0
    for theta in thetas:
        lw_pe, lw_inj = U.host_log_weights(comp.engine().bound, theta)
        for n_bins in HU.N_BINS:
            pb, ib = HU.bins(n_bins)
            for case in U.MASK_CASES:
                pm, im = U.masks(case)
                one = point_histograms2d_reference(lw_pe, lw_inj, pm, im, pb, ib, n_bins, HU.PAIRS)
                assert one["live"][0] == (2 if case == "masked" else 3) and one["live"][1] == 1
                for table, spread_out in ((one["obs"], False), (one["pred"], True)):  # (an event's samples may all lie inside the pooled edges)
                    sums = table.sum(axis=(-2, -1))
                    assert np.all(sums > 0.0) and np.all(sums < 1.0 if spread_out else sums <= 1.0 + 1e-12) and np.all(np.isfinite(table))
                if case == "free" and n_bins == 7:
                    ok = np.concatenate([HU.mi_comparable(one["obs"]), HU.mi_comparable(one["pred"])])
                    left_out += int(np.count_nonzero(~ok))
                    total += ok.size
    print(f"{name}: {left_out} of {total} (point, pair, side) tables left out of the mutual-information comparison")
    assert left_out <= 0.05 * total


def test_header_library_and_refusals_without_a_device():
    """The two exports are declared and bound with their argument counts (their names hold a digit: they are not in the list of names of
    letters and underscores); the header and the kernels' header cite DESIGN 8o; the ABI version stays 3; a null handle and a host-only
    handle answer GWI_ERR_INVALID, the latter with a message, and write nothing; the Python layer refuses a shard and a bad pair list."""
    import ctypes as C

    from gwinferno_amd import _native as N
    from gwinferno_amd import draws as D
    from gwinferno_amd.engine import NativePopulationLikelihood

    lib = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    raw = C.CDLL(N.LIB_PATH)
    for sym, n_args in (("gwi_point_histograms2d", 13), ("gwi_point_hist2d_times", 4)):
        assert sym in declared and hasattr(raw, sym) and len(getattr(lib, sym).argtypes) == n_args and sym not in N.EXPORTED_SYMBOLS
    assert lib.gwi_point_histograms2d.restype is C.c_int32 and lib.gwi_point_hist2d_times.restype is None
    assert "DESIGN 8o" in hdr and lib.gwi_abi_version() == 3  # added exports, no struct changed
    kernels = open(os.path.join(ROOT, "gwinferno_amd", "csrc", "gwi_hist2d.h")).read()
    assert "DESIGN 8o" in kernels and f"kMaxBins = {D.MAX_HIST2D_BINS};" in kernels and f"kMaxPairs = {D.MAX_HIST2D_PAIRS};" in kernels
    assert (D.MAX_HIST2D_BINS, D.MAX_HIST2D_PAIRS) == (64, 8) and "atomic" not in kernels.split("#pragma once")[1]
    assert lib.gwi_point_histograms2d(None, None, 1, 1, None, None, None, None, None, None, None, None, None) == -1
    eng = U.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    try:
        i32 = C.POINTER(C.c_int32)
        obs, pred, live, pairs = np.full((1, 1, 7, 7), 7.0), np.full((1, 1, 7, 7), 7.0), np.full((1, 2), 7, dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
        assert lib.gwi_point_histograms2d(eng.handle, N.as_dp(np.zeros(eng.n_theta)), 1, 1, pairs.ctypes.data_as(i32), None, None, None, N.as_dp(obs), N.as_dp(pred),
                                          live.ctypes.data_as(i32), None, None) == -1
        assert "gwi_point_histograms2d: host-only handle: no device to sum on" in lib.gwi_last_error(eng.handle).decode()
        assert np.all(obs == 7.0) and np.all(pred == 7.0) and np.all(live == 7)
        with pytest.raises(ValueError, match="thetas has shape"):
            eng.point_histograms2d(np.zeros(eng.n_theta + 1), [(0, 0)])
        with pytest.raises(ValueError, match="between 1 and 8"):
            eng.point_histograms2d(np.zeros(eng.n_theta), [(0, 0)] * 9)
        with pytest.raises(ValueError, match="between 1 and 8"):
            eng.point_histograms2d(np.zeros(eng.n_theta), np.zeros((0, 2)))
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
            eng.point_histograms2d(np.zeros(eng.n_theta), [(0, 0)])
    finally:
        eng.close()
    shard = object.__new__(NativePopulationLikelihood)
    shard.world = 2
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED: point_histograms2d: this engine holds one shard of the catalog; the injection table needs the global set"):
        shard.point_histograms2d(np.zeros(3), [(0, 0)])
