"""GPU: per-point tails of the inner importance sums on the device (include/gwi_engine.h: gwi_set_tail_sizes, gwi_point_tails;
gwinferno_amd/csrc/gwi_tail.h): tail, counts and below_max EQUAL to the statement (draws.point_tails_reference on the engine's
own log-weights), body and S under the derived bounds of tests/tail_util.py, exact ties across the cut-off, both signs, short and dead
segments, determinism over calls, splits and handles, the absence of side effects on the existing entries, the refusals, and
postprocess.importance_sum_diagnostics on both backends.

Shapes (tests/tail_util.py), PL+Peak x PL-q x PL-z on seeded synthetic catalogs: 5 x 700 with 2 500 injections (every last tile ragged,
three injection tiles), 2 x 1 024 with 2 048 (every tile full), 2 x 700 with 5 000 for m_inj = 4 096.  Three points per shape: two under
the default mass bounds and one under an upper bound that cuts through every event and the injection set.  The statement is vetted without a
device in tests/test_tail_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import tail_util as TU

pytestmark = pytest.mark.gpu

_CASES = {}


def _frozen(lw):
    for pair in lw:
        for a in pair:
            a.setflags(write=False)
    return lw


def _case(shape="ragged"):
    """Per shape two engines, made once and shared: the default mass bounds with three points (the first two are the shape's points, the
    third serves the determinism test) and the cut upper bound with one; their log-weights from the device."""
    if shape not in _CASES:
        comp, comp_cut = TU.composition(shape), TU.composition(shape, cut=True)
        eng, eng_cut = comp.engine(), comp_cut.engine()
        thetas, theta_cut = TU.points(comp, 3), TU.points(comp_cut, 1)
        thetas.setflags(write=False)
        theta_cut.setflags(write=False)
        _CASES[shape] = dict(eng=eng, thetas=thetas, lw=_frozen([eng.log_weights(t) for t in thetas]), eng_cut=eng_cut, theta_cut=theta_cut,
                             lw_cut=_frozen([eng_cut.log_weights(t) for t in theta_cut]))
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
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def _tails(eng, thetas, m_pe, m_inj, masks=(None, None)):
    try:
        eng.set_draw_mask(*masks)
        eng.set_tail_sizes(m_pe, m_inj)
        return eng.point_tails(thetas)
    finally:
        eng.set_draw_mask()


def _against_the_statement(eng, thetas, lws, m_pe, m_inj, masks=(None, None)):
    """tail, counts, max and below_max EQUAL to the statement on the engine's own log-weights; body and S under the derived bounds.
    Returns the device's arrays and the largest deviations as fractions of the bounds."""
    from gwinferno_amd import draws as D

    out = _tails(eng, thetas, m_pe, m_inj, masks)
    tail_pe, tail_inj, stats, counts = out
    k, n_ev = len(lws), eng.n_ev
    assert tail_pe.shape == (k, n_ev, m_pe) and tail_inj.shape == (k, m_inj) and stats.shape == (k, n_ev + 1, 4) and counts.shape == (k, n_ev + 1, 4) and counts.dtype == np.int32
    worst = dict(body=0.0, S=0.0)
    for p, (lw_pe, lw_inj) in enumerate(lws):
        w_pe, w_inj, w_stats, w_counts = D.point_tails_reference(lw_pe, lw_inj, masks[0], masks[1], m_pe, m_inj)
        assert np.array_equal(tail_pe[p], w_pe) and np.array_equal(tail_inj[p], w_inj) and np.array_equal(counts[p], w_counts)
        assert np.array_equal(stats[p][:, [0, 3]], w_stats[:, [0, 3]])
        for s in range(n_ev + 1):
            n_tiles = TU.n_tiles_of(eng.n_pe if s < n_ev else eng.n_inj)
            body, total, w_body, w_total = stats[p, s, 2], stats[p, s, 1], w_stats[s, 2], w_stats[s, 1]
            if w_counts[s, 3]:
                assert np.isnan(body) and np.isnan(w_body) and total == w_total == 0.0
                continue
            dev_b, dev_s = abs(body - w_body), abs(total - w_total)
            tol_b, tol_s = TU.body_bound(n_tiles) * w_body, TU.total_bound(int(w_counts[s, 0])) * w_total
            print(f"point {p}, segment {s}: body {body!r} vs {w_body!r} ({dev_b / tol_b if tol_b else 0.0:.4f} of the bound), S {total!r} vs {w_total!r} ({dev_s / tol_s:.4f})")
            assert dev_b <= tol_b and dev_s <= tol_s
            worst.update(body=max(worst["body"], dev_b / tol_b if tol_b else 0.0), S=max(worst["S"], dev_s / tol_s))
    return out, worst


SIZES = list(zip(TU.M_PE, TU.M_INJ))


@pytest.mark.parametrize("case", ["free", "masked"])
@pytest.mark.parametrize("shape,m_pe,m_inj", [(shape, m_pe, min(m_inj, TU.SHAPES[shape][2] - 1)) for shape in TU.SHAPES for m_pe, m_inj in SIZES] + [("long", 37, TU.M_LONG)])
def test_equal_to_the_statement(shape, m_pe, m_inj, case):
    """np.array_equal on tail, counts, max and below_max against point_tails_reference on eng.log_weights, at every shape, with and without
    masks, at m_pe in {1, 5, 37, 699} with m_inj in {1, 64, 671, 2 499} (one below n_inj where that is shorter) and m_inj = 4 096 on the
    long shape; body and S under the DERIVED bounds (tail_util.body_bound, total_bound), printed as fractions of them.  Two points under
    the default mass bounds, one under the bound that cuts through every segment: part of every segment is at -inf there."""
    c = _case(shape)
    masks = TU.masks(case, shape)
    (_, _, _, counts), worst = _against_the_statement(c["eng"], c["thetas"][: TU.N_FREE_POINTS], c["lw"][: TU.N_FREE_POINTS], m_pe, m_inj, masks)
    (_, _, _, counts_cut), worst_cut = _against_the_statement(c["eng_cut"], c["theta_cut"], c["lw_cut"], m_pe, m_inj, masks)
    n_ev, n_pe, n_inj = TU.SHAPES[shape]
    for lw_pe, lw_inj in c["lw_cut"]:
        assert all(0 < np.isfinite(lw_pe[e]).sum() < n_pe for e in range(n_ev)) and 0 < np.isfinite(lw_inj).sum() < n_inj
    alive = [e for e in range(n_ev) if not (case == "masked" and e == TU.DEAD_EVENT)]
    assert np.all(counts_cut[:, alive, 0] > 0) and np.all(counts_cut[:, alive, 0] < n_pe) and np.all(counts[:, alive, 3] == 0)
    if case == "masked":
        assert np.all(counts[:, TU.DEAD_EVENT] == [0, 0, 0, 1]) and np.all(counts_cut[:, TU.DEAD_EVENT] == [0, 0, 0, 1])
    print(f"{shape}, m = ({m_pe}, {m_inj}), {case}: largest fractions of the bounds: body {max(worst['body'], worst_cut['body']):.4f}, S {max(worst['S'], worst_cut['S']):.4f}")


def test_exact_ties_across_the_cutoff():
    """A catalog whose samples 2j and 2j + 1 are copies: their log-weights tie in every bit.  With m odd the tie straddles the cut-off:
    n_gt + n_eq > m, the tail holds m - n_gt copies of v*, and the derived cut-off is v* itself."""
    from gwinferno_amd import draws as D

    comp = TU.composition("ragged", ties=True)
    eng = comp.engine()
    try:
        thetas = TU.points(comp, 2)
        lws = [eng.log_weights(t) for t in thetas]
        for lw_pe, lw_inj in lws:
            assert np.array_equal(lw_pe[:, 0::2], lw_pe[:, 1::2], equal_nan=True) and np.array_equal(lw_inj[0::2], lw_inj[1::2], equal_nan=True)
        m_pe, m_inj = 37, 671
        (tail_pe, tail_inj, stats, counts), _ = _against_the_statement(eng, thetas, lws, m_pe, m_inj)
        for p in range(2):
            for s in range(eng.n_ev + 1):
                tail, m = (tail_pe[p, s], m_pe) if s < eng.n_ev else (tail_inj[p], m_inj)
                n_live, n_gt, n_eq, dead = counts[p, s]
                assert not dead and n_live > m and n_gt + n_eq > m and n_gt < m and n_eq >= 2 and np.all(tail[: m - n_gt] == tail[0]) and tail[m - n_gt] > tail[0]
                cutoff, rest = D.tail_cutoff_and_rest(tail, stats[p, s], counts[p, s])
                assert cutoff == tail[0] and rest >= stats[p, s, 2] + np.exp(tail[0] - stats[p, s, 0]) * (1 - 1e-15)
    finally:
        eng.close()


def test_both_signs_within_a_segment():
    """The priors multiplied by a constant each (a constant column of the prior) so that the median log-weight of event 0 and of the
    injection set is 0: live log-weights of both signs occur within those segments, checked from log_weights; the keys of negative and
    of non-negative values order as the numbers do."""
    c = _case()
    lw_pe, lw_inj = c["lw"][0]
    scale = (float(np.exp(np.median(lw_pe[0][np.isfinite(lw_pe[0])]))), float(np.exp(np.median(lw_inj[np.isfinite(lw_inj)]))))
    comp = TU.composition("ragged", prior_scale=scale)
    eng = comp.engine()
    try:
        thetas = c["thetas"][:1]
        lws = [eng.log_weights(t) for t in thetas]
        for seg in (lws[0][0][0], lws[0][1]):
            live = seg[np.isfinite(seg)]
            assert (live > 0).sum() > 100 and (live < 0).sum() > 100
        for m_pe, m_inj in ((37, 671), (500, 2000)):  # v* above and below 0
            (tail_pe, tail_inj, _, _), _ = _against_the_statement(eng, thetas, lws, m_pe, m_inj)
        assert tail_pe[0, 0, 0] < 0 < tail_pe[0, 0, -1] and tail_inj[0, 0] < 0 < tail_inj[0, -1]
    finally:
        eng.close()


def test_short_and_dead_segments():
    """Event 0 masked down to exactly m live samples, event 2 to m - 3, event 1 fully masked, the injection set to m_inj - 3: the live
    values sit at the top end of the tail with -inf in front, n_gt = n_live for a segment with fewer than m, the dead one has an all -inf
    tail, zero counts and NaN body.  And a point at which every sample of one event is outside the mass bounds."""
    c = _case()
    eng, m_pe, m_inj = c["eng"], 37, 64
    lw_pe, lw_inj = c["lw"][0]
    pe_mask = np.ones(lw_pe.shape, dtype=np.uint8)
    pe_mask[0], pe_mask[1], pe_mask[2] = TU.keep_first_live(lw_pe[0], m_pe), 0, TU.keep_first_live(lw_pe[2], m_pe - 3)
    inj_mask = TU.keep_first_live(lw_inj, m_inj - 3)
    (tail_pe, tail_inj, stats, counts), _ = _against_the_statement(eng, c["thetas"][:1], c["lw"][:1], m_pe, m_inj, (pe_mask, inj_mask))
    assert tuple(counts[0, 0][[0, 3]]) == (m_pe, 0) and counts[0, 0, 1] + counts[0, 0, 2] == m_pe and np.all(np.isfinite(tail_pe[0, 0])) and stats[0, 0, 2] == 0.0 and stats[0, 0, 3] == -np.inf
    assert tuple(counts[0, 2]) == (m_pe - 3, m_pe - 3, 0, 0) and np.all(tail_pe[0, 2, :3] == -np.inf) and np.all(np.isfinite(tail_pe[0, 2, 3:])) and stats[0, 2, 2] == 0.0
    assert tuple(counts[0, 1]) == (0, 0, 0, 1) and np.all(tail_pe[0, 1] == -np.inf) and np.isnan(stats[0, 1, 2])
    assert tuple(counts[0, -1]) == (m_inj - 3, m_inj - 3, 0, 0) and np.all(tail_inj[0, :3] == -np.inf) and np.all(np.isfinite(tail_inj[0, 3:]))
    # an upper mass bound below every sample of the heaviest event
    pe, _, _ = TU.catalog("ragged")
    heavy = int(np.argmax(pe["mass_1"].min(axis=1)))
    others = np.delete(pe["mass_1"], heavy, axis=0)
    bound = 0.999 * pe["mass_1"][heavy].min()
    assert (others < bound).any(axis=1).all()
    comp = TU.composition("ragged", cut=bound)
    eng2 = comp.engine()
    try:
        thetas = TU.points(comp, 1)
        lws = [eng2.log_weights(t) for t in thetas]
        assert not np.isfinite(lws[0][0][heavy]).any()
        (tail_pe, _, stats, counts), _ = _against_the_statement(eng2, thetas, lws, m_pe, m_inj)
        assert tuple(counts[0, heavy]) == (0, 0, 0, 1) and np.all(tail_pe[0, heavy] == -np.inf) and np.isnan(stats[0, heavy, 2]) and counts[0, :, 3].sum() == 1
    finally:
        eng2.close()


def test_determinism_over_calls_splits_and_handles():
    """Two calls, the points split 1 + 2 over calls and a second handle give equal bits in every output, body and S included."""
    c = _case()
    eng, thetas, masks = c["eng"], c["thetas"], TU.masks("masked")
    for mk in ((None, None), masks):
        first = _tails(eng, thetas, 37, 671, mk)
        assert _same(first, _tails(eng, thetas, 37, 671, mk))
        one, two = _tails(eng, thetas[:1], 37, 671, mk), _tails(eng, thetas[1:], 37, 671, mk)
        assert _same(first, [np.concatenate([a, b]) for a, b in zip(one, two)])
        eng2 = TU.composition().engine()
        try:
            assert _same(first, _tails(eng2, thetas, 37, 671, mk))
        finally:
            eng2.close()


def test_no_side_effects_on_the_existing_entries():
    """weighted_histograms, point_moments and point_rank_correlations give the same bits before and after a point_tails call."""
    from gwinferno_amd import draws as D

    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    x_pe, x_inj = TU.RU.columns(3)
    edges = [np.quantile(np.concatenate([p.ravel(), i]), np.linspace(0.02, 0.98, 17)) for p, i in zip(x_pe, x_inj)]
    eng.set_histogram_bins(np.stack([D.digitize(p, e) for p, e in zip(x_pe, edges)]), np.stack([D.digitize(i, e) for i, e in zip(x_inj, edges)]), n_bins=16)
    eng.set_kde_columns(x_pe, x_inj)
    eng.set_rankcorr_columns(x_pe, x_inj)

    def existing():
        return list(eng.weighted_histograms(thetas)) + list(eng.point_moments(thetas)) + list(eng.point_rank_correlations(thetas))

    before = existing()
    tails = _tails(eng, thetas, 37, 671)
    assert _same(before, existing()) and _same(tails, _tails(eng, thetas, 37, 671))


def test_refusals():
    """Nothing set, m out of range, m >= n, null outputs, k < 1: GWI_ERR_INVALID in the words of bad_point_args and of the setter, and
    nothing is written."""
    from gwinferno_amd import _native as N

    eng = TU.composition().engine()
    try:
        theta = _case()["thetas"][0]
        with pytest.raises(N.NativeEngineError, match=r"gwi_point_tails: no tail sizes are set \(gwi_set_tail_sizes\)"):
            eng.point_tails(theta)
        for bad, why in (((0, 5), "m_pe = 0 is not in 1 ... 4096"), ((4097, 5), "m_pe = 4097 is not in 1 ... 4096"), ((5, 0), "m_inj = 0 is not in 1 ... 4096"),
                         ((5, -1), "m_inj = -1 is not in"), ((700, 5), "m_pe = 700 is not below n_pe = 700"), ((5, 2500), "m_inj = 2500 is not below n_inj = 2500")):
            with pytest.raises(N.NativeEngineError, match="gwi_set_tail_sizes: " + why):
                eng.set_tail_sizes(*bad)
        with pytest.raises(N.NativeEngineError, match="no tail sizes are set"):  # (a refused size sets nothing)
            eng.point_tails(theta)
        eng.set_tail_sizes(5, 7)
        lib, i32 = eng.lib, C.POINTER(C.c_int32)
        tail, stats, counts = np.full((1, 5 * eng.n_ev + 7), 7.0), np.full((1, eng.n_ev + 1, 4), 7.0), np.full((1, eng.n_ev + 1, 4), 7, dtype=np.int32)
        args = [N.as_dp(tail), N.as_dp(stats), counts.ctypes.data_as(i32)]
        for i, name in enumerate(("tail", "stats", "counts")):
            assert lib.gwi_point_tails(eng.handle, N.as_dp(theta), 1, *[None if j == i else a for j, a in enumerate(args)]) == -1
            assert f"gwi_point_tails: {name} is null" in lib.gwi_last_error(eng.handle).decode()
        for th, k in ((N.as_dp(theta), 0), (N.as_dp(theta), -2), (None, 1)):
            assert lib.gwi_point_tails(eng.handle, th, k, *args) == -1 and "gwi_point_tails: thetas is null or k < 1" in lib.gwi_last_error(eng.handle).decode()
        assert np.all(tail == 7.0) and np.all(stats == 7.0) and np.all(counts == 7)
        assert lib.gwi_point_tails(eng.handle, N.as_dp(theta), 1, *args) == 0 and np.all(counts[..., 0] > 0)
        assert eng.set_tail_sizes() is None and eng._tail_shape == (80, 150)  # the rule: min(700 // 5, ceil(3 sqrt 700)), min(2500 // 5, ceil(3 sqrt 2500))
    finally:
        eng.close()


def test_diagnostics_on_both_backends():
    """importance_sum_diagnostics on the device and on the host (the statement on eng.log_weights) agree exactly in pareto_k, in every
    count and in which segments are skipped -- the fit is host code on equal inputs -- and in the log sums within the derived bounds;
    with masks that leave one event dead and with the mass cuts of posterior_predictive_draws."""
    from gwinferno_amd import postprocess as P

    c = _case()
    eng, thetas = c["eng"], c["thetas"]
    pe, inj, _ = TU.catalog("ragged")
    for kw, mk in ((dict(), (None, None)), (dict(m_pe=37, m_inj=64), TU.masks("masked")), (dict(pedata=pe, injdata=inj, m1min=5.0, m2min=5.0, mmax=60.0), None)):
        try:
            if mk is not None:
                eng.set_draw_mask(*mk)
            dev = P.importance_sum_diagnostics(eng, thetas, backend="device", **kw)
        finally:
            eng.set_draw_mask()
        host_kw = dict(kw)
        if mk is not None and mk[0] is not None:  # (the host backend takes its masks from the mass cuts alone: give the statement the same ones)
            host = _host_with_masks(eng, thetas, mk, **kw)
        else:
            host = P.importance_sum_diagnostics(eng, thetas, backend="host", **host_kw)
        for key in ("pareto_k", "n_live", "skipped", "counts", "n_skipped", "worst_point", "worst_k", "share_above_0.5", "share_above_0.7", "tail_pe", "tail_inj"):
            assert np.array_equal(dev[key], host[key], equal_nan=np.asarray(dev[key]).dtype.kind == "f"), key
        assert dev["m_pe"] == host["m_pe"] and dev["m_inj"] == host["m_inj"] and np.isfinite(dev["pareto_k"][~dev["skipped"]]).all()
        n_ev = eng.n_ev
        for p in range(len(thetas)):
            for s in range(n_ev + 1):
                if dev["counts"][p, s, 3]:
                    assert np.isnan(dev["log_sum_raw"][p, s]) and np.isnan(host["log_sum_raw"][p, s])
                    continue
                top, total = host["stats"][p, s, :2]
                raw = host["log_sum_raw"][p, s]
                assert abs(dev["log_sum_raw"][p, s] - raw) <= TU.log_sum_bound(TU.total_bound(int(host["n_live"][p, s])), np.log(total), raw)
                if not host["skipped"][p, s]:
                    psis = host["log_sum_psis"][p, s]
                    tol = TU.log_sum_bound(TU.body_bound(TU.n_tiles_of(eng.n_pe if s < n_ev else eng.n_inj)), psis - top, psis)
                    assert abs(dev["log_sum_psis"][p, s] - psis) <= tol
        if mk is not None and mk[0] is not None:
            assert np.all(dev["skipped"][:, TU.DEAD_EVENT]) and dev["n_skipped"][TU.DEAD_EVENT] == len(thetas)


def _host_with_masks(eng, thetas, masks, **kw):
    """the host backend of importance_sum_diagnostics under explicit masks: a stand-in engine whose log_weights are the device's with the
    masked samples at -inf (a masked sample and a -inf one are equally not live)"""
    from gwinferno_amd import postprocess as P

    lw_pe, lw_inj = [], []
    for th in thetas:
        a, b = eng.log_weights(th)
        lw_pe.append(np.where(masks[0] != 0, a, -np.inf))
        lw_inj.append(np.where(masks[1] != 0, b, -np.inf))
    stub = TU.RU.StubEngine(lw_pe, lw_inj)
    return P.importance_sum_diagnostics(stub, np.arange(len(thetas), dtype=np.float64)[:, None], backend="host", **kw)
