"""CPU: weighted histograms (include/gwi_engine.h: gwi_weighted_histograms; gwinferno_amd/csrc/gwi_hist.h) -- the NumPy statement
(gwinferno_amd/draws.py: weighted_histograms_reference, digitize) on a case worked by hand, the density normalisation of
postprocess.reweighted_event_posteriors(backend="host"), the header, the library's exports and the refusals that need no device, and
the inputs of tests/test_gpu_hist.py, which are vetted here."""
import ctypes as C
import os
import re

import hist_util as U
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_against_a_hand_case():
    """Three samples, two bins, one column, worked by hand.  Log-weights (log 1, log 3, log 4): M = log 4, w = (1/4, 3/4, 1), S = 2."""
    from gwinferno_amd import draws as D

    lw = np.log(np.array([1.0, 3.0, 4.0]))
    w = np.exp(lw - lw[2])  # the statement's own weights: (0.25, 0.75, 1) up to the rounding of log and exp
    both = lambda codes: D.weighted_histogram_segment(lw, None, np.array([codes]), 2)  # noqa: E731
    h, live = both([0, 1, 0])
    assert live and h.shape == (1, 2) and np.array_equal(h[0], [(w[0] + w[2]) / w.sum(), w[1] / w.sum()])
    assert np.allclose(h[0], [1.25 / 2.0, 0.75 / 2.0], rtol=1e-15, atol=0.0)
    # an outside sample is in no bin but stays in the total: the row sums to 1 - its share (the heaviest sample: 1 / 2)
    h, live = both([0, 1, D.OUTSIDE_BIN])
    assert live and np.allclose(h[0], [0.25 / 2.0, 0.75 / 2.0], rtol=1e-15, atol=0.0) and abs(h.sum() - 0.5) <= 1e-15
    # a masked sample leaves numerator AND total: M = log 3, w = (1/3, 1), S = 4/3
    h, live = D.weighted_histogram_segment(lw, np.array([1, 1, 0]), np.array([[0, 1, 0]]), 2)
    assert live and np.allclose(h[0], [0.25, 0.75], rtol=1e-15, atol=0.0)
    # -inf (and NaN, +inf) weights count for nothing
    h, live = D.weighted_histogram_segment(np.array([-np.inf, lw[1], np.nan]), None, np.array([[0, 1, 0]]), 2)
    assert live and np.array_equal(h[0], [0.0, 1.0])
    # nothing with weight: zeros, not live -- all -inf, all masked, or both
    for lw_dead, mask in ((np.full(3, -np.inf), None), (lw, np.zeros(3, dtype=np.uint8)), (np.array([0.0, -np.inf, -np.inf]), np.array([0, 1, 1]))):
        h, live = D.weighted_histogram_segment(lw_dead, mask, np.array([[0, 1, 0]]), 2)
        assert not live and np.array_equal(h, np.zeros((1, 2)))
    # the layout of one point: two events, the second dead, and the injection set; two columns
    lw_pe = np.stack([lw, np.full(3, -np.inf)])
    pe_bins = np.array([[[0, 1, 0], [0, 0, 0]], [[1, 1, D.OUTSIDE_BIN], [1, 1, 1]]])
    inj_bins = np.array([[1, 0], [0, 0]])
    hp, hi, dead = D.weighted_histograms_reference(lw_pe, np.log([1.0, 3.0]), None, None, pe_bins, inj_bins, 2)
    assert hp.shape == (2, 2, 2) and hi.shape == (2, 2) and dead.dtype == np.int32 and np.array_equal(dead, [0, 1, 0])
    assert np.allclose(hp[0], [[0.625, 0.375], [0.0, 0.5]], rtol=1e-15, atol=0.0) and np.array_equal(hp[1], np.zeros((2, 2)))
    assert np.allclose(hi, [[0.75, 0.25], [1.0, 0.0]], rtol=1e-15, atol=0.0)
    hp, hi, dead = D.weighted_histograms_reference(lw_pe, np.log([1.0, 3.0]), None, np.zeros(2), None, inj_bins, 2)
    assert hp is None and np.array_equal(hi, np.zeros((2, 2))) and np.array_equal(dead, [0, 0, 1])


def test_digitize_is_numpy_histogram():
    """Non-uniform edges, values on the edges, the inclusive last edge, values outside and NaN: the counts are np.histogram's."""
    from gwinferno_amd import draws as D

    e = np.array([1.0, 1.5, 4.0, 4.5, 10.0])
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(0.0, 11.0, 500), e, [np.nan, -np.inf, np.inf, np.nextafter(10.0, 11.0), np.nextafter(1.0, 0.0)]])
    code = D.digitize(x, e)
    assert code.dtype == np.uint16 and code.shape == x.shape
    inside = code != D.OUTSIDE_BIN
    assert np.array_equal(np.bincount(code[inside], minlength=4), np.histogram(x[np.isfinite(x)], bins=e)[0])
    assert np.array_equal(D.digitize(e, e), [0, 1, 2, 3, 3]) and np.all(code[-5:] == D.OUTSIDE_BIN)
    assert D.digitize(np.ones((2, 3)), e).shape == (2, 3)
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="increasing"):
            D.digitize(x, bad)


class _StubEngine:
    """What reweighted_event_posteriors(backend="host") needs of an engine: the shapes and log_weights."""

    def __init__(self, lw_pe, lw_inj):
        self.lw_pe, self.lw_inj = lw_pe, lw_inj
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe[0].shape, lw_inj[0].size, 1

    def log_weights(self, theta):
        k = int(theta[0])
        return self.lw_pe[k].copy(), self.lw_inj[k].copy()


def test_density_normalisation():
    """events * widths sums to 1 - outside to 1e-15, and so does predicted; a point at which a segment has no weight leaves its
    mean over the live points alone (n_points); the host backend is the statement, point by point."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    rng = np.random.default_rng(4)
    k, n_ev, n_pe, n_inj, n_bins = 5, 3, 400, 700, 12
    lw_pe, lw_inj = rng.normal(0.0, 3.0, (k, n_ev, n_pe)), rng.normal(0.0, 3.0, (k, n_inj))
    lw_pe[2, 1] = -np.inf  # event 1 is dead at point 2
    lw_inj[4] = np.nan     # ... and the injection set at point 4
    eng = _StubEngine(lw_pe, lw_inj)
    pe_values = {"a": rng.uniform(0.0, 10.0, (n_ev, n_pe)), "b": rng.lognormal(0.0, 1.0, (n_ev, n_pe))}
    inj_values = {"a": rng.uniform(0.0, 10.0, n_inj), "b": rng.lognormal(0.0, 1.0, n_inj)}
    edges = {"a": np.linspace(1.0, 9.0, n_bins + 1), "b": np.geomspace(0.2, 5.0, n_bins + 1)}
    thetas = np.arange(k, dtype=np.float64)[:, None]
    out = P.reweighted_event_posteriors(eng, thetas, pe_values, edges, inj_values=inj_values, backend="host")
    assert set(out) == {"a", "b", "edges"}
    for c, name in enumerate(("a", "b")):
        r, widths = out[name], np.diff(edges[name])
        assert r["events"].shape == (n_ev, n_bins) and r["predicted"].shape == (n_bins,) and r["outside"]["events"].shape == (n_ev,)
        assert np.array_equal(r["n_points"]["events"], [k, k - 1, k]) and r["n_points"]["predicted"] == k - 1
        assert np.all(np.abs((r["events"] * widths).sum(axis=1) - (1.0 - r["outside"]["events"])) <= 1e-15)
        assert abs((r["predicted"] * widths).sum() - (1.0 - r["outside"]["predicted"])) <= 1e-15
        assert np.all(r["outside"]["events"] > 0.0) and np.all(r["outside"]["events"] < 1.0) and 0.0 < r["outside"]["predicted"] < 1.0
        # ... and it is the statement: the mean over the live points of the per-point histograms
        want = np.zeros((n_ev, n_bins))
        for p in range(k):
            for ev in range(n_ev):
                want[ev] += D.weighted_histogram_segment(lw_pe[p, ev], None, D.digitize(pe_values[name][ev], edges[name])[None], n_bins)[0][0]
        assert np.array_equal(r["events"], want / np.array([k, k - 1, k])[:, None] / widths)
    only_a = P.reweighted_event_posteriors(eng, thetas, pe_values, edges, param_names=["a"], backend="host")
    assert set(only_a) == {"a", "edges"} and "predicted" not in only_a["a"] and np.array_equal(only_a["a"]["events"], out["a"]["events"])
    with pytest.raises(ValueError, match="same number of bins"):
        P.reweighted_event_posteriors(eng, thetas, pe_values, {"a": edges["a"], "b": edges["b"][:-1]}, backend="host")
    with pytest.raises(ValueError, match="pe_values\\['a'\\] has shape"):
        P.reweighted_event_posteriors(eng, thetas, {"a": np.zeros(3), "b": pe_values["b"]}, edges, backend="host")
    with pytest.raises(ValueError, match="together or not at all"):
        P.reweighted_event_posteriors(eng, thetas, pe_values, edges, m1min=5.0, backend="host")
    with pytest.raises(ValueError, match="backend"):
        P.reweighted_event_posteriors(eng, thetas, pe_values, edges, backend="eager")
    with pytest.raises(ValueError, match="chunk"):
        P.reweighted_event_posteriors(eng, thetas, pe_values, edges, backend="host", chunk=65)


def test_new_symbols_in_binding_header_and_library():
    from gwinferno_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym in ("gwi_set_histogram_bins", "gwi_weighted_histograms", "gwi_histogram_times"):
        assert sym in _native.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym)
    assert len(lib.gwi_set_histogram_bins.argtypes) == 5 and len(lib.gwi_weighted_histograms.argtypes) == 6 and len(lib.gwi_histogram_times.argtypes) == 4
    assert lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_set_histogram_bins(None, 1, 1, None, None) == -1 and lib.gwi_weighted_histograms(None, None, 1, None, None, None) == -1  # GWI_ERR_INVALID


def test_host_only_handle_and_validation():
    """A host-only handle answers GWI_ERR_INVALID with a message from both entries; the Python layer checks shapes, dtypes and the
    thetas before the library is asked, and the library the limits and the codes."""
    from gwinferno_amd import _native as N

    eng = U.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    pb, ib = U.bins(7)
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.set_histogram_bins(pb, ib, n_bins=7)
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.weighted_histograms(np.zeros(eng.n_theta))
    u16 = C.POINTER(C.c_uint16)
    assert eng.lib.gwi_set_histogram_bins(eng.handle, 2, 7, pb.ctypes.data_as(u16), ib.ctypes.data_as(u16)) == -1
    assert "host-only" in eng.lib.gwi_last_error(eng.handle).decode()
    th, dead = np.zeros(eng.n_theta), np.zeros(U.N_EV + 1, dtype=np.int32)
    assert eng.lib.gwi_weighted_histograms(eng.handle, N.as_dp(th), 1, None, None, dead.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert "host-only" in eng.lib.gwi_last_error(eng.handle).decode()
    with pytest.raises(ValueError, match="n_bins is needed"):
        eng.set_histogram_bins(pb, ib)
    with pytest.raises(ValueError, match="both None"):
        eng.set_histogram_bins(n_bins=7)
    with pytest.raises(ValueError, match="pe_bins has shape"):
        eng.set_histogram_bins(pb[:, :, :-1], ib, n_bins=7)
    with pytest.raises(ValueError, match="pe_bins has shape"):
        eng.set_histogram_bins(pb[0], ib, n_bins=7)
    with pytest.raises(ValueError, match="inj_bins has shape"):
        eng.set_histogram_bins(pb, ib[:, :-1], n_bins=7)
    with pytest.raises(ValueError, match="columns"):
        eng.set_histogram_bins(pb, ib[:1], n_bins=7)
    with pytest.raises(ValueError, match="not integer"):
        eng.set_histogram_bins(pb.astype(np.float64), ib, n_bins=7)
    with pytest.raises(ValueError, match="0xFFFF"):
        eng.set_histogram_bins(pb.astype(np.int64) - 1, ib, n_bins=7)
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.weighted_histograms(np.zeros(eng.n_theta + 1))
    with pytest.raises(ValueError, match="thetas has shape"):
        eng.weighted_histograms(np.zeros((0, eng.n_theta)))


def test_world_above_one_is_refused_in_python():
    """The message form of draw_indices and resample_injections; no handle is needed to refuse."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    eng = object.__new__(NativePopulationLikelihood)
    eng.world = 2
    for call, name in ((lambda: eng.set_histogram_bins(None, None, n_bins=4), "set_histogram_bins"), (lambda: eng.weighted_histograms(np.zeros(3)), "weighted_histograms")):
        with pytest.raises(N.NativeEngineError, match=f"GWI_ERR_UNSUPPORTED: {name}: this engine holds one shard of the catalog"):
            call()


def test_limits_of_the_user_facing_function():
    """At most 8 quantities and 256 bins (the library's own limits and its check of the codes need a device handle:
    tests/test_gpu_hist.py: test_limits)."""
    from gwinferno_amd import postprocess as P

    eng = _StubEngine(np.zeros((1, 2, 5)), np.zeros((1, 4)))
    vals = {str(i): np.zeros((2, 5)) for i in range(9)}
    with pytest.raises(ValueError, match="between 1 and 8"):
        P.reweighted_event_posteriors(eng, np.zeros((1, 1)), vals, {k: [0.0, 1.0] for k in vals}, backend="host")
    with pytest.raises(ValueError, match="1 ... 256"):
        P.reweighted_event_posteriors(eng, np.zeros((1, 1)), {"0": vals["0"]}, {"0": np.arange(258.0)}, backend="host")


@pytest.mark.parametrize("name", U.COMPS)
def test_inputs_of_the_gpu_tests(name):
    """Every case tests/test_gpu_hist.py compares, from the host evaluation of the bound model: every segment meant to be live
    has at least 200 samples with weight, all of them above LOG_FLOOR relative to the segment's maximum (so no weight can round to 0
    on one side only: a bin of the statement is 0 exactly when no live sample falls in it, and then the device's is 0 too); the
    "masked" case has exactly one dead segment; every column has samples with weight outside the edges on both sides and at least
    one live sample in some bin.  The cap on skipped comparisons is therefore ZERO: no bin and no segment is left out."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import OUTSIDE_BIN, draw_weights, weighted_histograms_reference

    comp = U.composition(name, device=N.DEVICE_HOST_ONLY)
    thetas = U.points(comp, name, 3)
    assert thetas.shape == (3, comp.engine().n_theta) and len({t.tobytes() for t in thetas}) == 3
    for p, theta in enumerate(thetas):
        lw_pe, lw_inj = U.host_log_weights(comp.engine().bound, theta)
        for case in U.MASK_CASES:
            pm, im = U.masks(case)
            n_dead = 0
            for seg, (lw, mask) in enumerate(U.segments(lw_pe, lw_inj, pm, im)):
                live = U.n_live(lw, mask)
                if case == "masked" and seg == U.DEAD_EVENT:
                    assert live == 0
                    n_dead += 1
                    continue
                on = np.isfinite(lw) if mask is None else np.isfinite(lw) & (mask != 0)
                print(f"{name} point {p} {case} segment {seg}: {live} live samples, spread {lw[on].max() - lw[on].min():.1f}")
                assert live >= 200 and live == on.sum() and lw[on].min() - lw[on].max() > U.LOG_FLOOR
            assert n_dead == (1 if case == "masked" else 0)
            if p:
                continue
            for n_bins in U.N_BINS:
                pb, ib = U.bins(n_bins)
                hp, hi, dead = weighted_histograms_reference(lw_pe, lw_inj, pm, im, pb, ib, n_bins)
                assert dead.sum() == n_dead and np.all(np.isfinite(hp)) and np.all(np.isfinite(hi))
                for seg, (lw, mask) in enumerate(U.segments(lw_pe, lw_inj, pm, im)):
                    if dead[seg]:
                        continue
                    w = draw_weights(lw, mask)
                    for c in range(len(U.COLUMNS)):
                        code = pb[c, seg] if seg < U.N_EV else ib[c]
                        row = hp[seg, c] if seg < U.N_EV else hi[c]
                        if seg == U.N_EV:  # (an event's samples cluster, the pooled edges may hold them all; the injections spread out)
                            assert np.any(w[code == OUTSIDE_BIN] > 0.0)
                        assert 0.0 < row.sum() <= 1.0 + 1e-12
                        # a bin is 0 exactly when it holds no live sample
                        assert np.array_equal(row > 0.0, np.bincount(code[(w > 0) & (code != OUTSIDE_BIN)], minlength=n_bins) > 0)
                for c in range(len(U.COLUMNS)):  # at least one outside sample per column in both sets
                    assert np.any(pb[c] == OUTSIDE_BIN) and np.any(ib[c] == OUTSIDE_BIN) and np.any(pb[c] != OUTSIDE_BIN)
                    assert np.any(hp[:, c].sum(axis=1)[dead[: U.N_EV] == 0] < 1.0 - 1e-6) and hi[c].sum() < 1.0 - 1e-6


def test_extreme_points_of_the_gpu_tests():
    """The two PL+Peak points of test_mask_dead_and_outside, from the host evaluation: at dead_event_params one event has no finite
    log-weight while another keeps 200; at wide_spread_params the finite log-weights of one event span more than 800."""
    from gwinferno_amd import _native as N

    comp = U.composition("plpeak", device=N.DEVICE_HOST_ONLY)
    lw_pe, _ = U.host_log_weights(comp.engine().bound, comp.theta(U.dead_event_params()))
    finite = np.isfinite(lw_pe).sum(axis=1)
    print("finite log-weights per event at the dead-event point:", finite)
    assert finite.min() == 0 and finite.max() >= 200
    lw_pe, _ = U.host_log_weights(comp.engine().bound, comp.theta(U.wide_spread_params()))
    spread = [np.ptp(r[np.isfinite(r)]) for r in lw_pe]
    print("spread of the finite log-weights per event at the wide-spread point:", spread)
    assert max(spread) > 800.0
