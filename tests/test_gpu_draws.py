"""GPU: weighted index draws on the device (include/gwi_engine.h: gwi_set_draw_mask / gwi_draw_indices;
gwinferno_amd/csrc/gwi_draw.h).

Bracket test, every draw: the expected log-weights come from the independent host evaluation of the bound model
(tests/bound_eval.log_weights), the cumulative weights C are formed in extended precision (np.longdouble), and a device index j
is accepted iff w_j > 0 and C_{j-1} - d <= u C_last < C_j + d with d = 1e-9 C_last -- the project's parity bound for weights;
fp64 summation error over at most 500 k terms is far inside it, and a live sample's weight is of order C_last / n_eff, at
least 1e-6 of the total here, so the band cannot hide a wrong index."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from golden_util import GoldenCase

pytestmark = pytest.mark.gpu

TOP = 1.0 - 2.0**-53
BAND = 1e-9
N_DRAWS = 256


def _bound_log_weights(bound, theta):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bound_eval import log_weights

    lpe, linj, _ = log_weights(bound, theta, include_consts=True)
    return np.asarray(lpe), np.asarray(linj)


def _uniforms(rng, *lead):
    u = rng.uniform(size=(*lead, N_DRAWS))
    u[..., 0], u[..., 1] = 0.0, TOP
    return u


def _check_segment(lw, mask, u, idx, what):
    """Every draw of one segment against the bracket of the expected cumulative weights."""
    from gwinferno_amd.draws import draw_weights

    w = draw_weights(lw, mask).astype(np.longdouble)
    cdf = np.cumsum(w)
    c_last = cdf[-1] if cdf.size else np.longdouble(0)
    idx = np.asarray(idx)
    if not c_last > 0:
        assert np.all(idx == -1), what
        return
    assert np.all((idx >= 0) & (idx < w.size)), (what, idx.min(), idx.max())
    assert np.all(w[idx] > 0), what
    d = np.longdouble(BAND) * c_last
    target = np.asarray(u, dtype=np.longdouble) * c_last
    below = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], np.longdouble(0))
    ok = (below - d <= target) & (target < cdf[idx] + d)
    assert np.all(ok), (what, int(np.sum(~ok)), idx[~ok][:5], np.asarray(u)[~ok][:5])


def _check_point(lw_pe, lw_inj, masks, u_pe, u_inj, idx_pe, idx_inj, what):
    m_pe, m_inj = masks
    assert idx_pe.dtype == np.int32 and idx_pe.shape == u_pe.shape and idx_inj.dtype == np.int32 and idx_inj.shape == u_inj.shape
    for ev in range(lw_pe.shape[0]):
        _check_segment(lw_pe[ev], None if m_pe is None else m_pe[ev], u_pe[ev], idx_pe[ev], (what, "event", ev))
    _check_segment(lw_inj, m_inj, u_inj, idx_inj, (what, "injections"))


def _thetas(comp, name, n, seed):
    from gwinferno_amd.compositions import draw_params

    rng = np.random.default_rng(seed)
    return np.stack([comp.theta(draw_params(name, rng)) for _ in range(n)])


def _bracket_run(eng, bound, thetas, what, masks=(None, None), seed=1):
    rng = np.random.default_rng(seed)
    k = thetas.shape[0]
    u_pe, u_inj = _uniforms(rng, k, eng.n_ev), _uniforms(rng, k)
    idx_pe, idx_inj = eng.draw_indices(thetas, u_pe, u_inj)
    for p in range(k):
        lw_pe, lw_inj = _bound_log_weights(bound, thetas[p])
        _check_point(lw_pe, lw_inj, masks, u_pe[p], u_inj[p], idx_pe[p], idx_inj[p], (what, "point", p))
    return u_pe, u_inj, idx_pe, idx_inj


# configs 2, 3 and 5 at the reduced sizes of test_gpu_parity.test_against_oracle_midsize, and config 2 at full size
@pytest.mark.parametrize("comp_name,size", [("plpeak", (69, 1000, 20000)), ("bspline_iid", (20, 700, 9000)), ("bspline_full", (12, 1500, 15001)), ("plpeak", "c2")])
def test_every_draw_lies_in_its_bracket(comp_name, size):
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog, make_config_catalog

    pe, inj, total = make_config_catalog(size) if isinstance(size, str) else make_catalog(*size, seed=99)
    comp = COMPOSITIONS[comp_name](pe, inj)
    eng = comp.engine()
    assert not eng.scan_kernel_name().startswith(("jit:", "generic"))
    _bracket_run(eng, eng.bound, _thetas(comp, comp_name, 2, seed=17), (comp_name, size))
    eng.close()


@pytest.mark.parametrize("how", ["hiprtc", "generic", "narrow"])
def test_every_draw_lies_in_its_bracket_on_the_other_scan_chains(how, monkeypatch, tmp_path):
    """The log-weight role of a chain compiled at run time, of the generic kernel, and of an engine with narrow columns."""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(9, 1100, 7000, seed=23)
    # (the chain compiled at run time is one no other test of the suite compiles: the code objects are cached process-wide)
    name = "plpeak_default_tilt" if how == "hiprtc" else "bspline_iid"
    if how == "narrow":
        for k in ("a_1", "a_2", "cos_tilt_1", "cos_tilt_2"):
            pe[k], inj[k] = pe[k].astype(np.float32).astype(np.float64), inj[k].astype(np.float32).astype(np.float64)
    wide = COMPOSITIONS[name](pe, inj)
    wide_eng = wide.engine()
    if how == "hiprtc":
        monkeypatch.setenv("GWI_FORCE_JIT", "1")
        monkeypatch.setenv("GWI_JIT_CACHE", str(tmp_path))
    if how == "generic":
        monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    comp = COMPOSITIONS[name](pe, inj)
    eng = comp.engine(narrow_columns="auto" if how == "narrow" else False)
    if how == "hiprtc":
        assert eng.scan_kernel_name().startswith("jit:") and eng.jit_info()["compiled_at_run_time"]
    elif how == "generic":
        assert eng.scan_kernel_name().startswith("generic")
    else:
        assert len(eng.bound.narrowed) == 4 and "splinef" in eng.scan_kernel_name()
    thetas = _thetas(comp, name, 2, seed=11)
    _bracket_run(eng, wide_eng.bound, thetas, how)  # expected weights: the wide, ahead-of-time model's bound form
    eng.close()
    wide_eng.close()


def test_masks():
    """With the reference's mass cuts as the mask no masked sample is ever drawn; an event masked out entirely yields -1 and
    leaves the other events' (and the injections') indices as they were; NULL masks restore every sample."""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.draws import mass_cut_masks
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(12, 2500, 9000, seed=31)
    comp = COMPOSITIONS["plpeak"](pe, inj)
    eng = comp.engine()
    thetas = _thetas(comp, "plpeak", 2, seed=3)
    m_pe, m_inj = mass_cut_masks(pe, inj, 10.0, 8.0, 60.0)
    assert 0 < m_pe.sum() < m_pe.size and 0 < m_inj.sum() < m_inj.size
    u_pe, u_inj, free_pe, free_inj = _bracket_run(eng, eng.bound, thetas, "no mask")
    eng.set_draw_mask(m_pe, m_inj)
    _, _, cut_pe, cut_inj = _bracket_run(eng, eng.bound, thetas, "mass cuts", masks=(m_pe, m_inj))
    ev = np.arange(12)[None, :, None]
    drawn = cut_pe >= 0
    assert np.all(m_pe[np.broadcast_to(ev, cut_pe.shape)[drawn], cut_pe[drawn]] == 1) and np.all(m_inj[cut_inj[cut_inj >= 0]] == 1)
    assert np.any(cut_pe != free_pe) and np.any(cut_inj != free_inj)
    gone = m_pe.copy()
    gone[3] = 0
    eng.set_draw_mask(gone, m_inj)
    _, _, gone_pe, gone_inj = _bracket_run(eng, eng.bound, thetas, "event 3 masked out", masks=(gone, m_inj))
    assert np.all(gone_pe[:, 3] == -1)
    keep = np.arange(12) != 3
    assert np.array_equal(gone_pe[:, keep], cut_pe[:, keep]) and np.array_equal(gone_inj, cut_inj)
    eng.set_draw_mask(None, np.zeros(eng.n_inj, dtype=np.uint8))  # PE mask dropped, no injection may be drawn
    back_pe, none_inj = eng.draw_indices(thetas, u_pe, u_inj)
    assert np.array_equal(back_pe, free_pe) and np.all(none_inj == -1)
    eng.set_draw_mask()
    back_pe, back_inj = eng.draw_indices(thetas, u_pe, u_inj)
    assert np.array_equal(back_pe, free_pe) and np.array_equal(back_inj, free_inj)
    # either count may be 0
    only_pe, nothing = eng.draw_indices(thetas, u_pe, None)
    nothing2, only_inj = eng.draw_indices(thetas, None, u_inj)
    assert nothing is None and nothing2 is None and np.array_equal(only_pe, free_pe) and np.array_equal(only_inj, free_inj)
    eng.close()


@pytest.mark.parametrize("comp_name", ["plpeak", "bspline_iid"])
def test_pure_function_of_the_inputs(comp_name):
    """k = 1 repeated equals k = 20 in one call (more than max_batch); two handles of one model agree; draws placed between
    single and batched evaluations leave their results bit-identical."""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(11, 1300, 5003, seed=41)
    comp, comp2 = COMPOSITIONS[comp_name](pe, inj), COMPOSITIONS[comp_name](pe, inj)
    eng, eng2 = comp.engine(), comp2.engine()
    k = 20
    assert k > eng.max_batch
    thetas = _thetas(comp, comp_name, k, seed=7)
    rng = np.random.default_rng(2)
    u_pe, u_inj = rng.uniform(size=(k, eng.n_ev, 5)), rng.uniform(size=(k, 9))
    single = [eng.evaluate(t, total, min_neff_cut=False) for t in thetas[:4]]
    batch = eng.evaluate_batch(thetas[:16], total, min_neff_cut=False)
    all_pe, all_inj = eng.draw_indices(thetas, u_pe, u_inj)
    assert all_pe.shape == (k, eng.n_ev, 5) and all_inj.shape == (k, 9) and np.all(all_pe >= 0) and np.all(all_inj >= 0)
    for p in range(k):
        one_pe, one_inj = eng.draw_indices(thetas[p], u_pe[p], u_inj[p])
        assert one_pe.shape == (eng.n_ev, 5) and np.array_equal(one_pe, all_pe[p]) and np.array_equal(one_inj, all_inj[p])
        if p < 4:  # a single evaluation after a draw, then a batch: the same bits as before any draw
            again = eng.evaluate(thetas[p], total, min_neff_cut=False)
            assert again.log_likelihood == single[p].log_likelihood and np.array_equal(again.log_bfs, single[p].log_bfs)
            # (spline-coefficient gradients go through LDS atomics: last-bit run-to-run noise outside replay mode, test_gpu_parity.test_run_to_run_bit_stability)
            assert np.array_equal(again.grad, single[p].grad) if comp_name == "plpeak" else np.allclose(again.grad, single[p].grad, rtol=1e-12, atol=1e-13)
    batch2 = eng.evaluate_batch(thetas[:16], total, min_neff_cut=False)
    for a, b in zip(batch, batch2):
        assert a.log_likelihood == b.log_likelihood and np.array_equal(a.log_bfs, b.log_bfs)
        assert np.array_equal(a.grad, b.grad) if comp_name == "plpeak" else np.allclose(a.grad, b.grad, rtol=1e-12, atol=1e-13)
    other_pe, other_inj = eng2.draw_indices(thetas, u_pe, u_inj)
    assert np.array_equal(other_pe, all_pe) and np.array_equal(other_inj, all_inj)
    twice_pe, twice_inj = eng.draw_indices(thetas, u_pe, u_inj)
    assert np.array_equal(twice_pe, all_pe) and np.array_equal(twice_inj, all_inj)
    # log_weights keeps its behaviour next to the draws
    lw = eng.log_weights(thetas[0])
    ref = _bound_log_weights(eng.bound, thetas[0])
    for x, y in zip(lw, ref):
        ok = np.isfinite(y)
        assert np.array_equal(np.isfinite(x), ok) and np.max(np.abs(x[ok] - y[ok])) < 1e-9
    eng.close()
    eng2.close()


def test_buffer_lifetime_across_entries_of_one_handle():
    """The device buffers one handle keeps for draw_indices, weighted_histograms and resample_injections, grown, dropped and shared
    between the entries: engine A draws (2 draws per segment at K = 1, then 64 at K = 3, which regrows the uniforms and the
    indices), sums histograms at K = 2 with (C, B) = (1, 4) and, the bins dropped and set anew, (2, 16), resamples 8 and then 600
    injections (which regrows the output pair) and repeats its first draw; engine B, fresh on the same catalog, starts with the
    histograms, so that they and not the draws allocate the tile workspace, then resamples, then draws.  Every result of A equals
    B's bit for bit, A's last draw its first, and each the NumPy statement (gwinferno_amd/draws.py) under the neighbouring tests'
    bounds: the bracket of this file for every index; the drawn log-weights those of log_weights bit for bit and the sums within
    1e-9 of the host's (tests/test_gpu_resample.py); every bin within hist_util.bound of the statement fed with the engine's own
    log-weights (tests/test_gpu_hist.py) -- the bound of one point holds for the running sum of two: all terms are non-negative, so
    the sum of two bins each within tol of its statement is within tol of the statements' sum, and the one rounding the addition
    makes on either side (2^-53 each) is inside the 8 units of 2^-52 the bound has to spare.
    3 events x 1 500 PE samples (two tiles, the second partial) and 2 500 injections (three tiles)."""
    import hist_util
    import resample_util
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.draws import digitize, resample_uniforms, weighted_histograms_reference
    from gwinferno_amd.synthetic import make_catalog

    n_ev, seed = 3, 77
    pe, inj, total = make_catalog(n_ev, 1500, 2500, seed=61)
    comp_a, comp_b = COMPOSITIONS["plpeak"](pe, inj), COMPOSITIONS["plpeak"](pe, inj)
    thetas = _thetas(comp_a, "plpeak", 3, seed=5)
    rng = np.random.default_rng(8)
    u1, u64 = (rng.uniform(size=(n_ev, 2)), rng.uniform(size=2)), (rng.uniform(size=(3, n_ev, 64)), rng.uniform(size=(3, 64)))
    bins = {}
    for cols, n_bins in ((("mass_1",), 4), (("mass_1", "mass_2"), 16)):
        edges = {c: np.linspace(*np.quantile(np.concatenate([pe[c].ravel(), inj[c]]), [0.02, 0.98]), n_bins + 1) for c in cols}
        bins[n_bins] = (np.stack([digitize(pe[c], edges[c]) for c in cols]), np.stack([digitize(inj[c], edges[c]) for c in cols]))

    def draws(eng, out):
        out["draw 2"] = eng.draw_indices(thetas[0], *u1)
        out["draw 64"] = eng.draw_indices(thetas, *u64)

    def histograms(eng, out):
        for n_bins in (4, 16):
            eng.set_histogram_bins(*bins[n_bins], n_bins=n_bins)
            out["hist", n_bins] = eng.weighted_histograms(thetas[:2])

    def resamples(eng, out):
        for n in (8, 600):
            out["resample", n] = eng.resample_injections(thetas[0], seed, n_request=n)

    eng_a, eng_b = comp_a.engine(), comp_b.engine()
    a, b = {}, {}
    try:
        for step in (draws, histograms, resamples):
            step(eng_a, a)
        a["draw 2 again"] = eng_a.draw_indices(thetas[0], *u1)
        for step in (histograms, resamples, draws):
            step(eng_b, b)
        lw_dev = [eng_a.log_weights(t) for t in thetas[:2]]  # (after every step: log_weights shares the entries' buffers)
        lw_host = [_bound_log_weights(eng_a.bound, t) for t in thetas]
    finally:
        eng_a.close()
        eng_b.close()
    for key, got in b.items():
        for x, y in zip(a[key], got):
            assert x == y if isinstance(x, dict) else (x.dtype == y.dtype and np.array_equal(x, y)), key
    assert all(np.array_equal(x, y) for x, y in zip(a["draw 2 again"], a["draw 2"]))
    # ... and each against its statement
    _check_point(*lw_host[0], (None, None), *u1, *a["draw 2"], "draw 2")
    for p in range(3):
        _check_point(*lw_host[p], (None, None), u64[0][p], u64[1][p], a["draw 64"][0][p], a["draw 64"][1][p], ("draw 64", p))
    for lw in lw_dev:  # (hist_util.bound asks that no live weight underflows next to its segment's largest)
        assert all(np.min(seg[np.isfinite(seg)]) - np.max(seg[np.isfinite(seg)]) > hist_util.LOG_FLOOR for seg in (*lw[0], lw[1]))
    for n_bins in (4, 16):
        want = [weighted_histograms_reference(*lw, None, None, *bins[n_bins], n_bins) for lw in lw_dev]
        hist_pe, hist_inj, dead = a["hist", n_bins]
        assert dead.dtype == np.int32 and np.array_equal(dead, want[0][2] + want[1][2])
        for seg in range(n_ev + 1):
            g, w = (hist_pe[seg], want[0][0][seg] + want[1][0][seg]) if seg < n_ev else (hist_inj, want[0][1] + want[1][1])
            tol = hist_util.bound(max(hist_util.n_live(lw[0][seg] if seg < n_ev else lw[1], None) for lw in lw_dev))
            assert g.shape == w.shape == (len(bins[n_bins][0]), n_bins) and np.all(np.abs(g - w) <= tol * w), (n_bins, seg)
    host = resample_util.host_sums(lw_host[0][1])
    for n in (8, 600):
        idx, lw_sel, sums = a["resample", n]
        assert idx.dtype == np.int32 and idx.size == n and np.array_equal(lw_sel, lw_dev[0][1][idx])
        _check_segment(lw_host[0][1], None, resample_uniforms(seed, 0, n), idx, ("resample", n))
        assert abs(sums["log_sum_w"] - host["log_sum_w"]) <= 1e-9 and abs(sums["log_sum_w2"] - host["log_sum_w2"]) <= 1e-9
        assert abs(sums["n_eff"] - host["n_eff"]) <= 1e-9 * host["n_eff"] and sums["n_live"] == host["n_live"] > 0


def _chm_model(name, case):
    """construct_hierarchical_model's dictionaries for the golden case, as tests/test_gpu_dropin_api.py feeds them."""
    from gwinferno_amd import interpolation as I
    from gwinferno_amd import numpyro_distributions as D
    from gwinferno_amd.cosmology import planck15_lvk
    from gwinferno_amd.parser import PopModel, PopPrior

    cosmo = planck15_lvk()
    tables = {}

    def redshift(lamb, maximum, grid):
        dv = tables.setdefault(id(grid), (grid, cosmo.dVc_dz(grid)))[1]
        return D.PowerlawRedshift(lamb, maximum, zgrid=grid, dVcdz=dv)

    if name == "chm_powerlaw":
        model_dict = {"mass_1": PopModel(D.Powerlaw, ["alpha", "minimum", "maximum"]), "mass_ratio": PopModel(D.Powerlaw, ["alpha", "minimum", "maximum"]),
                      "redshift": PopModel(redshift, ["lamb", "maximum"])}
        sampled = lambda p: {"mass_1_alpha": p["alpha"], "mass_1_minimum": p["mmin"], "mass_1_maximum": p["mmax"], "mass_ratio_alpha": p["beta"], "redshift_lamb": p["lamb"]}  # noqa: E731
        consts = dict(mass_ratio_minimum=0.02, mass_ratio_maximum=1.0, redshift_maximum=1.9)
    else:
        m_grid, q_grid = np.linspace(case.meta["mmin"], case.meta["mmax"], 1000), np.linspace(0.0, 1.0, 1000)
        m_dmat = I.LogXLogYBSpline(16, xrange=(case.meta["mmin"], case.meta["mmax"]), normalize=True).bases(m_grid)
        q_dmat = I.LogYBSpline(10, xrange=(0.0, 1.0), normalize=True).bases(q_grid)
        names = ["minimum", "maximum", "cs", "grid", "grid_dmat"]
        model_dict = {"mass_1": PopModel(D.BSplineDistribution, names), "mass_ratio": PopModel(D.BSplineDistribution, names), "redshift": PopModel(redshift, ["lamb", "maximum"])}
        sampled = lambda p: {"mass_1_cs": p["m_coefs"], "mass_ratio_cs": p["q_coefs"], "redshift_lamb": p["lamb"]}  # noqa: E731
        consts = dict(mass_1_minimum=case.meta["mmin"], mass_1_maximum=case.meta["mmax"], mass_1_grid=m_grid, mass_1_grid_dmat=m_dmat, mass_ratio_minimum=0.0, mass_ratio_maximum=1.0,
                      mass_ratio_grid=q_grid, mass_ratio_grid_dmat=q_dmat, redshift_maximum=1.9)
    prior_dict = {k: PopPrior(None, {}) for k in sampled(case.point(0))}
    prior_dict.update(consts)
    return model_dict, prior_dict, sampled


@pytest.mark.parametrize("name", ["chm_powerlaw", "chm_bspline"])
def test_device_mode_of_hierarchical_likelihood_gives_the_host_modes_sites(name):
    """The reference's default call (posterior_predictive_check=True) on the golden chm_* cases: set_ppc_draws("device") gives
    the sites of the host mode.  Where an index differs, the host's own cdf must bracket u cdf[-1] within d at the device's
    index (a rounding tie); any other difference fails."""
    from gwinferno_amd import likelihood as L

    case = GoldenCase(name)
    model_dict, prior_dict, sampled = _chm_model(name, case)
    L.SAMPLE_VALUES["unscaled_rate"] = case.meta["unscaled_rate"]
    L.clear_engine_cache()
    cuts = dict(m1min=2.0, m2min=2.0, mmax=100.0)  # what construct_hierarchical_model passes (analysis.py:417-419)
    model = L.construct_hierarchical_model(model_dict, prior_dict)
    try:
        for i in range(case.n_points):
            L.SAMPLE_VALUES.update(sampled(case.point(i)))
            assert L.set_ppc_draws("host") in ("host", "device")
            model(case.pe, case.inj, case.total_inj, case.nobs, case.tobs)
            host = L.last_sites()
            L.set_ppc_draws("device")
            model(case.pe, case.inj, case.total_inj, case.nobs, case.tobs)
            dev = L.last_sites()
            assert len(L._ENGINES) == 1
            eng, pe_w, _, _ = L._ENGINES[next(reversed(L._ENGINES))]
            ppc = [s for s in host if "_obs_event_" in s or "_pred_event_" in s]
            assert len(ppc) == 2 * len(model_dict) * case.nobs and set(host) == set(dev)
            for s in host:
                if s in ppc:
                    continue
                if "grad" in s:  # (last-bit run-to-run noise of spline-coefficient gradients)
                    assert np.allclose(np.asarray(host[s]), np.asarray(dev[s]), rtol=1e-12, atol=1e-13, equal_nan=True), s
                else:
                    assert np.array_equal(np.asarray(host[s]), np.asarray(dev[s]), equal_nan=True), s
            if all(host[s] == dev[s] for s in ppc):
                continue
            # a differing site: only a rounding tie of the host's own cumulative weights may explain it
            theta = eng.bound.theta_of(pe_w)
            ih = L._ppc_indices_host(eng, theta, case.pe, case.inj, case.nobs, **cuts)
            idv = L._ppc_indices_device(eng, theta, case.pe, case.inj, case.nobs, **cuts)
            lw_pe, lw_inj = eng.log_weights(theta)
            u = L.ppc_uniforms(case.nobs)
            for side, lw_all, data in ((0, lw_pe, case.pe), (1, None, case.inj)):
                for ev in range(case.nobs):
                    if ih[side, ev] == idv[side, ev]:
                        continue
                    lw = lw_all[ev] if side == 0 else lw_inj
                    m1 = np.asarray(data["mass_1"])[ev] if side == 0 else np.asarray(data["mass_1"])
                    q = np.asarray(data["mass_ratio"])[ev] if side == 0 else np.asarray(data["mass_ratio"])
                    with np.errstate(all="ignore"):
                        w = np.exp(lw - np.max(lw))
                        w = np.where((m1 < 2.0) | (m1 > 100.0) | (m1 * q < 2.0) | ~np.isfinite(w), 0.0, w)
                    cdf = np.cumsum(w)
                    j, d, t = int(idv[side, ev]), BAND * cdf[-1], u[side, ev] * cdf[-1]
                    assert w[j] > 0 and (cdf[j - 1] if j else 0.0) - d <= t < cdf[j] + d, (name, i, side, ev, int(ih[side, ev]), j)
            for s in ppc:  # ... and the sites are the catalog's values at those indices
                p, kind, ev = s.rsplit("_event_", 1)[0].rsplit("_", 1)[0], s.rsplit("_event_", 1)[0].rsplit("_", 1)[1], int(s.rsplit("_", 1)[1])
                want = np.asarray(case.pe[p])[ev, idv[0, ev]] if kind == "obs" else np.asarray(case.inj[p])[idv[1, ev]]
                assert dev[s] == want, s
    finally:
        L.set_ppc_draws("host")
        L.clear_engine_cache()


def test_posterior_predictive_draws():
    """Shapes, determinism in the seed, gathered parameters; with 4 096 draws of one event the drawn frequencies of the ten
    heaviest samples lie within five binomial standard deviations of their normalised weights."""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.draws import draw_weights, mass_cut_masks
    from gwinferno_amd.postprocess import posterior_predictive_draws
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(7, 900, 5000, seed=17)
    comp = COMPOSITIONS["plpeak"](pe, inj)
    eng = comp.engine()
    thetas = _thetas(comp, "plpeak", 3, seed=9)
    names = ["mass_1", "mass_ratio", "redshift"]
    cuts = dict(m1min=5.0, m2min=3.0, mmax=100.0)
    a = posterior_predictive_draws(eng, thetas, 6, seed=4, pedata=pe, injdata=inj, param_names=names, **cuts)
    b = posterior_predictive_draws(eng, thetas, 6, seed=4, pedata=pe, injdata=inj, param_names=names, **cuts)
    c = posterior_predictive_draws(eng, thetas, 6, seed=5)
    assert a["obs_idx"].shape == (3, 7, 6) and a["pred_idx"].shape == (3, 6) and a["obs_idx"].dtype == np.int32
    assert np.array_equal(a["obs_idx"], b["obs_idx"]) and np.array_equal(a["pred_idx"], b["pred_idx"])
    assert not np.array_equal(a["obs_idx"], c["obs_idx"]) and set(c) == {"obs_idx", "pred_idx"}
    m_pe, m_inj = mass_cut_masks(pe, inj, **cuts)
    ev = np.arange(7)[None, :, None]
    assert np.all(a["obs_idx"] >= 0) and np.all(a["pred_idx"] >= 0)
    assert np.all(m_pe[np.broadcast_to(ev, a["obs_idx"].shape), a["obs_idx"]] == 1) and np.all(m_inj[a["pred_idx"]] == 1)
    for p in names:
        assert a["obs"][p].shape == (3, 7, 6) and a["obs_pooled"][p].shape == (3, 42) and a["pred"][p].shape == (3, 6)
        assert np.array_equal(a["obs"][p], pe[p][ev, a["obs_idx"]]) and np.array_equal(a["pred"][p], inj[p][a["pred_idx"]])
        assert np.array_equal(a["obs_pooled"][p], a["obs"][p].reshape(3, -1))
    # frequencies: one hyper-parameter point, 4 096 draws per event; event 0 against its normalised weights
    n = 4096
    big = posterior_predictive_draws(eng, thetas[:1], n, seed=11)
    lw_pe, lw_inj = _bound_log_weights(eng.bound, thetas[0])
    for what, idx, lw, mask in (("event 0", big["obs_idx"][0, 0], lw_pe[0], m_pe[0]), ("injections", big["pred_idx"][0], lw_inj, m_inj)):
        w = draw_weights(lw, mask)
        prob = w / w.sum()
        counts = np.bincount(idx, minlength=w.size)
        assert counts.sum() == n and np.all(counts[w == 0] == 0)
        for j in np.argsort(prob)[-10:]:
            assert abs(counts[j] / n - prob[j]) <= 5.0 * np.sqrt(prob[j] * (1.0 - prob[j]) / n), (what, int(j), int(counts[j]), float(prob[j]))
    eng.close()


def test_error_paths():
    """A sharded handle (GWI_ERR_UNSUPPORTED, from Python and from the library), a mask of the wrong length, null outputs with
    non-zero counts, bad counts: each with a message, and the engine keeps working afterwards."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.engine import NativePopulationLikelihood
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(6, 300, 2000, seed=3)
    comp = COMPOSITIONS["plpeak"](pe, inj)
    eng = comp.engine()
    theta = _thetas(comp, "plpeak", 1, seed=1)[0]
    u_pe, u_inj = np.full((6, 2), 0.5), np.full(3, 0.5)
    good = eng.draw_indices(theta, u_pe, u_inj)
    with pytest.raises(ValueError, match="pe_mask has shape"):
        eng.set_draw_mask(np.ones(6 * 300 - 1, dtype=np.uint8), None)
    with pytest.raises(ValueError, match="inj_mask has shape"):
        eng.set_draw_mask(None, np.ones(2001, dtype=np.uint8))
    with pytest.raises(ValueError, match="u_pe has shape"):
        eng.draw_indices(theta, np.full((5, 2), 0.5), None)
    lib, dp, ip = eng.lib, N.as_dp, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    th, up, ui = N.f64(theta), N.f64(u_pe), N.f64(u_inj)
    out_pe, out_inj = np.zeros((6, 2), dtype=np.int32), np.zeros(3, dtype=np.int32)
    for args, word in (((dp(th), 1, dp(up), 2, dp(ui), 3, None, ip(out_inj)), "idx_pe"), ((dp(th), 1, dp(up), 2, dp(ui), 3, ip(out_pe), None), "idx_inj"),
                       ((dp(th), 1, None, 2, dp(ui), 3, ip(out_pe), ip(out_inj)), "u_pe"), ((dp(th), 0, dp(up), 2, dp(ui), 3, ip(out_pe), ip(out_inj)), "k < 1"),
                       ((dp(th), 1, dp(up), -1, dp(ui), 3, ip(out_pe), ip(out_inj)), "negative"), ((None, 1, dp(up), 2, dp(ui), 3, ip(out_pe), ip(out_inj)), "thetas")):
        assert lib.gwi_draw_indices(eng.handle, *args) == -1  # GWI_ERR_INVALID
        assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
    assert lib.gwi_draw_indices(eng.handle, dp(th), 1, None, 0, None, 0, None, None) == 0  # nothing asked for: nothing done
    again = eng.draw_indices(theta, u_pe, u_inj)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    eng.close()
    # shards: the Python engine refuses by its own world size; the library refuses a handle that has joined a communicator of two
    p = comp.placeholder()
    shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
        shards[0].draw_indices(theta, np.full((shards[0].n_ev, 1), 0.5), None)
    seg = f"/gwi_draw_test_{os.getpid()}"
    try:
        for r, s in enumerate(shards):
            s.shm_comm_init(seg, r, 2)
        up0 = N.f64(np.full((shards[0].n_ev, 1), 0.5))
        out0 = np.zeros((shards[0].n_ev, 1), dtype=np.int32)
        assert lib.gwi_draw_indices(shards[0].handle, dp(th), 1, dp(up0), 1, None, 0, ip(out0), None) == -4  # GWI_ERR_UNSUPPORTED
        assert "shard" in lib.gwi_last_error(shards[0].handle).decode()
    finally:
        lib.gwi_shm_comm_unlink(seg.encode())
        for s in shards:
            s.close()
