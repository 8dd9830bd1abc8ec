"""CPU: weighted kernel density estimates of the marginal weights (include/gwi_engine.h: gwi_set_kde_columns, gwi_weighted_kde,
gwi_weighted_kde2d; gwinferno_amd/csrc/gwi_kde.h) -- the NumPy statement (gwinferno_amd/draws.py: weighted_kde_reference,
weighted_kde2d_reference) against scipy.stats.gaussian_kde, reflection, the segments without a curve,
postprocess.event_posterior_densities(backend="host"), the header, the binding and the refusals that need no device, and the inputs
of tests/test_gpu_kde.py, which are vetted here."""
import ctypes as C
import os
import re

import hist_util as U
import kde_util as KU
import numpy as np
import pytest
import quant_util as QU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segments():
    """Seeded segments ``(W, broad, tight)``: 1 500 and 2 600 samples with a third of the weights zero, and one of 7 samples."""
    rng = np.random.default_rng(21)
    out = []
    for n in (1500, 2600, 7):
        W = rng.lognormal(0.0, 1.5, n)
        if n > 7:
            W[rng.permutation(n)[: n // 3]] = 0.0
        out.append((W, rng.lognormal(3.0, 0.5, n), rng.normal(30.0, 0.03, n)))  # a broad quantity and a tight one (mean 30, sd 0.03)
    return out


def _relative(got, want):
    """The largest relative deviation over the points whose density is at least 1e-30 of the peak."""
    held = want >= 1e-30 * want.max()
    return float(np.max(np.abs(got - want)[held] / want[held]))


def test_statement_against_scipy():
    """weighted_kde_reference and weighted_kde2d_reference against scipy.stats.gaussian_kde(weights=W, bw_method=...) for Scott,
    Silverman and a scalar scale: 1e-9 relative (the project's parity bar) at every grid point whose density is at least 1e-30 of the
    segment's peak (G = 300; 33 x 20).  The tight quantity exposes an uncentred variance: m2 / mass - mean^2 at mean 30, sd 0.03 keeps
    ten digits fewer."""
    from scipy.stats import gaussian_kde

    from gwinferno_amd import draws as D

    worst1, worst2 = 0.0, 0.0
    for W, broad, tight in _segments():
        for rule, scale in (("scott", 1.0), ("silverman", 1.0), ("scott", 0.6), ("silverman", 1.7)):
            for x in (broad, tight):
                grid = np.linspace(x.min() - 0.2 * np.ptp(x), x.max() + 0.2 * np.ptp(x), 300)
                rho, h, neff, flag = D.weighted_kde_reference(W, x, grid, rule, scale)
                assert flag == 0 and abs(neff - W.sum() ** 2 / (W * W).sum()) <= 1e-12 * neff
                ref = gaussian_kde(x, weights=W, bw_method=lambda k, r=rule, s=scale: s * (k.scotts_factor() if r == "scott" else k.silverman_factor()))
                assert abs(h - np.sqrt(ref.covariance[0, 0])) <= 1e-9 * h and abs(neff - ref.neff) <= 1e-12 * neff
                worst1 = max(worst1, _relative(rho, ref(grid)))
            gx, gy = np.linspace(broad.min(), broad.max(), 33), np.linspace(tight.min(), tight.max(), 20)
            rho, H, neff, flag = D.weighted_kde2d_reference(W, broad, tight, gx, gy, rule, scale)
            ref = gaussian_kde(np.vstack([broad, tight]), weights=W, bw_method=lambda k, r=rule, s=scale: s * (k.scotts_factor() if r == "scott" else k.silverman_factor()))
            assert flag == 0 and np.allclose(H, ref.covariance[[0, 0, 1], [0, 1, 1]], rtol=1e-9, atol=0)
            X, Y = np.meshgrid(gx, gy, indexing="ij")
            worst2 = max(worst2, _relative(rho, ref(np.vstack([X.ravel(), Y.ravel()])).reshape(33, 20)))
    print(f"largest relative deviation from scipy: {worst1:.2e} in 1-D, {worst2:.2e} in 2-D")
    assert worst1 <= 1e-9 and worst2 <= 1e-9, (worst1, worst2)
    # a Scott curve is the Silverman curve of d = 1 at the ratio of the factors
    W, broad, _ = _segments()[0]
    a = D.weighted_kde_reference(W, broad, [20.0, 25.0], "silverman")
    b = D.weighted_kde_reference(W, broad, [20.0, 25.0], "scott", scale=(3.0 / 4.0) ** -0.2)
    assert np.allclose(a[0], b[0], rtol=1e-13, atol=0) and abs(a[1] - b[1]) <= 1e-14 * a[1]


def test_reflection():
    """The reflected curve of a Beta-like sample on [0, 1] integrates to 1 (a 513-point grid, trapezoid: the reflected Gaussian sum
    has zero slope at either bound, so the quadrature error is of higher order), is 0 outside the bounds, and its bandwidth is the
    unreflected one; one bound alone reflects on that side only."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(22)
    x, W = rng.beta(5.0, 1.2, 2000), rng.lognormal(0.0, 1.0, 2000)
    grid = np.linspace(0.0, 1.0, 513)
    rho, h, neff, flag = D.weighted_kde_reference(W, x, grid, bounds=(0.0, 1.0))
    plain, h0, neff0, _ = D.weighted_kde_reference(W, x, grid)
    total = float(np.sum(0.5 * (rho[1:] + rho[:-1]) * np.diff(grid)))
    print(f"the reflected curve integrates to {total:.12f}; the unreflected one to {float(np.sum(0.5 * (plain[1:] + plain[:-1]) * np.diff(grid))):.6f}")
    assert flag == 0 and h == h0 and neff == neff0 and abs(total - 1.0) <= 1e-6
    assert np.all(rho >= plain) and rho[-1] > 1.9 * plain[-1]  # at the bound itself the image doubles the sample's own kernel
    outside = D.weighted_kde_reference(W, x, [-0.5, -1e-12, 0.0, 1.0, 1.0 + 1e-12, 2.0], bounds=(0.0, 1.0))[0]
    assert np.array_equal(outside[[0, 1, 4, 5]], np.zeros(4)) and outside[2] >= 0.0 and outside[3] > 0.0
    upper = D.weighted_kde_reference(W, x, [-0.5, 0.3, 1.0, 1.5], bounds=(None, 1.0))[0]
    assert upper[0] >= 0.0 and upper[1] > 0.0 and upper[3] == 0.0 and upper[2] > 1.9 * plain[-1]  # (-0.5 is inside: no lower bound)
    both_nan = D.weighted_kde_reference(W, x, grid, bounds=(np.nan, None))[0]
    assert np.array_equal(both_nan, plain)


def test_segments_without_a_curve():
    """A dead segment: NaN, n_eff = 0, no flag (so does everything when nothing is accumulated).  A single sample with weight and a
    zero variance: NaN and the flag.  Bad arguments raise."""
    from gwinferno_amd import draws as D

    x, y, g = np.array([1.0, 2.0, 4.0, 8.0]), np.array([1.0, 3.0, 2.0, 5.0]), np.array([0.0, 2.0])
    for W, flag, neff in ((np.zeros(4), 0, 0.0), (np.array([0.0, 3.0, 0.0, 0.0]), 1, 1.0)):
        rho, h, n_eff, got = D.weighted_kde_reference(W, x, g)
        assert np.all(np.isnan(rho)) and np.isnan(h) and n_eff == neff and got == flag
        rho2, H, n_eff, got = D.weighted_kde2d_reference(W, x, y, g, g)
        assert rho2.shape == (2, 2) and np.all(np.isnan(rho2)) and np.all(np.isnan(H)) and n_eff == neff and got == flag
    rho, h, n_eff, got = D.weighted_kde_reference(np.ones(4), np.full(4, 3.0), g)  # no variance
    assert np.all(np.isnan(rho)) and np.isnan(h) and n_eff == 4.0 and got == 1
    rho2, H, n_eff, got = D.weighted_kde2d_reference(np.ones(4), x, 2.0 * x, g, g)  # a singular covariance
    assert np.all(np.isnan(rho2)) and got == 1 and abs(n_eff - 4.0) <= 1e-15
    ok = D.weighted_kde_reference(np.array([1.0, 1.0, 0.0, 0.0]), x, g)  # two samples with weight are enough
    assert ok[3] == 0 and np.all(np.isfinite(ok[0])) and abs(ok[2] - 2.0) <= 1e-15
    for bad in (dict(rule="sheather"), dict(scale=0.0), dict(scale=np.nan), dict(grid=[np.inf]), dict(W=[1.0, -1.0, 0.0, 0.0]), dict(x=[1.0, np.nan, 0.0, 0.0])):
        kw = dict(W=np.ones(4), x=x, grid=g)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.weighted_kde_reference(**kw)


def test_new_symbols_in_binding_header_and_library():
    from gwinferno_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    raw = C.CDLL(_native.LIB_PATH)
    want = {"gwi_set_kde_columns": 5, "gwi_weighted_kde": 10, "gwi_weighted_kde2d": 14, "gwi_kde_times": 4}
    for sym, n_args in want.items():
        assert sym in declared and hasattr(raw, sym) and len(getattr(lib, sym).argtypes) == n_args, sym
        assert sym in _native.EXPORTED_SYMBOLS or not re.fullmatch(r"gwi_[a-z_]+", sym), sym  # (the list holds names of letters and underscores)
    assert lib.gwi_abi_version() == 3  # added exports, no struct changed
    assert lib.gwi_set_kde_columns(None, 1, None, None, None) == -1 and lib.gwi_weighted_kde(None, None, 1, 0, 1.0, None, None, None, None, None) == -1
    assert lib.gwi_weighted_kde2d(None, None, 1, None, 1, None, 1, 0, 1.0, None, None, None, None, None) == -1


def test_host_only_handle_and_validation():
    """A host-only handle answers GWI_ERR_INVALID with a message from every entry (the library refuses it before it looks at the
    other arguments, as every post-processing entry does); the counts, the rule, the scale and the grid are refused by the Python
    layer before the library is asked -- the library's own messages for them need a device: tests/test_gpu_kde.py."""
    from gwinferno_amd import _native as N

    eng = U.composition("plpeak", device=N.DEVICE_HOST_ONLY).engine()
    vp, vi = QU.columns(1)
    grid = KU.grid(1, 5)
    for call in (lambda: eng.set_kde_columns(vp, vi), lambda: eng.weighted_kde(grid), lambda: eng.weighted_kde2d([(0, 0)], grid[0], grid[0])):
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
            call()
    lib, i32 = eng.lib, C.POINTER(C.c_int32)
    rho_pe, rho_inj, bw, neff, flags = np.zeros((U.N_EV, 1, 5)), np.zeros((1, 5)), np.zeros((U.N_EV + 1, 3)), np.zeros(U.N_EV + 1), np.zeros((U.N_EV + 1, 1), dtype=np.int32)
    pairs = np.zeros((1, 2), dtype=np.int32)
    for st in (lib.gwi_set_kde_columns(eng.handle, 1, N.as_dp(vp), N.as_dp(vi), None),
               lib.gwi_weighted_kde(eng.handle, N.as_dp(grid), 5, 0, 1.0, N.as_dp(rho_pe), N.as_dp(rho_inj), N.as_dp(bw), N.as_dp(neff), flags.ctypes.data_as(i32)),
               lib.gwi_weighted_kde(eng.handle, N.as_dp(grid), 0, 7, -1.0, None, None, None, None, None),
               lib.gwi_weighted_kde2d(eng.handle, pairs.ctypes.data_as(i32), 1, N.as_dp(grid), 5, N.as_dp(grid), 1, 0, 1.0, N.as_dp(rho_pe), N.as_dp(rho_inj), N.as_dp(bw), N.as_dp(neff),
                                      flags.ctypes.data_as(i32))):
        assert st == -1 and "host-only" in lib.gwi_last_error(eng.handle).decode()
    with pytest.raises(ValueError, match="both None"):
        eng.set_kde_columns()
    with pytest.raises(ValueError, match="pe_values has shape"):
        eng.set_kde_columns(vp[:, :, :-1], vi)
    with pytest.raises(ValueError, match="inj_values has shape"):
        eng.set_kde_columns(vp, vi[:, :-1])
    with pytest.raises(ValueError, match="columns"):
        eng.set_kde_columns(np.concatenate([vp, vp]), vi)
    with pytest.raises(ValueError, match="between 1 and 8"):
        eng.set_kde_columns(np.concatenate([vp] * 9), np.concatenate([vi] * 9))
    bad = vi.copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="inj_values holds values that are not finite"):
        eng.set_kde_columns(vp, bad)
    with pytest.raises(ValueError, match="bounds has shape"):
        eng.set_kde_columns(vp, vi, bounds=[(0.0, 1.0), (0.0, 1.0)])
    with pytest.raises(ValueError, match="lo lies below hi"):
        eng.set_kde_columns(vp, vi, bounds=[(1.0, 0.0)])
    with pytest.raises(ValueError, match="grid has shape"):   # bad counts
        eng.weighted_kde(np.zeros(1025))
    with pytest.raises(ValueError, match="grid has shape"):
        eng.weighted_kde(np.zeros((1, 0)))
    with pytest.raises(ValueError, match="gridx has shape"):
        eng.weighted_kde2d([(0, 0)], np.zeros(129), np.zeros(3))
    with pytest.raises(ValueError, match="between 1 and 4"):
        eng.weighted_kde2d([(0, 0)] * 5, np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError, match="rule must be"):      # bad rule
        eng.weighted_kde(grid, rule="sheather")
    for scale in (0.0, -1.0, np.nan, np.inf):                  # bad scale
        with pytest.raises(ValueError, match="scale must be"):
            eng.weighted_kde(grid, scale=scale)
    with pytest.raises(ValueError, match="grid points must be finite"):  # a grid point that is not finite
        eng.weighted_kde(np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="grid points must be finite"):
        eng.weighted_kde2d([(0, 0)], np.array([1.0, np.inf]), np.zeros(3))


def test_world_above_one_is_refused_in_python():
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    eng = object.__new__(NativePopulationLikelihood)
    eng.world = 2
    for call, name in ((lambda: eng.set_kde_columns(np.zeros((1, 1, 1))), "set_kde_columns"), (lambda: eng.weighted_kde([0.5]), "weighted_kde"),
                       (lambda: eng.weighted_kde2d([(0, 0)], [0.5], [0.5]), "weighted_kde2d")):
        with pytest.raises(N.NativeEngineError, match=f"GWI_ERR_UNSUPPORTED: {name}: this engine holds one shard of the catalog"):
            call()


class _StubEngine:
    """What event_posterior_densities(backend="host") needs of an engine: the shapes and the marginal weights."""

    def __init__(self, W_pe, W_inj, dead):
        self.W_pe, self.W_inj, self.dead = W_pe, W_inj, dead
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta, self.calls = W_pe.shape, W_inj.size, 1, []

    def marginal_weights_reset(self):
        self.calls.append("reset")

    def marginal_weights_add(self, thetas):
        self.calls.append(("add", len(thetas)))

    def marginal_weights(self, weights=True):
        return self.W_pe.copy(), self.W_inj.copy(), self.dead.copy(), 4


def test_event_posterior_densities_on_the_host():
    """The host backend is the statement on the engine's marginal weights; names and arrays; pairs by name and by index; a dead event
    gives NaN without a flag; accumulate=False leaves the weights alone; the argument checks."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import postprocess as P

    rng = np.random.default_rng(23)
    n_ev, n_pe, n_inj = 3, 200, 350
    W_pe, W_inj = rng.lognormal(0.0, 1.0, (n_ev, n_pe)), rng.lognormal(0.0, 1.0, n_inj)
    W_pe[1] = 0.0
    eng = _StubEngine(W_pe, W_inj, np.array([0, 4, 0, 0], dtype=np.int32))
    pe_values = {"a": rng.normal(0.0, 1.0, (n_ev, n_pe)), "q": rng.beta(4.0, 1.5, (n_ev, n_pe))}
    inj_values = {"a": rng.normal(0.0, 1.0, n_inj), "q": rng.beta(4.0, 1.5, n_inj)}
    grid = {"a": np.linspace(-3.0, 3.0, 40), "q": np.linspace(-0.1, 1.1, 40)}
    thetas = np.zeros((4, 1))
    out = P.event_posterior_densities(eng, thetas, pe_values, grid, pairs=[("a", "q")], grid2d=(np.linspace(-2, 2, 9), np.linspace(0.1, 0.9, 6)), inj_values=inj_values,
                                      bounds={"q": (0.0, 1.0)}, backend="host")
    assert eng.calls == ["reset", ("add", 4)] and out["names"] == ["a", "q"] and out["n_points"] == 4
    assert out["density"].shape == (n_ev, 2, 40) and out["density_inj"].shape == (2, 40) and out["density2d"].shape == (n_ev, 1, 9, 6) and out["density2d_inj"].shape == (1, 9, 6)
    assert out["bandwidth"].shape == (n_ev, 2) and out["neff"].shape == (n_ev,) and out["covariance"].shape == (n_ev, 1, 3) and np.array_equal(out["pairs"], [[0, 1]])
    assert np.array_equal(out["dead"], [0, 4, 0]) and out["dead_inj"] == 0 and not out["degenerate"].any() and not out["degenerate2d"].any()
    assert np.all(np.isnan(out["density"][1])) and np.all(np.isnan(out["density2d"][1])) and np.all(np.isnan(out["bandwidth"][1])) and out["neff"][1] == 0.0
    want = D.weighted_kde_reference(W_pe[2], pe_values["q"][2], grid["q"], bounds=(0.0, 1.0))
    assert np.array_equal(out["density"][2, 1], want[0]) and out["bandwidth"][2, 1] == want[1] and out["neff"][2] == want[2]
    assert not out["density"][2, 1][grid["q"] < 0.0].any() and not out["density"][2, 1][grid["q"] > 1.0].any()
    want = D.weighted_kde2d_reference(W_inj, inj_values["a"], inj_values["q"], np.linspace(-2, 2, 9), np.linspace(0.1, 0.9, 6))
    assert np.array_equal(out["density2d_inj"][0], want[0]) and np.array_equal(out["covariance_inj"][0], want[1])
    named = P.event_posterior_densities(eng, thetas, None, grid["q"], pairs=[(0, 0)], grid2d=(grid["q"][:5], grid["q"][:4]), pedata=pe_values, injdata=inj_values,
                                        param_names=["q"], rule="silverman", scale=0.8, backend="host", accumulate=False)
    assert eng.calls == ["reset", ("add", 4)] and named["names"] == ["q"] and named["density"].shape == (n_ev, 1, 40)
    assert np.array_equal(named["density"][0, 0], D.weighted_kde_reference(W_pe[0], pe_values["q"][0], grid["q"], "silverman", 0.8)[0])
    assert named["degenerate2d"][0, 0] == 1 and named["degenerate2d"][1, 0] == 0  # (q against itself: a singular covariance; the dead event is not flagged)
    only_pe = P.event_posterior_densities(eng, thetas, pe_values, grid, backend="host")
    assert "density_inj" not in only_pe and "density2d" not in only_pe and np.array_equal(only_pe["density"][:, 0], out["density"][:, 0], equal_nan=True)
    for bad, match in ((dict(grid=np.zeros((3, 5))), "grid has shape"), (dict(grid=np.zeros(1025)), "grid has shape"), (dict(rule="sheather"), "rule must be"), (dict(scale=0.0), "scale must be"),
                       (dict(backend="eager"), "backend"), (dict(pairs=[("a", "q")]), "pairs need grid2d"), (dict(bounds={"z": (0, 1)}), "not one of the quantities"),
                       (dict(pairs=[(0, 2)], grid2d=(grid["a"], grid["a"])), "between 1 and 4 pairs"), (dict(pairs=[(0, 1)], grid2d=(np.zeros(129), grid["a"])), "grid2d holds"),
                       (dict(m1min=5.0), "together or not at all"), (dict(grid={"a": [np.nan], "q": [0.5]}), "grid points must be finite")):
        kw = dict(pe_values=pe_values, grid=grid, backend="host")
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            P.event_posterior_densities(eng, thetas, **kw)
    with pytest.raises(ValueError, match="no point"):
        P.event_posterior_densities(eng, np.zeros((0, 1)), pe_values, grid, backend="host")


@pytest.mark.parametrize("name", U.COMPS)
def test_inputs_of_the_gpu_tests(name):
    """CONDITION, not measurement.  Every case tests/test_gpu_kde.py compares, from the host evaluation of the bound model: the columns
    and grids are finite; the injection set spans three sample chunks, the last ragged, and an event two; the grids have fewer points
    than a wave has lanes and a ragged second (1-D) and third (2-D) grid block; the reflection grid has points outside either bound,
    on either bound and inside; no segment is degenerate or dead unless the mask case means it to be -- every other one has at least
    200 samples with weight, a positive variance in every column and, for every pair, |Hxy| >= 0.02 sqrt(Hxx Hyy) (so that H's
    off-diagonal entry can be held to 1e-12 relative) and 1 - r^2 >= 0.01."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.draws import marginal_weights_reference, weighted_kde2d_reference, weighted_kde_reference

    vp, vi = QU.columns(8)
    assert vp.shape == (8, U.N_EV, U.N_PE) and vi.shape == (8, U.N_INJ) and np.all(np.isfinite(vp)) and np.all(np.isfinite(vi))
    assert -(-U.N_INJ // KU.CHUNK) == 3 and U.N_INJ % KU.CHUNK not in (0,) and -(-U.N_PE // KU.CHUNK) == 2 and U.N_PE % KU.CHUNK
    assert KU.N_GRID[0] < 64 and KU.GRID_BLOCK < KU.N_GRID[1] < 2 * KU.GRID_BLOCK and KU.SHAPE_1[0] * KU.SHAPE_1[1] < 64
    assert 2 * KU.GRID_BLOCK < KU.SHAPE_2[0] * KU.SHAPE_2[1] < 3 * KU.GRID_BLOCK
    for n_cols in (1, 8):
        for g in KU.N_GRID:
            grid = KU.grid(n_cols, g)
            assert grid.shape == (n_cols, g) and np.all(np.isfinite(grid)) and np.any(np.diff(grid[0]) < 0)  # (not sorted)
    rg, (lo, hi) = KU.reflection_grid(), KU.Q_BOUNDS
    assert np.any(rg < lo) and np.any(rg == lo) and np.any((rg > lo) & (rg < hi)) and np.any(rg == hi) and np.any(rg > hi)
    assert QU.COLUMNS_8[KU.Q_COLUMN] == "mass_ratio" and vp[KU.Q_COLUMN].min() > lo and max(vp[KU.Q_COLUMN].max(), vi[KU.Q_COLUMN].max()) <= hi
    comp = U.composition(name, device=N.DEVICE_HOST_ONLY)
    thetas = U.points(comp, name, KU.K)
    lw = [U.host_log_weights(comp.engine().bound, th) for th in thetas]
    lw_pe, lw_inj = np.stack([a for a, _ in lw]), np.stack([b for _, b in lw])
    checked = 0
    for case in U.MASK_CASES:
        pm, im = U.masks(case)
        W_pe, W_inj, dead, _ = marginal_weights_reference(lw_pe, lw_inj, pm, im)
        for seg in range(U.N_EV + 1):
            W = W_pe[seg] if seg < U.N_EV else W_inj
            if dead[seg]:
                assert case == "masked" and seg == U.DEAD_EVENT and not W.any()
                continue
            assert np.count_nonzero(W > 0) >= 200
            for c in range(8):
                x = vp[c, seg] if seg < U.N_EV else vi[c]
                rho, h, neff, flag = weighted_kde_reference(W, x, KU.grid(8, 5)[c])
                assert flag == 0 and h > 0 and neff > 20 and np.all(np.isfinite(rho)), (name, case, seg, c)
                checked += 1
            for cx, cy in KU.PAIRS_1 + KU.PAIRS_2:
                x, y = (vp[cx, seg], vp[cy, seg]) if seg < U.N_EV else (vi[cx], vi[cy])
                _, H, _, flag = weighted_kde2d_reference(W, x, y, [x[0]], [y[0]])
                r2 = H[1] ** 2 / (H[0] * H[2])
                assert flag == 0 and 0.02**2 <= r2 <= 0.99, (name, case, seg, cx, cy, r2)
    assert checked == (4 + 3) * 8
