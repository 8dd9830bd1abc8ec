"""GPU: gwi_table_draws (gwinferno_amd/csrc/gwi_popdraw.h) against its NumPy statement (gwinferno_amd/population_draws.py) and against
the tables' own CDF in numpy.longdouble.

The kernel and the statement evaluate the same fp64 expressions on bit-identical uniforms (no contraction on the device), and the
statement sums the prefix in the kernel's own shape (population_draws.block_scan_prefix), so the two are expected to agree to the
bit; what is ASKED is |x_dev - x_host| <= 1e-9 (hi - lo) for all but at most 1 draw in 1e5 per table (a target within rounding of a
cell edge next to a run of cells without mass may land on either side of the gap).  The shape of the sum matters: with numpy.cumsum in
the statement the untruncated draws stay within that cap (tests/test_population_draws_cpu.py confirms it for two orders on the same
tables), but truncated draws whose bound keeps a fraction eps of a table's mass are differences of prefixes, precise to 2^-52 / eps
of the kept part, and on the steep table (1e12 end to end) 86 of 1000 moved by up to 3.3e-7 of the range between the two orders.
The CPU file also confirms that the inputs of the truncated draws keep every v further than 1e-9 from its mass, so `accept` is asked
byte for byte.  The device's draws satisfy the statement's own bound against the long-double CDF,
|CDF(x) - target| / C_last <= 4 G 2^-52."""
import numpy as np
import pytest
from popdraw_util import KS_POINT, LD, curve_cdf01, ks_distance, ld_cdf, make_tables, mesh_marginals, residual_bound, truncation_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    from gwinferno_amd import population_draws

    return population_draws


def close_enough(x_dev, x_host, lo, hi):
    far = np.abs(x_dev - x_host) > 1e-9 * (hi - lo)[:, None]
    allowed = max(1, x_dev.shape[1] // 100_000)
    assert np.all(far.sum(axis=1) <= allowed), (far.sum(axis=1), float(np.max(np.abs(x_dev - x_host) / (hi - lo)[:, None])))
    return int(far.sum())


@pytest.mark.parametrize("n_grid", [2, 5, 257, 1500])
@pytest.mark.parametrize("n_tables", [1, 3, 17])
def test_kernel_against_statement(P, n_grid, n_tables):
    """Every table kind (smooth, flat, from density 0, steep 1e12, leading / trailing / interior zero runs) at n_tables = 17; partial
    waves and partial blocks through n_draws."""
    lo, hi, pdf = make_tables(n_tables, n_grid, seed=n_grid)
    bound = residual_bound(n_grid)
    for n in (1, 63, 64, 65, 1000):
        x = P.table_draws(lo, hi, pdf, n, seed=11)
        assert x.shape == (n_tables, n)
        host = P.table_draws(lo, hi, pdf, n, seed=11, backend="host")
        moved = close_enough(x, host, lo, hi)
        worst = 0.0
        for t in range(n_tables):
            assert np.all((x[t] >= lo[t]) & (x[t] <= hi[t]))
            u, _ = P.draw_uniforms(11, 0, n, t)
            c, tot = ld_cdf(lo[t], hi[t], pdf[t], x[t])
            worst = max(worst, float(np.max(np.abs(c / tot - u.astype(LD)))))
        print(f"G = {n_grid}, {n_tables} tables, n = {n}: largest CDF residual {worst:.3e} (bound {bound:.3e}), bit-equal to the statement: "
              f"{int(np.sum(x == host))} of {x.size}, beyond 1e-9 of the range: {moved}")
        assert worst <= bound


def test_determinism_and_shards(P):
    """The same call twice, and [0, n) against [0, n/2) + [n/2, n) through first_index -- with n above one launch's 2^20 draws per
    table, so the host's own cut is crossed at a third place."""
    lo, hi, pdf = make_tables(2, 257, seed=4)
    n = (1 << 20) + 1000
    a = P.table_draws(lo, hi, pdf, n, seed=9)
    assert P.last_device_times()[2] == 2
    assert np.array_equal(a, P.table_draws(lo, hi, pdf, n, seed=9))
    h = n // 2
    b = np.concatenate([P.table_draws(lo, hi, pdf, h, seed=9), P.table_draws(lo, hi, pdf, n - h, seed=9, first_index=h)], axis=1)
    assert np.array_equal(a, b)
    # ... and the statement agrees on both sides of the cut
    tail = P.table_draws(lo, hi, pdf, 2000, seed=9, first_index=(1 << 20) - 1000, backend="host")
    close_enough(a[:, (1 << 20) - 1000 : (1 << 20) + 1000], tail, lo, hi)
    # a 64-bit first_index: the index's high word is counter word 1
    big = 2**40 + 12345
    close_enough(P.table_draws(lo, hi, pdf, 100, seed=9, first_index=big), P.table_draws(lo, hi, pdf, 100, seed=9, first_index=big, backend="host"), lo, hi)
    assert not np.array_equal(a[:, :100], P.table_draws(lo, hi, pdf, 100, seed=10))


@pytest.mark.parametrize("n_grid,n", [(5, 1000), (257, 1000), (1500, 65)])
def test_truncated_draws(P, n_grid, n):
    lo, hi, pdf, lower = truncation_inputs(n_grid, n, seed=100 + n_grid)
    x, mass, accept = P.table_draws(lo, hi, pdf, n, seed=77, lower=lower)
    hx, hmass, haccept = P.table_draws(lo, hi, pdf, n, seed=77, lower=lower, backend="host")
    bound = residual_bound(n_grid)
    close_enough(x, hx, lo, hi)
    assert accept.dtype == bool and np.array_equal(accept, haccept)
    assert float(np.max(np.abs(mass - hmass))) <= bound
    for t in range(pdf.shape[0]):
        lw = lower[t]
        assert np.all(x[t] >= np.minimum(np.maximum(lw, lo[t]), hi[t])) and np.all(x[t] <= hi[t])
        c_low, tot = ld_cdf(lo[t], hi[t], pdf[t], np.clip(lw, lo[t], hi[t]))
        assert float(np.max(np.abs(mass[t].astype(LD) - (1.0 - c_low / tot)))) <= bound
        free = lw <= lo[t]
        assert np.all(mass[t][free] == 1.0) and np.all(accept[t][free])
        empty = (mass[t] == 0.0) & ~free
        assert empty[1] and not accept[t][1] and np.array_equal(x[t][empty], np.minimum(np.maximum(lw[empty], lo[t]), hi[t]))
        live = ~empty
        u, _ = P.draw_uniforms(77, 0, n, t)
        c, _ = ld_cdf(lo[t], hi[t], pdf[t], x[t][live])
        assert float(np.max(np.abs(c - (c_low[live] + u[live].astype(LD) * (tot - c_low[live]))) / tot)) <= bound
    # without `lower`: mass and accept are 1 when asked for through the C ABI, and a bound at or below lo changes nothing
    x_free = P.table_draws(lo, hi, pdf, n, seed=77)
    x_lo, m_lo, a_lo = P.table_draws(lo, hi, pdf, n, seed=77, lower=lo[:, None] - 1.0)
    assert np.array_equal(x_free, x_lo) and np.all(m_lo == 1.0) and a_lo.all()


def test_argument_refusals_launch_nothing(P):
    """Each host check through the C ABI: GWI_ERR_INVALID, the first offending table named, the output untouched and no launch
    counted."""
    from gwinferno_amd import _native

    lib = _native.load_library()
    lo, hi, pdf = make_tables(3, 5, seed=0)
    P.table_draws(lo, hi, pdf, 4, seed=1)
    assert P.last_device_times()[2] == 1

    def call(lo, hi, pdf, n_grid=5):
        x = np.full((3, 4), -7.0)
        st = lib.gwi_table_draws(-1, 3, n_grid, _native.as_dp(lo), _native.as_dp(hi), _native.as_dp(np.ascontiguousarray(pdf)), 4, 1, 0, None, _native.as_dp(x), None, None)
        assert np.all(x == -7.0) and P.last_device_times() == (0.0, 0.0, 0)
        return st, lib.gwi_table_draws_error().decode()

    st, msg = call(lo, hi, pdf, n_grid=1)
    assert st == -1 and "n_grid" in msg and "table 0" in msg
    st, msg = call(lo, np.array([hi[0], lo[1], hi[2]]), pdf)
    assert st == -1 and msg.startswith("table 1: hi <= lo")
    for bad in (-1.0, np.nan, np.inf):
        q = pdf.copy()
        q[2, 3] = bad
        st, msg = call(lo, hi, q)
        assert st == -1 and msg.startswith("table 2: density entry 3")
    q = pdf.copy()
    q[1] = 0.0
    st, msg = call(lo, hi, q)
    assert st == -1 and msg == "table 1: the total mass is 0"
    assert lib.gwi_table_draws(10_000, 3, 5, _native.as_dp(lo), _native.as_dp(hi), _native.as_dp(pdf), 4, 1, 0, None, _native.as_dp(np.empty((3, 4))), None, None) == -2


def marginal_check(P, name, x_dev, x_host, grid, ppd, mesh_grid, mesh_pdf):
    """KS of the device's draws against the posterior-predictive curve of the same model -- the marginal of the same piecewise-linear
    model up to the mesh quadrature.  Where the HOST statement on these inputs is already further than half the bound from that curve,
    the quadrature is what is being measured, and the 2-D mesh marginal of the factor curves is the yardstick instead."""
    n = x_dev.size
    bound = KS_POINT / np.sqrt(n)
    d_host = ks_distance(x_host, curve_cdf01(grid, ppd, x_host))
    if d_host <= 0.5 * bound:
        d, against = ks_distance(x_dev, curve_cdf01(grid, ppd, x_dev)), "the posterior-predictive curve"
    else:
        d, against = ks_distance(x_dev, curve_cdf01(mesh_grid, mesh_pdf, x_dev)), "the mesh marginal of the factor curves"
    print(f"{name}: D = {d:.5f} against {against} (statement against the posterior-predictive curve: {d_host:.5f}; bound {bound:.5f}, n = {n})")
    assert d <= bound, (name, d, bound)


def test_powerlaw_peak_end_to_end(P):
    """Config 2's mass model at one point: 1e5 binaries; m1 against `mpdfs` and q against `qpdfs` of calculate_powerlaw_peak_mass_ppds."""
    from gwinferno_amd import postprocess

    lam = dict(alpha=-2.3, beta=1.1, mu_peak=34.0, sig_peak=4.0, lamb=0.08)
    mmin, mmax, n = 5.0, 100.0, 100_000
    curves = P.powerlaw_peak_factor_curves(**lam, mmin=mmin, mmax=mmax)
    out = P.draw_powerlaw_peak_masses(**lam, mmin=mmin, mmax=mmax, n_draws=n, seed=21, curves=curves)
    host = P.draw_powerlaw_peak_masses(**lam, mmin=mmin, mmax=mmax, n_draws=n, seed=21, curves=curves, backend="host")
    m1, q = out["mass_1"][0], out["mass_ratio"][0]
    assert np.all((m1 >= mmin) & (m1 <= mmax) & (q >= mmin / m1) & (q <= 1.0))
    mpdfs, ms, qpdfs, qs = postprocess.calculate_powerlaw_peak_mass_ppds(**lam, mmin=mmin, mmax=mmax)
    mf, p_m, qf, p_q, _ = mesh_marginals(curves[0], curves[1][0], curves[2], curves[3][0], mmin, refine=2, conditional=True)
    marginal_check(P, "PL+Peak m1", m1, host["mass_1"][0], ms, mpdfs[0], mf, p_m)
    marginal_check(P, "PL+Peak q", q, host["mass_ratio"][0], qs, qpdfs[0], qf, p_q)


def test_bspline_end_to_end(P):
    """BSplinePrimaryBSplineRatio at one coefficient draw: the kept pairs against calculate_bspline_mass_ppds, and n_kept / n against
    the mesh's kept fraction within 5 binomial standard deviations."""
    from gwinferno_amd import postprocess

    rng = np.random.default_rng(5)
    m_cs, q_cs, nsp = 0.5 * rng.normal(size=14), 0.5 * rng.normal(size=8), {"m1": 14, "q": 8}
    mmin, mmax, n = 5.0, 100.0, 100_000
    curves = P.bspline_factor_curves(m_cs, q_cs, nsp, mmin, mmax)
    out = P.draw_bspline_masses(m_cs, q_cs, nsp, mmin, mmax, n, seed=22, curves=curves)
    host = P.draw_bspline_masses(m_cs, q_cs, nsp, mmin, mmax, n, seed=22, curves=curves, backend="host")
    keep, hkeep = out["accept"][0], host["accept"][0]
    assert out["n_kept"][0] == keep.sum() and np.mean(keep != hkeep) <= 1e-4
    mpdfs, ms, qpdfs, qs = postprocess.calculate_bspline_mass_ppds(m_cs, q_cs, nsp, mmin, mmax)
    mf, p_m, qf, p_q, kept = mesh_marginals(curves[0], curves[1][0], curves[2], curves[3][0], mmin, refine=2)
    marginal_check(P, "B-spline m1", out["mass_1"][0][keep], host["mass_1"][0][hkeep], ms, mpdfs[0], mf, p_m)
    marginal_check(P, "B-spline q", out["mass_ratio"][0][keep], host["mass_ratio"][0][hkeep], qs, qpdfs[0], qf, p_q)
    print(f"B-spline: kept {keep.sum()} of {n}; the mesh keeps {kept:.5f}")
    assert abs(keep.sum() - n * kept) <= 5.0 * np.sqrt(n * kept * (1.0 - kept)) + 1.0


def test_redshift_and_spin_curves_end_to_end(P):
    """draw_powerlaw_redshifts on a redshift model's own grid, and a postprocess spin curve straight into draw_from_curves."""
    from gwinferno_amd import models as M
    from gwinferno_amd import postprocess

    rng = np.random.default_rng(1)
    z_model = M.PowerlawRedshiftModel(rng.uniform(0.01, 1.9, (4, 64)), rng.uniform(0.01, 1.9, 512))
    n = 100_000
    z = P.draw_powerlaw_redshifts([2.7], z_model, n, seed=23)["redshift"][0]
    zs = np.asarray(z_model.zs)
    want = np.asarray(z_model.dVdz_) * (1.0 + zs) ** (2.7 - 1.0)
    assert ks_distance(z, curve_cdf01(zs, want, z)) <= KS_POINT / np.sqrt(n)
    apdfs, aa = postprocess.calculate_beta_spin_mag([2.0, 1.5], [4.0, 3.0])
    a = P.draw_from_curves(aa, apdfs, n, seed=24)
    for k in range(2):
        assert ks_distance(a[k], curve_cdf01(aa, apdfs[k], a[k])) <= KS_POINT / np.sqrt(n)
