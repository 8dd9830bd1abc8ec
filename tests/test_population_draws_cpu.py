"""CPU: population draws (gwinferno_amd/population_draws.py, the NumPy statement of gwi_table_draws; gwinferno_amd/csrc/gwi_popdraw.h).

The statement is held to the table's own CDF re-evaluated in numpy.longdouble: |CDF(x) - target| / C_last <= 4 G 2^-52 for every
draw (popdraw_util.residual_bound: measured in probability space, since x itself is ill-conditioned where the density vanishes),
to the Kolmogorov-Smirnov bound D <= 2.69 / sqrt(n) at fixed seeds, and -- the truncation and thinning logic of the model-level
functions -- to brute-force 2-D mesh integration of hand-made curves.  The kernels are held to the statement in
tests/test_gpu_population_draws.py; the inputs of that file are vetted here, where no device is needed."""
import os
import re

import numpy as np
import pytest
from popdraw_util import (KINDS, KS_POINT, LD, curve_cdf01, ks_against_table, ks_distance, ld_cdf, make_tables, mesh_marginals, residual_bound, truncation_inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    from gwinferno_amd import population_draws

    return population_draws


def test_stream_known_answers(P):
    """The uniforms are those of spin_priors' generator (one definition) for the same counter and key."""
    from gwinferno_amd import spin_priors as S

    assert P.philox4x32_10 is S.philox4x32_10 and P._uniform53 is S._uniform53
    # Philox4x32-10 known answers (Random123 kat_vectors)
    assert [int(w) for w in S.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in S.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    seed, first, table, n = 0x0123456789ABCDEF, 2**32 - 3, 5, 8  # the index crosses 2^32: its high word is counter word 1
    u, v = P.draw_uniforms(seed, first, n, table)
    for j in range(n):
        idx = first + j
        w = S.philox4x32_10(idx & 0xFFFFFFFF, idx >> 32, table, P.COUNTER_TAG, seed & 0xFFFFFFFF, seed >> 32)
        assert u[j] == float(S._uniform53(w[0], w[1])) and v[j] == float(S._uniform53(w[2], w[3]))
        assert 0.0 <= u[j] < 1.0 and 0.0 <= v[j] < 1.0
    # counter word 3 sets this use apart from the chi_p draws (2 * attempt (+ 1), attempt < 65536) of the same key
    assert P.COUNTER_TAG >= 2 * 65536
    u2, _ = P.draw_uniforms(seed, first, n, table + 1)
    assert not np.any(u2 == u)


@pytest.mark.parametrize("n_grid", [2, 5, 257, 1500])
def test_cdf_residual(P, n_grid):
    n = 4000
    lo, hi, pdf = make_tables(len(KINDS), n_grid, seed=n_grid)
    x = P.table_draws(lo, hi, pdf, n, seed=11, backend="host")
    worst = 0.0
    for t in range(pdf.shape[0]):
        u, _ = P.draw_uniforms(11, 0, n, t)
        assert np.all((x[t] >= lo[t]) & (x[t] <= hi[t]))
        c, tot = ld_cdf(lo[t], hi[t], pdf[t], x[t])
        worst = max(worst, float(np.max(np.abs(c / tot - u.astype(LD)))))
    print(f"G = {n_grid}: largest CDF residual {worst:.3e} (bound {residual_bound(n_grid):.3e})")
    assert worst <= residual_bound(n_grid)


def test_no_cell_without_mass_is_chosen(P):
    """Zero runs: no draw lands strictly inside a run of cells without mass."""
    for n_grid in (5, 257):
        lo, hi, pdf = make_tables(len(KINDS), n_grid, seed=3)
        x = P.table_draws(lo, hi, pdf, 20000, seed=5, backend="host")
        for t in range(pdf.shape[0]):
            dx = (hi[t] - lo[t]) / (n_grid - 1)
            c = np.clip(np.floor((x[t] - lo[t]) / dx).astype(int), 0, n_grid - 2)
            dead = (pdf[t][c] + pdf[t][c + 1]) == 0.0
            on_edge = np.isclose(x[t], lo[t] + c * dx, rtol=0, atol=1e-12 * (hi[t] - lo[t])) | np.isclose(x[t], lo[t] + (c + 1) * dx, rtol=0, atol=1e-12 * (hi[t] - lo[t]))
            assert not np.any(dead & ~on_edge), (n_grid, t)


def test_kolmogorov_smirnov(P):
    n = 100_000
    lo, hi, pdf = make_tables(len(KINDS), 257, seed=1)
    x = P.table_draws(lo, hi, pdf, n, seed=2024, backend="host")
    for t in range(pdf.shape[0]):
        d = ks_against_table(lo[t], hi[t], pdf[t], x[t])
        print(f"table {t} ({KINDS[t]}): D = {d:.5f} (bound {KS_POINT / np.sqrt(n):.5f})")
        assert d <= KS_POINT / np.sqrt(n)


def test_shards_and_reruns(P):
    lo, hi, pdf = make_tables(3, 257, seed=4)
    a = P.table_draws(lo, hi, pdf, 1000, seed=9, backend="host")
    b = np.concatenate([P.table_draws(lo, hi, pdf, 500, seed=9, backend="host"), P.table_draws(lo, hi, pdf, 500, seed=9, first_index=500, backend="host")], axis=1)
    assert np.array_equal(a, b) and np.array_equal(a, P.table_draws(lo, hi, pdf, 1000, seed=9, backend="host"))
    assert not np.array_equal(a, P.table_draws(lo, hi, pdf, 1000, seed=10, backend="host"))


@pytest.mark.parametrize("n_grid", [2, 5, 257, 1500])
def test_truncation(P, n_grid):
    n = 20000
    lo, hi, pdf, lower = truncation_inputs(n_grid, n, seed=100 + n_grid)
    x, mass, accept = P.table_draws(lo, hi, pdf, n, seed=77, lower=lower, backend="host")
    bound = residual_bound(n_grid)
    for t in range(pdf.shape[0]):
        u, v = P.draw_uniforms(77, 0, n, t)
        lw = lower[t]
        assert np.all(x[t] >= np.minimum(np.maximum(lw, lo[t]), hi[t])) and np.all(x[t] <= hi[t])
        c_low, tot = ld_cdf(lo[t], hi[t], pdf[t], np.clip(lw, lo[t], hi[t]))
        kept = 1.0 - c_low / tot
        assert float(np.max(np.abs(mass[t].astype(LD) - kept))) <= bound, (t, float(np.max(np.abs(mass[t].astype(LD) - kept))))
        free = lw <= lo[t]
        assert np.all(mass[t][free] == 1.0) and np.all(accept[t][free])
        # no mass at or above lower: certainly so beyond the upper edge of the last cell with mass (elsewhere the mass bound above decides)
        last_live = int(np.max(np.flatnonzero(pdf[t][:-1] + pdf[t][1:] > 0.0)))
        surely_empty = lw > lo[t] + (last_live + 1 + 1e-9) * (hi[t] - lo[t]) / (n_grid - 1)
        empty = (mass[t] == 0.0) & ~free
        assert surely_empty[1] and np.all(empty[surely_empty]) and not np.any(accept[t][empty])
        assert np.array_equal(x[t][empty], np.minimum(np.maximum(lw[empty], lo[t]), hi[t]))
        live = ~empty
        c, _ = ld_cdf(lo[t], hi[t], pdf[t], x[t][live])
        target = c_low[live] + u[live].astype(LD) * (tot - c_low[live])
        assert float(np.max(np.abs(c - target) / tot)) <= bound, (t, float(np.max(np.abs(c - target) / tot)))
        assert np.array_equal(accept[t], v < mass[t])
        # the accept frequency against the mean mass: 5 binomial standard deviations at this seed
        sd = np.sqrt(np.sum(mass[t] * (1.0 - mass[t])))
        assert abs(accept[t].sum() - mass[t].sum()) <= 5.0 * sd + 1e-9, (t, accept[t].sum(), mass[t].sum(), sd)
    # draws without a bound are the draws with a bound at or below lo
    x_free = P.table_draws(lo, hi, pdf, n, seed=77, backend="host")
    x_lo, m_lo, a_lo = P.table_draws(lo, hi, pdf, n, seed=77, lower=lo[:, None] - 1.0, backend="host")
    assert np.array_equal(x_free, x_lo) and np.all(m_lo == 1.0) and a_lo.all()


def test_truncated_ks(P):
    """Draws under ONE bound per table follow the restricted, renormalised density."""
    n = 100_000
    lo, hi, pdf = make_tables(4, 257, seed=8)
    cut = lo + 0.37 * (hi - lo)
    x, mass, _ = P.table_draws(lo, hi, pdf, n, seed=31, lower=cut[:, None], backend="host")
    for t in range(4):
        c, tot = ld_cdf(lo[t], hi[t], pdf[t], x[t])
        c0, _ = ld_cdf(lo[t], hi[t], pdf[t], cut[t])
        d = ks_distance(x[t], ((c - c0) / (tot - c0)).astype(np.float64))
        assert d <= KS_POINT / np.sqrt(n), (t, d)
        assert abs(mass[t][0] - float(1 - c0 / tot)) <= residual_bound(257)


def test_prefix_order_stays_within_the_device_cap(P):
    """What the GPU test allows between kernel and statement -- |x_dev - x_host| <= 1e-9 (hi - lo) for all but 1 draw in 1e5 per
    table -- bounds what the order of the prefix sum can do: the statement with numpy.cumsum against the statement with a pairwise
    (tree) prefix, on the GPU test's own tables."""
    n = 1000
    for n_grid in (2, 5, 257, 1500):
        lo, hi, pdf = make_tables(17, n_grid, seed=n_grid)
        lo, hi, pdf = P._tables(lo, hi, pdf)
        a = P._host_table_draws(lo, hi, pdf, n, 11, 0, None, prefix=np.cumsum)[0]
        b = P._host_table_draws(lo, hi, pdf, n, 11, 0, None, prefix=P.pairwise_prefix)[0]
        far = np.abs(a - b) > 1e-9 * (hi - lo)[:, None]
        print(f"G = {n_grid}: {int(far.sum())} of {far.size} draws move by more than 1e-9 of the range; largest {float(np.max(np.abs(a - b) / (hi - lo)[:, None])):.2e}")
        assert np.all(far.sum(axis=1) <= max(1, n // 100_000))
    m = np.random.default_rng(0).uniform(size=1001)
    assert np.allclose(P.pairwise_prefix(m), np.cumsum(m), rtol=1e-13, atol=0)


def test_statement_sums_the_prefix_in_the_kernel_shape(P):
    """block_scan_prefix against gwi_draw.h's block_inclusive_scan written out lane by lane, and what the shape is for: on the
    truncated inputs of the GPU test another order of the same sums (numpy.cumsum) moves draws of the steep table by more than
    1e-9 of the range -- where the bound keeps a fraction eps of the mass the kept part is precise to 2^-52 / eps -- while `mass`
    and `accept` do not depend on the order beyond the residual bound."""
    def lane_by_lane(m):
        out, carry = np.empty(m.size), 0.0
        for base in range(0, m.size, 256):
            v = np.zeros(256)
            v[: min(256, m.size - base)] = m[base : base + 256]
            for o in (1, 2, 4, 8, 16, 32):
                t = v.copy()
                for lane in range(256):
                    if lane % 64 >= o:
                        v[lane] = t[lane] + t[lane - o]
            lds = v[63::64]
            for lane in range(min(256, m.size - base)):
                off = 0.0
                for w in range(lane // 64):
                    off += lds[w]
                out[base + lane] = carry + (off + v[lane])
            total = 0.0
            for w in range(4):
                total += lds[w]
            carry += total
        return out

    rng = np.random.default_rng(2)
    for n in (1, 4, 64, 65, 256, 257, 799, 1499):
        m = rng.uniform(size=n) * np.exp(5.0 * rng.normal(size=n))
        assert np.array_equal(P.block_scan_prefix(m), lane_by_lane(m)), n
    moved = 0
    for n_grid, n in ((5, 1000), (257, 1000), (1500, 65)):
        lo, hi, pdf, lower = truncation_inputs(n_grid, n, seed=100 + n_grid)
        lo, hi, pdf = P._tables(lo, hi, pdf)
        a = P._host_table_draws(lo, hi, pdf, n, 77, 0, lower, prefix=P.block_scan_prefix)
        b = P._host_table_draws(lo, hi, pdf, n, 77, 0, lower, prefix=np.cumsum)
        assert np.array_equal(a[0], P.table_draws(lo, hi, pdf, n, seed=77, lower=lower, backend="host")[0])  # the statement's default
        far = np.abs(a[0] - b[0]) > 1e-9 * (hi - lo)[:, None]
        steep = np.arange(pdf.shape[0]) % len(KINDS) == KINDS.index("steep")
        assert not far[~steep].any()
        moved += int(far.sum())
        assert float(np.max(np.abs(a[1] - b[1]))) <= residual_bound(n_grid) and np.array_equal(a[2], b[2])
    assert moved > 0


def test_gpu_truncation_inputs_keep_v_away_from_mass(P):
    """tests/test_gpu_population_draws.py asks for byte-equal `accept`: on its inputs no v lies within 1e-9 of its mass."""
    for n_grid, n in ((5, 1000), (257, 1000), (1500, 65)):
        lo, hi, pdf, lower = truncation_inputs(n_grid, n, seed=100 + n_grid)
        _, mass, _ = P.table_draws(lo, hi, pdf, n, seed=77, lower=lower, backend="host")
        for t in range(pdf.shape[0]):
            _, v = P.draw_uniforms(77, 0, n, t)
            assert np.min(np.abs(v - mass[t])) > 1e-9, (n_grid, t)


def test_refusals(P):
    lo, hi, pdf = make_tables(3, 5, seed=0)
    with pytest.raises(ValueError, match="n_grid"):
        P.table_draws(0.0, 1.0, np.ones((2, 1)), 4, 0, backend="host")
    with pytest.raises(ValueError, match="table 1: hi <= lo"):
        P.table_draws(lo, np.array([hi[0], lo[1], hi[2]]), pdf, 4, 0, backend="host")
    for bad in (-1.0, np.nan, np.inf):
        q = pdf.copy()
        q[2, 3] = bad
        with pytest.raises(ValueError, match="table 2: density entry 3"):
            P.table_draws(lo, hi, q, 4, 0, backend="host")
    q = pdf.copy()
    q[1] = 0.0
    with pytest.raises(ValueError, match="table 1: the total mass is 0"):
        P.table_draws(lo, hi, q, 4, 0, backend="host")
    with pytest.raises(ValueError):
        P.table_draws(lo, hi, pdf, 4, 0, backend="eager")
    with pytest.raises(ValueError, match="uniform"):
        P.draw_from_curves(np.array([0.0, 0.1, 1.0]), np.ones(3), 4, 0, backend="host")


def test_entry_point_refuses_on_the_host():
    """The C ABI's own argument checks run before a device is looked for: each returns GWI_ERR_INVALID with a message that names
    the first offending table, here without any GPU."""
    from gwinferno_amd import _native

    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym in ("gwi_table_draws", "gwi_table_draws_error", "gwi_table_draws_times"):
        assert sym in _native.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym)
    assert len(lib.gwi_table_draws.argtypes) == 13 and lib.gwi_abi_version() == 3
    lo, hi, pdf = make_tables(3, 5, seed=0)

    def call(lo, hi, pdf, n_grid=5):
        x = np.full((3, 4), -7.0)
        st = lib.gwi_table_draws(-1, 3, n_grid, _native.as_dp(lo), _native.as_dp(hi), _native.as_dp(np.ascontiguousarray(pdf)), 4, 1, 0, None, _native.as_dp(x), None, None)
        assert np.all(x == -7.0)
        return st, lib.gwi_table_draws_error().decode()

    assert call(lo, hi, pdf, n_grid=1) == (-1, "table 0: n_grid = 1 < 2 (a table has at least one cell)")
    st, msg = call(lo, np.array([hi[0], lo[1], hi[2]]), pdf)
    assert st == -1 and msg.startswith("table 1: hi <= lo")
    for bad in (-1.0, np.nan, np.inf):
        q = pdf.copy()
        q[2, 3] = bad
        st, msg = call(lo, hi, q)
        assert st == -1 and msg.startswith("table 2: density entry 3"), msg
    q = pdf.copy()
    q[1] = 0.0
    q[2, 0] = -1.0  # the FIRST offending table is named
    st, msg = call(lo, hi, q)
    assert st == -1 and msg == "table 1: the total mass is 0"


# ---- the model-level functions on hand-made curves ---------------------------------------------------------------------------
def hand_made_curves():
    ms, qs = np.linspace(3.0, 60.0, 33), np.linspace(0.05, 1.0, 41)
    m_pdf = ms**-1.5 + 0.02 * np.exp(-0.5 * ((ms - 35.0) / 4.0) ** 2)
    q_pdf = 0.2 + qs**1.3
    return ms, np.stack([m_pdf, m_pdf[::-1].copy()]), qs, np.stack([q_pdf, np.ones_like(qs)])


def test_thinned_product_against_the_mesh(P):
    """draw_bspline_masses' logic (product under the mask q >= mmin / m1, m1 thinned by `accept`): the m1 and q marginals of the
    kept pairs against brute-force 2-D mesh integration of the same piecewise-linear curves, and n_kept / n against the mesh's kept
    fraction within 5 binomial standard deviations."""
    n, mmin = 100_000, 3.0
    ms, m_pdfs, qs, q_pdfs = hand_made_curves()
    out = P.draw_bspline_masses(None, None, None, mmin, 60.0, n, seed=5, backend="host", curves=(ms, m_pdfs, qs, q_pdfs))
    assert set(out) == {"mass_1", "mass_ratio", "accept", "kept_mass", "n_kept"} and out["mass_1"].shape == (2, n) and out["n_kept"].shape == (2,)
    for k in range(2):
        keep = out["accept"][k]
        m1, q = out["mass_1"][k][keep], out["mass_ratio"][k][keep]
        assert np.all(out["mass_ratio"][k] >= np.minimum(mmin / out["mass_1"][k], 1.0))
        mf, p_m, qf, p_q, kept = mesh_marginals(ms, m_pdfs[k], qs, q_pdfs[k], mmin, refine=40)
        d_m, d_q = ks_distance(m1, curve_cdf01(mf, p_m, m1)), ks_distance(q, curve_cdf01(qf, p_q, q))
        print(f"point {k}: kept {keep.sum()} of {n} (mesh {kept:.5f}); D(m1) = {d_m:.5f}, D(q) = {d_q:.5f} (bound {KS_POINT / np.sqrt(keep.sum()):.5f})")
        assert d_m <= KS_POINT / np.sqrt(keep.sum()) and d_q <= KS_POINT / np.sqrt(keep.sum())
        assert abs(keep.sum() - n * kept) <= 5.0 * np.sqrt(n * kept * (1.0 - kept)) + 1.0
        assert out["n_kept"][k] == keep.sum()


def test_normalised_conditional_against_the_mesh(P):
    """draw_powerlaw_peak_masses' logic (m1 from its curve, q from q^beta restricted to q >= mmin / m1 and RENORMALISED, nothing
    thinned) against the mesh: the joint is p(m1) p(q) 1[q >= mmin / m1] / mass(m1)."""
    n, mmin, mmax = 100_000, 5.0, 80.0
    ms, qs = np.linspace(mmin, mmax, 61), np.linspace(mmin / mmax, 1.0, 61)
    lam, alpha, beta = 0.1, -2.5, 1.5
    m_pdf = (1 - lam) * ms**alpha * (alpha + 1) / (mmax ** (alpha + 1) - mmin ** (alpha + 1)) + lam * np.exp(-0.5 * ((ms - 35.0) / 4.0) ** 2) / (4.0 * np.sqrt(2 * np.pi))
    out = P.draw_powerlaw_peak_masses(None, None, None, None, None, mmin, mmax, n, seed=6, backend="host", curves=(ms, m_pdf[None, :], qs, (qs**beta)[None, :]))
    assert set(out) == {"mass_1", "mass_ratio"}
    m1, q = out["mass_1"][0], out["mass_ratio"][0]
    assert np.all(q >= mmin / m1) and np.all(q <= 1.0)
    assert ks_distance(m1, curve_cdf01(ms, m_pdf, m1)) <= KS_POINT / np.sqrt(n)
    refine = 40
    mf, qf = np.linspace(mmin, mmax, 60 * refine + 1), np.linspace(mmin / mmax, 1.0, 60 * refine + 1)
    pm, pq = np.interp(mf, ms, m_pdf), np.interp(qf, qs, qs**beta)
    joint = pq[None, :] * (qf[None, :] >= mmin / mf[:, None])
    joint = pm[:, None] * joint / np.trapezoid(joint, qf, axis=1)[:, None]
    d_q = ks_distance(q, curve_cdf01(qf, np.trapezoid(joint, mf, axis=0), q))
    print(f"D(q) = {d_q:.5f} (bound {KS_POINT / np.sqrt(n):.5f})")
    assert d_q <= KS_POINT / np.sqrt(n)


def test_redshift_draws_on_closed_form_curves(P):
    n = 100_000
    zs = np.linspace(1e-3, 2.3, 1000)
    lamb = np.array([2.7, -1.0])
    pdfs = (zs**2 / (1 + zs) ** 1.5)[None, :] * (1 + zs)[None, :] ** (lamb[:, None] - 1)  # a stand-in for dVc/dz: the curve is what is drawn from
    out = P.draw_powerlaw_redshifts(lamb, None, n, seed=12, backend="host", curves=(zs, pdfs))
    assert set(out) == {"redshift"} and out["redshift"].shape == (2, n)
    for k in range(2):
        z = out["redshift"][k]
        assert z.min() >= zs[0] and z.max() <= zs[-1]
        assert ks_distance(z, curve_cdf01(zs, pdfs[k], z)) <= KS_POINT / np.sqrt(n)
    # the m1 and q streams of one seed differ, and so do the streams of two seeds
    assert P.factor_seed(12, 0) != P.factor_seed(12, 1) and P.factor_seed(2**64 - 1, 1) < 2**64


def test_draw_from_curves_takes_postprocess_outputs(P):
    """(K, G) curves and their grid as the 1-D postprocess functions return them."""
    aa = np.linspace(0, 1, 800)
    apdfs = np.stack([aa * (1 - aa) ** 3, aa**2 * (1 - aa)])
    x = P.draw_from_curves(aa, apdfs, 500, seed=3, backend="host")
    assert x.shape == (2, 500) and x.min() >= 0.0 and x.max() <= 1.0
    assert np.array_equal(x, P.table_draws(0.0, 1.0, apdfs, 500, 3, backend="host"))
    assert np.array_equal(x[1:], P.draw_from_curves(aa, apdfs, 500, seed=3, backend="host")[1:])
