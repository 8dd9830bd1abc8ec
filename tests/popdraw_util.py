"""Shared by tests/test_population_draws_cpu.py and tests/test_gpu_population_draws.py: the tables, the CDF of a table in
numpy.longdouble, the residual bound and the Kolmogorov-Smirnov distance."""
import numpy as np

LD = np.longdouble
KS_POINT = 2.69  # D <= 2.69 / sqrt(n): the 1e-6 point of the Kolmogorov distribution


def residual_bound(n_grid):
    """|CDF(x) - target| / C_last <= 4 G 2^-52: the sequential-sum error bound for G positive terms, times 4 for the handful of further
    operations.  It holds in probability space, for grids whose points are not large against their width (x itself is rounded to
    2^-53 |x|, which moves the CDF by p(x) |x| 2^-53: every grid here has |x| <= 2 (hi - lo))."""
    return 4.0 * n_grid * 2.0**-52


def special_table(kind, n_grid, rng):
    """One density on ``n_grid`` points; every kind is defined for every ``n_grid >= 2``."""
    g = np.arange(n_grid) / (n_grid - 1.0)
    run = max(1, n_grid // 4)
    if kind == "smooth":
        return 0.2 + rng.uniform(0.0, 1.0, n_grid) * np.exp(-3.0 * g)
    if kind == "flat":  # s = 0 in every cell
        return np.full(n_grid, 0.75)
    if kind == "from_zero":  # p_c = 0 at the start of the first cell
        return g.copy() if n_grid > 2 else np.array([0.0, 1.0])
    if kind == "steep":  # ratio 1e12 end to end
        return np.exp(-np.log(1e12) * g)
    p = 0.1 + rng.uniform(0.0, 1.0, n_grid)
    if kind == "leading_zeros":
        p[:run] = 0.0
    elif kind == "trailing_zeros":
        p[-run:] = 0.0
    elif kind == "interior_zeros":
        if n_grid < 4:
            p[0] = 0.0
        else:
            mid = n_grid // 2
            p[mid - (run + 1) // 2 : mid + run // 2 + 1] = 0.0
    else:
        raise ValueError(kind)
    if not np.any(p[:-1] + p[1:] > 0.0):  # (n_grid = 2 with a zero run: keep one end alive)
        p[0 if kind == "trailing_zeros" else -1] = 1.0
    return p


KINDS = ("smooth", "flat", "from_zero", "steep", "leading_zeros", "trailing_zeros", "interior_zeros")
RANGES = ((0.0, 1.0), (-1.0, 1.0), (3.0, 100.0), (0.03, 1.0), (1e-3, 2.3))  # the reference's grids: spins, tilts, masses, ratios, redshifts


def make_tables(n_tables, n_grid, seed):
    """``(lo, hi, pdf)``: table t is of kind ``KINDS[t % 7]`` on the range ``RANGES[t % 5]``."""
    rng = np.random.default_rng(seed)
    pdf = np.stack([special_table(KINDS[t % len(KINDS)], n_grid, rng) for t in range(n_tables)])
    lo = np.array([RANGES[t % len(RANGES)][0] for t in range(n_tables)])
    hi = np.array([RANGES[t % len(RANGES)][1] for t in range(n_tables)])
    return lo, hi, pdf


def truncation_inputs(n_grid, n, seed):
    """Tables and per-draw lower bounds for the truncated draws: bounds inside the range, some at or below ``lo`` (no bound) and,
    on the tables with trailing zeros, some inside the zero run (no mass at or above them)."""
    lo, hi, pdf = make_tables(len(KINDS), n_grid, seed=seed)
    rng = np.random.default_rng(seed + 1)
    lower = lo[:, None] + (hi - lo)[:, None] * rng.uniform(-0.1, 0.95, (len(KINDS), n))
    lower[:, 0] = lo          # exactly lo: no bound
    lower[:, 1] = hi + 1.0    # above the range: nothing left
    return lo, hi, pdf, lower


def ld_prefix(lo, hi, p):
    """``(dx, C)`` in long double: C[c] = the mass of cells 0 .. c - 1 (C[0] = 0, C[-1] = the total)."""
    p = np.asarray(p, dtype=LD)
    dx = (LD(hi) - LD(lo)) / LD(p.size - 1)
    return dx, np.concatenate([[LD(0)], np.cumsum(LD(0.5) * (p[:-1] + p[1:]) * dx)])


def ld_cdf(lo, hi, p, x):
    """The unnormalised CDF of the piecewise-linear table at ``x`` (inside [lo, hi]) in long double, and the total."""
    p = np.asarray(p, dtype=LD)
    dx, cum = ld_prefix(lo, hi, p)
    x = np.asarray(x, dtype=LD)
    c = np.clip(np.floor((x - LD(lo)) / dx).astype(np.int64), 0, p.size - 2)
    d = x - (LD(lo) + c * dx)
    s = (p[c + 1] - p[c]) / dx
    return cum[c] + d * (p[c] + LD(0.5) * s * d), cum[-1]


def ks_distance(x, cdf01):
    """Kolmogorov-Smirnov distance of the sample ``x`` from the distribution with normalised CDF values ``cdf01`` AT the sample."""
    f = np.sort(np.asarray(cdf01, dtype=np.float64))
    n = f.size
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - f), np.max(f - (i - 1) / n)))


def ks_against_table(lo, hi, p, x):
    c, tot = ld_cdf(lo, hi, p, x)
    return ks_distance(x, c / tot)


def curve_cdf01(grid, pdf, x):
    """Normalised CDF at ``x`` of a tabulated curve (piecewise linear, like every table here)."""
    c, tot = ld_cdf(grid[0], grid[-1], pdf, np.clip(x, grid[0], grid[-1]))
    return (c / tot).astype(np.float64)


def mesh_marginals(ms, m_pdf, qs, q_pdf, mmin, refine=8, conditional=False):
    """Brute force: the product ``p(m) p(q) 1[q >= mmin / m]`` of two piecewise-linear curves on a mesh ``refine`` times finer than
    the curves' grids, integrated along each axis with the trapezoid rule.  Returns ``(mf, p_m, qf, p_q, kept)``: the marginal
    curves on the fine grids and the fraction of the unmasked product's mass the mask keeps.  ``conditional``: every row of the
    masked q factor is normalised first -- the joint p(m) p(q | m) of a model whose conditional is normalised."""
    mf = np.linspace(ms[0], ms[-1], (len(ms) - 1) * refine + 1)
    qf = np.linspace(qs[0], qs[-1], (len(qs) - 1) * refine + 1)
    pm, pq = np.interp(mf, ms, m_pdf), np.interp(qf, qs, q_pdf)
    rows = pq[None, :] * (qf[None, :] >= mmin / mf[:, None])
    if conditional:
        norm = np.trapezoid(rows, qf, axis=1)[:, None]
        rows = np.divide(rows, norm, out=np.zeros_like(rows), where=norm > 0.0)  # (m = mmin: only q = 1 is left, a null set)
    joint = pm[:, None] * rows
    p_m, p_q = np.trapezoid(joint, qf, axis=1), np.trapezoid(joint, mf, axis=0)
    return mf, p_m, qf, p_q, float(np.trapezoid(p_m, mf) / (np.trapezoid(pm, mf) * np.trapezoid(pq, qf)))
