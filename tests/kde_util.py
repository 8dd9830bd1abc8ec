"""TEST INFRASTRUCTURE shared by tests/test_kde_cpu.py and tests/test_gpu_kde.py: the grids, bounds and pairs of the weighted kernel
density tests, the derived error bounds and the comparison with the NumPy statement.  The catalog, the compositions, the points and
the masks are those of the weighted-histogram tests (tests/hist_util.py), the columns those of the quantile tests
(tests/quant_util.py)."""
import functools

import hist_util as U
import numpy as np
import quant_util as QU

K = QU.K
CHUNK = 1024                       # gwi_kde.h: kTile, the samples of one evaluation workgroup (3 chunks of injections, the last of 552)
GRID_BLOCK = 256                   # gwi_kde.h: kBlock, the grid points of one evaluation workgroup
N_GRID = (5, 300)                  # fewer grid points than lanes of a wave; a ragged second grid block
Q_COLUMN = 4                       # mass_ratio: the column that reflects in the reflection tests (QU.COLUMNS_8)
Q_BOUNDS = (0.0, 1.0)
PAIRS_1 = ((0, 4),)                # mass_1 - mass_ratio at 7 x 5
PAIRS_2 = ((0, 1), (4, 1))         # mass_1 - mass_2 (strongly correlated) and mass_ratio - mass_2 at 33 x 20: 660 points, three grid blocks
SHAPE_1, SHAPE_2 = (7, 5), (33, 20)
TINY = 1e-300                      # below it only finiteness and sign are held
EPS = 2.0**-52


@functools.lru_cache(maxsize=None)
def grid(n_cols, n_grid):
    """``(n_cols, n_grid)`` grid points, read-only: per column uniform from a tenth of the range below the smallest value of the PE
    and injection samples to a tenth above the largest -- then shuffled (the kernel evaluates at points: no order is needed)."""
    vp, vi = QU.columns(n_cols)
    out = np.empty((n_cols, n_grid))
    rng = np.random.default_rng(17)
    for c in range(n_cols):
        lo, hi = min(vp[c].min(), vi[c].min()), max(vp[c].max(), vi[c].max())
        out[c] = rng.permutation(np.linspace(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n_grid))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reflection_grid():
    """The 1-D grid of the reflection tests for mass_ratio on [0, 1]: points outside on both sides, both bounds exactly, the
    interior -- 41 points."""
    g = np.concatenate([[-0.2, -1e-9, 0.0, 1.0, 1.0 + 1e-9, 1.3], np.linspace(0.01, 0.99, 35)])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def grid2d(pairs, shape):
    """``(gridx (n_pairs, n_gx), gridy (n_pairs, n_gy))`` over the 1 % ... 99 % range of either column of every pair, read-only."""
    vp, vi = QU.columns(8)
    gx, gy = np.empty((len(pairs), shape[0])), np.empty((len(pairs), shape[1]))
    for t, (cx, cy) in enumerate(pairs):
        for out, c, n in ((gx, cx, shape[0]), (gy, cy, shape[1])):
            lo, hi = np.quantile(np.concatenate([vp[c].ravel(), vi[c]]), [0.01, 0.99])
            out[t] = np.linspace(lo, hi, n)
    gx.setflags(write=False)
    gy.setflags(write=False)
    return gx, gy


def moment_eps(live):
    """DERIVED, not measured: the relative error of h^2 (of an entry of H relative to sqrt(Hxx Hyy)) between the device and the
    statement.  The centred second moment and s2 = sum p^2 are sums of n_live terms (for Hxy of mixed sign, hence relative to the
    sum of the absolute terms, which Cauchy-Schwarz bounds by sqrt(Hxx Hyy)): at most (n_live - 1) 2^-53 each in any order on
    either side, 2 n_live 2^-52 together; the error of the mean enters squared; the products, the two divisions, 1 - s2, pow() of
    either side (2 ulp) and f^2 add fewer than 24 roundings."""
    return (2 * live + 24) * EPS


def bound_1d(W, x, grid_c, h, bounds=None):
    """DERIVED, not measured: per grid point the absolute bound on |device - statement| of the 1-D estimate, on the same W.
    rho = norm sum_i p_i e_i with e_i = exp(a_i), a_i = -(g - x_i)^2 / 2h^2 (and the same for the images of a reflection).  Each
    term is off by at most
      * the summation of n non-negative terms in any order, the product p e, the normalisation and its square root:
        (n_live + 8) 2^-52 relative to the whole sum (with reflection the sum has 3 n_live terms);
      * fast_exp's 1.6e-14 + 2.3e-17 |a| / ln 2 on the device (held by tests/test_gpu_math_probe.py) and one ulp of NumPy's exp on the host;
      * the rounding of the argument: d = g - x, d^2 and the product with -1/2h^2 round once each on either side (3 * 2^-52), and
        h^2 differs by moment_eps: exp(a (1 + delta)) = exp(a) (1 + a delta), so |a| (3 * 2^-52 + moment_eps) relative;
      * norm = 1 / (mass sqrt(2 pi h^2)) differs by moment_eps / 2 (within the flat term below).
    The bound is the sum over the terms of p_i e_i times its relative error, times norm: tight where one term dominates (the far
    tails, |a| of several hundred) and where many do."""
    W, x, g = np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(grid_c, dtype=np.float64)
    live = W > 0.0
    n_live = int(np.count_nonzero(live))
    p, xl = W[live] / W.sum(), x[live]
    lo, hi = (np.nan, np.nan) if bounds is None else (np.nan if b is None else float(b) for b in bounds)
    pts, images = [xl], 1
    for b in (lo, hi):
        if b == b:
            pts.append(2.0 * b - xl)
            images += 1
    arg = np.concatenate([-0.5 / h**2 * (g[:, None] - q[None, :]) ** 2 for q in pts], axis=1)
    term = np.exp(arg) * np.tile(p, images)[None, :]
    delta = moment_eps(n_live)
    rel = (images * n_live + 8) * EPS + delta + 1.6e-14 + EPS + np.abs(arg) * (2.3e-17 / np.log(2.0) + 3 * EPS + delta)
    out = np.sum(term * rel, axis=1) / np.sqrt(2.0 * np.pi * h**2)
    out[(g < lo) | (g > hi)] = 0.0  # outside the bounds both sides give exactly 0
    return out


def bound_2d(W, x, y, gx, gy, H):
    """DERIVED, not measured: the absolute bound of the 2-D estimate on the tensor grid, as bound_1d with
    a_i = c0 dx^2 + c1 dx dy + c2 dy^2 (c0 = -Hyy / 2|H|, c1 = Hxy / |H|, c2 = -Hxx / 2|H|).  The three products can cancel, so the
    rounding of the argument is proportional not to |a_i| but to A_i = (Hyy dx^2 + 2 sqrt(Hxx Hyy) |dx dy| + Hxx dy^2) / 2|H| >= the
    sum of the absolute products: 8 roundings on either side (8 * 2^-52).  Every entry of H is off by moment_eps relative to
    sqrt(Hxx Hyy) at most, so |H| = Hxx Hyy - Hxy^2 is off by 4 moment_eps Hxx Hyy, i.e. 4 moment_eps / (1 - r^2) relative with r the
    correlation, and each coefficient by (1 + 4 / (1 - r^2)) moment_eps relative to its counterpart in A_i.  norm = 1 / (mass 2 pi
    sqrt|H|) is off by half the determinant's error (within the flat term)."""
    W, x, y = (np.asarray(v, dtype=np.float64) for v in (W, x, y))
    live = W > 0.0
    n_live = int(np.count_nonzero(live))
    p, xl, yl = W[live] / W.sum(), x[live], y[live]
    hxx, hxy, hyy = (float(v) for v in H)
    det = hxx * hyy - hxy * hxy
    coef = (1.0 + 4.0 * hxx * hyy / det) * moment_eps(n_live)
    dx, dy = np.asarray(gx)[:, None, None] - xl[None, None, :], np.asarray(gy)[None, :, None] - yl[None, None, :]
    arg = (-0.5 * hyy / det) * dx * dx + (hxy / det) * dx * dy + (-0.5 * hxx / det) * dy * dy
    big = (hyy * dx * dx + 2.0 * np.sqrt(hxx * hyy) * np.abs(dx * dy) + hxx * dy * dy) / (2.0 * det)
    rel = (n_live + 8) * EPS + coef + 1.6e-14 + EPS + np.abs(arg) * 2.3e-17 / np.log(2.0) + big * (8 * EPS + coef)
    return np.sum(np.exp(arg) * p[None, None, :] * rel, axis=2) / (2.0 * np.pi * np.sqrt(det))


def compare(got, want, bound, what):
    """One curve or map of the device against the statement's under the derived bound; below TINY only finiteness and sign are held.
    Returns the worst ratio to the bound."""
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound)
    assert got.shape == want.shape == bound.shape, what
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    held = want >= TINY
    ratio = np.abs(got - want)[held] / bound[held]
    assert np.all(np.abs(got - want)[held] <= bound[held]), (what, float(ratio.max()))
    return float(ratio.max()) if ratio.size else 0.0


def check_1d(W, x, grid_c, rule, scale, bounds, got_rho, got_h, got_neff, got_flag, what):
    """One (segment, column) of the device against the statement on the same W: NaN and the flags as the statement has them, h and
    n_eff to 1e-12 relative, the curve under bound_1d.  Returns the worst ratio to the bound (0 without a curve)."""
    from gwinferno_amd.draws import weighted_kde_reference

    rho, h, neff, flag = weighted_kde_reference(W, x, grid_c, rule, scale, bounds)
    assert int(got_flag) == flag, (what, int(got_flag), flag)
    assert abs(got_neff - neff) <= 1e-12 * neff, (what, got_neff, neff)
    if not np.isfinite(h):
        assert np.all(np.isnan(got_rho)) and np.isnan(got_h), what
        return 0.0
    assert abs(got_h - h) <= 1e-12 * h, (what, got_h, h)
    if bounds is not None:  # outside reflecting bounds: exactly 0
        lo, hi = (np.nan if b is None else float(b) for b in bounds)
        outside = (np.asarray(grid_c) < lo) | (np.asarray(grid_c) > hi)
        assert not np.asarray(got_rho)[outside].any() and not rho[outside].any(), what
    return compare(got_rho, rho, bound_1d(W, x, grid_c, h, bounds), what)


def check_2d(W, x, y, gx, gy, rule, scale, got_rho, got_H, got_neff, got_flag, what):
    from gwinferno_amd.draws import weighted_kde2d_reference

    rho, H, neff, flag = weighted_kde2d_reference(W, x, y, gx, gy, rule, scale)
    assert int(got_flag) == flag, (what, int(got_flag), flag)
    assert abs(got_neff - neff) <= 1e-12 * neff, (what, got_neff, neff)
    if not np.all(np.isfinite(H)):
        assert np.all(np.isnan(got_rho)) and np.all(np.isnan(got_H)), what
        return 0.0
    assert np.all(np.abs(got_H - H) <= 1e-12 * np.abs(H)), (what, got_H, H)
    return compare(got_rho, rho, bound_2d(W, x, y, gx, gy, H), what)
