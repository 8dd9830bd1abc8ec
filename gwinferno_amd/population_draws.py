"""Fair draws from the population model: new sources distributed as ``p(. | Lambda)``, made on the device by ``gwi_table_draws``
(gwinferno_amd/csrc/gwi_popdraw.h) from the 1-D curves the engines already produce on the reference's grids.

A table is an unnormalised density on a uniform grid, read as piecewise linear -- the reading the trapezoid curves of
``postprocess`` make -- and its CDF is inverted exactly, cell by cell.  The reference's ``sample`` / ``icdf`` methods interpolate the
inverse CDF linearly instead; agreement with them is distributional, not numerical, and they are not mirrored here.

``backend="device"`` runs the HIP kernels; ``backend="host"`` is their NumPy statement -- the same Philox counters (the generator is
``spin_priors``'), the same prefix sum in the same shape, the same cell rule and the same inversion formula -- which the kernels are
tested against.  It is not a fall-back: without a device the device backend raises.

A draw is a pure function of (curves, seed, table, draw index): a rerun, or a shard of the draws taken through ``first_index``,
gives the same numbers.
"""
import ctypes as C

import numpy as np

from . import _native
from .spin_priors import _uniform53, philox4x32_10

BACKENDS = ("device", "host")
MAX_GRID = 4096          # a table is staged in LDS (gwi_popdraw.h: kMaxGrid)
COUNTER_TAG = 0x504F5044  # counter word 3 (gwi_popdraw.h: kTag); the chi_p draws of spin_priors use 2 * attempt (+ 1) there
GRID = 800               # points per axis of the reference's mass and spin curves (postprocess.GRID)
_M64 = 2**64 - 1


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, not {backend!r}")


def draw_uniforms(seed, first_index, n_draws, table):
    """The two uniforms ``(u, v)`` of draws ``first_index ... first_index + n_draws`` of table ``table``: one Philox block each."""
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    idx = np.arange(int(n_draws), dtype=np.uint64) + np.uint64(first_index)  # (wraps at 2^64, as the kernel's index does)
    w = philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full(idx.shape, int(table), dtype=np.uint64), np.full(idx.shape, COUNTER_TAG, dtype=np.uint64),
                      seed & 0xFFFFFFFF, seed >> 32)
    return _uniform53(w[0], w[1]), _uniform53(w[2], w[3])


def _tables(lo, hi, pdf):
    """``(lo[T], hi[T], pdf[T, G])`` as contiguous float64 arrays, refused as the entry point refuses them."""
    pdf = np.ascontiguousarray(np.atleast_2d(np.asarray(pdf, dtype=np.float64)))
    if pdf.ndim != 2:
        raise ValueError("pdf must be (n_tables, n_grid) or (n_grid,)")
    n_tables, n_grid = pdf.shape
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (n_tables,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (n_tables,)))
    if n_grid < 2:
        raise ValueError(f"table 0: n_grid = {n_grid} < 2 (a table has at least one cell)")
    if n_grid > MAX_GRID:
        raise ValueError(f"table 0: n_grid = {n_grid} > {MAX_GRID} (a table is staged in LDS)")
    with np.errstate(all="ignore"):
        width = hi - lo
        bad_range = ~(hi > lo) | ~(width < np.inf)
        bad_entry = ~(pdf >= 0.0) | ~(pdf < np.inf)
        dead = ~np.any(0.5 * (pdf[:, :-1] + pdf[:, 1:]) * (width / (n_grid - 1))[:, None] > 0.0, axis=1)
    for t in range(n_tables):  # the first offending table, its checks in the entry point's order
        if bad_range[t]:
            raise ValueError(f"table {t}: hi <= lo (or a bound that is not finite)")
        if bad_entry[t].any():
            raise ValueError(f"table {t}: density entry {int(np.argmax(bad_entry[t]))} is negative or not finite")
        if dead[t]:
            raise ValueError(f"table {t}: the total mass is 0")
    return lo, hi, pdf


def block_scan_prefix(m):
    """Inclusive prefix of ``m`` in the summation shape of ``table_cdf_kernel`` (gwi_draw.h: block_inclusive_scan): chunks of 256
    cells with a carry; inside a chunk four waves of 64 lanes, each scanned by doubling strides (lane l adds lane l - o for
    o = 1, 2, ... 32), then the waves' totals added in wave order.  Only additions, in the kernel's order: the same bits.

    The order matters to the truncated draws: where the restriction keeps a fraction eps of the total mass, the kept part is a
    difference of prefixes and carries a relative error of 2^-52 / eps, which another order of the same sums changes."""
    m = np.asarray(m, dtype=np.float64)
    n_chunks = -(-m.size // 256)
    v = np.zeros(n_chunks * 256)
    v[: m.size] = m
    v = v.reshape(n_chunks, 4, 64)
    for o in (1, 2, 4, 8, 16, 32):
        v = np.concatenate([v[..., :o], v[..., o:] + v[..., :-o]], axis=-1)
    waves = np.cumsum(v[..., 63], axis=1)  # (sequential: 0 + lds[0] + lds[1] ...)
    off = np.concatenate([np.zeros((n_chunks, 1)), waves[:, :3]], axis=1)
    carry = np.concatenate([[0.0], np.cumsum(waves[:, 3])[:-1]])
    return (carry[:, None, None] + (off[:, :, None] + v)).reshape(-1)[: m.size]


def pairwise_prefix(m):
    """Inclusive prefix of ``m`` summed as a balanced tree: another order of the same sums than ``numpy.cumsum``'s (the kernel's
    block scan, :func:`block_scan_prefix`, is a third one).  For the tests that bound what the order of summation can change."""
    m = np.asarray(m, dtype=np.float64)
    if m.size <= 1:
        return m.copy()
    even, odd = m[0::2], m[1::2]
    pairs = pairwise_prefix(even[: odd.size] + odd)  # prefix over the pairs = the prefix at the odd positions
    out = np.empty_like(m)
    out[1::2] = pairs
    out[0::2] = np.concatenate([[0.0], pairs])[: even.size] + even
    return out


def _host_one(lo, hi, p, n_draws, seed, first_index, table, lower, prefix):
    """The kernel's draw, statement by statement (gwi_popdraw.h: draw_one), for one table."""
    n_cell = p.size - 1
    dx = (hi - lo) / n_cell
    m = 0.5 * (p[:-1] + p[1:]) * dx
    cum = prefix(m)
    c_last = cum[-1]
    cells = np.arange(n_cell)
    last_live = int(np.max(np.where(m > 0.0, cells, -1)))
    # next_live[c]: the first cell >= c with mass, n_cell when there is none
    next_live = np.append(np.minimum.accumulate(np.where(m > 0.0, cells, n_cell)[::-1])[::-1], n_cell)
    u, v = draw_uniforms(seed, first_index, n_draws, table)
    n = int(n_draws)
    x, mass, accept = np.empty(n), np.ones(n), np.ones(n, dtype=bool)
    c_min, c_low = np.zeros(n, dtype=np.int64), np.zeros(n)
    bounded, done = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        if lower is not None:
            lw = lower
            nan = np.isnan(lw)
            x[nan], mass[nan], accept[nan] = np.nan, np.nan, False
            bounded = lw > lo
            empty = bounded & (lw > hi)
            i = np.flatnonzero(bounded & ~empty)
            b = lw[i]
            cl = np.minimum(((b - lo) / dx).astype(np.int64), n_cell - 1)
            cl = cl - (b < lo + cl * dx)  # the quotient rounded up
            d = np.minimum(np.maximum(b - (lo + cl * dx), 0.0), dx)
            p0, p1 = p[cl], p[cl + 1]
            s, mc = (p1 - p0) / dx, 0.5 * (p0 + p1) * dx
            part = np.minimum(np.maximum(d * (p0 + 0.5 * s * d), 0.0), mc)  # the trapezoid from x_cl to lower
            below = np.where(cl > 0, cum[np.maximum(cl - 1, 0)], 0.0) + part
            e = (cl > last_live) | ((cl == last_live) & ~(part < mc)) | ~(c_last - below > 0.0)
            empty[i[e]] = True
            keep = i[~e]
            c_min[keep], c_low[keep] = cl[~e], below[~e]
            mass[keep] = np.minimum(np.maximum(1.0 - below[~e] / c_last, 0.0), 1.0)
            x[empty], mass[empty], accept[empty] = np.minimum(np.maximum(lw[empty], lo), hi), 0.0, False
            done = nan | empty
        target = np.where(bounded, c_low + u * (c_last - c_low), u * c_last)
        # a cell in [c_min, n_cell) whose prefix exceeds the target while its predecessor's does not
        a, b = c_min.copy(), np.full(n, n_cell, dtype=np.int64)
        while True:
            todo = a < b
            if not todo.any():
                break
            mid = (a + b) >> 1
            above = cum[np.minimum(mid, n_cell - 1)] > target
            b = np.where(todo & above, mid, b)
            a = np.where(todo & ~above, mid + 1, a)
        c = next_live[a]                          # never a cell without mass
        c = np.where(c >= n_cell, last_live, c)   # past the end: the last cell with mass
        p0, p1 = p[c], p[c + 1]
        s, mc = (p1 - p0) / dx, 0.5 * (p0 + p1) * dx
        r = np.minimum(np.maximum(target - np.where(c > 0, cum[np.maximum(c - 1, 0)], 0.0), 0.0), mc)
        den = p0 + np.sqrt(np.maximum(p0 * p0 + 2.0 * s * r, 0.0))
        xc, xr = lo + c * dx, np.where(c + 1 == n_cell, hi, lo + (c + 1) * dx)
        xx = np.where(den > 0.0, xc + 2.0 * r / den, xc)
        xx = np.minimum(np.maximum(xx, xc), xr)
        if lower is not None:
            xx = np.where(bounded, np.maximum(xx, lower), xx)
        x = np.where(done, x, xx)
        accept = np.where(done, accept, v < mass)
    return x, mass, accept


def _host_table_draws(lo, hi, pdf, n_draws, seed, first_index, lower, prefix=block_scan_prefix):
    n_tables = pdf.shape[0]
    x, mass, accept = np.empty((n_tables, n_draws)), np.empty((n_tables, n_draws)), np.empty((n_tables, n_draws), dtype=bool)
    for t in range(n_tables):
        x[t], mass[t], accept[t] = _host_one(lo[t], hi[t], pdf[t], n_draws, seed, first_index, t, None if lower is None else lower[t], prefix)
    return x, mass, accept


def _device_table_draws(lo, hi, pdf, n_draws, seed, first_index, lower, device):
    lib = _native.load_library()
    if not hasattr(lib, "gwi_table_draws"):
        raise _native.NativeEngineError("this build of the engine has no gwi_table_draws")
    n_tables, n_grid = pdf.shape
    x = np.empty((n_tables, n_draws))
    mass = np.empty((n_tables, n_draws)) if lower is not None else None
    accept = np.empty((n_tables, n_draws), dtype=np.uint8) if lower is not None else None
    st = lib.gwi_table_draws(int(device), n_tables, n_grid, _native.as_dp(lo), _native.as_dp(hi), _native.as_dp(pdf), int(n_draws), int(seed) & _M64, int(first_index) & _M64,
                             _native.as_dp(lower), _native.as_dp(x), _native.as_dp(mass), accept.ctypes.data_as(C.POINTER(C.c_uint8)) if accept is not None else None)
    if st != 0:
        raise _native.NativeEngineError(f"gwi_table_draws: {_native.STATUS_NAMES.get(st, st)} {lib.gwi_table_draws_error().decode()}".rstrip())
    return x, mass, None if accept is None else accept.astype(bool)


def table_draws(lo, hi, pdf, n_draws, seed, first_index=0, lower=None, backend="device", device=_native.DEVICE_CURRENT):
    """``n_draws`` draws from each of the tables ``pdf[t]`` (unnormalised, piecewise linear on the uniform grid ``lo[t] ... hi[t]``;
    a single table may be 1-D, scalar bounds apply to every table).  Returns ``x (n_tables, n_draws)``.

    With ``lower`` (broadcast to ``(n_tables, n_draws)``) draw ``j`` of table ``t`` comes from the density restricted to
    ``x >= lower[t, j]`` and the result is ``(x, mass, accept)``: ``mass`` the probability the restriction keeps and
    ``accept = (v < mass)`` with the second uniform of the draw's Philox block -- thin the draws of another factor by it and the
    pair is an exact sample of the product under the constraint.  ``lower <= lo`` is no bound; where no mass lies at or above
    ``lower``: ``x = min(max(lower, lo), hi)``, ``mass = 0``, ``accept = False``.

    Draw ``j`` depends on ``(table, seed, t, first_index + j)`` only: ``[0, n)`` in one call equals ``[0, n/2)`` and ``[n/2, n)``
    (the second with ``first_index = n/2``) in two."""
    _check_backend(backend)
    n_draws = int(n_draws)
    if n_draws < 0 or int(first_index) < 0:
        raise ValueError("n_draws >= 0 and first_index >= 0 are required")
    lo, hi, pdf = _tables(lo, hi, pdf)
    if lower is not None:
        lower = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (pdf.shape[0], n_draws)))
    if backend == "host":
        x, mass, accept = _host_table_draws(lo, hi, pdf, n_draws, seed, first_index, lower)
    else:
        x, mass, accept = _device_table_draws(lo, hi, pdf, n_draws, seed, first_index, lower, device)
    return x if lower is None else (x, mass, accept)


def last_device_times():
    """DIAGNOSTIC: device time of this thread's last device-backend call -- ``(prefix kernel ms, draw launches ms, launches)``."""
    lib = _native.load_library()
    cdf, drw, n = C.c_double(), C.c_double(), C.c_int32()
    lib.gwi_table_draws_times(C.byref(cdf), C.byref(drw), C.byref(n))
    return cdf.value, drw.value, n.value


def _uniform_grid(grid):
    grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim != 1 or grid.size < 2:
        raise ValueError("grid must be 1-D with at least two points")
    lo, hi = float(grid[0]), float(grid[-1])
    if not hi > lo or np.max(np.abs(grid - np.linspace(lo, hi, grid.size))) > 1e-9 * (hi - lo):
        raise ValueError("grid must be uniform and ascending (numpy.linspace)")
    return lo, hi


def draw_from_curves(grid, pdfs, n_draws, seed, first_index=0, lower=None, backend="device", device=_native.DEVICE_CURRENT):
    """Draws from any ``(K, G)`` curve array on a uniform grid: the 1-D outputs of ``postprocess.calculate_beta_spin_mag``,
    ``calculate_mixture_iso_aligned_spin_tilt`` and ``calculate_bspline_spin_ppds`` go straight in (``pdfs, grid`` as they
    return them).  Returns what :func:`table_draws` returns."""
    lo, hi = _uniform_grid(grid)
    pdfs = np.atleast_2d(np.asarray(pdfs, dtype=np.float64))
    if pdfs.shape[1] != np.size(grid):
        raise ValueError("pdfs must be (K, len(grid))")
    return table_draws(lo, hi, pdfs, n_draws, seed, first_index=first_index, lower=lower, backend=backend, device=device)


# ------------------------------------------------------------------------------------------------------------------------------
# the model-level functions
# ------------------------------------------------------------------------------------------------------------------------------
def factor_seed(seed, factor):
    """The stream of factor ``factor`` (0: primary mass / redshift, 1: mass ratio) of a model-level draw: tables of different
    factors carry the same table numbers, so each factor gets a key of its own."""
    return (int(seed) + int(factor) * 0x9E3779B97F4A7C15) & _M64


def draw_product_masses(ms, m_pdfs, qs, q_pdfs, mmin, n_draws, seed, thin, first_index=0, backend="device", device=_native.DEVICE_CURRENT):
    """``(m1, q)`` from ``p(m1) p(q) 1[q >= mmin / m1]`` given the factor curves ``m_pdfs (K, len(ms))`` and ``q_pdfs (K, len(qs))``.

    m1 comes from its table, q from its table restricted to ``q >= mmin / m1``.  With ``thin`` the joint is the PRODUCT under the
    mask, so the m1 draws are thinned by the probability the mask keeps (``accept``): the accepted pairs are exact samples, with no
    rejection loop.  Without it the conditional ``p(q | m1)`` is normalised for every m1 and every pair is a sample.

    Returns ``mass_1, mass_ratio (K, n)`` and, with ``thin``, ``accept (K, n)``, ``kept_mass (K, n)`` and ``n_kept (K,)``."""
    m1 = draw_from_curves(ms, m_pdfs, n_draws, factor_seed(seed, 0), first_index=first_index, backend=backend, device=device)
    q, kept, accept = draw_from_curves(qs, q_pdfs, n_draws, factor_seed(seed, 1), first_index=first_index, lower=mmin / m1, backend=backend, device=device)
    out = {"mass_1": m1, "mass_ratio": q}
    if thin:
        out.update(accept=accept, kept_mass=kept, n_kept=accept.sum(axis=1))
    return out


def powerlaw_peak_factor_curves(alpha, beta, mu_peak, sig_peak, lamb, mmin, mmax):
    """``(ms, m_pdfs, qs, q_pdfs)``: the ``plpeak_primary_pdf`` curve on the engine, and the ``q^beta`` table, on the grids of
    ``postprocess.calculate_powerlaw_peak_mass_ppds``."""
    from . import models as M
    from .postprocess import _curves

    cols = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (alpha, beta, mu_peak, sig_peak, lamb)]
    ms, qs = np.linspace(mmin, mmax, GRID), np.linspace(mmin / mmax, 1, GRID)
    draws = list(zip(cols[0], cols[2], cols[3], cols[4]))
    m_pdfs = _curves(ms, lambda x, d: M.plpeak_primary_pdf(x, d[0], mmin, mmax, d[1], d[2], d[3]), draws, (-2.0, 30.0, 5.0, 0.1))
    return ms, m_pdfs, qs, qs[None, :] ** cols[1][:, None]


def draw_powerlaw_peak_masses(alpha, beta, mu_peak, sig_peak, lamb, mmin, mmax, n_draws, seed, first_index=0, backend="device", device=_native.DEVICE_CURRENT, curves=None):
    """Binaries from the PL+Peak mass model (``models.plpeak_primary_ratio_pdf``) at the K hyper-parameter points given as
    ``postprocess.calculate_powerlaw_peak_mass_ppds`` takes them: m1 from the ``plpeak_primary_pdf`` curve, q from the ``q^beta``
    table with ``lower = mmin / m1`` -- the conditional is normalised, so nothing is thinned.  ``curves`` replaces
    :func:`powerlaw_peak_factor_curves` (which needs the device)."""
    ms, m_pdfs, qs, q_pdfs = curves if curves is not None else powerlaw_peak_factor_curves(alpha, beta, mu_peak, sig_peak, lamb, mmin, mmax)
    return draw_product_masses(ms, m_pdfs, qs, q_pdfs, mmin, n_draws, seed, False, first_index=first_index, backend=backend, device=device)


def bspline_factor_curves(m_cs, q_cs, nspline_dict, mmin, mmax):
    """``(ms, m_pdfs, qs, q_pdfs)`` of ``models.BSplinePrimaryBSplineRatio`` on the grids of ``postprocess.calculate_bspline_mass_ppds``."""
    from . import models as M
    from .postprocess import _curves

    m_cs, q_cs = np.atleast_2d(np.asarray(m_cs, dtype=np.float64)), np.atleast_2d(np.asarray(q_cs, dtype=np.float64))
    ms, qs = np.linspace(mmin, mmax, GRID), np.linspace(mmin / mmax, 1, GRID)
    out = []
    for grid, model, coefs, n in ((ms, M.BSplineMass(nspline_dict["m1"], ms[None, :], ms, mmin=mmin, mmax=mmax), m_cs, nspline_dict["m1"]),
                                  (qs, M.BSplineRatio(nspline_dict["q"], qs[None, :], qs, qmin=mmin / mmax), q_cs, nspline_dict["q"])):
        out.append(_curves(grid, lambda x, c, model=model: model(c, pe_samples=np.ndim(x) == 2), list(coefs), np.zeros(n)))
    return ms, out[0], qs, out[1]


def draw_bspline_masses(m_cs, q_cs, nspline_dict, mmin, mmax, n_draws, seed, first_index=0, backend="device", device=_native.DEVICE_CURRENT, curves=None):
    """Binaries from ``models.BSplinePrimaryBSplineRatio`` (the product of the two spline densities under the mask
    ``q >= mmin / m1`` of ``postprocess.calculate_bspline_mass_ppds``) at K coefficient draws: m1 thinned by ``accept``, q from the
    truncated table.  ``n_kept`` counts the accepted pairs per point."""
    ms, m_pdfs, qs, q_pdfs = curves if curves is not None else bspline_factor_curves(m_cs, q_cs, nspline_dict, mmin, mmax)
    return draw_product_masses(ms, m_pdfs, qs, q_pdfs, mmin, n_draws, seed, True, first_index=first_index, backend=backend, device=device)


def powerlaw_redshift_curves(lamb, z_model):
    """``(zs, pdfs)``: ``dVc/dz (1 + z)^(lamb - 1)`` on ``z_model.zs``, the power law from the engine (the rate curve of
    ``postprocess.calculate_powerlaw_rate_of_z_ppds``)."""
    from .postprocess import calculate_powerlaw_rate_of_z_ppds

    lamb = np.atleast_1d(np.asarray(lamb, dtype=np.float64))
    rs, zs = calculate_powerlaw_rate_of_z_ppds(lamb, np.ones(lamb.size), z_model)
    return zs, rs * (np.asarray(z_model.dVdz_, dtype=np.float64) / (1.0 + zs))[None, :]


def draw_powerlaw_redshifts(lamb, z_model, n_draws, seed, first_index=0, backend="device", device=_native.DEVICE_CURRENT, curves=None):
    """Redshifts from ``p(z) ~ dVc/dz (1 + z)^(lamb - 1)`` (``models.PowerlawRedshiftModel``) on ``z_model.zs`` at K values of
    ``lamb``.  Returns ``{"redshift": (K, n)}``."""
    zs, pdfs = curves if curves is not None else powerlaw_redshift_curves(lamb, z_model)
    return {"redshift": draw_from_curves(zs, pdfs, n_draws, factor_seed(seed, 0), first_index=first_index, backend=backend, device=device)}
