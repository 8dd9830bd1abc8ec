"""TEST INFRASTRUCTURE shared by tests/test_pit_cpu.py and tests/test_gpu_point_pits.py: the grids, the exact un-gridded PIT and the
DERIVED error bounds of the per-event calibration tests (include/gwi_engine.h: gwi_point_pits).  The catalog, the grids'
construction, the masks and the three hyper-parameter points are tests/cdf_util.py's; the bound of a normalised bin is
tests/hist_util.py's."""
from fractions import Fraction

import cdf_util as CU
import hist_util as HU
import numpy as np

N_GRID = (1,) + CU.N_GRID  # one grid point (the walk has a single step), a handful, and the cap (every thread of the workgroup owns one)
U = CU.U


def exact_pit(lw, mask, x, lw_inj, inj_mask, x_inj):
    """The un-gridded PIT of ONE event and quantity as a Fraction: ``sum_i (w_i / S) F_det(x_i)`` with ``F_det(x) = (sum of u_j over
    the injections with y_j <= x) / (sum of u_j)``, in exact integer arithmetic on the statement's own weights ``w`` and ``u``
    (gwinferno_amd/draws.py: draw_weights): no grid, no bins, no rounding."""
    from gwinferno_amd.draws import _exact_integers, draw_weights

    w, _ = _exact_integers(draw_weights(lw, mask))  # (the common power of two cancels in the quotient)
    u, _ = _exact_integers(draw_weights(lw_inj, inj_mask))
    order = np.argsort(x_inj, kind="stable")
    prefix = [0]
    for j in order.tolist():
        prefix.append(prefix[-1] + u[j])
    rank = np.searchsorted(np.asarray(x_inj)[order], np.asarray(x), side="right")  # the number of injections with y <= x
    return Fraction(sum(wi * prefix[r] for wi, r in zip(w, rank.tolist())), sum(w) * prefix[-1])


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def statement_rounding(n_live_e, n_live_inj, n_grid):
    """DERIVED, not measured: ``(relative, absolute)`` bounds on the deviation of the STATEMENT's float64 bracket ends from the same
    ends in exact arithmetic on the same weights.  All terms are non-negative.  A normalised bin is a sum of at most n weights over a
    sum of n weights and one division: within (2 n + 1) 2^-53 <= (n + 1) 2^-52 relative.  D is a running sum of at most G bins: G
    2^-53 more.  A product q D carries both plus its own rounding; the walk adds at most G + 1 non-negative terms, (G + 1) 2^-53
    relative.  Together less than ``(n_e + n_inj + 2 G + 8) 2^-52`` relative.  The outside share o = max(0, 1 - F_e[G-1]) is a
    DIFFERENCE: F_e[G-1] <= 1 + tiny moves by (n_e + 1 + G) 2^-52 at most and the subtraction rounds once, so o moves by at most
    ``(n_e + G + 2) 2^-52`` ABSOLUTE, and it enters either end with a factor of at most 1."""
    return (n_live_e + n_live_inj + 2 * n_grid + 8) * U, (n_live_e + n_grid + 2) * U


def device_tolerance(pit_ref, f_last_ref, d_last_ref, n_live_e, n_live_inj, n_grid):
    """DERIVED, not measured: the bound ``(tol_lo, tol_hi)`` on ``|device - statement|`` of one event and column, from the statement's
    own bracket ``pit_ref = (lo, hi)``, its ``F_e[G-1]`` and ``D[G-1]``.  All terms are non-negative.

    * q: every normalised bin of the device is within ``hist_util.bound(n_live_e) = (n_live_e + 8) 2^-52`` relative of the statement's.
    * D: every entry of the device's detected CDF is within ``cdf_util.f_rel_bound(n_live_inj, G) = (n_live_inj + 8 + G) 2^-52``
      relative of the statement's.
    * the walk: one rounding per product and at most G + 1 additions of non-negative terms, (G + 2) 2^-53 relative on either side,
      ``(G + 2) 2^-52`` together.
      So every term q D, and with it the sum of the terms, is within r = 1.01 (the three added; 1.01 covers their products, each
      below 1e-12) relative of the statement's.
    * o = max(0, 1 - F_e[G-1]) is a difference, so it has no relative bound: F_e[G-1] of the device is within
      ``cdf_util.f_rel_bound(n_live_e, G)`` relative of the statement's (cdf_util), the subtraction rounds once on either side (o <= 1),
      and max(0, .) moves nothing further: ``|o_dev - o_ref| <= f_rel_bound(n_live_e, G) F_ref[G-1] + 2^-52`` ABSOLUTE.  o enters pit_hi
      with the factor 1 and pit_lo with D[G-1] (whose own relative error is in r, applied to the whole of pit_lo).

    ``tol_lo = r lo_ref + d_o (1 + r) D_ref[G-1]`` and ``tol_hi = r hi_ref + d_o``."""
    r = 1.01 * (HU.bound(n_live_e) + CU.f_rel_bound(n_live_inj, n_grid) + (n_grid + 2) * U)
    d_o = CU.f_rel_bound(n_live_e, n_grid) * f_last_ref + U
    return r * pit_ref[0] + d_o * (1.0 + r) * d_last_ref, r * pit_ref[1] + d_o


def statement_point(lw_pe, lw_inj, pe_mask, inj_mask, pe_codes, inj_codes, n_grid):
    """The statement of one point with what the bounds need of it: ``(pit, cdf_det, dead, tol (n_ev, n_cols, 2))``; the tolerance of a
    dead event is NaN (nothing is compared there but the NaN itself)."""
    from gwinferno_amd.draws import point_pits_reference, weighted_histogram_segment

    pit, det, dead = point_pits_reference(lw_pe, lw_inj, pe_mask, inj_mask, pe_codes, inj_codes, n_grid)
    tol = np.full(pit.shape, np.nan)
    if not dead[-1]:
        n_inj = HU.n_live(lw_inj, inj_mask)
        for e in range(lw_pe.shape[0]):
            if dead[e]:
                continue
            mask = None if pe_mask is None else pe_mask[e]
            q, _ = weighted_histogram_segment(lw_pe[e], mask, pe_codes[:, e], n_grid)
            for c in range(q.shape[0]):
                tol[e, c] = device_tolerance(pit[e, c], np.cumsum(q[c])[-1], det[c, -1], HU.n_live(lw_pe[e], mask), n_inj, n_grid)
    return pit, det, dead, tol
