"""TEST INFRASTRUCTURE shared by tests/test_rank_cpu.py and tests/test_gpu_point_ranks.py: the two columns, their ranks and grids, the
exact PIT with < and <= and the DERIVED error bound of the exact per-event calibration tests (include/gwi_engine.h:
gwi_set_rank_columns, gwi_point_pits_exact).  The catalog, the masks and the three hyper-parameter points are
tests/cdf_util.py's, the bound of a segment's total tests/hist_util.py's, the integer arithmetic gwinferno_amd/draws.py's, as
tests/pit_util.py uses it."""
import functools
from fractions import Fraction

import cdf_util as CU
import hist_util as HU
import numpy as np
import pit_util as PU

U = CU.U
COLUMNS = CU.COLUMNS   # mass_ratio: continuous (no value occurs twice); mass_1: rounded to whole solar masses, so that the two sets tie
ROUNDED = 1            # the column of rounded values
TILE = HU.TILE
N_GRID = PU.N_GRID


@functools.lru_cache(maxsize=None)
def columns():
    """``(x_pe (2, n_ev, n_pe), x_inj (2, n_inj))``, read-only: mass_ratio as it is, mass_1 rounded to an integer."""
    pe, inj, _ = CU.catalog()
    x_pe = np.stack([np.asarray(pe[COLUMNS[0]], dtype=np.float64), np.round(np.asarray(pe[COLUMNS[1]], dtype=np.float64))])
    x_inj = np.stack([np.asarray(inj[COLUMNS[0]], dtype=np.float64), np.round(np.asarray(inj[COLUMNS[1]], dtype=np.float64))])
    x_pe.setflags(write=False)
    x_inj.setflags(write=False)
    return x_pe, x_inj


def values():
    """the same as name -> array dictionaries, as the functions of gwinferno_amd/postprocess.py take them"""
    x_pe, x_inj = columns()
    return {n: x_pe[c] for c, n in enumerate(COLUMNS)}, {n: x_inj[c] for c, n in enumerate(COLUMNS)}


@functools.lru_cache(maxsize=None)
def ranks():
    """``(order_inj, rank_lt, rank_le)`` of :func:`gwinferno_amd.draws.rank_codes`, read-only."""
    from gwinferno_amd.draws import rank_codes

    out = rank_codes(*columns())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def distinct_grid():
    """``(2, G)``: for the rounded column ALL its distinct values over both sets (at most 200), so every sample of either set sits on a
    grid point; for the continuous one as many points of cdf_util's range."""
    x_pe, x_inj = columns()
    g = np.unique(np.concatenate([x_pe[ROUNDED].ravel(), x_inj[ROUNDED]]))
    out = np.stack([np.linspace(*CU.GRID_RANGE[COLUMNS[0]], g.size), g])
    out.setflags(write=False)
    return out


def codes(grid):
    """``(pe_codes, inj_codes)`` cumulative uint16 codes of :func:`columns` against ``grid (2, G)``."""
    from gwinferno_amd.draws import cdf_codes

    x_pe, x_inj = columns()
    return np.stack([cdf_codes(x_pe[c], grid[c]) for c in range(2)]), np.stack([cdf_codes(x_inj[c], grid[c]) for c in range(2)])


def exact_pits(lw, mask, x, lw_inj, inj_mask, x_inj):
    """``(pit_lt, pit_le)`` of ONE event and quantity as Fractions: pit_util.exact_pit's integer arithmetic on the statement's own
    weights, with the number of injections below the sample (``<``) and at or below it (``<=``)."""
    from gwinferno_amd.draws import _exact_integers, draw_weights

    w, _ = _exact_integers(draw_weights(lw, mask))  # (the common power of two cancels in the quotient)
    u, _ = _exact_integers(draw_weights(lw_inj, inj_mask))
    order = np.argsort(x_inj, kind="stable")
    prefix = [0]
    for j in order.tolist():
        prefix.append(prefix[-1] + u[j])
    ascending = np.asarray(x_inj)[order]
    den = sum(w) * prefix[-1]
    return tuple(Fraction(sum(wi * prefix[r] for wi, r in zip(w, np.searchsorted(ascending, np.asarray(x), side=side).tolist())), den) for side in ("left", "right"))


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
SCAN_DEPTH = 18    # additions on the longest path of a weight into an in-tile prefix: 3 in the lane, 6 in the wave scan, 3 over the waves
                   # before, 1 for the lane before, 4 along the lane's own ranks, 1 for the tile's offset (a tile's total and an event
                   # tile's partial sum take fewer: 3 + 6 + 3 and 4 + 6 + 3)


def statement_rounding():
    """DERIVED: the relative deviation of the STATEMENT's float64 pit from the same quotient in exact arithmetic on the same weights.
    P and T are exact sums rounded once (2^-53 each), every product rounds once, fsum rounds the exact sum of the rounded products once,
    S is exact and rounded once, and two divisions follow: 7 roundings of 2^-53, less than ``4 * 2^-52``.  All terms are non-negative."""
    return 4.0 * U


def device_tolerance(n_live_e, n_inj_tiles=None, tiles_per_event=None):
    """DERIVED, not measured: the RELATIVE bound on ``|device - statement|`` of one pit: the terms below, in units of 2^-52, added up.  All terms are
    non-negative, so a sum in any order carries one rounding (2^-53) per addition on the longest path, relative to its value.

    * u and w: exp() of the same rounded argument lw - M on both sides, right to an ulp on either: 2 units each where they enter -- w in
      the product, u in P[rank], u in T: 6.
    * P[rank] on the device: SCAN_DEPTH additions inside the tile and n_inj_tiles for the tile's offset, half a unit each; the
      statement's is the exact sum rounded once.  T = P[n_inj] likewise.  Twice (SCAN_DEPTH + n_inj_tiles + 1) / 2.
    * one product per term on either side: 1.
    * the sum over the event's samples: at most SCAN_DEPTH additions inside a tile and tiles_per_event over the tiles on the device,
      one rounding of fsum in the statement: (SCAN_DEPTH + tiles_per_event + 1) / 2.
    * S: hist_util.bound(n_live) = n_live + 8 units cover the device's total against the exact one (n_live terms); the statement's
      fsum adds half a unit.
    * two divisions on either side: 2.

    1.01 covers the products of these terms (each below 1e-12)."""
    n_inj_tiles = -(-CU.N_INJ // TILE) if n_inj_tiles is None else n_inj_tiles
    tiles_per_event = -(-CU.N_PE // TILE) if tiles_per_event is None else tiles_per_event
    units = 6 + (SCAN_DEPTH + n_inj_tiles + 1) + 1 + 0.5 * (SCAN_DEPTH + tiles_per_event + 1) + (n_live_e + 8 + 0.5) + 2
    return 1.01 * units * U


def statement_point(lw_pe, lw_inj, pe_mask, inj_mask):
    """The statement of one point on :func:`ranks` with its bound: ``(pit (n_ev, 2, 2), dead, tol (n_ev, 2, 2))``, the tolerance
    ABSOLUTE (the relative bound times the statement's value; NaN for a dead event: nothing is compared there but the NaN itself)."""
    from gwinferno_amd.draws import point_pits_exact_reference

    pit, dead = point_pits_exact_reference(lw_pe, lw_inj, pe_mask, inj_mask, *ranks())
    tol = np.full(pit.shape, np.nan)
    for e in range(lw_pe.shape[0]):
        if not dead[e] and not dead[-1]:
            tol[e] = device_tolerance(HU.n_live(lw_pe[e], None if pe_mask is None else pe_mask[e])) * pit[e]
    return pit, dead, tol
