"""TEST INFRASTRUCTURE shared by tests/test_cdf_cpu.py and tests/test_gpu_point_cdfs.py: the tiny catalog, the grids, the masks and
the DERIVED error bounds of the per-point CDF tests (include/gwi_engine.h: gwi_point_cdfs).  The hyper-parameter points,
the host evaluation and the bound of a normalised bin are tests/hist_util.py's."""
import functools

import hist_util as HU
import numpy as np

# the smallest shapes at which the kernels can still go wrong: three events (one to mask, two live), two tiles per event with the
# second ragged (476 samples), three tiles of injections with the last ragged (452), two columns, a handful of grid points and the
# cap (every thread of the workgroup owns one)
N_EV, N_PE, N_INJ = HU.N_EV, HU.N_PE, 2500
COLUMNS = ("mass_ratio", "mass_1")
GRID_RANGE = {"mass_ratio": (0.45, 0.90), "mass_1": (9.5, 14.5)}
N_GRID = (5, 256)
N_POINTS = 3
CATALOG_SEED = 37
DEAD_EVENT = 1
U = 2.0**-52


@functools.lru_cache(maxsize=None)
def catalog():
    from gwinferno_amd.synthetic import make_catalog

    return make_catalog(N_EV, N_PE, N_INJ, seed=CATALOG_SEED)


def composition(device=None):
    """PL+Peak on the shared catalog with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle)."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog()
    comp = COMPOSITIONS["plpeak"](pe, inj)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def points(comp, k=N_POINTS):
    return HU.points(comp, "plpeak", k)


def values():
    pe, inj, _ = catalog()
    return {c: pe[c] for c in COLUMNS}, {c: inj[c] for c in COLUMNS}


@functools.lru_cache(maxsize=None)
def grid(n_grid):
    """``(2, n_grid)`` strictly increasing points, ONE grid per column for the whole catalog as in use.  mass_ratio (uniform): every
    event's samples spread over the whole range, so every F lies strictly between 0 and 1 and all four slots are finite.  mass_1
    (geometric): the grid covers part of the lightest event only; the two heavy events have no sample at or below any grid point, their
    F is exactly 0 and log_all_below is -inf throughout -- on both sides, since a bin sum is 0 exactly when no live sample has the code.
    No F of a live segment comes near 1 (vetted in tests/test_cdf_cpu.py): log1p(-F) is ill-conditioned there, and which of -inf and
    -36 comes out is then decided by the last bit of F."""
    g = np.stack([np.linspace(*GRID_RANGE[name], n_grid) if name == "mass_ratio" else np.geomspace(*GRID_RANGE[name], n_grid) for name in COLUMNS])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def codes(n_grid):
    """``(pe_codes (2, n_ev, n_pe), inj_codes (2, n_inj))`` cumulative uint16 codes, read-only."""
    from gwinferno_amd.draws import cdf_codes

    pe, inj, _ = catalog()
    g = grid(n_grid)
    pc, ic = np.stack([cdf_codes(pe[c], g[i]) for i, c in enumerate(COLUMNS)]), np.stack([cdf_codes(inj[c], g[i]) for i, c in enumerate(COLUMNS)])
    pc.setflags(write=False)
    ic.setflags(write=False)
    return pc, ic


@functools.lru_cache(maxsize=None)
def masks(case):
    """"free": no mask.  "masked": event 0 loses every third sample, DEAD_EVENT all of them, the last event none; the injection set
    keeps its odd indices.  "no_inj": the PE mask of "masked" and an injection mask that removes everything."""
    if case == "free":
        return None, None
    pe = np.ones((N_EV, N_PE), dtype=np.uint8)
    pe[0, ::3] = 0
    pe[DEAD_EVENT] = 0
    inj = (np.arange(N_INJ) % 2).astype(np.uint8) if case == "masked" else np.zeros(N_INJ, dtype=np.uint8)
    pe.setflags(write=False)
    inj.setflags(write=False)
    return pe, inj


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def f_rel_bound(live, n_grid):
    """DERIVED, not measured: the relative deviation of a device F from the statement's.  Every normalised bin h of the device is
    within ``hist_util.bound(n_live) = (n_live + 8) 2^-52`` relative of the statement's (tests/hist_util.py: all terms are
    non-negative).  F is a running sum of at most G non-negative bins: on either side its G - 1 additions add at most (G - 1) 2^-53
    relative, together less than G 2^-52.  So ``|F_dev - F_ref| <= (n_live + 8 + G) 2^-52 F_ref``."""
    return HU.bound(live) + n_grid * U


LOG_ULPS = 2.0  # log and log1p: the HIP math library documents 1 ulp for either in double precision; the host's libm stays within 1 ulp too


def log_sum_bounds(f_ref, lives, n_grid):
    """DERIVED bounds ``(tol_below, tol_above)``, each ``(n_cols, n_grid)``, on the absolute deviation of slots 2 and 3 from the
    statement, from the statement's own event CDFs ``f_ref (n_live_events, n_cols, n_grid)`` and the events' live-sample counts
    ``lives``.  Per event, with r the relative bound on F (:func:`f_rel_bound`):

    * ``log F``: the argument moves by at most r F, so the logarithm by ``-log1p(-r)`` <= 1.01 r; the two evaluations add LOG_ULPS ulps
      of ``|log F|``.
    * ``log1p(-F)``: the argument 1 - F moves by at most r F, so the value by ``-log1p(-r F / (1 - F))``, which is <= 1.01 r F / (1 - F)
      while r F / (1 - F) <= 0.01 and UNBOUNDED otherwise (inf here: the grid of the tests is vetted to keep every F of a live event
      away from 1, so the bound is finite everywhere they compare); plus LOG_ULPS ulps of ``|log1p(-F)|``.
    * The sum over n live events in event order adds, on either side, at most (n - 1) 2^-53 of the sum of the absolute terms.

    Where the statement's F is 0 its term is -inf and so is the device's (a bin sum of the statement is 0 exactly when no live sample
    has that code: hist_util): the bound is 0 there and the comparison is of the infinities themselves."""
    f = np.asarray(f_ref, dtype=np.float64)
    n = f.shape[0]
    below, above = np.zeros(f.shape[1:]), np.zeros(f.shape[1:])
    abs_below, abs_above = np.zeros(f.shape[1:]), np.zeros(f.shape[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        for fe, live in zip(f, lives):
            r = f_rel_bound(live, n_grid)
            lb, la = np.abs(np.log(fe)), np.abs(np.log1p(-np.minimum(fe, 1.0)))
            below += np.where(fe > 0.0, 1.01 * r + LOG_ULPS * U * lb, 0.0)
            move = r * fe / (1.0 - fe)
            above += np.where(move <= 0.01, 1.01 * move + LOG_ULPS * U * la, np.inf)
            abs_below += np.where(fe > 0.0, lb, 0.0)
            abs_above += np.where(np.isfinite(la), la, 0.0)
    return below + n * U * abs_below, above + n * U * abs_above


def statement_event_cdfs(lw_pe, pe_mask, pe_codes, n_grid):
    """``(F (n_live_events, n_cols, n_grid), live-sample counts)`` of the live events, from the statement's own histogram."""
    from gwinferno_amd.draws import weighted_histogram_segment

    fs, lives = [], []
    for ev in range(lw_pe.shape[0]):
        mask = None if pe_mask is None else pe_mask[ev]
        h, alive = weighted_histogram_segment(lw_pe[ev], mask, pe_codes[:, ev], n_grid)
        if alive:
            fs.append(np.cumsum(h, axis=-1))
            lives.append(HU.n_live(lw_pe[ev], mask))
    return np.array(fs), lives
