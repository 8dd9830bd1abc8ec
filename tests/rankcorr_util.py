"""TEST INFRASTRUCTURE shared by tests/test_rankcorr_cpu.py and tests/test_gpu_rankcorr.py: the two tiny catalogs, the columns, the
masks, a stub engine and the DERIVED error bounds of the per-point rank-correlation tests (include/gwi_engine.h:
gwi_set_rankcorr_columns, gwi_point_rank_correlations; gwinferno_amd/csrc/gwi_rankcorr.h).  The hyper-parameter points and
the bound of a segment's total are tests/hist_util.py's, the depth of the in-tile scan tests/rank_util.py's."""
import functools

import hist_util as HU
import numpy as np

TILE = HU.TILE
U = 2.0**-52
COMP = "plpeak"  # PL+Peak x PL-q x PL-z
# the smallest shapes at which the kernels can still go wrong.  "ragged": 5 events x 700 PE samples -- the pooled set of 3 500 has four
# tiles along an order, the last ragged, a tile of the pooled order mixes events, and an event's one sample tile is ragged -- and 2 500
# injections, three tiles, the last ragged.  "full": 1 024 samples per event and exactly 2 048 injections: every tile is full.
SHAPES = {"ragged": (5, 700, 2500), "full": (2, 1024, 2048)}
CATALOG_SEED = {"ragged": 53, "full": 54}
N_COLS = (1, 3, 8)
N_POINTS = 3
DEAD_EVENT = 1  # the event the "masked" case removes
COLUMNS = ("mass_1", "mass_ratio", "chi_eff", "mass_2", "redshift", "chi_p", "a_1", "cos_tilt_1")
SCAN_DEPTH = 18  # rank_util.SCAN_DEPTH: additions on the longest path of a weight into an in-tile prefix, the tile's offset included


@functools.lru_cache(maxsize=None)
def catalog(shape="ragged"):
    from gwinferno_amd.synthetic import make_catalog

    return make_catalog(*SHAPES[shape], seed=CATALOG_SEED[shape])


def composition(shape="ragged", device=None):
    """PL+Peak on the shape's catalog with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle)."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog(shape)
    comp = COMPOSITIONS[COMP](pe, inj)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def points(comp, k=N_POINTS):
    return HU.points(comp, COMP, k)


@functools.lru_cache(maxsize=None)
def columns(n_cols, shape="ragged", ties=False):
    """``(x_pe (n_cols, n_ev, n_pe), x_inj (n_cols, n_inj))``, read-only: the first ``n_cols`` of COLUMNS.  With ``ties`` (three columns
    at least): column 0 rounded to two decimals of its logarithm -- hundreds of members share a value --, column 1 passed through
    float32, column 2 one constant: all members tie."""
    pe, inj, _ = catalog(shape)
    x_pe = np.stack([np.asarray(pe[n], dtype=np.float64) for n in COLUMNS[:n_cols]])
    x_inj = np.stack([np.asarray(inj[n], dtype=np.float64) for n in COLUMNS[:n_cols]])
    if ties:
        x_pe[0], x_inj[0] = np.round(np.log10(x_pe[0]), 2), np.round(np.log10(x_inj[0]), 2)
        x_pe[1], x_inj[1] = x_pe[1].astype(np.float32), x_inj[1].astype(np.float32)
        x_pe[2], x_inj[2] = 0.25, 0.25
    x_pe.setflags(write=False)
    x_inj.setflags(write=False)
    return x_pe, x_inj


def values(n_cols, shape="ragged"):
    """the same as name -> array dictionaries, as the functions of gwinferno_amd/postprocess.py take them"""
    x_pe, x_inj = columns(n_cols, shape)
    return {n: x_pe[c] for c, n in enumerate(COLUMNS[:n_cols])}, {n: x_inj[c] for c, n in enumerate(COLUMNS[:n_cols])}


def codes(x_pe, x_inj):
    """``(codes_obs, codes_det)`` of :func:`gwinferno_amd.draws.rankcorr_codes`: the PE samples pooled, the injections."""
    from gwinferno_amd.draws import rankcorr_codes

    return rankcorr_codes(x_pe.reshape(x_pe.shape[0], -1)), rankcorr_codes(x_inj)


@functools.lru_cache(maxsize=None)
def masks(case, shape="ragged"):
    """"free": no mask.  "masked": event 0 loses every third sample, DEAD_EVENT all of them; the injection set keeps its odd indices.
    "no_inj": the PE samples as in "masked", no injection left."""
    if case == "free":
        return None, None
    n_ev, n_pe, n_inj = SHAPES[shape]
    pe = np.ones((n_ev, n_pe), dtype=np.uint8)
    pe[0, ::3] = 0
    pe[DEAD_EVENT] = 0
    inj = (np.arange(n_inj) % 2).astype(np.uint8) if case == "masked" else np.zeros(n_inj, dtype=np.uint8)
    pe.setflags(write=False)
    inj.setflags(write=False)
    return pe, inj


class StubEngine:
    """What ``catalog_rank_correlation_check(backend="host")`` needs of an engine: the shapes and ``log_weights`` of point ``theta[0]``."""

    def __init__(self, lw_pe, lw_inj):
        self.lw_pe, self.lw_inj = lw_pe, lw_inj
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe[0].shape, lw_inj[0].size, 1

    def log_weights(self, theta):
        k = int(theta[0])
        return self.lw_pe[k].copy(), self.lw_inj[k].copy()


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def sum_depth(n_tiles):
    """Additions on the longest path of one term into a set's sum on the device: 3 along the lane's four samples, 6 in the butterfly
    over the wave, 3 over the four waves, ``n_tiles`` over the set's sample tiles."""
    return 3 + 6 + 3 + n_tiles


def weight_units(n_live, pooled):
    """DERIVED: the relative deviation of a member's weight u between device and statement, in units of 2^-52.  exp() of the same
    rounded argument lw - M on both sides, right to an ulp on either: 2.  The observed set divides by the event's total:
    ``hist_util.bound(n_live) = n_live + 8`` units cover the total of the unchanged draw launches against the exact one, the
    statement's fsum adds half a unit, and the division rounds once on either side: n_live + 9.5 more."""
    return 2.0 + ((n_live + 8 + 0.5) + 1.0 if pooled else 0.0)


def prefix_units(n_live, n_order_tiles, pooled):
    """DERIVED: the relative deviation of one entry of P (and of T = P[n]), in units of 2^-52: that of the weights -- all terms are
    non-negative, so a relative bound of the terms is one of the sum --, SCAN_DEPTH additions inside the tile (offset included) and
    ``n_order_tiles`` in the offsets' chain on the device, half a unit each, and the statement's one rounding of the exact sum."""
    return weight_units(n_live, pooled) + 0.5 * (SCAN_DEPTH + n_order_tiles + 1)


def d_units(n_live, n_order_tiles, pooled):
    """DERIVED: the ABSOLUTE deviation of a centred mid-rank d = ((P[lt] + P[le]) - T) / (2 T), in units of 2^-52.  With p =
    prefix_units: each of P[lt], P[le], T deviates by at most p T 2^-52; the addition rounds 2^-53 of at most 2 T on either side (2 T
    units together), the subtraction 2^-53 of at most T on either side (T): the numerator is within (3 p + 3) T, which the division by
    2 T halves.  The denominator's relative p acts on |d| <= 1/2: p / 2.  The division rounds 2^-53 |d| on either side: 1/2.  Sum:
    2 p + 2."""
    return 2.0 * prefix_units(n_live, n_order_tiles, pooled) + 2.0


def r_tolerance(n_live, n_order_tiles, n_sample_tiles, pooled):
    """DERIVED, not measured: the ABSOLUTE bound on ``|device - statement|`` of one ``R_cd = sum_i u_i d_ci d_di / U``; ``|d| <= 1/2``
    makes every term at most u_i / 4.  With a = weight_units, e = d_units and D = sum_depth(n_sample_tiles), in units of 2^-52:

    * a term (u d_c) d_d: u relative a and two products rounded on either side (2), of at most u / 4; d_c and d_d absolute e each,
      times the other factor, |d_c| + |d_d| <= 1: u ((a + 2) / 4 + e).  Over the members, divided by U: (a + 2) / 4 + e.
    * the sum: D additions on the device, 2^-53 of the sum of the absolute terms (at most U / 4) each, and fsum's one rounding:
      (D + 1) / 8.
    * U: relative a (its terms), (D + 1) / 2 (its own sum on either side) and the division's 1, acting on |R| <= 1/4:
      (a + (D + 1) / 2 + 1) / 4.

    ``n_live`` is the largest number of live samples of one event (it enters through that event's total only); 1.01 covers the
    products of these terms (each below 1e-11)."""
    a, e, depth = weight_units(n_live, pooled), d_units(n_live, n_order_tiles, pooled), sum_depth(n_sample_tiles)
    return 1.01 * U * (0.25 * (a + 2.0) + e + 0.125 * (depth + 1) + 0.25 * (a + 0.5 * (depth + 1) + 1.0))


STATEMENT_MEAN_ROUNDING = 6.0 * U  # m_c of the statement against 1/2: P, T (rounded once each), d, r, the product, fsum, U, the division


def mean_tolerance(n_live, n_order_tiles, n_sample_tiles, pooled):
    """DERIVED: the ABSOLUTE bound on ``|device - statement|`` of one mean rank ``m_c = sum_i u_i r_ci / U``, r = 1/2 + d in [0, 1]:
    a term deviates by u (a + 1 + e + 1) (u, the product, d, the addition 1/2 + d), the sum by (D + 1) / 2 of at most U, and U as in
    :func:`r_tolerance` acting on m <= 1.  The statement itself sits within STATEMENT_MEAN_ROUNDING of 1/2, which exact arithmetic
    gives."""
    a, e, depth = weight_units(n_live, pooled), d_units(n_live, n_order_tiles, pooled), sum_depth(n_sample_tiles)
    return 1.01 * U * ((a + e + 2.0) + 0.5 * (depth + 1) + (a + 0.5 * (depth + 1) + 1.0))


def rho_tolerance(tol_r, r_cd, r_cc, r_dd):
    """The bound on R propagated to rho = R_cd / sqrt(R_cc R_dd), first order: |d rho| <= tol (1 / sqrt(R_cc R_dd) + |rho| / (2 R_cc) +
    |rho| / (2 R_dd)).  Only where tol <= 1e-6 of both variances (checked): the second-order terms are then below 1e-5 of the first,
    which 1.01 covers."""
    assert np.all(tol_r <= 1e-6 * np.minimum(r_cc, r_dd))
    root = np.sqrt(r_cc * r_dd)
    return 1.01 * tol_r * (1.0 / root + 0.5 * np.abs(r_cd) / root * (1.0 / r_cc + 1.0 / r_dd))


def set_tolerances(lw_pe, lw_inj, pe_mask, inj_mask):
    """``(tol_r (2,), tol_mean (2,))`` for one point on the statement's own log-weights: the observed set with the largest live count
    of its events, the detected set."""
    n_ev, n_pe = lw_pe.shape
    n_live = max(HU.n_live(lw_pe[e], None if pe_mask is None else pe_mask[e]) for e in range(n_ev))
    obs = (n_live, -(-(n_ev * n_pe) // TILE), n_ev * -(-n_pe // TILE), True)
    det = (0, -(-lw_inj.size // TILE), -(-lw_inj.size // TILE), False)
    return np.array([r_tolerance(*obs), r_tolerance(*det)]), np.array([mean_tolerance(*obs), mean_tolerance(*det)])
