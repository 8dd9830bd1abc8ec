"""TEST INFRASTRUCTURE shared by tests/test_moment_cpu.py and tests/test_gpu_moments.py: the tiny catalog, the columns, the masks and
the DERIVED error bounds of the per-point moment tests (include/gwi_engine.h: gwi_point_moments; gwinferno_amd/csrc/gwi_moment.h;
DESIGN 8j).  The hyper-parameter points and the bound of a segment's total are tests/hist_util.py's."""
import functools

import hist_util as HU
import numpy as np

# the smallest shapes at which the kernels can still go wrong: three events (one to mask, one to mask down to a single sample, one
# thinned), two tiles per event with the second ragged (476 samples), three tiles of injections with the last ragged (452)
N_EV, N_PE, N_INJ = 3, 1500, 2500
TILE = HU.TILE
COMPS = ("plpeak", "bspline_iid")
N_COLS = (1, 3, 8)
N_POINTS = 3
CATALOG_SEED = 41
DEAD_EVENT = 1          # the event the mask removes entirely
SINGLE_EVENT = 2        # the event the mask leaves one sample of ...
SINGLE_SAMPLE = 1277    # ... in its second tile
OFFSET = 1.0e6          # added to the first column: a tightly measured quantity far from zero
U = 2.0**-52
# the offset column comes first, so that every number of columns holds it
COLUMNS = ("mass_1_offset", "mass_ratio", "chi_eff", "mass_2", "redshift", "chi_p", "a_1", "cos_tilt_1")


@functools.lru_cache(maxsize=None)
def catalog():
    from gwinferno_amd.synthetic import make_catalog

    return make_catalog(N_EV, N_PE, N_INJ, seed=CATALOG_SEED)


def composition(name, device=None):
    """The composition on the shared catalog with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle)."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog()
    comp = COMPOSITIONS[name](pe, inj)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def points(comp, name, k=N_POINTS):
    return HU.points(comp, name, k)


@functools.lru_cache(maxsize=None)
def columns(n_cols):
    """``(x_pe (n_cols, n_ev, n_pe), x_inj (n_cols, n_inj))``, read-only: the first ``n_cols`` of COLUMNS, mass_1 offset by 1e6."""
    pe, inj, _ = catalog()

    def one(d, name):
        return np.asarray(d["mass_1"], dtype=np.float64) + OFFSET if name == "mass_1_offset" else np.asarray(d[name], dtype=np.float64)

    x_pe, x_inj = np.stack([one(pe, n) for n in COLUMNS[:n_cols]]), np.stack([one(inj, n) for n in COLUMNS[:n_cols]])
    x_pe.setflags(write=False)
    x_inj.setflags(write=False)
    return x_pe, x_inj


def values(n_cols):
    """the same as name -> array dictionaries, as the functions of gwinferno_amd/postprocess.py take them"""
    x_pe, x_inj = columns(n_cols)
    return {n: x_pe[c] for c, n in enumerate(COLUMNS[:n_cols])}, {n: x_inj[c] for c, n in enumerate(COLUMNS[:n_cols])}


@functools.lru_cache(maxsize=None)
def masks(case):
    """"free": no mask.  "masked": event 0 loses every third sample, DEAD_EVENT all of them, SINGLE_EVENT all but SINGLE_SAMPLE; the
    injection set keeps its odd indices."""
    if case == "free":
        return None, None
    pe = np.ones((N_EV, N_PE), dtype=np.uint8)
    pe[0, ::3] = 0
    pe[DEAD_EVENT] = 0
    pe[SINGLE_EVENT] = 0
    pe[SINGLE_EVENT, SINGLE_SAMPLE] = 1
    inj = (np.arange(N_INJ) % 2).astype(np.uint8)
    pe.setflags(write=False)
    inj.setflags(write=False)
    return pe, inj


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def sum_depth(n_tiles):
    """Additions on the longest path of one term into a segment's sum on the device, the same for both passes: 3 along the lane's four
    samples, 6 in the butterfly over the wave, 3 over the four waves, ``n_tiles`` over the tiles (the first addition of every chain is
    onto 0 and exact)."""
    return 3 + 6 + 3 + n_tiles


def mean_units(n_live, n_tiles):
    """DERIVED, not measured: the bound on ``|device - statement|`` of a mean, in units of 2^-52 of ``sum_i (w_i / S) |x_ci|``.

    * w: exp() of the same rounded argument lw - M on both sides, right to an ulp on either: 2.
    * the product w x rounds once on either side (the device may fuse it into the addition: no rounding): 1.
    * the sum: ``sum_depth`` additions on the device, each 2^-53 of the sum of the absolute terms; the statement's fsum rounds the exact
      sum once: (sum_depth + 1) / 2.
    * S: ``hist_util.bound(n_live) = n_live + 8`` units cover the total of the unchanged draw launches against the exact one; the
      statement's fsum adds half a unit.
    * the division on either side: 1."""
    return 2 + 1 + 0.5 * (sum_depth(n_tiles) + 1) + (n_live + 8 + 0.5) + 1


def cov_units(n_live, n_tiles):
    """DERIVED, not measured: the first-order bound on ``|device - statement|`` of a covariance entry, in units of 2^-52 of ``sum_i (w_i /
    S) |x_ci - m_c| |x_di - m_d|``.

    * w: 2, as for the mean.
    * the two differences x - m round once each on either side, 2^-53 of |x - m|: 2.
    * the two products (w d_c, then times d_d), each rounded on its own on either side: 2.
    * the sum, S and the division as for the mean: (sum_depth + 1) / 2 + (n_live + 8.5) + 1."""
    return 2 + 2 + 2 + 0.5 * (sum_depth(n_tiles) + 1) + (n_live + 8 + 0.5) + 1


def tolerances(w, x, mean, n_tiles):
    """``(tol_mean (C,), tol_cov (C, C))`` ABSOLUTE, for ONE live segment with the statement's weights ``w (n,)``, values ``x (C, n)`` and
    means.  1.01 covers the products of the terms (each below 1e-12).  The covariance is centred on the side's OWN mean: the two means
    differ by at most ``tol_mean``, and each is within ``tol_mean`` of the mean its own weights define, so centring moves entry (c, d)
    by at most ``3 tol_mean_c tol_mean_d`` (``delta_c eps_d + eps_c delta_d + delta_c delta_d``): second order, and the only term
    that is not proportional to the centred scale.  It is added as it stands."""
    w = np.asarray(w, dtype=np.float64)
    share = w / w.sum()
    n_live = int(np.count_nonzero(w > 0.0))
    tol_mean = 1.01 * mean_units(n_live, n_tiles) * U * (share * np.abs(x)).sum(axis=1)
    d = np.abs(x - np.asarray(mean)[:, None])
    scale = np.einsum("i,ci,di->cd", share, d, d)
    return tol_mean, 1.01 * cov_units(n_live, n_tiles) * U * scale + 3.0 * np.outer(tol_mean, tol_mean)


def statement_point(lw_pe, lw_inj, x_pe, x_inj, pe_mask, inj_mask):
    """The statement of one point with its bounds: ``(mean, cov, dead, tol_mean, tol_cov)``; the tolerances are NaN for a dead segment
    (nothing is compared there but the NaN itself)."""
    from gwinferno_amd.draws import draw_weights, point_moments_reference

    mean, cov, dead = point_moments_reference(lw_pe, lw_inj, x_pe, x_inj, pe_mask, inj_mask)
    tol_mean, tol_cov = np.full(mean.shape, np.nan), np.full(cov.shape, np.nan)
    n_ev = lw_pe.shape[0]
    for seg in range(n_ev + 1):
        if dead[seg]:
            continue
        w = draw_weights(lw_pe[seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else draw_weights(lw_inj, inj_mask)
        x = (None if x_pe is None else x_pe[:, seg]) if seg < n_ev else x_inj
        if x is None:  # (a set without columns: NaN on both sides)
            continue
        tol_mean[seg], tol_cov[seg] = tolerances(w, x, mean[seg], -(-w.size // TILE))
    return mean, cov, dead, tol_mean, tol_cov
