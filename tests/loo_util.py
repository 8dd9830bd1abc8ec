"""TEST INFRASTRUCTURE shared by tests/test_loo_cpu.py and tests/test_gpu_loo.py: the catalog, the points, the point weights, the
bins, the columns and the derived error bounds of the point-weight / leave-one-out tests.  The parameter draws, the derived bounds of
one point and the comparisons are those of tests/hist_util.py, tests/quant_util.py and tests/kde_util.py."""
import functools

import hist_util as U
import numpy as np
import quant_util as QU

COMPS = U.COMPS
# the smallest shapes at which a tile boundary, a ragged tail and the segment bookkeeping are all exercised: a full tile of 1 024
# samples plus a ragged one of 476 per event (1 500 is no multiple of the 4 x 256 samples a workgroup stages), three tiles of
# injections with a ragged last one of 452, five points (splits 2 + 3 and 1 x 5)
N_EV, N_PE, N_INJ, K = 3, 1500, 2500, 5
CATALOG_SEED = 37
COLUMNS = ("mass_1", "mass_ratio")
N_BINS = 7
LEVELS = QU.LEVELS
DEAD_EVENT = 1
EPS = 2.0**-52


@functools.lru_cache(maxsize=None)
def catalog():
    """``(pe, inj, total_inj)``.  The redshift model takes its range from the extremes of the PE and injection redshifts, so a catalog
    without one event would be another MODEL whenever that event held an extreme: here every event holds both extremes of the PE set
    (its first two samples), and the model of every leave-one-out catalog is the model of the full one
    (tests/test_loo_cpu.py: test_inputs_of_the_gpu_tests)."""
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(N_EV, N_PE, N_INJ, seed=CATALOG_SEED)
    z = np.array(pe["redshift"], dtype=np.float64)
    z[:, 0], z[:, 1] = z.min(), z.max()
    pe = dict(pe, redshift=z)
    for d in (pe, inj):
        for a in d.values():
            a.setflags(write=False)
    return pe, inj, total


def composition(name, without=None, engine=True):
    """The composition on the catalog -- without event ``without`` when given -- with its engine made on the default GPU."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog()
    if without is not None:
        pe = {k: np.delete(v, without, axis=0) for k, v in pe.items()}
    comp = COMPOSITIONS[name](pe, inj)
    if engine:
        comp.engine()
    return comp


def points(comp, name, k=K):
    return U.points(comp, name, k)


@functools.lru_cache(maxsize=None)
def point_weights():
    """``v (K, n_ev + 1)``, read-only: log-uniform in [2^-20, 1] with an exact 1, an exact 2^-20 and three exact zeros -- one in an
    event's column, one in DEAD_EVENT's, one in the injection set's."""
    v = 2.0 ** np.random.default_rng(41).uniform(-20.0, 0.0, size=(K, N_EV + 1))
    v[0, 0], v[4, 2] = 1.0, 2.0**-20
    v[1, 0] = v[2, DEAD_EVENT] = v[3, N_EV] = 0.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def edges():
    pe, inj, _ = catalog()
    out = {}
    for name in COLUMNS:
        lo, hi = np.quantile(np.concatenate([pe[name].ravel(), inj[name]]), [0.02, 0.98])
        out[name] = np.linspace(lo, hi, N_BINS + 1)
    return out


@functools.lru_cache(maxsize=None)
def bins():
    """``(pe_bins (2, n_ev, n_pe), inj_bins (2, n_inj))`` uint16 codes, read-only; samples lie outside the edges on both sides."""
    from gwinferno_amd.draws import digitize

    pe, inj, _ = catalog()
    e = edges()
    pb, ib = np.stack([digitize(pe[c], e[c]) for c in COLUMNS]), np.stack([digitize(inj[c], e[c]) for c in COLUMNS])
    pb.setflags(write=False)
    ib.setflags(write=False)
    return pb, ib


@functools.lru_cache(maxsize=None)
def columns():
    """``(pe_values (2, n_ev, n_pe), inj_values (2, n_inj))`` of COLUMNS, read-only."""
    pe, inj, _ = catalog()
    vp, vi = np.stack([pe[c] for c in COLUMNS]), np.stack([inj[c] for c in COLUMNS])
    vp.setflags(write=False)
    vi.setflags(write=False)
    return vp, vi


@functools.lru_cache(maxsize=None)
def dead_mask():
    """DEAD_EVENT loses every sample; nothing else is masked."""
    pm, im = np.ones((N_EV, N_PE), dtype=np.uint8), np.ones(N_INJ, dtype=np.uint8)
    pm[DEAD_EVENT] = 0
    pm.setflags(write=False)
    im.setflags(write=False)
    return pm, im


def weight_bound(live, k=K):
    """DERIVED, not measured: quant_util.weight_bound -- (n_live + 8 + k) 2^-52 relative for the sum over k points of w_i / S --
    widened by the one rounding of the product v (w_i / S) of every term: 2^-52 relative (half an ulp on either side)."""
    return QU.weight_bound(live, k) + EPS


def hist_bound(live, k=K):
    """DERIVED, not measured: hist_util.bound -- (n_live + 8) 2^-52 relative for one point's bin -- and, as in weight_bound, k
    additions of non-negative terms onto the running sum that round once on either side (k 2^-52 together) and the one rounding of
    the product with v (2^-52)."""
    return U.bound(live) + (k + 1) * EPS


def vsum_bound(k=K):
    """(k + 2) 2^-52 relative: k additions of non-negative terms on either side, one rounding of v v."""
    return (k + 2) * EPS


def logsumexp(x):
    """log sum exp of a 1-D array by the textbook shift, the sum in extended precision."""
    x = np.asarray(x, dtype=np.longdouble)
    hi = x.max()
    return float(hi + np.log(np.sum(np.exp(x - hi))))
