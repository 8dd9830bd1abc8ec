"""TEST INFRASTRUCTURE shared by tests/test_hist_cpu.py and tests/test_gpu_hist.py: the catalog, the hyper-parameter points, the bin
edges, the masks and the derived error bound of the weighted-histogram tests, and the host evaluation (tests/bound_eval.py) the CPU
file vets them with where no device is needed."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COMPS = ("plpeak", "bspline_iid")
TILE = 1024
# the smallest shapes at which the kernels can still go wrong: two tiles per event, the second ragged (476 samples, not a multiple
# of the four samples a lane stages); three tiles of injections, the last ragged (552)
N_EV, N_PE, N_INJ = 3, 1500, 2600
COLUMNS = ("mass_1", "mass_2")  # mass_2 = q m1 is a derived quantity; two columns share one set of weights
N_BINS = (7, 256)               # a handful of bins (several (column, bin) pairs in one wave) and the cap (every thread owns a bin)
CATALOG_SEED = 31
THETA_SEED = {"plpeak": 11, "bspline_iid": 12}  # draw_params(name, default_rng(seed)): the fiducial point
MASK_CASES = ("free", "masked")
DEAD_EVENT = 1                  # the event the "masked" case masks entirely
LOG_FLOOR = -700.0              # vetted: every live weight's lw - M lies above it, so exp() cannot round to 0 on one side only


@functools.lru_cache(maxsize=None)
def catalog():
    from gwinferno_amd.synthetic import make_catalog

    return make_catalog(N_EV, N_PE, N_INJ, seed=CATALOG_SEED)


def params(name, seed=None):
    from gwinferno_amd.compositions import draw_params

    return draw_params(name, np.random.default_rng(THETA_SEED[name] if seed is None else seed))


def points(comp, name, k):
    """``k`` hyper-parameter points ``(k, n_theta)``: the fiducial one first, then draws of the seeds that follow its own."""
    return np.stack([comp.theta(params(name, THETA_SEED[name] + 100 * i)) for i in range(k)])


def composition(name, device=None):
    """The composition on the shared catalog with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle)."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog()
    comp = COMPOSITIONS[name](pe, inj)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def host_log_weights(bound, theta):
    """``(pe (n_ev, n_pe), inj (n_inj,))`` log-weights of the independent host evaluation, sample-independent constants included."""
    from bound_eval import log_weights

    lpe, linj, _ = log_weights(bound, np.asarray(theta, dtype=np.float64), include_consts=True)
    return np.asarray(lpe, dtype=np.float64).reshape(N_EV, N_PE), np.asarray(linj, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def edges(n_bins):
    """Per column ``n_bins + 1`` increasing edges between the 2 % and 98 % quantiles of the column's PE and injection values
    together, so that samples lie outside on both sides: geometric (non-uniform) for mass_1, uniform for mass_2."""
    pe, inj, _ = catalog()
    out = {}
    for name in COLUMNS:
        v = np.concatenate([pe[name].ravel(), inj[name]])
        lo, hi = np.quantile(v, [0.02, 0.98])
        out[name] = np.geomspace(lo, hi, n_bins + 1) if name == "mass_1" else np.linspace(lo, hi, n_bins + 1)
    return out


@functools.lru_cache(maxsize=None)
def bins(n_bins):
    """``(pe_bins (2, n_ev, n_pe), inj_bins (2, n_inj))`` uint16 codes, read-only."""
    from gwinferno_amd.draws import digitize

    pe, inj, _ = catalog()
    e = edges(n_bins)
    pb, ib = np.stack([digitize(pe[c], e[c]) for c in COLUMNS]), np.stack([digitize(inj[c], e[c]) for c in COLUMNS])
    pb.setflags(write=False)
    ib.setflags(write=False)
    return pb, ib


@functools.lru_cache(maxsize=None)
def masks(case):
    """"free": no mask.  "masked": event 0 loses every third sample, DEAD_EVENT all of them, the last event none; the injection set
    keeps its odd indices."""
    if case == "free":
        return None, None
    pe = np.ones((N_EV, N_PE), dtype=np.uint8)
    pe[0, ::3] = 0
    pe[DEAD_EVENT] = 0
    inj = (np.arange(N_INJ) % 2).astype(np.uint8)
    pe.setflags(write=False)
    inj.setflags(write=False)
    return pe, inj


def segments(lw_pe, lw_inj, pe_mask, inj_mask):
    """``(log-weights, mask)`` of every segment, the injection set last."""
    return [(lw_pe[ev], None if pe_mask is None else pe_mask[ev]) for ev in range(lw_pe.shape[0])] + [(lw_inj, inj_mask)]


def n_live(lw, mask):
    from gwinferno_amd.draws import draw_weights

    return int(np.count_nonzero(draw_weights(lw, mask) > 0.0))


def bound(live):
    """DERIVED, not measured.  Every term of a bin sum and of the segment total S is non-negative, so a sum of n terms in any order
    carries a relative error of at most (n - 1) 2^-53; each term is an exp() of the same rounded argument lw - M on both sides,
    right to an ulp on either (two exp roundings, 2 * 2^-52 together), and the quotient adds half an ulp: each bin sum and S are
    within (n_live + 8) 2^-52 relative of their exact values, and a bin of the device is compared with the statement's under
    that one bound (relative to the statement's value)."""
    return (live + 8) * 2.0**-52


# ---- the two extreme points of the GPU file's third test (PL+Peak) ----------------------------------------------------------------
def dead_event_params():
    """A steep primary-mass power law with a narrow, light peak: the heaviest event's samples get p(m1) = 0 (both components
    underflow) -- log-weights of -inf for the whole event -- while the lightest event keeps weight."""
    p = dict(params("plpeak"))
    p.update(alpha=-400.0, mpp=8.0, sigpp=0.5, lam=0.01)
    return p


def wide_spread_params():
    """A mass-ratio exponent of 1500: within one event beta log q spans more than 800, so most weights underflow to 0 next to the
    largest one."""
    p = dict(params("plpeak"))
    p.update(beta=1500.0)
    return p
