"""TEST INFRASTRUCTURE shared by tests/test_tail_cpu.py and tests/test_gpu_tails.py: the three tiny catalogs, their compositions, the
masks, a brute-force restatement and the DERIVED bounds of the per-point tail tests (include/gwi_engine.h: gwi_set_tail_sizes,
gwi_point_tails; gwinferno_amd/csrc/gwi_tail.h).  The hyper-parameter points and the bound of a segment's total are
tests/hist_util.py's, the depth of a sum of weights and the units of a weight tests/rankcorr_util.py's."""
import functools
import math

import hist_util as HU
import numpy as np
import rankcorr_util as RU

TILE = HU.TILE
U = 2.0**-52
COMP = "plpeak"  # PL+Peak x PL-q x PL-z
# the smallest shapes at which the kernels can still go wrong.  "ragged": 5 events x 700 PE samples with 2 500 injections -- every segment's
# last tile is ragged, the injection set spans three tiles.  "full": 1 024 samples per event and exactly 2 048 injections: every tile is
# full.  "long": 5 000 injections for m_inj = 4 096, the sort's full width.
SHAPES = {"ragged": (5, 700, 2500), "full": (2, 1024, 2048), "long": (2, 700, 5000)}
# seeds at which the events' primary masses overlap: one upper mass bound then cuts through every event (cut_mmax)
CATALOG_SEED = {"ragged": 96, "full": 69, "long": 69}
M_PE = (1, 5, 37, 699)
M_INJ = (1, 64, 671, 2499)
M_LONG = 4096
N_FREE_POINTS = 2  # points under the default mass bounds; a third one under cut_mmax
DEAD_EVENT = 1
# the lower mass bound of every composition here: the catalog's injections start at 2 solar masses, so under the default bound of 5 seven
# in ten would be at -inf and no injection tail of 2 499 or 4 096 would have a live sample below it
MMIN = 2.0


@functools.lru_cache(maxsize=None)
def catalog(shape="ragged", ties=False):
    """The seeded catalog; with ``ties`` every sample 2j + 1 is a copy of sample 2j in every array, so their log-weights tie in every bit."""
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(*SHAPES[shape], seed=CATALOG_SEED[shape])
    if ties:
        for d in (pe, inj):
            for key in d:
                d[key] = d[key].copy()
                d[key][..., 1::2] = d[key][..., 0::2]
    return pe, inj, total


@functools.lru_cache(maxsize=None)
def cut_mmax(shape="ragged"):
    """An upper mass bound inside every event's primary-mass samples: above every event's 10 % quantile and below every event's 90 %
    quantile (the seeds were chosen so that there is one), so part of every event and of the injection set lies outside it."""
    pe, inj, _ = catalog(shape)
    lo, hi = np.quantile(pe["mass_1"], 0.1, axis=1).max(), np.quantile(pe["mass_1"], 0.9, axis=1).min()
    assert lo < hi and inj["mass_1"].max() > hi
    return float(0.5 * (lo + hi))


def composition(shape="ragged", device=None, cut=False, ties=False, prior_scale=None):
    """PL+Peak on the shape's catalog with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle).  ``cut``: the
    upper mass bound is cut_mmax (True) or the number given.  ``prior_scale = (pe, inj)``: the priors multiplied by a constant each -- a constant column of the
    prior, which shifts every log-weight of the set."""
    from gwinferno_amd.compositions import COMPOSITIONS

    pe, inj, _ = catalog(shape, ties)
    if prior_scale is not None:
        pe, inj = dict(pe), dict(inj)
        pe["prior"], inj["prior"] = pe["prior"] * prior_scale[0], inj["prior"] * prior_scale[1]
    if cut is True:
        cut = cut_mmax(shape)
    comp = COMPOSITIONS[COMP](pe, inj, mmin=MMIN, mmax=float(cut)) if cut else COMPOSITIONS[COMP](pe, inj, mmin=MMIN)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def points(comp, k=N_FREE_POINTS):
    return HU.points(comp, COMP, k)


@functools.lru_cache(maxsize=None)
def masks(case, shape="ragged"):
    """"free": no mask.  "masked": event 0 loses every third sample, DEAD_EVENT all of them; the injection set keeps its odd indices."""
    if case == "free":
        return None, None
    n_ev, n_pe, n_inj = SHAPES[shape]
    pe = np.ones((n_ev, n_pe), dtype=np.uint8)
    pe[0, ::3] = 0
    pe[DEAD_EVENT] = 0
    inj = (np.arange(n_inj) % 2).astype(np.uint8)
    pe.setflags(write=False)
    inj.setflags(write=False)
    return pe, inj


def keep_first_live(lw, n_keep):
    """A mask of one segment that leaves its first ``n_keep`` finite log-weights."""
    mask = np.zeros(lw.size, dtype=np.uint8)
    mask[np.nonzero(np.isfinite(lw))[0][:n_keep]] = 1
    return mask


def brute_segment(logw, mask, m):
    """ONE segment by a Python loop over the samples, no sort: the m largest live values by repeated removal of the maximum."""
    live = [float(v) for j, v in enumerate(np.asarray(logw, dtype=np.float64).ravel()) if math.isfinite(v) and (mask is None or mask[j])]
    if not live:
        return [-math.inf] * m, (-math.inf, 0.0, math.nan, -math.inf), (0, 0, 0, 1)
    top = max(live)
    rest, tail = list(live), []
    for _ in range(min(m, len(live))):
        v = max(rest)
        rest.remove(v)
        tail.append(v)
    tail = [-math.inf] * (m - len(tail)) + tail[::-1]
    v_star = tail[0]
    below = [v for v in live if v < v_star]
    total = math.fsum(math.exp(v - top) for v in live)
    body = math.fsum(math.exp(v - top) for v in below)
    return tail, (top, total, body, max(below) if below else -math.inf), (len(live), sum(v > v_star for v in live), sum(v == v_star for v in live), 0)


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def body_bound(n_tiles):
    """DERIVED, not measured: the RELATIVE bound on ``|device - statement|`` of ``body``, a sum of non-negative weights exp(l - max) of a
    fixed shape: rankcorr_util.weight_units(0, False) = 2 units of 2^-52 for the two exp() of the same rounded argument, half a unit per
    addition on the longest path of the device's sum -- rankcorr_util.sum_depth(n_tiles): 3 along the lane's four samples, 6 in the
    butterfly, 3 over the waves, n_tiles over the tiles -- and half a unit for the statement's fsum; 1.01 covers the products."""
    return 1.01 * U * (RU.weight_units(0, False) + 0.5 * (RU.sum_depth(n_tiles) + 1))


def total_bound(n_live):
    """DERIVED: the relative bound on S, the total draw_merge_kernel leaves: tests/hist_util.py's ``bound``."""
    return HU.bound(n_live)


def log_sum_bound(rel, log_arg, value):
    """DERIVED: the absolute bound on ``top + log(arg)`` when ``arg`` is within ``rel`` relative on the two sides and ``top`` is equal:
    the logarithm moves by ``rel`` (1.01 covers the second order) and is rounded to an ulp on either side, the addition to half an ulp of
    the result on either side."""
    return 1.01 * rel + 2.0 * U * abs(log_arg) + U * abs(value)


def n_tiles_of(n):
    return -(-n // TILE)
