"""TEST INFRASTRUCTURE shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py: the catalogs, fiducial points and seeds
of the resampling tests, and the host evaluation they are held to (tests/bound_eval.py).  The CPU file vets these inputs -- every
set has live injections and a host n_eff that lies farther than 1e-6 relative from an integer -- where no device is needed."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COMPS = ("plpeak", "bspline_iid")
TILE = 1024
# injection counts for the kernels' edges: a single sample, one below / exactly / one above a tile, several tiles with a ragged
# end, more than 256 tiles (the carry in the merge and the stats chunk)
N_INJ = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 257 * TILE + 3)
N_EV, N_PE = 2, 64
# make_catalog's seed.  With 2 x 64 PE samples the redshift model's range ends at the PE samples' largest z, and masses below
# mmin = 5 carry no weight: of the seeds 100 ... 159 this one leaves the most injections with weight (about a fifth).  The set of
# ONE injection has none under any seed: the reference's redshift normaliser then spans [z, z] and is 0 (parametric.py:114-115).
CATALOG_SEED = 151
THETA_SEED = {"plpeak": 11, "bspline_iid": 12}  # draw_params(name, default_rng(seed)): the fiducial point
NEARBY_SEED = 77                                # the nearby point theta' of the end-to-end test
DRAW_SEED = 20240917                            # the seed of every resampling stream drawn in the tests


@functools.lru_cache(maxsize=None)
def catalog(n_inj):
    from gwinferno_amd.synthetic import make_catalog

    return make_catalog(N_EV, N_PE, n_inj, seed=CATALOG_SEED)


@functools.lru_cache(maxsize=None)
def end_to_end_catalog():
    """The 3 * 1024 + 5 set for the end-to-end test, where a model is built a second time from the resampled set.  The reference's
    redshift model takes its range from the data -- [max(min z_pe, min z_inj), min(max z_pe, max z_inj)], parametric.py:114-115 --
    so the two models are one function only if the PE samples set that range for both injection sets: the PE redshifts are moved
    into [1.0, 1.2], and injections beyond 1.2 are moved onto it (they carry weight there: the range is closed), so that the
    resampled set reaches it too.  The tests assert that it does."""
    pe, inj, total = catalog(3 * TILE + 5)
    pe, inj = dict(pe), dict(inj)
    pe["redshift"] = np.clip(pe["redshift"], 1.0, 1.2)
    inj["redshift"] = np.minimum(inj["redshift"], 1.2)
    return pe, inj, total


def same_redshift_range(pe, inj, new):
    """Whether the redshift model of (pe, new) has the range of the model of (pe, inj), and the PE samples set it."""
    z_pe, z, z_new = pe["redshift"], inj["redshift"], new["redshift"]
    return z_pe.min() >= max(z.min(), z_new.min()) and z_pe.max() <= min(z.max(), z_new.max())


def params(name, seed=None):
    from gwinferno_amd.compositions import draw_params

    return draw_params(name, np.random.default_rng(THETA_SEED[name] if seed is None else seed))


def nearby_params(name):
    """theta': the fiducial point moved by a few per cent of the prior widths of draw_params."""
    p, other = params(name), params(name, NEARBY_SEED)
    return {k: np.asarray(p[k]) + 0.05 * (np.asarray(other[k]) - np.asarray(p[k])) for k in p}


def composition(name, pe, inj, device=None):
    """The composition with its engine made: on ``device`` (None: the default GPU, -2: a host-only handle for the CPU suite)."""
    from gwinferno_amd.compositions import COMPOSITIONS

    comp = COMPOSITIONS[name](pe, inj)
    comp.engine() if device is None else comp.engine(device=device)
    return comp


def host_log_weights(bound, theta):
    """The injection log-weights of the independent host evaluation, sample-independent constants included."""
    from bound_eval import log_weights

    return np.asarray(log_weights(bound, theta, include_consts=True)[1], dtype=np.float64)


def host_sums(lw, mask=None):
    """{log_sum_w, log_sum_w2, n_eff, n_live, N} of the host evaluation, the sums in extended precision."""
    from gwinferno_amd.draws import draw_weights

    w = draw_weights(lw, mask).astype(np.longdouble)
    live = w > 0
    if not live.any():
        return {"log_sum_w": -np.inf, "log_sum_w2": -np.inf, "n_eff": 0.0, "n_live": 0, "N": 0}
    big = np.max(lw[live])
    c, q = np.sum(w), np.sum(w * w)
    n_eff = float(c * c / q)
    return {"log_sum_w": float(big + np.log(c)), "log_sum_w2": float(2 * big + np.log(q)), "n_eff": n_eff, "n_live": int(live.sum()), "N": int(np.floor(n_eff))}


class HostEngine:
    """What catalog.resample_injections(backend="host") needs of an engine: log_weights and n_inj, over the bound model."""

    def __init__(self, bound, n_inj):
        self.bound, self.n_inj = bound, n_inj

    def log_weights(self, theta):
        from bound_eval import log_weights

        lpe, linj, _ = log_weights(self.bound, np.asarray(theta, dtype=np.float64), include_consts=True)
        return np.asarray(lpe), np.asarray(linj)
