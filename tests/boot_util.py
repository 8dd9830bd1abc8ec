"""TEST INFRASTRUCTURE shared by tests/test_boot_cpu.py and tests/test_gpu_point_bootstrap.py: the shapes, a brute-force restatement, a stand-in engine
and the DERIVED bounds of the bootstrap tests (include/gwi_engine.h: gwi_set_bootstrap, gwi_point_bootstrap; gwinferno_amd/csrc/gwi_boot.h;
DESIGN 8n).  The tiny catalogs, compositions, masks and points are tests/tail_util.py's, the bound of a segment's total tests/hist_util.py's."""
import math
import types

import numpy as np
import tail_util as TU

U = TU.U  # 2^-52: one unit; an addition or a product rounds to half a unit
TILE = TU.TILE
SLICES = 8                 # gwi_boot.h: kSlices
SLICE = TILE // SLICES     # ... kSlice: the additions along one slice
SHAPES = ("ragged", "full")  # tail_util.SHAPES: 5 x 700 with 2 500 injections; 2 x 1 024 with 2 048
REPLICATES = (1, 5, 128, 260)  # one word of a group; a ragged group; one full pass of the tile kernel; three passes, the last ragged
SEED = 20261021


def sums_bound(n_tiles):
    """DERIVED, not measured: the RELATIVE bound on ``|device - statement|`` of a replicate's sum A_b = sum_i c_ib w_i, in units of 2^-52:
    ``1024 / 8 + 8 + n_tiles + 2``.  Every term is non-negative, so relative errors of terms and of partial sums do not amplify.  The
    device: w_i = exp() of the same rounded argument lw - M as the statement's, right to an ulp on either side (2 units together); one
    fused multiply-add per sample along a slice of 1024 / 8 = 128 samples, the 8 slices added in order, the segment's n_tiles tiles added
    in order -- 128 + 8 + n_tiles roundings of half a unit each on the longest path.  That is (128 + 8 + n_tiles) / 2 + 2 units for the
    device; the other half of the bound is left to the statement, whose np.sum rounds each product once (half a unit) and adds pairwise
    in blocks of at most 128 with eight running sums (fewer than 16 + 3 + log2(n / 128) + 1 < 30 roundings for n <= 2^20: under 16 units)."""
    return (TILE // SLICES + SLICES + n_tiles + 2) * U


def brute_bound(n):
    """DERIVED: the relative bound between the statement's sum of ``n`` terms and the exact one (math.fsum of exact products would need
    rationals: the loop adds the rounded products with fsum, so one product rounding and one final rounding on that side): n additions
    of non-negative terms and one product each on the statement's side at half a unit, as rankcorr_util's depth bound: (n + 2) units
    cover both sides with room."""
    return (n + 2) * U


def log_bound(rel):
    """DERIVED: what a relative deviation ``rel`` of a positive argument does to its logarithm (1.01 covers the second order), plus the
    logarithm's own rounding on either side relative to 1 (|log| of the ratios met here is below 1)."""
    return 1.01 * rel + 2.0 * U


def brute_counts(seed, first_index, n, reps):
    """Counts by a Python loop over samples and replicates: one scalar Philox block per (sample, group), thirteen comparisons."""
    from gwinferno_amd import draws as D

    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    out = np.empty((n, len(reps)), dtype=np.int64)
    for j in range(n):
        index = first_index + j
        blocks = {}
        for col, b in enumerate(reps):
            g = b // 4
            if g not in blocks:
                blocks[g] = philox_scalar((index & 0xFFFFFFFF, index >> 32, g, D.BOOTSTRAP_TAG), k0, k1)
            out[j, col] = sum(1 for t in D.POISSON1_THRESHOLDS if t <= blocks[g][b % 4])
    return out


def philox_scalar(c, k0, k1):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = c
    m = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def brute_segment(lw, mask, counts):
    """ONE segment by a Python loop: ``(sums (B,), (M, S), dead, C (B,))`` with fsum for every sum."""
    n, n_rep = counts.shape
    keep = [mask is None or bool(mask[j]) for j in range(n)]
    live = [j for j in range(n) if keep[j] and math.isfinite(lw[j])]
    c_b = [sum(int(counts[j, b]) for j in range(n) if keep[j]) for b in range(n_rep)]
    if not live:
        return [math.nan] * n_rep, (-math.inf, 0.0), 1, c_b
    top = max(float(lw[j]) for j in live)
    w = {j: math.exp(float(lw[j]) - top) for j in live}
    return [math.fsum(int(counts[j, b]) * w[j] for j in live) for b in range(n_rep)], (top, math.fsum(w.values())), 0, c_b


class StubEngine:
    """What ``likelihood_bootstrap(backend="host")`` needs of an engine: the shapes, ``log_weights`` and ``evaluate_batch``.  One
    hyper-parameter tilts every log-weight: ``lw(theta) = lw0 + theta[0] g`` with a fixed direction ``g`` per sample; the sites come
    from oracle/numpy_oracle.py's restatement of the reference's reductions."""

    max_batch = 16

    def __init__(self, lw_pe, lw_inj, g_pe, g_inj):
        self.lw_pe, self.lw_inj, self.g_pe, self.g_inj = lw_pe, lw_inj, g_pe, g_inj
        (self.n_ev, self.n_pe), self.n_inj, self.n_theta = lw_pe.shape, lw_inj.size, 1
        self.n_ev_global = self.n_ev

    def log_weights(self, theta):
        t = float(np.ravel(theta)[0])
        return self.lw_pe + t * self.g_pe, self.lw_inj + t * self.g_inj

    def sites(self, theta, total_inj):
        from oracle import numpy_oracle as O

        lw_pe, lw_inj = self.log_weights(theta)
        log_bf, log_neff, var = O.per_event_log_bayes_factors(lw_pe, log=True)
        log_mu, log_neff_inj, var_mu = O.detection_efficiency(lw_inj, total_inj, log=True)
        return dict(log_bf=log_bf, log_neff=log_neff, var=var, log_mu=float(log_mu), log_neff_inj=float(log_neff_inj), var_mu=float(var_mu))

    def evaluate_batch(self, thetas, total_inj, nobs=None, **_):
        n_obs = self.n_ev if nobs is None else nobs
        out = []
        for th in thetas:
            s = self.sites(th, total_inj)
            out.append(types.SimpleNamespace(log_bfs=s["log_bf"], summary=types.SimpleNamespace(log_det_eff=s["log_mu"], log_nEff_inj=s["log_neff_inj"],
                                                                                                variance_log_likelihood=n_obs**2 * s["var_mu"] + float(np.sum(s["var"])))))
        return out
