"""Weighted index draws: the NumPy statement of what ``gwi_draw_indices`` computes on the device (include/gwi_engine.h,
gwinferno_amd/csrc/gwi_draw.h).  The CPU tests and host-only stand-ins of the engine use it; it is not a fall-back of the
engine, which has none.

A segment is one event's posterior samples, or the injection set.  For log-weights ``lw_j``, a 0/1 mask ``a_j`` and a uniform
``u`` in ``[0, 1)``: ``M`` is the largest ``lw_j`` among samples with ``a_j = 1`` and ``lw_j`` finite, ``w_j = exp(lw_j - M)`` for
those samples and 0 for every other, ``C_j = w_0 + ... + w_j``; the draw is the smallest ``j`` with ``C_j > u C_last`` -- never a
sample with ``w_j = 0``; the last sample with positive weight when rounding runs past the end; ``-1`` when no sample has weight.

``gwi_resample_injections`` (gwinferno_amd/csrc/gwi_resample.h; the reference's ``resample_injections``,
preprocess/selection.py:143-156) draws from the injection segment by the same rule with uniforms of its own:
:func:`resample_uniforms` states them and :func:`resample_indices_reference` the draws."""
import numpy as np

RESAMPLE_TAG = 0x52534D50  # counter word 3 of the resampling stream (gwi_resample.h: kTag)


def draw_weights(logw, mask=None):
    """``w_j`` of one segment: ``exp(lw_j - M)`` where the sample may be drawn, 0 elsewhere (all zeros without a live sample)."""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    live = np.isfinite(lw)
    if mask is not None:
        live &= np.asarray(mask).ravel().astype(bool)
    w = np.zeros(lw.size)
    if live.any():
        w[live] = np.exp(lw[live] - lw[live].max())
    return w


def draw_indices_reference(logw, mask, u):
    """Indices drawn from ONE segment for the uniforms ``u`` (any shape; the result has the same shape, int32)."""
    w = draw_weights(logw, mask)
    u = np.asarray(u, dtype=np.float64)
    out = np.full(u.shape, -1, dtype=np.int32)
    positive = np.nonzero(w > 0.0)[0]
    if positive.size == 0:
        return out
    cdf = np.cumsum(w[positive])  # samples without weight add nothing and can never be the first to exceed the target
    k = np.searchsorted(cdf, u.ravel() * cdf[-1], side="right")
    out.ravel()[:] = positive[np.minimum(k, positive.size - 1)]
    return out


def resample_uniforms(seed, first_index, n):
    """The uniforms of draws ``first_index ... first_index + n`` of ``gwi_resample_injections``: one Philox4x32-10 block each, key =
    the seed's halves, counter ``(index low, index high, 0, RESAMPLE_TAG)``, ``u`` = words 0, 1 by the 53-bit rule -- the
    construction of :func:`gwinferno_amd.population_draws.draw_uniforms` with this stream's tag and table 0."""
    from .spin_priors import _uniform53, philox4x32_10

    m64 = 2**64 - 1
    seed, first_index = int(seed) & m64, int(first_index) & m64
    idx = np.arange(int(n), dtype=np.uint64) + np.uint64(first_index)  # (wraps at 2^64, as the kernel's index does)
    w = philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.zeros(idx.shape, dtype=np.uint64), np.full(idx.shape, RESAMPLE_TAG, dtype=np.uint64),
                      seed & 0xFFFFFFFF, seed >> 32)
    return _uniform53(w[0], w[1])


def resample_indices_reference(logw, mask, seed, first_index, n):
    """Draws ``first_index ... first_index + n`` of the injection segment: :func:`draw_indices_reference` fed with
    :func:`resample_uniforms`."""
    return draw_indices_reference(logw, mask, resample_uniforms(seed, first_index, n))


def draw_indices_segments(logw_pe, logw_inj, pe_mask, inj_mask, u_pe, u_inj):
    """One hyper-parameter point, as ``gwi_draw_indices`` lays it out: ``logw_pe (n_ev, n_pe)``, ``u_pe (n_ev, n_draw_pe)`` ->
    ``(n_ev, n_draw_pe)``; ``logw_inj (n_inj,)``, ``u_inj (n_draw_inj,)`` -> ``(n_draw_inj,)``."""
    logw_pe = np.asarray(logw_pe)
    u_pe = np.asarray(u_pe, dtype=np.float64).reshape(logw_pe.shape[0], -1)
    idx_pe = np.empty(u_pe.shape, dtype=np.int32)
    for ev in range(logw_pe.shape[0]):
        idx_pe[ev] = draw_indices_reference(logw_pe[ev], None if pe_mask is None else np.asarray(pe_mask).reshape(logw_pe.shape)[ev], u_pe[ev])
    return idx_pe, draw_indices_reference(logw_inj, inj_mask, np.asarray(u_inj, dtype=np.float64).ravel())


def mass_cut_masks(pedata, injdata, m1min, m2min, mmax):
    """The reference's posterior-predictive mass cuts (pipeline/analysis.py:326-338) as uint8 masks ``(n_ev, n_pe)`` and
    ``(n_inj,)``: 1 where ``m1min <= m1 <= mmax`` and ``m1 q >= m2min``.  They depend on the catalog only."""

    def one(d):
        with np.errstate(all="ignore"):
            m1, q = np.asarray(d["mass_1"], dtype=np.float64), np.asarray(d["mass_ratio"], dtype=np.float64)
            return (~((m1 < m1min) | (m1 > mmax) | (m1 * q < m2min))).astype(np.uint8)

    return one(pedata), one(injdata)
