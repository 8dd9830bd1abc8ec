"""Weighted index draws: the NumPy statement of what ``gwi_draw_indices`` computes on the device (include/gwi_engine.h,
gwinferno_amd/csrc/gwi_draw.h).  The CPU tests and host-only stand-ins of the engine use it; it is not a fall-back of the
engine, which has none.

A segment is one event's posterior samples, or the injection set.  For log-weights ``lw_j``, a 0/1 mask ``a_j`` and a uniform
``u`` in ``[0, 1)``: ``M`` is the largest ``lw_j`` among samples with ``a_j = 1`` and ``lw_j`` finite, ``w_j = exp(lw_j - M)`` for
those samples and 0 for every other, ``C_j = w_0 + ... + w_j``; the draw is the smallest ``j`` with ``C_j > u C_last`` -- never a
sample with ``w_j = 0``; the last sample with positive weight when rounding runs past the end; ``-1`` when no sample has weight.

``gwi_resample_injections`` (gwinferno_amd/csrc/gwi_resample.h; the reference's ``resample_injections``,
preprocess/selection.py:143-156) draws from the injection segment by the same rule with uniforms of its own:
:func:`resample_uniforms` states them and :func:`resample_indices_reference` the draws.

``gwi_weighted_histograms`` (gwinferno_amd/csrc/gwi_hist.h) sums the same ``w_j`` into bins instead of drawing from them:
:func:`weighted_histograms_reference` states one hyper-parameter point of it, :func:`digitize` the bin codes.

``gwi_marginal_weights_add`` / ``gwi_weighted_quantiles`` (gwinferno_amd/csrc/gwi_quant.h) keep the same ``w_j``, normalised and
summed over the points, per sample -- the marginal posterior weight ``W_j`` -- and select weighted quantiles and moments under it:
:func:`marginal_weights_reference` and :func:`weighted_quantiles_reference` state them.

``gwi_weighted_kde`` / ``gwi_weighted_kde2d`` (gwinferno_amd/csrc/gwi_kde.h) smooth the same ``W_j`` into a Gaussian kernel density
estimate with scipy's bandwidth rules: :func:`weighted_kde_reference` and :func:`weighted_kde2d_reference` state them.

``gwi_marginal_weights_add_weighted`` / ``gwi_weighted_histograms_weighted`` give every (point, segment) a linear weight ``v`` in
``[0, 1]``: the optional ``v`` of :func:`marginal_weights_reference` and :func:`weighted_histograms_reference` states them, and
:func:`leave_one_out_summary` the weights, scores and diagnostics of the leave-one-out posteriors made of them.

``gwi_point_cdfs`` (gwinferno_amd/csrc/gwi_cdf.h) returns, per point, the running sums of the same normalised bins over cumulative
codes -- exact CDFs at the grid points -- for the injection set and, reduced over the events, for the catalog: :func:`cdf_codes`
states the codes, :func:`point_cdfs_reference` one point, and :func:`weighted_percentiles` the bands over the points.

``gwi_point_pits`` (gwinferno_amd/csrc/gwi_pit.h) multiplies, per point, every event's normalised bins into the injection set's CDF: a
rigorous bracket of the event's probability integral transform under the predicted detected distribution.  :func:`pit_bracket` states
the loop and :func:`point_pits_reference` one point.

``gwi_point_pits_exact`` (gwinferno_amd/csrc/gwi_rank.h) gives the same transform without a grid, as the weighted rank of every PE sample
among the injections: :func:`rank_codes` states the theta-independent ranks and :func:`point_pits_exact_reference` one point;
:func:`pareto_smooth` and :func:`pareto_smoothed_summary` smooth the leave-one-out weights on the point axis.

``gwi_point_rank_correlations`` (gwinferno_amd/csrc/gwi_rankcorr.h) ranks the members of a set among themselves -- the pooled PE samples,
the injections -- under the point's weights and returns the second moments of the centred mid-ranks, of which Spearman's correlation
is a ratio: :func:`rankcorr_codes` states the theta-independent codes, :func:`rankcorr_set` one set and
:func:`point_rank_correlations_reference` one point.

``gwi_point_tails`` (gwinferno_amd/csrc/gwi_tail.h) selects, per point and segment, the largest live log-weights and what is needed of
the rest: :func:`tails_segment` and :func:`point_tails_reference` state them, :func:`tail_cutoff_and_rest` what the host derives, and
:func:`pareto_tail_fit` fits the tail under :func:`pareto_smooth`'s conventions.

``gwi_point_bootstrap`` (gwinferno_amd/csrc/gwi_boot.h) sums the same ``w_j`` under Poisson(1) counts that depend on (seed, sample,
replicate) and never on the point: :func:`bootstrap_counts` states the counts, :func:`point_bootstrap_reference` one point, and
:func:`bootstrap_likelihood` the replicates of the likelihood the host forms from the sums."""
import bisect
import itertools
import math

import numpy as np

RESAMPLE_TAG = 0x52534D50  # counter word 3 of the resampling stream (gwi_resample.h: kTag)
OUTSIDE_BIN = 0xFFFF       # bin code of a sample outside every bin (gwi_hist.h: kOutside)


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


def digitize(values, edges):
    """uint16 bin codes of ``values`` for the increasing ``edges`` (``B + 1`` of them, uniform or not), ``np.histogram``'s rule:
    bin ``b`` holds ``edges[b] <= x < edges[b + 1]``, the last bin its right edge too; :data:`OUTSIDE_BIN` for every other value
    (NaN included)."""
    edges = np.asarray(edges, dtype=np.float64).ravel()
    if edges.size < 2 or not np.all(np.diff(edges) > 0):
        raise ValueError("edges must be at least two increasing numbers")
    if edges.size - 1 >= OUTSIDE_BIN:
        raise ValueError("too many bins for a uint16 code")
    x = np.asarray(values, dtype=np.float64)
    code = np.searchsorted(edges, x, side="right") - 1
    code = np.where(x == edges[-1], edges.size - 2, code)
    with np.errstate(invalid="ignore"):
        inside = (x >= edges[0]) & (x <= edges[-1])
    return np.where(inside, code, OUTSIDE_BIN).astype(np.uint16)


def weighted_histogram_segment(logw, mask, bins, n_bins):
    """ONE segment at one point: ``(h (n_cols, n_bins), live)`` with ``h[c][b] = (sum of w_j over the samples with bins[c][j] == b)
    / (sum of w_j over the segment)`` in float64 -- a sample coded :data:`OUTSIDE_BIN` is in no bin but counts in the total --
    and zeros with ``live = False`` when no sample has weight."""
    bins = np.asarray(bins)
    w = draw_weights(logw, mask)
    total = w.sum()
    h = np.zeros((bins.shape[0], int(n_bins)))
    if not (total > 0.0 and np.isfinite(total)):
        return h, False
    for c in range(bins.shape[0]):
        code = bins[c].ravel().astype(np.int64)
        inside = code < n_bins
        h[c] = np.bincount(code[inside], weights=w[inside], minlength=int(n_bins)) / total
    return h, True


def point_weights_array(v, k, n_segs):
    """The linear weights of ``k`` points as a C-contiguous ``(k, n_segs)`` float64 array: ``v`` has that shape, or ``(k,)`` -- one
    weight per point, the same for every segment.  Every entry is a number in ``[0, 1]``; anything else raises ValueError."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape == (k,):
        v = np.repeat(v[:, None], n_segs, axis=1)
    if v.shape != (k, n_segs):
        raise ValueError(f"point weights have shape {v.shape}; expected ({k}, {n_segs}) or ({k},)")
    if not np.all((v >= 0.0) & (v <= 1.0)):
        raise ValueError("point weights must be numbers in [0, 1]")
    return np.ascontiguousarray(v)


def weighted_histograms_reference(logw_pe, logw_inj, pe_mask, inj_mask, pe_bins, inj_bins, n_bins, v=None):
    """One hyper-parameter point of ``gwi_weighted_histograms``: ``logw_pe (n_ev, n_pe)``, ``pe_bins (n_cols, n_ev, n_pe)``,
    ``logw_inj (n_inj,)``, ``inj_bins (n_cols, n_inj)`` -> ``(hist_pe (n_ev, n_cols, n_bins), hist_inj (n_cols, n_bins), dead
    (n_ev + 1,) int32)``: what the point adds to the running sums, and 1 in ``dead`` for every segment without weight (the
    injection set last).  A set whose bins are ``None`` is left out (``None`` in its place, 0 in ``dead``).

    ``v (n_ev + 1,)`` is the point's row of linear weights in ``[0, 1]`` (``gwi_weighted_histograms_weighted``): the point adds ``v
    h`` -- the quotient as without weights, then one product -- and a fourth value is returned, ``vsum (n_ev + 1,)``: ``v`` for every
    live segment of a set that is not left out, 0 elsewhere.  A segment whose ``v`` is 0 adds nothing and is not counted in ``dead``."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev = logw_pe.shape[0]
    dead = np.zeros(n_ev + 1, dtype=np.int32)
    if v is not None:
        v = point_weights_array(np.asarray(v, dtype=np.float64).reshape(1, -1), 1, n_ev + 1)[0]
    vsum = np.zeros(n_ev + 1)
    hist_pe = hist_inj = None

    def one(seg, logw, mask, bins):
        if v is not None and v[seg] == 0.0:
            return np.zeros((bins.shape[0], int(n_bins)))
        h, live = weighted_histogram_segment(logw, mask, bins, n_bins)
        dead[seg] = 0 if live else 1
        if v is not None and live:
            vsum[seg] = v[seg]
            h = v[seg] * h
        return h

    if pe_bins is not None:
        pe_bins = np.asarray(pe_bins)
        pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(logw_pe.shape)
        hist_pe = np.zeros((n_ev, pe_bins.shape[0], int(n_bins)))
        for ev in range(n_ev):
            hist_pe[ev] = one(ev, logw_pe[ev], None if pe_mask is None else pe_mask[ev], pe_bins[:, ev])
    if inj_bins is not None:
        hist_inj = one(n_ev, logw_inj, inj_mask, np.asarray(inj_bins))
    return (hist_pe, hist_inj, dead) if v is None else (hist_pe, hist_inj, dead, vsum)


MAX_CDF_GRID = 256  # grid points per column of gwi_point_cdfs (gwi_hist.h: kMaxBins)


def cdf_codes(values, grid):
    """uint16 CUMULATIVE codes of ``values`` for the grid ``g_0 < ... < g_{G-1}`` of ``gwi_point_cdfs``: the number of grid points
    ``< x`` (``np.searchsorted(grid, x, side="left")``), so code ``j < G`` means ``g_{j-1} < x <= g_j`` and ``x == g_j`` gets ``j``;
    :data:`OUTSIDE_BIN` for a value above ``g_{G-1}`` and for NaN: the sample counts in the segment's total and in no bin.  The
    running sum of a column's bins up to ``j`` is then exactly the weight share with ``x <= g_j``."""
    grid = np.asarray(grid, dtype=np.float64).ravel()
    if not 1 <= grid.size <= MAX_CDF_GRID:
        raise ValueError(f"the grid holds 1 ... {MAX_CDF_GRID} points")
    if not np.all(np.isfinite(grid)) or not np.all(np.diff(grid) > 0):
        raise ValueError("the grid must be finite and strictly increasing")
    x = np.asarray(values, dtype=np.float64)
    code = np.searchsorted(grid, x, side="left")  # (NaN sorts past the end)
    return np.where((code < grid.size) & ~np.isnan(x), code, OUTSIDE_BIN).astype(np.uint16)


def point_cdfs_reference(logw_pe, logw_inj, pe_mask, inj_mask, pe_bins, inj_bins, n_bins):
    """One hyper-parameter point of ``gwi_point_cdfs``: the arguments of :func:`weighted_histograms_reference` with
    the cumulative codes of :func:`cdf_codes` as bins -> ``(out (4, n_cols, n_bins), live (2,) int32)``.  With ``h`` of
    :func:`weighted_histogram_segment` and ``F = np.cumsum(h, axis=-1)`` per segment: slot 0 is ``F`` of the injection set (NaN
    when it has no weight or ``inj_bins`` is None); slot 1 ``(sum of F over the live events, in event order) / n_live`` (NaN when
    no event is live or ``pe_bins`` is None); slot 2 the sum of ``log F`` over the live events -- the log CDF of the catalog's
    maximum, ``-inf`` where an event has no weight at or below the grid point; slot 3 the sum of ``log1p(-min(F, 1))`` -- the CDF of
    the catalog's minimum is ``1 - exp`` of it.  Slots 2 and 3 are NaN without ``pe_bins`` and 0 without a live event.  ``live =
    (n_live, 1 if the injection set is live else 0)``."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_bins = logw_pe.shape[0], int(n_bins)
    n_cols = np.asarray(pe_bins if pe_bins is not None else inj_bins).shape[0]
    out = np.full((4, n_cols, n_bins), np.nan)
    live = np.zeros(2, dtype=np.int32)
    if inj_bins is not None:
        h, alive = weighted_histogram_segment(logw_inj, inj_mask, np.asarray(inj_bins), n_bins)
        if alive:
            out[0], live[1] = np.cumsum(h, axis=-1), 1
    if pe_bins is not None:
        pe_bins = np.asarray(pe_bins)
        pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(logw_pe.shape)
        sum_f, below, above = np.zeros((n_cols, n_bins)), np.zeros((n_cols, n_bins)), np.zeros((n_cols, n_bins))
        with np.errstate(divide="ignore"):
            for ev in range(n_ev):
                h, alive = weighted_histogram_segment(logw_pe[ev], None if pe_mask is None else pe_mask[ev], pe_bins[:, ev], n_bins)
                if not alive:
                    continue
                f = np.cumsum(h, axis=-1)
                live[0] += 1
                sum_f += f
                below += np.log(f)
                above += np.log1p(-np.minimum(f, 1.0))
        if live[0]:
            out[1] = sum_f / float(live[0])
        out[2], out[3] = below, above
    return out, live


def pit_bracket(q, D):
    """The loop of ``gwi_point_pits`` alone: ``q (G,)`` the normalised bins of one event and column over cumulative codes,
    ``D (G,)`` the CDF of the predicted detected distribution at the same grid points -> ``(pit_lo, pit_hi)`` as Python floats.  With
    ``o = max(0, 1 - cumsum(q)[G-1])``, the share above the grid: a sample with code ``j`` has its ``F_det`` in ``[D[j-1], D[j]]`` (``D[-1]
    := 0``), one outside in ``[D[G-1], 1]``, so

    ``pit_lo = q[1] D[0] + ... + q[G-1] D[G-2] + o D[G-1]`` and ``pit_hi = q[0] D[0] + ... + q[G-1] D[G-1] + o``

    bracket the un-gridded PIT.  Either is summed from 0.0 strictly left to right, the outside term last, every product and every
    sum a float64 operation of its own: the kernel's bits."""
    q, D = np.asarray(q, dtype=np.float64).ravel(), np.asarray(D, dtype=np.float64).ravel()
    if q.size < 1 or q.size != D.size:
        raise ValueError("q and D hold the same number (>= 1) of grid points")
    n = q.size
    o = max(0.0, 1.0 - float(np.cumsum(q)[-1]))
    ql, dl = q.tolist() + [o], D.tolist()
    lo = hi = 0.0
    for j in range(n):
        lo = lo + ql[j + 1] * dl[j]
        hi = hi + ql[j] * dl[j]
    return lo, hi + o


def point_pits_reference(logw_pe, logw_inj, pe_mask, inj_mask, pe_bins, inj_bins, n_bins):
    """One hyper-parameter point of ``gwi_point_pits``: the arguments of :func:`point_cdfs_reference`, both sets of
    cumulative codes given -> ``(pit (n_ev, n_cols, 2), cdf_det (n_cols, n_bins), dead (n_ev + 1,) int32)``.  With ``q`` of
    :func:`weighted_histogram_segment` per event and ``D = np.cumsum`` of the injection set's: ``pit[e][c] =``
    :func:`pit_bracket` ``(q[c], D[c])``; NaN for an event without weight, and everywhere (``cdf_det`` included) when the injection
    set has none; ``dead`` flags the segments without weight, the injection set last."""
    if pe_bins is None or inj_bins is None:
        raise ValueError("an event's PIT needs the bins of both sets")
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    pe_bins, inj_bins = np.asarray(pe_bins), np.asarray(inj_bins)
    n_ev, n_bins, n_cols = logw_pe.shape[0], int(n_bins), pe_bins.shape[0]
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(logw_pe.shape)
    pit, cdf_det, dead = np.full((n_ev, n_cols, 2), np.nan), np.full((n_cols, n_bins), np.nan), np.zeros(n_ev + 1, dtype=np.int32)
    h, inj_alive = weighted_histogram_segment(logw_inj, inj_mask, inj_bins, n_bins)
    if inj_alive:
        cdf_det = np.cumsum(h, axis=-1)
    dead[n_ev] = 0 if inj_alive else 1
    for ev in range(n_ev):
        q, alive = weighted_histogram_segment(logw_pe[ev], None if pe_mask is None else pe_mask[ev], pe_bins[:, ev], n_bins)
        dead[ev] = 0 if alive else 1
        if alive and inj_alive:
            for c in range(n_cols):
                pit[ev, c] = pit_bracket(q[c], cdf_det[c])
    return pit, cdf_det, dead


def weighted_percentiles(values, weights, levels):
    """Percentiles over the FIRST axis of ``values (K, ...)`` under the weights ``(K,)``, rule "inverted CDF" as in
    :func:`weighted_quantiles_reference`: per trailing index the value at the smallest rank ``r`` (values ascending, ties in point
    order) with ``C_r >= p C_last`` and weight there -- a value of the input, never an interpolation -- ``(Q, ...)``.  Points whose value
    is NaN or whose weight is 0 are left out; NaN where none is left.  The prefix is a plain float64 ``cumsum``."""
    values, weights = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64).ravel()
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if values.ndim < 1 or values.shape[0] != weights.size:
        raise ValueError("one weight per entry of the first axis")
    if np.any(~np.isfinite(weights)) or np.any(weights < 0.0):
        raise ValueError("weights must be finite and non-negative")
    if levels.ndim != 1 or np.any(~((levels >= 0.0) & (levels <= 1.0))):
        raise ValueError("levels must lie in [0, 1]")
    k = values.shape[0]
    flat = values.reshape(k, -1)
    out = np.full((levels.size, flat.shape[1]), np.nan)
    for j in range(flat.shape[1]):
        col = flat[:, j]
        keep = np.nonzero(~np.isnan(col) & (weights > 0.0))[0]
        if keep.size == 0:
            continue
        keep = keep[np.argsort(col[keep], kind="stable")]
        cum = np.cumsum(weights[keep])
        r = np.minimum(np.searchsorted(cum, levels * cum[-1], side="left"), keep.size - 1)
        out[:, j] = col[keep[r]]
    return out.reshape((levels.size,) + values.shape[1:])


def marginal_weights_reference(logw_pe, logw_inj, pe_mask, inj_mask, v=None):
    """The state ``gwi_marginal_weights_add`` leaves after the K points of ``logw_pe (K, n_ev, n_pe)`` and ``logw_inj (K, n_inj)``,
    added in order: ``(W_pe (n_ev, n_pe), W_inj (n_inj,), dead (n_ev + 1,) int32, n_points)`` with ``W_j = sum_k w_kj / S_k``,
    ``w`` from :func:`draw_weights` under the masks and ``S_k`` the segment's total by ``math.fsum`` (the exact sum, rounded once);
    a segment whose total is 0 adds nothing at that point and is counted in ``dead`` (the injection set last).

    ``v (K, n_ev + 1)`` (or ``(K,)``: the same for every segment) gives every (point, segment) a linear weight in ``[0, 1]``
    (``gwi_marginal_weights_add_weighted``): ``W_j = sum_k v_k (w_kj / S_k)`` -- the quotient as without weights, then one product --
    and two more values are returned, ``vsum`` and ``vsum2 (n_ev + 1,)``: the sums of ``v`` and of ``v v`` over the points at which
    the segment is live, in point order.  A point whose ``v`` is 0 adds nothing, is counted in ``n_points`` and not in ``dead``."""
    logw_pe, logw_inj = np.asarray(logw_pe, dtype=np.float64), np.asarray(logw_inj, dtype=np.float64)
    if logw_pe.ndim != 3 or logw_inj.ndim != 2 or logw_pe.shape[0] != logw_inj.shape[0]:
        raise ValueError("logw_pe is (K, n_ev, n_pe) and logw_inj (K, n_inj)")
    k, n_ev, n_pe = logw_pe.shape
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    w_pe, w_inj, dead = np.zeros((n_ev, n_pe)), np.zeros(logw_inj.shape[1]), np.zeros(n_ev + 1, dtype=np.int32)
    if v is not None:
        v = point_weights_array(v, k, n_ev + 1)
    vsum, vsum2 = np.zeros(n_ev + 1), np.zeros(n_ev + 1)
    for p in range(k):
        for seg in range(n_ev + 1):
            if v is not None and v[p, seg] == 0.0:
                continue
            w = draw_weights(logw_pe[p, seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else draw_weights(logw_inj[p], inj_mask)
            total = math.fsum(w.tolist())
            if not (total > 0.0 and np.isfinite(total)):
                dead[seg] += 1
                continue
            share = w / total
            if v is not None:
                share = v[p, seg] * share
                vsum[seg] += v[p, seg]
                vsum2[seg] += v[p, seg] * v[p, seg]
            if seg < n_ev:
                w_pe[seg] += share
            else:
                w_inj += share
    return (w_pe, w_inj, dead, k) if v is None else (w_pe, w_inj, dead, k, vsum, vsum2)


def leave_one_out_summary(log_l_event):
    """The leave-one-out weights, scores and diagnostics of ``log_l_event (K, n_ev)``, the table of ``l_ke``: event e's contribution
    to ``log L`` at hyper-posterior point k.  The points are draws from ``p(theta | all events)``; weighting point k by
    ``1 / exp(l_ke)`` turns them into draws from ``p(theta | all events but e)``.  Returns a dict:

    ``point_weights (K, n_ev + 1)``: ``exp(-l_ke + min_k l_ke)`` -- linear, the largest of every event exactly 1 -- and a last column
    of ones for the injection set, which has no event of its own; ``elpd_loo (n_ev,)``: ``-log mean_k exp(-l_ke)``, the logarithm of
    the event's leave-one-out predictive density (importance sampling; summed over the events it compares two population models
    fitted to one catalog); ``lpd (n_ev,)``: ``log mean_k exp(l_ke)``, the same without leaving the event out; ``neff_points
    (n_ev,)``: ``(sum_k v)^2 / sum_k v^2``, the effective number of points -- the reliability diagnostic of these raw weights (:func:`pareto_smoothed_summary` smooths them);
    ``n_bad (n_ev,)``: the points at which ``l_ke`` is not finite: they get weight 0 and the means run over the other points (NaN
    where there is none)."""
    ell = np.asarray(log_l_event, dtype=np.float64)
    if ell.ndim != 2 or ell.shape[0] < 1:
        raise ValueError("log_l_event is (K, n_ev) with K >= 1")
    k, n_ev = ell.shape
    good = np.isfinite(ell)
    n_good = good.sum(axis=0)
    n_bad = (k - n_good).astype(np.int64)
    v = np.ones((k, n_ev + 1))
    elpd, lpd, neff = np.full(n_ev, np.nan), np.full(n_ev, np.nan), np.zeros(n_ev)
    for e in range(n_ev):
        v[:, e] = 0.0
        if not n_good[e]:
            continue
        col = ell[good[:, e], e]
        lo, hi = col.min(), col.max()
        ve = np.exp(lo - col)
        v[good[:, e], e] = ve
        s1 = math.fsum(ve.tolist())
        elpd[e] = lo - math.log(s1 / n_good[e])
        lpd[e] = hi + math.log(math.fsum(np.exp(col - hi).tolist()) / n_good[e])
        neff[e] = s1 * s1 / math.fsum((ve * ve).tolist())
    return {"log_l_event": ell, "point_weights": v, "elpd_loo": elpd, "lpd": lpd, "neff_points": neff, "n_bad": n_bad}


def _exact_integers(w):
    """The non-negative finite doubles ``w`` as Python integers in units of one common power of two: ``(ints, exponent)`` with
    ``w_j == ints[j] * 2**exponent`` exactly."""
    m, e = np.frexp(np.asarray(w, dtype=np.float64))
    mant = np.ldexp(m, 53).astype(np.int64)  # (53 bits: exact)
    e = e.astype(np.int64) - 53
    low = int(e[mant > 0].min()) if np.any(mant > 0) else 0
    return [int(a) << (int(b) - low) if a else 0 for a, b in zip(mant.tolist(), e.tolist())], low


def weighted_quantiles_reference(W, order, x, levels):
    """Quantiles and moments of ONE segment and ONE quantity under the marginal weights ``W (n,)``: ``order (n,)`` is a permutation
    of the sample indices along which ``x (n,)`` does not decrease (``np.argsort(x, kind="stable")``), ``levels`` lie in ``[0, 1]``.
    Rule "inverted CDF" with an EXACT prefix (integer arithmetic on the doubles' bits: the exact answer, not a second rounding):
    the sample at the smallest rank ``r`` with ``C_r >= p C_last`` and ``W > 0`` there, ``C_r = W[order[0]] + ... + W[order[r]]``;
    ``-1`` without weight.  ``p = 0`` is the smallest value with weight, ``p = 1`` the largest.  Returns ``(idx (Q,) int32, (m1, m2),
    mass)`` with ``m1 = sum W x``, ``m2 = sum W x^2`` (``math.fsum`` of the rounded products) and ``mass = C_last`` rounded once."""
    W, x = np.asarray(W, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).ravel()
    order = np.asarray(order).ravel().astype(np.int64)
    levels = np.asarray(levels, dtype=np.float64).ravel()
    if not (W.size == x.size == order.size) or not np.array_equal(np.sort(order), np.arange(W.size)):
        raise ValueError("order must be a permutation of the segment's sample indices")
    if np.any(~np.isfinite(W)) or np.any(W < 0.0):
        raise ValueError("W must be finite and non-negative")
    if np.any(~((levels >= 0.0) & (levels <= 1.0))):
        raise ValueError("levels must lie in [0, 1]")
    ws, xs = W[order], x[order]
    if np.any(np.diff(xs) < 0.0):
        raise ValueError("x decreases along the order")
    idx = np.full(levels.size, -1, dtype=np.int32)
    live = np.nonzero(ws > 0.0)[0]
    if live.size == 0:
        return idx, (0.0, 0.0), 0.0
    ints, low = _exact_integers(ws[live])
    cum = list(itertools.accumulate(ints))  # exact inclusive prefixes over the ranks with weight
    c_last = cum[-1]
    for q, p in enumerate(levels.tolist()):
        num, den = float(p).as_integer_ratio()
        target = -((-num * c_last) // den)  # the smallest integer >= p C_last: C_r >= p C_last exactly when C_r >= it
        idx[q] = order[live[min(bisect.bisect_left(cum, target), live.size - 1)]]
    m1, m2 = math.fsum((ws * xs).tolist()), math.fsum((ws * xs * xs).tolist())
    mass = c_last / 2 ** (-low) if low < 0 else float(c_last * 2**low)  # (true division of integers rounds once)
    return idx, (m1, m2), float(mass)


KDE_RULES = {"scott": 0, "silverman": 1}  # the rule codes of gwi_weighted_kde / gwi_weighted_kde2d


def kde_rule_code(rule):
    if rule not in KDE_RULES:
        raise ValueError(f"rule must be 'scott' or 'silverman', not {rule!r}")
    return KDE_RULES[rule]


def _kde_weights(W, *columns):
    """The normalised weights of one segment and what scipy.stats.gaussian_kde derives from them: ``(p, s2, n_eff, state)`` with
    ``state`` "dead" (no weight: ``p`` is None), "degenerate" (fewer than two samples with weight) or "live"."""
    W = np.asarray(W, dtype=np.float64).ravel()
    if any(c.shape != W.shape for c in columns):
        raise ValueError("the values have the shape of W")
    if np.any(~np.isfinite(W)) or np.any(W < 0.0):
        raise ValueError("W must be finite and non-negative")
    if any(np.any(~np.isfinite(c)) for c in columns):
        raise ValueError("the values must be finite")
    mass = float(np.sum(W))
    if not (mass > 0.0 and np.isfinite(mass)):
        return None, np.nan, 0.0, "dead"
    p = W / mass
    s2 = float(np.sum(p * p))
    return p, s2, 1.0 / s2, "live" if np.count_nonzero(W > 0.0) >= 2 else "degenerate"


def kde_factor(n_eff, d, rule="scott", scale=1.0):
    """scipy.stats.gaussian_kde's factor on the square root of the covariance: ``n_eff^(-1/(d+4))`` (Scott) or
    ``(n_eff (d+2)/4)^(-1/(d+4))`` (Silverman), times ``scale``."""
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError("scale must be a positive finite number")
    base = n_eff * (d + 2.0) / 4.0 if kde_rule_code(rule) == 1 else n_eff
    return float(scale) * base ** (-1.0 / (d + 4.0))


def weighted_kde_reference(W, x, grid, rule="scott", scale=1.0, bounds=None):
    """The Gaussian kernel density estimate of ONE segment and ONE quantity under the marginal weights ``W (n,)`` at the points
    ``grid (G,)``: ``(rho (G,), h, n_eff, degenerate)``.  With ``p = W / sum W``: ``s2 = sum p^2``, ``n_eff = 1 / s2``, the CENTRED
    variance ``sum p (x - mean)^2 / (1 - s2)``, ``h^2 = var f^2`` with :func:`kde_factor`'s ``f``, and ``rho(g) = sum_i p_i
    exp(-(g - x_i)^2 / 2 h^2) / sqrt(2 pi h^2)`` -- scipy.stats.gaussian_kde(x, weights=W, bw_method=...).  ``bounds = (lo, hi)``
    (either may be None or NaN) reflects: the images ``2 lo - x_i`` and ``2 hi - x_i`` are added at points inside ``[lo, hi]``,
    points outside get 0, and the bandwidth stays that of the unreflected data.  Plain float64 sums.  A segment without weight
    gives NaN, ``n_eff = 0`` and no flag; one with fewer than two samples with weight, or whose variance is not positive and
    finite, gives NaN and ``degenerate = 1``."""
    x, grid = np.asarray(x, dtype=np.float64).ravel(), np.asarray(grid, dtype=np.float64).ravel()
    if np.any(~np.isfinite(grid)):
        raise ValueError("grid points must be finite")
    f_of = lambda n_eff: kde_factor(n_eff, 1, rule, scale)  # noqa: E731  (checks rule and scale whatever the segment)
    f_of(1.0)
    p, s2, n_eff, state = _kde_weights(W, x)
    nothing = np.full(grid.shape, np.nan)
    if state == "dead":
        return nothing, np.nan, 0.0, 0
    if state == "degenerate":
        return nothing, np.nan, n_eff, 1
    mean = float(np.sum(p * x))
    with np.errstate(divide="ignore", invalid="ignore"):
        h2 = float(np.sum(p * (x - mean) ** 2)) / (1.0 - s2) * f_of(n_eff) ** 2
    if not (h2 > 0.0 and np.isfinite(h2)):
        return nothing, np.nan, n_eff, 1
    lo, hi = (np.nan, np.nan) if bounds is None else (np.nan if b is None else float(b) for b in bounds)
    live = p > 0.0
    pl, xl = p[live], x[live]
    kernel = lambda pts: np.exp(-0.5 / h2 * (grid[:, None] - pts[None, :]) ** 2)  # noqa: E731
    e = kernel(xl)
    if lo == lo:
        e = e + kernel(2.0 * lo - xl)
    if hi == hi:
        e = e + kernel(2.0 * hi - xl)
    rho = np.sum(e * pl[None, :], axis=1) / np.sqrt(2.0 * np.pi * h2)
    rho[(grid < lo) | (grid > hi)] = 0.0
    return rho, float(np.sqrt(h2)), n_eff, 0


def weighted_kde2d_reference(W, x, y, gridx, gridy, rule="scott", scale=1.0):
    """The two-dimensional counterpart of :func:`weighted_kde_reference` on the tensor grid ``gridx (n_gx,) x gridy (n_gy,)``:
    ``(rho (n_gx, n_gy), H (3,) = (Hxx, Hxy, Hyy), n_eff, degenerate)`` with ``H = f^2 Cov``, the full centred weighted covariance
    ``sum p (x - mean_x)(y - mean_y) / (1 - s2)``, and ``rho(gx, gy) = sum_i p_i exp(-d^T H^-1 d / 2) / (2 pi sqrt|H|)``.  No
    reflection.  Degenerate also where ``|H|`` is not positive and finite."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    gridx, gridy = np.asarray(gridx, dtype=np.float64).ravel(), np.asarray(gridy, dtype=np.float64).ravel()
    if np.any(~np.isfinite(gridx)) or np.any(~np.isfinite(gridy)):
        raise ValueError("grid points must be finite")
    kde_factor(1.0, 2, rule, scale)
    p, s2, n_eff, state = _kde_weights(W, x, y)
    nothing, no_h = np.full((gridx.size, gridy.size), np.nan), np.full(3, np.nan)
    if state == "dead":
        return nothing, no_h, 0.0, 0
    if state == "degenerate":
        return nothing, no_h, n_eff, 1
    dx, dy = x - float(np.sum(p * x)), y - float(np.sum(p * y))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = kde_factor(n_eff, 2, rule, scale) ** 2 / (1.0 - s2)
        hxx, hxy, hyy = float(np.sum(p * dx * dx)) * k, float(np.sum(p * dx * dy)) * k, float(np.sum(p * dy * dy)) * k
        det = hxx * hyy - hxy * hxy
    if not (det > 0.0 and np.isfinite(det) and hxx > 0.0 and hyy > 0.0):
        return nothing, no_h, n_eff, 1
    live = p > 0.0
    pl, ex, ey = p[live], gridx[:, None] - x[live][None, :], gridy[:, None] - y[live][None, :]  # (n_gx, n), (n_gy, n)
    rho = np.empty((gridx.size, gridy.size))
    for i in range(gridx.size):  # (one row of the map at a time: n_gy x n numbers)
        arg = (-0.5 * hyy / det) * ex[i] ** 2 + (hxy / det) * ex[i] * ey + (-0.5 * hxx / det) * ey**2
        rho[i] = np.sum(np.exp(arg) * pl[None, :], axis=1)
    return rho / (2.0 * np.pi * np.sqrt(det)), np.array([hxx, hxy, hyy]), n_eff, 0


MAX_RANK_COLUMNS = 8  # columns of gwi_set_rank_columns (gwi_rank.h: kMaxCols)


def rank_codes(pe_values, inj_values):
    """The theta-independent setup of ``gwi_point_pits_exact``: ``pe_values (n_cols, n_ev, n_pe)`` and ``inj_values
    (n_cols, n_inj)``, finite -> ``(order_inj (n_cols, n_inj), rank_lt (n_cols, n_ev, n_pe), rank_le (n_cols, n_ev, n_pe))``, all
    int32.  Per column ``order_inj`` is a stable argsort of the injection values, ``rank_lt`` the number of injections with ``x_inj <
    x`` (``np.searchsorted(..., "left")``) and ``rank_le`` the number with ``x_inj <= x`` (``"right"``) of every PE sample: numbers in
    ``[0, n_inj]`` with ``rank_lt <= rank_le``, equal unless the sample ties with an injection."""
    pe, inj = np.asarray(pe_values, dtype=np.float64), np.asarray(inj_values, dtype=np.float64)
    if pe.ndim != 3 or inj.ndim != 2 or pe.shape[0] != inj.shape[0]:
        raise ValueError(f"pe_values is (n_cols, n_ev, n_pe) and inj_values (n_cols, n_inj); got {pe.shape} and {inj.shape}")
    if not 1 <= pe.shape[0] <= MAX_RANK_COLUMNS:
        raise ValueError(f"{pe.shape[0]} columns: between 1 and {MAX_RANK_COLUMNS} can be ranked")
    if inj.shape[1] >= 2**31 - 1:
        raise ValueError("more injections than an int32 rank can count")
    if not np.all(np.isfinite(pe)) or not np.all(np.isfinite(inj)):
        raise ValueError("the values must be finite")
    order = np.argsort(inj, axis=-1, kind="stable")
    lt, le = np.empty(pe.shape, dtype=np.int32), np.empty(pe.shape, dtype=np.int32)
    for c in range(pe.shape[0]):
        ascending = inj[c][order[c]]
        lt[c] = np.searchsorted(ascending, pe[c], side="left")
        le[c] = np.searchsorted(ascending, pe[c], side="right")
    return np.ascontiguousarray(order, dtype=np.int32), lt, le


def _rounded_prefix(w):
    """``P (n + 1,)`` with ``P[r] = w[0] + ... + w[r-1]``, every entry the EXACT sum rounded once (integer arithmetic on the doubles'
    bits, as :func:`weighted_quantiles_reference`'s prefix); ``w`` finite and non-negative."""
    ints, low = _exact_integers(w)
    cum = [0] + list(itertools.accumulate(ints))
    if low < 0:
        den = 2 ** (-low)
        return np.array([c / den for c in cum], dtype=np.float64)  # (true division of integers rounds once)
    return np.array([float(c * 2**low) for c in cum], dtype=np.float64)


def point_pits_exact_reference(logw_pe, logw_inj, pe_mask, inj_mask, order_inj, rank_lt, rank_le):
    """One hyper-parameter point of ``gwi_point_pits_exact``: ``logw_pe (n_ev, n_pe)``, ``logw_inj (n_inj,)``, the masks of
    ``gwi_set_draw_mask`` (or None) and the arrays of :func:`rank_codes` -> ``(pit (n_ev, n_cols, 2), dead (n_ev + 1,) int32)``.  With
    ``u`` and ``w`` of :func:`draw_weights` for the injection set and the event, ``P[c][r]`` the sum of ``u`` over the first ``r``
    injections along ``order_inj[c]`` (exact, rounded once), ``T_c = P[c][n_inj]`` and ``S`` the event's total (``math.fsum``):

    ``pit[e][c] = (fsum_i w_i P[c][rank_lt_i] / S / T_c, fsum_i w_i P[c][rank_le_i] / S / T_c)``

    -- the event's un-gridded probability integral transform under ``F_det(x) = share of detected weight with x_inj < x`` (first) or
    ``x_inj <= x`` (second); the two differ only through ties between the two sets, and their midpoint is the expectation of the
    randomised PIT.  NaN for an event whose ``S`` is 0 or not finite, and everywhere when the injection set's total is; ``dead`` flags
    the segments without weight, the injection set last."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    order_inj, rank_lt, rank_le = np.asarray(order_inj), np.asarray(rank_lt), np.asarray(rank_le)
    n_ev, n_pe = logw_pe.shape
    n_cols, n_inj = order_inj.shape
    if rank_lt.shape != (n_cols, n_ev, n_pe) or rank_le.shape != rank_lt.shape:
        raise ValueError("rank_lt and rank_le are (n_cols, n_ev, n_pe)")
    if rank_lt.size and (rank_lt.min() < 0 or rank_le.max() > n_inj or np.any(rank_lt > rank_le)):
        raise ValueError("the ranks lie in [0, n_inj] with rank_lt <= rank_le")
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    pit, dead = np.full((n_ev, n_cols, 2), np.nan), np.zeros(n_ev + 1, dtype=np.int32)
    u = draw_weights(logw_inj, inj_mask)
    t_all = math.fsum(u.tolist())
    inj_alive = t_all > 0.0 and np.isfinite(t_all)
    dead[n_ev] = 0 if inj_alive else 1
    prefix = [_rounded_prefix(u[order_inj[c].astype(np.int64)]) for c in range(n_cols)] if inj_alive else None
    for ev in range(n_ev):
        w = draw_weights(logw_pe[ev], None if pe_mask is None else pe_mask[ev])
        total = math.fsum(w.tolist())
        alive = total > 0.0 and np.isfinite(total)
        dead[ev] = 0 if alive else 1
        if not (alive and inj_alive):
            continue
        for c in range(n_cols):
            p = prefix[c]
            for i, ranks in enumerate((rank_lt[c, ev], rank_le[c, ev])):
                pit[ev, c, i] = math.fsum((w * p[ranks]).tolist()) / total / p[n_inj]
    return pit, dead


MAX_RANKCORR_COLUMNS = 8  # columns of gwi_set_rankcorr_columns (gwi_rankcorr.h: kMaxCols)
RANKCORR_TILE = 1024      # members per tile of the device's sums (gwi_draw.h: kDrawTile)


def rankcorr_codes(values):
    """The theta-independent setup of ``gwi_point_rank_correlations`` for ONE rank set: ``values (n_cols, n)``, finite --
    for the observed set the pooled ``(n_cols, n_ev n_pe)`` array -- -> ``(order, lt, le)``, each ``(n_cols, n)`` int32.  Per column
    ``order`` is the stable argsort of the values, ``lt`` the number of members of the same set with a smaller value
    (``np.searchsorted(..., "left")`` of the column in itself) and ``le`` the number with a value not larger (``"right"``): ``lt <=
    position of the member along the order < le``.  Only the order of the values enters: a strictly increasing map of a column leaves
    the three arrays as they are."""
    x = np.asarray(values, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"values is (n_cols, n); got {x.shape}")
    if not 1 <= x.shape[0] <= MAX_RANKCORR_COLUMNS:
        raise ValueError(f"{x.shape[0]} columns: between 1 and {MAX_RANKCORR_COLUMNS} can be ranked")
    if x.shape[1] >= 2**31 - 1:
        raise ValueError("more members than an int32 rank can count")
    if not np.all(np.isfinite(x)):
        raise ValueError("the values must be finite")
    order = np.argsort(x, axis=-1, kind="stable")
    lt, le = np.empty(x.shape, dtype=np.int32), np.empty(x.shape, dtype=np.int32)
    for c in range(x.shape[0]):
        ascending = x[c][order[c]]
        lt[c] = np.searchsorted(ascending, x[c], side="left")
        le[c] = np.searchsorted(ascending, x[c], side="right")
    return np.ascontiguousarray(order, dtype=np.int32), lt, le


def rankcorr_set(u, order, lt, le):
    """``(out (1 + C + C (C + 1) / 2,), alive)`` of ONE rank set with the members' weights ``u (n,)``, finite and non-negative, and the
    codes of :func:`rankcorr_codes`.  With ``P[c][r]`` the sum of ``u`` over the first ``r`` members along ``order[c]`` (exact, rounded
    once) and ``T_c = P[c][n]``:

    ``d_ci = ((P[c][lt_i] + P[c][le_i]) - T_c) / (2 T_c)``, the centred weighted mid-rank, and ``r_ci = 0.5 + d_ci``;
    ``out = (U, m_0 ... m_{C-1}, R_00, R_01, ..., R_{C-1,C-1})`` with ``U = fsum u``, ``m_c = fsum_i (u_i r_ci) / U`` and ``R_cd = fsum_i
    ((u_i d_ci) d_di) / U`` for ``c <= d``, the upper triangle row by row

    -- every product rounded on its own, every sum exact and rounded once (``math.fsum``).  Ties share a rank; a column whose members
    all tie has ``d = 0``, ``r = 0.5`` and ``R_cc = 0`` exactly; ``m_c`` is 0.5 in exact arithmetic.  Where ``U`` is 0 or not finite
    ``alive`` is False and every slot but ``U`` NaN."""
    u = np.asarray(u, dtype=np.float64).ravel()
    order, lt, le = np.asarray(order), np.asarray(lt), np.asarray(le)
    n_cols, n = order.shape
    if u.size != n or lt.shape != order.shape or le.shape != order.shape:
        raise ValueError("u is (n,), order, lt and le are (n_cols, n)")
    out = np.full(1 + n_cols + n_cols * (n_cols + 1) // 2, np.nan)
    total = math.fsum(u.tolist())
    out[0] = total
    if not (total > 0.0 and np.isfinite(total)):
        return out, False
    live = u > 0.0
    ul = u[live]
    d = np.empty((n_cols, ul.size))
    for c in range(n_cols):
        prefix = _rounded_prefix(u[order[c].astype(np.int64)])
        t_c = prefix[n]
        d[c] = ((prefix[lt[c][live]] + prefix[le[c][live]]) - t_c) / (2.0 * t_c)
        out[1 + c] = math.fsum((ul * (0.5 + d[c])).tolist()) / total
    t = 1 + n_cols
    for c in range(n_cols):
        ud = ul * d[c]
        for e in range(c, n_cols):
            out[t] = math.fsum((ud * d[e]).tolist()) / total
            t += 1
    return out, True


def rankcorr_weights(logw_pe, logw_inj, pe_mask=None, inj_mask=None):
    """The members' weights of the two rank sets at one point: ``(u_obs (n_ev n_pe,), u_det (n_inj,), dead (n_ev + 1,)
    int32)``.  ``u_obs`` pools the events: ``w_i / S_e`` with ``w`` of :func:`draw_weights` and ``S_e`` its ``math.fsum``, one division
    per sample, 0 for the samples of an event whose ``S_e`` is 0 or not finite; ``u_det`` is :func:`draw_weights` of the injection
    set.  ``dead`` flags the segments without weight, the injection set last."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_pe = logw_pe.shape
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    u_obs, dead = np.zeros((n_ev, n_pe)), np.zeros(n_ev + 1, dtype=np.int32)
    for ev in range(n_ev):
        w = draw_weights(logw_pe[ev], None if pe_mask is None else pe_mask[ev])
        total = math.fsum(w.tolist())
        if total > 0.0 and np.isfinite(total):
            u_obs[ev] = w / total
        else:
            dead[ev] = 1
    u_det = draw_weights(logw_inj, inj_mask)
    t_det = math.fsum(u_det.tolist())
    dead[n_ev] = 0 if t_det > 0.0 and np.isfinite(t_det) else 1
    return u_obs.ravel(), u_det, dead


def point_rank_correlations_reference(logw_pe, logw_inj, codes_obs, codes_det, pe_mask=None, inj_mask=None):
    """One hyper-parameter point of ``gwi_point_rank_correlations``: ``logw_pe (n_ev, n_pe)``, ``logw_inj (n_inj,)``,
    ``codes_obs`` and ``codes_det`` the triples of :func:`rankcorr_codes` of the pooled PE values and of the injection values, and the
    masks of ``gwi_set_draw_mask`` (or None) -> ``(out (2, 1 + C + C (C + 1) / 2), dead (n_ev + 2,) int32)``: per set (observed,
    detected) :func:`rankcorr_set` on the weights of :func:`rankcorr_weights`; ``dead`` flags the segments without weight, the
    injection set last, and then the observed set, which is dead when no event is live.  Spearman's rho of columns ``c <= d`` is ``R_cd /
    sqrt(R_cc R_dd)`` (:func:`rankcorr_matrix` unpacks the triangle)."""
    u_obs, u_det, seg_dead = rankcorr_weights(logw_pe, logw_inj, pe_mask, inj_mask)
    obs, obs_alive = rankcorr_set(u_obs, *codes_obs)
    det, _ = rankcorr_set(u_det, *codes_det)
    if obs.size != det.size:
        raise ValueError("the two sets hold different numbers of columns")
    return np.stack([obs, det]), np.concatenate([seg_dead, [0 if obs_alive else 1]]).astype(np.int32)


def rankcorr_matrix(out, n_cols):
    """``(U (...,), mean_rank (..., C), R (..., C, C))`` of rows ``out (..., 1 + C + C (C + 1) / 2)`` of ``gwi_point_rank_correlations``:
    the symmetric matrix filled from the upper triangle."""
    out = np.asarray(out, dtype=np.float64)
    iu = np.triu_indices(n_cols)
    cov = np.empty(out.shape[:-1] + (n_cols, n_cols))
    cov[..., iu[0], iu[1]] = out[..., 1 + n_cols :]
    cov[..., iu[1], iu[0]] = out[..., 1 + n_cols :]
    return np.ascontiguousarray(out[..., 0]), np.ascontiguousarray(out[..., 1 : 1 + n_cols]), cov


def rankcorr_error_bound(n_terms, n_order_tiles, n_sample_tiles, pooled):
    """An ABSOLUTE bound on the rounding of one ``R_cd`` of ``gwi_point_rank_correlations`` and of the statement together (DESIGN 8l,
    "Error"), from counts of roundings alone: ``n_terms`` bounds the live samples of one segment, ``n_order_tiles`` the tiles along
    the set's order, ``n_sample_tiles`` its tiles in sample order; ``pooled`` for the observed set, whose weights carry their
    event's total.  ``|d| <= 1/2`` makes the bound absolute.  What lies below it cannot be told from a rank variance of zero:
    :func:`gwinferno_amd.postprocess.catalog_rank_correlation_check` divides by nothing smaller."""
    eps = 2.0**-52
    a = (2.0 + (n_terms + 8.5) + 1.0) if pooled else 2.0        # u: exp on either side; S (n + 8 units and fsum's half); the division
    p = a + 0.5 * (18 + n_order_tiles + 1)                      # an entry of P, relative: the scan's depth, the offsets, the statement's rounding
    e_d = 2.0 * p + 2.0                                         # d, absolute
    depth = 3 + 6 + 3 + n_sample_tiles                          # lane, butterfly, waves, tiles
    return 1.01 * eps * (0.25 * (a + 2.0) + e_d + 0.125 * (depth + 1) + 0.25 * (a + 0.5 * (depth + 1) + 1.0))


MAX_MOMENT_COLUMNS = 8  # columns of gwi_point_moments (gwi_moment.h: kMaxCols)


def moments_segment(w, x):
    """``(mean (C,), cov (C, C), alive)`` of ONE segment with the weights ``w (n,)`` of :func:`draw_weights` and the values ``x (C, n)``,
    in two passes: ``S = fsum w``, ``m_c = fsum_i (w_i x_ci) / S`` and, centred on those means, ``V_cd = fsum_i ((w_i (x_ci - m_c))
    (x_di - m_d)) / S`` -- every product rounded on its own, every sum exact and rounded once (``math.fsum``).  NaN and ``alive =
    False`` where ``S`` is 0 or not finite.  A segment with one live sample has ``w = 1`` and ``S = 1``: the mean is the sample and the
    covariance exactly 0."""
    w, x = np.asarray(w, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64)
    n_cols = x.shape[0]
    mean, cov = np.full(n_cols, np.nan), np.full((n_cols, n_cols), np.nan)
    total = math.fsum(w.tolist())
    if not (total > 0.0 and np.isfinite(total)):
        return mean, cov, False
    live = w > 0.0
    w, x = w[live], x[:, live]
    for c in range(n_cols):
        mean[c] = math.fsum((w * x[c]).tolist()) / total
    d = x - mean[:, None]
    for c in range(n_cols):
        wd = w * d[c]
        for e in range(c, n_cols):
            cov[c, e] = cov[e, c] = math.fsum((wd * d[e]).tolist()) / total
    return mean, cov, True


def point_moments_reference(logw_pe, logw_inj, x_pe, x_inj, pe_mask=None, inj_mask=None):
    """One hyper-parameter point of ``gwi_point_moments``: ``logw_pe (n_ev, n_pe)``, ``logw_inj (n_inj,)``, the values
    ``x_pe (C, n_ev, n_pe)`` and ``x_inj (C, n_inj)`` (``None``: the set has no columns) and the masks of ``gwi_set_draw_mask`` (or
    None) -> ``(mean (n_ev + 1, C), cov (n_ev + 1, C, C), dead (n_ev + 1,) int32)``, the injection set last: per segment
    :func:`moments_segment` on the weights of :func:`draw_weights`.  NaN for a segment without weight, which ``dead`` flags, and for a
    set without columns."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_pe = logw_pe.shape
    if x_pe is None and x_inj is None:
        raise ValueError("x_pe and x_inj are both None")
    n_cols = (x_pe if x_pe is not None else x_inj).shape[0]
    if not 1 <= n_cols <= MAX_MOMENT_COLUMNS:
        raise ValueError(f"{n_cols} columns: between 1 and {MAX_MOMENT_COLUMNS}")
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    mean, cov, dead = np.full((n_ev + 1, n_cols), np.nan), np.full((n_ev + 1, n_cols, n_cols), np.nan), np.zeros(n_ev + 1, dtype=np.int32)
    for seg in range(n_ev + 1):
        w = draw_weights(logw_pe[seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else draw_weights(logw_inj, inj_mask)
        x = (None if x_pe is None else np.asarray(x_pe)[:, seg]) if seg < n_ev else x_inj
        total = math.fsum(w.tolist())
        dead[seg] = 0 if total > 0.0 and np.isfinite(total) else 1
        if x is not None and not dead[seg]:
            mean[seg], cov[seg], _ = moments_segment(w, x)
    return mean, cov, dead


MAX_CONDITIONAL_PAIRS = 8    # pairs of gwi_point_conditionals (gwi_cond.h: kMaxPairs)
MAX_CONDITIONAL_ITEMS = 512  # ... and n_pairs n_bins (gwi_cond.h: kMaxItems)


def conditionals_segment(w, code, y, n_bins):
    """``(out (3, B), alive)`` of ONE segment and ONE pair with the weights ``w (n,)`` of :func:`draw_weights`, the bin codes ``code (n,)``
    of the conditioning quantity and the values ``y (n,)``, in two passes: ``S = fsum w``; per bin ``b``, over the samples coded ``b``,
    ``W_b = fsum w_i``, ``a_b = W_b / S``, ``m_b = fsum (w_i y_i) / W_b`` and, centred on that mean, ``v_b = fsum ((w_i (y_i - m_b))
    (y_i - m_b)) / W_b`` -- every product rounded on its own, every sum exact and rounded once (``math.fsum``).  A sample coded
    :data:`OUTSIDE_BIN` counts in ``S`` and in no bin.  A bin with ``W_b = 0`` gives ``a_b = 0`` and NaN for the other two.  All NaN and
    ``alive = False`` where ``S`` is 0 or not finite."""
    w, code, y = np.asarray(w, dtype=np.float64).ravel(), np.asarray(code).ravel().astype(np.int64), np.asarray(y, dtype=np.float64).ravel()
    out = np.full((3, int(n_bins)), np.nan)
    total = math.fsum(w.tolist())
    if not (total > 0.0 and np.isfinite(total)):
        return out, False
    live = w > 0.0
    w, code, y = w[live], code[live], y[live]
    for b in range(int(n_bins)):
        sel = code == b
        wb, yb = w[sel], y[sel]
        w_bin = math.fsum(wb.tolist())
        out[0, b] = w_bin / total
        if w_bin > 0.0:
            out[1, b] = math.fsum((wb * yb).tolist()) / w_bin
            d = yb - out[1, b]
            out[2, b] = math.fsum(((wb * d) * d).tolist()) / w_bin
    return out, True


def point_conditionals_reference(logw_pe, logw_inj, codes_pe, codes_inj, x_pe, x_inj, pairs, n_bins, pe_mask=None, inj_mask=None):
    """One hyper-parameter point of ``gwi_point_conditionals``: ``logw_pe (n_ev, n_pe)``, ``logw_inj (n_inj,)``, the bin codes
    ``codes_pe (Cx, n_ev, n_pe)`` and ``codes_inj (Cx, n_inj)`` of ``gwi_set_histogram_bins``, the values ``x_pe (Cy, n_ev, n_pe)`` and
    ``x_inj (Cy, n_inj)`` of ``gwi_set_kde_columns`` (``None``: the set has none), ``pairs (R, 2)`` of ``(cx, cy)`` and the masks of
    ``gwi_set_draw_mask`` (or None) -> ``(out (n_ev + 1, R, 3, B), dead (n_ev + 1,) int32)``, the injection set last: per segment and
    pair :func:`conditionals_segment` on the weights of :func:`draw_weights` -- share, conditional mean, conditional variance per bin.
    NaN for a segment without weight, which ``dead`` flags, and for a set that lacks codes or values."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_pe = logw_pe.shape
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_bins = int(n_bins)
    if not 1 <= pairs.shape[0] <= MAX_CONDITIONAL_PAIRS:
        raise ValueError(f"{pairs.shape[0]} pairs: between 1 and {MAX_CONDITIONAL_PAIRS}")
    if n_bins < 1 or pairs.shape[0] * n_bins > MAX_CONDITIONAL_ITEMS:
        raise ValueError(f"n_pairs n_bins = {pairs.shape[0] * n_bins}: between 1 and {MAX_CONDITIONAL_ITEMS}")
    if codes_pe is None and codes_inj is None:
        raise ValueError("codes_pe and codes_inj are both None")
    if x_pe is None and x_inj is None:
        raise ValueError("x_pe and x_inj are both None")
    with_pe, with_inj = codes_pe is not None and x_pe is not None, codes_inj is not None and x_inj is not None
    if not with_pe and not with_inj:
        raise ValueError("no sample set has both codes and values")
    n_x, n_y = (codes_pe if codes_pe is not None else codes_inj).shape[0], (x_pe if x_pe is not None else x_inj).shape[0]
    if np.any(pairs < 0) or np.any(pairs[:, 0] >= n_x) or np.any(pairs[:, 1] >= n_y):
        raise ValueError(f"a pair is (bin column below {n_x}, value column below {n_y})")
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    out, dead = np.full((n_ev + 1, pairs.shape[0], 3, n_bins), np.nan), np.zeros(n_ev + 1, dtype=np.int32)
    for seg in range(n_ev + 1):
        w = draw_weights(logw_pe[seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else draw_weights(logw_inj, inj_mask)
        total = math.fsum(w.tolist())
        dead[seg] = 0 if total > 0.0 and np.isfinite(total) else 1
        if dead[seg] or not (with_pe if seg < n_ev else with_inj):
            continue
        for r, (cx, cy) in enumerate(pairs):
            code, y = (np.asarray(codes_pe)[cx, seg], np.asarray(x_pe)[cy, seg]) if seg < n_ev else (np.asarray(codes_inj)[cx], np.asarray(x_inj)[cy])
            out[seg, r], _ = conditionals_segment(w, code, y, n_bins)
    return out, dead


MAX_HIST2D_BINS = 64   # bins per axis of gwi_point_histograms2d (gwi_hist2d.h: kMaxBins)
MAX_HIST2D_PAIRS = 8   # pairs of one call (gwi_hist2d.h: kMaxPairs)


def joint_table_segment(w, code_x, code_y, n_bins):
    """ONE segment's joint table ``(B, B)`` for the weights ``w`` of :func:`draw_weights`: cell ``[bx, by]`` = (sum of ``w_i`` over the
    samples coded ``bx`` and ``by``) / (sum of ``w_i`` over the segment).  A sample coded :data:`OUTSIDE_BIN` (or no bin) in either
    column is in no cell but counts in the total.  ``None`` when the total is 0 or not finite."""
    total = w.sum()
    if not (total > 0.0 and np.isfinite(total)):
        return None
    cx, cy = np.asarray(code_x).ravel().astype(np.int64), np.asarray(code_y).ravel().astype(np.int64)
    inside = (cx < n_bins) & (cy < n_bins)
    table = np.zeros(n_bins * n_bins)
    np.add.at(table, cx[inside] * n_bins + cy[inside], w[inside])
    return (table / total).reshape(n_bins, n_bins)


def point_histograms2d_reference(logw_pe, logw_inj, pe_mask, inj_mask, pe_bins, inj_bins, n_bins, pairs, v=None):
    """One hyper-parameter point of ``gwi_point_histograms2d``: the arguments of :func:`weighted_histograms_reference` and
    ``pairs (R, 2)`` of bin columns ``(cx, cy)`` -> a dict.  ``hist_pe (n_ev, R, B, B)`` and ``hist_inj (R, B, B)``: what the point adds to
    the running sums, ``v`` times :func:`joint_table_segment` per segment and pair (``None`` for a set whose bins are ``None``; zeros for
    a dead segment).  ``obs (R, B, B)``: (the sum of the live events' tables, in event order) / their number; ``pred (R, B, B)``: the
    injection set's table; NaN without a live event / for a dead injection set / for a set without bins.  ``live (2,) int32`` = (live
    events, 1 if the injection set is live else 0); ``n_dead (n_ev + 1,) int32``: 1 for every segment without weight of a set that has
    bins; ``vsum (n_ev + 1,)``: ``v`` for every live segment of such a set (``None`` without ``v``).  ``v (n_ev + 1,)`` is the point's row
    of linear weights in ``[0, 1]``: a segment whose ``v`` is 0 adds nothing and is not counted in ``n_dead``; ``obs``, ``pred`` and
    ``live`` do not depend on ``v``."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_bins = logw_pe.shape[0], int(n_bins)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if not 1 <= pairs.shape[0] <= MAX_HIST2D_PAIRS:
        raise ValueError(f"{pairs.shape[0]} pairs: between 1 and {MAX_HIST2D_PAIRS}")
    if not 1 <= n_bins <= MAX_HIST2D_BINS:
        raise ValueError(f"n_bins = {n_bins}: between 1 and {MAX_HIST2D_BINS}")
    if pe_bins is None and inj_bins is None:
        raise ValueError("pe_bins and inj_bins are both None")
    n_cols = np.asarray(pe_bins if pe_bins is not None else inj_bins).shape[0]
    if np.any(pairs < 0) or np.any(pairs >= n_cols):
        raise ValueError(f"a pair is two bin columns below {n_cols}")
    if v is not None:
        v = point_weights_array(np.asarray(v, dtype=np.float64).reshape(1, -1), 1, n_ev + 1)[0]
    n_pairs = pairs.shape[0]
    n_dead, vsum, live = np.zeros(n_ev + 1, dtype=np.int32), np.zeros(n_ev + 1), np.zeros(2, dtype=np.int32)
    obs, pred = np.full((n_pairs, n_bins, n_bins), np.nan), np.full((n_pairs, n_bins, n_bins), np.nan)
    hist_pe = hist_inj = None

    def segment(seg, logw, mask, codes):
        """``(tables (R, B, B) or None when dead, what the segment adds to the running sums)``"""
        w = draw_weights(logw, mask)
        tables = [joint_table_segment(w, codes[cx], codes[cy], n_bins) for cx, cy in pairs]
        alive = tables[0] is not None
        pv = 1.0 if v is None else v[seg]
        add = np.zeros((n_pairs, n_bins, n_bins))
        if pv != 0.0:
            if not alive:
                n_dead[seg] = 1
            else:
                vsum[seg] = pv
                add = np.stack(tables) if v is None else pv * np.stack(tables)
        return (np.stack(tables) if alive else None), add

    if pe_bins is not None:
        pe_bins = np.asarray(pe_bins)
        pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(logw_pe.shape)
        hist_pe = np.zeros((n_ev, n_pairs, n_bins, n_bins))
        total = np.zeros((n_pairs, n_bins, n_bins))
        for ev in range(n_ev):
            tables, hist_pe[ev] = segment(ev, logw_pe[ev], None if pe_mask is None else pe_mask[ev], pe_bins[:, ev])
            if tables is not None:
                total += tables
                live[0] += 1
        if live[0]:
            obs = total / float(live[0])
    if inj_bins is not None:
        tables, hist_inj = segment(n_ev, logw_inj, inj_mask, np.asarray(inj_bins))
        if tables is not None:
            pred, live[1] = tables, 1
    return {"hist_pe": hist_pe, "hist_inj": hist_inj, "obs": obs, "pred": pred, "live": live, "n_dead": n_dead, "vsum": vsum if v is not None else None}


def joint_table_summaries(p):
    """Summaries of joint tables ``p (..., B, B)`` of non-negative shares whose in-range total ``t = sum p`` may fall short of 1 (the
    rest lies outside the edges): a dict with the marginals ``px (..., B) = sum_y p / t`` and ``py (..., B) = sum_x p / t``, the plug-in
    mutual information ``mi (...)`` = ``sum over the cells with p > 0 of (p / t) log((p / t) / (px py))`` in nats, ``total (...)`` = ``t``
    and ``outside (...)`` = ``1 - t``.  A table with ``t = 0`` (or a NaN in it) gives NaN marginals and ``mi``.

    The plug-in estimate is biased UPWARD by roughly ``(cells - 1) / (2 n_eff)`` with ``cells`` the occupied cells and ``n_eff`` the
    effective number of samples behind the table; no correction is applied."""
    p = np.asarray(p, dtype=np.float64)
    if p.ndim < 2 or p.shape[-1] != p.shape[-2]:
        raise ValueError(f"p has shape {p.shape}; expected (..., B, B)")
    t = p.sum(axis=(-2, -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        good = t > 0.0
        scale = np.where(good, t, np.nan)
        q = p / scale[..., None, None]
        px, py = q.sum(axis=-1), q.sum(axis=-2)
        has = q > 0.0
        ratio = np.where(has, q / (px[..., :, None] * py[..., None, :]), 1.0)
        mi = np.where(good, (np.where(has, q, 0.0) * np.log(ratio)).sum(axis=(-2, -1)), np.nan)
    return {"px": px, "py": py, "mi": mi, "total": t, "outside": 1.0 - t}


def pareto_smooth(log_ratios):
    """Pareto-smoothed importance sampling on the point axis (Vehtari, Simpson, Gelman, Yao & Gabry, *Pareto smoothed importance
    sampling*; the fit is Zhang & Stephens 2009): ``log_ratios (K, n_seg)`` -> ``(log_weights (K, n_seg), khat (n_seg,))``.  Per column:
    the maximum is subtracted; the tail is the ``M = min(floor(K / 5), ceil(3 sqrt K))`` largest entries and ``cutoff`` the largest
    below it; a generalised Pareto distribution is fitted to ``exp(tail) - exp(cutoff)`` (the profile-likelihood posterior mean of
    Zhang & Stephens over ``30 + floor(sqrt M)`` points, then ``khat = (M k + 5) / (M + 10)``, the weakly informative pull towards
    0.5); the tail's values are replaced, in ascending order, by ``log(exp(cutoff) + sigma expm1(-khat log1p(-p_i)) / khat)`` with
    ``p_i = (i - 1/2) / M`` and truncated at the raw maximum, 0 after the shift.  Every entry outside the tail keeps the bits of the
    shifted input, and the order of the tail's values does not decrease.  With ``M < 5`` or a constant tail nothing is smoothed and
    ``khat`` is inf.  Every entry must be finite.  ``khat`` below 0.5 is good, up to 0.7 usable, above it the estimate is unreliable;
    the value is reported and nothing is refitted."""
    lr = np.array(log_ratios, dtype=np.float64)
    if lr.ndim != 2 or lr.shape[0] < 1:
        raise ValueError("log_ratios is (K, n_seg) with K >= 1")
    if not np.all(np.isfinite(lr)):
        raise ValueError("log_ratios must be finite")
    k_pts, n_seg = lr.shape
    khat = np.full(n_seg, np.inf)
    m_tail = min(k_pts // 5, int(math.ceil(3.0 * math.sqrt(k_pts))))
    for s in range(n_seg):
        col = lr[:, s] - lr[:, s].max()
        lr[:, s] = col
        if m_tail < 5:
            continue
        order = np.argsort(col, kind="stable")
        tail_at = order[k_pts - m_tail :]  # ascending
        cutoff = col[order[k_pts - m_tail - 1]]
        kh, new = _smooth_shifted_tail(col[tail_at], cutoff)
        if new is None:
            continue
        khat[s] = kh
        lr[tail_at, s] = new
    return lr, khat


def _smooth_shifted_tail(tail, cutoff):
    """The fit and the replacement of :func:`pareto_smooth` for one ascending tail ``(M,)`` and its cut-off, both already shifted so
    that the largest value the tail may take is 0: ``(khat, new (M,))``, or ``(inf, None)`` where nothing is smoothed (``M < 5``, a
    constant tail, or a lowest quarter that ties with the cut-off)."""
    m_tail = tail.size
    if m_tail < 5 or not tail[-1] > tail[0]:
        return np.inf, None
    x = np.exp(tail) - math.exp(cutoff)
    if not x[int(m_tail / 4.0 + 0.5) - 1] > 0.0:  # (the lowest quarter of the tail ties with the cutoff: the fit has no scale)
        return np.inf, None
    k_fit, sigma = _gpd_fit(x)
    kh = (m_tail * k_fit + 5.0) / (m_tail + 10.0)
    p = (np.arange(1, m_tail + 1, dtype=np.float64) - 0.5) / m_tail
    with np.errstate(divide="ignore", invalid="ignore"):
        q = sigma * np.expm1(-kh * np.log1p(-p)) / kh if kh != 0.0 else -sigma * np.log1p(-p)
        new = np.log(math.exp(cutoff) + q)
    return kh, np.minimum(new, 0.0)


def _gpd_fit(x):
    """Zhang & Stephens' estimate ``(k, sigma)`` of the generalised Pareto distribution for the ascending positive sample ``x (n,)``,
    without the regularisation of ``k``."""
    n = x.size
    m = 30 + int(math.sqrt(n))
    j = np.arange(1, m + 1, dtype=np.float64)
    b = 1.0 - np.sqrt(m / (j - 0.5))
    b = b / (3.0 * x[int(n / 4.0 + 0.5) - 1]) + 1.0 / x[n - 1]
    k = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
    big_l = n * (np.log(-b / k) - k - 1.0)
    omega = 1.0 / np.sum(np.exp(big_l[None, :] - big_l[:, None]), axis=1)
    b_hat = float(np.sum(b * omega))
    k_hat = float(np.mean(np.log1p(-b_hat * x)))
    return k_hat, -k_hat / b_hat


def pareto_smoothed_summary(log_l_event):
    """:func:`leave_one_out_summary` with the leave-one-out weights of every event Pareto-smoothed on the point axis
    (:func:`pareto_smooth` of ``-l_ke`` over the points at which it is finite): the same dictionary with ``point_weights`` the smoothed
    weights, each event's largest exactly 1 and the injection column all ones; ``pareto_k (n_ev,)`` (inf where nothing was smoothed,
    NaN for an event without a finite point); ``elpd_loo = log(sum_k v_k exp(l_ke) / sum_k v_k)``, the self-normalised estimate,
    which is ``-log mean_k exp(-l_ke)`` when nothing is smoothed; and ``neff_points`` of the smoothed weights.  ``lpd`` and ``n_bad``
    are unchanged."""
    out = dict(leave_one_out_summary(log_l_event))
    ell = out["log_l_event"]
    k, n_ev = ell.shape
    good = np.isfinite(ell)
    v = np.ones((k, n_ev + 1))
    elpd, neff, khat = np.full(n_ev, np.nan), np.zeros(n_ev), np.full(n_ev, np.nan)
    for e in range(n_ev):
        v[:, e] = 0.0
        rows = np.nonzero(good[:, e])[0]
        if rows.size == 0:
            continue
        col = ell[rows, e]
        lw, kh = pareto_smooth(-col[:, None])
        lw = lw[:, 0] - lw[:, 0].max()  # (the largest becomes exactly exp(0) = 1)
        ve = np.exp(lw)
        v[rows, e] = ve
        khat[e] = kh[0]
        s1 = math.fsum(ve.tolist())
        hi = col.max()
        elpd[e] = hi + math.log(math.fsum((ve * np.exp(col - hi)).tolist()) / s1)
        neff[e] = s1 * s1 / math.fsum((ve * ve).tolist())
    out.update(point_weights=v, elpd_loo=elpd, neff_points=neff, pareto_k=khat)
    return out


MAX_TAIL = 4096  # the longest tail of gwi_point_tails (gwi_tail.h: kMaxTail)


def psis_tail_size(n):
    """The tail size of Pareto smoothed importance sampling for ``n`` samples: ``min(floor(n / 5), ceil(3 sqrt(n)))``, as
    :func:`pareto_smooth` takes it."""
    n = int(n)
    return min(n // 5, int(math.ceil(3.0 * math.sqrt(n))))


def tails_segment(logw, mask, m):
    """``(tail (m,), stats (4,), counts (4,) int32)`` of ONE segment of ``gwi_point_tails``.  The live values are the finite
    ``logw`` the mask leaves.  ``tail``: the ``m`` largest of them in ascending order (``np.sort``), ``-inf`` in front where fewer are
    live.  With ``v* = tail[0]``: ``counts = (n_live, #(l > v*), #(l == v*), dead)`` and ``stats = (max, S, body, below_max)``: the
    largest live value, ``S = fsum w`` of the shifted weights of :func:`draw_weights`, ``body = fsum`` of those of the values below
    ``v*`` and the largest live value below ``v*`` (``-inf``: none).  A segment whose ``S`` is 0 or not finite is dead: an all ``-inf``
    tail, zero counts, NaN ``body``."""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    live = np.isfinite(lw)
    if mask is not None:
        live &= np.asarray(mask).ravel().astype(bool)
    m = int(m)
    w = draw_weights(lw, mask)
    total = math.fsum(w.tolist())
    vals = lw[live]
    top = float(vals.max()) if vals.size else -np.inf
    tail = np.full(m, -np.inf)
    if not (total > 0.0 and np.isfinite(total)):
        return tail, np.array([top, total, np.nan, -np.inf]), np.array([0, 0, 0, 1], dtype=np.int32)
    take = min(m, vals.size)
    tail[m - take:] = np.sort(vals)[vals.size - take:]
    v_star = tail[0]
    below = live & (lw < v_star)
    stats = np.array([top, total, math.fsum(w[below].tolist()), float(lw[below].max()) if below.any() else -np.inf])
    return tail, stats, np.array([vals.size, np.count_nonzero(vals > v_star), np.count_nonzero(vals == v_star), 0], dtype=np.int32)


def point_tails_reference(logw_pe, logw_inj, pe_mask, inj_mask, m_pe, m_inj):
    """One hyper-parameter point of ``gwi_point_tails``: ``logw_pe (n_ev, n_pe)``, ``logw_inj (n_inj,)`` -- what
    ``Engine.log_weights`` returns --, the masks of ``gwi_set_draw_mask`` (or None) and the two tail sizes -> ``(tail_pe (n_ev, m_pe),
    tail_inj (m_inj,), stats (n_ev + 1, 4), counts (n_ev + 1, 4) int32)``, the injection set last: per segment :func:`tails_segment`."""
    logw_pe = np.asarray(logw_pe, dtype=np.float64)
    n_ev, n_pe = logw_pe.shape
    m_pe, m_inj = int(m_pe), int(m_inj)
    if not (1 <= m_pe <= MAX_TAIL and 1 <= m_inj <= MAX_TAIL) or m_pe >= n_pe or m_inj >= np.asarray(logw_inj).size:
        raise ValueError(f"a tail size is in 1 ... {MAX_TAIL} and below its segment's length")
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    tail_pe, stats, counts = np.empty((n_ev, m_pe)), np.empty((n_ev + 1, 4)), np.empty((n_ev + 1, 4), dtype=np.int32)
    for ev in range(n_ev):
        tail_pe[ev], stats[ev], counts[ev] = tails_segment(logw_pe[ev], None if pe_mask is None else pe_mask[ev], m_pe)
    tail_inj, stats[n_ev], counts[n_ev] = tails_segment(logw_inj, inj_mask, m_inj)
    return tail_pe, tail_inj, stats, counts


def tail_cutoff_and_rest(tail, stats, counts):
    """What the host derives from ``gwi_point_tails``' rows, for any leading shape: ``tail (..., m)``, ``stats (..., 4)``, ``counts (...,
    4)`` -> ``(cutoff (...), rest (...))``.  ``cutoff`` is the ``(m + 1)``-th largest live value: ``v* = tail[..., 0]`` where ``n_gt +
    n_eq > m`` (ties of ``v*`` remain outside the tail), else ``below_max``.  ``rest`` is the sum of ``exp(l - max)`` over everything
    outside the tail, ``body + (n_gt + n_eq - m) exp(v* - max)``: nothing is subtracted.  NaN ``rest`` for a dead segment."""
    tail, stats, counts = np.asarray(tail, dtype=np.float64), np.asarray(stats, dtype=np.float64), np.asarray(counts)
    m, v_star = tail.shape[-1], tail[..., 0]
    extra = np.maximum(counts[..., 1].astype(np.int64) + counts[..., 2] - m, 0)
    with np.errstate(invalid="ignore"):
        ties = np.where(extra > 0, extra * np.exp(v_star - stats[..., 0]), 0.0)
    return np.where(extra > 0, v_star, stats[..., 3]), stats[..., 2] + ties


def pareto_tail_fit(tail, cutoff, top):
    """The Pareto fit of ONE ascending tail ``(m,)`` of log-weights with its cut-off (the largest value outside the tail) and the value
    ``top`` to shift by (the segment's maximum): ``(khat, smoothed (m,))`` under exactly :func:`pareto_smooth`'s conventions -- the
    generalised Pareto distribution fitted to ``exp(tail - top) - exp(cutoff - top)``, the regularised ``khat``, the quantile
    replacement truncated at 0 -- with ``smoothed`` RELATIVE TO ``top``, as ``pareto_smooth``'s output is relative to the column's
    maximum: for a column's own tail, cut-off and maximum the bits are that function's.  ``khat`` is inf and ``smoothed = tail - top``
    when ``m < 5``, the tail is constant or its lowest quarter ties with the cut-off."""
    tail = np.asarray(tail, dtype=np.float64).ravel()
    shifted = tail - float(top)
    kh, new = _smooth_shifted_tail(shifted, float(cutoff) - float(top))
    return float(kh), shifted if new is None else new


# ---- bootstrap replicates of the inner importance sums (gwi_boot.h) ----------------------------------------------------------
BOOTSTRAP_TAG = 0x424F4F54  # counter word 3 of the bootstrap stream (gwi_boot.h: kTag, "BOOT")
MAX_BOOTSTRAP_REPLICATES = 1024    # replicates of one gwi_point_bootstrap call (gwi_boot.h: kMaxReplicates)
MAX_BOOTSTRAP_REPLICATE = 1 << 20  # first_replicate + n_replicates of gwi_set_bootstrap (gwi_boot.h: kMaxReplicate)
# floor(2^32 F(j)), F the Poisson(1) CDF, j = 0 ... 12 (gwi_boot.h: kPoisson1): the table ends with the largest word, which no later
# entry could exceed.  The count of a 32-bit word is the number of entries that are <= it
POISSON1_THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
                       4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295)


def _replicate_indices(replicates):
    """``replicates`` -- a number B (the replicates 0 ... B - 1) or the replicate numbers themselves -- as an int64 array."""
    if np.ndim(replicates) == 0:
        reps = np.arange(int(replicates), dtype=np.int64)
    else:
        reps = np.asarray(replicates, dtype=np.int64).ravel()
    if reps.size < 1 or reps.min() < 0 or reps.max() >= MAX_BOOTSTRAP_REPLICATE:
        raise ValueError(f"replicates are at least one number in 0 ... {MAX_BOOTSTRAP_REPLICATE - 1}")
    return reps


def bootstrap_counts(seed, first_index, n, replicates):
    """The Poisson(1) counts ``(n, B)`` int64 of the samples with the global indices ``first_index ... first_index + n`` in the
    replicates ``replicates`` (a number B: 0 ... B - 1; or the replicate numbers): replicate ``b`` takes word ``b % 4`` of the
    Philox4x32-10 block with the key ``(seed low, seed high)`` and the counter ``(index low, index high, b // 4, BOOTSTRAP_TAG)``, and the
    count is the number of entries of ``POISSON1_THRESHOLDS`` that are ``<=`` the word.  A pure function of (seed, index, replicate): any
    split of the indices or of the replicates gives the same numbers.  PE sample ``j`` of event ``e`` has the index ``e n_pe + j``,
    injection ``j`` the index ``n_ev n_pe + j``."""
    from .spin_priors import philox4x32_10

    m64 = 2**64 - 1
    seed, first_index, n = int(seed) & m64, int(first_index) & m64, int(n)
    reps = _replicate_indices(replicates)
    out = np.empty((n, reps.size), dtype=np.int64)
    if n == 0:
        return out
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    lo, hi = idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32)
    table = np.array(POISSON1_THRESHOLDS, dtype=np.uint64)
    groups, place = np.unique(reps // 4, return_inverse=True)
    step = max(1, (1 << 20) // n)  # about 2^20 blocks at a time
    for g0 in range(0, groups.size, step):
        g = groups[g0 : g0 + step].astype(np.uint64)
        words = philox4x32_10(np.repeat(lo[:, None], g.size, axis=1), np.repeat(hi[:, None], g.size, axis=1), np.repeat(g[None, :], n, axis=0),
                              np.full((n, g.size), BOOTSTRAP_TAG, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        cols = np.nonzero((place >= g0) & (place < g0 + g.size))[0]
        for word in range(4):
            sel = cols[reps[cols] % 4 == word]
            if sel.size:
                out[:, sel] = np.searchsorted(table, words[word][:, place[sel] - g0], side="right")
    return out


def bootstrap_segment(logw, mask, counts):
    """``(sums (B,), (M, S), dead, C (B,) int64)`` of ONE segment of ``gwi_point_bootstrap`` under the counts ``counts (n, B)`` of its
    samples: ``A_b = sum_i c_ib w_i`` with the ``w_i`` of :func:`draw_weights` (a plain ``np.sum`` per replicate), ``M`` the largest live
    log-weight, ``S = fsum w``, and ``C_b = sum_i c_ib`` over the unmasked samples, whether or not their weight is finite.  A segment
    whose ``S`` is 0 or not finite is dead: NaN sums."""
    lw = np.asarray(logw, dtype=np.float64).ravel()
    counts = np.asarray(counts, dtype=np.int64).reshape(lw.size, -1)
    keep = np.ones(lw.size, dtype=bool) if mask is None else np.asarray(mask).ravel().astype(bool)
    live = keep & np.isfinite(lw)
    w = draw_weights(lw, mask)
    total = math.fsum(w.tolist())
    top = float(lw[live].max()) if live.any() else -np.inf
    c_b = counts[keep].sum(axis=0)
    if not (total > 0.0 and np.isfinite(total)):
        return np.full(counts.shape[1], np.nan), (top, total), 1, c_b
    sums = np.sum(np.ascontiguousarray(counts[live].T) * w[live], axis=1)  # (a plain np.sum per replicate: each row on its own)
    return sums, (top, total), 0, c_b


def point_bootstrap_reference(log_w_pe, log_w_inj, masks, seed, replicates):
    """One hyper-parameter point of ``gwi_point_bootstrap``: ``log_w_pe (n_ev, n_pe)``, ``log_w_inj (n_inj,)`` -- what
    ``Engine.log_weights`` returns --, ``masks = (pe_mask, inj_mask)`` of ``gwi_set_draw_mask`` (or None, also for either), the seed and
    the replicates (a number B, or the replicate numbers) -> ``(sums (n_ev + 1, B), stats (n_ev + 1, 2), dead (n_ev + 1,) int32, counts
    (n_ev + 1, B) int64)``, the injection set last: per segment :func:`bootstrap_segment` under :func:`bootstrap_counts`.  It states the
    entry; it does not mirror the device's summation shape."""
    log_w_pe = np.asarray(log_w_pe, dtype=np.float64)
    log_w_inj = np.asarray(log_w_inj, dtype=np.float64).ravel()
    n_ev, n_pe = log_w_pe.shape
    pe_mask, inj_mask = (None, None) if masks is None else masks
    pe_mask = None if pe_mask is None else np.asarray(pe_mask).reshape(n_ev, n_pe)
    reps = _replicate_indices(replicates)
    sums, stats = np.empty((n_ev + 1, reps.size)), np.empty((n_ev + 1, 2))
    dead, counts = np.empty(n_ev + 1, dtype=np.int32), np.empty((n_ev + 1, reps.size), dtype=np.int64)
    for seg in range(n_ev + 1):
        lw, mk = (log_w_pe[seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else (log_w_inj, inj_mask)
        sums[seg], stats[seg], dead[seg], counts[seg] = bootstrap_segment(lw, mk, bootstrap_counts(seed, seg * n_pe, lw.size, reps))
    return sums, stats, dead, counts


def bootstrap_likelihood(sums, stats, dead, counts, n_live, total_inj, n_obs, seed):
    """The replicates of the likelihood from the raw sums of ``gwi_point_bootstrap`` / :func:`point_bootstrap_reference`, shared by the
    device route and the host route: ``sums (K, n_ev + 1, B)``, ``stats (K, n_ev + 1, 2)``, ``dead (K, n_ev + 1)``, ``counts
    (n_ev + 1, B)``, ``n_live (n_ev + 1,)`` the segments' unmasked sample counts ``n_e``, ``total_inj`` the injections made, ``n_obs``
    the events of the likelihood.  With ``logBF_e = M_e + log(S_e / n_e)`` and ``log mu = M_inj + log(S_inj / total_inj)``:

    * ``logBF_eb = logBF_e + log(A_eb / S_e) - log(C_eb / n_e)``,
    * ``log mu_b = log mu + log(A_inj,b / S_inj) - log((C_inj,b + C_miss,b) / total_inj)`` with ``C_miss,b ~ Poisson(total_inj -
      n_inj_unmasked)`` drawn here from ``np.random.Generator(np.random.Philox(seed))``, once per replicate and the same at every point:
      the injections that were not found are resampled as well,
    * ``log L_b = sum_e logBF_eb - n_obs log mu_b``.

    No cuts and no marginalised-selection term are applied.  A replicate of a dead segment, or one with ``C_eb = 0`` (possible only for
    tiny segments), is NaN and is counted, never divided.  Returns a dict: ``log_bf (K, n_ev)``, ``log_mu (K,)``, ``log_l (K,)``,
    ``log_bf_rep (K, n_ev, B)``, ``log_mu_rep (K, B)``, ``log_l_rep (K, B)``, ``c_miss (B,)``, ``n_dead`` (the (point, segment) pairs
    without weight) and ``n_empty`` (the (segment, replicate) pairs with ``C = 0``)."""
    sums, stats = np.asarray(sums, dtype=np.float64), np.asarray(stats, dtype=np.float64)
    counts, n_live = np.asarray(counts, dtype=np.int64), np.asarray(n_live, dtype=np.float64).ravel()
    is_dead = np.asarray(dead) != 0
    n_rep = sums.shape[2]
    missed = float(total_inj) - n_live[-1]
    if missed < 0.0:
        raise ValueError(f"total_inj = {total_inj} is below the {int(n_live[-1])} unmasked found injections")
    c_miss = np.random.Generator(np.random.Philox(int(seed) & (2**64 - 1))).poisson(missed, size=n_rep).astype(np.float64)
    denom = counts.astype(np.float64)
    denom[-1] += c_miss
    norm = n_live.copy()
    norm[-1] = float(total_inj)
    empty = denom <= 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        base = np.where(is_dead, np.nan, stats[..., 0] + np.log(stats[..., 1] / norm[None, :]))
        shift = np.log(sums / stats[..., 1][..., None]) - np.log(denom / norm[:, None])[None]
    rep = np.where(is_dead[..., None] | empty[None], np.nan, base[..., None] + shift)
    log_bf, log_mu = base[:, :-1], base[:, -1]
    log_bf_rep, log_mu_rep = rep[:, :-1], rep[:, -1]
    return {"log_bf": log_bf, "log_mu": log_mu, "log_l": log_bf.sum(axis=1) - float(n_obs) * log_mu, "log_bf_rep": log_bf_rep, "log_mu_rep": log_mu_rep,
            "log_l_rep": log_bf_rep.sum(axis=1) - float(n_obs) * log_mu_rep, "c_miss": c_miss, "n_dead": int(np.count_nonzero(is_dead)),
            "n_empty": int(np.count_nonzero(empty))}
