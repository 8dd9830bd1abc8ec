"""The post-processing wrappers of :class:`gwinferno_amd.engine.NativePopulationLikelihood`: per-sample log-weights, index draws,
injection resampling, weighted histograms, per-point CDFs, PIT brackets, exact PITs, moments, conditional moments, rank correlations, tails, bootstrap replicates and joint histograms, marginal weights and their
quantiles and kernel density estimates.
Host-side argument checks and array bookkeeping only -- every per-sample operation runs in gwinferno_amd/csrc (HIP, gfx950).
"""
import ctypes as C

import numpy as np

from . import _native as N


class PostprocessMixin:
    """What an engine that holds the whole catalog can do with it beside evaluating the likelihood.  The class that inherits this
    has ``lib``, ``handle``, ``_check``, ``world`` and the catalog's sizes ``n_theta``, ``n_ev``, ``n_pe``, ``n_inj``."""

    def _whole_catalog(self, what, need):
        if self.world > 1:
            raise N.NativeEngineError(f"GWI_ERR_UNSUPPORTED: {what}: this engine holds one shard of the catalog; {need} the global set")

    def _points(self, thetas, none_allowed=False):
        """``thetas`` -- one point ``(n_theta,)`` or ``(k, n_theta)`` -- as ``(k, n_theta)``; ``k = 0`` only where ``none_allowed``."""
        thetas = N.f64(thetas)
        if thetas.ndim not in (1, 2) or thetas.shape[-1] != self.n_theta or (thetas.size == 0 and not none_allowed):
            raise ValueError(f"thetas has shape {thetas.shape}; expected ({self.n_theta},) or (k, {self.n_theta})")
        return thetas.reshape(-1, self.n_theta)

    @staticmethod
    def _one_set(v, shape, name, codes=False):
        """One set's columns ``(n_cols, *shape)``: finite float64 values, or with ``codes`` integer bin codes as uint16."""
        if v is None:
            return None
        v = np.asarray(v) if codes else np.ascontiguousarray(v, dtype=np.float64)
        if v.ndim != len(shape) + 1 or v.shape[1:] != shape:
            raise ValueError(f"{name} has shape {v.shape}; expected (n_cols, {', '.join(str(s) for s in shape)})")
        if not codes:
            if not np.all(np.isfinite(v)):
                raise ValueError(f"{name} holds values that are not finite")
            return v
        if v.dtype.kind not in "iu":
            raise ValueError(f"{name} holds {v.dtype}, not integer bin codes")
        if v.size and (v.min() < 0 or v.max() > 0xFFFF):
            raise ValueError(f"{name} holds codes outside 0 ... 0xFFFF")
        return np.ascontiguousarray(v, dtype=np.uint16)

    def _two_sets(self, pe, inj, pe_name, inj_name, codes=False):
        """``(pe (n_cols, n_ev, n_pe), inj (n_cols, n_inj), n_cols)`` of the caller's columns: ``None`` leaves a set out, not both."""
        if pe is None and inj is None:
            raise ValueError(f"{pe_name} and {inj_name} are both None")
        pe, inj = self._one_set(pe, (self.n_ev, self.n_pe), pe_name, codes), self._one_set(inj, (self.n_inj,), inj_name, codes)
        if pe is not None and inj is not None and pe.shape[0] != inj.shape[0]:
            raise ValueError(f"{pe_name} holds {pe.shape[0]} columns, {inj_name} {inj.shape[0]}")
        return pe, inj, (pe if pe is not None else inj).shape[0]

    def _nothing_set(self, what, missing, entry, *args):
        """Nothing to work on: the library says so (``entry`` is called with nulls for its outputs), and where it does not, this does."""
        self._check(entry(self.handle, *args))
        raise N.NativeEngineError(f"GWI_ERR_INVALID: {what}: no {missing}")

    def _point_weights(self, point_weights, k):
        """``point_weights`` -- ``(k, n_ev + 1)``, or ``(k,)`` for one weight per point -- as the ``v[k][n_ev + 1]`` of the C ABI."""
        from .draws import point_weights_array

        return point_weights_array(point_weights, k, self.n_ev + 1)

    def log_weights(self, theta):
        """Per-sample log importance weights (diagnostic; parity with the arrays the reference's
        model function builds, tests/inference_test.py:174-175)."""
        theta = N.f64(theta)
        pe = np.zeros((self.n_ev, self.n_pe))
        inj = np.zeros(self.n_inj)
        self._check(self.lib.gwi_log_weights(self.handle, N.as_dp(theta), N.as_dp(pe), N.as_dp(inj)))
        return pe, inj

    def set_draw_mask(self, pe_mask=None, inj_mask=None):
        """Which samples :meth:`draw_indices` may draw (``gwi_set_draw_mask``): ``pe_mask (n_ev, n_pe)`` and ``inj_mask
        (n_inj,)``, non-zero = may be drawn, copied to HBM once; ``None`` = every sample.  The mass cuts of the reference's
        posterior-predictive branch (pipeline/analysis.py:326-338) belong here: :func:`gwinferno_amd.draws.mass_cut_masks`."""

        def one(m, shape, name):
            if m is None:
                return None
            m = np.asarray(m)
            if m.shape != shape:
                raise ValueError(f"{name} has shape {m.shape}, the engine's sample set {shape}")
            return np.ascontiguousarray(m != 0, dtype=np.uint8)

        pe, inj = one(pe_mask, (self.n_ev, self.n_pe), "pe_mask"), one(inj_mask, (self.n_inj,), "inj_mask")
        u8 = C.POINTER(C.c_uint8)
        self._check(self.lib.gwi_set_draw_mask(self.handle, pe.ctypes.data_as(u8) if pe is not None else None, inj.ctypes.data_as(u8) if inj is not None else None))

    def draw_indices(self, thetas, u_pe=None, u_inj=None):
        """Weighted index draws on the device (``gwi_draw_indices``; semantics: :mod:`gwinferno_amd.draws`).  ``thetas``
        is one point ``(n_theta,)`` or ``(k, n_theta)``; ``u_pe (k, n_ev, n_draw_pe)`` and ``u_inj (k, n_draw_inj)`` are the
        caller's uniforms in ``[0, 1)`` (the leading axis may be left out for a single point; ``None`` = no draws from that
        set).  Returns ``(idx_pe, idx_inj)``, int32 arrays of the uniforms' shapes (``None`` where no draws were asked for):
        indices within the event / within the injection set, -1 where a segment has no sample with weight.  Only the indices
        travel back from the device.  Not available on an engine that holds a shard (``world > 1``)."""
        self._whole_catalog("draw_indices", "injection draws need")
        thetas = N.f64(thetas)
        single = thetas.ndim == 1
        thetas = thetas.reshape(-1, self.n_theta)
        k = thetas.shape[0]

        def uniforms(u, lead, name):
            if u is None:
                return None, 0
            u = N.f64(u)
            if single and u.ndim == len(lead) + 1:
                u = u[None]
            if u.ndim != len(lead) + 2 or u.shape[: len(lead) + 1] != (k, *lead):
                raise ValueError(f"{name} has shape {u.shape}; expected ({', '.join(str(v) for v in (k, *lead))}, n_draws)")
            return u, u.shape[-1]

        u_pe, n_pe_draws = uniforms(u_pe, (self.n_ev,), "u_pe")
        u_inj, n_inj_draws = uniforms(u_inj, (), "u_inj")
        idx_pe = np.full(u_pe.shape, -1, dtype=np.int32) if n_pe_draws else None
        idx_inj = np.full(u_inj.shape, -1, dtype=np.int32) if n_inj_draws else None
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.gwi_draw_indices(self.handle, N.as_dp(thetas), k, N.as_dp(u_pe) if n_pe_draws else None, n_pe_draws, N.as_dp(u_inj) if n_inj_draws else None,
                                              n_inj_draws, idx_pe.ctypes.data_as(i32) if n_pe_draws else None, idx_inj.ctypes.data_as(i32) if n_inj_draws else None))
        if u_pe is not None and idx_pe is None:
            idx_pe = np.zeros(u_pe.shape, dtype=np.int32)
        if u_inj is not None and idx_inj is None:
            idx_inj = np.zeros(u_inj.shape, dtype=np.int32)
        if single:
            idx_pe, idx_inj = (None if idx_pe is None else idx_pe[0]), (None if idx_inj is None else idx_inj[0])
        return idx_pe, idx_inj

    def resample_injections(self, theta, seed, n_request=None, first_index=0):
        """Seeded draws from the injection set in proportion to ``w = p(.|theta) / prior`` on the device
        (``gwi_resample_injections``; preprocess/selection.py:143-156; semantics:
        :func:`gwinferno_amd.draws.resample_indices_reference`).  ``n_request=None`` makes the reference's
        ``N = floor((sum w)^2 / sum w^2)`` draws, a number exactly that many; draw ``d`` is draw ``first_index + d`` of the seed's
        stream, so a request may be split over calls.  The injection mask of :meth:`set_draw_mask` applies.  Returns
        ``(idx, logw_sel, sums)``: int32 indices, the drawn samples' log-weights (``log_weights(theta)[1][idx]``) and
        ``{"log_sum_w", "log_sum_w2", "n_eff", "n_live"}``; empty arrays when no injection has weight.  Not available on an
        engine that holds a shard (``world > 1``)."""
        self._whole_catalog("resample_injections", "injection draws need")
        theta = N.f64(theta)
        if theta.shape != (self.n_theta,):
            raise ValueError(f"theta has shape {theta.shape}; expected ({self.n_theta},)")
        n_request = -1 if n_request is None else int(n_request)
        if n_request < -1:
            raise ValueError("n_request must be None or >= 0")
        room = self.n_inj if n_request < 0 else n_request
        idx, lw = np.full(max(room, 1), -1, dtype=np.int32), np.full(max(room, 1), np.nan)
        sums, made = np.zeros(4), C.c_int64(0)
        self._check(self.lib.gwi_resample_injections(self.handle, N.as_dp(theta), int(seed) & (2**64 - 1), int(first_index), n_request, C.byref(made), N.as_dp(sums),
                                                     idx.ctypes.data_as(C.POINTER(C.c_int32)), N.as_dp(lw)))
        n = int(made.value)
        return idx[:n].copy(), lw[:n].copy(), {"log_sum_w": float(sums[0]), "log_sum_w2": float(sums[1]), "n_eff": float(sums[2]), "n_live": int(sums[3])}

    def set_histogram_bins(self, pe_bins=None, inj_bins=None, n_bins=None):
        """The bin codes :meth:`weighted_histograms` sums into (``gwi_set_histogram_bins``): ``pe_bins (n_cols, n_ev, n_pe)`` and
        ``inj_bins (n_cols, n_inj)``, integers in ``[0, n_bins)`` or ``0xFFFF`` for a sample outside every bin (it still counts in
        the segment's total); ``None`` leaves that set out, not both.  ``1 <= n_cols <= 8``, ``1 <= n_bins <= 256``.  The codes
        depend on the catalog only: they are copied to HBM once, and the workspace is allocated here.  Not available on an engine
        that holds a shard (``world > 1``)."""
        self._whole_catalog("set_histogram_bins", "the injection histogram needs")
        if n_bins is None:
            raise ValueError("n_bins is needed")
        pe, inj, n_cols = self._two_sets(pe_bins, inj_bins, "pe_bins", "inj_bins", codes=True)
        u16 = C.POINTER(C.c_uint16)
        self._check(self.lib.gwi_set_histogram_bins(self.handle, n_cols, int(n_bins), pe.ctypes.data_as(u16) if pe is not None else None,
                                                    inj.ctypes.data_as(u16) if inj is not None else None))
        self._hist_shape = (n_cols, int(n_bins), pe is not None, inj is not None)

    def weighted_histograms(self, thetas, out=None, point_weights=None):
        """Weighted histograms on the device (``gwi_weighted_histograms``; semantics:
        :func:`gwinferno_amd.draws.weighted_histograms_reference`).  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.
        Returns ``(hist_pe (n_ev, n_cols, n_bins), hist_inj (n_cols, n_bins), dead (n_ev + 1,) int32)``: running SUMS over the
        points of each point's normalised histogram (``None`` for a set without bins), and per segment (the injection set last)
        the number of points at which nothing had weight -- the mean over the live points is ``hist / (K - dead)``.  ``out``
        is such a triple from an earlier call: the new points are added onto it in place, with the bits one call over all
        points would give.  Only the sums travel back from the device.  Not available on an engine that holds a shard
        (``world > 1``).

        ``point_weights`` -- ``(k, n_ev + 1)``, the injection set last, or ``(k,)`` for one weight per point -- gives every (point,
        segment) a linear weight ``v`` in ``[0, 1]`` (``gwi_weighted_histograms_weighted``): the sums are of ``v`` times the point's
        normalised histogram, and both ``out`` and the return value are the 4-tuple ``(hist_pe, hist_inj, dead, vsum)`` with ``vsum
        (n_ev + 1,)`` the sum of ``v`` over the points at which the segment had weight: the weighted mean is ``hist / vsum``.  A
        point whose ``v`` is 0 adds nothing and is not counted in ``dead``.  ``v = 1`` gives the bits of the call without weights."""
        self._whole_catalog("weighted_histograms", "the injection histogram needs")
        thetas = self._points(thetas)
        v = None if point_weights is None else self._point_weights(point_weights, thetas.shape[0])
        shape = getattr(self, "_hist_shape", None)
        i32 = C.POINTER(C.c_int32)
        if shape is None:
            self._nothing_set("weighted_histograms", "bins are set (set_histogram_bins)", self.lib.gwi_weighted_histograms, N.as_dp(thetas), thetas.shape[0], None, None, None)
        n_cols, n_bins, with_pe, with_inj = shape
        want = ((self.n_ev, n_cols, n_bins) if with_pe else None, (n_cols, n_bins) if with_inj else None, (self.n_ev + 1,)) + (((self.n_ev + 1,),) if v is not None else ())
        parts, kinds = ("hist_pe", "hist_inj", "dead", "vsum")[: len(want)], (np.float64, np.float64, np.int32, np.float64)
        if out is None:
            out = tuple(None if s is None else np.zeros(s, dtype=dt) for s, dt in zip(want, kinds))
        else:
            if len(out) != len(want):
                raise ValueError(f"out is ({', '.join(parts)})")
            for o, s, name, dt in zip(out, want, parts, kinds):
                if s is None:
                    continue
                if not isinstance(o, np.ndarray) or o.shape != s or o.dtype != dt or not o.flags.c_contiguous or not o.flags.writeable:
                    raise ValueError(f"out: {name} must be a writeable C-contiguous {np.dtype(dt).name} array of shape {s}")
        hist_pe, hist_inj, dead = out[:3]
        if v is not None:
            self._check(self.lib.gwi_weighted_histograms_weighted(self.handle, N.as_dp(thetas), thetas.shape[0], N.as_dp(v), N.as_dp(hist_pe) if with_pe else None,
                                                                  N.as_dp(hist_inj) if with_inj else None, dead.ctypes.data_as(i32), N.as_dp(out[3])))
            return (hist_pe if with_pe else None), (hist_inj if with_inj else None), dead, out[3]
        self._check(self.lib.gwi_weighted_histograms(self.handle, N.as_dp(thetas), thetas.shape[0], N.as_dp(hist_pe) if with_pe else None, N.as_dp(hist_inj) if with_inj else None,
                                                     dead.ctypes.data_as(i32)))
        return (hist_pe if with_pe else None), (hist_inj if with_inj else None), dead

    def _per_point(self, what, need, shape_attr, missing, dtypes, shapes, thetas, extra=()):
        """One per-point entry: the library's ``gwi_<what>`` fills one array per dtype, float64, int32 or int64, of the shapes ``shapes(k, shape)``,
        where ``shape`` is what the setter left in ``shape_attr``; the arrays are returned.  ``need`` and ``missing`` word the refusals;
        ``extra`` holds the entry's own arguments between ``k`` and the outputs."""
        self._whole_catalog(what, need)
        thetas = self._points(thetas)
        k, entry = thetas.shape[0], getattr(self.lib, "gwi_" + what)
        shape = getattr(self, shape_attr, None)
        if shape is None:
            self._nothing_set(what, missing, entry, N.as_dp(thetas), k, *extra, *(None for _ in dtypes))
        out = [np.empty(s, dtype=dt) for s, dt in zip(shapes(k, shape), dtypes)]
        self._check(entry(self.handle, N.as_dp(thetas), k, *extra, *(N.as_dp(o) if o.dtype == np.float64 else o.ctypes.data_as(C.POINTER(C.c_int64 if o.dtype == np.int64 else C.c_int32)) for o in out)))
        return out

    def point_cdfs(self, thetas):
        """Per-point cumulative distributions on the device (``gwi_point_cdfs``; semantics:
        :func:`gwinferno_amd.draws.point_cdfs_reference`).  The bins of :meth:`set_histogram_bins` are cumulative codes
        (:func:`gwinferno_amd.draws.cdf_codes`).  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.  Returns ``(out (k, 4,
        n_cols, n_bins), live (k, 2) int32)``: per point the CDF of the predicted detected distribution (slot 0), the mean of the live
        events' CDFs (slot 1), the sum of their ``log F`` (slot 2: the log CDF of the catalog's maximum) and of their ``log1p(-F)``
        (slot 3: the CDF of the catalog's minimum is ``1 - exp`` of it), and ``(live events, injection set live)``.  NaN where a set
        has no bins or no weight.  ``4 n_cols n_bins`` doubles come back per point; the points may be split over calls without
        changing a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        out, live = self._per_point("point_cdfs", "the injection CDF needs", "_hist_shape", "bins are set (set_histogram_bins)",
                                    (np.float64, np.int32), lambda k, s: ((k, 4, s[0], s[1]), (k, 2)), thetas)
        return out, live

    def point_pits(self, thetas):
        """Per-point brackets of every event's probability integral transform under the predicted detected distribution, on the device
        (``gwi_point_pits``; semantics: :func:`gwinferno_amd.draws.point_pits_reference`).  The bins of
        :meth:`set_histogram_bins` are cumulative codes (:func:`gwinferno_amd.draws.cdf_codes`) of BOTH sets against one grid per
        column.  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.  Returns ``(pit (k, n_ev, n_cols, 2), cdf_det (k, n_cols,
        n_bins), dead (k, n_ev + 1) int32)``: per point, event and column the lower and upper end of the bracket (NaN where the event
        or the injection set has no weight), the CDF of the predicted detected distribution (the bits of :meth:`point_cdfs` slot 0)
        and 1 for every segment without weight at the point, the injection set last.  ``2 n_ev n_cols + n_cols n_bins`` doubles come
        back per point; the points may be split over calls without changing a bit.  Not available on an engine that holds a shard
        (``world > 1``)."""
        pit, cdf_det, dead = self._per_point("point_pits", "the injection CDF needs", "_hist_shape", "bins are set (set_histogram_bins)",
                                             (np.float64, np.float64, np.int32), lambda k, s: ((k, self.n_ev, s[0], 2), (k, s[0], s[1]), (k, self.n_ev + 1)), thetas)
        return pit, cdf_det, dead

    def set_rank_columns(self, pe_values, inj_values):
        """The quantities :meth:`point_pits_exact` ranks (``gwi_set_rank_columns``): ``pe_values (n_cols, n_ev, n_pe)`` and
        ``inj_values (n_cols, n_inj)``, finite, both needed; ``1 <= n_cols <= 8``.  The injections' sort order and every PE sample's
        ranks among the injections (:func:`gwinferno_amd.draws.rank_codes`) are made here and copied to HBM once: they do not depend
        on theta.  Not available on an engine that holds a shard (``world > 1``)."""
        from .draws import MAX_RANK_COLUMNS, rank_codes

        self._whole_catalog("set_rank_columns", "the injection ranks need")
        if pe_values is None or inj_values is None:
            raise ValueError("a rank is that of a PE sample among the injections: pe_values and inj_values are both needed")
        pe, inj, n_cols = self._two_sets(pe_values, inj_values, "pe_values", "inj_values")
        if not 1 <= n_cols <= MAX_RANK_COLUMNS:
            raise ValueError(f"{n_cols} columns: between 1 and {MAX_RANK_COLUMNS} can be set")
        order, lt, le = rank_codes(pe, inj)
        i32 = C.POINTER(C.c_int32)
        self._rank_shape = None
        self._check(self.lib.gwi_set_rank_columns(self.handle, n_cols, order.ctypes.data_as(i32), lt.ctypes.data_as(i32), le.ctypes.data_as(i32)))
        self._rank_shape = (n_cols,)

    def point_pits_exact(self, thetas):
        """Every event's un-gridded probability integral transform under the predicted detected distribution, per point, on the device
        (``gwi_point_pits_exact``; semantics: :func:`gwinferno_amd.draws.point_pits_exact_reference`).  ``thetas`` is one
        point ``(n_theta,)`` or ``(k, n_theta)``.  Returns ``(pit (k, n_ev, n_cols, 2), dead (k, n_ev + 1) int32)``: per point, event
        and column of :meth:`set_rank_columns` the PIT with ``<`` and with ``<=`` in the detected CDF (they differ only through ties
        between the two sets; NaN where the event or the injection set has no weight), and 1 for every segment without weight at the
        point, the injection set last.  ``2 n_ev n_cols`` doubles come back per point; the points may be split over calls without
        changing a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        pit, dead = self._per_point("point_pits_exact", "the injection ranks need", "_rank_shape", "rank columns are set (set_rank_columns)",
                                    (np.float64, np.int32), lambda k, s: ((k, self.n_ev, s[0], 2), (k, self.n_ev + 1)), thetas)
        return pit, dead

    def point_moments(self, thetas):
        """Per-point means and full covariance of every segment, on the device (``gwi_point_moments``; semantics:
        :func:`gwinferno_amd.draws.point_moments_reference`).  The quantities are the columns of :meth:`set_kde_columns`,
        read where they lie.  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.  Returns ``(mean (k, n_ev + 1, C), cov (k,
        n_ev + 1, C, C), dead (k, n_ev + 1) int32)``, the injection set last: the weighted means ``sum_i (w_i / S) x_ci``, the
        symmetric covariance ``sum_i (w_i / S)(x_ci - m_c)(x_di - m_d)`` centred on them (filled from the upper triangle the device
        returns) and 1 for every segment without weight at the point.  NaN for a segment without weight and for a set without
        columns; exactly 0 covariance for a segment with one live sample.  ``(n_ev + 1)(C + C (C + 1) / 2)`` doubles come back per
        point; the points may be split over calls without changing a bit.  Not available on an engine that holds a shard
        (``world > 1``)."""
        raw, dead = self._per_point("point_moments", "the injection moments need", "_kde_shape", "columns are set (set_kde_columns)",
                                    (np.float64, np.int32), lambda k, s: ((k, self.n_ev + 1, s[0] + s[0] * (s[0] + 1) // 2), (k, self.n_ev + 1)), thetas)
        k, n_cols = raw.shape[0], self._kde_shape[0]
        iu = np.triu_indices(n_cols)
        cov = np.empty((k, self.n_ev + 1, n_cols, n_cols))
        cov[..., iu[0], iu[1]] = raw[..., n_cols:]
        cov[..., iu[1], iu[0]] = raw[..., n_cols:]
        return np.ascontiguousarray(raw[..., :n_cols]), cov, dead

    def point_conditionals(self, thetas, pairs):
        """Per-point conditional moments of every segment, on the device (``gwi_point_conditionals``; semantics:
        :func:`gwinferno_amd.draws.point_conditionals_reference`).  ``pairs`` is ``(R, 2)`` of ``(cx, cy)``: ``cx`` a bin column
        of :meth:`set_histogram_bins` -- the conditioning quantity -- and ``cy`` a value column of :meth:`set_kde_columns`, both read
        where they lie; ``1 <= R <= 8`` and ``R n_bins <= 512``.  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.  Returns
        ``(share (k, n_ev + 1, R, B), mean (k, n_ev + 1, R, B), var (k, n_ev + 1, R, B), dead (k, n_ev + 1) int32)``, the injection set
        last: per bin ``b`` of ``cx`` the bin's share ``W_b / S`` of the segment's weight (the bits :meth:`weighted_histograms` adds for the
        point), the weighted mean of ``cy`` among the bin's samples and their weighted variance centred on that mean, and 1 for every
        segment without weight at the point.  A bin without weight has share 0 and NaN mean and variance; NaN everywhere for a segment
        without weight and for a set that lacks bins or columns.  ``3 (n_ev + 1) R B`` doubles come back per point; the points may be
        split over calls without changing a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        from .draws import MAX_CONDITIONAL_PAIRS

        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        if not 1 <= pairs.shape[0] <= MAX_CONDITIONAL_PAIRS:
            raise ValueError(f"{pairs.shape[0]} pairs: between 1 and {MAX_CONDITIONAL_PAIRS} can be asked for in one call")
        n_pairs = pairs.shape[0]
        no_bins = getattr(self, "_hist_shape", None) is None
        raw, dead = self._per_point("point_conditionals", "the injection moments need", "_hist_shape" if no_bins else "_kde_shape",
                                    "bins are set (set_histogram_bins)" if no_bins else "columns are set (set_kde_columns)", (np.float64, np.int32),
                                    lambda k, s: ((k, self.n_ev + 1, n_pairs, 3, self._hist_shape[1]), (k, self.n_ev + 1)), thetas,
                                    extra=(n_pairs, pairs.ctypes.data_as(C.POINTER(C.c_int32))))
        return np.ascontiguousarray(raw[:, :, :, 0]), np.ascontiguousarray(raw[:, :, :, 1]), np.ascontiguousarray(raw[:, :, :, 2]), dead

    def set_rankcorr_columns(self, pe_values, inj_values):
        """The quantities :meth:`point_rank_correlations` ranks (``gwi_set_rankcorr_columns``): ``pe_values (n_cols, n_ev,
        n_pe)`` and ``inj_values (n_cols, n_inj)``, finite, both needed; ``1 <= n_cols <= 8``.  Per set -- the PE samples pooled over
        the events, the injections -- and column the members' sort order and every member's ranks within its own set
        (:func:`gwinferno_amd.draws.rankcorr_codes`) are made here and copied to HBM once: they do not depend on theta.  A second call
        replaces the columns.  Not available on an engine that holds a shard (``world > 1``)."""
        from .draws import MAX_RANKCORR_COLUMNS, rankcorr_codes

        self._whole_catalog("set_rankcorr_columns", "the rank sets need")
        if pe_values is None or inj_values is None:
            raise ValueError("the observed and the predicted correlation are compared: pe_values and inj_values are both needed")
        pe, inj, n_cols = self._two_sets(pe_values, inj_values, "pe_values", "inj_values")
        if not 1 <= n_cols <= MAX_RANKCORR_COLUMNS:
            raise ValueError(f"{n_cols} columns: between 1 and {MAX_RANKCORR_COLUMNS} can be set")
        codes = rankcorr_codes(pe.reshape(n_cols, -1)) + rankcorr_codes(inj)
        i32 = C.POINTER(C.c_int32)
        self._rankcorr_shape = None
        self._check(self.lib.gwi_set_rankcorr_columns(self.handle, n_cols, *(a.ctypes.data_as(i32) for a in codes)))
        self._rankcorr_shape = (n_cols,)

    def point_rank_correlations(self, thetas):
        """Per-point second moments of the weighted mid-ranks of the two rank sets, on the device (``gwi_point_rank_correlations``;
        semantics: :func:`gwinferno_amd.draws.point_rank_correlations_reference`).  ``thetas`` is one point ``(n_theta,)``
        or ``(k, n_theta)``.  Returns ``(total (k, 2), mean_rank (k, 2, C), cov (k, 2, C, C), dead (k, n_ev + 1) int32, dead_set (k, 2)
        int32)``, the observed set (all PE samples pooled, each event's samples sharing the weight 1) first, the detected set (the
        injections) second: the set's weight ``U``, the weighted means of the mid-ranks (0.5 up to rounding: a self-check), the
        symmetric matrix ``R_cd = sum_i (u_i / U) d_ci d_di`` of the centred mid-ranks ``d`` (filled from the upper triangle the
        device returns) -- Spearman's rho is ``R_cd / sqrt(R_cc R_dd)`` -- the segments' flags, the injection set last, and the
        two sets' (the observed set is dead when no event is live).  NaN for a dead set; ``R_cc = 0`` exactly for a column whose
        members all tie.  ``2 (1 + C + C (C + 1) / 2)`` doubles come back per point; the points may be split over calls without changing
        a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        from .draws import rankcorr_matrix

        raw, dead = self._per_point("point_rank_correlations", "the rank sets need", "_rankcorr_shape", "rank-correlation columns are set (set_rankcorr_columns)",
                                    (np.float64, np.int32), lambda k, s: ((k, 2, 1 + s[0] + s[0] * (s[0] + 1) // 2), (k, self.n_ev + 2)), thetas)
        total, mean_rank, cov = rankcorr_matrix(raw, self._rankcorr_shape[0])
        n_ev = self.n_ev
        return total, mean_rank, cov, np.ascontiguousarray(dead[:, : n_ev + 1]), np.ascontiguousarray(dead[:, [n_ev + 1, n_ev]])

    def set_tail_sizes(self, m_pe=None, m_inj=None):
        """The tail sizes of :meth:`point_tails` (``gwi_set_tail_sizes``): ``m_pe`` for every event's segment and ``m_inj`` for
        the injection set, ``1 <= m <= 4096``, ``m_pe < n_pe`` and ``m_inj < n_inj``.  ``None`` means the rule of Pareto smoothed
        importance sampling on the segment's length, ``min(floor(n / 5), ceil(3 sqrt(n)))``, capped at 4096
        (:func:`gwinferno_amd.draws.psis_tail_size`).  Nothing is uploaded; a second call replaces the sizes.  Not available on an engine
        that holds a shard (``world > 1``)."""
        from .draws import MAX_TAIL, psis_tail_size

        self._whole_catalog("set_tail_sizes", "the injection tail needs")
        m_pe = min(psis_tail_size(self.n_pe), MAX_TAIL) if m_pe is None else int(m_pe)
        m_inj = min(psis_tail_size(self.n_inj), MAX_TAIL) if m_inj is None else int(m_inj)
        self._tail_shape = None
        self._check(self.lib.gwi_set_tail_sizes(self.handle, m_pe, m_inj))
        self._tail_shape = (m_pe, m_inj)

    def point_tails(self, thetas):
        """Per-point tails of the inner importance sums, on the device (``gwi_point_tails``; semantics:
        :func:`gwinferno_amd.draws.point_tails_reference`).  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.  Returns
        ``(tail_pe (k, n_ev, m_pe), tail_inj (k, m_inj), stats (k, n_ev + 1, 4), counts (k, n_ev + 1, 4) int32)``, the injection set last:
        per segment the ``m`` largest live log-weights in ascending order with the bits :meth:`log_weights` returns (``-inf`` in front
        where fewer are live), ``stats = (max, S, body, below_max)`` and ``counts = (n_live, n_gt, n_eq, dead)`` about ``v* = tail[0]``:
        the live samples, those above and at ``v*``, the largest live value below it and ``body``, the sum of ``exp(l - max)`` over the
        values below it.  The masks of :meth:`set_draw_mask` apply.  :func:`gwinferno_amd.draws.tail_cutoff_and_rest` gives the cut-off
        of the Pareto fit and the sum outside the tail, :func:`gwinferno_amd.draws.pareto_tail_fit` the fit.  A dead segment has an all
        ``-inf`` tail, zero counts and NaN ``body``.  ``n_ev m_pe + m_inj + 4 (n_ev + 1)`` doubles come back per point; the points may be
        split over calls without changing a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        row, stats, counts = self._per_point("point_tails", "the injection tail needs", "_tail_shape", "tail sizes are set (set_tail_sizes)", (np.float64, np.float64, np.int32),
                                             lambda k, s: ((k, self.n_ev * s[0] + s[1]), (k, self.n_ev + 1, 4), (k, self.n_ev + 1, 4)), thetas)
        m_pe, m_inj = self._tail_shape
        cut = self.n_ev * m_pe
        return np.ascontiguousarray(row[:, :cut]).reshape(-1, self.n_ev, m_pe), np.ascontiguousarray(row[:, cut:]), stats, counts

    def set_bootstrap(self, seed, n_replicates, first_replicate=0):
        """The replicates of :meth:`point_bootstrap` (``gwi_set_bootstrap``): the seed of the Poisson counts
        (:func:`gwinferno_amd.draws.bootstrap_counts`), ``1 <= n_replicates <= 1024`` replicates per call and the first of them,
        ``first_replicate >= 0`` with ``first_replicate + n_replicates <= 2^20``.  Nothing is uploaded; a second call replaces the setting.
        Not available on an engine that holds a shard (``world > 1``)."""
        from .draws import MAX_BOOTSTRAP_REPLICATE, MAX_BOOTSTRAP_REPLICATES

        self._whole_catalog("set_bootstrap", "the injection replicates need")
        seed, n_replicates, first_replicate = int(seed), int(n_replicates), int(first_replicate)
        if not 1 <= n_replicates <= MAX_BOOTSTRAP_REPLICATES:
            raise ValueError(f"n_replicates = {n_replicates} is not in 1 ... {MAX_BOOTSTRAP_REPLICATES}")
        if first_replicate < 0 or first_replicate + n_replicates > MAX_BOOTSTRAP_REPLICATE:
            raise ValueError(f"first_replicate = {first_replicate} is negative or first_replicate + n_replicates exceeds {MAX_BOOTSTRAP_REPLICATE}")
        self._boot_shape = None
        self._check(self.lib.gwi_set_bootstrap(self.handle, seed & (2**64 - 1), n_replicates, first_replicate))
        self._boot_shape = (n_replicates, first_replicate)

    def point_bootstrap(self, thetas):
        """Bootstrap replicates of the inner importance sums per point, on the device (``gwi_point_bootstrap``; semantics:
        :func:`gwinferno_amd.draws.point_bootstrap_reference`).  ``thetas`` is one point ``(n_theta,)`` or ``(k, n_theta)``.
        Returns ``(sums (k, n_ev + 1, B), stats (k, n_ev + 1, 2), dead (k, n_ev + 1) int32, counts (n_ev + 1, B) int64)``, the injection set
        last: per segment and replicate ``A_b = sum_i c_ib w_i`` with ``w_i = exp(lw_i - M)`` and the Poisson(1) counts ``c_ib`` of
        :func:`gwinferno_amd.draws.bootstrap_counts` -- the same at every point --, ``stats = (M, S)`` with the bits :meth:`point_tails`
        returns, ``dead`` = 1 for a segment without weight (NaN sums), and ``C_b = sum_i c_ib`` over the segment's unmasked samples, once
        per call.  The masks of :meth:`set_draw_mask` apply.  :func:`gwinferno_amd.draws.bootstrap_likelihood` forms the replicates of the
        likelihood.  ``(n_ev + 1)(B + 2)`` doubles come back per point; the points and the replicates may be split over calls without
        changing a bit.  Not available on an engine that holds a shard (``world > 1``)."""
        sums, stats, dead, counts = self._per_point("point_bootstrap", "the injection replicates need", "_boot_shape", "replicates are set (set_bootstrap)",
                                                    (np.float64, np.float64, np.int32, np.int64),
                                                    lambda k, s: ((k, self.n_ev + 1, s[0]), (k, self.n_ev + 1, 2), (k, self.n_ev + 1), (self.n_ev + 1, s[0])), thetas)
        return sums, stats, dead, counts

    def point_histograms2d(self, thetas, pairs, point_weights=None, accumulate=True, out=None):
        """Per-point joint histograms of pairs of bin columns, on the device (``gwi_point_histograms2d``; semantics:
        :func:`gwinferno_amd.draws.point_histograms2d_reference`).  ``pairs`` is ``(R, 2)`` of ``(cx, cy)``, both bin columns of
        :meth:`set_histogram_bins`, read where they lie; ``1 <= R <= 8`` and the bins were set with ``n_bins = B <= 64``.  ``thetas`` is one
        point ``(n_theta,)`` or ``(k, n_theta)``.  Returns a dict: ``obs (k, R, B, B)``, per point the mean over the live events of the
        event's table of weight shares (cell ``[bx, by]`` = the share of the samples coded ``bx`` in ``cx`` and ``by`` in ``cy``); ``pred
        (k, R, B, B)``, the injection set's table; ``live (k, 2) int32`` = (live events, injection set live); and the running SUMS over the
        points ``hist_pe (n_ev, R, B, B)``, ``hist_inj (R, B, B)`` with ``n_dead (n_ev + 1,) int32``, the points at which the segment had
        no weight, and ``vsum (n_ev + 1,)``, as :meth:`weighted_histograms` keeps them (``None`` for a set without bins; NaN ``obs`` /
        ``pred`` for it).  ``out`` is such a dict from an earlier call with the same pairs: the new points are added onto its sums in
        place, with the bits one call over all points would give.  ``accumulate=False`` keeps no sums (``None`` in their places) and leaves
        ``obs`` / ``pred`` / ``live`` as they are.  ``point_weights`` -- ``(k, n_ev + 1)``, the injection set last, or ``(k,)`` -- gives
        every (point, segment) a linear weight ``v`` in ``[0, 1]`` in the SUMS only (``vsum`` is ``None`` without): ``v = 1`` gives the
        bits of the call without weights, ``v = 0`` adds nothing and is not counted in ``n_dead``; ``obs`` and ``pred`` do not depend on
        it.  ``2 R B B`` doubles come back per point; the points may be split over calls without changing a bit.  Not available on an
        engine that holds a shard (``world > 1``)."""
        from .draws import MAX_HIST2D_PAIRS

        self._whole_catalog("point_histograms2d", "the injection table needs")
        thetas = self._points(thetas)
        k = thetas.shape[0]
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        n_pairs = pairs.shape[0]
        if not 1 <= n_pairs <= MAX_HIST2D_PAIRS:
            raise ValueError(f"{n_pairs} pairs: between 1 and {MAX_HIST2D_PAIRS} can be asked for in one call")
        v = None if point_weights is None else self._point_weights(point_weights, k)
        i32 = C.POINTER(C.c_int32)
        shape = getattr(self, "_hist_shape", None)
        if shape is None:
            self._nothing_set("point_histograms2d", "bins are set (set_histogram_bins)", self.lib.gwi_point_histograms2d, N.as_dp(thetas), k, n_pairs, pairs.ctypes.data_as(i32),
                              None, None, None, None, None, None, None, None)
        _, n_bins, with_pe, with_inj = shape
        table = (n_pairs, n_bins, n_bins)
        want = {"hist_pe": ((self.n_ev, *table), np.float64) if with_pe else None, "hist_inj": (table, np.float64) if with_inj else None,
                "n_dead": ((self.n_ev + 1,), np.int32), "vsum": ((self.n_ev + 1,), np.float64) if v is not None else None}
        if not accumulate:
            if out is not None:
                raise ValueError("accumulate=False keeps no sums: out must be None")
            sums = dict.fromkeys(want)
        elif out is None:
            sums = {name: None if w is None else np.zeros(w[0], dtype=w[1]) for name, w in want.items()}
        else:
            sums = {}
            for name, w in want.items():
                o = out.get(name)
                if w is not None and (not isinstance(o, np.ndarray) or o.shape != w[0] or o.dtype != w[1] or not o.flags.c_contiguous or not o.flags.writeable):
                    raise ValueError(f"out: {name} must be a writeable C-contiguous {np.dtype(w[1]).name} array of shape {w[0]}")
                sums[name] = o if w is not None else None
        obs, pred, live = np.empty((k, *table)), np.empty((k, *table)), np.empty((k, 2), dtype=np.int32)
        self._check(self.lib.gwi_point_histograms2d(self.handle, N.as_dp(thetas), k, n_pairs, pairs.ctypes.data_as(i32), N.as_dp(v), N.as_dp(sums["hist_pe"]),
                                                    N.as_dp(sums["hist_inj"]), N.as_dp(obs), N.as_dp(pred), live.ctypes.data_as(i32),
                                                    None if sums["n_dead"] is None else sums["n_dead"].ctypes.data_as(i32), N.as_dp(sums["vsum"])))
        return {"obs": obs, "pred": pred, "live": live, **sums}

    def marginal_weights_reset(self):
        """Zeroes the marginal weights, the dead counts and the number of points (``gwi_marginal_weights_reset``)."""
        self._whole_catalog("marginal_weights_reset", "the injection weights need")
        self._check(self.lib.gwi_marginal_weights_reset(self.handle))

    def marginal_weights_add(self, thetas, point_weights=None):
        """Adds the points ``thetas`` -- ``(n_theta,)`` or ``(k, n_theta)``, in order -- onto the marginal weights the engine keeps in
        HBM (``gwi_marginal_weights_add``; semantics: :func:`gwinferno_amd.draws.marginal_weights_reference`): ``W_i += w_i / S`` per
        sample under the masks of :meth:`set_draw_mask`.  Nothing travels back.  The sums stay until :meth:`marginal_weights_reset`;
        changing the mask does not reset them.  Not available on an engine that holds a shard (``world > 1``).

        ``point_weights`` -- ``(k, n_ev + 1)``, the injection set last, or ``(k,)`` for one weight per point -- gives every (point,
        segment) a linear weight ``v`` in ``[0, 1]`` (``gwi_marginal_weights_add_weighted``): ``W_i += v (w_i / S)``.  A point whose
        ``v`` is 0 adds nothing and is not counted in ``dead``; ``v = 1`` gives the bits of the call without weights.  The sums of
        ``v`` and ``v v`` per segment are kept beside ``W`` (:meth:`marginal_point_weights`); calls with and without weights mix."""
        self._whole_catalog("marginal_weights_add", "the injection weights need")
        thetas = self._points(thetas, none_allowed=True)
        if point_weights is None:
            self._check(self.lib.gwi_marginal_weights_add(self.handle, N.as_dp(thetas), thetas.shape[0]))
        else:
            v = self._point_weights(point_weights, thetas.shape[0])
            self._check(self.lib.gwi_marginal_weights_add_weighted(self.handle, N.as_dp(thetas), thetas.shape[0], N.as_dp(v)))

    def marginal_point_weights(self):
        """``(vsum (n_ev + 1,), vsum2 (n_ev + 1,))``: per segment (the injection set last) the sums of the points' weights ``v`` and of
        ``v v`` over the points at which the segment had weight, since the last reset (``gwi_marginal_point_weights``); a point added
        without weights counts ``v = 1``.  ``vsum ** 2 / vsum2`` is the segment's effective number of points."""
        self._whole_catalog("marginal_point_weights", "the injection weights need")
        vsum, vsum2 = np.zeros(self.n_ev + 1), np.zeros(self.n_ev + 1)
        self._check(self.lib.gwi_marginal_point_weights(self.handle, N.as_dp(vsum), N.as_dp(vsum2)))
        return vsum, vsum2

    def marginal_weights(self, weights=True):
        """``(W_pe (n_ev, n_pe), W_inj (n_inj,), dead (n_ev + 1,) int32, n_points)``: the marginal weights read back once
        (``gwi_marginal_weights_read``; 8 bytes per sample, whatever the number of points added), per segment (the injection set
        last) the number of points at which nothing had weight, and the number of points added since the last reset.
        ``weights=False`` leaves the two arrays on the device (``None`` in their places)."""
        self._whole_catalog("marginal_weights", "the injection weights need")
        pe, inj = (np.zeros((self.n_ev, self.n_pe)), np.zeros(self.n_inj)) if weights else (None, None)
        dead, n = np.zeros(self.n_ev + 1, dtype=np.int32), C.c_int64(0)
        self._check(self.lib.gwi_marginal_weights_read(self.handle, N.as_dp(pe), N.as_dp(inj), dead.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return pe, inj, dead, int(n.value)

    def set_quantile_columns(self, pe_values=None, inj_values=None):
        """The quantities :meth:`weighted_quantiles` selects from (``gwi_set_quantile_columns``): ``pe_values (n_cols, n_ev, n_pe)``
        and ``inj_values (n_cols, n_inj)``, finite; ``None`` leaves that set out, not both; ``1 <= n_cols <= 8``.  The sort order of
        every segment is made here (``np.argsort(kind="stable")``: ties stay in sample order) and copied to HBM with the values,
        once: it does not depend on theta.  Not available on an engine that holds a shard (``world > 1``)."""
        self._whole_catalog("set_quantile_columns", "the injection quantiles need")
        pe, inj, n_cols = self._two_sets(pe_values, inj_values, "pe_values", "inj_values")
        order_pe, order_inj = (None if v is None else np.ascontiguousarray(np.argsort(v, axis=-1, kind="stable"), dtype=np.int32) for v in (pe, inj))
        i32 = C.POINTER(C.c_int32)
        self._quant_shape = None
        self._check(self.lib.gwi_set_quantile_columns(self.handle, n_cols, N.as_dp(pe) if pe is not None else None, order_pe.ctypes.data_as(i32) if pe is not None else None,
                                                      N.as_dp(inj) if inj is not None else None, order_inj.ctypes.data_as(i32) if inj is not None else None))
        self._quant_shape = (n_cols, pe is not None, inj is not None)

    def weighted_quantiles(self, levels):
        """Weighted quantiles and moments under the marginal weights, on the device (``gwi_weighted_quantiles``; semantics:
        :func:`gwinferno_amd.draws.weighted_quantiles_reference`).  ``levels`` are 1 to 32 numbers in ``[0, 1]``.  Returns ``(idx_pe
        (n_ev, n_cols, Q), idx_inj (n_cols, Q), moments_pe (n_ev, n_cols, 2), moments_inj (n_cols, 2), mass (n_ev + 1,))``: int32
        sample indices within the segment (-1 where nothing has weight; ``None`` for a set without columns), ``(sum W x, sum W
        x^2)`` and per segment ``sum W`` (the injection set last), so that ``mean = m1 / mass``.  Only these travel back."""
        self._whole_catalog("weighted_quantiles", "the injection quantiles need")
        levels = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)))
        if levels.ndim != 1:
            raise ValueError(f"levels has shape {levels.shape}; expected (n_levels,)")
        shape = getattr(self, "_quant_shape", None)
        i32 = C.POINTER(C.c_int32)
        mass = np.zeros(self.n_ev + 1)
        if shape is None:
            self._nothing_set("weighted_quantiles", "columns are set (set_quantile_columns)", self.lib.gwi_weighted_quantiles, N.as_dp(levels), levels.size, None, None, None, None,
                              N.as_dp(mass))
        n_cols, with_pe, with_inj = shape
        idx_pe, mom_pe = (np.full((self.n_ev, n_cols, levels.size), -1, dtype=np.int32), np.zeros((self.n_ev, n_cols, 2))) if with_pe else (None, None)
        idx_inj, mom_inj = (np.full((n_cols, levels.size), -1, dtype=np.int32), np.zeros((n_cols, 2))) if with_inj else (None, None)
        self._check(self.lib.gwi_weighted_quantiles(self.handle, N.as_dp(levels), levels.size, idx_pe.ctypes.data_as(i32) if with_pe else None,
                                                    idx_inj.ctypes.data_as(i32) if with_inj else None, N.as_dp(mom_pe) if with_pe else None, N.as_dp(mom_inj) if with_inj else None,
                                                    N.as_dp(mass)))
        return idx_pe, idx_inj, mom_pe, mom_inj, mass

    def set_kde_columns(self, pe_values=None, inj_values=None, bounds=None):
        """The quantities :meth:`weighted_kde` and :meth:`weighted_kde2d` smooth (``gwi_set_kde_columns``): ``pe_values (n_cols, n_ev,
        n_pe)`` and ``inj_values (n_cols, n_inj)``, finite; ``None`` leaves that set out, not both; ``1 <= n_cols <= 8``.  ``bounds
        (n_cols, 2)`` holds reflecting bounds ``(lo, hi)`` of the 1-D estimate per column, NaN (or ``None`` in a sequence) where
        there is none; ``None``: no column reflects.  The values are copied to HBM once; no sort order is needed.  Not available
        on an engine that holds a shard (``world > 1``)."""
        self._whole_catalog("set_kde_columns", "the injection densities need")
        pe, inj, n_cols = self._two_sets(pe_values, inj_values, "pe_values", "inj_values")
        if not 1 <= n_cols <= 8:
            raise ValueError(f"{n_cols} columns: between 1 and 8 can be set")
        b = np.full((n_cols, 2), np.nan)
        if bounds is not None:
            given = np.array([[np.nan if v is None else float(v) for v in row] for row in bounds], dtype=np.float64)
            if given.shape != (n_cols, 2):
                raise ValueError(f"bounds has shape {given.shape}; expected ({n_cols}, 2)")
            if np.any(np.isinf(given)) or np.any(given[:, 0] >= given[:, 1]):
                raise ValueError("a bound is finite or NaN (none), and lo lies below hi")
            b = np.ascontiguousarray(given)
        self._kde_shape = None
        self._check(self.lib.gwi_set_kde_columns(self.handle, n_cols, N.as_dp(pe) if pe is not None else None, N.as_dp(inj) if inj is not None else None, N.as_dp(b)))
        self._kde_shape = (n_cols, pe is not None, inj is not None)

    def _kde_request(self, what, rule, scale):
        from .draws import kde_rule_code

        code, scale = kde_rule_code(rule), float(scale)
        if not (scale > 0.0 and np.isfinite(scale)):
            raise ValueError("scale must be a positive finite number")
        shape = getattr(self, "_kde_shape", None)
        if shape is None:
            none, flag = np.zeros(1), np.zeros(1, dtype=np.int32)
            self._nothing_set(what, "columns are set (set_kde_columns)", self.lib.gwi_weighted_kde, N.as_dp(none), 1, code, scale, None, None, N.as_dp(none),
                              N.as_dp(np.zeros(self.n_ev + 1)), flag.ctypes.data_as(C.POINTER(C.c_int32)))
        return code, scale, shape

    def weighted_kde(self, grid, rule="scott", scale=1.0):
        """Weighted Gaussian kernel density estimates of every segment and column under the marginal weights, on the device
        (``gwi_weighted_kde``; semantics: :func:`gwinferno_amd.draws.weighted_kde_reference`).  ``grid`` is ``(n_cols, G)``
        or ``(G,)`` (the same points for every column), ``1 <= G <= 1024``, finite, in any order; ``rule`` is ``"scott"`` or
        ``"silverman"`` and ``scale`` multiplies the factor.  Returns ``(rho_pe (n_ev, n_cols, G), rho_inj (n_cols, G), bw (n_ev + 1,
        n_cols), neff (n_ev + 1,), degenerate (n_ev + 1, n_cols) int32)``: the densities (``None`` for a set without columns; NaN for
        a segment without a curve), the bandwidth ``h`` and ``n_eff`` per segment (the injection set last) and the flags."""
        self._whole_catalog("weighted_kde", "the injection densities need")
        grid = np.asarray(grid, dtype=np.float64)
        if grid.ndim not in (1, 2) or grid.shape[-1] < 1 or grid.shape[-1] > 1024:
            raise ValueError(f"grid has shape {grid.shape}; expected (G,) or (n_cols, G) with 1 <= G <= 1024")
        if not np.all(np.isfinite(grid)):
            raise ValueError("grid points must be finite")
        code, scale, (n_cols, with_pe, with_inj) = self._kde_request("weighted_kde", rule, scale)
        if grid.ndim == 2 and grid.shape[0] != n_cols:
            raise ValueError(f"grid has shape {grid.shape}; {n_cols} columns are set")
        grid = np.ascontiguousarray(np.broadcast_to(grid, (n_cols, grid.shape[-1])))
        g = grid.shape[1]
        rho_pe = np.full((self.n_ev, n_cols, g), np.nan) if with_pe else None
        rho_inj = np.full((n_cols, g), np.nan) if with_inj else None
        bw, neff, flags = np.full((self.n_ev + 1, n_cols), np.nan), np.zeros(self.n_ev + 1), np.zeros((self.n_ev + 1, n_cols), dtype=np.int32)
        self._check(self.lib.gwi_weighted_kde(self.handle, N.as_dp(grid), g, code, scale, N.as_dp(rho_pe) if with_pe else None, N.as_dp(rho_inj) if with_inj else None,
                                              N.as_dp(bw), N.as_dp(neff), flags.ctypes.data_as(C.POINTER(C.c_int32))))
        return rho_pe, rho_inj, bw, neff, flags

    def weighted_kde2d(self, pairs, gridx, gridy, rule="scott", scale=1.0):
        """Two-dimensional weighted Gaussian kernel density estimates of every segment and pair of columns, on the device
        (``gwi_weighted_kde2d``; semantics: :func:`gwinferno_amd.draws.weighted_kde2d_reference`).  ``pairs`` is ``(n_pairs, 2)``
        column indices, ``1 <= n_pairs <= 4``; ``gridx (n_pairs, n_gx)`` or ``(n_gx,)`` and ``gridy`` likewise, at most 128 points
        each: the map is evaluated on the tensor grid.  No reflection.  Returns ``(rho_pe (n_ev, n_pairs, n_gx, n_gy), rho_inj (n_pairs,
        n_gx, n_gy), cov (n_ev + 1, n_pairs, 3) = (Hxx, Hxy, Hyy), neff (n_ev + 1,), degenerate (n_ev + 1, n_pairs) int32)``."""
        self._whole_catalog("weighted_kde2d", "the injection densities need")
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        if not 1 <= pairs.shape[0] <= 4:
            raise ValueError(f"{pairs.shape[0]} pairs: between 1 and 4 can be asked for in one query")
        gridx, gridy = np.asarray(gridx, dtype=np.float64), np.asarray(gridy, dtype=np.float64)
        for name, g in (("gridx", gridx), ("gridy", gridy)):
            if g.ndim not in (1, 2) or g.shape[-1] < 1 or g.shape[-1] > 128 or (g.ndim == 2 and g.shape[0] != pairs.shape[0]):
                raise ValueError(f"{name} has shape {g.shape}; expected (n,) or (n_pairs, n) with 1 <= n <= 128")
            if not np.all(np.isfinite(g)):
                raise ValueError("grid points must be finite")
        code, scale, (n_cols, with_pe, with_inj) = self._kde_request("weighted_kde2d", rule, scale)
        n_pairs = pairs.shape[0]
        gridx = np.ascontiguousarray(np.broadcast_to(gridx, (n_pairs, gridx.shape[-1])))
        gridy = np.ascontiguousarray(np.broadcast_to(gridy, (n_pairs, gridy.shape[-1])))
        n_gx, n_gy = gridx.shape[1], gridy.shape[1]
        rho_pe = np.full((self.n_ev, n_pairs, n_gx, n_gy), np.nan) if with_pe else None
        rho_inj = np.full((n_pairs, n_gx, n_gy), np.nan) if with_inj else None
        cov, neff, flags = np.full((self.n_ev + 1, n_pairs, 3), np.nan), np.zeros(self.n_ev + 1), np.zeros((self.n_ev + 1, n_pairs), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.gwi_weighted_kde2d(self.handle, pairs.ctypes.data_as(i32), n_pairs, N.as_dp(gridx), n_gx, N.as_dp(gridy), n_gy, code, scale,
                                                N.as_dp(rho_pe) if with_pe else None, N.as_dp(rho_inj) if with_inj else None, N.as_dp(cov), N.as_dp(neff),
                                                flags.ctypes.data_as(i32)))
        return rho_pe, rho_inj, cov, neff, flags

