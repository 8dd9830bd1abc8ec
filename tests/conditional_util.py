"""TEST INFRASTRUCTURE shared by tests/test_conditional_cpu.py and tests/test_gpu_conditionals.py: the bin codes, the pair lists and the
DERIVED error bounds of the per-point conditional-moment tests (include/gwi_engine.h: gwi_point_conditionals; gwinferno_amd/csrc/
gwi_cond.h).  The catalog, the value columns (the first offset by 1e6), the masks and the points are tests/moment_util.py's,
the bound of a bin's share tests/hist_util.py's."""
import functools

import hist_util as HU
import moment_util as MU
import numpy as np

U = MU.U
TILE = MU.TILE
BIN_COLUMNS = ("mass_ratio", "redshift")  # the conditioning quantities
N_VALUE_COLUMNS = 3                       # MU.columns(3): mass_1 + 1e6 (the centring case), mass_ratio, chi_eff
# setting 5: five pooled-quantile bins and a sixth that lies wholly above the data (designed empty); two samples per segment coded outside.
# setting 256: thread b owns bin b, and two pairs make n_pairs n_bins = 512, so the item loop strides.
SETTINGS = (5, 256)
N_BINS = {5: 6, 256: 256}
EMPTY_BIN = 5
PAIRS = {5: ((0, 2), (1, 0), (0, 0)),  # the bin and value indices differ, one cx is used twice, the offset column is included
         256: ((0, 2), (1, 0))}
# by the number of distinct value columns (MU.columns(n)): three reach cond_tile_kernel<4>, eight cond_tile_kernel<8>; setting 5
WIDE_PAIRS = {3: ((0, 0), (1, 1), (0, 2)), 8: ((0, 0), (1, 1), (0, 2), (1, 3), (0, 4), (1, 5), (0, 6), (1, 7))}
OUTSIDE_PE = (7, 1100)    # per event, one sample in each tile (neither is moment_util's SINGLE_SAMPLE)
OUTSIDE_INJ = (5, 2400)
OUTSIDE = 0xFFFF


@functools.lru_cache(maxsize=None)
def edges(setting):
    """Per bin column the increasing edges: ``setting`` bins between the pooled quantiles of the PE and injection values together, the last
    data edge just above the largest value (so no sample sits on it), and at setting 5 one more edge beyond: the sixth bin holds nothing."""
    pe, inj, _ = MU.catalog()
    out = {}
    for name in BIN_COLUMNS:
        v = np.concatenate([np.asarray(pe[name], dtype=np.float64).ravel(), np.asarray(inj[name], dtype=np.float64)])
        e = np.quantile(v, np.linspace(0.0, 1.0, setting + 1))
        e[-1] = v.max() + 1e-6 * (v.max() - v.min())
        if setting == 5:
            e = np.append(e, e[-1] + (v.max() - v.min()))
        assert np.all(np.diff(e) > 0.0) and e.size == N_BINS[setting] + 1
        out[name] = e
    return out


@functools.lru_cache(maxsize=None)
def codes(setting, outside=True):
    """``(codes_pe (2, n_ev, n_pe), codes_inj (2, n_inj))`` uint16, read-only.  With ``outside`` (setting 5 only) the samples OUTSIDE_PE of
    every event and OUTSIDE_INJ of the injection set are pushed outside the edges: code 0xFFFF."""
    from gwinferno_amd.draws import digitize

    pe, inj, _ = MU.catalog()
    e = edges(setting)
    cp = np.stack([digitize(np.asarray(pe[n], dtype=np.float64), e[n]) for n in BIN_COLUMNS])
    ci = np.stack([digitize(np.asarray(inj[n], dtype=np.float64), e[n]) for n in BIN_COLUMNS])
    assert not np.any(cp == OUTSIDE) and not np.any(ci == OUTSIDE)
    if outside and setting == 5:
        cp[:, :, list(OUTSIDE_PE)] = OUTSIDE
        ci[:, list(OUTSIDE_INJ)] = OUTSIDE
    cp.setflags(write=False)
    ci.setflags(write=False)
    return cp, ci


# ---- the derived bounds -----------------------------------------------------------------------------------------------------------
def mean_units(n_bin, n_tiles):
    """DERIVED, not measured: the bound on ``|device - statement|`` of a bin's conditional mean, in units of 2^-52 of ``sum_{i in b}
    (w_i / W_b) |y_i|``, with ``n_bin`` live samples in the bin.

    * w: exp() of the same rounded argument lw - M on both sides, right to an ulp on either: 2.
    * the product w y rounds once on either side: 1.
    * the sum: on the device at most ``n_bin`` sequential additions within a tile and bin (adding the +0.0 of another bin's sample is
      exact) and ``n_tiles`` merges, each 2^-53 of the sum of the absolute terms; the statement's fsum rounds the exact sum once:
      (n_bin + n_tiles + 1) / 2.
    * W_b, the divisor: 2 for exp, (n_bin + n_tiles) / 2 for the device's additions, 1/2 for the statement's fsum; relative to W_b, so
      it moves the mean by that many units of |m_b| <= sum (w / W_b)|y|.
    * the division on either side: 1.
    S does not enter: it divides the share alone."""
    return 2 + 1 + 0.5 * (n_bin + n_tiles + 1) + (2 + 0.5 * (n_bin + n_tiles) + 0.5) + 1


def var_units(n_bin, n_tiles):
    """DERIVED, not measured: the first-order bound on ``|device - statement|`` of a bin's conditional variance, in units of 2^-52 of
    ``sum_{i in b} (w_i / W_b) |y_i - m_b|^2``.

    * w: 2, as for the mean.
    * the difference y - m rounds once on either side, 2^-53 of |y - m|, and enters twice: 2.
    * the two products (w d, then times d), each rounded on its own on either side: 2.
    * the sum, W_b and the division as for the mean."""
    return 2 + 2 + 2 + 0.5 * (n_bin + n_tiles + 1) + (2 + 0.5 * (n_bin + n_tiles) + 0.5) + 1


def share_bound(n_live):
    """hist_util.bound: slot 0 is the histogram entry's number (and has its bits), relative to the statement's value."""
    return HU.bound(n_live)


def tolerances(w, code, y, mean, n_bins, n_tiles):
    """``(tol_share, tol_mean, tol_var)``, each ``(B,)`` and ABSOLUTE, for ONE live segment and pair with the statement's weights ``w
    (n,)``, codes, values and conditional means.  1.01 covers the products of the terms (each below 1e-12).  The variance is centred on
    the side's OWN mean: the two means differ by at most ``tol_mean``, and each is within ``tol_mean`` of the mean its own weights
    define, so centring moves the variance by at most ``3 tol_mean^2`` (as moment_util.tolerances writes down): second order, and the
    only term that is not proportional to the centred scale.  NaN for a bin without weight: nothing is compared there but the NaN."""
    w, code, y = np.asarray(w, dtype=np.float64), np.asarray(code).astype(np.int64), np.asarray(y, dtype=np.float64)
    live = w > 0.0
    total = w.sum()
    tol_a, tol_m, tol_v = np.full(n_bins, np.nan), np.full(n_bins, np.nan), np.full(n_bins, np.nan)
    for b in range(n_bins):
        sel = live & (code == b)
        n_bin = int(np.count_nonzero(sel))
        tol_a[b] = share_bound(int(np.count_nonzero(live))) * w[sel].sum() / total
        if n_bin == 0:
            continue
        share = w[sel] / w[sel].sum()
        tol_m[b] = 1.01 * mean_units(n_bin, n_tiles) * U * (share * np.abs(y[sel])).sum()
        d = np.abs(y[sel] - mean[b])
        tol_v[b] = 1.01 * var_units(n_bin, n_tiles) * U * (share * d * d).sum() + 3.0 * tol_m[b] * tol_m[b]
    return tol_a, tol_m, tol_v


def statement_point(lw_pe, lw_inj, codes_pe, codes_inj, x_pe, x_inj, pairs, n_bins, pe_mask, inj_mask):
    """The statement of one point with its bounds: ``(out (n_ev + 1, R, 3, B), dead, tol (n_ev + 1, R, 3, B))``; the tolerances are NaN
    wherever the statement is (a dead segment, a set left out, a bin without weight: nothing is compared there but the NaN itself)."""
    from gwinferno_amd.draws import draw_weights, point_conditionals_reference

    out, dead = point_conditionals_reference(lw_pe, lw_inj, codes_pe, codes_inj, x_pe, x_inj, pairs, n_bins, pe_mask, inj_mask)
    tol = np.full(out.shape, np.nan)
    n_ev = lw_pe.shape[0]
    for seg in range(n_ev + 1):
        if dead[seg] or (codes_pe is None or x_pe is None if seg < n_ev else codes_inj is None or x_inj is None):
            continue
        w = draw_weights(lw_pe[seg], None if pe_mask is None else pe_mask[seg]) if seg < n_ev else draw_weights(lw_inj, inj_mask)
        for r, (cx, cy) in enumerate(pairs):
            code, y = (codes_pe[cx, seg], x_pe[cy, seg]) if seg < n_ev else (codes_inj[cx], x_inj[cy])
            tol[seg, r] = tolerances(w, code, y, out[seg, r, 1], n_bins, -(-w.size // TILE))
    return out, dead, tol
