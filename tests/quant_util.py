"""TEST INFRASTRUCTURE shared by tests/test_quant_cpu.py and tests/test_gpu_quant.py: the quantile columns, the levels, the derived
error bounds and the comparison of the marginal-weight / weighted-quantile tests.  The catalog, the compositions, the points, the
masks and the two extreme points are those of the weighted-histogram tests (tests/hist_util.py)."""
import functools

import hist_util as U
import numpy as np

K = 3
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)
LEVELS_32 = tuple(float(v) for v in np.linspace(0.0, 1.0, 32))  # the cap; both ends among them
COLUMNS_8 = ("mass_1", "mass_2", "mass_1_rounded", "mass_1_signed", "mass_ratio", "redshift", "mass_2_rounded", "mass_ratio_signed")


@functools.lru_cache(maxsize=None)
def columns(n_cols):
    """``(pe_values (n_cols, n_ev, n_pe), inj_values (n_cols, n_inj))``, read-only: 1 column (mass_1) or the cap of 8 -- among them
    mass_2 = q m1 (a derived quantity), mass_1 rounded to integers (many ties), and mass_1 minus its median (signed: the moment
    sums have terms of both signs)."""
    pe, inj, _ = U.catalog()

    def derive(d):
        m1, q = np.asarray(d["mass_1"], dtype=np.float64), np.asarray(d["mass_ratio"], dtype=np.float64)
        m2 = np.asarray(d["mass_2"], dtype=np.float64) if "mass_2" in d else m1 * q
        full = {"mass_1": m1, "mass_2": m2, "mass_1_rounded": np.round(m1), "mass_1_signed": m1 - np.median(m1), "mass_ratio": q,
                "redshift": np.asarray(d["redshift"], dtype=np.float64), "mass_2_rounded": np.round(m2), "mass_ratio_signed": q - np.median(q)}
        return np.stack([full[c] for c in COLUMNS_8[:n_cols]])

    vp, vi = derive(pe), derive(inj)
    vp.setflags(write=False)
    vi.setflags(write=False)
    return vp, vi


@functools.lru_cache(maxsize=None)
def orders(n_cols):
    """The stable sort orders of :func:`columns`, as Engine.set_quantile_columns makes them."""
    vp, vi = columns(n_cols)
    return np.argsort(vp, axis=-1, kind="stable").astype(np.int32), np.argsort(vi, axis=-1, kind="stable").astype(np.int32)


def weight_bound(live, k=K):
    """DERIVED, not measured.  One point's w_i / S is within (n_live + 8) 2^-52 relative of the statement's (hist_util.bound: the
    summation of S over n_live non-negative terms, two exp roundings, the division); W_i is the sum of k such non-negative terms,
    and each of the k additions rounds once on either side (2^-53 each, 2^-52 together): (n_live + 8 + k) 2^-52 relative."""
    return (live + 8 + k) * 2.0**-52


def moment_bound(live):
    """DERIVED, not measured.  sum W_i x_i^m over n_live terms with weight: each product W x (and W x x) rounds once or twice on
    either side (at most 4 * 2^-53 together), the summation in any order carries at most (n_live - 1) 2^-53 on the device and none in
    the statement's fsum, one final rounding each: within (n_live + 10) 2^-52 of sum W_i |x_i|^m -- relative to the sum of the
    ABSOLUTE terms, since a signed column cancels."""
    return (live + 10) * 2.0**-52


def band(live):
    """The only indices that may differ from the statement's: a level whose target p C_last lies within (n_live + 8) 2^-52 C_last of
    one of the statement's prefix values -- the error of the device's prefix (a sum of at most n_live non-negative terms) and of its
    C_last and the product.  There the neighbouring rank with weight is also accepted.  Levels 0 and 1 are exempt: exact."""
    return (live + 8) * 2.0**-52


def check_segment(W, order, x, levels, got_idx, got_mom, got_mass, what):
    """One (segment, column) of the device against the statement on the same W.  Returns the number of levels in the band (accepted
    with the neighbouring rank); raises on anything else."""
    from gwinferno_amd.draws import weighted_quantiles_reference

    levels = np.asarray(levels, dtype=np.float64)
    idx, (m1, m2), mass = weighted_quantiles_reference(W, order, x, levels)
    live = int(np.count_nonzero(W > 0.0))
    if live == 0:
        assert np.all(got_idx == -1) and got_mass == 0.0 and got_mom[0] == 0.0 and got_mom[1] == 0.0, what
        return 0
    assert abs(got_mass - mass) <= U.bound(live) * mass, (what, got_mass, mass)
    ws, xs = W[order], x[order]
    for m, want, got in ((1, m1, got_mom[0]), (2, m2, got_mom[1])):
        scale = float(np.sum(ws * np.abs(xs) ** m))
        assert abs(got - want) <= moment_bound(live) * scale, (what, m, got, want, abs(got - want) / scale, moment_bound(live))
    in_band = 0
    ranks = np.nonzero(ws > 0.0)[0]       # the ranks with weight, ascending
    rank_of = np.empty(order.size, dtype=np.int64)
    rank_of[order] = np.arange(order.size)
    prefix = np.cumsum(ws[ranks].astype(np.longdouble))
    for q, p in enumerate(levels):
        if got_idx[q] == idx[q]:
            continue
        assert 0.0 < p < 1.0, (what, p, int(got_idx[q]), int(idx[q]))  # levels 0 and 1 are exact
        assert got_idx[q] >= 0 and W[got_idx[q]] > 0.0, (what, p, int(got_idx[q]))
        at, at_got = np.searchsorted(ranks, rank_of[idx[q]]), np.searchsorted(ranks, rank_of[got_idx[q]])
        near = float(np.min(np.abs(prefix - np.longdouble(p) * prefix[-1])) / prefix[-1])
        assert abs(int(at) - int(at_got)) == 1 and near <= band(live), (what, p, int(got_idx[q]), int(idx[q]), near, band(live))
        in_band += 1
    return in_band
