"""TEST INFRASTRUCTURE shared by tests/test_hist2d_cpu.py and tests/test_gpu_hist2d.py: hist_util's catalog (3 events x 1 500 PE samples
-- two tiles per event, the second ragged at 476 samples -- and 2 600 injections -- three tiles, the last ragged), its points and its
"free" / "masked" masks, with three bin columns and the derived error bounds of the joint tables and of what is computed from them."""
import functools

import hist_util as U
import numpy as np

COLUMNS = ("mass_1", "mass_2", "mass_ratio")
N_BINS = (7, 64)      # 7: several cells per owner thread and empty cells; 64: the cap, every LDS cell in use
PAIRS = ((0, 2), (1, 0))  # (mass_1, mass_ratio) and (mass_2, mass_1): a column on either side
K_POINTS = 3
MI_FLOOR = 2.0**-30   # a table's mutual information is compared only where every occupied cell of the statement exceeds this share


@functools.lru_cache(maxsize=None)
def edges(n_bins):
    """Per column ``n_bins + 1`` increasing edges between the 2 % and 98 % quantiles of the column's PE and injection values together, so
    that samples lie outside on both sides in either coordinate: geometric for mass_1, uniform for the others."""
    pe, inj, _ = U.catalog()
    out = {}
    for name in COLUMNS:
        v = np.concatenate([pe[name].ravel(), inj[name]])
        lo, hi = np.quantile(v, [0.02, 0.98])
        out[name] = np.geomspace(lo, hi, n_bins + 1) if name == "mass_1" else np.linspace(lo, hi, n_bins + 1)
    return out


@functools.lru_cache(maxsize=None)
def bins(n_bins):
    """``(pe_bins (3, n_ev, n_pe), inj_bins (3, n_inj))`` uint16 codes, read-only."""
    from gwinferno_amd.draws import digitize

    pe, inj, _ = U.catalog()
    e = edges(n_bins)
    pb, ib = np.stack([digitize(pe[c], e[c]) for c in COLUMNS]), np.stack([digitize(inj[c], e[c]) for c in COLUMNS])
    pb.setflags(write=False)
    ib.setflags(write=False)
    return pb, ib


def values():
    pe, inj, _ = U.catalog()
    return {c: pe[c] for c in COLUMNS}, {c: inj[c] for c in COLUMNS}


def live_counts(lw_pe, lw_inj, pm, im):
    """Live samples of every segment, the injection set last."""
    return [U.n_live(lw, mask) for lw, mask in U.segments(lw_pe, lw_inj, pm, im)]


def cell_bound(n_live):
    """A cell of one segment at one point: hist_util.bound -- (n_live + 8) 2^-52 relative: the same exp on both sides, non-negative terms
    summed in any order, one quotient."""
    return U.bound(n_live)


def obs_bound(n_live_events, n_ev=U.N_EV):
    """DERIVED.  obs = (sum of the live events' cells) / n_live: every term is non-negative and within cell_bound of its exact value, so
    the exact sum is within the largest of them; the sum of at most n_ev terms and the quotient round n_ev times at most on either side:
    n_ev + 1 more half-units (2^-53 each) on top of the largest cell bound, relative to the statement's value."""
    return cell_bound(max(n_live_events)) + (n_ev + 1) * 2.0**-53


def mean_bound(eps, k, weighted):
    """DERIVED.  The mean over k points of non-negative cells each within eps: k - 1 additions and one quotient on either side (k
    half-units each), and with point weights one product per term on either side; the divisor (k - dead, or the sum of the weights,
    added in the same order on both sides) has the same bits on both sides."""
    return eps + (2 * k + (2 if weighted else 0)) * 2.0**-53


def tv_bound(eps_obs, eps_pred, n_bins):
    """DERIVED, absolute.  tv = sum |o / t_o - p / t_p| / 2 with t the sum of the table's B^2 non-negative cells: t is within eps + B^2 2^-53
    (its own summation), a cell's o / t_o within 2 eps + (B^2 + 2) 2^-53 of its value, and the o / t_o sum to 1: the two sides move the sum
    of the absolute differences by at most (2 eps_obs + 2 eps_pred + 2 (B^2 + 2) 2^-53), halved; the final sum of B^2 terms that total at
    most 2 adds B^2 2^-52 on either side."""
    cells = n_bins * n_bins
    return eps_obs + eps_pred + (cells + 2) * 2.0**-53 + 2 * cells * 2.0**-52


def mi_bound(eps, n_bins, abs_log_sum):
    """DERIVED, absolute.  mi = sum q log(q / (px py)) with q = p / t: q is within eta = 2 eps + (B^2 + 2) 2^-53 relative, px and py (sums of
    B such terms) within eta + B 2^-53, so the logarithm moves by at most 3 eta + 2 B 2^-53 + 2^-52 (its own rounding) and a term by q
    times that plus eta q |log|; summed, with sum q = 1 and A = sum q |log(q / (px py))| taken from the STATEMENT's table: 3 eta + 2 B 2^-53
    + 2^-52 + eta A, and the summation of B^2 terms adds B^2 2^-53 (A + 1) on either side."""
    cells = n_bins * n_bins
    eta = 2.0 * eps + (cells + 2) * 2.0**-53
    return 3.0 * eta + 2 * n_bins * 2.0**-53 + 2.0**-52 + eta * abs_log_sum + 2 * cells * 2.0**-53 * (abs_log_sum + 1.0)


def abs_log_sum(p):
    """``A = sum q |log(q / (px py))|`` of tables ``p (..., B, B)`` (NaN where the total is 0)."""
    from gwinferno_amd.draws import joint_table_summaries

    s = joint_table_summaries(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = p / s["total"][..., None, None]
        has = q > 0.0
        ratio = np.where(has, q / (s["px"][..., :, None] * s["py"][..., None, :]), 1.0)
        return (np.where(has, q, 0.0) * np.abs(np.log(ratio))).sum(axis=(-2, -1))


def mi_comparable(p):
    """Per table of ``p (..., B, B)``: every occupied cell exceeds MI_FLOOR of the table's total (and the total is positive)."""
    p = np.asarray(p, dtype=np.float64)
    t = p.sum(axis=(-2, -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        small = (p > 0.0) & (p <= MI_FLOOR * t[..., None, None])
    return (t > 0.0) & ~small.any(axis=(-2, -1))
