"""Generator of tests/golden/math_probe_hp.npz: designed arguments for the device maths primitives of gwinferno_amd/csrc/gwi_device.h
(fast_exp, fast_exp_shift, fast_expm1, fast_rcp, cubic_taps, cubic_taps_weighted, spline_poly + spline_value, the spline_locate
family, wave_sum, wave_max, wave_max_coarse, wave_sum8, binades_of) and their values from the DEFINITIONS at 50 digits.

    python tests/golden/make_math_probe_hp.py       # rewrites math_probe_hp.npz (and checks the working precision)

Nothing of gwinferno_amd/ or oracle/ is imported: the fixture is the independent side of tests/test_math_probe_cpu.py and
tests/test_gpu_math_probe.py, which read only the .npz.

Conventions
  * Inputs are float64 and enter the arithmetic exactly.  A reference is rounded ONCE to float64 (``<op>_ref``); for the ops whose
    bars are a few units of 2^-53 the rounding residual is kept too (``<op>_ref_lo`` = round(exact - ref)), so ref + ref_lo is the
    exact value to ~106 bits.  ``generate(verify=True)`` repeats everything at 2 x DPS and asserts that no double moves.
  * What the code DOCUMENTS about its edges is part of the definition: fast_exp clamps its argument to [-1000, 710] and
    fast_exp_shift to [-7e5, 7e5] with v_max / v_min, which return the non-NaN operand, so NaN behaves as the lower clamp
    (exp -> 0, expm1 -> -1); a value of exp above the float64 range is +inf, one that rounds to zero is 0.  The reference of
    fast_exp_shift is exp(clamp(x)) 2^-shift.
  * The locate family returns k = clamp(floor(u), 0, n_basis - 4) and t = u - k, u = (x - lo) * inv_dx formed in float64 as the
    code states it (the inputs are chosen so that both steps are exact except at |x| >= 1e9); spline_locate_knot, on [0, n_int)
    only, k = floor(u), t = u - k.
  * ``expm1_parent_bits``: what fast_expm1 returned on an MI355X BEFORE it was repaired for x in [709.44, 709.78) -- recorded once
    from a build of the parent commit, not computable here.  The generator carries the array over from the existing file as long
    as ``expm1_x`` is unchanged (``python make_math_probe_hp.py --parent-bits FILE.npy`` stores a new recording).
"""
import math
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 50
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "math_probe_hp.npz")
LOG2E_D = 1.4426950408889634  # the double the kernels multiply by (gwi_device.h: kLog2e)
RCP_FLOOR = 1e-290            # gwi_device.h: kRcpFloor
INF, NAN = float("inf"), float("nan")


def F(x):
    return mp.mpf(float(x))


def to_double(v):
    """mpf -> float64, rounded to nearest once; overflow -> +-inf, underflow through the subnormals to 0"""
    v = mp.mpf(v)
    if mp.isinf(v):
        return INF if v > 0 else -INF
    sign, man, exp, _ = v._mpf_  # v = (-1)^sign man 2^exp exactly; Python's int / int is correctly rounded, subnormals included
    if man == 0:
        return 0.0
    try:
        r = float(man << exp) if exp >= 0 else man / (1 << -exp)
    except OverflowError:
        r = INF
    return -r if sign else r


def hi_lo(v):
    """v (an mpf, or a Fraction: exact) as its nearest double and the residual.  The residual is kept to float32 precision and dropped
    below 1e-30 |hi|: it refines a bar of a few 2^-53, and beyond that it would record the working precision, not the value."""
    exact = isinstance(v, Fraction)
    hi = float(v) if exact else to_double(v)
    if math.isinf(hi) or hi == 0.0:
        return hi, 0.0
    lo = float(v - Fraction(hi)) if exact else to_double(v - F(hi))
    if abs(lo) < 1e-30 * abs(hi):
        return hi, 0.0
    m, e = math.frexp(lo)
    return hi, math.ldexp(round(m * 2.0**24) / 2.0**24, e)  # 24 significant bits


def neighbours(x):
    return [np.nextafter(x, -INF), x, np.nextafter(x, INF)]


def ladder(lo_exp, hi_exp, per_decade):
    n = (hi_exp - lo_exp) * per_decade
    return [float(10.0 ** (lo_exp + i / per_decade)) for i in range(n + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# exp family
# ---------------------------------------------------------------------------------------------------------------------
def half_integer_points():
    xs = []
    ln2 = mp.log(2)
    for n in list(range(-1075, -1019)) + list(range(-2, 3)) + list(range(1020, 1025)):
        xs += neighbours(to_double((n + mp.mpf(1) / 2) * ln2))
    return xs


def exp_specials():
    xs = []
    for e in (-1000.0, 710.0, -7.0e5, 7.0e5):
        xs += neighbours(e)
    xs += [0.0, -0.0, 2.0**-1074, -(2.0**-1074), 1e-300, -1e-300, -745.13, -708.4, INF, -INF, NAN]
    return xs


def exp_clamped(x, lo, hi):
    if x != x:
        x = lo  # v_max returns the non-NaN operand
    x = min(max(x, lo), hi)
    return mp.exp(F(x))


def exp_inputs(rng):
    xs = half_integer_points() + exp_specials()
    xs += list(rng.uniform(-745.0, 709.7, 512)) + list(rng.uniform(-1.0, 1.0, 256))
    return np.array(xs, dtype=np.float64)


def exp_shift_inputs():
    xs, shifts = [], []
    for x in exp_specials() + half_integer_points():
        xs.append(x)
        shifts.append(0 if (x != x or math.isinf(x)) else int(round(min(max(x, -7e5), 7e5) * LOG2E_D)))
    for mag in ladder(-18, 5, 16) + [2e5, 3e5, 5e5, 6.9e5, 7e5]:
        if mag > 7e5:
            continue
        for s in (1.0, -1.0):
            n = int(round(s * mag * LOG2E_D))
            for d in (0, -1000, 1000):
                xs.append(s * mag)
                shifts.append(n + d)
    return np.array(xs, dtype=np.float64), np.array(shifts, dtype=np.float64)


def expm1_inputs(rng):
    xs = []
    for mag in ladder(-18, -1, 16) + list(np.linspace(0.1, 0.3466, 24)):
        xs += [mag, -mag]
    xs += half_integer_points()[56 * 3:(56 + 5) * 3]  # n = -2 .. 2 flips
    xs += [709.0 + i / 64.0 for i in range(65)]
    xs += [-40.0, -50.0, -100.0, -745.0, -1000.0, -1e5, -INF]
    xs += [0.0, -0.0, 2.0**-1074, -(2.0**-1074), 1e-300, -1e-300, INF, NAN, 710.0, 711.0]
    xs += list(rng.uniform(-40.0, 709.0, 512)) + list(rng.uniform(-1.0, 1.0, 256))
    return np.array(xs, dtype=np.float64)


def expm1_ref(x):
    if x != x:
        x = -1000.0
    x = min(max(x, -1000.0), 710.0)
    return mp.expm1(F(x))


# ---------------------------------------------------------------------------------------------------------------------
# fast_rcp
# ---------------------------------------------------------------------------------------------------------------------
def rcp_inputs():
    xs = []
    for k in range(-1022, 1024):
        xs += neighbours(2.0**k) if k % 8 == 0 else [2.0**k]
    lad = ladder(-308, 308, 3)
    lad[0] = 1e-308  # (subnormal: recorded, not held)
    xs += lad + [-v for v in lad]
    xs += neighbours(RCP_FLOOR) + [2.0**-1022, np.nextafter(2.0**-1022, INF)]
    xs += [2.0**1022 * (1.0 + i / 8.0) for i in range(8)] + [2.0**1023, np.nextafter(INF, 0.0)]
    xs += [2.0**-1074, 2.0**-1023, 1e-310, np.nextafter(2.0**-1022, 0.0)]  # subnormals
    xs += [0.0, -0.0, INF, -INF]
    return np.array(xs, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# taps, spline value
# ---------------------------------------------------------------------------------------------------------------------
def tap_fractions(rng):
    ts = [0.0, 2.0**-52, 2.0**-30, 1.0 / 3.0, 0.5, 1.0 - 2.0**-30, 1.0 - 2.0**-52, 1.0]
    ts += [i / 255.0 for i in range(256)] + list(rng.uniform(0.0, 1.0, 256))
    return np.array(ts, dtype=np.float64)


def basis(t):
    """the four non-zero uniform cubic B-spline bases on a knot interval at fraction t (exact rational functions of t)"""
    t = Fraction(float(t))
    v = 1 - t
    return [v**3 / 6, (3 * t**3 - 6 * t**2 + 4) / 6, (3 * v**3 - 6 * v**2 + 4) / 6, t**3 / 6]


WEIGHTS = [1.0, 1e-300, 1e-150, 1e150, 1e300, -1.0, 3.7]


# ---------------------------------------------------------------------------------------------------------------------
# locate family
# ---------------------------------------------------------------------------------------------------------------------
N_BASIS = [4, 5, 16, 17, 200]
GRIDS = [(2.0, 4.0), (-1.5, 8.0)]  # (lo, inv_dx): powers of two, so x = lo + u / inv_dx and back are exact next to the knots


def locate_u_points(n_basis, knot_domain_only):
    n_int = n_basis - 3
    us = []
    for j in range(n_int + 1):
        us += neighbours(float(j))
    if knot_domain_only:
        return [u for u in us if 0.0 <= u < n_int] + [-0.0, 0.5, n_int - 0.5]
    return us + [-0.0, -1e-300, -1.0, n_int + 1e-9, 1e9, 1e300, INF, -INF, 0.5, n_int - 0.5]


def locate_ref(u, n_basis):
    last = n_basis - 4
    if math.isinf(u):
        k = last if u > 0 else 0
        return k, u
    k = min(max(int(mp.floor(F(u))), 0), last)
    return k, to_double(F(u) - k)


# ---------------------------------------------------------------------------------------------------------------------
def compute(rng_seed=20240607):
    rng = np.random.default_rng(rng_seed)
    out = {}
    # ---- exp
    x = exp_inputs(rng)
    out["exp_x"] = x
    out["exp_ref"] = np.array([to_double(exp_clamped(v, -1000.0, 710.0)) for v in x])
    # ---- exp_shift
    x, sh = exp_shift_inputs()
    out["exp_shift_x"], out["exp_shift_shift"] = x, sh
    out["exp_shift_ref"] = np.array([to_double(mp.ldexp(exp_clamped(v, -7e5, 7e5), -int(s))) for v, s in zip(x, sh)])
    # ---- expm1
    x = expm1_inputs(rng)
    out["expm1_x"] = x
    pairs = [hi_lo(expm1_ref(v)) for v in x]
    out["expm1_ref"], out["expm1_ref_lo"] = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    # ---- rcp (1/0 and 1/inf: placeholders, nothing is asserted there)
    x = rcp_inputs()
    out["rcp_x"] = x
    pairs = [(math.copysign(INF, v), 0.0) if v == 0 else (math.copysign(0.0, v), 0.0) if math.isinf(v) else hi_lo(1 / F(v)) for v in x]
    out["rcp_ref"], out["rcp_ref_lo"] = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    # ---- taps
    ts = tap_fractions(rng)
    out["taps_t"] = ts
    pairs = [[hi_lo(b) for b in basis(t)] for t in ts]
    out["taps_ref"] = np.array([[p[0] for p in row] for row in pairs])
    out["taps_ref_lo"] = np.array([[p[1] for p in row] for row in pairs])
    wt, ww = np.repeat(ts, len(WEIGHTS)), np.tile(np.array(WEIGHTS), len(ts))
    out["taps_w_t"], out["taps_w_w"] = wt, ww
    pairs = [[hi_lo(Fraction(float(w)) * b) for b in basis(t)] for t, w in zip(wt, ww)]
    out["taps_w_ref"] = np.array([[p[0] for p in row] for row in pairs])
    out["taps_w_ref_lo"] = np.array([[p[1] for p in row] for row in pairs])
    # ---- spline value: groups of four lanes share four coefficients; 4 sets x (520 fractions in groups of four)
    coef_sets = np.array([[2.5, 2.5, 2.5, 2.5], [1e3, -1e3, 1e3, -1e3], [1e6, 1e-6, 1e-6, 1e-6], list(rng.normal(0.0, 3.0, 4))])
    assert ts.size % 4 == 0
    sv_t = np.tile(ts, len(coef_sets))
    sv_c = np.concatenate([np.tile(c, ts.size // 4) for c in coef_sets])  # lane i carries coefficient i % 4 of its set
    sv_set = np.repeat(np.arange(len(coef_sets)), ts.size)
    out["spline_t"], out["spline_c"], out["spline_set"], out["spline_coef_sets"] = sv_t, sv_c, sv_set.astype(np.int32), coef_sets
    ref, ref_lo, scale = [], [], []
    for t, s in zip(sv_t, sv_set):
        b = basis(t)
        c = [Fraction(float(v)) for v in coef_sets[s]]
        h, l = hi_lo(sum(ci * bi for ci, bi in zip(c, b)))
        ref.append(h), ref_lo.append(l), scale.append(float(sum(abs(ci) * bi for ci, bi in zip(c, b))))
    out["spline_ref"], out["spline_ref_lo"], out["spline_abs"] = np.array(ref), np.array(ref_lo), np.array(scale)
    # ---- locate family
    lu, lnb, lk, lt = [], [], [], []
    for nb in N_BASIS:
        for u in locate_u_points(nb, False):
            k, t = locate_ref(u, nb)
            lu.append(u), lnb.append(nb), lk.append(k), lt.append(t)
    out["locate_term_u"], out["locate_term_n_basis"] = np.array(lu), np.array(lnb, dtype=np.float64)
    out["locate_term_k"], out["locate_term_t"] = np.array(lk, dtype=np.int32), np.array(lt)
    lu, lk, lt, lnb = [], [], [], []
    for nb in N_BASIS:
        for u in locate_u_points(nb, True):
            k = int(mp.floor(F(u)))
            lu.append(u), lk.append(k), lt.append(to_double(F(u) - k)), lnb.append(nb)
    out["locate_knot_u"], out["locate_knot_k"], out["locate_knot_t"] = np.array(lu), np.array(lk, dtype=np.int32), np.array(lt)
    out["locate_knot_n_basis"] = np.array(lnb, dtype=np.float64)
    lx, lb3, lk, lt = [], [], [], []
    for lo, inv_dx in GRIDS:
        for nb in N_BASIS:
            for u0 in locate_u_points(nb, False):
                # the x next to the knot: x = lo + u0 / inv_dx rounded once, and the u the code forms from it in float64
                xs = [to_double(F(lo) + F(u0) / F(inv_dx))] if not math.isinf(u0) else [u0]
                if abs(u0) < 1e6 and u0 == math.floor(u0):
                    xs = neighbours(xs[0])
                for xv in xs:
                    d = xv - lo if math.isinf(xv) else to_double(F(xv) - F(lo))
                    u = d * inv_dx if math.isinf(d) else to_double(F(d) * F(inv_dx))
                    k, t = locate_ref(u, nb)
                    lx.append(xv), lb3.append([lo, inv_dx, float(nb)]), lk.append(k), lt.append(t)
    out["locate_x"], out["locate_b"] = np.array(lx), np.array(lb3)
    out["locate_k"], out["locate_t"] = np.array(lk, dtype=np.int32), np.array(lt)
    # ---- binades_of: rint(clamp(m, +-7e5) * kLog2e), product rounded to double, then to the nearest integer, ties to even
    ms = []
    for n in list(range(-3, 4)) + [100, -100, 1000, -1000, 54321, -54321, 1009886, -1009886]:
        ms += neighbours(to_double((n + mp.mpf(1) / 2) / F(LOG2E_D)))
    for e in (-7e5, 7e5):
        ms += neighbours(e)
    ms += [0.0, -0.0, 1e6, -1e6, INF, -INF, 1e300, 2.0**-1074] + list(rng.uniform(-7e5, 7e5, 512)) + list(rng.uniform(-800.0, 800.0, 256))
    ms = np.array(ms)
    out["binades_m"] = ms
    out["binades_ref"] = np.array([int(mp.nint(F(to_double(F(min(max(m, -7e5), 7e5)) * F(LOG2E_D))))) for m in ms], dtype=np.int32)
    # ---- wave reductions: rows of 64 lanes
    pow2 = np.array([2.0**l if l < 52 else 0.0 for l in range(64)])
    waves = [np.ones(64)] + [np.eye(64)[j] for j in range(64)] + [pow2]
    n_exact = len(waves)
    for scale in (1.0, 1e-8, 1e8, 1.0):
        waves.append(rng.normal(0.0, scale, 64))
    waves.append(rng.normal(0.0, 1.0, 64) * 10.0 ** rng.uniform(-10, 10, 64))
    waves = np.array(waves)
    out["wave_sum_v"], out["wave_sum_n_exact"] = waves, np.array(n_exact)
    out["wave_sum_ref"] = np.array([math.fsum(w) for w in waves])
    out["wave_sum_abs"] = np.array([math.fsum(np.abs(w)) for w in waves])
    mx = []
    for j in range(64):  # the maximum at each lane in turn, over positive, negative and mixed backgrounds
        bg = rng.uniform(-1.0, 1.0, 64) if j % 3 == 0 else (rng.uniform(-9.0, -1.0, 64) if j % 3 == 1 else rng.uniform(0.1, 1.0, 64))
        bg[j] = 2.0 if j % 3 != 1 else -0.5
        mx.append(bg)
    mx += [np.full(64, -INF), rng.normal(0.0, 1.0, 64), -np.abs(rng.normal(0.0, 1.0, 64)) - 1.0, np.full(64, -0.0), np.where(np.arange(64) == 17, 0.0, -0.0),
           np.where(np.arange(64) == 40, -3.0, -INF)]
    out["wave_max_v"] = np.array(mx)
    out["wave_max_ref"] = np.array([np.max(w) for w in mx])
    cz = [np.where(np.arange(64) == 5, 1e-30, -1.0), np.where(np.arange(64) == 63, 3e38, 1.0), np.where(np.arange(64) == 0, -3e38, -INF),
          np.where(np.arange(64) == 31, 1e-30, 0.0), rng.normal(0.0, 1.0, 64) * 1e30, rng.normal(0.0, 1.0, 64) * 1e-30]
    out["wave_max_coarse_extra_v"] = np.array(cz)
    out["wave_max_coarse_extra_ref"] = np.array([np.max(w) for w in cz])
    out["wave_max_coarse_outside_v"] = np.array([np.where(np.arange(64) == 9, 1e300, 1.0), np.where(np.arange(64) == 9, 1e-300, 0.0), np.where(np.arange(64) == 9, 3.5e38, 1.0)])
    # ---- wave_sum8: [wave][lane][slot]; slot s carries the pattern under test, slot j != s the exact filler (j + 1)(lane + 1)
    filler = np.array([[(j + 1.0) * (l + 1.0) for j in range(8)] for l in range(64)])
    s8 = []
    for s in range(8):
        for pat in [np.ones(64), pow2] + [np.eye(64)[j] for j in range(64)]:
            w = filler.copy()
            w[:, s] = pat
            s8.append(w)
    n_exact8 = len(s8)
    for _ in range(4):
        s8.append(rng.normal(0.0, 1.0, (64, 8)))
    s8 = np.array(s8)
    out["wave_sum8_v"], out["wave_sum8_n_exact"] = s8, np.array(n_exact8)
    out["wave_sum8_ref"] = np.array([[math.fsum(w[:, j]) for j in range(8)] for w in s8])
    out["wave_sum8_abs"] = np.array([[math.fsum(np.abs(w[:, j])) for j in range(8)] for w in s8])
    return out


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def generate(verify=True, parent_bits=None):
    mp.mp.dps = DPS
    out = compute()
    if verify:
        mp.mp.dps = 2 * DPS
        again = compute()
        mp.mp.dps = DPS
        moved = [k for k in out if not same(out[k], again[k])]
        assert not moved, f"references move between {DPS} and {2 * DPS} digits: {moved}"
    if parent_bits is not None:
        bits = np.load(parent_bits)
        assert bits.dtype == np.uint64 and bits.shape == out["expm1_x"].shape
        out["expm1_parent_bits"] = bits
    elif os.path.exists(OUT):
        old = np.load(OUT)
        if "expm1_parent_bits" in old.files and same(old["expm1_x"], out["expm1_x"]):
            out["expm1_parent_bits"] = old["expm1_parent_bits"]
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 512 * 1024, size
    print(f"wrote {OUT}: {size} bytes, {len(out)} arrays" + ("" if "expm1_parent_bits" in out else " (WITHOUT expm1_parent_bits: record them on a GPU)"))


if __name__ == "__main__":
    generate(parent_bits=sys.argv[sys.argv.index("--parent-bits") + 1] if "--parent-bits" in sys.argv else None)
