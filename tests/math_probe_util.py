"""Shared by tests/test_math_probe_cpu.py and tests/test_gpu_math_probe.py: the fixture, the call of gwi_math_probe, the bars, and a
plain float64 emulation of the device maths primitives of gwinferno_amd/csrc/gwi_device.h (FMAs exact, through integer arithmetic).

The bars -- derived from the constants in the source and the number format, never from what a device returned
  u = 2^-53 (half an ulp of 1).
  fast_exp, fast_exp_shift   relative error <= E_POLY + LN2_ERR |n| + 4 u, n = rint(clamp(x) log2 e):
                               E_POLY   the largest relative error of e^r = 1 + r q(r) over |r| <= 0.3466 for the COMMITTED coefficients
                                        (parsed from gwi_device.h), as tools/exp_poly.py: fp64_error reports it (1.6e-14);
                               LN2_ERR  |ln2 rounded to double - ln 2| = 2.32e-17: the one-piece reduction r = fma(n, -ln2, x) moves r,
                                        and so the result, by that times |n|;
                               4 u      the roundings of q r, 1 + rq and the half-ulp of the reference (ldexp is exact for a normal result).
                             A result below 2^-1022 is NOT flushed: ldexp rounds it to the subnormal grid, so it is held to the same
                             bar plus one quantum 2^-1074.  Where the reference is 0 or +inf the device must return exactly that.
  fast_expm1                 relative error of e^x - 1.  n = 0 (|x| <= 0.3466...): the result is x q(x), so the error is that of q
                             against q* = (e^x - 1)/x: min(E_Q, E_POLY e^x / |e^x - 1|) + 4 u, E_Q = max |q / q* - 1| over the interval
                             = 2.2e-13 (the minimax fit bounds |x (q - q*)|, so q itself is 1.5e-14 / |x| off for small |x|, up to E_Q near
                             |x| = 0.07; at x -> 0 the error is |C0 - 1| = 8.7e-14).  n != 0: f = e^x / |e^x - 1| times the polynomial's and the
                             reduction's share of the fast_exp bar (an absolute error of e^x, divided by the smaller e^x - 1), + 4 u max(f, 1)
                             for the roundings (the last one is relative to the result).  x <= -40: exactly -1.  Reference +inf: +inf.
  fast_rcp                   2 ulp of the reference on 2^-1022 <= |x| <= 2^1022 (x and 1/x both normal).  The emulation starts the two
                             Newton steps from seeds (1/x)(1 + d), |d| <= 2^-20: after one step the error is d^2 = 2^-40, after two
                             2^-80 + the last FMA's half ulp.
  cubic_taps(_weighted)      each tap within 4 u max(|reference|, |w| / 6); the four unweighted taps sum to 1 within 4 u.
  spline_value               within 8 u sum_i |c_i| b_i(t) of sum_i c_i b_i(t): what the four taps (4 u each) and their dot product (a
                             product and three additions) hold, and what the Bernstein form of spline_poly + spline_value holds too.
  locate family, binades_of, wave_max, the exact patterns of wave_sum and wave_sum8: equality.
  wave_sum, wave_sum8 on random data: within 64 u sum |v| of math.fsum (63 additions of at most u sum |v| each).
  wave_max_coarse            within 2^-24 |max| of the maximum (one float32 rounding) on -inf, 0 and 2^-126 <= |v| <= 3.4e38.
"""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "math_probe_hp.npz")
DEVICE_H = os.path.join(ROOT, "gwinferno_amd", "csrc", "gwi_device.h")

OPS = {"exp": 1, "exp_shift": 2, "expm1": 3, "rcp": 4, "taps": 5, "taps_w": 6, "spline": 7, "locate_knot": 8, "locate_term": 9, "locate_x": 10, "locate": 11,
       "wave_sum": 12, "wave_max": 13, "wave_max_coarse": 14, "wave_sum8": 15, "binades": 16}
U = 2.0**-53
LN2_D = 6.93147180559945286227e-01
LN2_ERR = 2.32e-17  # |LN2_D - ln 2| = 2.3190468138462996e-17, rounded up
LOG2E_D = 1.4426950408889634
QUANTUM = 2.0**-1074
INF = float("inf")

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
        for v in _fixture.values():
            v.setflags(write=False)
    return _fixture


# ---------------------------------------------------------------------------------------------------------------------
# the constants of the source
# ---------------------------------------------------------------------------------------------------------------------
def source_constants():
    """GWI_EXP_C0..C8, the ln 2 of exp_reduce, kLog2e and kRcpFloor as the header spells them"""
    src = open(DEVICE_H).read()
    c = [float(re.search(rf"#define GWI_EXP_C{j} (\S+)", src).group(1)) for j in range(9)]
    ln2 = float(re.search(r"return fma\(nf, -([0-9.e+-]+), x\);", src).group(1))
    log2e = float(re.search(r"constexpr double kLog2e = ([0-9.e+-]+);", src).group(1))
    floor = float(re.search(r"constexpr double kRcpFloor = ([0-9.e+-]+);", src).group(1))
    return {"c": c, "ln2": ln2, "log2e": log2e, "rcp_floor": floor}


_poly = None


def poly_errors():
    """(E_POLY, E_Q) of the committed coefficients: the relative error of 1 + r q(r) against e^r as tools/exp_poly.py measures it, and of
    q(r) against (e^r - 1)/r, both over |r| <= 0.3466"""
    global _poly
    if _poly is None:
        spec = importlib.util.spec_from_file_location("exp_poly", os.path.join(ROOT, "tools", "exp_poly.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        c = np.array(source_constants()["c"], dtype=np.float64)
        e_poly = mod.fp64_error(c)
        LD = np.longdouble
        r = (np.linspace(-1.0, 1.0, 200001) * 0.3466).astype(LD)
        r = r[r != 0]
        q = np.full_like(r, LD(c[-1]))
        for cj in c[-2::-1]:
            q = q * r + LD(cj)
        e_q = float(np.max(np.abs(q / mod.q_exact(r) - 1)))
        _poly = (e_poly, max(e_q, abs(c[0] - 1.0)))
    return _poly


def binades(x, lo, hi):
    x = np.where(np.isnan(x), lo, x)
    return np.rint(np.clip(x, lo, hi) * LOG2E_D)


def exp_bar(x, lo=-1000.0, hi=710.0):
    """relative bar of fast_exp (lo, hi: its clamp) / fast_exp_shift (+-7e5) per argument"""
    return poly_errors()[0] + LN2_ERR * np.abs(binades(x, lo, hi)) + 4 * U


def expm1_bar(x, ref):
    n = binades(x, -1000.0, 710.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ex = ref + 1.0
        factor = np.where(np.isfinite(ref) & (ref != 0), np.abs(ex / ref), 1.0)
    factor = np.where(ref > 1e15, 1.0, factor)
    return np.where(n == 0, np.minimum(poly_errors()[1], poly_errors()[0] * factor) + 4 * U, (exp_bar(x) - 4 * U) * factor + 4 * U * np.maximum(factor, 1.0))


def rel_error(dev, ref, ref_lo=None):
    """|dev - (ref + ref_lo)| / |ref| where the reference is finite and non-zero (elsewhere 0 if equal, inf if not)"""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lo = np.zeros_like(ref) if ref_lo is None else ref_lo
    with np.errstate(all="ignore"):
        ordinary = np.isfinite(ref) & (ref != 0) & np.isfinite(dev)
        err = np.where(ordinary, np.abs(((dev - ref) - lo) / np.where(ordinary, ref, 1.0)), np.where(dev == ref, 0.0, INF))
    return err


def abs_error(dev, ref, ref_lo=None):
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lo = np.zeros_like(ref) if ref_lo is None else ref_lo
    with np.errstate(all="ignore"):
        ordinary = np.isfinite(ref) & np.isfinite(dev)
        return np.where(ordinary, np.abs((dev - ref) - lo), np.where(dev == ref, 0.0, INF))


def worst(err, bar, args):
    """(largest err / bar, err there, bar there, argument there) -- what the tests print before they assert"""
    with np.errstate(all="ignore"):
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, INF))
    i = int(np.argmax(ratio))
    return float(ratio[i]), float(err[i]), float(np.asarray(bar).reshape(-1)[i] if np.ndim(bar) else bar), np.asarray(args)[i]


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
def a_stride(op):
    return 8 if op == OPS["wave_sum8"] else 1


def b_stride(op):
    return 3 if op in (OPS["locate_term"], OPS["locate_x"], OPS["locate"]) else 1


def probe_raw(op, n, a, b, out, iout, device=-1):
    """gwi_math_probe with the pointers as given (None = NULL): the status"""
    from gwinferno_amd import _native as N

    lib = N.load_library()
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptr = lambda v, t: None if v is None else v.ctypes.data_as(t)  # noqa: E731
    return lib.gwi_math_probe(int(device), int(op), int(n), ptr(a, DP), ptr(b, DP), ptr(out, DP), ptr(iout, IP))


def probe(op, a, b=None):
    """(out[n, 4], iout[n]) of one launch of primitive ``op`` (a name of OPS) over the lanes of ``a``"""
    code = OPS[op]
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.size // a_stride(code)
    b = np.zeros(n * b_stride(code)) if b is None else np.ascontiguousarray(b, dtype=np.float64)
    assert a.size == n * a_stride(code) and b.size == n * b_stride(code)
    out, iout = np.full((max(n, 1), 4), np.nan), np.full(max(n, 1), -12345, dtype=np.int32)
    st = probe_raw(code, n, a, b, out, iout)
    assert st == 0, st
    return out[:n], iout[:n]


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulation of the algorithms as gwi_device.h writes them
# ---------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    num = na * nb * dc + nc * da * db
    if num == 0:
        return a * b + c  # (the sign of an exact zero)
    try:
        return num / (da * db * dc)  # int / int: correctly rounded, subnormals included
    except OverflowError:
        return math.copysign(INF, num)


def ldexp(m, n):
    try:
        return math.ldexp(m, int(max(min(n, 5000), -5000)))
    except OverflowError:
        return math.copysign(INF, m)


def clamp(x, lo, hi):
    if x != x:
        return lo  # v_max_f64 / v_min_f64 return the operand that is a number
    return min(max(x, lo), hi)


class Emulation:
    def __init__(self, constants=None, old_expm1=False):
        k = constants or source_constants()
        self.c, self.ln2, self.log2e, self.old_expm1 = k["c"], k["ln2"], k["log2e"], old_expm1

    def exp_q(self, r):
        q = self.c[8]
        for j in range(7, -1, -1):
            q = fma(q, r, self.c[j])
        return q

    def exp_parts(self, x):
        x = clamp(x, -1000.0, 710.0)
        nf = float(round(x * self.log2e))
        r = fma(nf, -self.ln2, x)
        return self.exp_q(r) * r, int(nf)

    def fast_exp(self, x):
        rq, n = self.exp_parts(x)
        return ldexp(rq + 1.0, n)

    def fast_exp_shift(self, x, shift):
        x = clamp(x, -7.0e5, 7.0e5)
        nf = float(round(x * self.log2e))
        r = fma(nf, -self.ln2, x)
        return ldexp(fma(self.exp_q(r), r, 1.0), int(nf) - int(shift))

    def fast_expm1(self, x):
        rq, n = self.exp_parts(x)
        if self.old_expm1:
            s = ldexp(1.0, n)
            return fma(s, rq, s - 1.0)
        m = min(n, 1023)
        s = ldexp(1.0, m)
        return ldexp(fma(s, rq, s - 1.0), n - m)

    @staticmethod
    def fast_rcp(x, seed_error):
        r = (1.0 / x) * (1.0 + seed_error)
        e = fma(-x, r, 1.0)
        r = fma(r, e, r)
        e = fma(-x, r, 1.0)
        return fma(r, e, r)

    @staticmethod
    def cubic_taps(t):
        v = 1.0 - t
        t2, v2 = t * t, v * v
        P = fma(t, v, 1.0)
        return [v2 * (v * (1.0 / 6.0)), fma(0.5 * v, P, 1.0 / 6.0), fma(0.5 * t, P, 1.0 / 6.0), t2 * (t * (1.0 / 6.0))]

    @staticmethod
    def cubic_taps_weighted(t, w):
        w6, wh = w * (1.0 / 6.0), w * 0.5
        v = 1.0 - t
        t2, v2 = t * t, v * v
        P = fma(t, v, 1.0)
        return [(w6 * v) * v2, fma(wh * v, P, w6), fma(wh * t, P, w6), (w6 * t) * t2]

    @staticmethod
    def spline_value(c, t):
        c0, c1, c2, c3 = c
        E = (c0 + 4.0 * c1 + c2) * (1.0 / 6.0)
        F = fma(2.0, c1, c2)  # (the compiler contracts a product and a sum; the product by two is exact either way)
        G = fma(2.0, c2, c1)
        H = (c1 + 4.0 * c2 + c3) * (1.0 / 6.0)
        v = 1.0 - t
        lo, hi = fma(E, v, F * t), fma(H, t, G * v)
        return fma(lo * v, v, (hi * t) * t)

    @staticmethod
    def to_int(u):
        """(int)u of the device: truncation, saturating, NaN -> 0"""
        if u != u:
            return 0
        if u >= 2147483647.0:
            return 2147483647
        if u <= -2147483648.0:
            return -2147483648
        return int(u)

    @classmethod
    def locate_term(cls, u, n_basis):
        k = max(0, min(cls.to_int(u), n_basis - 4))
        return k, u - float(k)

    @classmethod
    def locate(cls, x, lo, inv_dx, n_basis):
        return cls.locate_term((x - lo) * inv_dx, n_basis)

    @classmethod
    def locate_knot(cls, u):
        return cls.to_int(u), u - math.floor(u)  # v_fract_f64 on [0, n_int)

    def binades_of(self, m):
        return int(round(clamp(m, -7.0e5, 7.0e5) * self.log2e))

    # ---- wave reductions: the DPP network lane by lane (numpy arrays of 64)
    @staticmethod
    def _row_shr(v, k, fill):
        lane = np.arange(64)
        src = lane - k
        ok = (src // 16) == (lane // 16)
        return np.where(ok, v[np.where(ok, src, lane)], fill), np.ones(64, dtype=bool)

    @staticmethod
    def _row_bcast(v, last_lane_of, rows):
        lane = np.arange(64)
        written = np.isin(lane // 16, rows)
        src = (lane // 16) * 16 - 1 if last_lane_of == 15 else np.full(64, 31)
        return v[np.clip(src, 0, 63)], written

    @classmethod
    def _tree(cls, v, combine, fill):
        v = np.array(v, dtype=np.float64)
        for k in (1, 2, 4, 8):
            got, _ = cls._row_shr(v, k, fill)
            v = combine(v, got)
        got, written = cls._row_bcast(v, 15, [1, 3])
        v = np.where(written, combine(v, got), v)
        got, written = cls._row_bcast(v, 31, [2, 3])
        v = np.where(written, combine(v, got), v)
        return float(v[63])

    @classmethod
    def wave_sum(cls, v):
        return cls._tree(v, lambda a, b: a + b, 0.0)

    @classmethod
    def wave_max(cls, v):
        return cls._tree(v, np.fmax, 0.0)

    @staticmethod
    def wave_max_coarse(v):
        with np.errstate(over="ignore"):
            return float(np.max(np.asarray(v, dtype=np.float64).astype(np.float32)))

    @staticmethod
    def wave_sum8(V):
        """V[lane][slot] -> what each of the 64 lanes returns"""
        V = np.asarray(V, dtype=np.float64)
        lane = np.arange(64)
        lo = lane < 32
        x = [np.where(lo, V[lane % 32, j] + V[lane % 32 + 32, j], V[lane % 32, j + 4] + V[lane % 32 + 32, j + 4]) for j in range(4)]
        first = (lane % 32) < 16
        base = lane - (lane % 32) + (lane % 16)
        y = [np.where(first, x[j][base] + x[j][base + 16], x[j + 2][base] + x[j + 2][base + 16]) for j in range(2)]
        up = (lane & 8) != 0
        keep, send = np.where(up, y[1], y[0]), np.where(up, y[0], y[1])
        z = keep + send[lane ^ 8]
        z = z + z[(lane & ~7) + 7 - (lane & 7)]
        z = z + z[lane ^ 1]
        z = z + z[lane ^ 2]
        return z
