"""Generator of tests/golden/terms_hp.npz: term-level log-densities and their hyper-parameter derivatives at >= 50 digits.

Every density is written here from its definition in the reference (gwinferno/distributions.py: powerlaw_pdf :100-119,
truncnorm_pdf :122-143, betadist :146-162, smooth :16-21; models/parametric/parametric.py: plpeak_primary_pdf :49-53,
plpeak_primary_ratio_pdf :39-46, mixture_isoalign_spin_tilt :84-86, default_spin_tilt :97-102) in mpmath, with analytic
derivatives, and rounded ONCE to float64.  Nothing of gwinferno_amd/ or oracle/ is imported: the fixture is the
independent side of tests/test_terms_hp_cpu.py and tests/test_gpu_terms_hp.py.

    python tests/golden/make_terms_hp.py            # rewrites terms_hp.npz (and checks the working precision)

Conventions
  * Inputs are float64 numbers and enter the arithmetic exactly (mpf(double) is exact); the exponent sweep is built as
    ``-1.0 + e`` in float64 and the double that results is what the fixture records and what mpmath sees.
  * WHETHER a sample is in the support is decided the way the reference decides it, by comparing doubles (``q < mmin / m1``
    with the quotient rounded to float64); the VALUE inside the support is exact.
  * The taper ``smooth`` is the reference's expression as IEEE arithmetic evaluates it: S = 1 / (1 + exp(d/y + d/(y - d))) for
    every y, with S = 0 where a denominator is +0 (y == 0, y == d: d/+0 = +inf).
  * A density that rounds to zero in float64 (log p < log 2^-1075) is stored as -inf: that is what "excluded" means to the
    reference (a zero weight) and to the engine.  No finite value below -650 (a density of 1e-282) is stored, ``_compute`` asserts
    it: next to the bottom of the float64 range 1/p, which every gradient of a mixture needs, overflows or meets subnormals, and
    the engine documents 1e-290 as the density below which a mixture's gradient counts as zero (gwi_device.h, kRcpFloor).  The
    sample vectors and hyper-points are chosen so that nothing falls between the two.
  * m1 == mmin in the mass-ratio power law: low == high == 1, the reference's normaliser is (1+beta)/0 -- a NaN / inf weight, which
    counts as zero.  Stored as -inf.
  * Derivatives of excluded samples are stored as 0.
  * Working precision: DPS digits; ``generate(verify=True)`` repeats everything at 2 x DPS and asserts that the rounded doubles do
    not change.
"""
import os

import mpmath as mp
import numpy as np

DPS = 80
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "terms_hp.npz")

MMIN, MMAX = 5.0, 100.0
SWEEP_E = [0.0] + [s * e for e in (2.0**-52, 1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1) for s in (1.0, -1.0)]
SWEEP = [-1.0 + e for e in SWEEP_E]  # float64 arithmetic: the doubles the fixture records
LOG_TINY = -745.14  # log(2^-1075): below it a density rounds to zero in float64
LOG_FLOOR = -650.0


def F(x):
    return mp.mpf(float(x))


# ---------------------------------------------------------------------------------------------------------------------
# normalisers
# ---------------------------------------------------------------------------------------------------------------------
def pl_lognorm(alpha, lo, hi):
    """log A and d log A / d alpha of A = (1+alpha) / (hi^(1+alpha) - lo^(1+alpha)); alpha == -1: A = 1 / log(hi/lo)."""
    a1 = 1 + alpha
    llo, lhi = mp.log(lo), mp.log(hi)
    if a1 == 0:
        return -mp.log(lhi - llo), -(lhi + llo) / 2
    ph, pw = mp.exp(a1 * lhi), mp.exp(a1 * llo)
    return mp.log(a1 / (ph - pw)), 1 / a1 - (ph * lhi - pw * llo) / (ph - pw)


def tn_lognorm(mu, sg, lo, hi):
    """log C, dlogC/dmu, dlogC/dsig of C = 1 / (sig sqrt(2 pi) (Phi(b) - Phi(a)))."""
    a, b = (lo - mu) / sg, (hi - mu) / sg
    D = (mp.erf(b / mp.sqrt(2)) - mp.erf(a / mp.sqrt(2))) / 2
    pa, pb = mp.npdf(a), mp.npdf(b)
    return -mp.log(sg) - mp.log(2 * mp.pi) / 2 - mp.log(D), (pb - pa) / (sg * D), -1 / sg + (b * pb - a * pa) / (sg * D)


def taper(y, dl):
    """S and d log S / d delta."""
    if y == 0 or y == dl:
        return mp.mpf(0), mp.mpf(0)
    u = dl / y + dl / (y - dl)
    E = mp.exp(u)
    S = 1 / (1 + E)
    return S, -(E * S) * (1 / y + y / (y - dl) ** 2)


# ---------------------------------------------------------------------------------------------------------------------
# terms: fn(theta (mpf list), prepared hyper-point state, sample (tuple of float64)) -> None (excluded) | (logp, [dlogp])
# ---------------------------------------------------------------------------------------------------------------------
def powerlaw_prep(th):
    return pl_lognorm(th[0], F(MMIN), F(MMAX))


def powerlaw_eval(th, st, x):
    (m,) = x
    if m < MMIN or m > MMAX:
        return None
    lx = mp.log(F(m))
    return th[0] * lx + st[0], [lx + st[1]]


def plpeak_prep(th):
    alpha, mpp, sig = th[0], th[1], th[2]
    return pl_lognorm(alpha, F(MMIN), F(MMAX)), tn_lognorm(mpp, sig, F(MMIN), F(MMAX))


def _plpeak_parts(th, st, m, delta=None):
    """(p, [dp/dalpha, dp/dmpp, dp/dsig, dp/dlam(, dp/ddelta)]) of the PL+Peak mixture at one in-support m."""
    alpha, mpp, sig, lam = th[0], th[1], th[2], th[3]
    (la, dla), (lc, dmu, dsg) = st
    x = F(m)
    lx = mp.log(x)
    PL = mp.exp(alpha * lx + la)
    TN = mp.exp(-((x - mpp) ** 2) / (2 * sig**2) + lc)
    out_extra = []
    if delta is not None:
        S, dlogS = taper(x - F(MMIN), delta)
        PL = PL * S
        out_extra = [(1 - lam) * PL * dlogS]
    p = (1 - lam) * PL + lam * TN
    dp = [(1 - lam) * PL * (lx + dla), lam * TN * ((x - mpp) / sig**2 + dmu), lam * TN * ((x - mpp) ** 2 / sig**3 + dsg), TN - PL] + out_extra
    return p, dp


def _log_and_ratio(p, dp):
    if p == 0 or mp.log(p) < LOG_TINY:
        return None
    return mp.log(p), [d / p for d in dp]


def plpeak_eval(th, st, x):
    (m,) = x
    if m < MMIN or m > MMAX:
        return None
    return _log_and_ratio(*_plpeak_parts(th, st, m))


def plpeak_smooth_prep(th):
    return plpeak_prep(th)


def plpeak_smooth_eval(th, st, x):
    (m,) = x
    if m < MMIN or m > MMAX:
        return None
    return _log_and_ratio(*_plpeak_parts(th, st, m, delta=th[4]))


def ratio_eval(th, st, x):
    """powerlaw_pdf(q, beta, mmin / m1, 1)."""
    q, m = x
    low = MMIN / m  # float64, as the reference forms it
    if q < low or q > 1.0 or low == 1.0:
        return None
    la, dla = pl_lognorm(th[0], F(MMIN) / F(m), mp.mpf(1))
    lq = mp.log(F(q))
    return th[0] * lq + la, [lq + dla]


def plpeak_ratio_prep(th):  # theta = (alpha, beta, mpp, sigpp, lam)
    return plpeak_prep([th[0], th[2], th[3], th[4]])


def plpeak_ratio_eval(th, st, x):
    m, q = x
    a = plpeak_eval([th[0], th[2], th[3], th[4]], st, (m,))
    b = ratio_eval([th[1]], None, (q, m))
    if a is None or b is None:
        return None
    return a[0] + b[0], [a[1][0], b[1][0], a[1][1], a[1][2], a[1][3]]


def tilt_prep(th):
    return tn_lognorm(mp.mpf(1), th[1], mp.mpf(-1), mp.mpf(1))


def tilt_eval(th, st, x):
    (c,) = x
    if c > 1.0 or c < -1.0:
        return None
    xi, sg = th
    lc, _, dsg = st
    d = F(c) - 1
    TN = mp.exp(-(d**2) / (2 * sg**2) + lc)
    return _log_and_ratio((1 - xi) / 2 + xi * TN, [TN - mp.mpf(1) / 2, xi * TN * (d**2 / sg**3 + dsg)])


def tilt_joint_eval(th, st, x):
    c1, c2 = x
    if c1 > 1.0 or c1 < -1.0 or c2 > 1.0 or c2 < -1.0:
        return None
    xi, sg = th
    lc, _, dsg = st
    r2 = (F(c1) - 1) ** 2 + (F(c2) - 1) ** 2
    A = mp.exp(-r2 / (2 * sg**2) + 2 * lc)
    return _log_and_ratio((1 - xi) / 4 + xi * A, [A - mp.mpf(1) / 4, xi * A * (r2 / sg**3 + 2 * dsg)])


def beta_prep(th):
    a, b = th
    return mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b), mp.digamma(a + b) - mp.digamma(a), mp.digamma(a + b) - mp.digamma(b)


def beta_eval(th, st, x):
    (v,) = x
    if not (0.0 < v < 1.0):  # the ends: (alpha-1) log 0 is -inf, +inf or NaN -- a zero, infinite or NaN weight, excluded alike
        return None
    a, b = th
    l0, l1 = mp.log(F(v)), mp.log(1 - F(v))
    return (a - 1) * l0 + (b - 1) * l1 - st[0], [l0 + st[1], l1 + st[2]]


TN_LO, TN_HI = 0.0, 1.0


def truncnorm_prep(th):
    return tn_lognorm(th[0], th[1], F(TN_LO), F(TN_HI))


def truncnorm_eval(th, st, x):
    (v,) = x
    if v > TN_HI or v < TN_LO:
        return None
    mu, sg = th
    lc, dmu, dsg = st
    d = F(v) - mu
    return -(d**2) / (2 * sg**2) + lc, [d / sg**2 + dmu, d**2 / sg**3 + dsg]


# ---------------------------------------------------------------------------------------------------------------------
# samples (built with IEEE +, *, / and nextafter only: the same doubles everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def _geometric(first, ratio, n):
    out, v = [], first
    for _ in range(n):
        out.append(v)
        v = v * ratio
    return out


def m1_samples():
    bulk = _geometric(5.3, 1.1375, 23)  # 5.3 .. 90.2
    edge = [MMIN, np.nextafter(MMIN, 200.0), np.nextafter(MMIN, 0.0), MMAX, np.nextafter(MMAX, 0.0), np.nextafter(MMAX, 200.0), 4.0, 120.0, 99.5]
    return np.array(bulk + edge, dtype=np.float64)


def ratio_samples():
    """(m1, q).  m1: the bulk of m1_samples(), m1 == mmin and the out-of-range values.  The nextafter neighbours of mmin are left
    out ON PURPOSE: there log p = -log(log(m1/mmin)) + ... has a condition number of 1 / log(m1/mmin) ~ 1e16 with respect to m1,
    so half an ulp of the INPUT moves it by O(1); the engine's log m1 column (|error| <= 1 ulp of log m1 ~ 9e-16) holds the 1e-11 bar
    for log(m1/mmin) > ~1e-4, and the smallest bulk value, 5.3, has 0.058."""
    bulk = _geometric(5.3, 1.1375, 23)
    m1, q = [], []
    for k, m in enumerate(bulk):
        low = MMIN / m
        f = ((k + 1) * 0.6180339887498949) % 1.0
        m1.append(m)
        q.append(low + (1.0 - low) * (0.02 + 0.96 * f))
    for m, qq in ((bulk[3], 1.0), (bulk[7], MMIN / bulk[7]), (bulk[7], np.nextafter(MMIN / bulk[7], 1.0)), (bulk[7], np.nextafter(MMIN / bulk[7], 0.0)),
                  (bulk[20], MMIN / bulk[20]), (bulk[20], np.nextafter(MMIN / bulk[20], 1.0)), (MMIN, 1.0), (MMIN, 0.5), (4.0, 0.9), (120.0, 0.5), (bulk[11], np.nextafter(1.0, 2.0)),
                  (MMAX, 0.3)):
        m1.append(m)
        q.append(qq)
    return np.array(m1, dtype=np.float64), np.array(q, dtype=np.float64)


DELTAS = (0.1, 5.0, 30.0)


def smooth_samples():
    """m1 = mmin + y: y = 0, the smallest y > 0 a double m1 can hold, and for each delta of the sweep delta/2, the neighbours of
    delta, delta itself where mmin + delta is a double, and beyond."""
    out = [MMIN, np.nextafter(MMIN, 200.0), 4.0, 120.0, MMAX]
    for d in DELTAS:
        at = MMIN + d
        out += [MMIN + d / 2, np.nextafter(at, 0.0), at, np.nextafter(at, 200.0), MMIN + 1.5 * d, MMIN + 0.9 * d, MMIN + 0.97 * d]
    out += _geometric(5.6, 1.21, 14)  # 5.6 .. 66.7
    return np.array(out, dtype=np.float64)


def ct_samples():
    inner = [-1.0 + 2.0 * (k + 0.8) / 26 for k in range(26)]
    return np.array([-1.0, 1.0, np.nextafter(-1.0, -2.0), np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 0.999] + inner, dtype=np.float64)


def unit_samples(top=np.nextafter(1.0, 0.0)):
    inner = [(k + 0.5) / 26 for k in range(26)]
    return np.array([0.0, 1.0, 1e-6, top, 0.999, 1e-3] + inner, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# hyper-points
# ---------------------------------------------------------------------------------------------------------------------
LAMS = (0.0, 1e-12, 0.5, 1.0 - 1e-12, 1.0)
ORD_MASS = [(-2.5, 1.0, 35.0, 5.0, 0.1), (-3.5, 2.0, 20.0, 1.0, 0.0), (-1.5, 0.0, 50.0, 10.0, 0.2), (-0.3, -2.0, 27.3, 3.3, 0.05), (1.7, 3.1, 42.0, 7.7, 0.15)]  # alpha, beta, mpp, sigpp, lam
SIGPPS = (0.05, 0.33, 5.0, 25.0)


def powerlaw_points():
    # (no alpha = 0: the density is then flat and every log_l of the gradient catalogs exactly 0 -- nothing a relative bar can hold)
    return [("ordinary", (a,)) for a in (-2.5, -3.5, -1.5, 0.4, 1.7, 12.0, -14.0)] + [(f"sweep{e:+.3g}", (a,)) for e, a in zip(SWEEP_E, SWEEP)]


def plpeak_points():
    pts = [("ordinary", (a, mpp, s, lam)) for a, _, mpp, s, lam in ORD_MASS]
    pts += [(f"sweep{e:+.3g}", (a, 35.0, 5.0, 0.1)) for e, a in zip(SWEEP_E, SWEEP)]
    pts += [(f"lam{lam:g}", (-2.5, 35.0, 5.0, lam)) for lam in LAMS]
    pts += [(f"lam{lam:g}/sweep-1e-10", (-1.0 - 1e-10, 35.0, 5.0, lam)) for lam in (0.0, 1.0)]
    pts += [(f"sigpp{s:g}", (-2.5, 35.0, s, 0.1)) for s in SIGPPS]
    pts += [("sigpp0.05/sweep+1e-8", (-1.0 + 1e-8, 35.0, 0.05, 0.3))]
    return pts


def ratio_points():
    return [("ordinary", (b,)) for b in (1.0, 2.0, 0.0, -2.0, 3.1, -3.5, 8.0)] + [(f"sweep{e:+.3g}", (b,)) for e, b in zip(SWEEP_E, SWEEP)]


def plpeak_ratio_points():
    pts = [("ordinary", p) for p in ORD_MASS]
    pts += [(f"beta-sweep{e:+.3g}", (-2.5, b, 35.0, 5.0, 0.1)) for e, b in zip(SWEEP_E, SWEEP)]
    # alpha and beta both next to -1, from opposite sides
    pts += [(f"alpha-sweep{e:+.3g}", (a, SWEEP[len(SWEEP) - 1 - i], 35.0, 5.0, 0.1)) for i, (e, a) in enumerate(zip(SWEEP_E, SWEEP)) if i % 2 == 0]
    pts += [(f"lam{lam:g}", (-1.0 + 1e-6, -1.0 - 1e-6, 35.0, 5.0, lam)) for lam in LAMS]
    return pts


def plpeak_smooth_points():
    pts = [("ordinary", (a, mpp, s, lam, d)) for (a, _, mpp, s, lam), d in zip(ORD_MASS, (3.0, 1.0, 8.0, 5.5, 2.2))]
    pts += [(f"delta{d:g}/lam{lam:g}", (-2.5, 35.0, 5.0, lam, d)) for d in DELTAS for lam in (0.0, 0.1, 1.0)]
    pts += [(f"delta{d:g}/sweep{e:+.3g}", (-1.0 + e, 35.0, 5.0, 0.1, d)) for d in DELTAS for e in (0.0, 1e-10, -1e-6, 2.0**-52)]
    return pts


def tilt_points():
    pts = [("ordinary", p) for p in ((0.7, 1.3), (0.2, 0.4), (0.95, 3.7))]
    # (not xi = 1 with sig_t = 0.05: the pure peak, 40 sigma wide across the interval, puts samples anywhere between e^-650 and 2^-1075)
    pts += [(f"xi{xi:g}/sig{s:g}", (xi, s)) for xi in LAMS for s in (0.05, 1.0, 6.0) if not (xi == 1.0 and s == 0.05)]
    return pts


def beta_points():
    # (the Beta term works in the log domain and never forms the density: its sample vector stops at 0.9999, where Beta(50, 80) is
    # still e^-639, so that "rounds to zero in float64" is not asked of it)
    return [("ordinary", p) for p in ((1.7, 4.2), (2.9, 1.1), (1.3, 2.6))] + [(f"a{a:g}/b{b:g}", (a, b)) for a, b in ((1.0, 1.0), (1e-2, 3.0), (50.0, 80.0))]


def truncnorm_points():
    pts = []
    for s in (0.05, 0.3, 2.0):
        pts += [(f"sig{s:g}/inside", (0.4, s)), (f"sig{s:g}/at-lo", (0.0, s)), (f"sig{s:g}/+2sig", (1.0 + 2 * s, s)), (f"sig{s:g}/-2sig", (0.0 - 2 * s, s)),
                (f"sig{s:g}/+4sig", (1.0 + 4 * s, s)), (f"sig{s:g}/-4sig", (0.0 - 4 * s, s))]
    return pts


def terms():
    m1 = m1_samples()
    rm, rq = ratio_samples()
    ct = ct_samples()
    # second tilt column: the first one reversed in its bulk, so that (ct1, ct2) cover the square and each end meets an inner value
    ct2 = np.concatenate([ct[:6][::-1], ct[6:][::-1]])
    return {
        "powerlaw": dict(params=["alpha"], cols={"m1": m1}, points=powerlaw_points(), prep=powerlaw_prep, fn=powerlaw_eval),
        "plpeak": dict(params=["alpha", "mpp", "sigpp", "lam"], cols={"m1": m1}, points=plpeak_points(), prep=plpeak_prep, fn=plpeak_eval),
        "plpeak_ratio": dict(params=["alpha", "beta", "mpp", "sigpp", "lam"], cols={"m1": rm, "q": rq}, points=plpeak_ratio_points(), prep=plpeak_ratio_prep, fn=plpeak_ratio_eval),
        "ratio": dict(params=["beta"], cols={"q": rq, "m1": rm}, points=ratio_points(), prep=lambda th: None, fn=ratio_eval),
        "plpeak_smooth": dict(params=["alpha", "mpp", "sigpp", "lam", "delta"], cols={"m1": smooth_samples()}, points=plpeak_smooth_points(), prep=plpeak_smooth_prep,
                              fn=plpeak_smooth_eval),
        "tilt": dict(params=["xi", "sig_t"], cols={"ct": ct}, points=tilt_points(), prep=tilt_prep, fn=tilt_eval),
        "tilt_joint": dict(params=["xi", "sig_t"], cols={"ct1": ct, "ct2": ct2}, points=tilt_points(), prep=tilt_prep, fn=tilt_joint_eval),
        "beta": dict(params=["a", "b"], cols={"a": unit_samples(top=0.9999)}, points=beta_points(), prep=beta_prep, fn=beta_eval),
        "truncnorm": dict(params=["mu", "sig"], cols={"x": unit_samples()}, points=truncnorm_points(), prep=truncnorm_prep, fn=truncnorm_eval),
    }


def _compute(dps):
    out = {}
    with mp.workdps(dps):
        for name, t in terms().items():
            cols = list(t["cols"].values())
            n, P = len(cols[0]), len(t["params"])
            theta = np.array([p for _, p in t["points"]], dtype=np.float64)
            logp = np.full((len(theta), n), -np.inf)
            dlogp = np.zeros((len(theta), P, n))
            for h, th_d in enumerate(theta):
                th = [F(v) for v in th_d]
                st = t["prep"](th)
                for i in range(n):
                    r = t["fn"](th, st, tuple(float(c[i]) for c in cols))
                    if r is None or r[0] < LOG_TINY:
                        continue
                    assert r[0] > LOG_FLOOR, (name, t["points"][h][0], i, float(r[0]))
                    logp[h, i] = float(r[0])
                    dlogp[h, :, i] = [float(d) for d in r[1]]
            out[f"{name}/params"] = np.array(t["params"])
            out[f"{name}/columns"] = np.array(list(t["cols"].keys()))
            for k, c in t["cols"].items():
                out[f"{name}/col/{k}"] = c
            out[f"{name}/tags"] = np.array([tag for tag, _ in t["points"]])
            out[f"{name}/theta"] = theta
            out[f"{name}/logp"] = logp
            out[f"{name}/dlogp"] = dlogp
    return out


def generate(verify=True):
    """The fixture's arrays.  ``verify``: compute them again with twice the digits and assert that no double changes."""
    out = _compute(DPS)
    if verify:
        again = _compute(2 * DPS)
        for k, v in out.items():
            assert np.array_equal(v, again[k]), f"{k}: {DPS} digits are not enough"
    return out


if __name__ == "__main__":
    arrays = generate(verify=True)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays")
