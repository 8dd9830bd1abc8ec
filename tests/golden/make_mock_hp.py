"""Generator of tests/golden/mock_hp.npz: the arithmetic of the mock-catalog observation model ("Mock catalogs") at 40
digits -- noisy data, truncated-normal posterior samples and the prior column of ONE coordinate -- from fp64 inputs and uniforms.

Nothing of gwinferno_amd/ or oracle/ is imported: the fixture is the independent side of tests/test_mock_catalog_cpu.py and
tests/test_gpu_mock_catalog.py.

    python tests/golden/make_mock_hp.py            # rewrites mock_hp.npz (and checks the working precision)

Conventions
  * Inputs are float64 numbers and enter the arithmetic exactly (mpf(double) is exact).  The T-space support [t_lo, t_hi] is an input
    (log(lo), log(hi) rounded to float64 for a log coordinate), as are the data d, the scale sigma and the uniform u = k 2^-53.
  * Data: d = T(x_true) + sigma Phi^-1(u), u = 0 read as 2^-54.
  * Sample: t = d + sigma Phi^-1(Phi(a) + u (Phi(b) - Phi(a))) with a = (t_lo - d) / sigma, b = (t_hi - d) / sigma formed exactly,
    clamped into [t_lo, t_hi]; x = T^-1(t) clamped into [lo, hi].  t and x are each rounded ONCE to float64.  The normal quantile is
    found by Newton's iteration on log Phi from the Abramowitz-Stegun 26.2.23 start, on the side of the smaller tail.
  * Prior: 1 / (x ln(hi / lo)) for a log coordinate at the float64 x stored, 1 / (hi - lo) for an identity one.
  * Working precision: DPS digits; ``generate(verify=True)`` repeats everything at 2 x DPS and asserts that no double changes.
"""
import os

import mpmath as mp
import numpy as np

DPS = 40
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mock_hp.npz")
N = 150  # draws per regime and transform
SUPPORTS = {"identity": (0.05, 1.0), "log": (2.0, 100.0)}
REGIMES = ("inside", "beyond_lo", "beyond_hi", "narrow", "wide", "u_edge")
U_EDGES = [0.0, 2.0**-53, 2.0**-52, 1.0 - 2.0**-53, 1.0 - 2.0**-52, 0.5, 0.5 - 2.0**-53, 0.5 + 2.0**-53]


def F(x):
    return mp.mpf(float(x))


def log_phi(y):
    """log Phi(y), through erfc of a positive argument for y <= 0."""
    r2 = mp.sqrt(2)
    return mp.log(mp.erfc(-y / r2) / 2) if y <= 0 else mp.log1p(-mp.erfc(y / r2) / 2)


def ppf_lower(logp):
    """y <= 0 with log Phi(y) = logp (logp <= log 1/2)."""
    if logp >= mp.log(mp.mpf(1) / 2):
        return mp.mpf(0)
    t = mp.sqrt(-2 * logp)
    y = -(t - (2.515517 + 0.802853 * t + 0.010328 * t**2) / (1 + 1.432788 * t + 0.189269 * t**2 + 0.001308 * t**3))
    for _ in range(60):
        lp = log_phi(y)
        step = (lp - logp) * mp.exp(lp) / mp.npdf(y)  # Newton on log Phi: d log Phi / dy = phi / Phi
        y = y - step
        if abs(step) < mp.mpf(10) ** (-(mp.mp.dps - 5)) * (1 + abs(y)):
            return y
    raise RuntimeError("ppf_lower did not converge")


def normal_quantile(u):
    u = F(u)
    if u == 0:
        u = mp.mpf(2) ** -54
    return ppf_lower(mp.log(u)) if u <= mp.mpf(1) / 2 else -ppf_lower(mp.log(1 - u))


def truncnorm_quantile(a, b, u):
    """Phi^-1(Phi(a) + u (Phi(b) - Phi(a))), evaluated on the side where the tail is the smaller one."""
    r2 = mp.sqrt(2)
    u = F(u)
    if a > 0:  # work in the mirrored problem: every probability below is then a lower tail
        return -truncnorm_quantile(-b, -a, 1 - u)
    pa = mp.erfc(-a / r2) / 2
    if b <= 0:
        p = pa + u * (mp.erfc(-b / r2) / 2 - pa)
        return a if p == 0 else ppf_lower(mp.log(p))
    qb = mp.erfc(b / r2) / 2
    z = 1 - pa - qb
    low = pa + u * z
    if low <= mp.mpf(1) / 2:
        return a if low == 0 else ppf_lower(mp.log(low))
    up = qb + (1 - u) * z
    return b if up == 0 else -ppf_lower(mp.log(up))


def inputs():
    """The fp64 inputs of every case: built with numpy's generator and IEEE +, *, / only."""
    rng = np.random.default_rng(20260301)
    rows = []
    for tr, (lo, hi) in SUPPORTS.items():
        t_lo, t_hi = (float(np.log(lo)), float(np.log(hi))) if tr == "log" else (lo, hi)
        rng_w = t_hi - t_lo
        for regime in REGIMES:
            k = rng.integers(0, 2**53, N).astype(np.float64) * 2.0**-53
            f = rng.uniform(0.0, 1.0, N)
            sigma = np.full(N, 0.1 * rng_w)
            if regime == "inside":
                d = t_lo + f * rng_w
            elif regime == "beyond_lo":
                d = t_lo - 8.0 * f * sigma
            elif regime == "beyond_hi":
                d = t_hi + 8.0 * f * sigma
            elif regime == "narrow":
                sigma = np.full(N, 1e-6 * rng_w)
                d = np.where(f < 0.5, t_lo + 2.0 * f * rng_w, np.where(f < 0.75, t_lo - 32.0 * (f - 0.5) * sigma, t_hi + 32.0 * (f - 0.75) * sigma))
            elif regime == "wide":
                sigma = np.full(N, 1e2 * rng_w)
                d = t_lo + rng_w / 2 + 16.0 * (f - 0.5) * sigma
            else:
                k = np.array([U_EDGES[i % len(U_EDGES)] for i in range(N)])
                sigma = np.where(np.arange(N) % 3 == 0, 1e-6, np.where(np.arange(N) % 3 == 1, 0.1, 1e2)) * rng_w
                d = t_lo + rng_w / 2 + 16.0 * (f - 0.5) * np.minimum(sigma, rng_w)
            x_true = lo + f * (hi - lo)
            for i in range(N):
                rows.append((tr == "log", regime, lo, hi, t_lo, t_hi, float(sigma[i]), float(d[i]), float(k[i]), float(x_true[i])))
    return rows


def _compute(dps):
    rows = inputs()
    out = {k: [] for k in ("data", "t", "x", "prior")}
    with mp.workdps(dps):
        for is_log, _, lo, hi, t_lo, t_hi, sigma, d, u, x_true in rows:
            sg = F(sigma)
            out["data"].append(float((mp.log(F(x_true)) if is_log else F(x_true)) + sg * normal_quantile(u)))
            a, b = (F(t_lo) - F(d)) / sg, (F(t_hi) - F(d)) / sg
            t = min(max(F(d) + sg * truncnorm_quantile(a, b, u), F(t_lo)), F(t_hi))
            x = min(max(mp.exp(t) if is_log else t, F(lo)), F(hi))
            out["t"].append(float(t))
            out["x"].append(float(x))
            out["prior"].append(float(1 / (F(float(x)) * mp.log(F(hi) / F(lo))) if is_log else 1 / (F(hi) - F(lo))))
    res = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    res["is_log"] = np.array([r[0] for r in rows])
    res["regime"] = np.array([r[1] for r in rows])
    for j, k in enumerate(("lo", "hi", "t_lo", "t_hi", "sigma", "d", "u", "x_true")):
        res[k] = np.array([r[2 + j] for r in rows], dtype=np.float64)
    return res


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
