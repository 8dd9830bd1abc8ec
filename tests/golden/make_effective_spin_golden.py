"""Generate tests/golden/effective_spins.npz from the UNMODIFIED reference (preprocess/priors.py, preprocess/conversions.py, imported
by file path under a bare stand-in package: the package's own __init__ pulls in xarray and arviz, these two files need NumPy and
SciPy only) and from mpmath at 50 digits.      python tests/golden/make_effective_spin_golden.py

(i)   closed forms: N_RANDOM random component-spin samples (q in (0.05, 1), a in (0, 1), cos tilt in (-1, 1)) and hand-placed ones --
      chi_eff exactly 0, exactly on every case boundary as the reference computes the boundary, |chi_eff| >= a_max, chi_p on its case
      boundary and >= a_max -- for a_max in {1.0, 0.8}, and a float32-valued copy of the random inputs (a_max = 1).  Random samples
      within 1e-6 of a boundary are masked out; hand-placed samples go through SCALAR calls of the isotropic prior, the only way the
      reference's boundary fallback works.
(ii)  the same priors at 50 digits (mpmath.polylog), evaluated at the reference's float64 chi_eff / chi_p, and E: the reference's own
      largest relative deviation from them, per prior.
(iii) the conditional prior p(chi_p | chi_eff, q): 24 points with |chi_eff| <= 0.5, each evaluated by the reference under
      np.random.seed(s) for 64 seeds at ndraws = 10000: mean and standard deviation per point."""
import importlib.util
import os
import sys
import types

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_import import REFERENCE_ROOT  # noqa: E402

N_RANDOM = 4096
A_MAXES = (1.0, 0.8)
N_SEEDS = 64
mp.mp.dps = 50


def load_priors():
    if not hasattr(np, "trapz"):  # (the reference predates NumPy 2.4)
        np.trapz = np.trapezoid
    pkg = types.ModuleType("refpre")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "gwinferno", "preprocess")]
    sys.modules["refpre"] = pkg
    mods = {}
    for name in ("conversions", "priors"):
        spec = importlib.util.spec_from_file_location(f"refpre.{name}", os.path.join(pkg.__path__[0], f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refpre.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["priors"], mods["conversions"]


P, CV = load_priors()


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------
def li2(x):
    return mp.re(mp.polylog(2, x))


def hp_iso_open(x, q, A):
    """The open form at x = |chi_eff| (mp numbers); None on a boundary."""
    if x == 0:
        return (1 + q) / (2 * A) * (2 - mp.log(q))
    if x >= A:
        return mp.mpf(0)
    b1, b2, b3 = A * (1 - q) / (1 + q), q * A / (1 + q), A / (1 + q)
    s, qA, lA = (1 + q) * x, q * A, mp.log(A)
    pref = (1 + q) / (4 * q * A**2)
    if x < b1 and x < b2:
        t = qA * (4 + 2 * lA - mp.log(qA**2 - s**2)) - 2 * s * mp.atanh(s / qA) + s * (li2(-qA / s) - li2(qA / s))
    elif x < b1 and x > b2:
        t = 4 * qA + 2 * qA * lA - 2 * s * mp.atanh(qA / s) - qA * mp.log(s**2 - qA**2) + s * (li2(-qA / s) - li2(qA / s))
    elif x > b1 and x < b2:
        t = (2 * (1 + q) * (A - x) - s * lA**2 + (A + s * mp.log(s)) * mp.log(qA / (A - s)) - s * lA * (2 + mp.log(q) - mp.log(A - s)) + qA * mp.log(A / (qA - s))
             + s * mp.log((A - s) * (qA - s) / q) + s * (li2(1 - A / s) - li2(qA / s)))
    elif x > b1 and x < b3 and x >= b2:
        t = (-x * lA**2 + 2 * (1 + q) * (A - x) + qA * mp.log(A / (s - qA)) + A * mp.log(qA / (A - s)) - x * lA * (2 * (1 + q) - mp.log(s) - q * mp.log(s / A))
             + s * mp.log((s - qA) * (A - s) / q) + s * mp.log(A / s) * mp.log((A - s) / q) + s * (li2(1 - A / s) - li2(qA / s)))
    elif x > b1 and x > b3 and x < A:
        t = (2 * (1 + q) * (A - x) - s * lA**2 + lA * (A - 2 * s - s * mp.log(q / (s - A))) - A * mp.log((s - A) / q) + s * mp.log((s - A) * (s - qA) / q)
             + s * mp.log(s) * mp.log(qA / (s - A)) - qA * mp.log((s - qA) / A) + s * (li2(1 - A / s) - li2(qA / s)))
    else:
        return None
    return pref * t


def hp_iso(chi_eff, q, A, on_boundary):
    """At the float64 chi_eff.  A sample the reference treats as a boundary (decided in float64) is the mean at +-1e-6."""
    x, q, A = abs(mp.mpf(float(chi_eff))), mp.mpf(float(q)), mp.mpf(float(A))
    if on_boundary:
        hi, lo = float(abs(chi_eff)) + 1e-6, abs(float(abs(chi_eff)) - 1e-6)  # the float64 arguments the fallback evaluates
        return float((hp_iso_open(mp.mpf(hi), q, A) + hp_iso_open(mp.mpf(lo), q, A)) / 2)
    v = hp_iso_open(x, q, A)
    return float(v)


def hp_aligned(chi_eff, q, A):
    x, q, A = mp.mpf(float(chi_eff)), mp.mpf(float(q)), mp.mpf(float(A))
    b1 = A * (1 - q) / (1 + q)
    if b1 < x <= A:
        return float((1 + q) ** 2 * (A - x) / (4 * q * A**2))
    if -A <= x < -b1:
        return float((1 + q) ** 2 * (A + x) / (4 * q * A**2))
    if -b1 <= x <= b1:
        return float((1 + q) / (2 * A))
    return 0.0


def hp_chi_p(chi_p, q, A):
    x, q, A = mp.mpf(float(chi_p)), mp.mpf(float(q)), mp.mpf(float(A))
    f = (3 + 4 * q) / (4 + 3 * q)
    if x < q * A * f:
        u = x / (f * q * A)
        return float(1 / (A**2 * q) / f * (mp.acos(u) * (A - mp.sqrt(A**2 - x**2) + x * mp.acos(x / A)) + mp.acos(x / A) * (A * q * f - mp.sqrt((A * q * f) ** 2 - x**2) + x * mp.acos(u))))
    if x < A:
        return float(mp.acos(x / A) / A)
    return 0.0


# ---- the reference, case by case ---------------------------------------------------------------------------------------------
def thresholds(q, A):
    return A * (1.0 - q) / (1.0 + q), q * A / (1.0 + q), A / (1.0 + q)


def ref_case(chi_eff, q, A):
    """The reference's case tests (priors.py:102-108) on scalars: 'Z', 'A'..'F' or None (its boundary fallback)."""
    x = abs(chi_eff)
    b1, b2, b3 = thresholds(q, A)
    tests = [("Z", x == 0), ("A", x > 0 and x < b1 and x < b2), ("B", x < b1 and x > b2), ("C", x > b1 and x < b2), ("D", x > b1 and x < b3 and x >= b2),
             ("E", x > b1 and x > b3 and x < A), ("F", x >= A)]
    hit = [n for n, t in tests if t]
    return hit[0] if hit else None


def near_boundary(chi_eff, q, A, width=1e-6):
    x = np.abs(chi_eff)
    b1, b2, b3 = thresholds(q, A)
    return (np.abs(x - b1) < width) | (np.abs(x - b2) < width) | (np.abs(x - b3) < width) | (np.abs(x - A) < width) | (x < width)


def place_on(target, q, sign):
    """(a1, ct1) with a2 = 0 such that the reference's chi_eff == sign * target exactly, or None."""
    guess = target * (1.0 + q)
    for k in range(-6, 7):
        a1 = guess
        for _ in range(abs(k)):
            a1 = np.nextafter(a1, np.inf if k > 0 else -np.inf)
        if 0.0 <= a1 <= 1.0 and CV.chieff_from_q_component_spins(q, a1, 0.0, float(sign), 0.0) == sign * target:
            return float(a1)
    return None


def hand_placed(A):
    rows = []  # (q, a1, a2, ct1, ct2)
    for q in (0.5, 0.25, 0.3, 0.75, 0.9, 1.0):
        rows.append((q, 0.3, 0.4, 0.0, 0.0))  # chi_eff == 0
        b1, b2, b3 = thresholds(q, A)
        for target in (b1, b2, b3):
            for sign in (1, -1):
                a1 = place_on(target, q, sign)
                if a1 is not None and target > 0.0 and ref_case(sign * target, q, A) is None:  # (b2 above b1 is the closed end of case D, no boundary)
                    rows.append((q, a1, 0.0, float(sign), 0.0))
        top = min(1.0, A * 1.1)
        rows.append((q, top, top, 1.0, 1.0))    # |chi_eff| >= a_max (== a_max for a_max = 1)
        rows.append((q, top, top, -1.0, -1.0))
        edge = q * A * (3.0 + 4.0 * q) / (4.0 + 3.0 * q)
        if edge <= 1.0:
            rows.append((q, edge, 0.0, 0.0, 0.0))  # chi_p on its case boundary
        rows.append((q, top, 0.0, 0.0, 0.0))    # chi_p >= a_max
    return np.array(rows).T.copy()


def reference_outputs(cols, A, scalar_iso):
    q, a1, a2, ct1, ct2 = cols
    chi_eff = CV.chieff_from_q_component_spins(q, a1, a2, ct1, ct2)
    chi_p = CV.chip_from_q_component_spins(q, a1, a2, ct1, ct2)
    if scalar_iso:
        iso = np.array([float(P.chi_effective_prior_from_isotropic_spins(float(c), float(qq), a_max=A)[0]) for c, qq in zip(chi_eff, q)])
    else:
        iso = P.chi_effective_prior_from_isotropic_spins(chi_eff, q, a_max=A)
    return chi_eff, chi_p, iso, P.chi_effective_prior_from_aligned_spins(chi_eff, q, a_max=A), P.chi_p_prior_from_isotropic_spins(chi_p, q, a_max=A)


def hp_outputs(chi_eff, chi_p, q, A, cases):
    iso = np.array([hp_iso(c, qq, A, cs == "boundary") for c, qq, cs in zip(chi_eff, q, cases)])
    return iso, np.array([hp_aligned(c, qq, A) for c, qq in zip(chi_eff, q)]), np.array([hp_chi_p(c, qq, A) for c, qq in zip(chi_p, q)])


def rel_dev(ref, hp, keep):
    m = keep & (hp != 0.0)
    return float(np.max(np.abs(ref[m] - hp[m]) / np.abs(hp[m]))) if m.any() else 0.0


def closed_forms(out):
    rng = np.random.default_rng(20260401)
    cols = np.stack([rng.uniform(0.05, 1.0, N_RANDOM), rng.uniform(0.0, 1.0, N_RANDOM), rng.uniform(0.0, 1.0, N_RANDOM), rng.uniform(-1.0, 1.0, N_RANDOM),
                     rng.uniform(-1.0, 1.0, N_RANDOM)])
    cols32 = cols.astype(np.float32)
    out["random_inputs"] = cols
    out["random_inputs_f32"] = cols32
    E = {"iso": 0.0, "aligned": 0.0, "chi_p": 0.0}
    for A in A_MAXES:
        tag = f"{A:g}"
        sets = [("random", cols, False)] + ([("random_f32", cols32.astype(np.float64), False)] if A == 1.0 else []) + [("hand", hand_placed(A), True)]
        for name, c, scalar in sets:
            chi_eff, chi_p, iso, ali, pcp = reference_outputs(c, A, scalar)
            cases = np.array([ref_case(float(x), float(qq), A) or "boundary" for x, qq in zip(chi_eff, c[0])])
            keep = np.ones(c.shape[1], dtype=bool) if scalar else ~near_boundary(chi_eff, c[0], A)
            if name == "hand":
                out[f"hand_inputs_{tag}"] = c
            if A == 1.0 or name == "hand":
                out[f"{name}_chi_eff_{tag}"], out[f"{name}_chi_p_{tag}"] = chi_eff, chi_p
            out[f"{name}_ref_{tag}"] = np.stack([iso, ali, pcp])
            out[f"{name}_keep_{tag}"] = keep
            out[f"{name}_case_{tag}"] = cases
            assert np.all(np.isfinite(np.stack([iso, ali, pcp])[:, keep])), (name, A)
            if name != "random_f32":
                hp = np.stack(hp_outputs(chi_eff, chi_p, c[0], A, cases))
                out[f"{name}_hp_{tag}"] = hp
                for k, key in enumerate(("iso", "aligned", "chi_p")):
                    E[key] = max(E[key], rel_dev(np.stack([iso, ali, pcp])[k], hp[k], keep))
            counts = {k: int(np.sum((cases == k) & keep)) for k in "ABCDE"}
            print(f"a_max {A} {name}: {c.shape[1]} samples, kept {int(keep.sum())}, cases {counts}, boundary {int(np.sum(cases == 'boundary'))}")
            if name == "random":
                assert min(counts.values()) >= 32, counts
    out["E_names"] = np.array(["iso", "aligned", "chi_p"])
    out["E"] = np.array([E["iso"], E["aligned"], E["chi_p"]])
    print("E (largest relative deviation of the reference from the 50-digit values):", E)


def conditional(out):
    rng = np.random.default_rng(20260402)
    pts = []
    while len(pts) < 24:
        q, chi_eff = rng.uniform(0.3, 1.0), rng.uniform(-0.5, 0.5)
        reach = (1.0 + q) * abs(chi_eff)
        top = 1.0 if reach / q < 1.0 else np.sqrt(1.0 - (reach - q) ** 2)
        pts.append((rng.uniform(0.1, 0.85) * top, chi_eff, q))
    pts[0] = (0.3, 0.1, 0.7)
    pts = np.array(pts)
    vals = np.empty((len(pts), N_SEEDS))
    for i, (cp, ce, q) in enumerate(pts):
        for s in range(N_SEEDS):
            np.random.seed(s)
            vals[i, s] = float(P.chi_p_prior_given_chi_eff_q(cp, ce, q, a_max=1.0, ndraws=10000))
        print(f"conditional point {i}: {pts[i]} mean {vals[i].mean():.5f} sd {vals[i].std(ddof=1):.5f}", flush=True)
    out["cond_points"] = pts
    out["cond_mean"] = vals.mean(axis=1)
    out["cond_sd"] = vals.std(axis=1, ddof=1)
    out["cond_n_seeds"] = np.array(N_SEEDS)


def beta_helpers(out):
    alpha, beta = np.array([0.5, 2.0, 3.5, 10.0]), np.array([1.5, 2.0, 0.7, 4.0])
    mu, var = CV.mu_var_from_alpha_beta(alpha, beta, xmax=0.9)
    a2, b2 = CV.alpha_beta_from_mu_var(mu.copy(), var.copy(), xmax=0.9)
    out["beta_alpha_beta"], out["beta_mu_var"], out["beta_roundtrip"] = np.stack([alpha, beta]), np.stack([mu, var]), np.stack([a2, b2])


def main():
    out = {}
    closed_forms(out)
    beta_helpers(out)
    conditional(out)
    path = os.path.join(HERE, "effective_spins.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
