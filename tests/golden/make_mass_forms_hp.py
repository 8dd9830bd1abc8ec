"""Generator of tests/golden/mass_forms_hp.npz: the three pieces of mass-model arithmetic that the other high-precision fixtures
leave out, at 80 digits -- the power law with SAMPLED bounds, the unnormalised pairing factor of the component-mass models, and the
mass-ratio power law whose m1 is the sample column of a spline fixture.

Every density is written here from its definition in the reference (gwinferno/numpyro_distributions.py: Powerlaw.log_prob :127-136;
gwinferno/models/bsplines/separable.py: BSplineIIDComponentMasses.__call__ :606-613, BSplineIndependentComponentMasses.__call__
:700-703, BSplinePrimaryPowerlawRatio.__call__ :363-365; gwinferno/distributions.py: powerlaw_pdf :100-119) in mpmath, with analytic
derivatives, and rounded ONCE to float64.  Nothing of gwinferno_amd/ or oracle/ is imported.  The sample columns of
spline_terms_hp_logxlogy17.npz and spline_terms_hp_logxlogy20.npz are read as DATA: the new terms share them.

    python tests/golden/make_mass_forms_hp.py       # rewrites mass_forms_hp.npz (and checks the working precision and the cap)

Key layout of terms_hp.npz (``{name}/params, columns, col/*, tags, theta, logp, dlogp``; tests/terms_hp_util.Term reads it) and its
conventions: inputs are exact doubles; WHETHER a sample is in the support is decided on doubles, as the reference decides it; -inf
marks an excluded sample, its derivatives are 0; no finite value below -650 is stored.

plbounds  (params alpha, lo, hi; column x)
  log p = alpha log x + log((1 + alpha) / (hi^(1+alpha) - lo^(1+alpha))) for lo <= x <= hi, -inf outside (a sample ON a bound is
  inside).  AT alpha == -1.0 EXACTLY the reference returns -log x - log(hi / lo), not -log x - log log(hi / lo) (:131): recorded as
  written.  dlogp holds d/d alpha, d/d lo, d/d hi.  At alpha == -1.0 the alpha-derivative is the limit of the regular branch,
  log x - (log hi + log lo) / 2, and the two bound derivatives are those of the expression the reference returns, 1 / lo and -1 / hi.
  The bound derivatives are the same for every live sample of a hyper-point, so they cancel in any likelihood whose number of
  events is the N_obs of the selection term -- every catalog of tests/terms_hp_util.py -- where the engine returns 0 by convention.
  ``plbounds/group``: the catalogs for summed gradients need samples that are live at EVERY point they are run at; the points fall
  in two nests of intervals -- group 0, every interval that contains [20, 30]; group 1, [30, 33] and the two narrower ones inside
  it -- and catalog A of a group is made of the samples inside its narrowest interval.
pairing_iid, pairing_indep  (param beta; columns m1, m2 = x, x[perm], x the sample column of logxlogy17)
  log p = beta log(fl(m2 / m1)), the quotient rounded to float64 as the reference forms it.  pairing_iid carries the reference's
  exclusion q < 0 | q > 1 (:609-613); pairing_indep has none (q > 1 has a positive logarithm).  ``pairing/perm`` is the permutation.
  Hand pairs are made THROUGH it, since both columns are the spline term's own: m2 one ulp above m1 (2.0 and its neighbour),
  q near 30 (2.23.. and 65.76..), q near 1/30, and q = 1 / 394 ~ 2.5e-3 (394 and 1.0: both outside the spline's domain, so live in
  the pairing term alone).  No m2 == 0: 0^beta is a different case per sign of beta and is not claimed.
ratio_on_logxlogy20_mmin3, ratio_on_logxlogy20_mmin5  (param beta; columns m1, q; m1 the sample column of logxlogy20)
  powerlaw_pdf(q, beta, mmin / m1, 1) as make_terms_hp.py's ``ratio``: excluded where q < fl(mmin / m1), q > 1 or fl(mmin / m1) == 1.
  q is placed per sample inside [mmin / m1, 1] by the golden ratio, with hand cases on and next to both ends.  mmin = 3.0 is the
  spline's lower edge (the sample m1 == 3.0 is excluded); mmin = 5.0 lies inside the domain (samples below it are live for the spline,
  excluded here).  Two more arrays: ``dlogp_dlogm1`` = d log p / d log m1 (the condition number of log p with respect to the one
  input the engine rounds, log m1) and ``d2logp_dbeta_dlogm1``, the same for the beta-derivative.  A sample whose conditioning term
  |dlogp_dlogm1| EPS_LM_FOLD exceeds COND_CAP tells nothing about the arithmetic; ``_compute`` asserts that there are at most
  MAX_WAIVED of them per mmin (the nextafter neighbour above 3.0; none at 5.0).
"""
import os

import mpmath as mp
import numpy as np

DPS = 80
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mass_forms_hp.npz")
LOG_TINY = -745.14  # log(2^-1075)
LOG_FLOOR = -650.0
SWEEP_E = [0.0] + [s * e for e in (2.0**-52, 1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1) for s in (1.0, -1.0)]  # as make_terms_hp.py
SWEEP = [-1.0 + e for e in SWEEP_E]
SUBSET_E = [0.0, 1e-10, -1e-10, 1e-6, -1e-6]
# the rounding of log m1 as the engine's two forms see it (derived in tests/terms_hp_util.py, which is held to these numbers)
EPS_LM_OWN = 2.0**-50
EPS_LM_FOLD = 5.5 * 2.0**-50
COND_CAP = 1e-9
MAX_WAIVED = 2


def F(x):
    return mp.mpf(float(x))


def _geometric(first, ratio, n):
    out, v = [], first
    for _ in range(n):
        out.append(v)
        v = v * ratio
    return out


def _neighbours(v):
    return [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]


def _spline_column(name):
    with np.load(os.path.join(HERE, f"spline_terms_hp_{name}.npz")) as z:
        x = z[f"{name}/col/x"]
    assert x.dtype == np.float64
    return x


# ---------------------------------------------------------------------------------------------------------------------
# plbounds
# ---------------------------------------------------------------------------------------------------------------------
NARROW_LO = 30.0
NARROW = [("1e-1", NARROW_LO * (1.0 + 1e-1)), ("1e-3", NARROW_LO * (1.0 + 1e-3)), ("1e-6", NARROW_LO * (1.0 + 1e-6))]
WIDE = (1e-2, 1e3)
INNER = (0.125, 0.25, 0.5, 0.75, 0.875)


def plbounds_points():
    """(tag, (alpha, lo, hi), group)."""
    up5, dn100 = float(np.nextafter(5.0, np.inf)), float(np.nextafter(100.0, -np.inf))
    pts = [(f"ordinary{a:g}", (a, lo, hi), 0) for a, lo, hi in ((-2.5, 5.0, 100.0), (-3.5, 2.0, 50.0), (-1.5, 20.0, 30.0), (0.4, 5.0, 100.0), (1.7, 2.0, 50.0))]
    pts += [(f"sweep{e:+.3g}", (a, 5.0, 100.0), 0) for e, a in zip(SWEEP_E, SWEEP)]
    for lo, hi in ((2.0, 50.0), (20.0, 30.0)):
        pts += [(f"[{lo:g},{hi:g}]/sweep{e:+.3g}", (-1.0 + e, lo, hi), 0) for e in SUBSET_E]
    for w, hi in NARROW:
        pts += [(f"narrow{w}/alpha{t}", (a, NARROW_LO, hi), 1) for t, a in (("-2.5", -2.5), ("-1+1e-6", -1.0 + 1e-6), ("-1-1e-6", -1.0 - 1e-6), ("-1", -1.0))]
    pts += [(f"wide/alpha{a:g}", (a, WIDE[0], WIDE[1]), 0) for a in (12.0, -14.0, 40.0, -40.0)]
    # pairs that differ only in a bound: a sample changes sides between them (the first of each pair is ``ordinary-2.5``)
    pts += [("lo+1ulp", (-2.5, up5, 100.0), 0), ("hi-1ulp", (-2.5, 5.0, dn100), 0), ("lo8", (-2.5, 8.0, 100.0), 0), ("hi60", (-2.5, 5.0, 60.0), 0),
            ("hi30", (-2.5, 5.0, NARROW_LO), 0)]  # 30.0: hi here, lo of the narrow intervals
    return pts


def plbounds_samples(points):
    bounds = sorted({b for _, (_, lo, hi), _ in points for b in (lo, hi)})
    out = []
    for b in bounds:
        out += _neighbours(b)
    for _, hi in NARROW:
        out += [NARROW_LO + (hi - NARROW_LO) * f for f in INNER]
    out += _geometric(2.3, 1.21, 20)  # 2.3 .. 86: five of them inside [20, 30]
    out += [21.0, 23.5, 26.0, 28.5, 0.5, 400.0, 5e-3, 2e3]
    seen, xs = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            xs.append(v)
    return np.array(xs, dtype=np.float64)


def plbounds_lognorm(alpha, lo, hi):
    """(log A, d/d alpha, d/d lo, d/d hi) of A = (1+alpha) / (hi^(1+alpha) - lo^(1+alpha)); alpha == -1: the reference's 1 / (hi / lo)."""
    a1 = 1 + alpha
    llo, lhi = mp.log(lo), mp.log(hi)
    if a1 == 0:
        return -(lhi - llo), -(lhi + llo) / 2, 1 / lo, -1 / hi
    ph, pw = mp.exp(a1 * lhi), mp.exp(a1 * llo)
    return mp.log(a1 / (ph - pw)), 1 / a1 - (ph * lhi - pw * llo) / (ph - pw), a1 * pw / lo / (ph - pw), -a1 * ph / hi / (ph - pw)


def _plbounds_term():
    points = plbounds_points()
    xs = plbounds_samples(points)
    H, n = len(points), len(xs)
    logp = np.full((H, n), -np.inf)
    dlogp = np.zeros((H, 3, n))
    lx = [mp.log(F(x)) if x > 0 else None for x in xs]
    for h, (tag, (alpha, lo, hi), _) in enumerate(points):
        assert alpha != 0.0 and lo < hi
        if tag.startswith("wide"):  # the reference's own float64 expression stays finite
            with np.errstate(all="raise"):
                ref = np.log((1.0 + alpha) / (np.float64(hi) ** (1.0 + alpha) - np.float64(lo) ** (1.0 + alpha)))
            assert np.isfinite(ref), (tag, ref)
        la, da, dlo, dhi = plbounds_lognorm(F(alpha), F(lo), F(hi))
        for i, x in enumerate(xs):
            if x < lo or x > hi:
                continue
            lp = F(alpha) * lx[i] + la
            assert lp > LOG_FLOOR, (tag, i, float(lp))
            logp[h, i] = float(lp)
            dlogp[h, :, i] = [float(lx[i] + da), float(dlo), float(dhi)]
    group = np.array([g for _, _, g in points], dtype=np.int64)
    live = np.isfinite(logp)
    for g in (0, 1):
        core = live[group == g].all(axis=0)
        assert core.sum() >= 9, (g, int(core.sum()))  # catalog A: the samples inside the group's narrowest interval
        assert (live[group == g].any(axis=0) & ~core).sum() >= 4, g
        for h in np.flatnonzero(group == g):  # no tag at which every live sample of the group's core has the same log-density
            assert len(set(logp[h, core])) > 1, points[h][0]
    name = "plbounds"
    return {f"{name}/params": np.array(["alpha", "lo", "hi"]), f"{name}/columns": np.array(["x"]), f"{name}/col/x": xs, f"{name}/tags": np.array([t for t, _, _ in points]),
            f"{name}/theta": np.array([p for _, p, _ in points], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp, f"{name}/group": group}


# ---------------------------------------------------------------------------------------------------------------------
# pairing
# ---------------------------------------------------------------------------------------------------------------------
BETAS = [("beta1", 1.0), ("beta-1", -1.0), ("beta2.5", 2.5), ("beta-3.5", -3.5), ("beta12", 12.0), ("beta-8", -8.0), ("beta1e-12", 1e-12), ("beta0", 0.0)]


def pairing_perm(x):
    """Forced pairs (m1 -> m2, as indices into x), three fixed points, and every other sample seven places on among the rest."""
    at = lambda v: int(np.flatnonzero(x == v)[0])  # noqa: E731
    near = lambda v: int(np.argmin(np.abs(x - v)))  # noqa: E731
    two, two_up = at(2.0), at(float(np.nextafter(2.0, np.inf)))
    forced = {two: two_up,              # m2 one ulp above m1
              near(2.2309): near(65.76),  # q ~ 29.5
              near(75.97): near(2.6447),  # q ~ 1 / 28.7
              at(394.0): at(1.0),       # q ~ 2.5e-3: both outside the spline's domain
              near(14.1421): near(14.1421), near(41.2486): near(41.2486), at(100.0): at(100.0)}  # q == 1 exactly
    n = len(x)
    perm = np.full(n, -1, dtype=np.int64)
    for a, b in forced.items():
        perm[a] = b
    src = [i for i in range(n) if perm[i] < 0]
    dst = [i for i in range(n) if i not in set(forced.values())]
    assert len(src) == len(dst)
    for k, i in enumerate(src):
        perm[i] = dst[(k + 7) % len(dst)]
    assert sorted(perm.tolist()) == list(range(n))
    return perm


def _pairing_terms():
    x = _spline_column("logxlogy17")
    perm = pairing_perm(x)
    m1, m2 = x, np.ascontiguousarray(x[perm])
    assert np.all(m2 != 0.0) and np.all(m1 > 0.0)
    q = m2 / m1  # float64, as the reference forms it
    n = len(x)
    assert np.sum(q < 1.0) >= n / 3 and np.sum(q > 1.0) >= n / 5 and np.sum(q == 1.0) >= 3
    assert np.any(np.abs(q - 30.0) < 1.0) and np.any(np.abs(1.0 / q - 30.0) < 2.0) and np.any(np.abs(q - 2.5e-3) < 1e-4) and q[int(np.flatnonzero(x == 2.0)[0])] == 1.0 + 2.0**-52
    lq = [mp.log(F(v)) for v in q]
    out = {"pairing/perm": perm}
    for name, masked in (("pairing_iid", True), ("pairing_indep", False)):
        logp = np.full((len(BETAS), n), -np.inf)
        dlogp = np.zeros((len(BETAS), 1, n))
        for h, (_, beta) in enumerate(BETAS):
            for i in range(n):
                if masked and (q[i] < 0.0 or q[i] > 1.0):
                    continue
                lp = F(beta) * lq[i]
                assert lp > LOG_FLOOR
                logp[h, i] = float(lp)
                dlogp[h, 0, i] = float(lq[i])
        out.update({f"{name}/params": np.array(["beta"]), f"{name}/columns": np.array(["m1", "m2"]), f"{name}/col/m1": m1, f"{name}/col/m2": m2,
                    f"{name}/tags": np.array([t for t, _ in BETAS]), f"{name}/theta": np.array([[b] for _, b in BETAS], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the mass-ratio power law on the m1 column of logxlogy20
# ---------------------------------------------------------------------------------------------------------------------
RATIO_MMINS = [("mmin3", 3.0), ("mmin5", 5.0)]
SPLINE_RANGE = (3.0, 100.0)


def ratio_points():
    return [("ordinary", (b,)) for b in (1.0, 2.0, 0.0, -2.0, 3.1, -3.5, 8.0)] + [(f"sweep{e:+.3g}", (b,)) for e, b in zip(SWEEP_E, SWEEP)]  # as make_terms_hp.py


def ratio_q(m1, mmin):
    """q per sample: inside [mmin / m1, 1] by the golden ratio (as make_terms_hp.ratio_samples); hand cases on and next to both ends,
    put on the samples of the spline's domain that lie above 6 (so that both values of mmin meet them) in the order of the column."""
    q = np.empty(len(m1))
    for k, m in enumerate(m1):
        low = mmin / m
        f = ((k + 1) * 0.6180339887498949) % 1.0
        q[k] = low + (1.0 - low) * (0.02 + 0.96 * f) if low < 1.0 else 0.9
    hosts = [k for k, m in enumerate(m1) if 6.0 < m <= SPLINE_RANGE[1]]
    hand = [lambda low: 1.0, lambda low: low, lambda low: float(np.nextafter(low, 1.0)), lambda low: float(np.nextafter(low, 0.0)), lambda low: float(np.nextafter(1.0, 2.0)),
            lambda low: float(np.nextafter(1.0, 0.0)), lambda low: low, lambda low: float(np.nextafter(low, 1.0))]
    for k, fn in zip(hosts[2::3], hand):
        q[k] = fn(mmin / m1[k])
    return q


def _ratio_terms():
    m1 = _spline_column("logxlogy20")
    points = ratio_points()
    H, n = len(points), len(m1)
    out = {}
    for label, mmin in RATIO_MMINS:
        name = f"ratio_on_logxlogy20_{label}"
        q = ratio_q(m1, mmin)
        logp = np.full((H, n), -np.inf)
        dlogp = np.zeros((H, 1, n))
        dlm = np.zeros((H, n))
        d2 = np.zeros((H, n))
        for h, (_, (beta,)) in enumerate(points):
            b1 = 1 + F(beta)
            for i in range(n):
                low = mmin / m1[i]  # float64, as the reference forms it
                if q[i] < low or q[i] > 1.0 or low == 1.0:
                    continue
                lr = mp.log(F(mmin) / F(m1[i]))  # log r < 0
                lq = mp.log(F(q[i]))
                t = b1 * lr
                if b1 == 0:
                    lp, db, g, dg = -lq - mp.log(-lr), lq - lr / 2, mp.mpf(1), mp.mpf(1) / 2
                else:
                    em1 = mp.expm1(t)  # r^b1 - 1
                    lp = F(beta) * lq + mp.log(b1 / -em1)
                    db = lq + 1 / b1 + (em1 + 1) * lr / -em1
                    g = t * (em1 + 1) / em1                       # d log p / d log m1 = g(t) / log r
                    dg = (em1 + 1) * (em1 - t) / em1**2           # g'(t): d^2 log p / d beta d log m1
                assert lp > LOG_FLOOR, (name, h, i, float(lp))
                logp[h, i] = float(lp)
                dlogp[h, 0, i] = float(db)
                dlm[h, i] = float(g / lr)
                d2[h, i] = float(dg)
        live = np.isfinite(logp)
        waived = np.flatnonzero((np.abs(dlm) * EPS_LM_FOLD > COND_CAP).any(axis=0))
        assert len(waived) <= MAX_WAIVED and np.all(m1[waived] == np.nextafter(SPLINE_RANGE[0], np.inf)) and (mmin == 3.0 or len(waived) == 0), (name, m1[waived])
        inside = (m1 >= SPLINE_RANGE[0]) & (m1 <= SPLINE_RANGE[1])
        assert np.array_equal(live.all(axis=0), live.any(axis=0))  # the support does not depend on beta
        assert np.sum(live[0] & inside) >= 16 and np.sum(~live[0] & inside) >= 3 and not live[0][m1 == mmin].any()
        if mmin == 5.0:
            assert np.sum(inside & (m1 < mmin)) >= 5
        out.update({f"{name}/params": np.array(["beta"]), f"{name}/columns": np.array(["m1", "q"]), f"{name}/col/m1": m1, f"{name}/col/q": q,
                    f"{name}/tags": np.array([t for t, _ in points]), f"{name}/theta": np.array([p for _, p in points], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp,
                    f"{name}/dlogp_dlogm1": dlm, f"{name}/d2logp_dbeta_dlogm1": d2, f"{name}/mmin": np.float64(mmin)})
    return out


TERM_NAMES = ["plbounds", "pairing_iid", "pairing_indep"] + [f"ratio_on_logxlogy20_{label}" for label, _ in RATIO_MMINS]


def _compute(dps):
    out = {}
    with mp.workdps(dps):
        out.update(_plbounds_term())
        out.update(_pairing_terms())
        out.update(_ratio_terms())
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
    size = os.path.getsize(OUT)
    assert size < 256 * 1024, size
    print(f"wrote {OUT}: {size} bytes, {len(arrays)} arrays")
