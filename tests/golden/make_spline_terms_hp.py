"""Generator of tests/golden/spline_terms_hp_*.npz: log-densities of the 1-D B-spline models and of the tabulated power-law
redshift distribution, and their derivatives with respect to EVERY coefficient, at 80 digits.

Every density is written here from its definition in the reference (gwinferno/interpolation.py: knot vector :98-106, Cox-de Boor
recursion :128-149, B-spline scaling :278, design matrix and domain :163-175, the four bases and their grids :280-317, :320-449;
gwinferno/models/bsplines/single.py:35-58; gwinferno/numpyro_distributions.py:163-195) in mpmath, with analytic derivatives, and
rounded ONCE to float64.  Nothing of gwinferno_amd/ or oracle/ is imported, and the closed-form taps of a uniform knot vector that
the engine and its C oracle share are NOT used: the bases come out of the recursion on the knot vector's own doubles.

    python tests/golden/make_spline_terms_hp.py      # rewrites the files (and checks the working precision)
    python tests/golden/make_spline_terms_hp.py --tabulate   # first tabulates dVc/dz at the redshift samples from the reference

One file per term (tests/test_terms_hp_cpu.py holds each below 256 KiB), in the layout of terms_hp.npz:
``{name}/params, columns, col/*, tags, theta, logp, dlogp`` -- tests/terms_hp_util.Term loads them unchanged.

Conventions
  * Inputs are float64 numbers and enter the arithmetic exactly.  The knot vector is the reference's: ``interior =
    linspace(lo, hi, N - 2)``, ``dx = interior[1] - interior[0]``, ``knots = linspace(lo - 3 dx, hi + 3 dx, N + 4)`` in float64; the
    normalisation grid is ``linspace(xmin, xmax, 1000)`` (1500 for LogXLogY) in float64, linear in x.
  * Recursion: order-1 pieces are half-open, 1 on ``knots[i] <= u < knots[i+1]``; B_{i,k}(u) = (u - t_i) / (t_{i+k-1} - t_i) B_{i,k-1}
    + (t_{i+k} - u) / (t_{i+k} - t_{i+1}) B_{i+1,k-1} -- the reference's M-spline recursion times its scaling (t_{i+4} - t_i) / 4.
    Only the pieces that can be non-zero at u are visited; that skips zeros, nothing else.
  * A log-x basis lives on u = log(x) ROUNDED TO FLOAT64 (the reference takes the logarithm in float64 before it evaluates the
    recursion); that double enters exactly.  Its domain is log(xrange) rounded to float64.
  * WHETHER a sample (or a grid node) is in the domain is decided the way the reference decides it, by comparing doubles:
    ``xmin <= x <= xmax`` and not (``u < lo`` or ``u > hi``).  A grid node outside contributes 0 to the trapezoid sum (the bases are 0
    there, or -inf under the exponential).  The VALUE inside is exact.
  * Exponentiated bases (LogY, LogXLogY): p = exp(sum_k c_k B_k(u)) / Z, Z = trapz(exp(sum_k c_k B_k(grid)), grid);
    d log p / d c_j = B_j(u) - sum_i w_i B_j(g_i) e_i / Z.
    Linear bases (BSpline, LogXBSpline; normalize=True): p = f / Z, f = sum_k c_k B_k(u), Z = sum_k c_k I_k, I_k = trapz(B_k(grid),
    grid); d log p / d c_j = B_j(u) / f - I_j / Z.  A sample with f <= 0 is excluded (the engine's rule: it defines f, Z > 0 only);
    ``_compute`` asserts Z > 0 and that no in-domain sample has 0 < |f| < 1e-3 sum_k |c_k B_k|, so the sign is never a rounding matter.
    The trapezoid rule is exact arithmetic on the grid's doubles.
  * PowerlawRedshift on the z grid and dVc/dz table that tests/golden/terms.npz holds from the unmodified reference:
    log p = log interp(z) + (lamb - 1) log(1 + z) - log trapz(dVc/dz (1 + z)^(lamb - 1), zgrid) for z <= maximum, interp linear with the
    end values held outside the grid (jnp.interp); exact arithmetic on the committed doubles.
  * The spline redshift models (PowerlawSplineRedshiftModel, models/spline_perturbation.py:304-372; BSplineRedshift, models/bsplines/
    single.py:398-492): see ``_plz_term`` and ``_zspline_term``.  Cosmology is INPUT DATA: dVc/dz on the 1000-point z grid is the table
    tests/golden/terms.npz holds from the unmodified reference, and the data ends of every term are that grid's ends (1e-9 and 1.9), so
    that the models' own ``linspace(zmin, zmax, 1000)`` IS that grid; dVc/dz at the samples is tests/golden/z_samples_dVcdz.npz, tabulated
    from the unmodified reference's cosmology (through ref_import.py) by ``python tests/golden/make_spline_terms_hp.py --tabulate``,
    which needs the reference tree; without the flag the committed table is read.  d log p / d c_j carries -d log Z / d c_j, but
    NO CATALOG EXERCISES THAT PART: log Z is the same for every sample, so it cancels between the events and the injections of a
    hierarchical likelihood, neither the engine nor its oracle forms it, and the cross term d^2 / d lamb d c of the normaliser is not
    refereed.  What is held of the normaliser is its VALUE, in every log-weight of the values catalog.
  * BSplineDistribution (numpyro_distributions.py:266-293): see ``_lerp_term``, which also states what is recorded at a grid node that
    carries -inf.
  * Excluded samples: logp = -inf, derivatives 0.  No finite value below -650 is stored (asserted, as in make_terms_hp.py).
  * Adding one constant to every coefficient of an exponentiated basis does not move the density inside the domain (the bases sum
    to one there): the points tagged ``shift+300`` / ``shift-300`` are ``normal1`` shifted, and ``_compute`` asserts that their
    log-densities agree with ``normal1``'s to 60 digits -- to 600 (gap / dx)^3 ~ 1e-42 for the knot vectors whose float64 linspace
    leaves knots[3] an ulp above lo or knots[N] an ulp below hi (``gap``), where the reference's basis set is short of one by that.
  * "Random" numbers come from numpy's frozen legacy generator and are rounded to a multiple of 2^-20, so that the last bits of a
    platform's libm do not enter the fixture.
  * A LOG-DENSITY below 1e-40 in magnitude is stored as 0 (the flat spline's on a domain of length 1 is exactly that, and the working
    precision leaves 1e-80 in its place).  Derivatives are rounded once, as they come.
  * Working precision: DPS digits; ``generate(verify=True)`` repeats everything at 2 x DPS and asserts that no double changes.
"""
import os

import mpmath as mp
import numpy as np

DPS = 80
HERE = os.path.dirname(os.path.abspath(__file__))
PREFIX = "spline_terms_hp_"
LOG_TINY = -745.14  # log(2^-1075)
LOG_FLOOR = -650.0
CONDITION = 1e-3  # a live linear-spline sample keeps f >= CONDITION sum_k |c_k B_k|
F32 = np.float32


def F(x):
    return mp.mpf(float(x))


def _rounded(v):
    """The double nearest to v; exactly 0 where |v| < 1e-40.  (A flat spline on a domain of length 1 has log p = 0: the working
    precision leaves 1e-80 of rounding in its place, and a missing edge basis -- see ``gap`` below -- 1e-45.)"""
    return 0.0 if abs(v) < mp.mpf(10) ** -40 else float(v)


def _quantised(values):
    return np.round(np.asarray(values, dtype=np.float64) * 2.0**20) / 2.0**20


# ---------------------------------------------------------------------------------------------------------------------
# the basis
# ---------------------------------------------------------------------------------------------------------------------
class Basis:
    def __init__(self, kind, N, xrange):
        self.kind, self.N = kind, N
        self.log_x = kind in ("LogXBSpline", "LogXLogYBSpline")
        self.log_y = kind in ("LogYBSpline", "LogXLogYBSpline")
        self.xmin, self.xmax = float(xrange[0]), float(xrange[1])
        dom = np.log(np.asarray(xrange, dtype=np.float64)) if self.log_x else np.asarray(xrange, dtype=np.float64)
        self.lo, self.hi = float(dom[0]), float(dom[1])
        interior = np.linspace(self.lo, self.hi, N - 4 + 2)
        dx = interior[1] - interior[0]
        self.knots = np.linspace(self.lo - dx * 3, self.hi + dx * 3, len(interior) + 6)
        assert len(self.knots) == N + 4 and np.all(np.diff(self.knots) > 0)
        assert np.all(self.knots[4:] - self.knots[:-4] >= 1e-6)  # (the reference zeroes a basis narrower than that, :141)
        ends = np.exp(dom) if self.log_x else dom
        self.grid = np.linspace(ends[0], ends[1], 1500 if kind == "LogXLogYBSpline" else 1000)

    def coordinate(self, x):
        with np.errstate(all="ignore"):
            return np.log(np.asarray(x, dtype=np.float64)) if self.log_x else np.asarray(x, dtype=np.float64)

    def inside(self, x, u):
        return bool(x >= self.xmin and x <= self.xmax and not (u < self.lo or u > self.hi))

    def grid_inside(self, u):  # the design matrix's own test (:175, :407, :449); the model's xrange mask does not see the grid
        return not (u < self.lo or u > self.hi)

    def bases(self, u):
        """{i: B_i(u)} of the order-4 bases that can be non-zero at the double u, by the Cox-de Boor recursion."""
        t = self.knots
        j = int(np.searchsorted(t, u, side="right")) - 1  # t[j] <= u < t[j+1], compared as doubles
        if j < 0 or j >= len(t) - 1:
            return {}
        um, tm = F(u), self._knots_mp()
        B = {j: mp.mpf(1)}
        for k in (2, 3, 4):
            nxt = {}
            for i in range(max(j - k + 1, 0), j + 1):
                if i + k > len(t) - 1:
                    continue
                v = mp.mpf(0)
                if i in B:
                    v += (um - tm[i]) / (tm[i + k - 1] - tm[i]) * B[i]
                if i + 1 in B:
                    v += (tm[i + k] - um) / (tm[i + k] - tm[i + 1]) * B[i + 1]
                nxt[i] = v
            B = nxt
        return {i: v for i, v in B.items() if i < self.N}

    def _knots_mp(self):
        # (per working precision: an mpf made at 80 digits from a double is exact at 160 too, but keep the caches apart)
        key = mp.mp.dps
        cache = self.__dict__.setdefault("_tm", {})
        if key not in cache:
            cache[key] = [F(v) for v in self.knots]
        return cache[key]


def _trapezoid(nodes, values):
    return sum(((nodes[i + 1] - nodes[i]) * (values[i] + values[i + 1]) / 2 for i in range(len(nodes) - 1)), mp.mpf(0))


def _trapezoid_weights(nodes):
    w = [mp.mpf(0)] * len(nodes)
    for i in range(len(nodes) - 1):
        h = (nodes[i + 1] - nodes[i]) / 2
        w[i] += h
        w[i + 1] += h
    return w


# ---------------------------------------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------------------------------------
def _neighbours(v, dtype=np.float64):
    v = dtype(v)
    return [float(np.nextafter(v, dtype(-np.inf))), float(v), float(np.nextafter(v, dtype(np.inf)))]


def _log_landing(target):
    """Doubles x whose float64 log is nextafter(target, -inf), target, nextafter(target, +inf) (each where one exists)."""
    out = []
    for want in _neighbours(target):
        x = float(np.exp(want))
        for _ in range(64):  # walk to a double whose log is exactly `want`
            got = float(np.log(x))
            if got == want:
                out.append(x)
                break
            x = float(np.nextafter(x, np.inf if got < want else -np.inf))
    return out


def samples(b, seed, float32=False):
    """lo, hi and their neighbours; knots with both neighbours (every interior knot for N <= 7, a spread otherwise); interval
    mid-points; seeded random points; points outside.  ``float32``: every sample is a float32 number (the neighbours are float32
    neighbours).  Log-x bases: also x whose float64 log lands on a knot coordinate and next to it."""
    dt = F32 if float32 else np.float64
    n_int = b.N - 3
    inner = list(range(1, n_int)) if b.N <= 7 else sorted({1, n_int // 2, n_int - 1})
    mids = list(range(n_int)) if n_int <= 6 else sorted({0, 1, n_int // 3, n_int // 2, n_int - 2, n_int - 1})
    out = _neighbours(b.xmin, dt) + _neighbours(b.xmax, dt)
    kn = b.knots[3:3 + n_int + 1]
    if b.log_x:
        for m in inner:
            out += _log_landing(kn[m])
        out += [float(np.exp(0.5 * (kn[m] + kn[m + 1]))) for m in mids]
    else:
        for m in inner:
            out += _neighbours(kn[m], dt)
        out += [float(dt(0.5 * (kn[m] + kn[m + 1]))) for m in mids]
    rs = np.random.RandomState(seed)
    r = _quantised(rs.uniform(0.0, 1.0, 16))
    if b.log_x:
        out += [float(v) for v in _quantised(np.exp(b.lo + (b.hi - b.lo) * r) * 64.0) / 64.0]
    else:
        out += [float(dt(v)) for v in b.xmin + (b.xmax - b.xmin) * r]
    span = b.xmax - b.xmin
    out += [float(dt(b.xmin - 0.25 * span)) if not b.log_x else 0.5 * b.xmin, float(dt(b.xmax + 0.25 * span)), float(dt(b.xmax + 3.0 * span))]
    x = np.array(out, dtype=np.float64)
    if float32:
        assert np.array_equal(x.astype(F32).astype(np.float64), x)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# hyper-points
# ---------------------------------------------------------------------------------------------------------------------
def exp_points(N, seed):
    rs = np.random.RandomState(seed)
    z = _quantised(rs.standard_normal((4, N)))
    e = np.eye(N)
    saw = np.array([10.0 if k % 2 == 0 else -10.0 for k in range(N)])
    hole = z[3].copy()
    hole[N // 2] = -300.0
    return [("zeros", np.zeros(N)), ("5e0", 5.0 * e[0]), (f"5e{N // 2}", 5.0 * e[N // 2]), (f"5e{N - 1}", 5.0 * e[N - 1]), ("normal1", z[0]), ("normal10", 10.0 * z[1]),
            ("normal40", 40.0 * z[2]), ("sawtooth10", saw), ("shift+300", z[0] + 300.0), ("shift-300", z[0] - 300.0), ("hole-300", hole)]


def linear_points(N, seed):
    rs = np.random.RandomState(seed)
    u = _quantised(rs.uniform(0.5, 1.5, (4, N)))
    wide = np.array([2.0 ** int(v) for v in np.round(4.0 * _quantised(rs.standard_normal(N)))])  # positive, 2^-12 .. 2^12
    mixed = np.array([1.5 if k % 2 == 0 else -0.3 for k in range(N)])  # positive everywhere: at a knot (c_k + 4 c_k+1 + c_k+2) / 6 >= 0.3
    dip = np.ones(N)
    dip[N // 2] = -2.0  # negative around its own basis: those samples are excluded
    pts = [("ones", np.ones(N)), ("pos0.01", 0.01 * u[0]), ("pos0.1", 0.1 * u[1]), ("pos1", u[2]), ("pos10", 10.0 * u[3]), ("wide", wide), ("mixed", mixed)]
    return pts + [("dip", dip)] if N >= 7 else pts  # (N = 4: one interval, a dip that deep turns the integral negative)


# ---------------------------------------------------------------------------------------------------------------------
# terms
# ---------------------------------------------------------------------------------------------------------------------
SPLINES = [  # name, basis, N, xrange, float32 samples
    ("logy4", "LogYBSpline", 4, (0.0, 1.0), False),
    ("logy7", "LogYBSpline", 7, (-1.0, 1.0), False),
    ("logy16", "LogYBSpline", 16, (0.0, 1.0), False),
    ("logy17", "LogYBSpline", 17, (0.0, 1.0), False),
    ("logy20", "LogYBSpline", 20, (0.0, 1.0), False),
    ("logy7_f32", "LogYBSpline", 7, (0.0, 1.0), True),
    ("logxlogy4", "LogXLogYBSpline", 4, (0.1, 1.0), False),
    ("logxlogy17", "LogXLogYBSpline", 17, (2.0, 100.0), False),
    ("logxlogy20", "LogXLogYBSpline", 20, (3.0, 100.0), False),
    ("bspline4", "BSpline", 4, (0.0, 1.0), False),
    ("bspline7", "BSpline", 7, (-1.0, 1.0), False),
    ("bspline17", "BSpline", 17, (0.0, 1.0), False),
    ("bspline7_f32", "BSpline", 7, (0.0, 1.0), True),
    ("logx4", "LogXBSpline", 4, (0.01, 1.0), False),
    ("logx7", "LogXBSpline", 7, (0.001, 2.3), False),
    ("logx17", "LogXBSpline", 17, (0.01, 1.0), False),
]
META = {name: dict(basis=kind, n=N, xrange=xr, float32=f32) for name, kind, N, xr, f32 in SPLINES}
Z_LAMBS = [("lamb-4", -4.0), ("lamb-1", -1.0), ("lamb0", 0.0), ("lamb1", 1.0), ("lamb1+2^-52", 1.0 + 2.0**-52), ("lamb1-2^-52", 1.0 - 2.0**-52), ("lamb2.7", 2.7), ("lamb8", 8.0)]


def _spline_term(name, kind, N, xrange, float32):
    b = Basis(kind, N, xrange)
    seed = 1000 + sum(ord(ch) for ch in name)
    xs = samples(b, seed, float32)
    points = exp_points(N, seed + 1) if b.log_y else linear_points(N, seed + 1)
    us = b.coordinate(xs)
    live = [b.inside(float(x), float(u)) for x, u in zip(xs, us)]
    Bx = [b.bases(float(u)) if ok else None for u, ok in zip(us, live)]
    # the grid, ONCE per term: nodes, bases at the nodes inside the domain
    g = [F(v) for v in b.grid]
    gu = b.coordinate(b.grid)
    Bg = [b.bases(float(u)) if b.grid_inside(float(u)) else None for u in gu]
    tw = _trapezoid_weights(g)
    H, n = len(points), len(xs)
    logp = np.full((H, n), -np.inf)
    dlogp = np.zeros((H, N, n))
    exact = {}
    for h, (tag, c_d) in enumerate(points):
        c = [F(v) for v in c_d]
        if b.log_y:
            e = [mp.exp(sum(c[i] * v for i, v in Bi.items())) if Bi is not None else mp.mpf(0) for Bi in Bg]
            Z = _trapezoid(g, e)
            dlogZ = [mp.mpf(0)] * N
            for w, ei, Bi in zip(tw, e, Bg):
                if Bi is not None:
                    for i, v in Bi.items():
                        dlogZ[i] += w * ei * v
            dlogZ = [d / Z for d in dlogZ]
            logZ = mp.log(Z)
        else:
            I = [mp.mpf(0)] * N  # trapz(B_k(grid), grid): the same for every hyper-point, cheap next to the bases themselves
            for w, Bi in zip(tw, Bg):
                if Bi is not None:
                    for i, v in Bi.items():
                        I[i] += w * v
            Z = sum(ci * Ii for ci, Ii in zip(c, I))
            assert Z > 0, (name, tag)
        row = []
        for s in range(n):
            if Bx[s] is None:
                row.append(None)
                continue
            f = sum(c[i] * v for i, v in Bx[s].items())
            if b.log_y:
                lp, d = f - logZ, [Bx[s].get(j, mp.mpf(0)) - dlogZ[j] for j in range(N)]
            else:
                size = sum(abs(c[i] * v) for i, v in Bx[s].items())
                assert f == 0 or abs(f) >= CONDITION * size, (name, tag, s, float(f), float(size))
                if f <= 0:
                    row.append(None)
                    continue
                lp, d = mp.log(f) - mp.log(Z), [Bx[s].get(j, mp.mpf(0)) / f - I[j] / Z for j in range(N)]
            row.append(lp)
            if lp < LOG_TINY:
                continue
            assert lp > LOG_FLOOR, (name, tag, s, float(lp))
            logp[h, s] = _rounded(lp)
            dlogp[h, :, s] = [float(v) for v in d]
        exact[tag] = row
    if b.log_y:
        # partition of unity holds on [knots[3], knots[N]]; where linspace left lo one ulp below knots[3] (or hi above knots[N]) the
        # basis B_-1 (B_N) that the reference does not carry is worth at most (gap / dx)^3 there, ~1e-45: times the shift, twice (the
        # sample and the grid's end node).  Zero for the knot vectors whose ends are exact.
        gap = max(0.0, b.knots[3] - b.lo, b.hi - b.knots[N]) / (b.knots[4] - b.knots[3])
        tol = mp.mpf(10) ** -60 + 2 * 300 * F(gap) ** 3
        for tag in ("shift+300", "shift-300"):
            for a, r in zip(exact[tag], exact["normal1"]):
                assert (a is None) == (r is None) and (a is None or abs(a - r) < tol), (name, tag)
    return {f"{name}/params": np.array([f"c{k}" for k in range(N)]), f"{name}/columns": np.array(["x"]), f"{name}/col/x": xs,
            f"{name}/tags": np.array([t for t, _ in points]), f"{name}/theta": np.array([c for _, c in points], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp}


def redshift_samples(zg, maximum):
    nodes = [0, 1, 2, 137, 500, int(np.searchsorted(zg, maximum)) - 1, int(np.searchsorted(zg, maximum))]
    out = [0.0]
    for i in nodes:
        out += _neighbours(zg[i]) if i else [float(zg[0]), float(np.nextafter(zg[0], 1.0))]
    out += [0.5 * (zg[i] + zg[i + 1]) for i in (0, 1, 40, 137, 333, 500, 640, 700)]
    out += [0.1, 0.25, 0.7, 1.1, 1.3]
    out += [float(maximum), float(np.nextafter(maximum, 0.0)), float(np.nextafter(maximum, 9.0)), 1.5, float(zg[-1]), 2.0]
    return np.array(out, dtype=np.float64)


def _redshift_term():
    t = np.load(os.path.join(HERE, "terms.npz"))
    zg, dv, maximum = t["dist/z_grid"], t["dist/z_dVcdz"], float(t["dist/powerlaw_redshift/maximum"])
    assert zg.dtype == np.float64 and dv.dtype == np.float64 and np.all(np.diff(zg) > 0)
    zs = redshift_samples(zg, maximum)
    g, d = [F(v) for v in zg], [F(v) for v in dv]
    l1g = [mp.log(1 + v) for v in g]
    name, n = "powerlaw_redshift", len(zs)
    logp = np.full((len(Z_LAMBS), n), -np.inf)
    dlogp = np.zeros((len(Z_LAMBS), 1, n))
    for h, (_, lamb) in enumerate(Z_LAMBS):
        lm = F(lamb)
        y = [di * mp.exp((lm - 1) * li) for di, li in zip(d, l1g)]
        Z = _trapezoid(g, y)
        dlogZ = _trapezoid(g, [yi * li for yi, li in zip(y, l1g)]) / Z
        for s, z in enumerate(zs):
            if not z <= maximum:
                continue
            zm = F(z)
            i = int(np.searchsorted(zg, z, side="right")) - 1
            if i < 0:
                v = d[0]
            elif i >= len(zg) - 1:
                v = d[-1]
            else:
                v = d[i] + (zm - g[i]) * (d[i + 1] - d[i]) / (g[i + 1] - g[i])
            l1 = mp.log(1 + zm)
            lp = mp.log(v) + (lm - 1) * l1 - mp.log(Z)
            assert lp > LOG_FLOOR, (name, lamb, s)
            logp[h, s] = float(lp)
            dlogp[h, 0, s] = float(l1 - dlogZ)
    return {f"{name}/params": np.array(["lamb"]), f"{name}/columns": np.array(["z"]), f"{name}/col/z": zs, f"{name}/tags": np.array([t for t, _ in Z_LAMBS]),
            f"{name}/theta": np.array([[v] for _, v in Z_LAMBS], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp}


# ---------------------------------------------------------------------------------------------------------------------
# the spline redshift models
# ---------------------------------------------------------------------------------------------------------------------
Z_SPLINES = [  # name, model, N, xrange (None: the data range), normalize
    ("plzspline4", "PowerlawSplineRedshiftModel", 4, None, False),
    ("plzspline7", "PowerlawSplineRedshiftModel", 7, None, False),
    ("plzspline17", "PowerlawSplineRedshiftModel", 17, None, False),
    ("zspline4", "BSplineRedshift", 4, (1e-4, 1.5), True),
    ("zspline16", "BSplineRedshift", 16, (1e-4, 1.5), True),
    ("zspline17", "BSplineRedshift", 17, (1e-4, 1.5), True),
    ("zspline7_raw", "BSplineRedshift", 7, (1e-4, 1.5), False),
]
Z_META = {name: dict(model=model, n=N, xrange=xr, normalize=nz) for name, model, N, xr, nz in Z_SPLINES}
COSMOLOGY = "z_samples_dVcdz.npz"  # dVc/dz of the unmodified reference at every redshift sample of the terms above


def _z_grid():
    with np.load(os.path.join(HERE, "terms.npz")) as t:
        zg, dv = t["dist/z_grid"], t["dist/z_dVcdz"]
    assert zg.dtype == np.float64 and dv.dtype == np.float64 and np.array_equal(np.linspace(zg[0], zg[-1], 1000), zg)
    return zg, dv


def z_samples(b, zmin, zmax, seed):
    """Redshift samples of one term: the data ends zmin and zmax EXACTLY (the models take their grid from them), their inner
    neighbours and nextafter(zmax, +inf); the two neighbours of each end of the spline domain where it lies inside the data range,
    and points outside it on both sides; doubles whose float64 log lands on lo, on hi, on interior knots and one ulp either side
    (and the neighbouring doubles of the z that lands on it); interval mid-points; seeded log-uniform points (float32 numbers); 2.0, beyond the grid."""
    n_int = b.N - 3
    inner = list(range(1, n_int)) if b.N <= 7 else sorted({1, 2, n_int // 2, n_int - 2, n_int - 1})
    mids = list(range(n_int)) if n_int <= 6 else sorted({0, 1, n_int // 3, n_int // 2, n_int - 2, n_int - 1})
    top = float(np.nextafter(zmax, np.inf))
    # (zmin and zmax second and third: in a product with a fixture term on [0, 1] or [-1, 1], whose first sample lies below its domain,
    # both stay live)
    out = [float(np.nextafter(zmin, np.inf)), zmin, zmax, float(np.nextafter(zmax, -np.inf)), top]
    if (b.xmin, b.xmax) != (zmin, zmax):
        out += _neighbours(b.xmin) + _neighbours(b.xmax) + [1e-6, 3e-5, float(F32(0.5 * (b.xmax + zmax)))]
    kn = b.knots[3:3 + n_int + 1]
    for target in [b.lo, b.hi] + [kn[m] for m in inner]:
        # (where the doubles are sparser than their logs no z lands one ulp beside the target: the neighbours in z stand in)
        out += _log_landing(target) + [v for x in _log_landing(target) if float(np.log(x)) == target for v in _neighbours(x)]
    out += [float(np.exp(0.5 * (kn[m] + kn[m + 1]))) for m in mids]
    r = _quantised(np.random.RandomState(seed).uniform(0.0, 1.0, max(12, 54 - len({v for v in out if zmin <= v <= top}))))
    out += [float(F32(v)) for v in np.exp(b.lo + (b.hi - b.lo) * r)]
    out += [2.0]
    seen, zs = set(), []
    for v in out:
        if zmin <= v and (v <= top or v == 2.0) and v not in seen:
            seen.add(v)
            zs.append(v)
    return np.array(zs, dtype=np.float64)


def _z_basis(name):
    m = Z_META[name]
    zg, _ = _z_grid()
    zmin, zmax = float(zg[0]), float(zg[-1])
    b = Basis("LogXBSpline", m["n"], m["xrange"] or (zmin, zmax))
    return b, z_samples(b, zmin, zmax, 2000 + sum(ord(ch) for ch in name))


def all_z_samples():
    return np.unique(np.concatenate([_z_basis(name)[1] for name in Z_META]))


def tabulate_cosmology():
    """Rewrite COSMOLOGY from the unmodified reference's cosmology (imported through ref_import.py); needs the reference tree."""
    import sys

    sys.path.insert(0, HERE)
    from ref_import import load_reference

    ref = load_reference()
    z = all_z_samples()
    dv = np.asarray(ref.cosmology.PLANCK_2015_LVK_Cosmology.dVcdz(ref.jnp.asarray(z)), dtype=np.float64)
    zg, dvg = _z_grid()
    assert np.array_equal(np.asarray(ref.cosmology.PLANCK_2015_LVK_Cosmology.dVcdz(ref.jnp.asarray(zg)), dtype=np.float64), dvg)
    np.savez_compressed(os.path.join(HERE, COSMOLOGY), z=z, dVcdz=dv)


def _dvcdz_at(zs):
    with np.load(os.path.join(HERE, COSMOLOGY)) as t:
        z, dv = t["z"], t["dVcdz"]
    i = np.searchsorted(z, zs)
    assert np.all(i < len(z)) and np.array_equal(z[np.minimum(i, len(z) - 1)], zs), f"{COSMOLOGY} does not hold every sample: tabulate it again"
    return dv[i]


def plz_points(N, seed):
    rs = np.random.RandomState(seed)
    z = _quantised(rs.standard_normal((3, N)))
    saw = np.array([10.0 if k % 2 == 0 else -10.0 for k in range(N)])
    hole = z[0].copy()
    hole[N // 2] = -300.0
    zero = np.zeros(N)
    return [("zeros/lamb-2", -2.0, zero), ("zeros/lamb0", 0.0, zero), ("zeros/lamb1", 1.0, zero), ("zeros/lamb2.7", 2.7, zero), ("zeros/lamb6", 6.0, zero),
            ("normal1/lamb1", 1.0, z[0]), ("normal10/lamb2.7", 2.7, 10.0 * z[1]), ("normal40/lamb-2", -2.0, 40.0 * z[2]), ("sawtooth10/lamb6", 6.0, saw),
            ("hole-300/lamb0", 0.0, hole), ("shift+300/lamb1", 1.0, z[0] + 300.0), ("shift-300/lamb1", 1.0, z[0] - 300.0)]


def zspline_points(N, seed, normalize):
    rs = np.random.RandomState(seed)
    z = _quantised(rs.standard_normal((3, N)))
    e = np.eye(N)
    saw = np.array([10.0 if k % 2 == 0 else -10.0 for k in range(N)])
    hole = z[0].copy()
    hole[N // 2] = -300.0
    # (all zeros under normalize=True is 0 / 0 in the reference: the flat point there is all ones)
    # (and 5 e_0 would be divided by I_0 ~ 1e-4, the integral of the first basis over a grid linear in z: an exponent of thousands)
    first = N // 2 if normalize else 0
    return [("ones", np.ones(N)) if normalize else ("zeros", np.zeros(N)), (f"5e{first}", 5.0 * e[first]), (f"5e{N - 1}", 5.0 * e[N - 1]), ("normal1", z[0]), ("normal10", 10.0 * z[1]),
            ("normal40", 40.0 * z[2]), ("sawtooth10", saw), ("hole-300", hole)]


def _grid_tables(b, zg, dv, divide_by_1pz):
    """Nodes, trapezoid weights, the static weight of every node (dVc/dz, over 1 + z for BSplineRedshift), log(1 + z) and the bases at
    the nodes inside the spline domain (None outside: exponent 0 there)."""
    g = [F(v) for v in zg]
    tw = _trapezoid_weights(g)
    stat = [F(d) / (1 + gi) if divide_by_1pz else F(d) for d, gi in zip(dv, g)]
    l1 = [mp.log(1 + gi) for gi in g]
    gu = b.coordinate(zg)
    Bg = [b.bases(float(u)) if b.grid_inside(float(u)) else None for u in gu]
    return g, tw, stat, l1, Bg


def _exp_grid_sum(c, tw, stat, Bg, extra=None):
    """Z = sum_g tw_g stat_g extra_g exp(sum_k c_k B_k(g)), and sum_g (the same) B_j(g) for every j."""
    N = len(c)
    Z, dZ, terms = mp.mpf(0), [mp.mpf(0)] * N, []
    for i, (w, s, Bi) in enumerate(zip(tw, stat, Bg)):
        y = w * s * (extra[i] if extra is not None else 1)
        if Bi is not None:
            y *= mp.exp(sum(c[k] * v for k, v in Bi.items()))
            for k, v in Bi.items():
                dZ[k] += y * v
        terms.append(y)
        Z += y
    return Z, dZ, terms


def _plz_term(name):
    """PowerlawSplineRedshiftModel (models/spline_perturbation.py:304-372): p = dVc/dz (1 + z)^(lamb - 1) exp(sum_k c_k B_k(log z)) / Z
    for z <= zmax, the bases 0 outside [lo, hi] (interpolation.py:175), Z the trapezoid sum of the same on the model's z grid.
    Parameters (lamb, c_0 .. c_{N-1}); columns (z, dVc/dz(z))."""
    N = Z_META[name]["n"]
    b, zs = _z_basis(name)
    zg, dvg = _z_grid()
    zmax = float(zg[-1])
    dvs = _dvcdz_at(zs)
    g, tw, stat, l1, Bg = _grid_tables(b, zg, dvg, False)
    assert all(Bi is not None for Bi in Bg)  # the basis covers the whole grid: the shift points are invariant
    us = b.coordinate(zs)
    points = plz_points(N, 2001 + sum(ord(ch) for ch in name))
    H, n = len(points), len(zs)
    logp = np.full((H, n), -np.inf)
    dlogp = np.zeros((H, 1 + N, n))
    exact = {}
    gap = max(0.0, b.knots[3] - b.lo, b.hi - b.knots[N]) / (b.knots[4] - b.knots[3])
    tol = mp.mpf(10) ** -60 + 2 * 300 * F(gap) ** 3
    for h, (tag, lamb, c_d) in enumerate(points):
        lm, c = F(lamb), [F(v) for v in c_d]
        pw = [mp.exp((lm - 1) * li) for li in l1]
        Z, dZ, terms = _exp_grid_sum(c, tw, stat, Bg, pw)
        assert Z > 0, (name, tag)
        dlam = sum((y * li for y, li in zip(terms, l1)), mp.mpf(0)) / Z
        dlogZ = [d / Z for d in dZ]
        logZ = mp.log(Z)
        if tag.startswith("zeros"):  # the power law alone: the tabulated distribution's normaliser, as _redshift_term writes it
            y = [F(d) * mp.exp((lm - 1) * li) for d, li in zip(dvg, l1)]
            Zp = _trapezoid(g, y)
            assert abs(logZ - mp.log(Zp)) < mp.mpf(10) ** -60 and abs(dlam - _trapezoid(g, [yi * li for yi, li in zip(y, l1)]) / Zp) < mp.mpf(10) ** -60, (name, tag)
        row = []
        for s, (z, u) in enumerate(zip(zs, us)):
            if not z <= zmax:
                row.append(None)
                continue
            Bs = b.bases(float(u)) if b.grid_inside(float(u)) else {}
            l1z = mp.log(1 + F(z))
            lp = mp.log(F(dvs[s])) + (lm - 1) * l1z + sum(c[k] * v for k, v in Bs.items()) - logZ
            d = [l1z - dlam] + [Bs.get(j, mp.mpf(0)) - dlogZ[j] for j in range(N)]
            row.append(lp)
            assert lp > LOG_FLOOR, (name, tag, s, float(lp))
            if tag.startswith("shift"):  # sum_j d log p / d c_j = sum_j B_j(u) - sum_j dlogZ_j = 1 - 1
                assert abs(sum(d[1:])) < tol, (name, tag, s)
            logp[h, s] = float(lp)
            dlogp[h, :, s] = [float(v) for v in d]
        exact[tag] = row
    for tag in ("shift+300/lamb1", "shift-300/lamb1"):
        for a, r in zip(exact[tag], exact["normal1/lamb1"]):
            assert (a is None) == (r is None) and (a is None or abs(a - r) < tol), (name, tag)
    return {f"{name}/params": np.array(["lamb"] + [f"c{k}" for k in range(N)]), f"{name}/columns": np.array(["z", "dVcdz"]), f"{name}/col/z": zs, f"{name}/col/dVcdz": dvs,
            f"{name}/tags": np.array([t for t, _, _ in points]), f"{name}/theta": np.array([np.concatenate([[l], c]) for _, l, c in points], dtype=np.float64),
            f"{name}/logp": logp, f"{name}/dlogp": dlogp}


def _zspline_term(name):
    """BSplineRedshift (models/bsplines/single.py:398-492): p = exp(f(z)) dVc/dz / (1 + z) / Z(c); f = sum_k e_k B_k(log z) where
    xmin <= z <= xmax (:54-55) and log z is in [lo, hi] (interpolation.py:175), 0 elsewhere; Z(c) the trapezoid sum of
    dVc/dz / (1 + z) exp(sum_k c_k B_k(log z)) on the model's z grid, exponent 0 at the nodes outside [lo, hi].  No sample is excluded.
    normalize=True (the reference's default): e = c / (c . I), I_k = trapz(B_k(grid), grid) on the basis's own 1000-point grid
    (interpolation.py:290, :343) -- a host matter; the parameters here are the two blocks (e_0 .. e_{N-1}, c_0 .. c_{N-1}), e the
    double nearest to c / (c . I), and each block is differentiated alone: d / d e_k = B_k(log z), d / d c_j = -d log Z / d c_j.
    ``{name}/I`` holds I_k.  normalize=False: one block, e = c."""
    N, normalize = Z_META[name]["n"], Z_META[name]["normalize"]
    b, zs = _z_basis(name)
    zg, dvg = _z_grid()
    dvs = _dvcdz_at(zs)
    g, tw, stat, l1, Bg = _grid_tables(b, zg, dvg, True)
    assert any(Bi is None for Bi in Bg[:5]) and any(Bi is None for Bi in Bg[-5:])  # live nodes outside the spline domain, both sides
    us = b.coordinate(zs)
    Bs = [b.bases(float(u)) if b.inside(float(z), float(u)) else {} for z, u in zip(zs, us)]
    points = zspline_points(N, 2001 + sum(ord(ch) for ch in name), normalize)
    I = [mp.mpf(0)] * N
    if normalize:
        bg = [F(v) for v in b.grid]
        for w, u in zip(_trapezoid_weights(bg), b.coordinate(b.grid)):
            if b.grid_inside(float(u)):
                for k, v in b.bases(float(u)).items():
                    I[k] += w * v
    H, n, P = len(points), len(zs), (2 * N if normalize else N)
    logp = np.full((H, n), -np.inf)
    dlogp = np.zeros((H, P, n))
    theta = np.zeros((H, P))
    for h, (tag, c_d) in enumerate(points):
        c = [F(v) for v in c_d]
        if normalize:
            cI = sum(ck * Ik for ck, Ik in zip(c, I))
            assert abs(cI) >= CONDITION * sum(abs(ck * Ik) for ck, Ik in zip(c, I)), (name, tag)
            e_d = np.array([float(ck / cI) for ck in c])
            theta[h] = np.concatenate([e_d, c_d])
        else:
            e_d = np.asarray(c_d, dtype=np.float64)
            theta[h] = c_d
        e = [F(v) for v in e_d]
        Z, dZ, _ = _exp_grid_sum(c, tw, stat, Bg)
        assert Z > 0, (name, tag)
        logZ, dlogZ = mp.log(Z), [d / Z for d in dZ]
        for s, z in enumerate(zs):
            lp = sum(e[k] * v for k, v in Bs[s].items()) + mp.log(F(dvs[s])) - mp.log(1 + F(z)) - logZ
            assert LOG_FLOOR < lp < -LOG_FLOOR, (name, tag, s, float(lp))
            logp[h, s] = float(lp)
            dB = [Bs[s].get(j, mp.mpf(0)) for j in range(N)]
            d = dB + [-v for v in dlogZ] if normalize else [bj - v for bj, v in zip(dB, dlogZ)]
            dlogp[h, :, s] = [float(v) for v in d]
    out = {f"{name}/params": np.array([f"e{k}" for k in range(N)] + [f"c{k}" for k in range(N)] if normalize else [f"c{k}" for k in range(N)]),
           f"{name}/columns": np.array(["z", "dVcdz"]), f"{name}/col/z": zs, f"{name}/col/dVcdz": dvs, f"{name}/tags": np.array([t for t, _ in points]), f"{name}/theta": theta,
           f"{name}/logp": logp, f"{name}/dlogp": dlogp}
    if normalize:
        out[f"{name}/I"] = np.array([float(v) for v in I])
    return out



# ---------------------------------------------------------------------------------------------------------------------
# BSplineDistribution: a log-density tabulated on a grid and interpolated linearly
# ---------------------------------------------------------------------------------------------------------------------
LERPS = [  # name, basis, N, xrange, (first node, last node, number of nodes): the grid reaches beyond the basis domain on one side
    ("lerp_logy7", "LogYBSpline", 7, (0.0, 1.0), (0.0, 1.25, 101)),          # above: node 80 is 1.0 = hi, nodes 81.. carry -inf
    ("lerp_logxlogy20", "LogXLogYBSpline", 20, (3.0, 100.0), (2.0, 100.0, 197)),  # below: nodes 0, 1 carry -inf, node 2 is 3.0
    ("lerp_bspline7", "BSpline", 7, (-1.0, 1.0), (-1.5, 1.0, 126)),           # below: the bases are 0 there, the log-density 0
]
LERP_META = {name: dict(basis=kind, n=N, xrange=xr, grid=gr) for name, kind, N, xr, gr in LERPS}


def lerp_samples(b, grid, seed):
    """On a node (f = 0) and one ulp either side; on grid[0] and grid[-1]; outside the grid on both sides (end values are held);
    in the last cell one ulp below the end; on the nodes at both ends of the basis domain, on the first node outside it, and inside
    the cells that touch it; cell mid-points and quarter points; seeded points over the whole grid (multiples of 2^-20)."""
    n = len(grid)
    us = b.coordinate(grid)
    inside = np.array([b.grid_inside(float(u)) for u in us])
    first, last = int(np.flatnonzero(inside)[0]), int(np.flatnonzero(inside)[-1])
    span = grid[-1] - grid[0]
    out = _neighbours(grid[n // 3]) + [float(grid[0]), float(np.nextafter(grid[0], np.inf)), float(grid[-1]), float(np.nextafter(grid[-1], -np.inf))]
    out += [float(grid[0] - 0.125 * span), float(np.nextafter(grid[0], -np.inf)), float(np.nextafter(grid[-1], np.inf)), float(grid[-1] + 0.5 * span)]
    for j in (first, last):
        out += _neighbours(grid[j])
    for j in (first - 1, first, last - 1, last):  # the cells that touch a node outside the domain, and their inner neighbours
        if 0 <= j < n - 1:
            out += [float(0.75 * grid[j] + 0.25 * grid[j + 1]), float(0.5 * (grid[j] + grid[j + 1]))]
    for j in (first - 1, last + 1):
        if 0 <= j < n:
            out.append(float(grid[j]))
    out += [float(0.5 * (grid[j] + grid[j + 1])) for j in sorted({0, 1, n // 5, n // 2, (2 * n) // 3, n - 3, n - 2})]
    r = _quantised(np.random.RandomState(seed).uniform(0.0, 1.0, 64))
    for v in _quantised(grid[0] + span * r):
        if len(set(out)) >= 54:
            break
        out.append(float(v))
    seen, xs = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            xs.append(v)
    return np.array(xs, dtype=np.float64)


def _lerp_term(name):
    """BSplineDistribution.log_prob (numpyro_distributions.py:266-293): lpdf_g = sum_k c_k B_k(grid_g) at the nodes inside the basis
    domain; outside it the design matrix of a log-Y basis holds -inf (interpolation.py:407, :449) and that of a linear one 0 (:175).
    log_prob(x) = interp(x, grid, lpdf) - log trapz(exp(lpdf), grid), linear between the nodes, the end values held outside the grid,
    the cell of x being grid[j] <= x < grid[j+1] (compared as doubles); no sample is masked.

    A NODE WITH -inf: c_k (-inf) summed over k is NaN for coefficients of mixed sign or with a zero among them, -inf for positive
    ones, and ``nan_to_num(nan=-inf)`` makes both -inf (all-negative coefficients give +inf, which nan_to_num turns into 1.8e308: not a
    density; ``_compute`` asserts that no hyper-point is one).  A sample strictly inside a cell that touches such a node, or on the
    node, has log_prob = -inf (NaN = inf - inf under jax.numpy's interp, -inf under numpy's: zero weight either way).  A sample
    EXACTLY ON THE LAST FINITE NODE whose right-hand partner is -inf has weight 0 on that partner: numpy.interp returns the node's own
    finite value, which is also the limit from the left, and that is what is recorded here -- and what the unmodified reference yields
    when run through ref_import.py, whose jax.numpy stand-in is numpy (``confirm_lerp_convention``, run with --tabulate).  jax.numpy's
    own interp evaluates fp[j] + 0 * (fp[j+1] - fp[j]) = NaN there, which a hierarchical likelihood counts as zero weight."""
    m = LERP_META[name]
    N = m["n"]
    b = Basis(m["basis"], N, m["xrange"])
    grid = np.linspace(*m["grid"])
    assert len(grid) <= 200
    seed = 3000 + sum(ord(ch) for ch in name)
    xs = lerp_samples(b, grid, seed)
    points = [pt for pt in exp_points(N, seed + 1) if not pt[0].startswith("shift")]  # (a shift is invariant only where the basis covers the grid)
    g = [F(v) for v in grid]
    tw = _trapezoid_weights(g)
    Bg = [b.bases(float(u)) if b.grid_inside(float(u)) else None for u in b.coordinate(grid)]
    assert any(Bi is None for Bi in Bg)
    cell = np.clip(np.searchsorted(grid, xs, side="right") - 1, 0, len(grid) - 2)
    H, n = len(points), len(xs)
    logp = np.full((H, n), -np.inf)
    dlogp = np.zeros((H, N, n))
    for h, (tag, c_d) in enumerate(points):
        assert not np.all(c_d < 0), (name, tag)
        c = [F(v) for v in c_d]
        lp = [sum(c[k] * v for k, v in Bi.items()) if Bi is not None else (None if b.log_y else mp.mpf(0)) for Bi in Bg]
        Z, dZ = mp.mpf(0), [mp.mpf(0)] * N
        for w, l, Bi in zip(tw, lp, Bg):
            if l is not None:
                y = w * mp.exp(l)
                Z += y
                for k, v in (Bi or {}).items():
                    dZ[k] += y * v
        assert Z > 0, (name, tag)
        logZ, dlogZ = mp.log(Z), [d / Z for d in dZ]
        for s, (x, j) in enumerate(zip(xs, cell)):
            j = int(j)
            f = min(max((F(x) - g[j]) / (g[j + 1] - g[j]), mp.mpf(0)), mp.mpf(1))  # the end values are held outside the grid
            parts = [(wt, j + e) for e, wt in ((0, 1 - f), (1, f)) if wt != 0]
            if any(lp[i] is None for _, i in parts):
                continue
            val = sum(wt * lp[i] for wt, i in parts) - logZ
            assert val > LOG_FLOOR, (name, tag, s, float(val))
            logp[h, s] = _rounded(val)
            d = [-v for v in dlogZ]
            for wt, i in parts:
                for k, v in (Bg[i] or {}).items():
                    d[k] += wt * v
            dlogp[h, :, s] = [float(v) for v in d]
    return {f"{name}/params": np.array([f"c{k}" for k in range(N)]), f"{name}/columns": np.array(["x"]), f"{name}/col/x": xs, f"{name}/grid": grid,
            f"{name}/tags": np.array([t for t, _ in points]), f"{name}/theta": np.array([c for _, c in points], dtype=np.float64), f"{name}/logp": logp, f"{name}/dlogp": dlogp}


def confirm_lerp_convention():
    """Run the unmodified reference's BSplineDistribution (through ref_import.py) on every LERP term at ``normal1`` and assert that
    it is dead exactly where the fixture is and finite on the last finite node next to a -inf one; needs the reference tree."""
    import sys

    sys.path.insert(0, HERE)
    from ref_import import load_reference

    ref = load_reference()
    for name, m in LERP_META.items():
        with mp.workdps(DPS):
            a = _lerp_term(name)
        grid, xs = a[f"{name}/grid"], a[f"{name}/col/x"]
        h = [str(t) for t in a[f"{name}/tags"]].index("normal1")
        kw = dict(xrange=m["xrange"]) if m["basis"] != "BSpline" else dict(xrange=m["xrange"], normalize=False)
        basis = getattr(ref.interpolation, m["basis"])(m["n"], **kw)
        with np.errstate(all="ignore"):
            dist = ref.numpyro_distributions.BSplineDistribution(grid[0], grid[-1], ref.jnp.asarray(a[f"{name}/theta"][h]), ref.jnp.asarray(grid), ref.jnp.asarray(basis.bases(ref.jnp.asarray(grid))))
            got = np.asarray(dist.log_prob(ref.jnp.asarray(xs)), dtype=np.float64)
        want = a[f"{name}/logp"][h]
        dead = np.isneginf(want)
        assert np.array_equal(~np.isfinite(got) | (got < -1e300), dead), (name, np.flatnonzero((~np.isfinite(got) | (got < -1e300)) != dead))
        assert np.max(np.abs(got[~dead] - want[~dead])) < 1e-9, name


def names():
    return [s[0] for s in SPLINES] + ["powerlaw_redshift"] + [s[0] for s in Z_SPLINES] + [s[0] for s in LERPS]


def _compute(dps, only=None):
    out = {}
    with mp.workdps(dps):
        for spec in SPLINES:
            if only is None or spec[0] in only:
                out[PREFIX + spec[0] + ".npz"] = _spline_term(*spec)
        if only is None or "powerlaw_redshift" in only:
            out[PREFIX + "powerlaw_redshift.npz"] = _redshift_term()
        for name, model, _, _, _ in Z_SPLINES:
            if only is None or name in only:
                out[PREFIX + name + ".npz"] = _plz_term(name) if model == "PowerlawSplineRedshiftModel" else _zspline_term(name)
        for spec in LERPS:
            if only is None or spec[0] in only:
                out[PREFIX + spec[0] + ".npz"] = _lerp_term(spec[0])
    return out


def generate(verify=True, only=None):
    """{file name: arrays}.  ``verify``: compute them again with twice the digits and assert that no double changes."""
    out = _compute(DPS, only)
    if verify:
        again = _compute(2 * DPS, only)
        for fn, arrays in out.items():
            for k, v in arrays.items():
                assert np.array_equal(v, again[fn][k]), f"{k}: {DPS} digits are not enough"
    return out


if __name__ == "__main__":
    import sys

    if "--tabulate" in sys.argv[1:]:
        tabulate_cosmology()
        confirm_lerp_convention()
    for fn, arrays in generate(verify=True).items():
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < 256 * 1024, (fn, size)
        print(f"wrote {path}: {size} bytes")
