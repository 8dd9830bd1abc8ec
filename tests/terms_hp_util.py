"""Shared by tests/test_terms_hp_cpu.py, tests/test_mass_forms_hp_cpu.py (C oracle), tests/test_gpu_terms_hp.py,
tests/test_gpu_spline_terms_hp.py and tests/test_gpu_mass_forms_hp.py (engine): the high-precision term fixtures
(tests/golden/terms_hp.npz, written by tests/golden/make_terms_hp.py; tests/golden/spline_terms_hp_*.npz, written by
tests/golden/make_spline_terms_hp.py; tests/golden/mass_forms_hp.npz, written by tests/golden/make_mass_forms_hp.py), the drop-in
model call of every term in them, the catalogs that make a summed gradient transparent, and the assertions -- the same ones, with the
same bars, for both.

An EVALUATOR is anything with ``log_weights(theta) -> (n_ev, n_pe) array`` and ``evaluate(theta, total_inj) -> (log_l, grad)``
on a catalog it was built for; ``make(d_pe, d_inj)`` builds one from a pair of lazy densities and must expose ``.bound``.

Catalogs (the engine returns only the summed gradient):
  values  every sample of the fixture as an event of ONE sample: the log-weight of event i is the log-density of sample i.
  A       the samples that are in the support at every hyper-point ("core"), one per event, and ONE injection x_0 with
          total_inj = 1:  log_l = sum_i l(x_i) - B l(x_0),  grad_j = sum_i g_j(x_i) - B g_j(x_0).
  B       events of 3 samples, 5 injections, total_inj = 5; samples that are excluded at some hyper-points ride along with core
          ones.  Reference: the weight-averaged form, assembled from the fixture in np.longdouble.
  pinned  the spline redshift models take zmin, zmax and their z grid from the data: for their terms (and products with one) both sides
          of every catalog carry the two end samples and no injection lies beyond zmax (``pins``); A has injections {z_lo, x_0, z_hi}
          and total_inj = 3.  ``check_tables`` holds the models' grid and dVc/dz tables to the fixture's when a catalog is built.
"""
import glob
import os

import numpy as np
from golden_util import GOLDEN_DIR

VALUE_ATOL = 1e-11  # term-level bar of tests/test_gpu_terms.py, uniform over the exponent sweep
GRAD_RTOL = 1e-8    # per COMPONENT: |got_j - ref_j| <= GRAD_RTOL max(1, |ref_j|)
LOGL_RTOL = 1e-9    # |got - ref| <= LOGL_RTOL |ref|, as tests/test_gpu_fuzz.py and tests/test_c_oracle.py
# The hyper-points at which the density is flat (xi = 0, Beta(1, 1)) or flat to 1e-12 (xi = 1e-12): there the sums log_l is assembled
# from cancel, exactly or to ~1e-10 of their size, the fixture's log_l is 0 or below 2.1e-9, and a bar relative to it asks for digits
# that no float64 sum of numbers of order 20-40 holds.  At these tags ALONE the bar is LOGL_RTOL of the largest of those sums (an
# absolute floor of 1.6e-8 to 4.2e-8); everywhere else it is relative to |log_l| itself.
LOGL_CANCELLED = {
    "tilt": {"xi0/sig0.05", "xi0/sig1", "xi0/sig6", "xi1e-12/sig0.05", "xi1e-12/sig1", "xi1e-12/sig6"},
    "tilt_joint": {"xi0/sig0.05", "xi0/sig1", "xi0/sig6", "xi1e-12/sig0.05", "xi1e-12/sig1", "xi1e-12/sig6"},
    "beta": {"a1/b1"},
}

# The spline fixture: name -> (basis, number of coefficients, xrange, float32 samples).  tests/test_terms_hp_cpu.py holds this table to
# the generator's own.
SPLINE_TERMS = {
    "logy4": ("LogYBSpline", 4, (0.0, 1.0), False), "logy7": ("LogYBSpline", 7, (-1.0, 1.0), False), "logy16": ("LogYBSpline", 16, (0.0, 1.0), False),
    "logy17": ("LogYBSpline", 17, (0.0, 1.0), False), "logy20": ("LogYBSpline", 20, (0.0, 1.0), False), "logy7_f32": ("LogYBSpline", 7, (0.0, 1.0), True),
    "logxlogy4": ("LogXLogYBSpline", 4, (0.1, 1.0), False), "logxlogy17": ("LogXLogYBSpline", 17, (2.0, 100.0), False),
    "logxlogy20": ("LogXLogYBSpline", 20, (3.0, 100.0), False),
    "bspline4": ("BSpline", 4, (0.0, 1.0), False), "bspline7": ("BSpline", 7, (-1.0, 1.0), False), "bspline17": ("BSpline", 17, (0.0, 1.0), False),
    "bspline7_f32": ("BSpline", 7, (0.0, 1.0), True),
    "logx4": ("LogXBSpline", 4, (0.01, 1.0), False), "logx7": ("LogXBSpline", 7, (0.001, 2.3), False), "logx17": ("LogXBSpline", 17, (0.01, 1.0), False),
}
# The spline redshift models of the same fixture: name -> (model, number of coefficients, xrange (None: the data range), normalize).
# Their z grid comes from the DATA (the common range of the two sides), so their catalogs are built to pin it: see ``pins``.
Z_SPLINE_TERMS = {
    "plzspline4": ("PowerlawSplineRedshiftModel", 4, None, False), "plzspline7": ("PowerlawSplineRedshiftModel", 7, None, False),
    "plzspline17": ("PowerlawSplineRedshiftModel", 17, None, False),
    "zspline4": ("BSplineRedshift", 4, (1e-4, 1.5), True), "zspline16": ("BSplineRedshift", 16, (1e-4, 1.5), True), "zspline17": ("BSplineRedshift", 17, (1e-4, 1.5), True),
    "zspline7_raw": ("BSplineRedshift", 7, (1e-4, 1.5), False),
}
# BSplineDistribution.log_prob (GWI_TERM_EXP_SPLINE_LERP) of the same fixture: name -> (basis, number of coefficients, xrange, (first
# node, last node, number of nodes) of the grid, which reaches beyond the basis domain on one side).
LERP_TERMS = {
    "lerp_logy7": ("LogYBSpline", 7, (0.0, 1.0), (0.0, 1.25, 101)), "lerp_logxlogy20": ("LogXLogYBSpline", 20, (3.0, 100.0), (2.0, 100.0, 197)),
    "lerp_bspline7": ("BSpline", 7, (-1.0, 1.0), (-1.5, 1.0, 126)),
}
TABLE_RTOL = 1e-13  # the models' dVc/dz tables against the fixture's: two orders under VALUE_ATOL (the cosmology is input data)
SPLINE_FIXTURE_TERMS = list(SPLINE_TERMS) + ["powerlaw_redshift"] + list(Z_SPLINE_TERMS) + list(LERP_TERMS)
# A flat density again: all coefficients zero under the exponential, all coefficients one for a linear spline (the bases sum to one
# inside the domain).  Every log-density is then the same number -log Z (0 on a domain of length 1), the fixture's log_l is 0 or the
# rounding of sums that cancel, and the bar is relative to those sums as above.  On a domain of length 1 the sums themselves are 0
# (every log-density is 0, one sample per event): there the floor is LOGL_RTOL x 1, which is what the VALUE bar already allows a sum of
# up to 50 log-weights, each within VALUE_ATOL = 1e-11 (the older cancelled tags have sums of 16 to 42 and are not touched by it).
for _name, (_basis, _, _, _) in SPLINE_TERMS.items():
    LOGL_CANCELLED[_name] = {"zeros"} if "LogY" in _basis else {"ones"}
# The tabulated log-density at all-zero coefficients is exactly flat wherever it is finite (lpdf = 0 at every live node): the same
# cancellation, barred relative to the cancelled sums (n_obs |log Z|; log Z = log 1.00625, log 97.25 and log 2.5 for the three grids).
for _name in LERP_TERMS:
    LOGL_CANCELLED[_name] = {"zeros"}
# ``dip`` (all ones but one coefficient at -2) with 17 coefficients, ON CATALOG A ONLY: the samples that are live at EVERY hyper-point,
# which is all that catalog A is made of, lie outside the four intervals the negative coefficient touches -- among them the spline is
# flat again.  Catalog B also carries samples inside the dip and is held to the plain relative bar.
LOGL_CANCELLED_A = {"bspline17": {"dip"}, "logx17": {"dip"}}

# The pairing factor (m2 / m1)^beta at beta = 0 is 1 for every pair: every live sample has the same log-density, 0.
LOGL_CANCELLED["pairing_iid"] = {"beta0"}
LOGL_CANCELLED["pairing_indep"] = {"beta0"}

# ``plbounds`` on the narrow intervals, ON CATALOG A ONLY: catalog A of that nest of intervals is made of the samples inside its
# narrowest one, [30, 30.00003], across which x^alpha changes by |alpha| 1e-6 -- every live sample has the same log-density to six
# digits.  log_l is then ~1e-5 (4.5e-6 at alpha = -1 - 1e-6) assembled from sums of ~30: a bar of 1e-9 relative to it asks for 4e-15
# absolute, 1.5e-16 of the sums, which ten float64 additions do not hold (the C oracle's error there is 1.1e-14).  Catalog B of the same
# points carries samples from all of [30, 33] and is held to the plain relative bar, as are the values and every gradient component.
LOGL_CANCELLED_A["plbounds"] = {f"narrow{w}/alpha{a}" for w in ("1e-1", "1e-3", "1e-6") for a in ("-2.5", "-1+1e-6", "-1-1e-6", "-1")}

# tests/golden/mass_forms_hp.npz: the terms, and for the mass-ratio power laws the call's mmin; tests/test_mass_forms_hp_cpu.py holds
# this table and the numbers below to the generator's.
MASS_FORM_TERMS = ["plbounds", "pairing_iid", "pairing_indep", "ratio_on_logxlogy20_mmin3", "ratio_on_logxlogy20_mmin5"]
RATIO_MMIN = {"ratio_on_logxlogy20_mmin3": 3.0, "ratio_on_logxlogy20_mmin5": 5.0}
# ``ratio_on_logxlogy20_*``: log p is ill-conditioned in log m1 next to m1 = mmin (d log p / d log m1 ~ 1 / log(mmin / m1)), and log m1
# is a ROUNDED input of the term: the value bar at sample i is VALUE_ATOL + |dlogp_dlogm1[i]| eps_lm, with eps_lm the error of the
# log m1 the term works with -- derived from the arithmetic in the source, never from what a device returned.  u = 2^-53.
#   own column (GWI_FOLD_LOGM=0): the term reads log m1 as the setup kernel's logarithm wrote it: one ulp of log m1.  m1 <= 100, so
#     log m1 < 8 and an ulp is at most 2^-50:                                            EPS_LM_OWN = 2^-50 = 8.9e-16.
#   folded (GWI_RATIO_LOGM_FROM_SPLINE): the term rebuilds log m1 = fma(u, dx, lo) from the m1 spline's knot coordinate
#     u = (log m1 - lo) inv_dx (gwi_ingest.h: spline_knot_kernel, contraction off; engine.py: inv_dx = n_int / (hi - lo),
#     dx = (hi - lo) / n_int).  With D = log m1 - lo <= log(100 / 3) < 4, on top of the column's own ulp:
#       the subtraction                        D u
#       hi - lo and the division in inv_dx      2 D u
#       the product (log m1 - lo) inv_dx        D u
#       the clamp into [0, nextafter(n_int, 0)] D 2u   (a live sample lies in the closed domain: only x = hi moves, by one ulp of u)
#       hi - lo and the division in dx          2 D u
#       the one rounding of fma(u, dx, lo)      half an ulp of log m1 < 8: 2^-51
#     (lo itself is the same double in the subtraction and in the FMA and cancels.)  8 D u + 2^-51 <= 4 x 2^-50 + 2^-51:
#                                                                                      EPS_LM_FOLD = 5.5 x 2^-50 = 4.9e-15.
# The gradient bar gains the same product with the second derivative d^2 log p / d beta d log m1 (and, in an event of several
# samples, with the move of the weights; ``_conditioning``).  A sample whose conditioning term exceeds COND_CAP tells nothing about
# the arithmetic: only its liveness is compared, it stays out of the gradient catalogs, and the generator asserts that there are at
# most two per mmin (the nextafter neighbour above 3.0, where 1 / log(m1 / mmin) = 6.8e15).
EPS_LM_OWN = 2.0**-50
EPS_LM_FOLD = EPS_LM_OWN + 4.0 * 2.0**-50 + 2.0**-51
COND_CAP = 1e-9

MMIN, MMAX = 5.0, 100.0


def load():
    return np.load(os.path.join(GOLDEN_DIR, "terms_hp.npz"))


def spline_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "spline_terms_hp_*.npz")))


def load_spline():
    """The arrays of every tests/golden/spline_terms_hp_*.npz in one dict (one file per term; their keys carry the term's name)."""
    out = {}
    for path in spline_files():
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def load_mass_forms():
    with np.load(os.path.join(GOLDEN_DIR, "mass_forms_hp.npz")) as z:
        return {k: z[k] for k in z.files}


_Z_TABLE = []


def _z_table():
    """(z grid, dVc/dz, maximum) of tests/golden/terms.npz: loaded once, the distribution keys its tables on the arrays' identity."""
    if not _Z_TABLE:
        with np.load(os.path.join(GOLDEN_DIR, "terms.npz")) as z:
            _Z_TABLE.extend([z["dist/z_grid"], z["dist/z_dVcdz"], float(z["dist/powerlaw_redshift/maximum"])])
    return _Z_TABLE


class Term:
    def __init__(self, z, name):
        self.name = name
        self.params = [str(p) for p in z[f"{name}/params"]]
        self.columns = [str(c) for c in z[f"{name}/columns"]]
        self.cols = [z[f"{name}/col/{c}"] for c in self.columns]
        self.tags = [str(t) for t in z[f"{name}/tags"]]
        self.theta = z[f"{name}/theta"]
        self.logp = z[f"{name}/logp"]
        self.dlogp = z[f"{name}/dlogp"]

    @property
    def n(self):
        return len(self.cols[0])


class Product(Term):
    """Fixture terms on disjoint columns and parameters as one model: sample i is every part's sample i, hyper-point h is every part's
    point h mod its number of points, h running over the longest list."""

    def __init__(self, *parts):
        n = min(t.n for t in parts)
        hs = [np.arange(max(len(t.theta) for t in parts)) % len(t.theta) for t in parts]
        self.name = "*".join(t.name for t in parts)
        self.parts = parts
        self.part_points = hs
        self.params = [f"{t.name}.{p}" for t in parts for p in t.params]
        self.cols = [c[:n] for t in parts for c in t.cols]
        self.tags = ["|".join(t.tags[h[k]] for t, h in zip(parts, hs)) for k in range(len(hs[0]))]
        self.theta = np.concatenate([t.theta[h] for t, h in zip(parts, hs)], axis=1)
        self.logp = sum(t.logp[h][:, :n] for t, h in zip(parts, hs))
        self.dlogp = np.concatenate([t.dlogp[h][:, :, :n] for t, h in zip(parts, hs)], axis=1)
        dead = np.isneginf(self.logp)
        self.dlogp = np.where(dead[:, None, :], 0.0, self.dlogp)


class Shared(Term):
    """ONE fixture term read twice with ONE coefficient vector (the IID pair models: two terms scatter into the same gradient slots):
    sample i is (x_i, x_perm[i]), its log-density and every derivative the sum of the two, dead where either part is."""

    def __init__(self, term, perm):
        perm = np.asarray(perm)
        assert len(term.cols) == 1 and sorted(perm.tolist()) == list(range(term.n))
        self.base, self.perm = term, perm
        self.name = f"shared({term.name})"
        self.params, self.tags, self.theta = term.params, term.tags, term.theta
        self.columns = ["x1", "x2"]
        self.cols = [term.cols[0], np.ascontiguousarray(term.cols[0][perm])]
        self.logp = term.logp + term.logp[:, perm]
        dead = np.isneginf(self.logp)
        self.dlogp = np.where(dead[:, None, :], 0.0, term.dlogp + term.dlogp[:, :, perm])


class RatioTerm(Term):
    """``ratio_on_logxlogy20_*`` of mass_forms_hp.npz: the call's mmin and the two conditioning arrays with the term."""

    def __init__(self, z, name):
        super().__init__(z, name)
        self.mmin = float(z[f"{name}/mmin"])
        self.cond = z[f"{name}/dlogp_dlogm1"]                       # (H, n)
        self.cond2 = z[f"{name}/d2logp_dbeta_dlogm1"][:, None, :]   # (H, 1, n)


class Subset(Term):
    """The samples ``idx`` of a fixture term, in that order, under a name of its own (a second reading of one term in a ``Product``)."""

    def __init__(self, term, idx, name):
        idx = np.asarray(idx)
        self.name, self.params, self.columns, self.tags, self.theta = name, term.params, term.columns, term.tags, term.theta
        self.cols = [np.ascontiguousarray(c[idx]) for c in term.cols]
        self.logp, self.dlogp = term.logp[:, idx], term.dlogp[:, :, idx]
        self.base_term = term


class Joint(Term):
    """Fixture terms that SHARE A COLUMN as one model (``Product`` is for disjoint columns): a column of a later part that equals one
    already seen is that column.  ``Joint(logxlogy20, ratio_on_logxlogy20_*)`` share m1 (BSplinePrimaryPowerlawRatio);
    ``Joint(Shared(logxlogy17), pairing_*)`` share both (the component-mass models).  Parameters are the parts' in turn; sample i is
    every part's sample i, hyper-point h every part's point h mod its number of points; dead where any part is."""

    def __init__(self, *parts):
        n = parts[0].n
        assert all(t.n == n for t in parts)
        hs = [np.arange(max(len(t.theta) for t in parts)) % len(t.theta) for t in parts]
        self.name = "&".join(t.name for t in parts)
        self.parts, self.part_points = parts, hs
        self.params = [f"{t.name}.{p}" for t in parts for p in t.params]
        self.cols, self.col_of = [], []
        for t in parts:
            at = []
            for c in t.cols:
                hit = [k for k, have in enumerate(self.cols) if np.array_equal(have, c)]
                if not hit:
                    self.cols.append(c)
                at.append(hit[0] if hit else len(self.cols) - 1)
            self.col_of.append(at)
        assert len(self.cols) < sum(len(t.cols) for t in parts), "no column is shared: this is a Product"
        self.tags = ["|".join(t.tags[h[k]] for t, h in zip(parts, hs)) for k in range(len(hs[0]))]
        self.theta = np.concatenate([t.theta[h] for t, h in zip(parts, hs)], axis=1)
        self.logp = sum(t.logp[h] for t, h in zip(parts, hs))
        dead = np.isneginf(self.logp)
        self.dlogp = np.where(dead[:, None, :], 0.0, np.concatenate([t.dlogp[h] for t, h in zip(parts, hs)], axis=1))
        # conditioning with respect to a rounded input (the ratio term's log m1): |d log p / d log m1| and the same for every
        # derivative; zero for the parts that have none
        if any(hasattr(t, "cond") for t in parts):
            self.cond = np.where(dead, 0.0, sum(t.cond[h] for t, h in zip(parts, hs) if hasattr(t, "cond")))
            self.cond2 = np.where(dead[:, None, :], 0.0, np.concatenate([t.cond2[h] if hasattr(t, "cond2") else np.zeros_like(t.dlogp[h]) for t, h in zip(parts, hs)], axis=1))
            self.waived = np.flatnonzero((np.abs(self.cond) * EPS_LM_FOLD > COND_CAP).any(axis=0))

    @property
    def kind(self):
        return self.parts[-1].name


class LerpModel:
    """The grid and design matrix of a BSplineDistribution term, made ONCE per catalog (the distribution keys its device tables on the
    identity of the two arrays), and the drop-in call on them."""

    def __init__(self, name):
        from gwinferno_amd import interpolation as I

        basis, n, xrange, grid = LERP_TERMS[name]
        self.grid = np.linspace(*grid)
        self.dmat = getattr(I, basis)(n, xrange=xrange).bases(self.grid)

    def __call__(self, x, cs):
        from gwinferno_amd import numpyro_distributions as D

        return D.BSplineDistribution(self.grid[0], self.grid[-1], cs, self.grid, self.dmat).log_prob(x)


def base_name(term):
    return term.base.name if isinstance(term, Shared) else term.name


def check_tables(name, model, pe, inj):
    """The z grid of a spline redshift model must be the fixture's EXACTLY and its dVc/dz tables the fixture's to TABLE_RTOL, before
    any density is compared: a miss here names the table, not the spline."""
    zg, dv, _ = _z_table()
    assert model.zmin == zg[0] and model.zmax == zg[-1], f"{name}: the catalog does not pin the redshift range: ({model.zmin!r}, {model.zmax!r})"
    grid, table = (model.zs, model.dVdz_) if Z_SPLINE_TERMS[name][0] == "PowerlawSplineRedshiftModel" else (model.zgrid, model.dVcdzgrid)
    assert np.array_equal(grid, zg), f"{name}: the model's z grid is not the fixture's"
    err = np.max(np.abs(table / dv - 1.0))
    assert err <= TABLE_RTOL, f"{name}: dVc/dz on the z grid differs from the fixture's table by {err:.3e} relative"
    if Z_SPLINE_TERMS[name][0] == "PowerlawSplineRedshiftModel":  # this model tabulates dVc/dz at the samples itself
        for side, got, ref in (("injection", model.dVdzs[0], inj[1]), ("posterior", model.dVdzs[1], pe[1])):
            err = np.max(np.abs(np.asarray(got) / ref - 1.0))
            assert err <= TABLE_RTOL, f"{name}: dVc/dz at the {side} samples differs from the fixture's column by {err:.3e} relative"


def model_of(name, pe, inj):
    """The model OBJECT of a term whose drop-in call is a method of one (the spline models are constructed on both data arrays and
    called with ``pe_samples=``); None for the terms that are plain functions.  ``name``: a term's name, or a ``Shared`` term."""
    from gwinferno_amd import interpolation as I
    from gwinferno_amd import models as M

    if isinstance(name, Joint) or name in ("pairing_iid", "pairing_indep"):
        kind = name.kind if isinstance(name, Joint) else name
        if kind in ("pairing_iid", "pairing_indep"):  # columns (m1, m2); the splines are logxlogy17's
            basis, n, (mmin, mmax), _ = SPLINE_TERMS["logxlogy17"]
            assert basis == "LogXLogYBSpline" and (not isinstance(name, Joint) or base_name(name.parts[0]) == "logxlogy17")
            if kind == "pairing_iid":
                return M.BSplineIIDComponentMasses(n, pe[0], pe[1], inj[0], inj[1], mmin=mmin, mmax=mmax)
            return M.BSplineIndependentComponentMasses(n, n, pe[0], pe[1], inj[0], inj[1], mmin1=mmin, mmax1=mmax, mmin2=mmin, mmax2=mmax)
        basis, n, (mmin, mmax), _ = SPLINE_TERMS["logxlogy20"]  # columns (m1, q)
        assert kind in RATIO_MMIN and name.parts[0].name == "logxlogy20" and basis == "LogXLogYBSpline"
        return M.BSplinePrimaryPowerlawRatio(n, pe[0], inj[0], mmin=mmin, mmax=mmax)
    if isinstance(name, Shared):
        basis, n, xrange, _ = SPLINE_TERMS[name.base.name]
        assert basis == "LogYBSpline" and xrange in ((0.0, 1.0), (-1.0, 1.0))
        cls = M.BSplineIIDSpinMagnitudes if xrange == (0.0, 1.0) else M.BSplineIIDSpinTilts
        return cls(n, pe[0], pe[1], inj[0], inj[1])
    if name in LERP_TERMS:
        return LerpModel(name)
    if name in Z_SPLINE_TERMS:
        kind, n, xrange, normalize = Z_SPLINE_TERMS[name]
        if kind == "PowerlawSplineRedshiftModel":
            model = M.PowerlawSplineRedshiftModel(n, pe[0], inj[0])
        else:
            model = M.BSplineRedshift(n, pe[0], inj[0], pe[1], inj[1], xrange=xrange, normalize=normalize)
        check_tables(name, model, pe, inj)
        return model
    if name not in SPLINE_TERMS:
        return None
    basis, n, xrange, _ = SPLINE_TERMS[name]
    return M.Base1DBSplineModel(n, pe[0], inj[0], xrange=xrange, basis=getattr(I, basis), normalize=True)


def density(name, cols, p, model=None, pe_samples=True):
    """The drop-in model call of fixture term ``name`` on the data arrays ``cols`` (PE- or injection-shaped) at parameters ``p``;
    ``model``: what ``model_of`` made on the catalog's two sides, ``pe_samples`` which of them ``cols`` is."""
    from gwinferno_amd import models as M

    if isinstance(name, Joint):
        coefs = np.asarray(p[:-1], dtype=np.float64)  # ONE array: the binder gives one block of slots to a vector it meets twice
        if name.kind == "pairing_iid":
            return model(coefs, p[-1], pe_samples=pe_samples)
        if name.kind == "pairing_indep":
            return model(coefs, coefs, p[-1], pe_samples=pe_samples)
        return model(cols[0], cols[1], p[-1], RATIO_MMIN[name.kind], coefs, pe_samples=pe_samples)
    if name in ("pairing_iid", "pairing_indep"):  # the pairing factor alone, as the component-mass models form it
        return model._pairing(p[0], pe_samples)
    if name == "plbounds" or name.startswith("plbounds:"):
        from gwinferno_amd import numpyro_distributions as D

        return D.Powerlaw(p[0], minimum=p[1], maximum=p[2]).log_prob(cols[0])
    if name in LERP_TERMS:
        return model(cols[0], np.asarray(p, dtype=np.float64))
    if name in Z_SPLINE_TERMS:
        kind, n, _, normalize = Z_SPLINE_TERMS[name]
        p = np.asarray(p, dtype=np.float64)
        if kind == "PowerlawSplineRedshiftModel":
            return model(cols[0], p[0], p[1:])
        if not normalize:
            return model(p, pe_samples=pe_samples)
        # theta as the engine lays it out: the exponent's block e and the normaliser's block c, each a parameter of its own here (the
        # host's e = c / (c . I) is held to the fixture in tests/test_terms_hp_cpu.py)
        return model(p[n:], pe_samples=pe_samples, exponent_coefs=p[:n])
    if model is not None:
        return model(np.asarray(p, dtype=np.float64), pe_samples=pe_samples)
    if name == "powerlaw_redshift":
        from gwinferno_amd import numpyro_distributions as D

        zg, dv, maximum = _z_table()
        return D.PowerlawRedshift(p[0], maximum, zg, dv).log_prob(cols[0])
    if name == "powerlaw":
        return M.powerlaw_pdf(cols[0], p[0], MMIN, MMAX)
    if name == "plpeak":
        return M.plpeak_primary_pdf(cols[0], p[0], MMIN, MMAX, p[1], p[2], p[3])
    if name == "plpeak_ratio":
        return M.plpeak_primary_ratio_pdf(cols[0], cols[1], p[0], p[1], MMIN, MMAX, p[2], p[3], p[4])
    if name == "ratio":  # columns (q, m1, mmin / m1): the per-sample lower bound is a data array of its own
        return M.powerlaw_pdf(cols[0], p[0], cols[2], 1)
    if name == "plpeak_smooth":
        return M.plpeak_primary_pdf(cols[0], p[0], MMIN, MMAX, p[1], p[2], p[3], delta=p[4])
    if name == "tilt":
        return M.mixture_isoalign_spin_tilt(cols[0], p[0], p[1])
    if name == "tilt_joint":
        return M.default_spin_tilt(cols[0], cols[1], p[0], p[1])
    if name == "beta":
        return M.betadist(cols[0], p[0], p[1])
    if name == "truncnorm":
        return M.truncnorm_pdf(cols[0], p[0], p[1], 0.0, 1.0)
    raise KeyError(name)


class Catalog:
    """Sample indices of a fixture term arranged as events and injections, and the model bound to them."""

    def __init__(self, term, make, pe_idx, inj_idx):
        self.term = term
        self.pe_idx, self.inj_idx = np.asarray(pe_idx), np.asarray(inj_idx)
        self.pe = [np.ascontiguousarray(c[self.pe_idx]) for c in term.cols]
        self.inj = [np.ascontiguousarray(c[self.inj_idx]) for c in term.cols]
        if term.name == "ratio":  # mmin / m1 once: the model functions key their columns on the identity of the arrays
            with np.errstate(all="ignore"):
                self.pe.append(MMIN / self.pe[1])
                self.inj.append(MMIN / self.inj[1])
        parts = term.parts if isinstance(term, Product) else (term,)
        at = np.cumsum([0] + [len(t.cols) for t in parts])
        self.models = [model_of(t if isinstance(t, (Shared, Joint)) else t.name, self.pe[a:b], self.inj[a:b]) for t, a, b in zip(parts, at[:-1], at[1:])]
        p0 = term.theta[0]
        self.ev = make(self._density(self.pe, p0), self._density(self.inj, p0))
        # theta slot of every named parameter: bind the model once more, lazily, with marker values (distinct and positive: the
        # coefficients of a spline are one vector parameter, and a linear spline is defined for a positive one)
        marks = np.arange(1.0, len(term.params) + 1.0)
        layout = self.ev.bound.theta_of(self._density(self.pe, marks))
        self.slot = [int(np.flatnonzero(layout == m)[0]) for m in marks]
        assert self.ev.bound.n_theta == len(marks)

    def _density(self, cols, p):
        t = self.term
        pe = cols is self.pe
        if isinstance(t, Product):
            from gwinferno_amd.lazy import Density

            out, c0, p0 = None, 0, 0
            for part, model in zip(t.parts, self.models):
                d = density(part.name, cols[c0:c0 + len(part.cols)], p[p0:p0 + len(part.params)], model, pe)
                out = d if out is None else Density.__mul__(out, d)
                c0, p0 = c0 + len(part.cols), p0 + len(part.params)
            return out
        return density(t if isinstance(t, Joint) else t.name, cols, p, self.models[0], pe)

    def theta(self, h):
        th = np.zeros(len(self.slot))
        th[self.slot] = self.term.theta[h]
        return th

    def close(self):
        close = getattr(self.ev, "close", None)
        if close:
            close()


def core_samples(term, points=None):
    """Samples in the support at every hyper-point (of ``points``), and those in it at some but not all.  The samples a term waives
    (``Joint.waived``: conditioned beyond COND_CAP) are in neither."""
    live = np.isfinite(term.logp if points is None else term.logp[list(points)])
    keep = np.ones(live.shape[1], dtype=bool)
    keep[getattr(term, "waived", [])] = False
    return np.flatnonzero(live.all(axis=0) & keep), np.flatnonzero(live.any(axis=0) & ~live.all(axis=0) & keep)


def group_points(term, z, group):
    """Hyper-points of ``plbounds`` (or of a product that carries it as its longest part) in nest ``group`` of intervals: the catalogs
    of summed gradients are built per nest, from the samples inside its narrowest interval."""
    g = z["plbounds/group"]
    assert len(g) == len(term.theta)
    return [int(h) for h in np.flatnonzero(g == group)]


def pins(term):
    """None, or (index of z == zmin, index of z == zmax, whether z <= zmax per sample) where ``term`` is or contains a spline redshift
    model: zmin and zmax of these models are the common range of the two sides' data, so BOTH sides of every catalog carry the two
    end samples, and a sample beyond zmax stays off the injection side."""
    parts = term.parts if isinstance(term, Product) else (term,)
    at = 0
    for t in parts:
        if t.name in Z_SPLINE_TERMS:
            zg, _, _ = _z_table()
            z = term.cols[at]
            return int(np.flatnonzero(z == zg[0])[0]), int(np.flatnonzero(z == zg[-1])[0]), z <= zg[-1]
        at += len(t.cols)
    return None


def plbounds_arranged(z, n, second=False):
    """The first ``n`` samples of an arrangement of ``plbounds`` that leads with the samples inside [20, 30], the narrowest interval of
    nest 0 (a ``Product`` keeps only as many samples as its shortest part has: catalog A needs its core among them).  ``second``:
    another arrangement with the same property, under another name."""
    t = Term(z, "plbounds")
    core, _ = core_samples(t, group_points(t, z, 0))
    rest = [i for i in range(t.n) if i not in set(core)]
    order = (list(np.roll(core, 3)) + list(np.roll(rest, 11))) if second else (list(core) + rest)
    return Subset(t, order[:n], "plbounds:2" if second else "plbounds:1")


def plbounds_product(z, spline_z):
    """powerlaw_redshift x plbounds x plbounds on a second arrangement of the samples (the ahead-of-time chain "plz+plb2")."""
    zt = Term(spline_z, "powerlaw_redshift")
    return Product(zt, plbounds_arranged(z, zt.n), plbounds_arranged(z, zt.n, second=True))


def values_catalog(term, make):
    idx = np.arange(term.n)
    pin = pins(term)
    return Catalog(term, make, idx.reshape(-1, 1), idx if pin is None else idx[pin[2]])


def catalog_a(term, make, points=None):
    """``points``: the hyper-points the catalog will be run at (plbounds: one nest of intervals); every point otherwise."""
    core, _ = core_samples(term, points)
    assert len(core) >= 8, (term.name, len(core))
    pin = pins(term)
    if pin is None:
        return Catalog(term, make, core.reshape(-1, 1), core[:1])
    lo, hi, inside = pin
    assert lo in core and hi in core, (term.name, "an end sample is not live at every hyper-point")
    x0 = [c for c in core if c not in (lo, hi) and inside[c]][0]
    return Catalog(term, make, core.reshape(-1, 1), [lo, x0, hi])  # total_inj = 3


def catalog_b(term, make, points=None):
    core, some = core_samples(term, points)
    pin = pins(term)
    if pin is not None:
        # the two ends lead the events; samples dead at every hyper-point (beyond zmax) ride along with the partly dead ones
        lo, hi, inside = pin
        never = np.flatnonzero(~np.isfinite(term.logp).any(axis=0))
        rest = [c for c in core if c not in (lo, hi)]
        seq, s = [lo, hi], list(some) + list(never)
        for k, c in enumerate(rest):
            seq.append(c)
            if k % 2 == 1 and s:
                seq.append(s.pop(0))
        n_ev = len(seq) // 3
        assert n_ev >= 4 and lo in core and hi in core, (term.name, n_ev)
        ok = [c for c in rest if inside[c]]
        return Catalog(term, make, np.array(seq[: 3 * n_ev]).reshape(n_ev, 3), [lo, ok[1], ok[3], ok[5], hi])
    seq, s = [], list(some)
    if isinstance(term, Joint) and not s:  # a support that no hyper-parameter moves: the samples outside it ride along instead
        s = [int(i) for i in np.flatnonzero(~np.isfinite(term.logp).any(axis=0))]
    for k, c in enumerate(core):
        seq.append(c)
        if k % 2 == 1 and s:
            seq.append(s.pop(0))
    n_ev = len(seq) // 3
    assert n_ev >= 4, (term.name, n_ev)
    inj = [core[0], some[0] if len(some) else core[1], core[3], core[5], core[7]]
    return Catalog(term, make, np.array(seq[: 3 * n_ev]).reshape(n_ev, 3), inj)


def reference(cat, h):
    """(log_l, grad, scale) of the hierarchical likelihood on ``cat`` at hyper-point ``h`` (n_obs = number of events, total_inj = number
    of injections, no cuts), from the fixture in extended precision: sum_e log mean_i p - n_obs log(sum_inj p / total_inj).

    ``scale`` is the largest of the four sums log_l is assembled from (sum_e logsumexp_e, n_obs log n_pe, n_obs logsumexp_inj, n_obs log
    total_inj): the size of the absolute floor at the LOGL_CANCELLED hyper-points, where they cancel; unused elsewhere."""
    L = np.longdouble
    t = cat.term
    def side(idx):  # idx: (..., n) sample indices -> logsumexp (...), weight-averaged derivatives (P, ...)
        lp = t.logp[h][idx].astype(L)
        d = t.dlogp[h][:, idx].astype(L)
        m = np.max(lp, axis=-1, keepdims=True)
        w = np.exp(lp - m)
        s = np.sum(w, axis=-1)
        return np.log(s) + m[..., 0], np.sum(w * d, axis=-1) / s

    lse_pe, g_pe = side(cat.pe_idx)
    lse_inj, g_inj = side(cat.inj_idx)
    n_ev, n_pe = cat.pe_idx.shape
    n_inj = len(cat.inj_idx)
    parts = [np.sum(lse_pe), -n_ev * np.log(L(n_pe)), -n_ev * lse_inj, n_ev * np.log(L(n_inj))]
    grad = np.sum(g_pe, axis=1) - n_ev * g_inj
    return float(sum(parts)), grad.astype(np.float64), float(max(abs(p) for p in parts))


def reference_marginalised(cat, h):
    """``reference`` with the selection function's Monte-Carlo uncertainty marginalised (the reference's analysis.py:270-271): log mu
    becomes log mu - (3 + n_obs) / (2 n_eff) with the reference's n_eff of the injections (analysis.py:128-134), 1 / n_eff = sum w^2 /
    (sum w)^2 - 1 / total_inj, so log_l gains n_obs (3 + n_obs) / 2 times that and the gradient n_obs (3 + n_obs) / 2 times
    2 sum w^2 g / (sum w)^2 - 2 sum w^2 sum w g / (sum w)^3."""
    L = np.longdouble
    t = cat.term
    log_l, grad, scale = reference(cat, h)
    lp = t.logp[h][cat.inj_idx].astype(L)
    g = t.dlogp[h][:, cat.inj_idx].astype(L)
    w = np.exp(lp - np.max(lp))
    s1, s2 = np.sum(w), np.sum(w * w)
    n_ev = cat.pe_idx.shape[0]
    k = L(n_ev * (3 + n_ev)) / 2
    extra = k * (s2 / s1**2 - 1 / L(len(cat.inj_idx)))
    d_extra = k * (2 * np.sum(w * w * g, axis=-1) / s1**2 - 2 * s2 * np.sum(w * g, axis=-1) / s1**3)
    return float(L(log_l) + extra), (grad.astype(L) + d_extra).astype(np.float64), max(scale, float(abs(extra)))


def is_cancelled(term, h, cat=None):
    """Whether hyper-point ``h`` is one of LOGL_CANCELLED (or, on a catalog of one sample per event and one injection -- catalog A -- of
    LOGL_CANCELLED_A); a product's is where every part's is (a flat density times a flat one)."""
    if isinstance(term, (Product, Joint)):
        return all(is_cancelled(t, int(hs[h]), cat) for t, hs in zip(term.parts, term.part_points))
    if isinstance(term, Subset):
        return is_cancelled(term.base_term, h, cat)
    if isinstance(term, Shared):  # a flat density times itself
        return is_cancelled(term.base, h, cat)
    only_a = cat is not None and cat.pe_idx.shape[1] == 1 and len(cat.inj_idx) == 1
    return term.tags[h] in LOGL_CANCELLED.get(term.name, ()) or (only_a and term.tags[h] in LOGL_CANCELLED_A.get(term.name, ()))


def marginalised_points(term):
    """Every hyper-point but the flat ones: with equal weights on all ``total_inj`` injections the reference's Monte-Carlo variance
    (analysis.py:128) is exactly 0, its n_eff infinite and the derivative of its own expression 0 / 0."""
    flat = LOGL_CANCELLED.get(base_name(term), ())
    return [h for h, tag in enumerate(term.tags) if tag not in flat]


class Worst:
    """Largest error seen per (term, path, what), for assertion messages and profiles/near_singular/RESULTS.md."""

    def __init__(self):
        self.rows = {}

    def note(self, key, err, where):
        if not (err <= self.rows.get(key, (-1.0, ""))[0]):
            self.rows[key] = (float(err), where)

    def lines(self):
        return [f"{' / '.join(k)}: {e:.3e} at {w}" for k, (e, w) in sorted(self.rows.items())]


def check_values(cat, path, worst, failures, eps_lm=None):
    """``eps_lm`` (terms with a ``cond`` array): the bar at sample i is VALUE_ATOL + |cond_i| eps_lm; a sample whose conditioning term
    exceeds COND_CAP is compared for liveness only.  The error is noted in units of the bar times VALUE_ATOL."""
    t = cat.term
    for h in range(len(t.theta)):
        got = cat.ev.log_weights(cat.theta(h))[:, 0]
        ref = t.logp[h]
        dead = np.isneginf(ref)
        # (the liveness of a WAIVED sample is ``check_waived_liveness``'s, a test of its own: a miss there must not hide the rest)
        told = np.ones(len(ref), dtype=bool) if eps_lm is None else ~(np.abs(t.cond[h]) * eps_lm > COND_CAP)
        if not np.array_equal(np.isneginf(got)[told], dead[told]):
            failures.append(f"{t.name} [{path}] {t.tags[h]}: support differs at samples {np.flatnonzero((np.isneginf(got) != dead) & told)[:6].tolist()}")
            continue
        keep = ~dead
        scale = np.ones(len(ref))
        if eps_lm is not None:
            extra = np.abs(t.cond[h]) * eps_lm
            keep &= told
        if not keep.any():  # (a product whose parts have no common live sample at this point: the support was all there is to compare)
            continue
        if eps_lm is not None:
            scale = 1.0 + extra / VALUE_ATOL
            raw = np.abs(got[keep] - ref[keep])
            worst.note((t.name, path, "value, unscaled"), raw.max(), f"{t.tags[h]} sample {np.flatnonzero(keep)[int(np.argmax(raw))]}")
        err = np.abs(got[keep] - ref[keep]) / scale[keep]
        k = int(np.argmax(err))
        worst.note((t.name, path, "value"), err[k], f"{t.tags[h]} theta={t.theta[h].tolist()} sample {np.flatnonzero(keep)[k]}")
        if not err[k] < VALUE_ATOL:
            failures.append(f"{t.name} [{path}] {t.tags[h]}: |log w - ref| = {err[k]:.3e} x its bar / {VALUE_ATOL:g} >= {VALUE_ATOL:g} (sample {np.flatnonzero(keep)[k]})")


def check_waived_liveness(cat, failures):
    """A sample conditioned beyond COND_CAP tells nothing about the arithmetic, but it is finite or -inf as the fixture has it."""
    t = cat.term
    for h in range(len(t.theta)):
        got = cat.ev.log_weights(cat.theta(h))[:, 0]
        for i in t.waived:
            if np.isneginf(got[i]) != np.isneginf(t.logp[h][i]):
                failures.append(f"{t.name} {t.tags[h]}: sample {i} ({[c[i] for c in t.cols]}) is {'dead' if np.isneginf(got[i]) else 'alive'}, the fixture has {t.logp[h][i]!r}")


def _conditioning(cat, h, eps_lm):
    """First-order bound on what an error of ``eps_lm`` in the rounded input of every sample does to log_l and to every gradient
    component on ``cat``: per event (and, n_obs times, for the injections), with normalised weights w_i, conditioning c_i = |d log p_i /
    d log m1| and c2_ij the same for derivative j:  log_l moves by at most eps sum_i w_i c_i, the weight-averaged derivative j by at
    most eps sum_i w_i (|g_ij - mean_j| c_i + c2_ij)."""
    t = cat.term

    def side(idx):
        lp, g = t.logp[h][idx], t.dlogp[h][:, idx]
        c, c2 = np.abs(t.cond[h][idx]), np.abs(t.cond2[h][:, idx])
        w = np.exp(lp - np.max(lp, axis=-1, keepdims=True))
        w = w / np.sum(w, axis=-1, keepdims=True)
        mean = np.sum(w * g, axis=-1, keepdims=True)
        return eps_lm * np.sum(w * c, axis=-1), eps_lm * np.sum(w * (np.abs(g - mean) * c + c2), axis=-1)

    (l_pe, g_pe), (l_inj, g_inj) = side(cat.pe_idx), side(cat.inj_idx)
    n_ev = cat.pe_idx.shape[0]
    return float(np.sum(l_pe) + n_ev * l_inj), np.sum(g_pe, axis=-1) + n_ev * g_inj


def grad_errors(t, got_grad, ref_grad):
    """Per-component error in units of the bar: |got_j - ref_j| / max(1, |ref_j|)."""
    return np.abs(got_grad - ref_grad) / np.maximum(1.0, np.abs(ref_grad))


def check_gradients(cat, path, worst, failures, points=None, results=None, marginalised=False, eps_lm=None):
    """``marginalised``: against ``reference_marginalised``, the evaluator called with ``marginalize_selection=True``.  ``eps_lm`` (terms
    with a ``cond`` array): the bars gain what ``_conditioning`` allows a rounded input; the errors are then noted in units of the
    widened bar, i.e. divided by (size + allowance / RTOL)."""
    t = cat.term
    total = float(len(cat.inj_idx))
    for h in (range(len(t.theta)) if points is None else points):
        if results is not None:
            log_l, grad = results[h]
        else:
            log_l, grad = cat.ev.evaluate(cat.theta(h), total, marginalize_selection=True) if marginalised else cat.ev.evaluate(cat.theta(h), total)
        grad = np.asarray(grad)[cat.slot]
        ref_l, ref_g, scale_l = (reference_marginalised if marginalised else reference)(cat, h)
        cancelled = is_cancelled(t, h, cat)
        extra_l, extra_g = _conditioning(cat, h, eps_lm) if eps_lm is not None else (0.0, 0.0)
        e_l = 0.0 if log_l == ref_l else abs(log_l - ref_l) / ((max(scale_l, abs(ref_l), 1.0 if base_name(t) in SPLINE_TERMS else 0.0) if cancelled else (abs(ref_l) or 1e-300)) + extra_l / LOGL_RTOL)
        worst.note((t.name, path, "log_l (relative)"), e_l, t.tags[h])
        if not e_l < LOGL_RTOL:
            failures.append(f"{t.name} [{path}] {t.tags[h]}: log_l {log_l!r} vs {ref_l!r}: relative {e_l:.3e} >= {LOGL_RTOL:g}{' (of the cancelled sums)' if cancelled else ''}")
        e = np.abs(grad - ref_g) / (np.maximum(1.0, np.abs(ref_g)) + extra_g / GRAD_RTOL)
        for j, name in enumerate(t.params):
            worst.note((t.name, path, f"d/d{name}"), e[j], f"{t.tags[h]} theta={t.theta[h].tolist()} ref={ref_g[j]:.6g}")
            if not e[j] <= GRAD_RTOL:
                failures.append(f"{t.name} [{path}] {t.tags[h]}: d/d{name} = {grad[j]!r} vs {ref_g[j]!r}: error {e[j]:.3e} of max(1, |ref|) > {GRAD_RTOL:g}")


def report(failures, worst):
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:40]) + "\nworst errors:\n  " + "\n  ".join(worst.lines())
