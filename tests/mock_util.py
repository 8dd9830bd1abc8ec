"""Shared by tests/test_mock_catalog_cpu.py and tests/test_gpu_mock_catalog.py: the fixture's tolerances, the test inputs, the
population curves in NumPy and the two identities."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "mock_hp.npz")

# Worst |T(x) - T(x_40)| / sigma of the HOST statement (scipy's erfc / erfcinv) against tests/golden/mock_hp.npz, per transform and
# regime, as measured by tests/test_mock_catalog_cpu.py::test_host_statement_against_the_fixture (which asserts that they still
# hold); x is the float64 sample in natural units, so the figure includes the rounding of x itself (one ulp of 100 is 3.6e-11 sigma
# in the narrow log regime).  "data" is the same for d = T(x_true) + sigma n.  The device is held to 8 x these, floor 1e-12.
HOST_MEASURED = {
    ("identity", "inside"): 1.2e-15, ("identity", "beyond_lo"): 4.6e-15, ("identity", "beyond_hi"): 3.6e-15, ("identity", "narrow"): 0.0,
    ("identity", "wide"): 3.2e-15, ("identity", "u_edge"): 2.5e-15,
    ("log", "inside"): 2.3e-15, ("log", "beyond_lo"): 4.0e-15, ("log", "beyond_hi"): 2.3e-15, ("log", "narrow"): 2.3e-10, ("log", "wide"): 3.3e-15,
    ("log", "u_edge"): 5.7e-11,
}
HOST_MEASURED_DATA = {
    ("identity", "inside"): 1.2e-15, ("identity", "beyond_lo"): 2.4e-15, ("identity", "beyond_hi"): 1.2e-15, ("identity", "narrow"): 0.0,
    ("identity", "wide"): 9.0e-16, ("identity", "u_edge"): 3.6e-15,
    ("log", "inside"): 2.3e-15, ("log", "beyond_lo"): 2.3e-15, ("log", "beyond_hi"): 2.3e-15, ("log", "narrow"): 2.3e-10, ("log", "wide"): 8.8e-16,
    ("log", "u_edge"): 2.3e-10,
}
DEVICE_FACTOR, FLOOR = 8.0, 1e-12
PRIOR_RTOL = 1e-13


def device_tolerance(table, key):
    return max(DEVICE_FACTOR * table[key], FLOOR)


def fixture():
    return dict(np.load(FIXTURE))


def fixture_groups(f):
    """``(transform, regime, mask)`` of every group of the fixture."""
    for tr in ("identity", "log"):
        for regime in np.unique(f["regime"]):
            yield tr, str(regime), (f["is_log"] == (tr == "log")) & (f["regime"] == regime)


def one_coordinate_model(MC, tr, lo, hi, sigma):
    return MC.ObservationModel(["x"], [tr], [sigma], [lo], [hi])


def fixture_errors(MC, f, sample_fn, data_fn):
    """Per group: the worst sample error, data error (both in sigma) and prior relative error of ``sample_fn(model, d, u) -> (x,
    prior)`` and ``data_fn(model, x_true, u) -> d`` -- one-coordinate problems evaluated at the fixture's own uniforms."""
    out = {}
    for tr, regime, m in fixture_groups(f):
        e_s = e_d = e_p = 0.0
        for sigma in np.unique(f["sigma"][m]):
            k = m & (f["sigma"] == sigma)
            model = one_coordinate_model(MC, tr, float(f["lo"][k][0]), float(f["hi"][k][0]), float(sigma))
            x, prior = sample_fn(model, f["d"][k], f["u"][k])
            d = data_fn(model, f["x_true"][k], f["u"][k])
            T = np.log if tr == "log" else (lambda v: v)
            e_s = max(e_s, float(np.max(np.abs(T(x) - T(f["x"][k])) / sigma)))
            e_d = max(e_d, float(np.max(np.abs(d - f["data"][k]) / sigma)))
            # the prior is a function of the sample: a log coordinate's 1 / (x ln(hi / lo)) is compared as prior * x, so that the sample's
            # own deviation (held above, in sigma) does not count against the prior's arithmetic
            sx, s40 = (x, f["x"][k]) if tr == "log" else (1.0, 1.0)
            e_p = max(e_p, float(np.max(np.abs(prior * sx / (f["prior"][k] * s40) - 1.0))))
            assert np.all((x >= f["lo"][k]) & (x <= f["hi"][k]))
        out[(tr, regime)] = (e_s, e_d, e_p)
    return out


# ---- multi-coordinate inputs ------------------------------------------------------------------------------------------------
def coords_model(MC, n_coords):
    """C = 1: log m1 alone (no detection roles); C = 3: m1, q, z; C = 7: with spins."""
    if n_coords == 1:
        return MC.ObservationModel(["mass_1"], ["log"], [0.08], [2.0], [100.0])
    return MC.default_model(spins=n_coords == 7)


def true_sources(model, n, seed, with_nan=False):
    """``(C, n)`` true parameters inside the supports (redshift >= 0.01: rho's sensitivity to z_d is 1 / z_d)."""
    rng = np.random.default_rng(seed)
    x = model.lo[:, None] + (model.hi - model.lo)[:, None] * rng.uniform(0.02, 0.98, (model.n_coords, n))
    if "mass_1" in model.names:
        i = model.names.index("mass_1")
        x[i] = np.exp(rng.uniform(np.log(5.0), np.log(90.0), n))
    if "redshift" in model.names:
        i = model.names.index("redshift")
        x[i] = rng.uniform(0.05, 1.5, n)
    if with_nan and n > 2:
        x[0, 1] = np.nan
        x[-1, n // 2] = np.nan
    return np.ascontiguousarray(x)


# ---- the population of the selection and end-to-end tests ---------------------------------------------------------------------
THETA = dict(alpha=-2.5, beta=1.0, mpp=35.0, sigpp=4.0, lam=0.08, lamb=2.0)
MMIN, MMAX = 5.0, 100.0
DETECTION = dict(rho_ref=8.0, mc_ref=25.0, dl_ref=4000.0, rho_th=8.0)


def numpy_mass_curves():
    """The PL+Peak curve and the q^beta table on ``population_draws``' grids, from the NumPy oracle (no device needed)."""
    from oracle import numpy_oracle as O

    ms, qs = np.linspace(MMIN, MMAX, 800), np.linspace(MMIN / MMAX, 1, 800)
    return ms, O.plpeak_primary_pdf(ms, THETA["alpha"], MMIN, MMAX, THETA["mpp"], THETA["sigpp"], THETA["lam"]), qs, qs ** THETA["beta"]


def population(MC, on_host=True):
    return MC.plpeak_population(mmin=MMIN, mmax=MMAX, mass_curves=numpy_mass_curves() if on_host else None, **THETA)


def catalog_model(MC):
    return MC.default_model(**DETECTION)


def injection_tables(model):
    """Broad piecewise-linear tables on the model's supports: m1^-1.8, q flat above 0.05 rising from the support's end, z^1.5 (1 + z)."""
    g = {k: np.linspace(model.lo[c], model.hi[c], 800) for c, k in enumerate(model.names)}
    pdf = {"mass_1": g["mass_1"] ** -1.8, "mass_ratio": np.minimum(1.0, 0.05 + g["mass_ratio"] / 0.1), "redshift": g["redshift"] ** 1.5 * (1 + g["redshift"])}
    return {k: (float(model.lo[c]), float(model.hi[c]), pdf[k]) for c, k in enumerate(model.names)}


def population_density(x):
    """The normalised PL+Peak x PL q x PL z density at ``x (3, n)`` (NumPy oracle forms; the z factor normalised on the curve's grid)."""
    from oracle import numpy_oracle as O

    from gwinferno_amd.cosmology import planck15_lvk

    m1, q, z = x
    zs = np.linspace(1e-3, 1.9, 1000)
    pz = lambda v: planck15_lvk().dVc_dz(v) * (1.0 + v) ** (THETA["lamb"] - 1.0)  # noqa: E731
    with np.errstate(all="ignore"):
        p = O.plpeak_primary_ratio_pdf(m1, q, THETA["alpha"], THETA["beta"], MMIN, MMAX, THETA["mpp"], THETA["sigpp"], THETA["lam"]) * pz(z) / np.trapezoid(pz(zs), zs)
    return np.where(np.isfinite(p) & (z >= 1e-3) & (z <= 1.9), p, 0.0)


def direct_found_fraction(MC, n, seed, backend):
    """Found fraction of ``n`` sources drawn from the population and observed, and its binomial variance."""
    pop, model = population(MC), catalog_model(MC)
    x, _ = MC.draw_true_sources(pop, model.names, n, seed, 0, backend=backend)
    _, _, found = MC.observe(x, model, MC.sub_seed(seed, 2), backend=backend)
    f = float(found.mean())
    return f, f * (1.0 - f) / n, int(found.sum())


def mock_injections(MC, n_generated, seed, backend):
    from gwinferno_amd.population_draws import table_draws

    model = catalog_model(MC)
    tabs = injection_tables(model)
    x, dens = np.empty((3, n_generated)), np.ones(n_generated)
    for c, name in enumerate(model.names):
        lo, hi, pdf = tabs[name]
        x[c] = table_draws(lo, hi, pdf, n_generated, MC.sub_seed(seed, 32 + c), backend=backend)[0]
        dens = dens * MC.table_density(lo, hi, pdf, x[c])
    return MC.found_injections(x, dens, model, MC.sub_seed(seed, 4), backend=backend)


def importance_efficiency(inj, total):
    """``(mu, var_mu, n_eff)`` of the detection efficiency in NumPy (analysis.py:91-136)."""
    w = population_density(np.stack([inj["mass_1"], inj["mass_ratio"], inj["redshift"]])) / inj["prior"]
    mu = np.sum(w) / total
    var = np.sum(w * w) / total**2 - mu * mu / total
    return float(mu), float(var), float(mu * mu / var)


# ---- the evidence identity ------------------------------------------------------------------------------------------------------
EVIDENCE_LO, EVIDENCE_HI, EVIDENCE_SIGMA, EVIDENCE_ALPHA, EVIDENCE_NPE = 5.0, 80.0, 0.25, -2.3, 65536
EVIDENCE_DATA = (np.log(12.0), np.log(70.0), np.log(80.0) + 0.3)  # the last one lies outside the support


def evidence_identity(MC, d, seed, backend):
    """One event, one coordinate (log m1), a power-law population on [lo, hi]: the importance average of p_pop / prior over the
    posterior samples, its standard error, and int L p_pop / int L pi by trapezoid on 20 001 points."""
    model = MC.ObservationModel(["mass_1"], ["log"], [EVIDENCE_SIGMA], [EVIDENCE_LO], [EVIDENCE_HI])
    a1 = EVIDENCE_ALPHA + 1.0
    p_pop = lambda x: a1 * x**EVIDENCE_ALPHA / (EVIDENCE_HI**a1 - EVIDENCE_LO**a1)  # noqa: E731
    pe = MC.posterior_samples(np.array([[d]]), model, EVIDENCE_NPE, seed, backend=backend)
    x, prior = pe["mass_1"][0], pe["prior"][0]
    assert np.allclose(prior, MC.pe_prior(x[None, :], model), rtol=1e-13)
    w = p_pop(x) / prior
    grid = np.linspace(EVIDENCE_LO, EVIDENCE_HI, 20001)
    like = np.exp(-0.5 * ((np.log(grid) - d) / EVIDENCE_SIGMA) ** 2)
    pi = 1.0 / (grid * np.log(EVIDENCE_HI / EVIDENCE_LO))
    exact = np.trapezoid(like * p_pop(grid), grid) / np.trapezoid(like * pi, grid)
    return float(np.mean(w)), float(np.std(w, ddof=1) / np.sqrt(w.size)), float(exact)
