"""GPU: the mock-catalog kernels (gwinferno_amd/csrc/gwi_mock.h) against their NumPy statement and the 40-digit fixture, their
determinism across calls, shards and the launch cut, the evidence and selection identities on the device backend, and a catalog
through the engine end to end.  Tolerances: tests/mock_util.py (8 x the host statement's measured error, floor 1e-12 sigma)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mock_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
pytest.importorskip("scipy")


@pytest.fixture(scope="module")
def MC():
    from gwinferno_amd import mock_catalog

    return mock_catalog


def test_device_against_the_fixture(MC):
    """The fixture's regimes on the device.  The kernels draw their uniforms themselves, so the fixture's (d, u) pairs cannot be fed
    to them: every datum of the fixture gets 65 samples from the device's own stream, and device and statement -- which the CPU file
    holds to the fixture at the fixture's uniforms -- are compared under the regime's tolerance (8 x the statement's measured error
    against the fixture, floor 1e-12 sigma); the prior as prior x sample to 1e-13."""
    f = U.fixture()
    for tr, regime, m in U.fixture_groups(f):
        tol_s, tol_d = U.device_tolerance(U.HOST_MEASURED, (tr, regime)), U.device_tolerance(U.HOST_MEASURED_DATA, (tr, regime))
        for sigma in np.unique(f["sigma"][m]):
            k = m & (f["sigma"] == sigma)
            model = U.one_coordinate_model(MC, tr, float(f["lo"][k][0]), float(f["hi"][k][0]), float(sigma))
            data = np.ascontiguousarray(f["d"][k][None, :])
            dev, host = (MC.posterior_samples(data, model, 65, 17, backend=b) for b in ("device", "host"))
            T = np.log if tr == "log" else (lambda v: v)
            e_s = float(np.max(np.abs(T(dev["x"]) - T(host["x"])) / sigma))
            sx = (dev["x"], host["x"]) if tr == "log" else (1.0, 1.0)  # (prior * x: the sample's own deviation is held above)
            e_p = float(np.max(np.abs(dev["prior"] * sx[0] / (host["prior"] * sx[1]) - 1.0)))
            print(tr, regime, sigma, f"sample {e_s:.3g} sigma (tolerance {tol_s:.3g}), prior {e_p:.3g}")
            assert e_s <= tol_s and e_p <= U.PRIOR_RTOL
            assert np.all((dev["x"] >= model.lo[0]) & (dev["x"] <= model.hi[0]))
            assert np.allclose(dev["prior"], MC.pe_prior(dev, model), rtol=U.PRIOR_RTOL, atol=0.0)


@pytest.mark.parametrize("n_coords", [1, 3, 7])
@pytest.mark.parametrize("n_ev,n_pe", [(1, 1), (3, 65), (3, 257)])
def test_posterior_kernel_against_the_statement(MC, n_coords, n_ev, n_pe):
    model = U.coords_model(MC, n_coords)
    t_lo, t_hi, _ = model.t_bounds()
    rng = np.random.default_rng(n_coords * 100 + n_pe)
    data = np.ascontiguousarray(t_lo[:, None] + (t_hi - t_lo)[:, None] * rng.uniform(-0.3, 1.3, (n_coords, n_ev)))
    if n_ev > 1:
        data[0, 1] = np.nan
    dev, host = (MC.posterior_samples(data, model, n_pe, 31, first_event=2**33, backend=b) for b in ("device", "host"))
    tol = U.device_tolerance(U.HOST_MEASURED, ("log", "beyond_lo"))  # ordinary sigmas, data up to 0.3 ranges outside: the 1e-12 floor
    for c, k in enumerate(model.names):
        T = np.log if model.is_log[c] else (lambda v: v)
        ok = ~np.isnan(host[k])
        assert np.array_equal(np.isnan(dev[k]), ~ok)
        assert np.all(np.abs(T(dev[k][ok]) - T(host[k][ok])) <= tol * model.sigmas[c])
        assert np.all((dev[k][ok] >= model.lo[c]) & (dev[k][ok] <= model.hi[c]))
    ok = ~np.isnan(host["prior"])
    assert np.array_equal(np.isnan(dev["prior"]), ~ok) and (n_ev == 1 or np.all(~ok[1]))
    assert np.allclose(dev["prior"][ok], MC.pe_prior(dev, model)[ok], rtol=U.PRIOR_RTOL, atol=0.0)


@pytest.mark.parametrize("n_coords", [3, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_observe_kernel_against_the_statement(MC, n_coords, n):
    """Data within the tolerance; snr to 1e-9 relative (rho's log-derivatives with respect to the data are at most 1 / z_d <= 1e3 for
    the z_d > 1e-3 that can be found, times data that agree to 1e-12 sigma); found byte for byte (the CPU file has confirmed the
    margin to the threshold); NaN inputs give NaN data, NaN snr and found = 0."""
    model = U.coords_model(MC, n_coords)
    x = U.true_sources(model, n, 100 + n, with_nan=True)
    dev, host = (MC.observe(x, model, 7, backend=b) for b in ("device", "host"))
    tol = U.device_tolerance(U.HOST_MEASURED_DATA, ("log", "inside"))
    ok = ~np.isnan(host[0])
    assert np.array_equal(np.isnan(dev[0]), ~ok)
    assert np.all(np.abs(dev[0] - host[0])[ok] <= tol * np.broadcast_to(model.sigmas[:, None], ok.shape)[ok])
    ok = ~np.isnan(host[1])
    assert np.array_equal(np.isnan(dev[1]), ~ok) and np.allclose(dev[1][ok], host[1][ok], rtol=1e-9, atol=0.0)
    assert np.array_equal(dev[2], host[2]) and not np.any(dev[2][~ok])


def test_refusals_reach_python_with_their_messages(MC):
    from gwinferno_amd import _native

    model = MC.default_model()
    model.sigmas[1] = -1.0
    with pytest.raises(_native.NativeEngineError, match="coordinate 1: sigma <= 0 or not finite"):
        MC.posterior_samples(np.zeros((3, 2)), model, 4, 1)
    model = MC.ObservationModel(["mass_1"], ["log"], [0.1], [2.0], [100.0])
    with pytest.raises(_native.NativeEngineError, match="role index m1 = 0 out of range|role index q = -1 out of range"):
        MC.observe(np.ones((1, 2)), model, 1)


def test_determinism_shards_and_the_launch_cut(MC):
    model3, model1 = U.coords_model(MC, 3), U.coords_model(MC, 1)
    x = U.true_sources(model3, 1000, 5, with_nan=True)
    a, b = MC.observe(x, model3, 9), MC.observe(x, model3, 9)
    lo, hi = MC.observe(x[:, :500], model3, 9), MC.observe(np.ascontiguousarray(x[:, 500:]), model3, 9, first_index=500)
    for k in range(3):
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=-1), equal_nan=True)
    # n_pe = 2^20 + 1000 at C = 1: the cut into launches of 2^20 lanes is crossed
    n_pe = 2**20 + 1000
    data = np.array([[np.log(30.0), np.log(1.5)]])
    whole = MC.posterior_samples(data, model1, n_pe, 3)
    again = MC.posterior_samples(data, model1, n_pe, 3)
    second = MC.posterior_samples(data[:, 1:], model1, n_pe, 3, first_event=1)
    assert MC.last_device_times()[2] == 2
    host_tail = MC.posterior_samples(data, model1, n_pe, 3, backend="host")["mass_1"][:, -1500:]
    for k in whole:
        assert np.array_equal(whole[k], again[k]) and np.array_equal(whole[k][1:], second[k])
    assert np.all(np.abs(np.log(whole["mass_1"][:, -1500:]) - np.log(host_tail)) <= U.FLOOR * model1.sigmas[0])


@pytest.mark.parametrize("d", U.EVIDENCE_DATA)
def test_evidence_identity(MC, d):
    mean, se, exact = U.evidence_identity(MC, d, seed=5, backend="device")
    print(f"d = {d:.4f}: importance average {mean:.6f} +- {se:.2g}, integrals {exact:.6f}")
    assert abs(mean - exact) <= 5.0 * se


def test_selection_identity(MC):
    """The found fraction of 2e5 observed sources against `detection_efficiency` of the engine at theta_true on 4e5 mock injections;
    var_IS from the engine's own variance site."""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.likelihood import detection_efficiency

    f, var_f, n_found = U.direct_found_fraction(MC, 200_000, 11, "device")
    inj, total = U.mock_injections(MC, 400_000, 12, "device")
    model = U.catalog_model(MC)
    pe = MC.posterior_samples(np.array([[np.log(30.0)], [0.8], [0.3]]), model, 8, 1)
    # the redshift model normalises on [max of the minima, min of the maxima] of the PE and injection redshifts: pin that grid to the
    # population's support [1e-3, 1.9] with two PE samples and two injections of zero weight (prior 1e300) at its ends
    pe["redshift"][0, :2] = (1e-3, 1.9)
    ends = {"mass_1": [30.0, 30.0], "mass_ratio": [0.8, 0.8], "redshift": [1e-3, 1.9], "prior": [1e300, 1e300]}
    inj = {k: np.concatenate([inj[k], ends[k]]) for k in ends}
    comp = COMPOSITIONS["plpeak"](pe, inj, mmin=U.MMIN, mmax=U.MMAX)
    p = {k: U.THETA[k] for k in comp.PARAMS}
    logmu, log_neff, var_log = detection_efficiency(comp.weights(p, False), total)
    mu, var_mu, n_eff = float(np.exp(logmu)), float(var_log * np.exp(2 * logmu)), float(np.exp(log_neff))
    print(f"direct {f:.5f} +- {var_f**0.5:.2g} ({n_found} found); engine {mu:.5f} +- {var_mu**0.5:.2g} (n_eff {n_eff:.0f})")
    assert n_eff >= 4 * n_found / 50
    assert abs(f - mu) <= 5.0 * np.sqrt(var_f + var_mu)


def test_end_to_end_through_the_engine(MC):
    from gwinferno_amd import likelihood as L
    from gwinferno_amd.compositions import COMPOSITIONS

    model = U.catalog_model(MC)
    args = (U.population(MC, on_host=False), U.injection_tables(model), model, 8, 256, 20_000, 3)
    pe, inj, total, truth = MC.make_mock_catalog(*args)
    pe2, inj2, total2, _ = MC.make_mock_catalog(*args)
    assert total == total2 == 20_000 and all(np.array_equal(pe[k], pe2[k]) for k in pe) and all(np.array_equal(inj[k], inj2[k]) for k in inj)
    comp = COMPOSITIONS["plpeak"](pe, {k: v for k, v in inj.items() if k != "snr"}, mmin=U.MMIN, mmax=U.MMAX)
    p = {k: U.THETA[k] for k in comp.PARAMS}
    L.hierarchical_likelihood(comp.weights(p, True), comp.weights(p, False), total, 8, 1.0, surveyed_hypervolume=comp.hypervolume(p), min_neff_cut=False)
    s = L.last_sites()
    print(f"log_l {float(s['log_l']):.4f}, min n_eff {float(np.exp(np.min(s['log_nEffs']))):.1f}, n_eff_inj {float(np.exp(s['log_nEff_inj'])):.1f}")
    assert np.isfinite(s["log_l"]) and np.all(np.isfinite(s["grad_log_likelihood"]))
    assert np.all(np.exp(s["log_nEffs"]) > 8) and np.exp(s["log_nEff_inj"]) >= 4 * 8
