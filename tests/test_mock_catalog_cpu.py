"""CPU: the mock-catalog generator's NumPy statement (gwinferno_amd/mock_catalog.py, backend="host") against the 40-digit fixture
tests/golden/mock_hp.npz, its determinism, the refusals of the Python layer and of the C entries (made on the host before any
device is looked for), and the two identities the observation model must satisfy: the evidence identity of one coordinate and the
selection identity.  The GPU twin is tests/test_gpu_mock_catalog.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mock_util as U  # noqa: E402

pytest.importorskip("scipy")


@pytest.fixture(scope="module")
def MC():
    from gwinferno_amd import mock_catalog

    return mock_catalog


def test_fixture_regenerates_bit_for_bit():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_mock_hp

    new, old = make_mock_hp.generate(verify=True), U.fixture()
    assert set(new) == set(old)
    for k in new:
        assert np.array_equal(new[k], old[k]), k


def host_sample(MC):
    def fn(model, d, u):  # the statement at the fixture's own uniforms
        t_lo, t_hi, _ = model.t_bounds()
        y = MC.truncnorm_icdf((t_lo[0] - d) / model.sigmas[0], (t_hi[0] - d) / model.sigmas[0], u)
        t = np.minimum(np.maximum(d + model.sigmas[0] * y, t_lo[0]), t_hi[0])
        x = np.minimum(np.maximum(np.exp(t) if model.is_log[0] else t, model.lo[0]), model.hi[0])
        return x, MC.pe_prior(x[None, :], model)

    def data(model, x_true, u):
        return (np.log(x_true) if model.is_log[0] else x_true) + model.sigmas[0] * MC.normal_from_uniform(u)

    return fn, data


def test_host_statement_against_the_fixture(MC):
    """The figures quoted in mock_util.HOST_MEASURED (and profiles/mock_catalog/RESULTS.md) still hold; prior: 1e-13 relative."""
    errs = U.fixture_errors(MC, U.fixture(), *host_sample(MC))
    for key, (e_s, e_d, e_p) in errs.items():
        print(key, f"sample {e_s:.3g} sigma, data {e_d:.3g} sigma, prior {e_p:.3g}")
        assert e_s <= 1.5 * U.HOST_MEASURED[key] + 1e-15, (key, e_s)
        assert e_d <= 1.5 * U.HOST_MEASURED_DATA[key] + 1e-15, (key, e_d)
        assert e_p <= U.PRIOR_RTOL, (key, e_p)


def test_counters_and_tags(MC):
    """One Philox block serves two coordinates; the tags are disjoint from the other entries'."""
    from gwinferno_amd.spin_priors import _uniform53, philox4x32_10

    u = MC.coordinate_uniforms(5, np.array([2**33 + 7], dtype=np.uint64), 3, MC.TAG_POSTERIOR, 7)
    for b in range(4):
        w = philox4x32_10(np.array([7]), np.array([2]), np.array([3]), np.array([MC.TAG_POSTERIOR + b]), 5, 0)
        assert u[2 * b, 0] == _uniform53(w[0], w[1])[0]
        if 2 * b + 1 < 7:
            assert u[2 * b + 1, 0] == _uniform53(w[2], w[3])[0]
    tags = {MC.TAG_OBSERVE + b for b in range(4)} | {MC.TAG_POSTERIOR + b for b in range(4)}
    assert len(tags) == 8 and not tags & {0x504F5044, 0x52534D50} and min(tags) >= 2**17


@pytest.mark.parametrize("n_coords", [1, 3, 7])
def test_determinism_and_splits(MC, n_coords):
    model = U.coords_model(MC, n_coords)
    rng = np.random.default_rng(1)
    t_lo, t_hi, _ = model.t_bounds()
    data = np.ascontiguousarray(t_lo[:, None] + (t_hi - t_lo)[:, None] * rng.uniform(-0.2, 1.2, (n_coords, 6)))
    a = MC.posterior_samples(data, model, 65, 9, backend="host")
    b = MC.posterior_samples(data, model, 65, 9, backend="host")
    lo, hi = MC.posterior_samples(data[:, :3], model, 65, 9, backend="host"), MC.posterior_samples(data[:, 3:], model, 65, 9, first_event=3, backend="host")
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], np.concatenate([lo[k], hi[k]]))
    for c, k in enumerate(model.names):
        assert np.all((a[k] >= model.lo[c]) & (a[k] <= model.hi[c]))
    assert np.allclose(a["prior"], MC.pe_prior(a, model), rtol=1e-15)
    if n_coords >= 3:
        x = U.true_sources(model, 100, 3, with_nan=True)
        d, snr, found = MC.observe(x, model, 4, backend="host")
        d2, snr2, found2 = MC.observe(x[:, 50:], model, 4, first_index=50, backend="host")
        assert np.array_equal(d[:, 50:], d2, equal_nan=True) and np.array_equal(snr[50:], snr2, equal_nan=True) and np.array_equal(found[50:], found2)
        assert np.isnan(d[0, 1]) and not found[1] and np.isnan(snr[1]) and not found[50]
        pe = MC.posterior_samples(d[:, :3], model, 4, 1, backend="host")
        assert np.all(np.isnan(pe["prior"][1])) and np.all(np.isfinite(pe["prior"][0]))


def test_gpu_found_inputs_stay_clear_of_the_threshold(MC):
    """The inputs on which tests/test_gpu_mock_catalog.py compares `found` byte for byte keep every rho further than 1e-9 rho_th from
    the threshold, by the statement alone."""
    for n_coords in (3, 7):
        model = U.coords_model(MC, n_coords)
        for n in (1, 63, 64, 65, 1000):
            _, snr, found = MC.observe(U.true_sources(model, n, 100 + n, with_nan=True), model, 7, backend="host")
            assert np.nanmin(np.abs(snr / model.rho_th - 1.0)) > 1e-7
            assert n < 1000 or 0 < found.sum() < n


REFUSALS = [
    (dict(names=list("abcdefghi"), transforms=["identity"] * 9, sigmas=[1.0] * 9, lo=[0.0] * 9, hi=[1.0] * 9), "n_coords = 9 outside 1 ... 8"),
    (dict(sigmas=[0.1, 0.0, 0.1]), "coordinate 1: sigma <= 0 or not finite"),
    (dict(sigmas=[0.1, 0.1, np.inf]), "coordinate 2: sigma <= 0 or not finite"),
    (dict(hi=[100.0, 0.02, 1.9]), "coordinate 1: hi <= lo"),
    (dict(lo=[0.0, 0.05, 1e-3]), "coordinate 0: a log coordinate needs lo > 0"),
    (dict(roles=("mass_1", "mass_ratio", "nope")), "role index z = -1 out of range"),
    (dict(roles=("mass_1", "mass_1", "redshift")), "the role indices m1, q, z must differ"),
    (dict(rho_th=0.0), "detection parameter 3"),
]


def refused_model(MC, change):
    base = dict(names=["mass_1", "mass_ratio", "redshift"], transforms=["log", "identity", "identity"], sigmas=[0.1, 0.1, 0.1], lo=[2.0, 0.05, 1e-3], hi=[100.0, 1.0, 1.9])
    base.update(change)
    return MC.ObservationModel(**base)


@pytest.mark.parametrize("change,message", REFUSALS)
def test_refusals_of_the_statement(MC, change, message):
    model = refused_model(MC, change)
    with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)").replace("...", r"\.\.\.")):
        MC.observe(np.ones((model.n_coords, 2)), model, 1, backend="host")


def test_entry_points_refuse_on_the_host(MC):
    """The C entries check their arguments before they look for a device: every refusal is GWI_ERR_INVALID with its message, on a
    machine without a GPU too; valid arguments then meet GWI_ERR_NO_DEVICE there -- there is no CPU fallback."""
    from gwinferno_amd import _native

    lib = _native.load_library()
    for change, message in REFUSALS:
        model = refused_model(MC, change)
        with pytest.raises(_native.NativeEngineError, match="GWI_ERR_INVALID"):
            try:
                MC.observe(np.ones((model.n_coords, 2)), model, 1, backend="device")
            except _native.NativeEngineError as exc:
                assert message in str(exc), (message, str(exc))
                raise
    model = refused_model(MC, {})
    model._table = (np.array([0.0, 1.0]), np.array([0.0, 5000.0]))  # ends below hi_z + 9 sigma_z
    with pytest.raises(_native.NativeEngineError, match="the DL table covers"):
        MC.observe(np.ones((3, 2)), model, 1, backend="device")
    model._table = (np.array([0.0, 2.0, 1.0, 9.0]), np.array([0.0, 1.0, 2.0, 3.0]))
    with pytest.raises(_native.NativeEngineError, match="not ascending at entry 2"):
        MC.observe(np.ones((3, 2)), model, 1, backend="device")
    il = model.is_log
    dp = _native.as_dp
    st = lib.gwi_mock_posteriors(-1, 3, il.ctypes.data_as(C.POINTER(C.c_int32)), dp(model.sigmas), dp(model.lo), dp(model.hi), 2, 2, None, 1, 0, None, None)
    assert st == -1 and b"null data" in lib.gwi_mock_error()
    st = lib.gwi_mock_posteriors(-1, 3, None, dp(model.sigmas), dp(model.lo), dp(model.hi), 2, 2, None, 1, 0, None, None)
    assert st == -1 and b"null is_log" in lib.gwi_mock_error()
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        with pytest.raises(_native.NativeEngineError, match="GWI_ERR_NO_DEVICE"):
            MC.observe(np.ones((3, 2)), refused_model(MC, {}), 1, backend="device")


@pytest.mark.parametrize("d", U.EVIDENCE_DATA)
def test_evidence_identity(MC, d):
    mean, se, exact = U.evidence_identity(MC, d, seed=5, backend="host")
    print(f"d = {d:.4f}: importance average {mean:.6f} +- {se:.2g}, integrals {exact:.6f}")
    assert abs(mean - exact) <= 5.0 * se


def test_selection_identity(MC):
    """Found fraction of 2e5 sources from PL+Peak x PL q x PL z against the importance estimate from 4e5 mock injections (NumPy
    forms of the oracle), and the condition on n_eff the GPU test relies on."""
    f, var_f, n_found = U.direct_found_fraction(MC, 200_000, 11, "host")
    inj, total = U.mock_injections(MC, 400_000, 12, "host")
    mu, var_mu, n_eff = U.importance_efficiency(inj, total)
    print(f"direct {f:.5f} +- {var_f**0.5:.2g} ({n_found} found); importance {mu:.5f} +- {var_mu**0.5:.2g} (n_eff {n_eff:.0f})")
    assert n_eff >= 4 * n_found / 50
    assert abs(f - mu) <= 5.0 * np.sqrt(var_f + var_mu)


def test_make_mock_catalog_on_the_host(MC):
    model = U.catalog_model(MC)
    args = (U.population(MC), U.injection_tables(model), model, 5, 33, 6000, 21)
    pe, inj, total, truth = MC.make_mock_catalog(*args, backend="host")
    pe2, inj2, _, _ = MC.make_mock_catalog(*args, backend="host")
    assert total == 6000 and pe["mass_1"].shape == (5, 33) and truth["data"].shape == (3, 5) and np.all(truth["snr"] >= model.rho_th)
    assert all(np.array_equal(pe[k], pe2[k]) for k in pe) and all(np.array_equal(inj[k], inj2[k]) for k in inj)
    assert np.allclose(pe["prior"], MC.pe_prior(pe, model), rtol=1e-15) and inj["prior"].size == inj["mass_1"].size > 0
    strict = MC.default_model(rho_ref=8.0, mc_ref=25.0, dl_ref=1.0, rho_th=8.0)
    with pytest.raises(RuntimeError, match="detected fraction"):
        MC.make_mock_catalog(U.population(MC), U.injection_tables(strict), strict, 5, 4, 100, 21, backend="host", max_chunks=2)
