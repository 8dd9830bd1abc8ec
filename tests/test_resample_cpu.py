"""CPU: resampled injection sets (include/gwi_engine.h: gwi_resample_injections; gwinferno_amd/csrc/gwi_resample.h; the reference's
resample_injections, preprocess/selection.py:143-156) -- the uniforms and the NumPy statement of the draws (gwinferno_amd/draws.py),
the arithmetic of catalog.resample_injections(backend="host") against the reference's formulas written out here, the header and the
library's exports, and the inputs of tests/test_gpu_resample.py, which are vetted here where no device is needed."""
import os
import re

import numpy as np
import pytest
import resample_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_uniforms():
    """population_draws.draw_uniforms' construction with the resampling stream's tag and table 0; a split at first_index
    concatenates to the whole."""
    from gwinferno_amd import draws as D
    from gwinferno_amd import population_draws as P
    from gwinferno_amd import spin_priors as S

    assert D.RESAMPLE_TAG == 0x52534D50 and D.RESAMPLE_TAG != P.COUNTER_TAG and D.RESAMPLE_TAG >= 2 * 65536
    seed, first, n = 0x0123456789ABCDEF, 2**32 - 3, 8  # the index crosses 2^32: its high word is counter word 1
    u = D.resample_uniforms(seed, first, n)
    assert u.dtype == np.float64 and u.shape == (n,) and np.all((u >= 0.0) & (u < 1.0))
    for j in range(n):
        idx = first + j
        w = S.philox4x32_10(idx & 0xFFFFFFFF, idx >> 32, 0, D.RESAMPLE_TAG, seed & 0xFFFFFFFF, seed >> 32)
        assert u[j] == float(S._uniform53(w[0], w[1]))
    tag = P.COUNTER_TAG
    try:
        P.COUNTER_TAG = D.RESAMPLE_TAG
        assert np.array_equal(P.draw_uniforms(seed, first, n, 0)[0], u)
    finally:
        P.COUNTER_TAG = tag
    assert not np.any(P.draw_uniforms(seed, first, n, 0)[0] == u)  # another tag: another stream
    whole = D.resample_uniforms(7, 0, 1000)
    for a in (0, 1, 255, 256, 999, 1000):
        assert np.array_equal(np.concatenate([D.resample_uniforms(7, 0, a), D.resample_uniforms(7, a, 1000 - a)]), whole)
    assert not np.array_equal(D.resample_uniforms(8, 0, 1000), whole)


def test_statement_draws_follow_the_weights():
    """resample_indices_reference on a 5 000-sample weight vector: draw_indices_reference fed with the stream's uniforms, no sample
    without weight, and the drawn frequencies of the ten heaviest samples within five binomial standard deviations of their
    normalised weights (the check of tests/test_gpu_draws.py:348-350)."""
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(5)
    lw = rng.normal(0.0, 2.0, size=5000)
    lw[rng.uniform(size=5000) < 0.1] = -np.inf
    lw[17] = np.nan
    mask = (rng.uniform(size=5000) < 0.8).astype(np.uint8)
    n = 4096
    idx = D.resample_indices_reference(lw, mask, seed=3, first_index=0, n=n)
    assert idx.dtype == np.int32 and idx.shape == (n,)
    assert np.array_equal(idx, D.draw_indices_reference(lw, mask, D.resample_uniforms(3, 0, n)))
    assert np.array_equal(idx[100:], D.resample_indices_reference(lw, mask, 3, 100, n - 100))
    w = D.draw_weights(lw, mask)
    prob = w / w.sum()
    counts = np.bincount(idx, minlength=w.size)
    assert counts.sum() == n and np.all(counts[w == 0] == 0)
    for j in np.argsort(prob)[-10:]:
        assert abs(counts[j] / n - prob[j]) <= 5.0 * np.sqrt(prob[j] * (1.0 - prob[j]) / n), (int(j), int(counts[j]), float(prob[j]))
    assert np.all(D.resample_indices_reference(np.full(9, -np.inf), None, 1, 0, 4) == -1)


class _StubEngine:
    """An engine that exposes log_weights only."""

    def __init__(self, lw_inj):
        self.lw_inj = np.asarray(lw_inj, dtype=np.float64)

    def log_weights(self, theta):
        return np.zeros((1, 1)), self.lw_inj.copy()


def test_host_backend_is_the_references_arithmetic():
    """catalog.resample_injections(backend="host") over a stub engine against selection.py:143-156 written out: N, norm, the new
    prior and Neff_new; shapes, keys; the array + param_map form gives the same numbers; no weight raises."""
    from gwinferno_amd import catalog as K
    from gwinferno_amd import draws as D

    rng = np.random.default_rng(8)
    n_inj, n_draw, seed = 3000, 60_000.0, 21
    injdict = {"mass_1": rng.uniform(5, 80, n_inj), "redshift": rng.uniform(0, 1, n_inj), "prior": rng.uniform(0.01, 2.0, n_inj)}
    model_prob = rng.lognormal(0.0, 1.5, n_inj)          # p(theta_i | Lambda_0)
    model_prob[rng.uniform(size=n_inj) < 0.2] = 0.0      # outside the model's support
    with np.errstate(divide="ignore"):
        eng = _StubEngine(np.log(model_prob / injdict["prior"]))
    # the reference, line by line
    wts = model_prob / injdict["prior"]
    n_ref = int(np.sum(wts) ** 2 // np.sum(wts * wts))
    norm = np.sum(wts) / n_draw
    s2_new = np.sum(wts * wts) / (n_draw * n_draw) - norm * norm / n_draw
    neff_ref = norm * norm / s2_new
    new, n, neff = K.resample_injections(seed, eng, np.zeros(3), injdict, n_draw, backend="host")
    assert n == n_ref and 1 < n < n_inj and isinstance(n, int) and isinstance(neff, float)
    assert abs(neff - neff_ref) <= 1e-12 * neff_ref
    idx = D.resample_indices_reference(eng.lw_inj, None, seed, 0, n)
    assert np.all(model_prob[idx] > 0)
    assert set(new) == set(injdict) and all(v.shape == (n,) for v in new.values())
    for k in ("mass_1", "redshift"):
        assert np.array_equal(new[k], injdict[k][idx])
    assert np.allclose(new["prior"], model_prob[idx] / norm, rtol=1e-12, atol=0.0)
    # under the fiducial model every new weight is norm: with total_generated = N the detection efficiency is unchanged
    assert np.allclose(model_prob[idx] / new["prior"], norm, rtol=1e-12, atol=0.0)
    assert abs(np.sum(model_prob[idx] / new["prior"]) / n - np.sum(wts) / n_draw) <= 1e-12 * norm
    # the reference's (injdata, param_map) form
    param_map = {"redshift": 0, "prior": 1, "mass_1": 2}
    injdata = np.stack([injdict["redshift"], injdict["prior"], injdict["mass_1"]])
    new_arr, n_arr, neff_arr = K.resample_injections(seed, eng, np.zeros(3), (injdata, param_map), n_draw, backend="host")
    assert new_arr.shape == (3, n) and n_arr == n and neff_arr == neff
    for k, row in param_map.items():
        assert np.array_equal(new_arr[row], new[k])
    assert np.array_equal(injdata[1], injdict["prior"])  # the caller's array is left alone
    # a mask thins the set like weights of zero do
    mask = (np.arange(n_inj) % 2).astype(np.uint8)
    _, n_half, _ = K.resample_injections(seed, eng, np.zeros(3), injdict, n_draw, backend="host", inj_mask=mask)
    assert n_half == int(np.sum(wts * mask) ** 2 // np.sum((wts * mask) ** 2)) != n
    with pytest.raises(ValueError, match="no injection carries weight"):
        K.resample_injections(seed, _StubEngine(np.full(n_inj, -np.inf)), np.zeros(3), injdict, n_draw, backend="host")
    with pytest.raises(ValueError, match="no injection carries weight"):
        K.resample_injections(seed, eng, np.zeros(3), injdict, n_draw, backend="host", inj_mask=np.zeros(n_inj, dtype=np.uint8))
    with pytest.raises(ValueError, match="backend"):
        K.resample_injections(seed, eng, np.zeros(3), injdict, n_draw, backend="eager")
    with pytest.raises(ValueError, match="prior has shape"):
        K.resample_injections(seed, eng, np.zeros(3), {"prior": np.ones((2, 3))}, n_draw, backend="host")


def test_new_symbols_in_binding_header_and_library():
    from gwinferno_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym in ("gwi_resample_injections", "gwi_resample_times"):
        assert sym in _native.EXPORTED_SYMBOLS and sym in declared and hasattr(lib, sym)
    assert "selection.py:143-156" in hdr
    assert len(lib.gwi_resample_injections.argtypes) == 9 and len(lib.gwi_resample_times.argtypes) == 4
    assert lib.gwi_abi_version() == 3  # an added export, no struct changed
    assert lib.gwi_resample_injections(None, None, 0, 0, 0, None, None, None, None) == -1  # GWI_ERR_INVALID


def test_host_only_handle_is_refused():
    from gwinferno_amd import _native as N

    pe, inj, _ = U.catalog(U.TILE - 1)
    eng = U.composition("plpeak", pe, inj, device=N.DEVICE_HOST_ONLY).engine()
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
        eng.resample_injections(np.zeros(eng.n_theta), 1)
    with pytest.raises(ValueError, match="theta has shape"):
        eng.resample_injections(np.zeros(eng.n_theta + 1), 1)
    with pytest.raises(ValueError, match="n_request"):
        eng.resample_injections(np.zeros(eng.n_theta), 1, n_request=-5)


@pytest.mark.parametrize("name", U.COMPS)
def test_inputs_of_the_gpu_tests(name):
    """Every set of tests/test_gpu_resample.py at its fiducial point, from the host evaluation: live injections (none in the set
    of one, whose redshift normaliser is 0), a host n_eff farther than 1e-6 relative from an integer (so N = floor(n_eff) cannot
    differ between two evaluations that agree to 1e-9), and |log sum w|, |log sum w^2| >= 1 (so that 1e-9 absolute on a logarithm --
    1e-9 relative on the sum -- asks no less than 1e-9 relative on the logarithm).  The same for the half-masked sets."""
    from gwinferno_amd import _native as N

    for n_inj in U.N_INJ:
        pe, inj, _ = U.catalog(n_inj)
        comp = U.composition(name, pe, inj, device=N.DEVICE_HOST_ONLY)
        lw = U.host_log_weights(comp.engine().bound, comp.theta(U.params(name)))
        for mask in (None, (np.arange(n_inj) % 2).astype(np.uint8)):
            s = U.host_sums(lw, mask)
            print(f"{name} n_inj = {n_inj}{' (odd indices only)' if mask is not None else ''}: {s}")
            if n_inj == 1:
                assert s["n_live"] == 0 and s["N"] == 0
                continue
            assert s["n_live"] >= 90 and s["N"] >= 8
            assert abs(s["n_eff"] - round(s["n_eff"])) > 1e-6 * s["n_eff"]
            assert abs(s["log_sum_w"]) >= 1.0 and abs(s["log_sum_w2"]) >= 1.0
        assert U.host_sums(lw, None)["N"] != U.host_sums(lw, mask)["N"] or n_inj == 1


def _log_mu_and_neff(comp, p, total):
    lw = U.host_log_weights(comp.engine().bound, comp.theta(p))
    s = U.host_sums(lw)
    return s["log_sum_w"] - np.log(total), s["n_eff"]


@pytest.mark.parametrize("name", U.COMPS)
def test_end_to_end_on_the_host(name):
    """The host backend on the 3 * 1024 + 5 set (resample_util.end_to_end_catalog): a model built from the resampled set with total_generated = N has the full set's
    log mu at the fiducial point (1e-9: every new weight is norm), and at the nearby point theta' of the GPU test
    |log mu_res - log mu_full| <= 5 sqrt(1 / n_eff_res + 1 / n_eff_full).  The values printed here are the ones quoted in
    tests/test_gpu_resample.py: test_end_to_end."""
    from gwinferno_amd import _native as N
    from gwinferno_amd import catalog as K

    pe, inj, total = U.end_to_end_catalog()
    full = U.composition(name, pe, inj, device=N.DEVICE_HOST_ONLY)
    p0, p1 = U.params(name), U.nearby_params(name)
    host = U.HostEngine(full.engine().bound, inj["prior"].size)
    new, n, neff_new = K.resample_injections(U.DRAW_SEED, host, full.theta(p0), inj, total, backend="host")
    s = U.host_sums(host.log_weights(full.theta(p0))[1])
    assert n == s["N"] and set(new) == set(inj) and all(v.shape == (n,) for v in new.values())
    assert abs(neff_new - 1.0 / (1.0 / s["n_eff"] - 1.0 / total)) <= 1e-9 * neff_new
    assert U.same_redshift_range(pe, inj, new)
    res = U.composition(name, pe, new, device=N.DEVICE_HOST_ONLY)
    mu_full, _ = _log_mu_and_neff(full, p0, total)
    mu_res, neff_res0 = _log_mu_and_neff(res, p0, float(n))
    print(f"{name}: N = {n}, Neff_new = {neff_new:.6f}; fiducial: log mu full {mu_full:.12f} resampled {mu_res:.12f} (n_eff of the resampled set {neff_res0:.3f})")
    assert abs(mu_res - mu_full) <= 1e-9 and abs(neff_res0 - n) <= 1e-6 * n
    mu_full1, neff_full1 = _log_mu_and_neff(full, p1, total)
    mu_res1, neff_res1 = _log_mu_and_neff(res, p1, float(n))
    bound = 5.0 * np.sqrt(1.0 / neff_res1 + 1.0 / neff_full1)
    print(f"{name}: theta': log mu full {mu_full1:.9f} resampled {mu_res1:.9f}: |difference| {abs(mu_res1 - mu_full1):.6f} <= {bound:.6f} (n_eff {neff_full1:.3f}, {neff_res1:.3f})")
    assert abs(mu_res1 - mu_full1) <= bound
