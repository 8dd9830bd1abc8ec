"""GPU: gwi_effective_spins and gwi_chi_p_conditional_prior (gwinferno_amd/csrc/gwi_spinprior.h) against the golden file, the 50-digit
values and the NumPy statement (gwinferno_amd/spin_priors.py), and catalogs made on the device against catalogs made by the statement,
through the engine.  Bounds as in tests/test_spin_priors_cpu.py: 4 E for the closed forms (E the reference's own deviation from the 50-digit
values, per prior and per sample set).  The conditional prior is held to the statement on the same stream of uniforms: `accepted`
exactly, and p to COND_BOUND = 1e-12.  That bound is worked out, not measured (no device figure has been taken yet; once one has, the
bound is 10 x the measured maximum per case, recorded in profiles/effective_spins/RESULTS.md).  Both sides evaluate the same fp64
expressions on bit-identical draws and weights (no contraction on the device), so they differ by (a) the device's exponential,
<= 1.6e-14 relative per term (gwi_device.h), and (b) the order of sums of at most 10^4 terms: both sum in trees whose longest serial
run is 40 terms, an error of at most 64 x 2^-53 = 7e-15 per sum; the variance is a difference of moments about the mid-point of the
range, which loses at most a factor ~10, and a relative change of the bandwidth moves a kernel sum by a factor of order 10 times as
much in the tails: 7e-15 x 10 x 10 = 7e-13.  A difference above 1e-9 would mean that the two do not evaluate the same sums at all."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "effective_spins.npz")
PRIORS = ("p_chi_eff_iso", "p_chi_eff_aligned", "p_chi_p_iso")
E_FLOOR = 2.0**-50
COND_BOUND = 1e-12


def cond_check(case, err):
    print(f"{case}: largest relative difference device vs statement {err:.3e} (bound {COND_BOUND:.1e})")
    assert err <= COND_BOUND, (case, err)


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def S():
    from gwinferno_amd import spin_priors

    return spin_priors


def rel(got, want):
    m = want != 0.0
    if not m.all():
        return max(float(np.max(np.abs(got[~m]))), rel(got[m], want[m]))
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0


def set_bounds(ref, hp, keep):
    """4 E per prior for one sample set, E being the reference's own largest relative deviation from the 50-digit values on that set."""
    out = {}
    for k, p in enumerate(PRIORS):
        m = keep & (hp[k] != 0.0)
        e = float(np.max(np.abs(ref[k][m] - hp[k][m]) / np.abs(hp[k][m]))) if m.any() else 0.0
        out[p] = 4.0 * max(e, E_FLOOR)
    return out


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_closed_forms_against_golden_50_digits_and_statement(G, S):
    sets = []
    for tag, A in (("1", 1.0), ("0.8", 0.8)):
        sets.append((f"random a_max={tag}", A, G["random_inputs"], G[f"random_ref_{tag}"], G[f"random_hp_{tag}"], G[f"random_keep_{tag}"]))
        sets.append((f"hand a_max={tag}", A, G[f"hand_inputs_{tag}"], G[f"hand_ref_{tag}"], G[f"hand_hp_{tag}"], G[f"hand_keep_{tag}"]))
    sets.append(("random float32 a_max=1", 1.0, G["random_inputs_f32"], G["random_f32_ref_1"], None, G["random_f32_keep_1"]))
    failures = []
    for name, A, cols, ref, hp, keep in sets:
        bound = set_bounds(ref, hp, keep) if hp is not None else set_bounds(G["random_ref_1"], G["random_hp_1"], G["random_keep_1"])
        dev = S.effective_spins(*cols, a_max=A, backend="device")  # (float32 columns are widened by the Python layer)
        host = S.effective_spins(*cols, a_max=A, backend="host")
        for k in ("chi_eff", "chi_p"):
            assert np.max(np.abs(dev[k] - host[k])) <= 1e-15, (name, k)
        for k, p in enumerate(PRIORS):
            e_ref, e_host = rel(dev[p][keep], ref[k][keep]), rel(dev[p][keep], host[p][keep])
            e_hp = rel(dev[p][keep], hp[k][keep]) if hp is not None else 0.0
            print(f"{name:26s} {p:18s} device vs reference {e_ref:.3e}  vs 50 digits {e_hp:.3e}  vs statement {e_host:.3e}  bound {bound[p]:.3e}")
            if max(e_ref, e_hp, e_host) > bound[p] or not np.all(np.isfinite(dev[p][keep])):
                failures.append((name, p, e_ref, e_hp, e_host))
    assert not failures, failures


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 2048 * 256 + 300])
def test_shapes(S, n):
    """One lane per sample, 2048 workgroups of 256 at most: the last size runs the stride loop twice."""
    rng = np.random.default_rng(n)
    cols = [rng.uniform(0.05, 1.0, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)]
    dev = S.effective_spins(*cols, backend="device")
    assert all(v.shape == (n,) for v in dev.values()) and set(dev) == set(S.OUTPUTS)
    pick = np.unique(np.concatenate([np.arange(min(n, 300)), np.arange(max(n - 600, 0), n)])).astype(int)
    host = S.effective_spins(*(c[pick] for c in cols), backend="host")
    for k in S.OUTPUTS:
        assert np.all(np.isfinite(dev[k])) and np.allclose(dev[k][pick], host[k], rtol=1e-7, atol=1e-12), k
    if n == 0:
        from gwinferno_amd import _native

        lib = _native.load_library()
        guard = np.full(4, 7.0)
        st = lib.gwi_effective_spins(0, None, None, None, None, None, 1.0, _native.as_dp(guard), None, None, None, None, -1)
        assert st == 0 and np.all(guard == 7.0)


def test_null_outputs_bad_inputs_and_a_max(S, G):
    cols = [c[:500].copy() for c in G["random_inputs"]]
    full = S.effective_spins(*cols, a_max=0.8, backend="device")
    for mask in range(32):  # each subset of outputs: the others are NULL
        outs = tuple(o for i, o in enumerate(S.OUTPUTS) if mask >> i & 1)
        got = S.effective_spins(*cols, a_max=0.8, backend="device", outputs=outs)
        assert set(got) == set(outs) and all(same(got[o], full[o]) for o in outs)
    host = S.effective_spins(*cols, a_max=0.8, backend="host")
    assert np.any(full["p_chi_p_iso"] == 0.0)  # chi_p >= a_max = 0.8
    for p in PRIORS:
        assert same(full[p] == 0.0, host[p] == 0.0), p
    bad = [np.array([0.5, np.nan, 0.0, -0.2, 0.5, 0.5, 0.5, np.inf]), np.array([0.2, 0.2, 0.2, 0.2, np.nan, 0.2, 0.2, 0.2]), np.full(8, 0.1),
           np.array([0.3, 0.3, 0.3, 0.3, 0.3, 1.5, 0.3, 0.3]), np.array([0.3, 0.3, 0.3, 0.3, 0.3, 0.3, -1.0000001, 0.3])]
    out = S.effective_spins(*bad, backend="device")
    for v in out.values():
        assert np.isfinite(v[0]) and np.all(np.isnan(v[1:]))


COND_CASES = {"n37_d1000": (37, 1000), "n3_d257": (3, 257), "n3_d4096": (3, 4096), "n3_d10000": (3, 10000)}


def cond_points(n, seed):
    rng = np.random.default_rng(seed)
    q, chi_eff = rng.uniform(0.3, 1.0, n), rng.uniform(-0.5, 0.5, n)
    return rng.uniform(0.05, 0.8, n), chi_eff, q


@pytest.mark.parametrize("case", sorted(COND_CASES))
def test_conditional_prior_agrees_with_the_statement(S, case):
    n, ndraws = COND_CASES[case]
    pts = cond_points(n, ndraws)
    dev, acc_d = S.chi_p_prior_given_chi_eff_q(*pts, ndraws=ndraws, seed=17, first_index=5, backend="device", return_accepted=True)
    host, acc_h = S.chi_p_prior_given_chi_eff_q(*pts, ndraws=ndraws, seed=17, first_index=5, backend="host", return_accepted=True)
    assert np.array_equal(acc_d, acc_h) and np.all(acc_d == ndraws)  # integer logic on identical uniforms
    err = float(np.max(np.abs(dev - host) / np.abs(host)))
    assert np.all(np.isfinite(dev))
    cond_check(case, err)


def test_conditional_prior_is_reproducible_and_shardable(S):
    pts = cond_points(64, 3)
    kw = dict(ndraws=500, seed=99, backend="device", return_accepted=True)
    a, acc_a = S.chi_p_prior_given_chi_eff_q(*pts, **kw)
    b, acc_b = S.chi_p_prior_given_chi_eff_q(*pts, **kw)
    assert same(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(acc_a, acc_b)
    lo, _ = S.chi_p_prior_given_chi_eff_q(*(p[:32] for p in pts), first_index=0, **kw)
    hi, _ = S.chi_p_prior_given_chi_eff_q(*(p[32:] for p in pts), first_index=32, **kw)
    assert same(np.concatenate([lo, hi]).view(np.uint64), a.view(np.uint64))
    # few physical draws: the count is reported and agrees with the statement; none: 0 and NaN
    p, acc = S.chi_p_prior_given_chi_eff_q(0.2, 0.9, 0.9, ndraws=2000, seed=3, max_attempts=8, backend="device", return_accepted=True)
    ph, acch = S.chi_p_prior_given_chi_eff_q(0.2, 0.9, 0.9, ndraws=2000, seed=3, max_attempts=8, backend="host", return_accepted=True)
    assert 2 <= int(acc) < 2000 and int(acc) == int(acch)
    cond_check("few_draws", float(abs(p - ph) / abs(ph)))
    p, acc = S.chi_p_prior_given_chi_eff_q([0.3, 0.3], [1.5, np.nan], [0.7, 0.7], ndraws=100, max_attempts=1, backend="device", return_accepted=True)
    assert np.all(acc == 0) and np.all(np.isnan(p))


def test_invalid_arguments_and_code_object(S):
    from gwinferno_amd import _native

    lib = _native.load_library()
    x = np.array([0.3])
    p, acc = np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
    args = lambda nd, ma: (1, _native.as_dp(x), _native.as_dp(x), _native.as_dp(x), 1.0, nd, ma, 0, 0, _native.as_dp(p), acc.ctypes.data_as(C.POINTER(C.c_int32)), -1)  # noqa: E731
    assert lib.gwi_chi_p_conditional_prior(*args(1, 64)) == -1 and lib.gwi_chi_p_conditional_prior(*args(100, 0)) == -1
    assert p[0] == 7.0 and acc[0] == 7
    assert lib.gwi_chi_p_conditional_prior(*args(100, 64)) == 0 and np.isfinite(p[0]) and acc[0] == 100
    total, longest, launches = S.last_device_times()
    assert launches == 1 and 0.0 < longest <= total
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    notes = subprocess.run([readelf, "--notes", os.path.join(os.path.dirname(_native.LIB_PATH), "gwi_kernels.hsaco")], capture_output=True, text=True).stdout
    per = dict(zip(re.findall(r"\.name:\s+(\S+)", notes), re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)))
    ours = {n: s for n, s in per.items() if "spinprior" in n}
    assert len(ours) == 2 and set(ours.values()) == {"0"}, ours


def _engines_agree(name, pe_d, inj_d, pe_h, inj_h, total):
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params

    results = []
    for pe, inj in ((pe_d, inj_d), (pe_h, inj_h)):
        comp = COMPOSITIONS[name](pe, inj)
        eng = comp.engine(device=0)
        try:
            results.append(eng.evaluate(comp.theta(draw_params(name, np.random.default_rng(3))), total, min_neff_cut=False))
        finally:
            eng.close()
    d, h = results
    assert np.isfinite(h.log_likelihood) and abs(d.log_likelihood - h.log_likelihood) <= 1e-9 * abs(h.log_likelihood)
    for site in ("log_bfs", "log_neffs", "variances"):
        assert np.allclose(getattr(d, site), getattr(h, site), rtol=1e-9, atol=1e-9), site
    assert float(np.max(np.abs(d.grad - h.grad))) <= 1e-8 * max(1.0, float(np.max(np.abs(h.grad))))


@pytest.fixture(scope="module")
def component_catalog():
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(8, 512, 2000, seed=11)
    drop = ("chi_eff", "chi_p")
    return {k: v for k, v in pe.items() if k not in drop}, {k: v for k, v in inj.items() if k not in drop}, total


def test_catalog_end_to_end_chi_eff(component_catalog):
    """Catalogs with `chi_eff` alone.  The `bspline_chieff` composition (BSplineEffectiveSpinDims) also reads `chi_p`, so it is the next
    test's; the composition here is `bspline_misc`, the one that reads `chi_eff` and no `chi_p`."""
    from gwinferno_amd.catalog import effective_spin_catalogs

    pe, inj, total = component_catalog
    names = ["mass_1", "mass_ratio", "redshift", "chi_eff"]
    pe_d, inj_d = effective_spin_catalogs(pe, inj, names, backend="device")
    pe_h, inj_h = effective_spin_catalogs(pe, inj, names, backend="host")
    assert "chi_p" not in pe_d and pe_d["chi_eff"].shape == (8, 512) and inj_d["prior"].shape == (2000,)
    _engines_agree("bspline_misc", pe_d, inj_d, pe_h, inj_h, total)


def test_catalog_end_to_end_chi_eff_and_chi_p(component_catalog):
    """BSplineEffectiveSpinDims (the `bspline_chieff` composition) on catalogs with the joint prior at ndraws = 2000: the device and the
    statement share the stream of uniforms, so the project's bars apply.  (Most of this test's time is the statement on the host.)"""
    from gwinferno_amd.catalog import effective_spin_catalogs

    pe, inj, total = component_catalog
    names = ["mass_1", "mass_ratio", "redshift", "chi_eff", "chi_p"]
    pe_d, inj_d = effective_spin_catalogs(pe, inj, names, backend="device", ndraws=2000, seed=4)
    pe_h, inj_h = effective_spin_catalogs(pe, inj, names, backend="host", ndraws=2000, seed=4)
    ok = np.isfinite(pe_h["prior"])
    assert np.array_equal(ok, np.isfinite(pe_d["prior"]))
    cond_check("catalog_chi_p", float(np.max(np.abs(pe_d["prior"][ok] / pe_h["prior"][ok] - 1.0))))
    _engines_agree("bspline_chieff", pe_d, inj_d, pe_h, inj_h, total)
