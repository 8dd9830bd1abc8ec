"""GPU: resampled injection sets on the device (include/gwi_engine.h: gwi_resample_injections; gwinferno_amd/csrc/gwi_resample.h;
the reference's resample_injections, preprocess/selection.py:143-156).

The kernels are pinned to the NumPy statement (gwinferno_amd/draws.py: resample_indices_reference) by the bracket of
tests/test_gpu_draws.py: the expected log-weights come from the independent host evaluation of the bound model
(tests/bound_eval.py), their cumulative weights C are formed in np.longdouble, the uniforms are resample_uniforms', and a device
index j is accepted iff w_j > 0 and C_{j-1} - d <= u C_last < C_j + d with d = 1e-9 C_last, the project's parity bound for weights.
Every draw of every call is checked.  The sets (tests/resample_util.py: 2 events x 64 PE samples, injection counts at the kernels'
edges) are vetted without a device in tests/test_resample_cpu.py: test_inputs_of_the_gpu_tests; the host values at the fiducial
points (seed 151 catalogs, theta seeds 11 / 12) are

    injections   plpeak: n_eff, N           bspline_iid: n_eff, N        with weight
    1            0, 0 (the redshift normaliser of a one-injection set is 0)        0
    1023         144.39311220844638, 144    26.254024240174292, 26           198
    1024         127.48997880564691, 127    22.18780552941276, 22            210
    1025         112.08663119040327, 112    15.224573413810248, 15           199
    3077         226.68387824201037, 226    35.726017872634344, 35           592
    263171       16360.464760984469, 16360  1246.1826050234622, 1246       46496

each n_eff at least 2.8e-5 relative away from an integer, so N cannot differ between evaluations that agree to 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest
import resample_util as U
from test_gpu_draws import _check_segment

pytestmark = pytest.mark.gpu

SEED = U.DRAW_SEED
E2E = 3 * U.TILE + 5
_CASES = {}


def _case(name, n_inj):
    """One engine per (composition, set), its fiducial theta and the host evaluation: made once, shared, never changed."""
    key = (name, n_inj)
    if key not in _CASES:
        pe, inj, total = U.catalog(n_inj)
        comp = U.composition(name, pe, inj)
        eng = comp.engine()
        theta = comp.theta(U.params(name))
        lw = U.host_log_weights(eng.bound, theta)
        lw.setflags(write=False)
        _CASES[key] = dict(comp=comp, eng=eng, theta=theta, lw=lw, host=U.host_sums(lw), inj=inj, pe=pe, total=total)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for c in _CASES.values():
        c["eng"].close()
    _CASES.clear()


def _uniforms(first, n):
    from gwinferno_amd.draws import resample_uniforms

    return resample_uniforms(SEED, first, n)


def _check_sums(sums, host, what):
    """log sum w, log sum w^2 (1e-9 on the logarithm: every |log| of these sets is >= 1, so this asks no less than 1e-9 relative)
    and n_eff (1e-9 relative) against the host evaluation."""
    print(what, "device", sums, "host", host)
    assert abs(sums["log_sum_w"] - host["log_sum_w"]) <= 1e-9, what
    assert abs(sums["log_sum_w2"] - host["log_sum_w2"]) <= 1e-9, what
    assert abs(sums["n_eff"] - host["n_eff"]) <= 1e-9 * host["n_eff"], what
    assert sums["n_live"] == host["n_live"], what


@pytest.mark.parametrize("n_inj", U.N_INJ)
@pytest.mark.parametrize("name", U.COMPS)
def test_bracket_drawn_weights_and_sums(name, n_inj):
    """The reference's N draws and 4 096 draws of every set: every index in its bracket, the drawn log-weights those of
    log_weights bit for bit, the sums against the host, N = floor(n_eff) of the device's own doubles = the host's N."""
    c = _case(name, n_inj)
    eng, theta, host = c["eng"], c["theta"], c["host"]
    idx, lw_sel, sums = eng.resample_injections(theta, SEED)
    more_idx, more_lw, more_sums = eng.resample_injections(theta, SEED, n_request=4096)
    assert idx.dtype == np.int32 and lw_sel.dtype == np.float64 and idx.shape == lw_sel.shape and sums == more_sums
    if n_inj == 1:  # no injection with weight: nothing is drawn, whatever is asked for
        assert host["n_live"] == 0 and idx.size == 0 and more_idx.size == 0
        assert sums == {"log_sum_w": -np.inf, "log_sum_w2": -np.inf, "n_eff": 0.0, "n_live": 0}
        return
    _check_sums(sums, host, (name, n_inj))
    n = idx.size
    assert n == int(np.floor(sums["n_eff"])) and n == host["N"] and more_idx.size == 4096
    m = min(n, 4096)
    assert np.array_equal(more_idx[:m], idx[:m]) and np.array_equal(more_lw[:m], lw_sel[:m])
    _check_segment(c["lw"], None, _uniforms(0, 4096), more_idx, (name, n_inj))
    _check_segment(c["lw"], None, _uniforms(0, n), idx, (name, n_inj, "N draws"))
    dev_lw = eng.log_weights(theta)[1]
    assert np.array_equal(more_lw, dev_lw[more_idx]) and np.array_equal(lw_sel, dev_lw[idx])
    assert np.all(np.isfinite(more_lw))


@pytest.mark.parametrize("name", U.COMPS)
def test_draw_counts_and_purity(name):
    """n_request = 0, 1, 255, 256, 257 and 2^20 + 3 (over the launch cut) on the 3 * 1024 + 5 set: draws [0, n) equal
    [0, a) ++ [a, n) taken through first_index, bit for bit; a second call and a second handle of the same model give the
    same; every draw lies in its bracket."""
    c = _case(name, E2E)
    eng, theta = c["eng"], c["theta"]
    big = 2**20 + 3
    whole_idx, whole_lw, sums = eng.resample_injections(theta, SEED, n_request=big)
    assert whole_idx.size == big
    _check_segment(c["lw"], None, _uniforms(0, big), whole_idx, (name, "2^20 + 3"))
    for n in (0, 1, 255, 256, 257):
        idx, lw, s = eng.resample_injections(theta, SEED, n_request=n)
        assert idx.size == n and s == sums and np.array_equal(idx, whole_idx[:n]) and np.array_equal(lw, whole_lw[:n])
        for a in {0, n // 2, n}:
            i0, l0, _ = eng.resample_injections(theta, SEED, n_request=a)
            i1, l1, _ = eng.resample_injections(theta, SEED, n_request=n - a, first_index=a)
            assert np.array_equal(np.concatenate([i0, i1]), idx) and np.array_equal(np.concatenate([l0, l1]), lw)
    a = 2**20 - 7  # the second part starts before the cut of the whole and crosses it
    i1, l1, _ = eng.resample_injections(theta, SEED, n_request=big - a, first_index=a)
    assert np.array_equal(i1, whole_idx[a:]) and np.array_equal(l1, whole_lw[a:])
    i0, l0, _ = eng.resample_injections(theta, SEED, n_request=503, first_index=2**20 - 500)  # one launch where the whole had two
    assert np.array_equal(i0, whole_idx[2**20 - 500 :]) and np.array_equal(l0, whole_lw[2**20 - 500 :])
    again_idx, again_lw, again_sums = eng.resample_injections(theta, SEED, n_request=big)
    assert np.array_equal(again_idx, whole_idx) and np.array_equal(again_lw, whole_lw) and again_sums == sums
    ms, n_launch = [C.c_double(-1.0) for _ in range(3)], C.c_int32(-1)
    eng.lib.gwi_resample_times(*[C.byref(m) for m in ms], C.byref(n_launch))
    assert n_launch.value == 2 and all(m.value > 0.0 for m in ms)  # the calling thread's last call: 2^20 + 3 draws, two launches
    other_seed, _, _ = eng.resample_injections(theta, SEED + 1, n_request=257)
    assert not np.array_equal(other_seed, whole_idx[:257])
    comp2 = U.composition(name, c["pe"], c["inj"])
    eng2 = comp2.engine()
    try:
        idx2, lw2, sums2 = eng2.resample_injections(theta, SEED, n_request=4096)
        assert np.array_equal(idx2, whole_idx[:4096]) and np.array_equal(lw2, whole_lw[:4096]) and sums2 == sums
    finally:
        eng2.close()


@pytest.mark.parametrize("name", U.COMPS)
def test_against_draw_indices(name):
    """The same uniforms through gwi_draw_indices and through the new path: both pass the bracket (no equality between them is
    asked: the two searches may resolve a last-bit tie differently)."""
    c = _case(name, E2E)
    eng, theta = c["eng"], c["theta"]
    u = _uniforms(0, 512)
    _, old = eng.draw_indices(theta, None, u)
    new, _, _ = eng.resample_injections(theta, SEED, n_request=512)
    _check_segment(c["lw"], None, u, old, (name, "draw_indices"))
    _check_segment(c["lw"], None, u, new, (name, "resample_injections"))
    print(name, "indices that differ between the two paths:", int(np.sum(old != new)))


@pytest.mark.parametrize("name", U.COMPS)
def test_masks(name):
    """A mask that removes every other injection never yields a masked index and changes N; with one injection left, every draw
    is that one; an all-zero mask gives no draw and a ValueError from the catalog function; None restores the set."""
    from gwinferno_amd import catalog as K

    n_inj = U.TILE + 1
    c = _case(name, n_inj)
    eng, theta, lw = c["eng"], c["theta"], c["lw"]
    free_idx, _, free_sums = eng.resample_injections(theta, SEED, n_request=2048)
    half = (np.arange(n_inj) % 2).astype(np.uint8)
    try:
        eng.set_draw_mask(None, half)
        idx, lw_sel, sums = eng.resample_injections(theta, SEED)
        more_idx, _, _ = eng.resample_injections(theta, SEED, n_request=2048)
        host = U.host_sums(lw, half)
        _check_sums(sums, host, (name, "odd indices only"))
        assert idx.size == host["N"] == int(np.floor(sums["n_eff"])) and idx.size != int(np.floor(free_sums["n_eff"]))
        assert np.all(half[more_idx] == 1) and np.array_equal(more_idx[: idx.size], idx)
        _check_segment(lw, half, _uniforms(0, 2048), more_idx, (name, "odd indices only"))
        live = np.nonzero(np.isfinite(lw))[0]
        lone = np.zeros(n_inj, dtype=np.uint8)
        lone[live[-1]] = 1
        eng.set_draw_mask(None, lone)
        idx, lw_sel, sums = eng.resample_injections(theta, SEED, n_request=300)
        assert np.all(idx == live[-1]) and idx.size == 300 and sums["n_eff"] == 1.0 and sums["n_live"] == 1
        assert eng.resample_injections(theta, SEED)[0].size == 1
        assert np.all(lw_sel == eng.log_weights(theta)[1][live[-1]])
        eng.set_draw_mask(None, np.zeros(n_inj, dtype=np.uint8))
        idx, lw_sel, sums = eng.resample_injections(theta, SEED, n_request=300)
        assert idx.size == 0 and lw_sel.size == 0 and sums == {"log_sum_w": -np.inf, "log_sum_w2": -np.inf, "n_eff": 0.0, "n_live": 0}
        assert eng.resample_injections(theta, SEED)[0].size == 0
        with pytest.raises(ValueError, match="no injection carries weight"):
            K.resample_injections(SEED, eng, theta, c["inj"], c["total"], backend="device")
    finally:
        eng.set_draw_mask()
    back_idx, _, back_sums = eng.resample_injections(theta, SEED, n_request=2048)
    assert np.array_equal(back_idx, free_idx) and back_sums == free_sums


def test_refusals():
    """Null pointers and first_index < 0 (GWI_ERR_INVALID, with a message), a handle that holds a shard (GWI_ERR_UNSUPPORTED, from
    Python and from the library); the engine keeps working afterwards."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import NativePopulationLikelihood

    c = _case("plpeak", U.TILE - 1)
    eng, theta, comp = c["eng"], c["theta"], c["comp"]
    good = eng.resample_injections(theta, SEED, n_request=64)
    lib, dp, ip = eng.lib, N.as_dp, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    th, sums, idx, lw, made = N.f64(theta), np.zeros(4), np.zeros(64, dtype=np.int32), np.zeros(64), C.c_int64(0)
    m = C.byref(made)
    for args, word in (((None, 1, 0, 64, m, dp(sums), ip(idx), dp(lw)), "theta"), ((dp(th), 1, 0, 64, None, dp(sums), ip(idx), dp(lw)), "n_draws"),
                       ((dp(th), 1, 0, 64, m, None, ip(idx), dp(lw)), "sums"), ((dp(th), 1, 0, 64, m, dp(sums), None, dp(lw)), "idx"),
                       ((dp(th), 1, 0, -1, m, dp(sums), ip(idx), None), "logw_sel"), ((dp(th), 1, -1, 64, m, dp(sums), ip(idx), dp(lw)), "first_index")):
        assert lib.gwi_resample_injections(eng.handle, *args) == -1  # GWI_ERR_INVALID
        assert word in lib.gwi_last_error(eng.handle).decode(), (word, lib.gwi_last_error(eng.handle).decode())
    assert lib.gwi_resample_injections(eng.handle, dp(th), 1, 0, 0, m, dp(sums), None, None) == 0 and made.value == 0 and sums[2] == good[2]["n_eff"]
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*first_index"):
        eng.resample_injections(theta, SEED, n_request=4, first_index=-1)
    again = eng.resample_injections(theta, SEED, n_request=64)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1]) and again[2] == good[2]
    p = comp.placeholder()
    shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2) for r in range(2)]
    with pytest.raises(N.NativeEngineError, match="GWI_ERR_UNSUPPORTED"):
        shards[0].resample_injections(theta, SEED, n_request=4)
    seg = f"/gwi_resample_test_{os.getpid()}"
    try:
        for r, s in enumerate(shards):
            s.shm_comm_init(seg, r, 2)
        assert lib.gwi_resample_injections(shards[0].handle, dp(th), 1, 0, 64, m, dp(sums), ip(idx), dp(lw)) == -4  # GWI_ERR_UNSUPPORTED
        assert "shard" in lib.gwi_last_error(shards[0].handle).decode()
    finally:
        lib.gwi_shm_comm_unlink(seg.encode())
        for s in shards:
            s.close()


@pytest.mark.parametrize("name", U.COMPS)
def test_end_to_end(name):
    """catalog.resample_injections on the 3 * 1024 + 5 set (resample_util.end_to_end_catalog, seed 20240917): the device and host
    backends give the same indices except where the bracket allows another, and new priors that agree to 1e-12; an engine built
    from the new set with total_generated = N reproduces the full set's log mu at the fiducial theta to 1e-9 (every new weight
    is norm), and at the nearby theta' |log mu_res - log mu_full| <= 5 sqrt(1 / n_eff_res + 1 / n_eff_full) with the engines' own
    n_eff.  From the host backend on the CPU (tests/test_resample_cpu.py: test_end_to_end_on_the_host):
        plpeak       N = 189, |difference at theta'| = 0.006971 <= 0.511564
        bspline_iid  N = 33,  |difference at theta'| = 0.022953 <= 1.226778
    (there with n_eff = (sum w)^2 / sum w^2; the engines' own n_eff is the reference's mu^2 / sigma^2, which is larger, and gives the
    tighter bounds 0.359189 and 0.864294 on the device; at the fiducial point it is infinite for the resampled set)."""
    from gwinferno_amd import catalog as K
    from gwinferno_amd.draws import resample_indices_reference

    pe, inj, total = U.end_to_end_catalog()
    full = U.composition(name, pe, inj)
    eng = full.engine()
    res_eng = None
    try:
        p0, p1 = U.params(name), U.nearby_params(name)
        theta0 = full.theta(p0)
        lw = U.host_log_weights(eng.bound, theta0)
        new_h, n_h, neff_h = K.resample_injections(SEED, eng, theta0, inj, total, backend="host")  # Engine.log_weights + the statement
        new_d, n_d, neff_d = K.resample_injections(SEED, eng, theta0, inj, total, backend="device")
        assert n_d == n_h == {"plpeak": 189, "bspline_iid": 33}[name] and abs(neff_d - neff_h) <= 1e-9 * neff_h
        assert set(new_d) == set(inj) and all(v.shape == (n_d,) and v.dtype == np.float64 for v in new_d.values())
        idx_d, _, _ = eng.resample_injections(theta0, SEED)
        idx_h = resample_indices_reference(eng.log_weights(theta0)[1], None, SEED, 0, n_h)
        _check_segment(lw, None, _uniforms(0, n_d), idx_d, (name, "end to end"))  # where the indices differ, the bracket allows it
        same = idx_d == idx_h
        print(name, "indices that differ between the backends:", int(np.sum(~same)))
        for k in inj:
            if k != "prior":
                assert np.array_equal(new_d[k], inj[k][idx_d]) and np.array_equal(new_d[k][same], new_h[k][same])
        assert np.allclose(new_d["prior"][same], new_h["prior"][same], rtol=1e-12, atol=0.0)
        # the array form through the device backend
        names = list(inj)
        arr, n_a, neff_a = K.resample_injections(SEED, eng, theta0, (np.stack([inj[k] for k in names]), {k: i for i, k in enumerate(names)}), total)
        assert n_a == n_d and neff_a == neff_d and all(np.array_equal(arr[i], new_d[k]) for i, k in enumerate(names))
        assert U.same_redshift_range(pe, inj, new_d)
        res = U.composition(name, pe, new_d)
        res_eng = res.engine()
        at0_full = eng.evaluate(theta0, total, min_neff_cut=False).summary
        at0_res = res_eng.evaluate(res.theta(p0), float(n_d), min_neff_cut=False).summary
        print(name, "fiducial log mu: full", at0_full.log_det_eff, "resampled", at0_res.log_det_eff)
        assert abs(at0_res.log_det_eff - at0_full.log_det_eff) <= 1e-9
        at1_full = eng.evaluate(full.theta(p1), total, min_neff_cut=False).summary
        at1_res = res_eng.evaluate(res.theta(p1), float(n_d), min_neff_cut=False).summary
        bound = 5.0 * np.sqrt(1.0 / np.exp(at1_res.log_nEff_inj) + 1.0 / np.exp(at1_full.log_nEff_inj))
        print(name, "theta': |log mu_res - log mu_full| =", abs(at1_res.log_det_eff - at1_full.log_det_eff), "<=", bound)
        assert abs(at1_res.log_det_eff - at1_full.log_det_eff) <= bound
    finally:
        eng.close()
        if res_eng is not None:
            res_eng.close()
