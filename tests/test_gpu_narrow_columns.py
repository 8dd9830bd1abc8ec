"""GPU: float32 spline coordinates in HBM (narrow_columns; include/gwi_engine.h: GWI_TERM_EXP_SPLINE_F32).  Config-3- and
config-5-shaped catalogs at reduced size whose spline coordinates (spin magnitudes and tilts; config 5's mass ratio too) are
float32 numbers: a narrow engine and a wide engine on the same arrays, both setup paths, give the same bits -- single
evaluations, gradients in replay mode, K = 16 batches on the matrix-core and on the 4-tap kernel, the per-sample log-weights --
lie within the C oracle's tolerances, shard like the wide engine, pick the same batched kernel and stream 4 bytes less per
narrowed column and sample.  A narrow column whose values are not float32 numbers is refused by the engine itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {"c3": ("bspline_iid", ("a_1", "a_2", "cos_tilt_1", "cos_tilt_2")), "c5": ("bspline_full", ("mass_ratio", "a_1", "a_2", "cos_tilt_1", "cos_tilt_2"))}
N_EV, N_PE, N_INJ = 24, 1024, 16384


def _catalog(cfg, nan=False):
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(N_EV, N_PE, N_INJ, seed=11)
    for k in CASES[cfg][1]:
        pe[k] = pe[k].astype(np.float32).astype(np.float64)
        inj[k] = inj[k].astype(np.float32).astype(np.float64)
    if nan:
        pe["a_1"] = pe["a_1"].copy()
        pe["a_1"][1, 7] = np.nan
        inj["cos_tilt_2"] = inj["cos_tilt_2"].copy()
        inj["cos_tilt_2"][5] = np.nan
    return pe, inj, total


def _pair(cfg, device_setup=None, nan=False):
    """(wide composition, narrow composition, total_inj): engines built, the narrow one first checked to be narrow."""
    from gwinferno_amd.compositions import COMPOSITIONS

    name = CASES[cfg][0]
    pe, inj, total = _catalog(cfg, nan)
    wide, narrow = COMPOSITIONS[name](pe, inj), COMPOSITIONS[name](pe, inj)
    wide.engine(device_setup=device_setup)
    narrow.engine(device_setup=device_setup, narrow_columns="auto")
    assert len(narrow.engine().bound.narrowed) == len(CASES[cfg][1])
    assert not wide.engine().bound.narrowed
    return wide, narrow, total


def _thetas(cfg, comp, n, seed=5):
    from gwinferno_amd.compositions import draw_params

    rng = np.random.default_rng(seed)
    return np.stack([comp.theta(draw_params(CASES[cfg][0], rng)) for _ in range(n)])


def _same_grad(a, b, exact):
    return np.array_equal(a, b) if exact else np.allclose(a, b, rtol=1e-12, atol=1e-13)


def _assert_same(a, b, exact_grad):
    assert a.log_likelihood == b.log_likelihood
    for f in ("log_l", "sum_logBFs", "selection_factor", "log_det_eff", "log_nEff_inj", "variance_log_detection_efficiency", "variance_log_likelihood",
              "min_log_nEff", "surveyed_hypervolume_norm", "log_norm_const"):
        assert getattr(a.summary, f) == getattr(b.summary, f), f
    assert np.array_equal(a.log_bfs, b.log_bfs) and np.array_equal(a.log_neffs, b.log_neffs) and np.array_equal(a.variances, b.variances)
    assert np.array_equal(a.norms, b.norms)
    assert _same_grad(a.grad, b.grad, exact_grad)


@pytest.mark.parametrize("device_setup", [True, False])
@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_single_evaluations_and_log_weights_equal_the_wide_engine(cfg, device_setup):
    wide, narrow, total = _pair(cfg, device_setup)
    ew, en = wide.engine(), narrow.engine()
    for th in _thetas(cfg, wide, 3):
        for sel in (False, True):
            _assert_same(en.evaluate(th, total, marginalize_selection=sel), ew.evaluate(th, total, marginalize_selection=sel), exact_grad=False)
    pw, iw = ew.log_weights(th)
    pn, inn = en.log_weights(th)
    assert np.array_equal(pw, pn) and np.array_equal(iw, inn)


@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_replay_mode_gradients_are_bit_equal(cfg, monkeypatch):
    monkeypatch.setenv("GWI_DETERMINISTIC", "1")
    wide, narrow, total = _pair(cfg)
    for th in _thetas(cfg, wide, 2, seed=8):
        _assert_same(narrow.engine().evaluate(th, total), wide.engine().evaluate(th, total), exact_grad=True)


@pytest.mark.parametrize("path,env", [("mfma", {"GWI_BATCH_MFMA": "1"}), ("taps", {"GWI_BATCH_MFMA": "0"})])
@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_batches_of_16_equal_the_wide_engine(cfg, path, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wide, narrow, total = _pair(cfg)
    ew, en = wide.engine(), narrow.engine()
    assert ew.batch_path(16) == en.batch_path(16) == path
    ths = _thetas(cfg, wide, 16, seed=13)
    bw, bn = ew.evaluate_batch(ths, total), en.evaluate_batch(ths, total)
    for a, b in zip(bn, bw):
        _assert_same(a, b, exact_grad=path == "mfma")  # the matrix-core gradient is bit-reproducible, the 4-tap one sums with LDS atomics


@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_within_the_c_oracle_tolerances(cfg):
    from golden_util import rel_err

    from oracle.c_oracle import COracle

    wide, narrow, total = _pair(cfg)
    orc = COracle(wide.engine().bound)
    for th in _thetas(cfg, wide, 2, seed=21):
        got = narrow.engine().evaluate(th, total, min_neff_cut=False)
        ref = orc.evaluate(th, total, min_neff_cut=False)
        assert rel_err(got.log_likelihood, ref["log_likelihood"]) < 1e-9
        assert rel_err(got.log_bfs, ref["logBFs"]) < 1e-9
        assert rel_err(got.log_neffs, ref["log_nEffs"]) < 1e-8
        scale = max(1.0, float(np.max(np.abs(ref["grad"]))))
        assert float(np.max(np.abs(got.grad - ref["grad"]))) / scale < 1e-8


@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_two_narrow_shards_equal_the_unsharded_wide_engine(cfg):
    from golden_util import rel_err

    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.engine import NativePopulationLikelihood

    wide, _, total = _pair(cfg)
    name = CASES[cfg][0]
    pe, inj, _ = _catalog(cfg)
    comp = COMPOSITIONS[name](pe, inj)
    p = comp.placeholder()
    shards = [NativePopulationLikelihood(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), rank=r, world=2, narrow_columns="auto") for r in range(2)]
    assert [t["kind"] for t in shards[0].bound.terms] == [t["kind"] for t in shards[1].bound.terms]
    assert len(shards[0].bound.narrowed) == len(CASES[cfg][1])
    ths = _thetas(cfg, wide, 4, seed=3)
    recs = np.stack([s.eval_batch_partial(ths)[0] for s in shards])
    got = shards[0].combine_batch(ths, recs, total)
    ref = wide.engine().evaluate_batch(ths, total)
    for g, r in zip(got, ref):
        assert rel_err(g.log_likelihood, r.log_likelihood) < 1e-12
        scale = max(1.0, float(np.max(np.abs(r.grad))))
        assert float(np.max(np.abs(g.grad - r.grad))) / scale < 1e-9
    for s in shards:
        s.close()


@pytest.mark.parametrize("env", [{}, {"GWI_BATCH_MFMA": "1"}, {"GWI_BATCH_MFMA": "0"}, {"GWI_BATCH_ROWS": "1"}, {"GWI_DETERMINISTIC": "1"}])
@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_kernel_choice_and_resident_bytes(cfg, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wide, narrow, _ = _pair(cfg)
    ew, en = wide.engine(), narrow.engine()
    for k in (1, 4, 9, 16):
        assert en.batch_path(k) == ew.batch_path(k), (k, en.batch_path(k), ew.batch_path(k))
    name = en.scan_kernel_name()
    assert "generic" not in name and "splinef" in name, name
    pw, iw = ew.resident_bytes()
    pn, inn = en.resident_bytes()
    n_narrow = len(CASES[cfg][1])
    assert pw - pn == 4 * n_narrow * N_EV * N_PE and iw - inn == 4 * n_narrow * N_INJ
    # gwi_read_column: the narrow column widened is the catalog's value (as parked by the binding)
    bm = en.bound
    c = bm.terms[bm.narrowed[0]]["cols"][0]
    assert np.array_equal(en.read_column("pe", c), bm.resident_columns("pe")[c])
    assert np.array_equal(en.read_column("inj", c), bm.resident_columns("inj")[c])


@pytest.mark.parametrize("device_setup", [True, False])
def test_an_fp64_column_asked_to_be_narrow_is_refused_by_the_engine(device_setup, monkeypatch):
    """The binding's own check stood aside: the engine counts the values a float32 round trip changes and names the term."""
    from gwinferno_amd import _native as N
    from gwinferno_amd import engine as E
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, _ = make_catalog(4, 256, 2048, seed=2)  # float64 spins
    monkeypatch.setattr(E, "_float32_exact", lambda values: True)
    comp = COMPOSITIONS["bspline_iid"](pe, inj)
    with pytest.raises(N.NativeEngineError, match=r"term 3 \(narrow spline, kind 15\): \d+ values of column \d+ do not survive a float32 round trip"):
        comp.engine(device_setup=device_setup, narrow_columns="auto")


@pytest.mark.parametrize("device_setup", [True, False])
def test_non_finite_entries_give_the_wide_results(device_setup):
    wide, narrow, total = _pair("c3", device_setup, nan=True)
    for th in _thetas("c3", wide, 2, seed=17):
        _assert_same(narrow.engine().evaluate(th, total), wide.engine().evaluate(th, total), exact_grad=False)
