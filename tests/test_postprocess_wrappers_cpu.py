"""CPU: the refusals of the post-processing wrappers (gwinferno_amd/engine_post.py) that need no engine: the shard refusal of every
wrapper that has one, and the shape, dtype and value refusals of the helpers the wrappers share.  Every message is written out here."""
import numpy as np
import pytest

from gwinferno_amd import _native as N
from gwinferno_amd.engine import NativePopulationLikelihood

N_THETA, N_EV, N_PE, N_INJ = 3, 2, 5, 7
TH = np.zeros(N_THETA)

# method -> (arguments, the text of the refusal on an engine that holds a shard)
SHARD_REFUSALS = {
    "draw_indices": ((TH,), "GWI_ERR_UNSUPPORTED: draw_indices: this engine holds one shard of the catalog; injection draws need the global set"),
    "resample_injections": ((TH, 1), "GWI_ERR_UNSUPPORTED: resample_injections: this engine holds one shard of the catalog; injection draws need the global set"),
    "set_histogram_bins": ((None, None, 4), "GWI_ERR_UNSUPPORTED: set_histogram_bins: this engine holds one shard of the catalog; the injection histogram needs the global set"),
    "weighted_histograms": ((TH,), "GWI_ERR_UNSUPPORTED: weighted_histograms: this engine holds one shard of the catalog; the injection histogram needs the global set"),
    "point_cdfs": ((TH,), "GWI_ERR_UNSUPPORTED: point_cdfs: this engine holds one shard of the catalog; the injection CDF needs the global set"),
    "marginal_weights_reset": ((), "GWI_ERR_UNSUPPORTED: marginal_weights_reset: this engine holds one shard of the catalog; the injection weights need the global set"),
    "marginal_weights_add": ((TH,), "GWI_ERR_UNSUPPORTED: marginal_weights_add: this engine holds one shard of the catalog; the injection weights need the global set"),
    "marginal_point_weights": ((), "GWI_ERR_UNSUPPORTED: marginal_point_weights: this engine holds one shard of the catalog; the injection weights need the global set"),
    "marginal_weights": ((), "GWI_ERR_UNSUPPORTED: marginal_weights: this engine holds one shard of the catalog; the injection weights need the global set"),
    "set_quantile_columns": ((), "GWI_ERR_UNSUPPORTED: set_quantile_columns: this engine holds one shard of the catalog; the injection quantiles need the global set"),
    "weighted_quantiles": (([0.5],), "GWI_ERR_UNSUPPORTED: weighted_quantiles: this engine holds one shard of the catalog; the injection quantiles need the global set"),
    "set_kde_columns": ((), "GWI_ERR_UNSUPPORTED: set_kde_columns: this engine holds one shard of the catalog; the injection densities need the global set"),
    "weighted_kde": (([0.0],), "GWI_ERR_UNSUPPORTED: weighted_kde: this engine holds one shard of the catalog; the injection densities need the global set"),
    "weighted_kde2d": (([[0, 1]], [0.0], [0.0]), "GWI_ERR_UNSUPPORTED: weighted_kde2d: this engine holds one shard of the catalog; the injection densities need the global set"),
}


def _stub(world):
    eng = object.__new__(NativePopulationLikelihood)
    eng.world = world
    if world == 1:
        eng.n_theta, eng.n_ev, eng.n_pe, eng.n_inj = N_THETA, N_EV, N_PE, N_INJ
    return eng


@pytest.mark.parametrize("method", sorted(SHARD_REFUSALS))
def test_a_shard_is_refused_before_anything_else(method):
    args, text = SHARD_REFUSALS[method]
    with pytest.raises(N.NativeEngineError) as err:
        getattr(_stub(2), method)(*args)  # (only .world is set: nothing else is looked at first)
    assert str(err.value) == text


@pytest.mark.parametrize("method,args", [("log_weights", (TH,)), ("set_draw_mask", ())])
def test_the_two_wrappers_a_shard_may_use_do_not_refuse_it(method, args):
    """A shard has log-weights and may keep a mask (the library's gwi_set_draw_mask says so): these two go on to the engine, which
    the stub does not have."""
    with pytest.raises(AttributeError):
        getattr(_stub(2), method)(*args)


def _refused(call, text):
    with pytest.raises(ValueError) as err:
        call()
    assert str(err.value) == text


@pytest.mark.parametrize("method", ["weighted_histograms", "point_cdfs", "marginal_weights_add"])
def test_thetas_of_the_wrong_shape(method):
    eng = _stub(1)
    _refused(lambda: getattr(eng, method)(np.zeros((2, 4))), "thetas has shape (2, 4); expected (3,) or (k, 3)")
    _refused(lambda: getattr(eng, method)(np.zeros((1, 2, 3))), "thetas has shape (1, 2, 3); expected (3,) or (k, 3)")


@pytest.mark.parametrize("method", ["weighted_histograms", "point_cdfs"])
def test_no_point_is_refused_where_one_is_needed(method):
    _refused(lambda: getattr(_stub(1), method)(np.zeros((0, 3))), "thetas has shape (0, 3); expected (3,) or (k, 3)")


def test_no_point_is_accepted_by_marginal_weights_add():
    with pytest.raises(AttributeError):  # past the check: on to the engine, which the stub does not have
        _stub(1).marginal_weights_add(np.zeros((0, 3)))


@pytest.mark.parametrize("method,pe_name,inj_name", [("set_quantile_columns", "pe_values", "inj_values"), ("set_kde_columns", "pe_values", "inj_values"),
                                                     ("set_histogram_bins", "pe_bins", "inj_bins")])
def test_sets_of_the_wrong_shape_or_number_of_columns(method, pe_name, inj_name):
    eng = _stub(1)
    dt, more = (np.int32, {"n_bins": 4}) if method == "set_histogram_bins" else (np.float64, {})
    call = getattr(eng, method)
    _refused(lambda: call(**more), f"{pe_name} and {inj_name} are both None")
    _refused(lambda: call(np.zeros((1, N_EV, N_PE + 1), dtype=dt), **more), f"{pe_name} has shape (1, 2, 6); expected (n_cols, 2, 5)")
    _refused(lambda: call(np.zeros((N_EV, N_PE), dtype=dt), **more), f"{pe_name} has shape (2, 5); expected (n_cols, 2, 5)")
    _refused(lambda: call(None, np.zeros((1, N_INJ + 1), dtype=dt), **more), f"{inj_name} has shape (1, 8); expected (n_cols, 7)")
    _refused(lambda: call(np.zeros((1, N_EV, N_PE), dtype=dt), np.zeros((2, N_INJ), dtype=dt), **more), f"{pe_name} holds 1 columns, {inj_name} 2")


@pytest.mark.parametrize("method", ["set_quantile_columns", "set_kde_columns"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_values_that_are_not_finite(method, bad):
    eng = _stub(1)
    pe, inj = np.zeros((1, N_EV, N_PE)), np.zeros((1, N_INJ))
    pe[0, 1, 2] = inj[0, 3] = bad
    _refused(lambda: getattr(eng, method)(pe), "pe_values holds values that are not finite")
    _refused(lambda: getattr(eng, method)(None, inj), "inj_values holds values that are not finite")


def test_bin_codes_keep_their_integer_rules():
    eng = _stub(1)
    _refused(lambda: eng.set_histogram_bins(np.zeros((1, N_EV, N_PE), dtype=np.int32)), "n_bins is needed")
    _refused(lambda: eng.set_histogram_bins(np.zeros((1, N_EV, N_PE)), n_bins=4), "pe_bins holds float64, not integer bin codes")
    _refused(lambda: eng.set_histogram_bins(None, np.zeros((1, N_INJ), dtype=np.float32), n_bins=4), "inj_bins holds float32, not integer bin codes")
    _refused(lambda: eng.set_histogram_bins(np.full((1, N_EV, N_PE), -1), n_bins=4), "pe_bins holds codes outside 0 ... 0xFFFF")
    _refused(lambda: eng.set_histogram_bins(None, np.full((1, N_INJ), 0x10000), n_bins=4), "inj_bins holds codes outside 0 ... 0xFFFF")
    with pytest.raises(AttributeError):  # 0xFFFF is a code (outside every bin): on to the engine, which the stub does not have
        eng.set_histogram_bins(None, np.full((1, N_INJ), 0xFFFF), n_bins=4)
