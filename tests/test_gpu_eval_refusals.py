"""GPU: the refusals of the evaluation entry points that need a handle with a scan kernel, so that test_eval_refusals_cpu.py cannot
reach them: the max_variance_cut text on the launching entries, the missing exchange, a count above max_batch under each entry's
name for it, and the busy refusal with the refused entry's name (gwi_eval_begin in its own words).  One fault per call; status and
gwi_last_error text are those the entries answered with before their preambles were folded."""
import ctypes as C
import os

import numpy as np
import pytest

from gwinferno_amd import _native as N
from test_eval_refusals_cpu import INVALID, K_MAX, NO_EXCHANGE, SHARDED, SIGNATURES, VARIANCE

pytestmark = pytest.mark.gpu

LAUNCHING = [e for e in SIGNATURES if not e.endswith("_end") and not e.startswith("gwi_combine")]
WITH_OPTIONS = [e for e in LAUNCHING if "opt" in SIGNATURES[e]]
TOO_MANY = {
    "gwi_eval_batch": "k_batch",
    "gwi_eval_batch_begin": "k_batch",
    "gwi_eval_batch_sharded": "k_batch",
    "gwi_eval_batch_sharded_begin": "k_batch",
    "gwi_eval_batch_partial": "k",
}
BUSY = "{who}: an evaluation begun with gwi_eval_begin has not been collected (gwi_eval_end)"
BUSY_TEXT = {
    "gwi_eval": "gwi_eval_begin: the previous evaluation of this handle has not been collected (gwi_eval_end)",
    "gwi_eval_begin": "gwi_eval_begin: the previous evaluation of this handle has not been collected (gwi_eval_end)",
    "gwi_eval_batch": BUSY.format(who="gwi_eval_batch_begin"),
    "gwi_eval_batch_begin": BUSY.format(who="gwi_eval_batch_begin"),
    "gwi_eval_sharded": BUSY.format(who="gwi_eval_sharded"),
    "gwi_eval_batch_sharded": BUSY.format(who="gwi_eval_batch_sharded_begin"),
    "gwi_eval_batch_sharded_begin": BUSY.format(who="gwi_eval_batch_sharded_begin"),
    "gwi_eval_partial": BUSY.format(who="gwi_eval_partial"),
    "gwi_eval_batch_partial": BUSY.format(who="gwi_eval_batch_partial"),
}


@pytest.fixture(scope="module")
def handles():
    """(lib, an engine on device 0, one with a one-rank shared-memory exchange, a point to evaluate)"""
    from gwinferno_amd.compositions import COMPOSITIONS, draw_params
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, _ = make_catalog(5, 32, 200, seed=3)
    comp = COMPOSITIONS["plpeak"](pe, inj)
    plain, sharded = (c.engine(device=0) for c in (comp, COMPOSITIONS["plpeak"](pe, inj)))
    name = f"/gwi_gpu_refusals_{os.getpid()}".encode()
    assert plain.lib.gwi_shm_comm_init(sharded.handle, name, 0, 1) == 0
    yield plain.lib, plain, sharded, N.f64(comp.theta(draw_params("plpeak", np.random.default_rng(3))))
    plain.lib.gwi_shm_comm_unlink(name)
    sharded.close()
    plain.close()


def call(lib, eng, entry, opt, k=3):
    """entry on eng with valid arguments but for what `opt` and `k` spoil; returns (status, last error)"""
    theta = np.zeros(K_MAX * eng.n_theta)
    slot = {"h": eng.handle, "theta": N.as_dp(theta), "opt": C.byref(opt), "k": k, "flag": 0, "out": None, "grad": None}
    status = getattr(lib, entry)(*[slot[s] for s in SIGNATURES[entry]])
    return status, lib.gwi_last_error(eng.handle).decode()


def options(**spoiled):
    return N.GwiOptions(**dict(dict(n_obs=5.0, total_inj=200.0, marginalize_selection=0, min_neff_cut=0, max_variance_cut=0), **spoiled))


@pytest.mark.parametrize("entry", WITH_OPTIONS)
def test_max_variance_cut_combination(handles, entry):
    lib, plain, sharded, _ = handles
    assert call(lib, sharded if entry in SHARDED else plain, entry, options(max_variance_cut=1, min_neff_cut=1)) == (INVALID, VARIANCE)


@pytest.mark.parametrize("entry", SHARDED)
def test_sharded_entry_without_exchange(handles, entry):
    lib, plain, _, _ = handles
    assert call(lib, plain, entry, options()) == (INVALID, NO_EXCHANGE)


@pytest.mark.parametrize("entry", sorted(TOO_MANY))
def test_count_above_max_batch(handles, entry):
    lib, plain, sharded, _ = handles
    want = f"{TOO_MANY[entry]} exceeds the engine's max_batch (GWI_MAX_BATCH, default 16)"
    assert call(lib, sharded if entry in SHARDED else plain, entry, options(), k=K_MAX + 1) == (INVALID, want)


@pytest.mark.parametrize("which", ["plain", "sharded"])
def test_busy_handle_names_the_refused_entry(handles, which):
    lib, plain, sharded, theta = handles
    eng = sharded if which == "sharded" else plain
    assert lib.gwi_eval_begin(eng.handle, N.as_dp(theta), C.byref(options()), 0) == 0
    try:
        for entry in LAUNCHING:
            if (entry in SHARDED) == (which == "sharded"):
                assert call(lib, eng, entry, options()) == (INVALID, BUSY_TEXT[entry]), entry
        assert (lib.gwi_log_weights(eng.handle, N.as_dp(theta), None, None), lib.gwi_last_error(eng.handle).decode()) == (INVALID, BUSY.format(who="gwi_log_weights"))
    finally:
        assert lib.gwi_eval_end(eng.handle, *([None] * 6)) == 0
