"""CPU: what the evaluation entry points refuse, and in which words, on a host-only handle (device = -2) through the ctypes
binding.  Every single fault that can be reached without a device is pinned by its status code and its gwi_last_error text:
null handle / theta / options / records, k out of range, the max_variance_cut combination, a sharded entry without an exchange, an
*_end without its *_begin, a gradient under marginalize_selection through the caller-exchanged path, and the call whose only
fault is that the handle has no device.

A host-only handle carries no scan kernel, and the entries that launch one test for it together with their null arguments: they
answer GWI_ERR_INVALID without a message (SILENT below) before they look at anything else.  SILENT is checked as "the handle's
last error is still the one planted before the call"."""
import ctypes as C
import os

import numpy as np
import pytest

from gwinferno_amd import _native as N

INVALID, UNSUPPORTED = -1, -4
SILENT = None
K_MAX = 16  # a host-only handle keeps the default max_batch

ONE = ("h", "theta", "opt", "out", "grad", "out", "out", "out", "out")
BATCH = ("h", "theta", "k", "opt", "out", "grad", "out", "out", "out", "out")
BATCH_BEGIN = ("h", "theta", "k", "opt", "flag", "flag")
END = ("h", "out", "grad", "out", "out", "out", "out")
SIGNATURES = {
    "gwi_eval": ONE,
    "gwi_eval_begin": ("h", "theta", "opt", "flag"),
    "gwi_eval_end": END,
    "gwi_eval_batch": BATCH,
    "gwi_eval_batch_begin": BATCH_BEGIN,
    "gwi_eval_batch_end": END,
    "gwi_eval_sharded": ONE,
    "gwi_eval_batch_sharded": BATCH,
    "gwi_eval_batch_sharded_begin": BATCH_BEGIN,
    "gwi_eval_batch_sharded_end": END,
    "gwi_eval_partial": ("h", "theta", "out", "out", "out", "out"),
    "gwi_eval_batch_partial": ("h", "theta", "k", "out", "out", "out", "out"),
    "gwi_combine": ("h", "records", "n_ranks", "opt", "out", "grad", "out"),
    "gwi_combine_batch": ("h", "theta", "k", "records", "n_ranks", "opt", "out", "grad", "out"),
}
SHARDED = ("gwi_eval_sharded", "gwi_eval_batch_sharded", "gwi_eval_batch_sharded_begin")
COMBINES = ("gwi_combine", "gwi_combine_batch")

VARIANCE = "max_variance_cut requires marginalize_selection and min_neff_cut to be off (analysis.py:237-243)"
NO_EXCHANGE = "neither gwi_shm_comm_init nor gwi_comm_init has been called"
# the fault -> which slot it spoils (None: the arguments are all valid)
FAULTS = {
    "null handle": "h",
    "null theta": "theta",
    "null options": "opt",
    "null records": "records",
    "k = 0": "k",
    "k > max_batch": "k",
    "max_variance_cut with min_neff_cut": "opt",
    "gradient under marginalize_selection": "grad",
    "no exchange": None,
    "host-only": None,
    "end without begin": None,
}

EXPECTED = {
    # ---- the entries that launch: the missing scan kernel of a host-only handle answers for every fault but a null handle
    **{(e, f): (INVALID, SILENT) for e in ("gwi_eval", "gwi_eval_begin", "gwi_eval_partial") for f in ("null handle", "null theta", "host-only")},
    **{(e, f): (INVALID, SILENT) for e in ("gwi_eval", "gwi_eval_begin") for f in ("null options", "max_variance_cut with min_neff_cut")},
    **{(e, f): (INVALID, SILENT) for e in ("gwi_eval_batch", "gwi_eval_batch_begin", "gwi_eval_batch_partial")
       for f in ("null handle", "null theta", "k = 0", "k > max_batch", "host-only")},
    **{(e, f): (INVALID, SILENT) for e in ("gwi_eval_batch", "gwi_eval_batch_begin") for f in ("null options", "max_variance_cut with min_neff_cut")},
    **{("gwi_eval_sharded", f): (INVALID, SILENT) for f in ("null handle", "null theta", "null options", "max_variance_cut with min_neff_cut", "no exchange", "host-only")},
    **{(e, f): (INVALID, SILENT) for e in ("gwi_eval_batch_sharded", "gwi_eval_batch_sharded_begin")
       for f in ("null handle", "null theta", "null options", "k = 0", "k > max_batch", "max_variance_cut with min_neff_cut", "no exchange", "host-only")},
    # ---- the ends
    **{(e, "null handle"): (INVALID, SILENT) for e in ("gwi_eval_end", "gwi_eval_batch_end", "gwi_eval_batch_sharded_end")},
    ("gwi_eval_end", "end without begin"): (INVALID, "gwi_eval_end without gwi_eval_begin"),
    ("gwi_eval_batch_end", "end without begin"): (INVALID, "gwi_eval_batch_end without gwi_eval_batch_begin"),
    ("gwi_eval_batch_sharded_end", "end without begin"): (INVALID, "gwi_eval_batch_sharded_end without gwi_eval_batch_sharded_begin"),
    # ---- the caller-exchanged assembly needs no kernel and no device
    **{(e, f): (INVALID, SILENT) for e in COMBINES for f in ("null handle", "null records", "null options")},
    ("gwi_combine_batch", "null theta"): (INVALID, SILENT),
    ("gwi_combine_batch", "k = 0"): (INVALID, SILENT),
    **{(e, "max_variance_cut with min_neff_cut"): (INVALID, VARIANCE) for e in COMBINES},
    ("gwi_combine", "gradient under marginalize_selection"): (
        UNSUPPORTED,
        "gradient with marginalize_selection=True needs the squared-weight records, which the caller-exchanged path "
        "(gwi_eval_partial / gwi_combine) does not carry: use gwi_eval or gwi_eval_sharded",
    ),
    ("gwi_combine_batch", "gradient under marginalize_selection"): (
        UNSUPPORTED,
        "gradient with marginalize_selection=True needs the squared-weight records, which the caller-exchanged path "
        "(gwi_eval_batch_partial / gwi_combine_batch) does not carry: use gwi_eval_batch_sharded",
    ),
}


def applicable(entry, fault):
    sig = SIGNATURES[entry]
    if fault == "end without begin":
        return entry.endswith("_end")
    if entry.endswith("_end"):
        return fault == "null handle"
    if fault == "no exchange":
        return entry in SHARDED
    if fault == "host-only":
        return entry not in COMBINES  # (a valid gwi_combine on a host-only handle is no fault: it is what such handles are for)
    if fault == "k > max_batch":
        return "k" in sig and entry != "gwi_combine_batch"  # (the assembly takes any number of points)
    if fault == "gradient under marginalize_selection":
        return entry in COMBINES
    return FAULTS[fault] in sig


def test_every_reachable_fault_of_every_entry_is_pinned():
    assert {(e, f) for e in SIGNATURES for f in FAULTS if applicable(e, f)} == set(EXPECTED)


@pytest.fixture(scope="module")
def handles():
    """(lib, a host-only handle, one with a one-rank shared-memory exchange, n_theta, record length)"""
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, _ = make_catalog(5, 32, 200, seed=3)
    plain, sharded = (COMPOSITIONS["plpeak"](pe, inj).engine(device=N.DEVICE_HOST_ONLY) for _ in range(2))
    name = f"/gwi_refusals_{os.getpid()}".encode()
    assert plain.lib.gwi_shm_comm_init(sharded.handle, name, 0, 1) == 0
    yield plain.lib, plain.handle, sharded.handle, plain.n_theta, plain.partial_len
    plain.lib.gwi_shm_comm_unlink(name)
    sharded.close()
    plain.close()


@pytest.mark.parametrize("entry,fault", sorted(EXPECTED))
def test_single_fault_status_and_message(handles, entry, fault):
    lib, plain, sharded, n_theta, rec_len = handles
    h = sharded if (entry in SHARDED and fault != "no exchange") else plain
    opt = N.GwiOptions(n_obs=5.0, total_inj=200.0, marginalize_selection=0, min_neff_cut=0, max_variance_cut=0)
    theta, records, grad = np.zeros(K_MAX * n_theta), np.zeros(2 * K_MAX * rec_len), np.zeros(K_MAX * n_theta)
    slot = {"h": h, "theta": N.as_dp(theta), "opt": C.byref(opt), "records": N.as_dp(records), "n_ranks": 2, "k": 3, "flag": 0, "out": None, "grad": None}
    spoiled = FAULTS[fault]
    if fault == "k = 0":
        slot["k"] = 0
    elif fault == "k > max_batch":
        slot["k"] = K_MAX + 1
    elif fault == "max_variance_cut with min_neff_cut":
        opt.max_variance_cut = opt.min_neff_cut = 1
    elif fault == "gradient under marginalize_selection":
        opt.marginalize_selection = 1
        slot["grad"] = N.as_dp(grad)
    elif spoiled is not None:
        slot[spoiled] = None
    want_status, want_text = EXPECTED[(entry, fault)]
    # plant a known last error (another entry's) so that a call which writes none is told from one which does
    planter = "gwi_eval_batch_end" if entry != "gwi_eval_batch_end" else "gwi_eval_end"
    assert getattr(lib, planter)(h, *([None] * 6)) == INVALID
    planted = lib.gwi_last_error(h).decode()
    assert planted == f"{planter} without {planter[:-3]}begin"
    status = getattr(lib, entry)(*[slot[s] for s in SIGNATURES[entry]])
    text = lib.gwi_last_error(h).decode()
    print(f"{entry} [{fault}]: {N.STATUS_NAMES.get(status, status)} {text!r}")
    assert status == want_status
    assert text == (planted if want_text is SILENT else want_text)
