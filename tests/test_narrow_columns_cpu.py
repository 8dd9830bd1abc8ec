"""CPU: the narrow-column plan (float32 spline coordinates in HBM, include/gwi_engine.h: GWI_TERM_EXP_SPLINE_F32).  Which spline
terms ``narrow_columns="auto"`` narrows on small bound models -- coordinates cast through float32 yes; float64 ones, log coordinates
and columns another term reads no -- that ``True`` refuses a column that does not qualify, that the constants of _native match the
header, and that gwi_create refuses a spec in which another term reads a narrow column (spec validation runs on host-only
handles too).  The GPU side is test_gpu_narrow_columns.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPINS = ("a_1", "a_2", "cos_tilt_1", "cos_tilt_2")


@pytest.fixture(scope="module")
def lib():
    from gwinferno_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return N.load_library()


def _catalog(cast=(), n_ev=3, n_pe=64, n_inj=400, seed=4):
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(n_ev, n_pe, n_inj, seed=seed)
    for k in cast:
        pe[k] = pe[k].astype(np.float32).astype(np.float64)
        inj[k] = inj[k].astype(np.float32).astype(np.float64)
    return pe, inj, total


def _bind(name, pe, inj, narrow):
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.engine import bind

    comp = COMPOSITIONS[name](pe, inj)
    p = comp.placeholder()
    return bind(comp.weights(p, True), comp.weights(p, False), comp.hypervolume(p), narrow_columns=narrow)


def test_constants_match_the_header():
    from gwinferno_amd import _native as N

    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"GWI_(TERM_[A-Z_0-9]+)\s*=\s*(\d+)", hdr))
    assert enum["TERM_EXP_SPLINE_F32"] == N.TERM_EXP_SPLINE_F32 == 15
    assert enum["TERM_LINEAR_SPLINE_F32"] == N.TERM_LINEAR_SPLINE_F32 == 16
    assert N.NARROW_KIND == {7: 15, 9: 16}
    assert "gwi_resident_bytes" in N.EXPORTED_SYMBOLS
    assert N.GWI_ABI_VERSION == 3


def test_auto_narrows_float32_spline_coordinates_and_nothing_else():
    from gwinferno_amd import _native as N

    # config 3/4: log m1 spline (a transformed coordinate, and read by the mass-ratio power law) stays wide; the four spins narrow
    bm = _bind("bspline_iid", *_catalog(SPINS)[:2], "auto")
    assert [t["kind"] for t in bm.terms] == [N.TERM_POWERLAW_RATIO, N.TERM_POWERLAW_REDSHIFT, 7, 15, 15, 15, 15]
    assert bm.narrowed == [3, 4, 5, 6]
    # config 5: the mass ratio too; the log m1 and log z splines stay wide, and the term order is the wide model's
    bm5 = _bind("bspline_full", *_catalog(SPINS + ("mass_ratio",))[:2], "auto")
    assert [t["kind"] for t in bm5.terms] == [N.TERM_POWERLAW_REDSHIFT, 7, 15, 15, 15, 15, 15, 7]
    # only the spins cast: the mass ratio, float64 numbers, stays wide
    bm5s = _bind("bspline_full", *_catalog(SPINS)[:2], "auto")
    assert [t["kind"] for t in bm5s.terms] == [N.TERM_POWERLAW_REDSHIFT, 7, 7, 15, 15, 15, 15, 7]
    # float64 spins: nothing; False: nothing
    assert _bind("bspline_iid", *_catalog()[:2], "auto").narrowed == []
    assert _bind("bspline_iid", *_catalog(SPINS)[:2], False).narrowed == []
    # one float64 value among the injections is enough to keep a column wide
    pe, inj, _ = _catalog(SPINS)
    inj["a_2"][17] = 0.1
    assert _bind("bspline_iid", pe, inj, "auto").narrowed == [3, 5, 6]


def test_parked_values_of_a_narrow_column_are_float32_numbers():
    """Excluded samples are parked at the spline's lower bound; config 5's mass ratio has lo = 5 / 100, not a float32 number: the
    narrow column parks them at the next float32 number inside the domain instead."""
    bm = _bind("bspline_full", *_catalog(SPINS + ("mass_ratio",), n_ev=6, n_pe=256)[:2], "auto")
    for ti in bm.narrowed:
        c = bm.terms[ti]["cols"][0]
        for side in ("pe", "inj"):
            v = np.asarray(bm.pe_cols[c] if side == "pe" else bm.inj_cols[c]).ravel()
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    q = bm.terms[bm.narrowed[0]]
    assert q["p"][0] == 0.05
    assert np.min(bm.pe_cols[q["cols"][0]]) >= 0.05 or np.min(bm.inj_cols[q["cols"][0]]) >= 0.05


def test_a_column_read_by_another_term_is_not_narrowed():
    from gwinferno_amd import _native as N
    from gwinferno_amd.engine import plan_narrow_columns

    bm = _bind("bspline_iid", *_catalog(SPINS)[:2], False)
    c = bm.terms[3]["cols"][0]
    bm.terms.append(dict(kind=N.TERM_TILT_MIXTURE, cols=[c], theta=[0, 1], n_basis=0, coef_off=0, flags=0, norm=-1, p=(), owner=None))
    assert plan_narrow_columns(bm, "auto") == [4, 5, 6]
    assert bm.terms[3]["kind"] == N.TERM_EXP_SPLINE


def test_true_raises_on_a_column_that_does_not_qualify():
    with pytest.raises(ValueError, match=r"narrow_columns=True: the coordinate column \d+ of spline term 2 is also read by term 0 \(kind 3\)"):
        _bind("bspline_iid", *_catalog(SPINS)[:2], True)  # log m1, which the mass-ratio power law reads too
    with pytest.raises(ValueError, match=r"narrow_columns=True: the coordinate column \d+ of spline term 1 is not a raw catalog array"):
        _bind("bspline_full", *_catalog(SPINS + ("mass_ratio",))[:2], True)  # log m1
    with pytest.raises(ValueError, match=r"spline term 0 holds posterior-sample values that do not survive a float32 round trip"):
        _tilts(_catalog(), True)  # float64 tilts
    with pytest.raises(ValueError, match="narrow_columns must be"):
        _bind("bspline_iid", *_catalog(SPINS)[:2], "yes")


def _tilts(catalog, narrow):
    from gwinferno_amd.engine import bind
    from gwinferno_amd.models import BSplineIIDSpinTilts

    pe, inj, _ = catalog
    tilts = BSplineIIDSpinTilts(8, pe["cos_tilt_1"], pe["cos_tilt_2"], inj["cos_tilt_1"], inj["cos_tilt_2"], normalize=True)
    c = np.zeros(8)
    return bind(tilts(c, pe_samples=True), tilts(c, pe_samples=False), narrow_columns=narrow)


def test_true_narrows_every_spline_term_of_a_qualifying_model():
    bm = _tilts(_catalog(SPINS), True)
    assert [t["kind"] for t in bm.terms] == [15, 15]


def _spec(kinds_cols, n_cols=3):
    from gwinferno_amd import _native as N

    s = N.GwiSpec()
    s.abi_version = N.GWI_ABI_VERSION
    s.n_cols, s.kappa_col, s.n_theta, s.n_terms, s.n_norms, s.vt_norm = n_cols, n_cols - 1, 16, len(kinds_cols), 0, -1
    for i, (kind, cols) in enumerate(kinds_cols):
        g = s.terms[i]
        g.kind = kind
        g.cols[0], g.cols[1] = (cols + [-1, -1])[:2]
        for k in range(4):
            g.theta[k] = k
        g.n_basis, g.coef_off, g.norm = 8, 4, -1
        g.p[0], g.p[1] = 0.0, 1.0
    return s


def _create(lib, spec):
    from gwinferno_amd import _native as N

    dummy = np.zeros(1)
    ptrs = (N._DP * spec.n_cols)(*[N.as_dp(dummy)] * spec.n_cols)
    h = C.c_void_p()
    st = lib.gwi_create(C.byref(spec), ptrs, 1, 1, ptrs, 1, N.DEVICE_HOST_ONLY, C.byref(h))
    msg = lib.gwi_last_error(h).decode() if h else ""
    if h:
        lib.gwi_destroy(h)
    return st, msg


def test_gwi_create_refuses_a_narrow_column_another_term_reads(lib):
    from gwinferno_amd import _native as N

    assert _create(lib, _spec([(15, [0]), (16, [1])]))[0] == 0
    assert _create(lib, _spec([(15, [0]), (15, [0])]))[0] == 0  # several narrow terms may share one
    for other, cols in ((N.TERM_TILT_MIXTURE, [0]), (N.TERM_EXP_SPLINE, [0]), (N.TERM_POWERLAW_RATIO, [1, 0])):
        st, msg = _create(lib, _spec([(15, [0]), (other, cols)]))
        assert st == -1 and "a narrow column may be read by narrow spline terms only" in msg and "term 0" in msg, (other, st, msg)
    st, msg = _create(lib, _spec([(16, [2])]))
    assert st == -1 and "kappa" in msg
    assert _create(lib, _spec([(17, [0])]))[0] == -1


def test_run_time_chains_rank_the_narrow_kinds_as_their_wide_twins(lib):
    from gwinferno_amd import _native as N

    with pytest.raises(N.NativeEngineError):
        N.jit_compile([15, 6], 2)  # 15 ranks as 7: not ascending
    with pytest.raises(N.NativeEngineError):
        N.jit_compile([6, 17], 2)  # not a term kind
