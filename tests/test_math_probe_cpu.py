"""The fixture tests/golden/math_probe_hp.npz against a plain float64 emulation of the device maths primitives (tests/math_probe_util.py:
Emulation -- the arithmetic of gwinferno_amd/csrc/gwi_device.h line by line, every FMA rounded once), with the bars of
tests/test_gpu_math_probe.py.  No GPU: this is the evidence that the bars are attainable by the algorithms as written and that the
50-digit references lie inside them, and it reads the coefficients out of the header, so a typo in one fails here.

Worst figures of the emulation as error / bar (the device returned the same figures; profiles/math_probe/RESULTS.md has the table):
fast_exp 1.0 (one subnormal quantum, x = -716.4), fast_exp_shift 1.0 (|x| = 7e5: the reduction's 2.32e-17 |n| is the whole error),
fast_expm1 0.998 (x = 0.0587: 2.2e-13 relative), fast_rcp 0.5 ulp against 2, the taps 0.60 (4.4e-17 against 7.4e-17), wave_sum 0.009.

spline_value 0.56 (c = (1e6, 1e-6, 1e-6, 1e-6) at t = 0.42).  The inner taps and spline_value were rewritten to get there: as
2/3 - s^2 + s^3/2 the taps were at 1.5 to 1.8, and in powers of t the spline value was at 2e10 for that coefficient set.
"""
import math
import struct

import numpy as np
import pytest

import math_probe_util as M

INF = float("inf")


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


@pytest.fixture(scope="module")
def emu():
    return M.Emulation()


def report(name, err, bar, args):
    ratio, e, b, at = M.worst(np.asarray(err), np.asarray(bar), args)
    print(f"{name}: worst error / bar = {ratio:.3g} (error {e:.3g}, bar {b:.3g}) at {at!r}")
    return ratio


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_source_constants_are_the_ones_the_bars_were_derived_for():
    """The nine coefficients, ln 2 and log2 e of gwi_device.h, to the bit.  A change of one of them changes E_POLY, E_Q and LN2_ERR: the
    bars are re-derived (tools/exp_poly.py) and these values replaced together."""
    k = M.source_constants()
    want = ["0x1.ffffffffffcf2p-1", "0x1.ffffffffeed9ap-2", "0x1.55555555b4533p-3", "0x1.555555812238dp-5", "0x1.1111105df9b38p-7", "0x1.6c1636bb1305dp-10",
            "0x1.a01bcbe416d47p-13", "0x1.a1736dfc73862p-16", "0x1.70c9649cbc43ap-19"]
    assert [float(c).hex() for c in k["c"]] == want
    assert k["ln2"] == math.log(2.0) == M.LN2_D and k["log2e"] == M.LOG2E_D and k["rcp_floor"] == 1e-290
    e_poly, e_q = M.poly_errors()
    print(f"E_POLY = {e_poly:.3e}, E_Q = {e_q:.3e}")
    assert 1.0e-14 < e_poly < 1.7e-14 and abs(k["c"][0] - 1.0) <= e_q < 2.5e-13


def test_fast_exp(fx, emu):
    x, ref = fx["exp_x"], fx["exp_ref"]
    got = np.array([emu.fast_exp(v) for v in x])
    special = ~np.isfinite(ref) | (ref == 0)
    assert np.array_equal(got[special], ref[special])  # exactly 0 / +inf where the reference is (NaN -> 0 among them)
    bar = M.exp_bar(x) * np.abs(ref) + np.where(np.abs(ref) < 2.0**-1022, M.QUANTUM, 0.0)
    assert report("fast_exp", M.abs_error(got, ref), bar, x) <= 1.0


def test_fast_exp_shift(fx, emu):
    x, sh, ref = fx["exp_shift_x"], fx["exp_shift_shift"], fx["exp_shift_ref"]
    got = np.array([emu.fast_exp_shift(v, s) for v, s in zip(x, sh)])
    special = ~np.isfinite(ref) | (ref == 0)
    assert np.array_equal(got[special], ref[special])
    bar = M.exp_bar(x, -7e5, 7e5) * np.abs(ref) + np.where(np.abs(ref) < 2.0**-1022, M.QUANTUM, 0.0)
    assert report("fast_exp_shift", M.abs_error(got, ref), bar, x) <= 1.0


def test_fast_expm1(fx, emu):
    x, ref, lo = fx["expm1_x"], fx["expm1_ref"], fx["expm1_ref_lo"]
    got = np.array([emu.fast_expm1(v) for v in x])
    assert not np.any(np.isnan(got))  # the [709, 710] ladder included
    assert np.all(got[(x <= -40.0) | np.isnan(x)] == -1.0)
    assert np.all(got[ref == INF] == INF) and np.all(np.isfinite(got[np.isfinite(ref)]))
    bar = M.expm1_bar(x, ref) * np.abs(ref) + np.where(np.abs(ref) < 2.0**-1022, M.QUANTUM, 0.0)
    assert report("fast_expm1", M.abs_error(got, ref, lo), bar, x) <= 1.0


def test_fast_expm1_keeps_the_parent_bits_below_709_43(fx):
    """The repaired fast_expm1 (the power of two stops at 2^1023) against the arithmetic it replaces, fma(2^n, rq, 2^n - 1), and against what the parent
    build returned on an MI355X (expm1_parent_bits): the same bits for every x < 709.43, NaN before and a finite value now on
    [709.44, 709.78)."""
    x = fx["expm1_x"]
    new, old = M.Emulation(), M.Emulation(old_expm1=True)
    below = ~(x >= 709.43)
    a = np.array([bits(new.fast_expm1(v)) for v in x], dtype=np.uint64)
    b = np.array([bits(old.fast_expm1(v)) for v in x], dtype=np.uint64)
    assert np.array_equal(a[below], b[below])
    hole = (x >= 709.44) & (x < 709.78)
    assert hole.sum() >= 20 and np.all(np.isnan(b.view(np.float64)[hole])) and np.all(np.isfinite(a.view(np.float64)[hole]))
    assert "expm1_parent_bits" in fx, "the fixture lost the parent build's recording (tests/golden/make_math_probe_hp.py)"
    assert np.array_equal(fx["expm1_parent_bits"][below], a[below])
    assert np.all(np.isnan(fx["expm1_parent_bits"].view(np.float64)[hole]))


def test_fast_rcp(fx):
    """Two Newton steps from any seed good to 2^-20 hold 2 ulp (they hold 0.5 ulp + 2^-80) wherever x and 1/x are normal."""
    x, ref, lo = fx["rcp_x"], fx["rcp_ref"], fx["rcp_ref_lo"]
    dom = (np.abs(x) >= 2.0**-1022) & (np.abs(x) <= 2.0**1022)
    assert dom.sum() > 3000
    worst = 0.0
    for seed_error in (2.0**-20, -(2.0**-20), 3.1e-7, -7.7e-8, 0.0):
        got = np.array([M.Emulation.fast_rcp(v, seed_error) for v in x[dom]])
        ulps = M.abs_error(got, ref[dom], lo[dom]) / np.spacing(np.abs(ref[dom]))
        worst = max(worst, report(f"fast_rcp (seed error {seed_error:+.1e})", ulps, np.full(ulps.shape, 2.0), x[dom]))
    assert worst <= 1.0


def test_cubic_taps(fx):
    t, ref, lo = fx["taps_t"], fx["taps_ref"], fx["taps_ref_lo"]
    got = np.array([M.Emulation.cubic_taps(v) for v in t])
    bar = 4 * M.U * np.maximum(np.abs(ref), 1.0 / 6.0)
    assert report("cubic_taps", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0
    total = np.array([math.fsum(row) for row in got])
    assert np.max(np.abs(total - 1.0)) <= 4 * M.U
    assert all(abs(math.fsum(list(r) + list(l) + [-1.0])) <= 2.0**-70 for r, l in zip(ref, lo))  # the reference sums to 1 (one rounding of the exact sum)


def test_cubic_taps_weighted(fx):
    t, w, ref, lo = fx["taps_w_t"], fx["taps_w_w"], fx["taps_w_ref"], fx["taps_w_ref_lo"]
    got = np.array([M.Emulation.cubic_taps_weighted(a, b) for a, b in zip(t, w)])
    bar = 4 * M.U * np.maximum(np.abs(ref), np.abs(w)[:, None] / 6.0)
    assert report("cubic_taps_weighted", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0


def test_cubic_taps_hold_the_bound_of_the_algorithm_as_written(fx):
    """as tests/test_gpu_math_probe.py: a second count: 4 u (2/3) |w| for the inner taps, 8 u of their value for the outer ones"""
    E = M.Emulation
    for name, t, w, ref, lo in (("taps", fx["taps_t"], np.ones_like(fx["taps_t"]), fx["taps_ref"], fx["taps_ref_lo"]),
                                ("taps_w", fx["taps_w_t"], fx["taps_w_w"], fx["taps_w_ref"], fx["taps_w_ref_lo"])):
        got = np.array([E.cubic_taps(a) if name == "taps" else E.cubic_taps_weighted(a, b) for a, b in zip(t, w)])
        bar = M.U * np.stack([8 * np.abs(ref[:, 0]), 4 * np.abs(w) * (2.0 / 3.0), 4 * np.abs(w) * (2.0 / 3.0), 8 * np.abs(ref[:, 3])], axis=1) + M.QUANTUM
        assert report(f"{name} (own bound)", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0


SETS = ["equal", "alternating", "big_beside_small", "random"]


@pytest.mark.parametrize("which", range(4), ids=SETS)
def test_spline_value(fx, which):
    sel = fx["spline_set"] == which
    t, ref, lo, scale = fx["spline_t"][sel], fx["spline_ref"][sel], fx["spline_ref_lo"][sel], fx["spline_abs"][sel]
    c = fx["spline_coef_sets"][which]
    assert np.array_equal(fx["spline_c"][sel], np.tile(c, t.size // 4))
    got = np.array([M.Emulation.spline_value(c, v) for v in t])
    assert report(f"spline_value[{SETS[which]}]", M.abs_error(got, ref, lo), 8 * M.U * scale, t) <= 1.0


def test_locate_family(fx):
    E = M.Emulation
    got = [E.locate_term(u, int(nb)) for u, nb in zip(fx["locate_term_u"], fx["locate_term_n_basis"])]
    assert np.array_equal([g[0] for g in got], fx["locate_term_k"]) and np.array_equal([g[1] for g in got], fx["locate_term_t"])
    got = [E.locate(x, b[0], b[1], int(b[2])) for x, b in zip(fx["locate_x"], fx["locate_b"])]
    assert np.array_equal([g[0] for g in got], fx["locate_k"]) and np.array_equal([g[1] for g in got], fx["locate_t"])
    u, nb = fx["locate_knot_u"], fx["locate_knot_n_basis"]
    assert np.all((u >= 0) & (u < nb - 3))  # the documented domain only
    got = [E.locate_knot(v) for v in u]
    assert np.array_equal([g[0] for g in got], fx["locate_knot_k"]) and np.array_equal([g[1] for g in got], fx["locate_knot_t"])
    # the fixture visits every integer, both neighbours and the far ends of every basis size
    for n_b in (4, 5, 16, 17, 200):
        us = fx["locate_term_u"][fx["locate_term_n_basis"] == n_b]
        assert all(float(j) in us and np.nextafter(float(j), INF) in us and np.nextafter(float(j), -INF) in us for j in range(n_b - 2))
        assert INF in us and -INF in us and 1e300 in us


def test_binades_of(fx, emu):
    assert np.array_equal([emu.binades_of(m) for m in fx["binades_m"]], fx["binades_ref"])


def test_wave_reductions(fx):
    E = M.Emulation
    v, ref, n_exact = fx["wave_sum_v"], fx["wave_sum_ref"], int(fx["wave_sum_n_exact"])
    got = np.array([E.wave_sum(w) for w in v])
    assert np.array_equal(got[:n_exact], ref[:n_exact]) and ref[0] == 64.0 and np.all(ref[1:65] == 1.0) and ref[65] == 2.0**52 - 1
    assert report("wave_sum", np.abs(got - ref)[n_exact:], (64 * M.U * fx["wave_sum_abs"])[n_exact:], np.arange(n_exact, len(v))) <= 1.0
    assert np.array_equal([E.wave_max(w) for w in fx["wave_max_v"]], fx["wave_max_ref"])
    for key in ("wave_max_v", "wave_max_coarse_extra_v"):
        ws = fx[key]
        mx = np.max(ws, axis=1)
        got = np.array([E.wave_max_coarse(w) for w in ws])
        with np.errstate(invalid="ignore"):
            assert np.all(np.where(np.isinf(mx), got == mx, np.abs(got - mx) <= 2.0**-24 * np.abs(mx)))
    v8, ref8, n8 = fx["wave_sum8_v"], fx["wave_sum8_ref"], int(fx["wave_sum8_n_exact"])
    got = np.array([E.wave_sum8(w) for w in v8])  # [wave][lane]
    want = np.repeat(ref8, 8, axis=1)             # lanes 8k .. 8k + 7 hold the total of slot k
    assert np.array_equal(got[:n8], want[:n8])
    assert np.all(np.abs(got - want)[n8:] <= np.repeat(64 * M.U * fx["wave_sum8_abs"], 8, axis=1)[n8:])


def test_fixture_is_small_and_regenerates():
    """well under the 1 MiB limit of a committed file, and the generator reproduces the arrays it computes (at 50 and 100 digits)"""
    import importlib.util
    import os

    assert os.path.getsize(M.FIXTURE) < 512 * 1024
    spec = importlib.util.spec_from_file_location("make_math_probe_hp", os.path.join(M.ROOT, "tests", "golden", "make_math_probe_hp.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.mp.mp.dps = gen.DPS
    again = gen.compute()
    fx = M.fixture()
    assert set(again) | {"expm1_parent_bits"} == set(fx)
    assert all(gen.same(again[k], fx[k]) for k in again)
