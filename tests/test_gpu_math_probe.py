"""The device maths primitives of gwinferno_amd/csrc/gwi_device.h, each called on its own through gwi_math_probe (gwi_probe.h), against
the 50-digit references of tests/golden/math_probe_hp.npz.  The bars are derived in tests/math_probe_util.py (its docstring) from the
constants of the source and the number format; tests/test_math_probe_cpu.py holds a float64 emulation of the same algorithms to the same
bars.  Each test is one or two launches of a few thousand lanes.  Every figure is printed before it is asserted
(profiles/math_probe/RESULTS.md has the table).

Two primitives missed these bars when the tests were written, in the emulation and on the device alike, and were rewritten:
  * the inner taps, as 2/3 - s^2 + s^3/2, were 1.5 x (weighted: 1.8 x) the bar where they fall to 1/6; about their small end,
    1/6 + (s/2)(1 + t v), they are at 0.60 of it;
  * spline_value in powers of t was 2e10 x the bar for c = (1e6, 1e-6, 1e-6, 1e-6) near t = 1 (its error is proportional to max |c_i|);
    in Bernstein form it is at 0.56.
"""
import numpy as np
import pytest

import math_probe_util as M

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def report(name, err, bar, args):
    ratio, e, b, at = M.worst(np.asarray(err), np.asarray(bar), args)
    print(f"{name}: worst error / bar = {ratio:.3g} (error {e:.3g}, bar {b:.3g}) at {at!r}")
    return ratio


def run_twice(op, a, b=None):
    """the op's results, after checking that a second launch returns the same bits"""
    out, iout = M.probe(op, a, b)
    out2, iout2 = M.probe(op, a, b)
    assert out.tobytes() == out2.tobytes() and iout.tobytes() == iout2.tobytes(), f"{op}: two launches differ"
    return out, iout


def subnormal_quantum(ref):
    return np.where(np.abs(ref) < 2.0**-1022, M.QUANTUM, 0.0)


def test_fast_exp(fx):
    x, ref = fx["exp_x"], fx["exp_ref"]
    got = run_twice("exp", x)[0][:, 0]
    special = ~np.isfinite(ref) | (ref == 0)
    assert np.array_equal(got[special], ref[special])  # exactly 0 / +inf where the reference is; NaN -> 0 among them
    assert report("fast_exp", M.abs_error(got, ref), M.exp_bar(x) * np.abs(ref) + subnormal_quantum(ref), x) <= 1.0


def test_fast_exp_shift(fx):
    x, sh, ref = fx["exp_shift_x"], fx["exp_shift_shift"], fx["exp_shift_ref"]
    got = run_twice("exp_shift", x, sh)[0][:, 0]
    special = ~np.isfinite(ref) | (ref == 0)
    assert np.array_equal(got[special], ref[special])
    assert report("fast_exp_shift", M.abs_error(got, ref), M.exp_bar(x, -7e5, 7e5) * np.abs(ref) + subnormal_quantum(ref), x) <= 1.0


def test_fast_expm1(fx):
    x, ref, lo = fx["expm1_x"], fx["expm1_ref"], fx["expm1_ref_lo"]
    got = run_twice("expm1", x)[0][:, 0]
    assert not np.any(np.isnan(got))  # the [709, 710] ladder included
    assert np.all(got[(x <= -40.0) | np.isnan(x)] == -1.0)
    assert np.all(got[ref == INF] == INF) and np.all(np.isfinite(got[np.isfinite(ref)]))
    assert report("fast_expm1", M.abs_error(got, ref, lo), M.expm1_bar(x, ref) * np.abs(ref) + subnormal_quantum(ref), x) <= 1.0
    # every x below 709.43: the bits the parent build returned on an MI355X
    below = ~(x >= 709.43)
    assert np.array_equal(got.view(np.uint64)[below], fx["expm1_parent_bits"][below])


def test_fast_rcp(fx):
    """2 ulp wherever x and 1/x are normal, 2^-1022 <= |x| <= 2^1022; what comes back outside is printed, not held."""
    x, ref, lo = fx["rcp_x"], fx["rcp_ref"], fx["rcp_ref_lo"]
    got = run_twice("rcp", x)[0][:, 0]
    dom = (np.abs(x) >= 2.0**-1022) & (np.abs(x) <= 2.0**1022)
    for v, g, r in zip(x[~dom], got[~dom], ref[~dom]):
        print(f"fast_rcp outside its domain: x = {v!r}: {g!r} (1/x = {r!r})")
    ulps = M.abs_error(got[dom], ref[dom], lo[dom]) / np.spacing(np.abs(ref[dom]))
    assert report("fast_rcp [ulp]", ulps, np.full(ulps.shape, 2.0), x[dom]) <= 1.0


def test_cubic_taps(fx):
    t, ref, lo = fx["taps_t"], fx["taps_ref"], fx["taps_ref_lo"]
    got = run_twice("taps", t)[0]
    total = np.array([np.sum(row.astype(np.longdouble)) for row in got]).astype(np.float64)
    print(f"cubic_taps: largest |sum of the taps - 1| = {np.max(np.abs(total - 1.0)):.3g} (bar {4 * M.U:.3g})")
    assert np.max(np.abs(total - 1.0)) <= 4 * M.U
    bar = 4 * M.U * np.maximum(np.abs(ref), 1.0 / 6.0)
    assert report("cubic_taps", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0


def test_cubic_taps_weighted(fx):
    t, w, ref, lo = fx["taps_w_t"], fx["taps_w_w"], fx["taps_w_ref"], fx["taps_w_ref_lo"]
    got = run_twice("taps_w", t, w)[0]
    bar = 4 * M.U * np.maximum(np.abs(ref), np.abs(w)[:, None] / 6.0)
    assert report("cubic_taps_weighted", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0


def test_cubic_taps_hold_the_bound_of_the_algorithm_as_written(fx):
    """Beside the bar asked of the taps (above): a second count of the roundings of cubic_taps and cubic_taps_weighted.  The inner
    taps are sums of three addends of size at most 2/3 |w| with four roundings of at most u each of that size: 4 u (2/3) |w|; the outer
    ones are products, (w/6 s) s^2 with s = 1 - t rounded (u, entering three times), the rounded 1/6 and four products: 8 u of their value.  A swap of two taps, a wrong constant or a dropped term is off by a multiple of |w|."""
    for op, t, w, ref, lo in (("taps", fx["taps_t"], np.ones_like(fx["taps_t"]), fx["taps_ref"], fx["taps_ref_lo"]),
                              ("taps_w", fx["taps_w_t"], fx["taps_w_w"], fx["taps_w_ref"], fx["taps_w_ref_lo"])):
        got = M.probe(op, t, w)[0]
        bar = M.U * np.stack([8 * np.abs(ref[:, 0]), 4 * np.abs(w) * (2.0 / 3.0), 4 * np.abs(w) * (2.0 / 3.0), 8 * np.abs(ref[:, 3])], axis=1) + M.QUANTUM
        assert report(f"{op} (own bound)", M.abs_error(got, ref, lo).ravel(), bar.ravel(), np.repeat(t, 4)) <= 1.0


SETS = ["equal", "alternating", "big_beside_small", "random"]


@pytest.fixture(scope="module")
def spline_values(fx):
    return run_twice("spline", fx["spline_t"], fx["spline_c"])[0][:, 0]


@pytest.mark.parametrize("which", range(4), ids=SETS)
def test_spline_value(fx, spline_values, which):
    sel = fx["spline_set"] == which
    err = M.abs_error(spline_values[sel], fx["spline_ref"][sel], fx["spline_ref_lo"][sel])
    assert report(f"spline_value[{SETS[which]}]", err, 8 * M.U * fx["spline_abs"][sel], fx["spline_t"][sel]) <= 1.0


def test_locate_family(fx):
    u, nb = fx["locate_term_u"], fx["locate_term_n_basis"]
    out, k = run_twice("locate_term", u, np.stack([np.zeros_like(u), np.zeros_like(u), nb], axis=1))
    assert np.array_equal(k, fx["locate_term_k"]) and np.array_equal(out[:, 0], fx["locate_term_t"])
    for op in ("locate", "locate_x"):
        out, k = run_twice(op, fx["locate_x"], fx["locate_b"])
        assert np.array_equal(k, fx["locate_k"]) and np.array_equal(out[:, 0], fx["locate_t"]), op
    out, k = run_twice("locate_knot", fx["locate_knot_u"])
    assert np.array_equal(k, fx["locate_knot_k"]) and np.array_equal(out[:, 0], fx["locate_knot_t"])


def test_binades_of(fx):
    assert np.array_equal(run_twice("binades", fx["binades_m"])[1], fx["binades_ref"])


def per_wave(out):
    """[wave][lane] of slot 0, after checking that lane 0 and lane 63 (and every lane between) hold the same value"""
    lanes = out[:, 0].reshape(-1, 64)
    assert np.array_equal(lanes[:, 0], lanes[:, 63], equal_nan=True)
    assert all(np.array_equal(lanes[:, 0], lanes[:, j], equal_nan=True) for j in range(64))
    return lanes[:, 0]


def test_wave_sum(fx):
    v, ref, n_exact = fx["wave_sum_v"], fx["wave_sum_ref"], int(fx["wave_sum_n_exact"])
    got = per_wave(run_twice("wave_sum", v.ravel())[0])
    assert np.array_equal(got[:n_exact], ref[:n_exact])  # all ones -> 64, one-hot -> 1 at every lane, 2^lane: every lane counted once
    assert report("wave_sum", np.abs(got - ref)[n_exact:], (64 * M.U * fx["wave_sum_abs"])[n_exact:], np.arange(n_exact, len(v))) <= 1.0


def test_wave_max_and_coarse(fx):
    v, ref = fx["wave_max_v"], fx["wave_max_ref"]
    assert np.array_equal(per_wave(run_twice("wave_max", v.ravel())[0]), ref)
    assert np.array_equal(per_wave(run_twice("wave_max", fx["wave_max_coarse_extra_v"].ravel())[0]), fx["wave_max_coarse_extra_ref"])
    for ws in (v, fx["wave_max_coarse_extra_v"]):  # -inf, 0 and 2^-126 <= |v| <= 3.4e38: within one float32 rounding
        mx = np.max(ws, axis=1)
        got = per_wave(run_twice("wave_max_coarse", ws.ravel())[0])
        with np.errstate(invalid="ignore"):
            err = np.where(np.isinf(mx), np.where(got == mx, 0.0, INF), np.abs(got - mx))
        assert report("wave_max_coarse", err, 2.0**-24 * np.where(np.isinf(mx), 0.0, np.abs(mx)), np.arange(len(ws))) <= 1.0
    outside = fx["wave_max_coarse_outside_v"]
    got = per_wave(M.probe("wave_max_coarse", outside.ravel())[0])
    print(f"wave_max_coarse outside the float32 range (maxima {np.max(outside, axis=1)}): {got}")


def test_wave_sum8(fx):
    v, ref, n_exact = fx["wave_sum8_v"], fx["wave_sum8_ref"], int(fx["wave_sum8_n_exact"])
    got = run_twice("wave_sum8", v.ravel())[0][:, 0].reshape(-1, 64)
    want = np.repeat(ref, 8, axis=1)  # lanes 8k .. 8k + 7 hold the total of slot k: every one of the 64 lanes is checked
    assert np.array_equal(got[:n_exact], want[:n_exact])
    bar = np.repeat(64 * M.U * fx["wave_sum8_abs"], 8, axis=1)
    assert report("wave_sum8", np.abs(got - want)[n_exact:].ravel(), bar[n_exact:].ravel(), np.arange(got[n_exact:].size)) <= 1.0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, None])
def test_shapes(fx, n):
    """Lanes past n take no part: wave_sum over the first n lanes of all-ones is, wave by wave, the number of live lanes; wave_max of
    negative values is not raised by the padding; nothing is written past n."""
    n = fx["rcp_x"].size if n is None else n
    out, _ = M.probe("wave_sum", np.ones(n))
    want = np.minimum(64, n - (np.arange(n) // 64) * 64).astype(np.float64)
    assert np.array_equal(out[:, 0], want)
    out, _ = M.probe("wave_max", np.full(n, -3.0))
    assert np.all(out[:, 0] == -3.0)
    a = np.linspace(0.5, 2.0, n + 8)
    guard_out, guard_i = np.full((n + 8, 4), 7.25), np.full(n + 8, 77, dtype=np.int32)
    assert M.probe_raw(M.OPS["rcp"], n, a, np.zeros(n + 8), guard_out, guard_i) == 0
    assert np.all(guard_out[n:] == 7.25) and np.all(guard_i[n:] == 77)
    assert np.all(guard_out[:n, 1:] == 0.0) and np.all(guard_i[:n] == 0) and np.all(np.abs(guard_out[:n, 0] * a[:n] - 1.0) < 1e-15)


def test_refusals_write_nothing():
    a, b = np.ones(64), np.ones(64 * 3)
    out, iout = np.full((64, 4), 7.25), np.full(64, 77, dtype=np.int32)
    ok = M.OPS["exp"]
    for args in [(ok, 64, None, b, out, iout), (ok, 64, a, None, out, iout), (ok, 64, a, b, None, iout), (ok, 64, a, b, out, None), (ok, -1, a, b, out, iout),
                 (0, 64, a, b, out, iout), (17, 64, a, b, out, iout), (-3, 64, a, b, out, iout)]:
        assert M.probe_raw(*args) == -1, args[:2]  # GWI_ERR_INVALID
        assert np.all(out == 7.25) and np.all(iout == 77)
    assert M.probe_raw(ok, 0, a, b, out, iout) == 0 and np.all(out == 7.25) and np.all(iout == 77)  # n = 0: a successful no-op
    assert M.probe_raw(ok, 64, a, b, out, iout, device=10_000) == -2 and np.all(out == 7.25)        # GWI_ERR_NO_DEVICE
