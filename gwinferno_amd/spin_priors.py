"""Effective spins and the sampling prior re-expressed in them: what ``gwi_effective_spins`` and ``gwi_chi_p_conditional_prior``
compute on the device (include/gwi_engine.h, gwinferno_amd/csrc/gwi_spinprior.h), under the reference's function names and argument
orders (preprocess/priors.py, preprocess/conversions.py).

``backend="host"`` is the NumPy statement of the semantics -- the same formulas, the same counter-based generator, the same slot and
attempt rule, the same KDE -- that the device kernels are held to (as :mod:`gwinferno_amd.draws` is for the index draws).  It is not
a fall-back: ``backend="device"`` raises when the library or the device is missing.

Closed forms (Callister, arXiv:2104.09508): every function is array-valued and broadcasts ``chi_eff`` / ``chi_p`` against ``q``; a value
exactly on a boundary between two cases of ``p(chi_eff | q)`` is the mean of the form at ``|chi_eff| +- 1e-6``, sample by sample.
NaN, or ``q <= 0``, gives NaN.  The device evaluates the closed forms at a sample's own ``chi_eff`` / ``chi_p``
(:func:`effective_spins`), which is what a catalog needs; the functions of a free ``chi_eff`` below are the host statement only.

The conditional prior ``p(chi_p | chi_eff, q)`` is the reference's Monte-Carlo / KDE estimator with a seeded Philox4x32-10 stream and
bounded rejection; its values are a pure function of ``(seed, first_index + position of the sample, ndraws, max_attempts)``."""
import numpy as np

from . import _native

# Li2(x) = x P(x) on [0, 1/2]: tools/li2_poly.py (degree 20), lowest degree first
LI2_COEFS = (
    1.0,
    0.24999999999999967,
    0.11111111111120708,
    0.062499999988869764,
    0.04000000068202435,
    0.027777752257025577,
    0.020408798911562887,
    0.015613853663483654,
    0.012488668267175072,
    0.00862164425198887,
    0.01843546916997321,
    -0.05121318921247027,
    0.26536320034856065,
    -0.8994807340933034,
    2.460643951558273,
    -5.138827887034316,
    8.154635504607475,
    -9.472072074700625,
    7.645711180855402,
    -3.8401006270449325,
    0.9196852539474791,
)
N_GRID = 50
BACKENDS = ("device", "host")


# ------------------------------------------------------------------------------------------------------------------------------
# conversions (preprocess/conversions.py)
# ------------------------------------------------------------------------------------------------------------------------------
def chieff_from_q_component_spins(q, a1, a2, ct1, ct2):
    """``(a1 ct1 + q a2 ct2) / (1 + q)`` (conversions.py:8-33)."""
    return (a1 * ct1 + q * a2 * ct2) / (1.0 + q)


def chip_from_q_component_spins(q, a1, a2, ct1, ct2, math=np):
    """``max(a1 sin t1, (3 + 4q) / (4 + 3q) q a2 sin t2)`` (conversions.py:36-62)."""
    sint1 = math.sqrt(1.0 - ct1**2)
    sint2 = math.sqrt(1.0 - ct2**2)
    return math.maximum(a1 * sint1, ((3.0 + 4.0 * q) / (4.0 + 3.0 * q)) * q * a2 * sint2)


def mu_var_from_alpha_beta(alpha, beta, xmax=1):
    """Mean and variance of a Beta distribution on ``[0, xmax]`` (conversions.py:65-85)."""
    total = alpha + beta
    return alpha / total * xmax, alpha * beta / (total**2 * (total + 1)) * xmax**2


def alpha_beta_from_mu_var(mu, var, xmax=1):
    """The Beta shape parameters of a mean and a variance on ``[0, xmax]`` (conversions.py:88-110); the arguments are not modified."""
    mu = mu / xmax
    var = var / xmax**2
    return (mu**2 * (1 - mu) - mu * var) / var, (mu * (1 - mu) ** 2 - (1 - mu) * var) / var


# ------------------------------------------------------------------------------------------------------------------------------
# Re Li2(x) for every real x
# ------------------------------------------------------------------------------------------------------------------------------
def _li2_core(x):
    p = np.full_like(x, LI2_COEFS[-1])
    for c in LI2_COEFS[-2::-1]:
        p = p * x + c
    return p * x


def _li2_unit(x):
    out = np.full_like(x, np.nan)
    one = x == 1.0
    out[one] = np.pi**2 / 6.0
    m = (x > 0.5) & ~one
    out[m] = np.pi**2 / 6.0 - np.log(x[m]) * np.log1p(-x[m]) - _li2_core(1.0 - x[m])  # reflection
    m = (x >= 0.0) & (x <= 0.5)
    out[m] = _li2_core(x[m])
    m = x < 0.0
    ell = np.log1p(-x[m])
    out[m] = -_li2_core(x[m] / (x[m] - 1.0)) - 0.5 * ell * ell  # Landen: x / (x - 1) in (0, 1/2]
    return out


def re_li2(x):
    """The real part of the dilogarithm for real ``x`` of any size (what ``np.real(scipy.special.spence(1 - x + 0j))`` is): inversion
    for ``|x| > 1``, reflection on ``(1/2, 1]``, Landen's map on ``[-1, 0)``, a polynomial on ``[0, 1/2]``."""
    x = np.asarray(x, dtype=np.float64)
    flat = np.atleast_1d(x).ravel()
    out = np.full_like(flat, np.nan)
    m = flat > 1.0
    ell = np.log(flat[m])
    out[m] = np.pi**2 / 3.0 - 0.5 * ell * ell - _li2_unit(1.0 / flat[m])
    m = flat < -1.0
    ell = np.log(-flat[m])
    out[m] = -np.pi**2 / 6.0 - 0.5 * ell * ell - _li2_unit(1.0 / flat[m])
    m = np.abs(flat) <= 1.0
    out[m] = _li2_unit(flat[m])
    return out.reshape(x.shape)


# ------------------------------------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------------------------------------
CASE_NAMES = ("zero", "A", "B", "C", "D", "E", "outside", "boundary")


def isotropic_case(chi_eff, q, a_max=1.0):
    """Which case of ``p(chi_eff | q)`` each sample takes: an index into :data:`CASE_NAMES` (7 = exactly on a boundary, or NaN)."""
    x, q = np.broadcast_arrays(np.abs(np.asarray(chi_eff, dtype=np.float64)), np.asarray(q, dtype=np.float64))
    A = a_max
    with np.errstate(invalid="ignore"):
        b1, b2, b3 = A * (1.0 - q) / (1.0 + q), q * A / (1.0 + q), A / (1.0 + q)
        conds = [x == 0.0, x >= A, (x > 0.0) & (x < b1) & (x < b2), (x < b1) & (x > b2), (x > b1) & (x < b2), (x > b1) & (x < b3) & (x >= b2), (x > b1) & (x > b3) & (x < A)]
    return np.select(conds, [0, 6, 1, 2, 3, 4, 5], default=7)


def _iso_open(x, q, A):
    """The form on flat arrays ``x = |chi_eff|`` and ``q``; also the mask of samples in no case.  Only the selected case of a sample is
    evaluated, so no logarithm or square root of a negative number is ever taken."""
    case = isotropic_case(x, q, A)
    out = np.zeros_like(x)
    m = case == 0
    out[m] = (1.0 + q[m]) / (2.0 * A) * (2.0 - np.log(q[m]))
    lA = np.log(A)
    for c in range(1, 6):
        m = case == c
        if not m.any():
            continue
        xc, qc = x[m], q[m]
        s, qA = (1.0 + qc) * xc, qc * A
        r = qA / s
        dl = re_li2(-r if c <= 2 else 1.0 - A / s) - re_li2(r)
        if c == 1:
            t = qA * (4.0 + 2.0 * lA - np.log(qA * qA - s * s)) - 2.0 * s * np.arctanh(s / qA)
        elif c == 2:
            t = 4.0 * qA + 2.0 * qA * lA - 2.0 * s * np.arctanh(r) - qA * np.log(s * s - qA * qA)
        elif c == 3:
            t = (2.0 * (1.0 + qc) * (A - xc) - s * lA * lA + (A + s * np.log(s)) * np.log(qA / (A - s)) - s * lA * (2.0 + np.log(qc) - np.log(A - s))
                 + qA * np.log(A / (qA - s)) + s * np.log((A - s) * (qA - s) / qc))
        elif c == 4:
            t = (-xc * lA * lA + 2.0 * (1.0 + qc) * (A - xc) + qA * np.log(A / (s - qA)) + A * np.log(qA / (A - s))
                 - xc * lA * (2.0 * (1.0 + qc) - np.log(s) - qc * np.log(s / A)) + s * np.log((s - qA) * (A - s) / qc) + s * np.log(A / s) * np.log((A - s) / qc))
        else:
            t = (2.0 * (1.0 + qc) * (A - xc) - s * lA * lA + lA * (A - 2.0 * s - s * np.log(qc / (s - A))) - A * np.log((s - A) / qc)
                 + s * np.log((s - A) * (s - qA) / qc) + s * np.log(s) * np.log(qA / (s - A)) - qA * np.log((s - qA) / A))
        out[m] = (1.0 + qc) / (4.0 * qc * A * A) * (t + s * dl)
    return out, case == 7


def _flat_pair(v, q):
    v, q = np.broadcast_arrays(np.asarray(v, dtype=np.float64), np.asarray(q, dtype=np.float64))
    return np.ravel(v).astype(np.float64), np.ravel(q).astype(np.float64), v.shape


def chi_effective_prior_from_isotropic_spins(chi_eff, q, a_max=1.0):
    """``p(chi_eff | q)`` for uniform, isotropic component spins below ``a_max`` (priors.py:79-196), array-valued in both arguments."""
    x, qf, shape = _flat_pair(chi_eff, q)
    x = np.abs(x)
    bad = ~(qf > 0.0) | np.isnan(x)
    out = np.full_like(x, np.nan)
    good = ~bad
    val, edge = _iso_open(x[good], qf[good], a_max)
    if edge.any():  # the reference's one-level fallback, each sample with its own q
        xe, qe = x[good][edge], qf[good][edge]
        total = np.zeros_like(xe)
        for moved in (xe + 1e-6, xe - 1e-6):
            v, inner = _iso_open(np.abs(moved), qe, a_max)
            v[inner] = np.nan
            total = total + v
        val[edge] = 0.5 * total
    out[good] = val
    return out.reshape(shape)


def chi_effective_prior_from_aligned_spins(chi_eff, q, a_max=1.0):
    """``p(chi_eff | q)`` for uniform, aligned component spins (priors.py:38-76)."""
    x, qf, shape = _flat_pair(chi_eff, q)
    A = a_max
    with np.errstate(invalid="ignore", divide="ignore"):
        b1 = A * (1.0 - qf) / (1.0 + qf)
        out = np.select(
            [(x > b1) & (x <= A), (x < -b1) & (x >= -A), (x >= -b1) & (x <= b1)],
            [(1.0 + qf) * (1.0 + qf) * (A - x) / (4.0 * qf * A * A), (1.0 + qf) * (1.0 + qf) * (A + x) / (4.0 * qf * A * A), (1.0 + qf) / (2.0 * A)],
            default=0.0,
        )
    out = np.where(~(qf > 0.0) | np.isnan(x), np.nan, out)
    return out.reshape(shape)


def chi_p_prior_from_isotropic_spins(chi_p, q, a_max=1.0):
    """``p(chi_p | q)`` for uniform, isotropic component spins (priors.py:199-244): zero from ``a_max`` on."""
    x, qf, shape = _flat_pair(chi_p, q)
    A = a_max
    out = np.full_like(x, np.nan)
    ok = (qf > 0.0) & ~np.isnan(x)
    f = (3.0 + 4.0 * qf) / (4.0 + 3.0 * qf)
    edge = qf * A * (3.0 + 4.0 * qf) / (4.0 + 3.0 * qf)
    out[ok & (x >= A)] = 0.0
    m = ok & (x >= edge) & (x < A)
    out[m] = 1.0 / A * np.arccos(x[m] / A)
    m = ok & (x < edge)
    xm, qm, fm = x[m], qf[m], f[m]
    with np.errstate(invalid="ignore"):  # (a negative chi_p below -a_max: NaN, as the form gives)
        u = (4.0 + 3.0 * qm) * xm / ((3.0 + 4.0 * qm) * qm * A)
        ac_u, ac_x = np.arccos(u), np.arccos(xm / A)
        first = ac_u * (A - np.sqrt(A * A - xm * xm) + xm * ac_x)
        second = ac_x * (A * qm * (3.0 + 4.0 * qm) / (4.0 + 3.0 * qm) - np.sqrt(A * A * (qm * qm) * (fm * fm) - xm * xm) + xm * ac_u)
    out[m] = 1.0 / (A * A * qm) * ((4.0 + 3.0 * qm) / (3.0 + 4.0 * qm)) * (first + second)
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of counters (uint64 arrays holding 32-bit words); returns four such arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _uniform53(hi, lo):
    return (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))).astype(np.float64) * 2.0**-53


def draw_uniforms(seed, index, slots, attempt):
    """The three uniforms ``(u_a1, u_a2, u_cost2)`` of attempt ``attempt`` of the draw slots ``slots`` of catalog sample ``index``."""
    slots = np.asarray(slots, dtype=np.uint64)
    seed, index = int(seed) & (2**64 - 1), int(index)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    i0 = np.full(slots.shape, index & 0xFFFFFFFF, dtype=np.uint64)
    i1 = np.full(slots.shape, (index >> 32) & 0xFFFFFFFF, dtype=np.uint64)
    t = np.asarray(attempt, dtype=np.uint64) * np.uint64(2)
    r0 = philox4x32_10(i0, i1, slots, t + np.zeros_like(slots), k0, k1)
    r1 = philox4x32_10(i0, i1, slots, t + np.ones_like(slots), k0, k1)
    return _uniform53(r0[0], r0[1]), _uniform53(r0[2], r0[3]), _uniform53(r1[0], r1[1])


def conditional_draws(chi_eff, q, a_max, ndraws, seed, index, max_attempts):
    """``(chi_p draws, weights)`` of one sample: slot ``d`` holds its first attempt with ``|cos t1| <= 1``; weight 0 = none."""
    x, w = np.zeros(ndraws), np.zeros(ndraws)
    todo = np.arange(ndraws)
    target, f = chi_eff * (1.0 + q), (3.0 + 4.0 * q) / (4.0 + 3.0 * q)
    for t in range(max_attempts):
        if todo.size == 0:
            break
        u0, u1, u2 = draw_uniforms(seed, index, todo, t)
        a1, a2, ct2 = u0 * a_max, u1 * a_max, 2.0 * u2 - 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            ct1 = (target - q * a2 * ct2) / a1
            keep = np.abs(ct1) <= 1.0
            ct1k, a1k, a2k, ct2k = ct1[keep], a1[keep], a2[keep], ct2[keep]
            x[todo[keep]] = np.maximum(a1k * np.sqrt(1.0 - ct1k * ct1k), f * q * a2k * np.sqrt(1.0 - ct2k * ct2k))
            w[todo[keep]] = (1.0 + q) / a1k
        todo = todo[~keep]
    return x, w


def max_chi_p(chi_eff, q, a_max=1.0):
    """The reference's largest ``chi_p`` compatible with ``(chi_eff, q)`` (priors.py:317-320, both branches as they stand)."""
    reach = (1.0 + q) * abs(chi_eff)
    if reach / q < a_max:
        return a_max
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(a_max * a_max - (reach - q) * (reach - q)))


def _conditional_one(chi_p, chi_eff, q, a_max, ndraws, seed, index, max_attempts):
    x, w = conditional_draws(chi_eff, q, a_max, ndraws, seed, index, max_attempts)
    live = w > 0.0
    filled = int(live.sum())
    if filled == 0 or np.isnan(chi_p):
        return np.nan, filled
    x, w = x[live], w[live]
    top = max_chi_p(chi_eff, q, a_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = x - 0.5 * top
        sw = w.sum()
        w2 = (w * w).sum() / (sw * sw)
        mean_c = (w * c).sum() / sw
        var = ((w * c * c).sum() / sw - mean_c * mean_c) / (1.0 - w2)  # weighted variance, scipy's 1 / (1 - sum w^2) correction
        factor = (1.0 / w2) ** -0.2                                      # Scott's factor n_eff^(-1/5)
        h2 = var * factor * factor
        grid = np.linspace(0.05 * top, 0.95 * top, N_GRID)
        vals = (w[None, :] * np.exp((grid[:, None] - x[None, :]) ** 2 * (-0.5 / h2))).sum(axis=1) / (sw * np.sqrt(2.0 * np.pi * h2))
        grid = np.concatenate([[0.0], grid, [top]])
        vals = np.concatenate([[0.0], vals, [0.0]])
        norm = np.sum(0.5 * (vals[1:] + vals[:-1]) * np.diff(grid))
        if np.isnan(top):
            return np.nan, filled
        return float(np.interp(chi_p, grid, vals / norm)), filled


def _device_conditional(chi_p, chi_eff, q, a_max, ndraws, seed, first_index, max_attempts, device):
    lib = _native.load_library()
    if not hasattr(lib, "gwi_chi_p_conditional_prior"):
        raise _native.NativeEngineError("this build of the engine has no gwi_chi_p_conditional_prior")
    n = chi_p.size
    p, acc = np.empty(n), np.empty(n, dtype=np.int32)
    import ctypes as C

    st = lib.gwi_chi_p_conditional_prior(n, _native.as_dp(chi_p), _native.as_dp(chi_eff), _native.as_dp(q), float(a_max), int(ndraws), int(max_attempts),
                                         int(seed) & (2**64 - 1), int(first_index), _native.as_dp(p), acc.ctypes.data_as(C.POINTER(C.c_int32)), int(device))
    if st != 0:
        raise _native.NativeEngineError(f"gwi_chi_p_conditional_prior: {_native.STATUS_NAMES.get(st, st)}")
    return p, acc


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, not {backend!r}")


def chi_p_prior_given_chi_eff_q(chi_p, chi_eff, q, a_max=1.0, ndraws=10000, bw_method="scott", *, seed=0, first_index=0, max_attempts=64, backend="device",
                                device=_native.DEVICE_CURRENT, return_accepted=False):
    """``p(chi_p | chi_eff, q)`` (priors.py:247-333), array-valued: the three arguments broadcast, and element ``k`` (C order) is catalog
    sample ``first_index + k`` of the stream ``seed``.  ``return_accepted`` adds the number of filled draw slots per sample."""
    if bw_method != "scott":
        raise NotImplementedError("only Scott's bandwidth rule is implemented")
    _check_backend(backend)
    if ndraws < 2 or max_attempts < 1 or first_index < 0:
        raise ValueError("ndraws >= 2, max_attempts >= 1 and first_index >= 0 are required")
    cp, ce, qq = np.broadcast_arrays(np.asarray(chi_p, dtype=np.float64), np.asarray(chi_eff, dtype=np.float64), np.asarray(q, dtype=np.float64))
    shape = cp.shape
    cp, ce, qq = (np.ascontiguousarray(v.ravel(), dtype=np.float64) for v in (cp, ce, qq))
    if backend == "device":
        p, acc = _device_conditional(cp, ce, qq, a_max, ndraws, seed, first_index, max_attempts, device)
    else:
        p, acc = np.empty(cp.size), np.empty(cp.size, dtype=np.int32)
        for k in range(cp.size):
            p[k], acc[k] = _conditional_one(float(cp[k]), float(ce[k]), float(qq[k]), a_max, ndraws, seed, first_index + k, max_attempts)
    p, acc = p.reshape(shape), acc.reshape(shape)
    return (p, acc) if return_accepted else p


def joint_prior_from_isotropic_spins(chi_p, chi_eff, q, a_max=1.0, **kwargs):
    """``p(chi_eff, chi_p | q) = p(chi_p | chi_eff, q) p(chi_eff | q)`` (priors.py:336-379); ``kwargs`` go to
    :func:`chi_p_prior_given_chi_eff_q`."""
    chi_p, chi_eff = np.atleast_1d(chi_p), np.atleast_1d(chi_eff)
    return chi_effective_prior_from_isotropic_spins(chi_eff, q, a_max=a_max) * chi_p_prior_given_chi_eff_q(chi_p, chi_eff, q, a_max=a_max, **kwargs)


# ------------------------------------------------------------------------------------------------------------------------------
# a component-spin catalog in one call: what gwi_effective_spins returns
# ------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("chi_eff", "chi_p", "p_chi_eff_iso", "p_chi_eff_aligned", "p_chi_p_iso")


def effective_spins(q, a1, a2, ct1, ct2, a_max=1.0, outputs=OUTPUTS, backend="device", device=_native.DEVICE_CURRENT):
    """``chi_eff``, ``chi_p`` and the closed-form priors at them for samples given by component spins: a dict with the requested
    ``outputs``, each shaped like the (broadcast) inputs.  float32 columns are widened.  A sample with a NaN, ``q <= 0`` or
    ``|cos tilt| > 1`` is NaN in every output."""
    _check_backend(backend)
    unknown = [o for o in outputs if o not in OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}")
    cols = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (q, a1, a2, ct1, ct2)))
    shape = cols[0].shape
    cols = [np.ascontiguousarray(c.ravel(), dtype=np.float64) for c in cols]
    n = cols[0].size
    if backend == "device":
        lib = _native.load_library()
        if not hasattr(lib, "gwi_effective_spins"):
            raise _native.NativeEngineError("this build of the engine has no gwi_effective_spins")
        res = {o: np.empty(n) for o in outputs}
        st = lib.gwi_effective_spins(n, *(_native.as_dp(c) for c in cols), float(a_max), *(_native.as_dp(res[o]) if o in res else None for o in OUTPUTS), int(device))
        if st != 0:
            raise _native.NativeEngineError(f"gwi_effective_spins: {_native.STATUS_NAMES.get(st, st)}")
        return {o: v.reshape(shape) for o, v in res.items()}
    qf, a1f, a2f, c1f, c2f = cols
    with np.errstate(invalid="ignore"):
        ok = (qf > 0.0) & np.isfinite(qf) & np.isfinite(a1f) & np.isfinite(a2f) & (np.abs(c1f) <= 1.0) & (np.abs(c2f) <= 1.0)
    chi_eff, chi_p = np.full(n, np.nan), np.full(n, np.nan)
    chi_eff[ok] = chieff_from_q_component_spins(qf[ok], a1f[ok], a2f[ok], c1f[ok], c2f[ok])
    chi_p[ok] = chip_from_q_component_spins(qf[ok], a1f[ok], a2f[ok], c1f[ok], c2f[ok])
    qn = np.where(ok, qf, np.nan)
    make = {
        "chi_eff": lambda: chi_eff,
        "chi_p": lambda: chi_p,
        "p_chi_eff_iso": lambda: chi_effective_prior_from_isotropic_spins(chi_eff, qn, a_max),
        "p_chi_eff_aligned": lambda: chi_effective_prior_from_aligned_spins(chi_eff, qn, a_max),
        "p_chi_p_iso": lambda: chi_p_prior_from_isotropic_spins(chi_p, qn, a_max),
    }
    return {o: make[o]().reshape(shape) for o in outputs}


def last_device_times():
    """``(total ms, longest single launch ms, launches)`` of this thread's last device call of either entry (HIP events)."""
    import ctypes as C

    lib = _native.load_library()
    total, longest, n = C.c_double(), C.c_double(), C.c_int32()
    lib.gwi_spin_prior_times(C.byref(total), C.byref(longest), C.byref(n))
    return total.value, longest.value, n.value
