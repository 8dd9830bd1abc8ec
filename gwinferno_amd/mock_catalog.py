"""Mock catalogs: observed events with posterior samples, found injections and ``total_generated``, drawn FROM a population through a
written-down observation model, so that the ``prior`` columns are exact for the way the samples were made and the likelihood is
correct at the true hyper-parameters by construction ("Mock catalogs"; kernels: gwinferno_amd/csrc/gwi_mock.h, entries
``gwi_mock_observe`` / ``gwi_mock_posteriors``).

The observation model.  A source has C <= 8 coordinates; coordinate c has a transform T_c (identity or log), a noise scale sigma_c in
T-space and a support [lo_c, hi_c].  Data: ``d_c = T_c(x_c) + sigma_c n_c``.  Detection is a function of the data only:
``Mc = m1_d (1 + z_d) q_d^(3/5) / (1 + q_d)^(1/5)``, ``rho = rho_ref (Mc / Mc_ref)^(5/6) DL_ref / DL(z_d)``, found where the three
detector-frame quantities are positive and ``rho >= rho_th``.  The PE prior is flat in T_c(x_c) on the support, so the posterior is a
truncated normal in T-space, sampled by inverse CDF from one uniform per coordinate, and ``prior = prod_c |T_c'(x_c)| / (T_c(hi_c) -
T_c(lo_c))``.

``backend="device"`` runs the HIP kernels; ``backend="host"`` is their NumPy statement -- the same Philox counters, the same branch
rules, ``scipy.special.erfc`` / ``erfcinv`` standing for the device library's -- which the kernels are tested against.  It is not a
fall-back: without a device the device backend raises.

A value is a pure function of (inputs, seed, stream index, sample index, coordinate): reruns, and requests split through
``first_index`` / ``first_event``, give the same numbers.
"""
import ctypes as C

import numpy as np

from . import _native
from .spin_priors import _uniform53, philox4x32_10

BACKENDS = ("device", "host")
MAX_COORDS = 8
TAG_OBSERVE = 0x4D4F4B00    # counter word 3 of the data's Philox blocks, + the block number (gwi_mock.h: kTagObserve)
TAG_POSTERIOR = 0x4D4F4B10  # ... of the posterior samples' (kTagPosterior)
SQRT2, INV_SQRT2 = 1.4142135623730951, 0.7071067811865476
CHUNK = 4096                # true sources drawn and observed per step of make_mock_catalog: fixed, so a catalog does not depend on the hardware
MAX_CHUNKS = 4096
_M64 = 2**64 - 1


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, not {backend!r}")


class ObservationModel:
    """Names, transforms (``"identity"`` / ``"log"``), noise scales (T-space) and supports (natural units) of the coordinates, the
    names of the three coordinates detection reads, and the detection parameters: a source whose detector-frame chirp mass is
    ``mc_ref`` (solar masses) at luminosity distance ``dl_ref`` (Mpc) has SNR ``rho_ref``; found means ``rho >= rho_th``.
    Defaults: SNR 8 for a 25 solar-mass chirp mass at 2 Gpc, threshold 8."""

    def __init__(self, names, transforms, sigmas, lo, hi, roles=("mass_1", "mass_ratio", "redshift"), rho_ref=8.0, mc_ref=25.0, dl_ref=2000.0, rho_th=8.0):
        self.names = tuple(names)
        self.transforms = tuple(transforms)
        self.sigmas = np.ascontiguousarray(sigmas, dtype=np.float64)
        self.lo = np.ascontiguousarray(lo, dtype=np.float64)
        self.hi = np.ascontiguousarray(hi, dtype=np.float64)
        self.roles = tuple(roles)
        self.rho_ref, self.mc_ref, self.dl_ref, self.rho_th = float(rho_ref), float(mc_ref), float(dl_ref), float(rho_th)
        self._table = None
        n = len(self.names)
        if not (len(self.transforms) == self.sigmas.size == self.lo.size == self.hi.size == n):
            raise ValueError("names, transforms, sigmas, lo and hi must have one entry per coordinate")
        if any(t not in ("identity", "log") for t in self.transforms):
            raise ValueError("a transform is 'identity' or 'log'")

    @property
    def n_coords(self):
        return len(self.names)

    @property
    def is_log(self):
        return np.array([t == "log" for t in self.transforms], dtype=np.int32)

    def role_indices(self):
        """Positions of the (m1, q, z) coordinates; -1 where a role's name is not among the coordinates."""
        return tuple(self.names.index(r) if r in self.names else -1 for r in self.roles)

    def check(self, need_roles=False):
        """The refusals of the entry points, with their messages (gwi_engine.hip: mock_model)."""
        n = self.n_coords
        if n < 1 or n > MAX_COORDS:
            raise ValueError(f"n_coords = {n} outside 1 ... {MAX_COORDS}")
        for c in range(n):
            if not (self.sigmas[c] > 0.0 and self.sigmas[c] < np.inf):
                raise ValueError(f"coordinate {c}: sigma <= 0 or not finite")
            if not (self.hi[c] > self.lo[c] and self.hi[c] - self.lo[c] < np.inf):
                raise ValueError(f"coordinate {c}: hi <= lo (or a bound that is not finite)")
            if self.is_log[c] and not self.lo[c] > 0.0:
                raise ValueError(f"coordinate {c}: a log coordinate needs lo > 0")
        if need_roles:
            roles = self.role_indices()
            for name, r in zip(("m1", "q", "z"), roles):
                if r < 0:
                    raise ValueError(f"role index {name} = {r} out of range")
            if len(set(roles)) != 3:
                raise ValueError("the role indices m1, q, z must differ")
            for k, v in enumerate(self.detection):
                if not (v > 0.0 and v < np.inf):
                    raise ValueError(f"detection parameter {k} (rho_ref, mc_ref, dl_ref, rho_th) is not positive and finite")

    @property
    def detection(self):
        return np.array([self.rho_ref, self.mc_ref, self.dl_ref, self.rho_th])

    def t_bounds(self):
        """``(T(lo), T(hi), T(hi) - T(lo))`` as the entry points form them: log(lo), log(hi), log(hi / lo) for a log coordinate."""
        lg = self.is_log.astype(bool)
        with np.errstate(all="ignore"):
            return np.where(lg, np.log(self.lo), self.lo), np.where(lg, np.log(self.hi), self.hi), np.where(lg, np.log(self.hi / self.lo), self.hi - self.lo)

    def z_top(self):
        """The largest redshift the data can show: 9 sigma above the support's end (a 53-bit uniform gives |n| < 8.3)."""
        iz = self.role_indices()[2]
        t = self.t_bounds()[1][iz] + 9.0 * self.sigmas[iz]
        return float(np.exp(t) if self.is_log[iz] else t)

    def dl_table(self):
        """``(z, DL)``: the table ``cosmology.FlatLambdaCDM.z_to_DL`` interpolates in (Planck 2015 "LVK"), extended past :meth:`z_top`."""
        if self._table is None:
            from .cosmology import DEFAULT_DZ, PLANCK15_LVK_H0, PLANCK15_LVK_OMEGA_M, FlatLambdaCDM

            top = self.z_top() if self.role_indices()[2] >= 0 else 0.0
            top = top if np.isfinite(top) else 0.0  # (a model the entry point will refuse: any table does)
            cosmo = FlatLambdaCDM(PLANCK15_LVK_H0, PLANCK15_LVK_OMEGA_M, max_z=max(10.0, top + 3 * DEFAULT_DZ))
            self._table = (np.ascontiguousarray(cosmo.z), np.ascontiguousarray(cosmo.Dc * (1 + cosmo.z)))
        return self._table


def default_model(spins=False, sigma_logm=0.08, sigma_q=0.12, sigma_z=0.08, sigma_spin=0.25, mmin=2.0, mmax=100.0, zmax=1.9, **detection):
    """``mass_1`` (log), ``mass_ratio``, ``redshift`` and, with ``spins``, ``a_1, a_2, cos_tilt_1, cos_tilt_2`` on the supports the
    reference's catalogs use."""
    names, tr = ["mass_1", "mass_ratio", "redshift"], ["log", "identity", "identity"]
    sig, lo, hi = [sigma_logm, sigma_q, sigma_z], [mmin, mmin / mmax, 1e-3], [mmax, 1.0, zmax]
    if spins:
        names += ["a_1", "a_2", "cos_tilt_1", "cos_tilt_2"]
        tr += ["identity"] * 4
        sig += [sigma_spin] * 2 + [2 * sigma_spin] * 2
        lo += [0.0, 0.0, -1.0, -1.0]
        hi += [1.0, 1.0, 1.0, 1.0]
    return ObservationModel(names, tr, sig, lo, hi, **detection)


# ------------------------------------------------------------------------------------------------------------------------------
# the NumPy statement
# ------------------------------------------------------------------------------------------------------------------------------
def coordinate_uniforms(seed, index, sample, tag, n_coords):
    """``u[c]`` for every coordinate: Philox block ``c // 2`` with counter ``(index low, index high, sample, tag + c // 2)``, words
    0, 1 for an even and 2, 3 for an odd coordinate.  ``index`` and ``sample`` broadcast against each other."""
    seed = int(seed) & _M64
    index, sample = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    out = np.empty((n_coords,) + index.shape)
    for b in range((n_coords + 1) // 2):
        w = philox4x32_10(index & np.uint64(0xFFFFFFFF), index >> np.uint64(32), sample, np.full(index.shape, tag + b, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        out[2 * b] = _uniform53(w[0], w[1])
        if 2 * b + 1 < n_coords:
            out[2 * b + 1] = _uniform53(w[2], w[3])
    return out


def _special():
    import scipy.special as sp  # lazily, as catalog.py does

    return sp


def normal_from_uniform(u):
    """Standard normal from a uniform in [0, 1): both tails through ``erfcinv`` of an argument <= 1; ``u = 0`` is read as 2^-54."""
    sp = _special()
    u = np.where(u == 0.0, 2.0**-54, np.asarray(u, dtype=np.float64))
    low = u <= 0.5
    return np.where(low, -SQRT2 * sp.erfcinv(2.0 * np.where(low, u, 0.5)), SQRT2 * sp.erfcinv(2.0 * (1.0 - np.where(low, 0.5, u))))


def truncnorm_icdf(a, b, u):
    """The standardised truncated normal on ``[a, b]`` at the uniform ``u`` in the cancellation-free form (gwi_mock.h)."""
    sp = _special()
    a, b, u = (np.array(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, u))
    with np.errstate(all="ignore"):
        mirror = a > 0.0
        a, b, u = np.where(mirror, -b, a), np.where(mirror, -a, b), np.where(mirror, 1.0 - u, u)
        pa = 0.5 * sp.erfc(-a * INV_SQRT2)
        tail = b <= 0.0
        pb = 0.5 * sp.erfc(-np.where(tail, b, 0.0) * INV_SQRT2)
        y_tail = -SQRT2 * sp.erfcinv(np.minimum(2.0 * (pa + u * (pb - pa)), 1.0))
        qb = 0.5 * sp.erfc(np.where(tail, 0.0, b) * INV_SQRT2)
        z = 1.0 - pa - qb
        lower = 2.0 * (pa + u * z)
        y_low = -SQRT2 * sp.erfcinv(np.minimum(lower, 1.0))
        y_up = SQRT2 * sp.erfcinv(np.minimum(2.0 * (qb + (1.0 - u) * z), 1.0))
        y = np.where(tail, y_tail, np.where(lower <= 1.0, y_low, y_up))
        y = np.where(np.isnan(y), y, np.minimum(np.maximum(y, a), b))
        return np.where(mirror, -y, y)


def interp_table(tz, tv, z):
    """``numpy.interp``'s form, cell by cell: ``(v1 - v0) / (z1 - z0) * (z - z0) + v0`` with ``tz[a] <= z`` (gwi_mock.h: interp_table)."""
    a = np.clip(np.searchsorted(tz, z, side="right") - 1, 0, tz.size - 2)
    return (tv[a + 1] - tv[a]) / (tz[a + 1] - tz[a]) * (z - tz[a]) + tv[a]


def _host_observe(x_true, model, seed, first_index):
    n = x_true.shape[1]
    lg = model.is_log.astype(bool)
    u = coordinate_uniforms(seed, np.arange(n, dtype=np.uint64) + np.uint64(int(first_index) & _M64), 0, TAG_OBSERVE, model.n_coords)
    with np.errstate(all="ignore"):
        t = np.where(lg[:, None], np.log(x_true), x_true)
        d = t + model.sigmas[:, None] * normal_from_uniform(u)
        nat = np.where(lg[:, None], np.exp(d), d)
        im, iq, iz = model.role_indices()
        m1, q, z = nat[im], nat[iq], nat[iz]
        tz, tv = model.dl_table()
        nan = np.isnan(m1) | np.isnan(q) | np.isnan(z)
        ok = ~nan & (m1 > 0.0) & (q > 0.0) & (z > 0.0) & (z <= tz[-1]) & (m1 < np.inf) & (q < np.inf)
        zz, qq, mm = np.where(ok, z, 1.0), np.where(ok, q, 1.0), np.where(ok, m1, 1.0)
        mc = mm * (1.0 + zz) * np.power(qq, 0.6) / np.power(1.0 + qq, 0.2)
        rho = model.rho_ref * np.power(mc / model.mc_ref, 5.0 / 6.0) * model.dl_ref / interp_table(tz, tv, zz)
        rho = np.where(ok, rho, np.where(nan, np.nan, 0.0))
        return d, rho, rho >= model.rho_th


def _host_posteriors(data, model, n_pe, seed, first_event):
    n_ev = data.shape[1]
    lg = model.is_log.astype(bool)
    t_lo, t_hi, width = model.t_bounds()
    idx = (np.arange(n_ev, dtype=np.uint64) + np.uint64(int(first_event) & _M64))[:, None]
    u = coordinate_uniforms(seed, idx, np.arange(n_pe, dtype=np.uint64)[None, :], TAG_POSTERIOR, model.n_coords)
    sh = (model.n_coords, 1, 1)
    d, sg = data[:, :, None], model.sigmas.reshape(sh)
    with np.errstate(all="ignore"):
        fin = np.isfinite(d)
        dd = np.where(fin, d, 0.0)
        y = truncnorm_icdf((t_lo.reshape(sh) - dd) / sg, (t_hi.reshape(sh) - dd) / sg, u)
        t = np.minimum(np.maximum(dd + sg * y, t_lo.reshape(sh)), t_hi.reshape(sh))
        x = np.minimum(np.maximum(np.where(lg.reshape(sh), np.exp(t), t), model.lo.reshape(sh)), model.hi.reshape(sh))
        x = np.where(fin, x, np.nan)
    return x, pe_prior(x, model)


def pe_prior(samples, model):
    """The ``prior`` column in NumPy: ``prod_c |T_c'(x_c)| / (T_c(hi_c) - T_c(lo_c))`` -- ``1 / (x ln(hi / lo))`` for a log coordinate,
    ``1 / (hi - lo)`` for an identity one -- multiplied in coordinate order.  ``samples``: ``(C, ...)`` or a dict by coordinate name."""
    if isinstance(samples, dict):
        samples = np.stack([np.asarray(samples[k], dtype=np.float64) for k in model.names])
    width = model.t_bounds()[2]
    out = np.ones(samples.shape[1:])
    with np.errstate(all="ignore"):
        for c in range(model.n_coords):
            out = out * (1.0 / (samples[c] * width[c]) if model.is_log[c] else np.where(np.isnan(samples[c]), np.nan, 1.0 / width[c]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the device
# ------------------------------------------------------------------------------------------------------------------------------
_IP = C.POINTER(C.c_int32)


def _lib():
    lib = _native.load_library()
    if not hasattr(lib, "gwi_mock_observe"):
        raise _native.NativeEngineError("this build of the engine has no gwi_mock_observe")
    return lib


def _raise(lib, where, st):
    raise _native.NativeEngineError(f"{where}: {_native.STATUS_NAMES.get(st, st)} {lib.gwi_mock_error().decode()}".rstrip())


def _device_observe(x_true, model, seed, first_index, device):
    lib = _lib()
    n = x_true.shape[1]
    tz, tv = model.dl_table()
    im, iq, iz = model.role_indices()
    is_log, det = model.is_log, model.detection
    d, snr, found = np.empty_like(x_true), np.empty(n), np.empty(n, dtype=np.uint8)
    st = lib.gwi_mock_observe(int(device), model.n_coords, is_log.ctypes.data_as(_IP), _native.as_dp(model.sigmas), _native.as_dp(model.lo), _native.as_dp(model.hi), im, iq, iz,
                              _native.as_dp(det), tz.size, _native.as_dp(tz), _native.as_dp(tv), n, _native.as_dp(x_true), int(seed) & _M64, int(first_index) & _M64,
                              _native.as_dp(d), _native.as_dp(snr), found.ctypes.data_as(C.POINTER(C.c_uint8)))
    if st != 0:
        _raise(lib, "gwi_mock_observe", st)
    return d, snr, found.astype(bool)


def _device_posteriors(data, model, n_pe, seed, first_event, device):
    lib = _lib()
    n_ev = data.shape[1]
    is_log = model.is_log
    x, prior = np.empty((model.n_coords, n_ev, n_pe)), np.empty((n_ev, n_pe))
    st = lib.gwi_mock_posteriors(int(device), model.n_coords, is_log.ctypes.data_as(_IP), _native.as_dp(model.sigmas), _native.as_dp(model.lo), _native.as_dp(model.hi), n_ev,
                                 int(n_pe), _native.as_dp(data), int(seed) & _M64, int(first_event) & _M64, _native.as_dp(x), _native.as_dp(prior))
    if st != 0:
        _raise(lib, "gwi_mock_posteriors", st)
    return x, prior


def last_device_times():
    """DIAGNOSTIC: device time of this thread's last device-backend call -- ``(observe ms, posterior ms, launches)``."""
    lib = _lib()
    a, b, n = C.c_double(), C.c_double(), C.c_int32()
    lib.gwi_mock_times(C.byref(a), C.byref(b), C.byref(n))
    return a.value, b.value, n.value


# ------------------------------------------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------------------------------------------
def _coords(x, model):
    if isinstance(x, dict):
        x = np.stack([np.asarray(x[k], dtype=np.float64) for k in model.names])
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != model.n_coords:
        raise ValueError(f"expected ({model.n_coords}, n) values or a dict with the keys {model.names}")
    return x


def observe(x_true, model, seed, first_index=0, backend="device", device=_native.DEVICE_CURRENT):
    """Observe the true sources ``x_true`` (``(C, n)`` in natural units, or a dict by coordinate name): returns ``(data (C, n) in
    T-space, snr (n,), found (n,) bool)``.  Source ``j`` has stream index ``first_index + j``.  NaN true parameters give NaN data
    and ``found = False``."""
    _check_backend(backend)
    if backend == "host":
        model.check(need_roles=True)
    x = _coords(x_true, model)
    if int(first_index) < 0:
        raise ValueError("first_index >= 0 is required")
    if backend == "host":
        return _host_observe(x, model, seed, first_index)
    return _device_observe(x, model, seed, first_index, device)


def posterior_samples(data, model, n_pe, seed, first_event=0, backend="device", device=_native.DEVICE_CURRENT):
    """``n_pe`` posterior samples of every event from its data ``(C, n_ev)``: a dict of ``(n_ev, n_pe)`` arrays by coordinate name
    plus ``prior``.  Event ``e`` has stream index ``first_event + e``."""
    _check_backend(backend)
    if backend == "host":
        model.check()
    data = _coords(data, model)
    if int(n_pe) < 0 or int(first_event) < 0:
        raise ValueError("n_pe >= 0 and first_event >= 0 are required")
    x, prior = (_host_posteriors(data, model, int(n_pe), seed, first_event) if backend == "host" else _device_posteriors(data, model, int(n_pe), seed, first_event, device))
    out = {k: x[c] for c, k in enumerate(model.names)}
    out["prior"] = prior
    return out


def found_injections(x_true, draw_density, model, seed, first_index=0, backend="device", device=_native.DEVICE_CURRENT):
    """Observe the injections ``x_true`` (true sources with the known draw density ``draw_density (n,)``): the found ones keep
    their TRUE parameters and that density as ``prior``.  Returns ``(injdict, total_generated)``, ``total_generated`` the number
    observed."""
    x = _coords(x_true, model)
    _, snr, found = observe(x, model, seed, first_index=first_index, backend=backend, device=device)
    inj = {k: np.ascontiguousarray(x[c][found]) for c, k in enumerate(model.names)}
    inj["prior"] = np.ascontiguousarray(np.asarray(draw_density, dtype=np.float64)[found])
    inj["snr"] = snr[found]
    return inj, int(x.shape[1])


def sub_seed(seed, k):
    """The key of stage ``k`` of a catalog (true sources, their observation, the samples, the injections ...).  The multiplier is not
    ``population_draws.factor_seed``'s: ``seed + k G`` there would hand the mass-ratio factor and the next stage the same stream."""
    return (int(seed) + (int(k) + 1) * 0xD1B54A32D192ED03) & _M64


def table_density(lo, hi, pdf, x):
    """The normalised density at ``x`` of the piecewise-linear table ``population_draws.table_draws`` draws from: the interpolant
    over the sum of the trapezoid cell masses."""
    pdf = np.asarray(pdf, dtype=np.float64)
    grid = np.linspace(lo, hi, pdf.size)
    total = np.sum(0.5 * (pdf[:-1] + pdf[1:])) * ((hi - lo) / (pdf.size - 1))
    return np.where((x >= lo) & (x <= hi), np.interp(x, grid, pdf), 0.0) / total


def plpeak_population(alpha, beta, mpp, sigpp, lam, lamb, mmin=5.0, mmax=100.0, zmin=1e-3, zmax=1.9, mass_curves=None, spin_curves=None):
    """PL+Peak x PL q x PL z as the curves :func:`make_mock_catalog` draws from.  ``mass_curves = (ms, m_pdf, qs, q_pdf)`` replaces
    ``population_draws.powerlaw_peak_factor_curves`` (which evaluates the mass curve on the device)."""
    from .cosmology import planck15_lvk
    from .population_draws import powerlaw_peak_factor_curves

    if mass_curves is None:
        ms, m_pdfs, qs, q_pdfs = powerlaw_peak_factor_curves(alpha, beta, mpp, sigpp, lam, mmin, mmax)
        mass_curves = (ms, m_pdfs[0], qs, q_pdfs[0])
    zs = np.linspace(zmin, zmax, 1000)
    return {"mass_curves": mass_curves, "mmin": float(mmin), "thin": False, "z_curve": (zs, planck15_lvk().dVc_dz(zs) * (1.0 + zs) ** (lamb - 1.0)), "spin_curves": spin_curves or {},
            "theta": {"alpha": alpha, "beta": beta, "mpp": mpp, "sigpp": sigpp, "lam": lam, "lamb": lamb}}


def bspline_population(m_cs, q_cs, nspline_dict, lamb, mmin=5.0, mmax=100.0, zmin=1e-3, zmax=1.9, mass_curves=None, spin_curves=None):
    """``models.BSplinePrimaryBSplineRatio`` x PL z: the product of the two spline curves under the mask ``q >= mmin / m1``, thinned."""
    from .population_draws import bspline_factor_curves

    pop = plpeak_population(None, None, None, None, None, lamb, mmin, mmax, zmin, zmax, mass_curves=mass_curves or tuple(
        c[0] if np.ndim(c) == 2 else c for c in bspline_factor_curves(m_cs, q_cs, nspline_dict, mmin, mmax)), spin_curves=spin_curves)
    pop.update(thin=True, theta={"m1_coefs": m_cs, "q_coefs": q_cs, "lamb": lamb})
    return pop


def draw_true_sources(population, names, n, seed, first_index, backend="device", device=_native.DEVICE_CURRENT):
    """``n`` sources with stream indices ``first_index ...`` from the population's curves: ``(x (C, n), keep (n,))`` -- ``keep``
    all True unless the mass model is a thinned product."""
    from .population_draws import draw_from_curves, draw_product_masses

    ms, m_pdf, qs, q_pdf = population["mass_curves"]
    kw = dict(first_index=first_index, backend=backend, device=device)
    mass = draw_product_masses(ms, np.atleast_2d(m_pdf), qs, np.atleast_2d(q_pdf), population["mmin"], n, sub_seed(seed, 0), bool(population["thin"]), **kw)
    cols = {"mass_1": mass["mass_1"][0], "mass_ratio": mass["mass_ratio"][0]}
    zs, z_pdf = population["z_curve"]
    cols["redshift"] = draw_from_curves(zs, z_pdf, n, sub_seed(seed, 1), **kw)[0]
    for k, (name, (grid, pdf)) in enumerate(sorted(population["spin_curves"].items())):
        cols[name] = draw_from_curves(grid, pdf, n, sub_seed(seed, 16 + k), **kw)[0]
    missing = [k for k in names if k not in cols]
    if missing:
        raise ValueError(f"the population has no curve for {missing}")
    keep = mass["accept"][0] if population["thin"] else np.ones(n, dtype=bool)
    return np.stack([cols[k] for k in names]), keep


def make_mock_catalog(population, injection_tables, model, n_ev, n_pe, n_generated, seed, backend="device", device=_native.DEVICE_CURRENT, max_chunks=MAX_CHUNKS):
    """A catalog drawn from ``population`` (:func:`plpeak_population`, :func:`bspline_population`) through ``model``.

    True sources are drawn (``population_draws``) and observed in chunks of ``CHUNK`` until ``n_ev`` are found -- at most
    ``max_chunks`` chunks, else a RuntimeError names the detected fraction -- and the first ``n_ev`` found are kept; each gets ``n_pe``
    posterior samples.  Injections: ``n_generated`` draws from ``injection_tables[name] = (lo, hi, pdf)`` (broad piecewise-linear
    tables, one per coordinate, independent), observed the same way; their ``prior`` is the product of the tables' normalised
    densities, exactly the density the draws have.

    Returns ``(pedict, injdict, total_generated, truth)``; ``truth`` holds the events' true parameters (by name), ``data``, ``snr``,
    the number of sources drawn and ``theta``.  The first three go into ``models`` / ``likelihood.hierarchical_likelihood`` and
    ``Engine`` unchanged."""
    from .population_draws import table_draws

    _check_backend(backend)
    model.check(need_roles=True)
    n_ev, n_pe, n_generated = int(n_ev), int(n_pe), int(n_generated)
    kw = dict(backend=backend, device=device)
    xs, ds, snrs, n_found, n_seen, n_drawn = [], [], [], 0, 0, 0
    for chunk in range(int(max_chunks)):
        if n_found >= n_ev:
            break
        x, keep = draw_true_sources(population, model.names, CHUNK, seed, chunk * CHUNK, **kw)
        d, snr, found = observe(x, model, sub_seed(seed, 2), first_index=chunk * CHUNK, **kw)
        found &= keep
        xs.append(x[:, found])
        ds.append(d[:, found])
        snrs.append(snr[found])
        n_found += int(found.sum())
        n_seen += int(keep.sum())
        n_drawn += CHUNK
    if n_found < n_ev:
        raise RuntimeError(f"make_mock_catalog: {n_found} of {n_ev} events found after {max_chunks} chunks of {CHUNK} sources "
                           f"(detected fraction {n_found / max(n_seen, 1):.3g}); loosen the detection parameters or raise max_chunks")
    x_ev, d_ev, snr_ev = np.concatenate(xs, axis=1)[:, :n_ev], np.ascontiguousarray(np.concatenate(ds, axis=1)[:, :n_ev]), np.concatenate(snrs)[:n_ev]
    pedict = posterior_samples(d_ev, model, n_pe, sub_seed(seed, 3), **kw)
    x_inj, dens = np.empty((model.n_coords, n_generated)), np.ones(n_generated)
    for c, name in enumerate(model.names):
        lo, hi, pdf = injection_tables[name]
        x_inj[c] = table_draws(lo, hi, np.asarray(pdf, dtype=np.float64), n_generated, sub_seed(seed, 32 + c), **kw)[0]
        dens = dens * table_density(lo, hi, pdf, x_inj[c])
    injdict, total = found_injections(x_inj, dens, model, sub_seed(seed, 4), **kw)
    truth = {k: x_ev[c] for c, k in enumerate(model.names)}
    truth.update(data=d_ev, snr=snr_ev, n_drawn=n_drawn, n_seen=n_seen, theta=population.get("theta"))
    return pedict, injdict, total, truth
