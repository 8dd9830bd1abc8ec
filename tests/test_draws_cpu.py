"""CPU: weighted index draws (include/gwi_engine.h: gwi_draw_indices) -- the NumPy statement of the semantics against the
definition on hand-made segments, the ``"device"`` mode of the posterior-predictive branch of ``hierarchical_likelihood``
through a host-only stand-in of the engine, and the two new symbols in the binding, the header and the library."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_definition(lw, mask, u):
    """The definition, one sample at a time, with exactly rounded prefixes (math.fsum)."""
    lw = [float(v) for v in lw]
    mask = [1] * len(lw) if mask is None else [int(m) for m in mask]
    live = [j for j in range(len(lw)) if mask[j] and math.isfinite(lw[j])]
    if not live:
        return -1
    big = max(lw[j] for j in live)
    w = [math.exp(lw[j] - big) if j in live else 0.0 for j in range(len(lw))]
    positive = [j for j in range(len(w)) if w[j] > 0.0]
    if not positive:
        return -1
    c_last = math.fsum(w)
    for j in positive:
        if math.fsum(w[: j + 1]) > u * c_last:
            return j
    return positive[-1]


def test_reference_function_on_hand_made_segments():
    from gwinferno_amd.draws import draw_indices_reference as draw

    inf, nan = float("inf"), float("nan")
    top = 1.0 - 2.0**-53
    us = np.array([0.0, 0.1, 0.25, 0.5, 0.75, 0.999, top])
    # the heaviest sample is masked out: never drawn, and the maximum is taken over the others
    lw = np.log(np.array([1.0, 1000.0, 2.0, 1.0]))
    mask = np.array([1, 0, 1, 1], dtype=np.uint8)
    got = draw(lw, mask, us)
    assert got.dtype == np.int32 and got.shape == us.shape
    assert [int(g) for g in got] == [_by_definition(lw, mask, u) for u in us] == [0, 0, 2, 2, 3, 3, 3]
    # -inf, +inf and NaN log-weights have no weight
    lw = np.array([-inf, 0.0, nan, -1.0, inf, -inf])
    got = draw(lw, None, us)
    assert [int(g) for g in got] == [_by_definition(lw, None, u) for u in us]
    assert set(int(g) for g in got) == {1, 3}
    assert int(draw(lw, None, np.array(0.0))) == 1 and int(draw(lw, None, np.array(top))) == 3  # u = 0 skips the dead first sample; the top ends on the last live one
    # nothing has weight -> -1, for every uniform
    assert list(draw(np.array([-inf, nan, -inf]), None, us)) == [-1] * us.size
    assert list(draw(np.zeros(4), np.zeros(4, dtype=np.uint8), us)) == [-1] * us.size
    assert list(draw(np.zeros(0), None, us)) == [-1] * us.size
    # a single live sample takes every draw
    lw = np.array([-inf, -inf, -700.0, -inf])
    assert list(draw(lw, None, us)) == [2] * us.size
    # weights far below the maximum underflow to zero and are never drawn
    lw = np.array([-2000.0, 0.0, -2000.0])
    assert list(draw(lw, None, us)) == [1] * us.size
    # a shaped batch of uniforms keeps its shape; random segments agree with the definition draw by draw
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 300):
        lw = rng.normal(scale=4.0, size=n)
        lw[rng.uniform(size=n) < 0.2] = -inf
        mask = (rng.uniform(size=n) < 0.8).astype(np.uint8)
        u = np.concatenate([[0.0, top], rng.uniform(size=30)]).reshape(4, 8)
        got = draw(lw, mask, u)
        assert got.shape == (4, 8)
        assert [int(g) for g in got.ravel()] == [_by_definition(lw, mask, x) for x in u.ravel()]


def test_segments_layout_and_mass_cut_masks():
    from gwinferno_amd.draws import draw_indices_reference, draw_indices_segments, mass_cut_masks

    rng = np.random.default_rng(11)
    lw_pe, lw_inj = rng.normal(size=(3, 40)), rng.normal(size=90)
    pe = {"mass_1": rng.uniform(2.0, 120.0, size=(3, 40)), "mass_ratio": rng.uniform(0.05, 1.0, size=(3, 40))}
    inj = {"mass_1": rng.uniform(2.0, 120.0, size=90), "mass_ratio": rng.uniform(0.05, 1.0, size=90)}
    m_pe, m_inj = mass_cut_masks(pe, inj, 5.0, 3.0, 100.0)
    assert m_pe.dtype == np.uint8 and m_pe.shape == (3, 40) and m_inj.shape == (90,)
    assert np.array_equal(m_pe != 0, (pe["mass_1"] >= 5.0) & (pe["mass_1"] <= 100.0) & (pe["mass_1"] * pe["mass_ratio"] >= 3.0))
    assert 0 < m_pe.sum() < m_pe.size
    u_pe, u_inj = rng.uniform(size=(3, 7)), rng.uniform(size=5)
    idx_pe, idx_inj = draw_indices_segments(lw_pe, lw_inj, m_pe, m_inj, u_pe, u_inj)
    assert idx_pe.shape == (3, 7) and idx_inj.shape == (5,)
    for ev in range(3):
        assert np.array_equal(idx_pe[ev], draw_indices_reference(lw_pe[ev], m_pe[ev], u_pe[ev]))
        assert np.all(m_pe[ev][idx_pe[ev]] == 1)
    assert np.all(m_inj[idx_inj] == 1)


class _DrawingOracleEngine:
    """Host-only stand-in of the engine: log_weights from the independent host evaluation, draw_indices from the NumPy
    statement of the semantics (as tests/test_jax_adapter_cpu.py does for evaluate / log_weights)."""

    def __init__(self, eng):
        from oracle.c_oracle import COracle

        self._eng, self._orc = eng, COracle(eng.bound)
        self.masks = (None, None)
        self.mask_uploads = self.draw_calls = self.log_weight_calls = 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def evaluate(self, theta, total_inj, nobs=None, marginalize_selection=False, min_neff_cut=True, max_variance_cut=False, want_grad=True, copy=True):
        from gwinferno_amd.engine import EvalResult

        r = self._orc.evaluate(theta, total_inj, nobs=nobs, marginalize_selection=marginalize_selection, min_neff_cut=min_neff_cut, max_variance_cut=max_variance_cut)
        return EvalResult(log_likelihood=r["log_likelihood"], grad=r["grad"] if want_grad else None, summary=r["summary"], log_bfs=r["logBFs"], log_neffs=r["log_nEffs"],
                          variances=r["variance_log_BFs"], norms=r["norms"])

    def evaluate_batch(self, thetas, total_inj, **kw):
        return [self.evaluate(t, total_inj, **kw) for t in np.asarray(thetas)]

    def log_weights(self, theta):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from bound_eval import log_weights

        self.log_weight_calls += 1
        lpe, linj, _ = log_weights(self._eng.bound, theta, include_consts=True)
        return lpe, linj

    def set_draw_mask(self, pe_mask=None, inj_mask=None):
        self.mask_uploads += 1
        self.masks = (pe_mask, inj_mask)

    def draw_indices(self, thetas, u_pe=None, u_inj=None):
        from gwinferno_amd.draws import draw_indices_segments

        self.draw_calls += 1
        n_before = self.log_weight_calls
        lpe, linj = self.log_weights(np.asarray(thetas, dtype=np.float64))
        self.log_weight_calls = n_before
        return draw_indices_segments(lpe, linj, self.masks[0], self.masks[1], u_pe, u_inj)


@pytest.fixture
def shim(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tests", "jaxshim"))
    for m in [k for k in sys.modules if k == "jax" or k.startswith("jax.")]:
        monkeypatch.delitem(sys.modules, m)
    import jax

    yield jax
    for m in [k for k in sys.modules if k == "jax" or k.startswith("jax.")]:
        sys.modules.pop(m, None)


def test_device_mode_of_the_posterior_predictive_branch(shim, monkeypatch):
    """set_ppc_draws("device"): the sites {p}_obs_event_{ev} / {p}_pred_event_{ev} equal the host mode's, from the NumPy call
    and from the traced one; the mask is built once per engine and cut values; no per-sample weight is fetched."""
    import jax.numpy as jnp

    from gwinferno_amd import _native as N
    from gwinferno_amd import likelihood as L
    from gwinferno_amd.engine import NativePopulationLikelihood
    from gwinferno_amd.lazy import where_finite
    from gwinferno_amd.models import PowerlawRedshiftModel, powerlaw_primary_ratio_pdf
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, total = make_catalog(6, 64, 600, seed=17)
    z_model = PowerlawRedshiftModel(z_pe=pe["redshift"], z_inj=inj["redshift"])
    made = {}

    def fake_engine_for(pe_w, inj_w, hv=None, device=-1):
        if "eng" not in made:
            made["eng"] = _DrawingOracleEngine(NativePopulationLikelihood(pe_w, inj_w, hv, device=N.DEVICE_HOST_ONLY))
        return made["eng"]

    monkeypatch.setattr(L, "engine_for", fake_engine_for)
    monkeypatch.setattr(L, "_NUMPYRO", [None])
    names = ["mass_1", "mass_ratio", "redshift"]

    def model(alpha, beta, lamb, m2min=3.0):
        def get_weights(d):
            return where_finite(powerlaw_primary_ratio_pdf(d["mass_1"], d["mass_ratio"], alpha=alpha, beta=beta, mmin=5.0, mmax=100.0) * z_model(d["redshift"], lamb) / d["prior"])

        L.hierarchical_likelihood(get_weights(pe), get_weights(inj), total_inj=total, Nobs=6, Tobs=1.0, surveyed_hypervolume=z_model.normalization(lamb=lamb),
                                  min_neff_cut=False, posterior_predictive_check=True, param_names=names, pedata=pe, injdata=inj, m1min=5.0, m2min=m2min, mmax=100.0)
        return L.last_sites()

    ppc = [f"{p}_{kind}_event_{ev}" for p in names for kind in ("obs", "pred") for ev in range(6)]
    point = dict(alpha=-2.3, beta=0.8, lamb=2.5)
    assert L._PPC_DRAWS[0] == "host"  # the default
    host = model(**point)
    eng = made["eng"]
    assert eng.draw_calls == 0 and eng.log_weight_calls == 1
    assert L.set_ppc_draws("device") == "host"
    try:
        dev = model(**point)
        assert eng.draw_calls == 1 and eng.mask_uploads == 1 and eng.log_weight_calls == 1
        for name in ppc:
            assert dev[name] == host[name], name
        traced = model(**{k: jnp.asarray(v) for k, v in point.items()})
        for name in ppc:
            assert traced[name].val == host[name], name
        assert eng.mask_uploads == 1  # same engine, same cuts: the mask stays
        other = model(**dict(point, alpha=-1.1))
        assert eng.mask_uploads == 1 and any(other[name] != host[name] for name in ppc)
        model(**point, m2min=4.0)
        assert eng.mask_uploads == 2  # other cut values: a new mask
        assert np.array_equal(eng.masks[0] != 0, (pe["mass_1"] >= 5.0) & (pe["mass_1"] <= 100.0) & (pe["mass_1"] * pe["mass_ratio"] >= 4.0))
        with pytest.raises(ValueError):
            L.set_ppc_draws("gpu")
    finally:
        assert L.set_ppc_draws("host") == "device"
    again = model(**point)
    for name in ppc:
        assert again[name] == host[name], name


def test_new_symbols_in_binding_header_and_library():
    from gwinferno_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gwi_engine.h")).read()
    declared = set(re.findall(r"^(?:const )?[a-z_0-9]+\**\s+\**(gwi_[a-z_]+)\s*\(", hdr, flags=re.M))
    for sym in ("gwi_set_draw_mask", "gwi_draw_indices"):
        assert sym in _native.EXPORTED_SYMBOLS and sym in declared
        fn = getattr(lib, sym)
        assert fn.restype is not None and fn.argtypes
    assert len(lib.gwi_draw_indices.argtypes) == 9 and len(lib.gwi_set_draw_mask.argtypes) == 3
    assert lib.gwi_abi_version() == 3  # no struct changed


def test_host_only_handle_refuses_both_entries():
    """A host-only handle owns no device: both entries answer GWI_ERR_INVALID with a message; a sharded engine refuses in Python."""
    from gwinferno_amd import _native as N
    from gwinferno_amd.compositions import COMPOSITIONS
    from gwinferno_amd.synthetic import make_catalog

    pe, inj, _ = make_catalog(2, 8, 16, seed=1)
    eng = COMPOSITIONS["plpeak"](pe, inj).engine(device=N.DEVICE_HOST_ONLY)
    try:
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
            eng.set_draw_mask(np.ones((2, 8), dtype=np.uint8), None)
        with pytest.raises(N.NativeEngineError, match="GWI_ERR_INVALID.*host-only"):
            eng.draw_indices(np.zeros(eng.n_theta), np.zeros((2, 1)), np.zeros(3))
        with pytest.raises(ValueError, match="pe_mask has shape"):
            eng.set_draw_mask(np.ones((2, 7), dtype=np.uint8), None)
        with pytest.raises(ValueError, match="u_pe has shape"):
            eng.draw_indices(np.zeros(eng.n_theta), np.zeros((3, 1)), None)
    finally:
        eng.close()
