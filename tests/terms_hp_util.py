"""Shared by tests/test_terms_hp_cpu.py (C oracle) and tests/test_gpu_terms_hp.py (engine): the high-precision term fixture
(tests/golden/terms_hp.npz, written by tests/golden/make_terms_hp.py), the drop-in model call of every term in it, the
catalogs that make a summed gradient transparent, and the assertions -- the same ones, with the same bars, for both.

An EVALUATOR is anything with ``log_weights(theta) -> (n_ev, n_pe) array`` and ``evaluate(theta, total_inj) -> (log_l, grad)``
on a catalog it was built for; ``make(d_pe, d_inj)`` builds one from a pair of lazy densities and must expose ``.bound``.

Catalogs (the engine returns only the summed gradient):
  values  every sample of the fixture as an event of ONE sample: the log-weight of event i is the log-density of sample i.
  A       the samples that are in the support at every hyper-point ("core"), one per event, and ONE injection x_0 with
          total_inj = 1:  log_l = sum_i l(x_i) - B l(x_0),  grad_j = sum_i g_j(x_i) - B g_j(x_0).
  B       events of 3 samples, 5 injections, total_inj = 5; samples that are excluded at some hyper-points ride along with core
          ones.  Reference: the weight-averaged form, assembled from the fixture in np.longdouble.
"""
import os

import numpy as np
from golden_util import GOLDEN_DIR

VALUE_ATOL = 1e-11  # term-level bar of tests/test_gpu_terms.py, uniform over the exponent sweep
GRAD_RTOL = 1e-8    # per COMPONENT: |got_j - ref_j| <= GRAD_RTOL max(1, |ref_j|)
LOGL_RTOL = 1e-9    # |got - ref| <= LOGL_RTOL |ref|, as tests/test_gpu_fuzz.py and tests/test_c_oracle.py
# The hyper-points at which the density is flat (xi = 0, Beta(1, 1)) or flat to 1e-12 (xi = 1e-12): there the sums log_l is assembled
# from cancel, exactly or to ~1e-10 of their size, the fixture's log_l is 0 or below 2.1e-9, and a bar relative to it asks for digits
# that no float64 sum of numbers of order 20-40 holds.  At these tags ALONE the bar is LOGL_RTOL of the largest of those sums (an
# absolute floor of 1.6e-8 to 4.2e-8); everywhere else it is relative to |log_l| itself.
LOGL_CANCELLED = {
    "tilt": {"xi0/sig0.05", "xi0/sig1", "xi0/sig6", "xi1e-12/sig0.05", "xi1e-12/sig1", "xi1e-12/sig6"},
    "tilt_joint": {"xi0/sig0.05", "xi0/sig1", "xi0/sig6", "xi1e-12/sig0.05", "xi1e-12/sig1", "xi1e-12/sig6"},
    "beta": {"a1/b1"},
}

MMIN, MMAX = 5.0, 100.0


def load():
    return np.load(os.path.join(GOLDEN_DIR, "terms_hp.npz"))


class Term:
    def __init__(self, z, name):
        self.name = name
        self.params = [str(p) for p in z[f"{name}/params"]]
        self.columns = [str(c) for c in z[f"{name}/columns"]]
        self.cols = [z[f"{name}/col/{c}"] for c in self.columns]
        self.tags = [str(t) for t in z[f"{name}/tags"]]
        self.theta = z[f"{name}/theta"]
        self.logp = z[f"{name}/logp"]
        self.dlogp = z[f"{name}/dlogp"]

    @property
    def n(self):
        return len(self.cols[0])


class Product(Term):
    """Two fixture terms on disjoint columns and parameters as one model: sample i is (a's sample i, b's sample i), hyper-point
    h is (a's point h, b's point h mod len(b))."""

    def __init__(self, a, b):
        n = min(a.n, b.n)
        hb = np.arange(len(a.theta)) % len(b.theta)
        self.name = f"{a.name}*{b.name}"
        self.parts = (a, b)
        self.params = [f"{a.name}.{p}" for p in a.params] + [f"{b.name}.{p}" for p in b.params]
        self.cols = [c[:n] for c in a.cols] + [c[:n] for c in b.cols]
        self.tags = [f"{ta}|{b.tags[j]}" for ta, j in zip(a.tags, hb)]
        self.theta = np.concatenate([a.theta, b.theta[hb]], axis=1)
        self.logp = a.logp[:, :n] + b.logp[hb][:, :n]
        self.dlogp = np.concatenate([a.dlogp[:, :, :n], b.dlogp[hb][:, :, :n]], axis=1)
        dead = np.isneginf(self.logp)
        self.dlogp = np.where(dead[:, None, :], 0.0, self.dlogp)


def density(name, cols, p):
    """The drop-in model call of fixture term ``name`` on the data arrays ``cols`` (PE- or injection-shaped) at parameters ``p``."""
    from gwinferno_amd import models as M

    if name == "powerlaw":
        return M.powerlaw_pdf(cols[0], p[0], MMIN, MMAX)
    if name == "plpeak":
        return M.plpeak_primary_pdf(cols[0], p[0], MMIN, MMAX, p[1], p[2], p[3])
    if name == "plpeak_ratio":
        return M.plpeak_primary_ratio_pdf(cols[0], cols[1], p[0], p[1], MMIN, MMAX, p[2], p[3], p[4])
    if name == "ratio":  # columns (q, m1, mmin / m1): the per-sample lower bound is a data array of its own
        return M.powerlaw_pdf(cols[0], p[0], cols[2], 1)
    if name == "plpeak_smooth":
        return M.plpeak_primary_pdf(cols[0], p[0], MMIN, MMAX, p[1], p[2], p[3], delta=p[4])
    if name == "tilt":
        return M.mixture_isoalign_spin_tilt(cols[0], p[0], p[1])
    if name == "tilt_joint":
        return M.default_spin_tilt(cols[0], cols[1], p[0], p[1])
    if name == "beta":
        return M.betadist(cols[0], p[0], p[1])
    if name == "truncnorm":
        return M.truncnorm_pdf(cols[0], p[0], p[1], 0.0, 1.0)
    raise KeyError(name)


class Catalog:
    """Sample indices of a fixture term arranged as events and injections, and the model bound to them."""

    def __init__(self, term, make, pe_idx, inj_idx):
        self.term = term
        self.pe_idx, self.inj_idx = np.asarray(pe_idx), np.asarray(inj_idx)
        self.pe = [np.ascontiguousarray(c[self.pe_idx]) for c in term.cols]
        self.inj = [np.ascontiguousarray(c[self.inj_idx]) for c in term.cols]
        if term.name == "ratio":  # mmin / m1 once: the model functions key their columns on the identity of the arrays
            with np.errstate(all="ignore"):
                self.pe.append(MMIN / self.pe[1])
                self.inj.append(MMIN / self.inj[1])
        p0 = term.theta[0]
        self.ev = make(self._density(self.pe, p0), self._density(self.inj, p0))
        # theta slot of every named parameter: bind the model once more, lazily, with marker values
        marks = np.arange(1.0, len(term.params) + 1.0)
        layout = self.ev.bound.theta_of(self._density(self.pe, marks))
        self.slot = [int(np.flatnonzero(layout == m)[0]) for m in marks]
        assert self.ev.bound.n_theta == len(marks)

    def _density(self, cols, p):
        t = self.term
        if isinstance(t, Product):
            a, b = t.parts
            na, ka = len(a.cols), len(a.params)
            return density(a.name, cols[:na], p[:ka]) * density(b.name, cols[na:], p[ka:])
        return density(t.name, cols, p)

    def theta(self, h):
        th = np.zeros(len(self.slot))
        th[self.slot] = self.term.theta[h]
        return th

    def close(self):
        close = getattr(self.ev, "close", None)
        if close:
            close()


def core_samples(term):
    """Samples in the support at every hyper-point, and those in it at some but not all."""
    live = np.isfinite(term.logp)
    return np.flatnonzero(live.all(axis=0)), np.flatnonzero(live.any(axis=0) & ~live.all(axis=0))


def values_catalog(term, make):
    idx = np.arange(term.n)
    return Catalog(term, make, idx.reshape(-1, 1), idx)


def catalog_a(term, make):
    core, _ = core_samples(term)
    assert len(core) >= 8, (term.name, len(core))
    return Catalog(term, make, core.reshape(-1, 1), core[:1])


def catalog_b(term, make):
    core, some = core_samples(term)
    seq, s = [], list(some)
    for k, c in enumerate(core):
        seq.append(c)
        if k % 2 == 1 and s:
            seq.append(s.pop(0))
    n_ev = len(seq) // 3
    assert n_ev >= 4, (term.name, n_ev)
    inj = [core[0], some[0] if len(some) else core[1], core[3], core[5], core[7]]
    return Catalog(term, make, np.array(seq[: 3 * n_ev]).reshape(n_ev, 3), inj)


def reference(cat, h):
    """(log_l, grad, scale) of the hierarchical likelihood on ``cat`` at hyper-point ``h`` (n_obs = number of events, total_inj = number
    of injections, no cuts), from the fixture in extended precision: sum_e log mean_i p - n_obs log(sum_inj p / total_inj).

    ``scale`` is the largest of the four sums log_l is assembled from (sum_e logsumexp_e, n_obs log n_pe, n_obs logsumexp_inj, n_obs log
    total_inj): the size of the absolute floor at the LOGL_CANCELLED hyper-points, where they cancel; unused elsewhere."""
    L = np.longdouble
    t = cat.term
    def side(idx):  # idx: (..., n) sample indices -> logsumexp (...), weight-averaged derivatives (P, ...)
        lp = t.logp[h][idx].astype(L)
        d = t.dlogp[h][:, idx].astype(L)
        m = np.max(lp, axis=-1, keepdims=True)
        w = np.exp(lp - m)
        s = np.sum(w, axis=-1)
        return np.log(s) + m[..., 0], np.sum(w * d, axis=-1) / s

    lse_pe, g_pe = side(cat.pe_idx)
    lse_inj, g_inj = side(cat.inj_idx)
    n_ev, n_pe = cat.pe_idx.shape
    n_inj = len(cat.inj_idx)
    parts = [np.sum(lse_pe), -n_ev * np.log(L(n_pe)), -n_ev * lse_inj, n_ev * np.log(L(n_inj))]
    grad = np.sum(g_pe, axis=1) - n_ev * g_inj
    return float(sum(parts)), grad.astype(np.float64), float(max(abs(p) for p in parts))


class Worst:
    """Largest error seen per (term, path, what), for assertion messages and profiles/near_singular/RESULTS.md."""

    def __init__(self):
        self.rows = {}

    def note(self, key, err, where):
        if not (err <= self.rows.get(key, (-1.0, ""))[0]):
            self.rows[key] = (float(err), where)

    def lines(self):
        return [f"{' / '.join(k)}: {e:.3e} at {w}" for k, (e, w) in sorted(self.rows.items())]


def check_values(cat, path, worst, failures):
    t = cat.term
    for h in range(len(t.theta)):
        got = cat.ev.log_weights(cat.theta(h))[:, 0]
        ref = t.logp[h]
        dead = np.isneginf(ref)
        if not np.array_equal(np.isneginf(got), dead):
            failures.append(f"{t.name} [{path}] {t.tags[h]}: support differs at samples {np.flatnonzero(np.isneginf(got) != dead)[:6].tolist()}")
            continue
        err = np.abs(got[~dead] - ref[~dead])
        k = int(np.argmax(err))
        worst.note((t.name, path, "value"), err[k], f"{t.tags[h]} theta={t.theta[h].tolist()} sample {np.flatnonzero(~dead)[k]}")
        if not err[k] < VALUE_ATOL:
            failures.append(f"{t.name} [{path}] {t.tags[h]}: |log w - ref| = {err[k]:.3e} >= {VALUE_ATOL:g} (sample {np.flatnonzero(~dead)[k]})")


def grad_errors(t, got_grad, ref_grad):
    """Per-component error in units of the bar: |got_j - ref_j| / max(1, |ref_j|)."""
    return np.abs(got_grad - ref_grad) / np.maximum(1.0, np.abs(ref_grad))


def check_gradients(cat, path, worst, failures, points=None, results=None):
    t = cat.term
    total = float(len(cat.inj_idx))
    for h in (range(len(t.theta)) if points is None else points):
        log_l, grad = results[h] if results is not None else cat.ev.evaluate(cat.theta(h), total)
        grad = np.asarray(grad)[cat.slot]
        ref_l, ref_g, scale_l = reference(cat, h)
        cancelled = t.tags[h] in LOGL_CANCELLED.get(t.name, ())
        e_l = 0.0 if log_l == ref_l else abs(log_l - ref_l) / (max(scale_l, abs(ref_l)) if cancelled else (abs(ref_l) or 1e-300))
        worst.note((t.name, path, "log_l (relative)"), e_l, t.tags[h])
        if not e_l < LOGL_RTOL:
            failures.append(f"{t.name} [{path}] {t.tags[h]}: log_l {log_l!r} vs {ref_l!r}: relative {e_l:.3e} >= {LOGL_RTOL:g}{' (of the cancelled sums)' if cancelled else ''}")
        e = grad_errors(t, grad, ref_g)
        for j, name in enumerate(t.params):
            worst.note((t.name, path, f"d/d{name}"), e[j], f"{t.tags[h]} theta={t.theta[h].tolist()} ref={ref_g[j]:.6g}")
            if not e[j] <= GRAD_RTOL:
                failures.append(f"{t.name} [{path}] {t.tags[h]}: d/d{name} = {grad[j]!r} vs {ref_g[j]!r}: error {e[j]:.3e} of max(1, |ref|) > {GRAD_RTOL:g}")


def report(failures, worst):
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:40]) + "\nworst errors:\n  " + "\n  ".join(worst.lines())
