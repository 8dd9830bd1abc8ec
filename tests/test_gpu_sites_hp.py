"""GPU (-m gpu): EVERYTHING the tail of an evaluation outputs -- per-event logBF, log n_eff and variance, the selection summary, the
three comparisons of the two cuts next to their thresholds, the dead-event rules and the gradient under a cut -- against the
np.longdouble referee of tests/sites_hp_util.py (bars derived there from VALUE_ATOL), on EVERY tail the engine has, each path
asserting through ``tail_path()`` / ``launch_geometry()`` / ``batch_path()`` that it ran what it claims (replay mode has no query of
its own: it is asserted through what it promises, the same bits from a second evaluation):

  host-final          the default for these sizes: the combine launch publishes rows, the host sums them
  device-final G=1/4  GWI_HOST_FINAL=0 with GWI_FINAL_GROUPS=1 / 4 (7 events over 4 final workgroups: 1/2/2/2)
  combine threads     GWI_COMBINE_THREADS at the value the engine would not pick
  batch K=4, K=16     always device-final with published events; one launch per flag set and N_obs, every point also against its
                      own single evaluation (the bars of test_batched_evaluation_matches_single)
  replay              GWI_DETERMINISTIC=1
  generic             GWI_FORCE_GENERIC=1, one parametric and one spline term
  records             eval_partial + combine, eval_batch_partial + combine_batch (summary and gradient; no per-event arrays)
  marginalised        marginalize_selection=True on host-final and batch K=4 (values only at the flat hyper-points)

Catalogs: ``sites_small`` (one tile per group) and ``sites_tiles`` under GWI_SAMPLES_PER_BLOCK=256 (several tiles per event, the
last ragged; dead, single-sample and uniform events; a graded event and graded injections whose tiles have different maxima),
with and without its designed events and with a heavy event that lets the event comparison decide.  All chains are ahead-of-time ones or the
generic kernel.  With GWI_TERMS_HP_REPORT=<file> the worst error per (term, path, site) IN UNITS OF ITS BAR is appended to that file
(profiles/sites_hp/RESULTS.md keeps one run)."""
import os

import numpy as np
import pytest
import sites_hp_util as S
import terms_hp_util as U

pytestmark = pytest.mark.gpu

NAMES = [n for _, n in S.TERMS]


@pytest.fixture(scope="module")
def terms():
    return {name: S.load_term((kind, name)) for kind, name in S.TERMS}


class EngineEvaluator:
    def __init__(self, d_pe, d_inj):
        from gwinferno_amd.engine import NativePopulationLikelihood

        self.eng = NativePopulationLikelihood(d_pe, d_inj)
        self.bound = self.eng.bound

    def close(self):
        self.eng.close()


def _got(r):
    return S.Got(r.summary, r.grad, r.log_bfs, r.log_neffs, r.variances)


def _finish(worst, failures):
    out = os.environ.get("GWI_TERMS_HP_REPORT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(worst.lines()) + "\n")
    U.report(failures, worst)


def _catalogs(term, monkeypatch, tiles=True):
    """sites_small, then sites_tiles with and without its designed events (built under GWI_SAMPLES_PER_BLOCK=256, geometry asserted)."""
    if term.name == "plzspline7":  # no ahead-of-time chain for this term alone: the generic kernel, not one compiled at run time
        monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    yield S.sites_small(term, EngineEvaluator)
    if not tiles:
        return
    monkeypatch.setenv("GWI_SAMPLES_PER_BLOCK", "256")
    for designed, heavy in ((True, False), (False, False), (False, True)):
        cat = S.sites_tiles(term, EngineEvaluator, designed=designed, heavy=heavy)
        geo = cat.ev.eng.launch_geometry()
        # the tiles the engine really made: live tiles of the graded event and of the injections have different maxima
        spread = [max(S.tile_maxima_spread(cat, h, idx, chunk) for h in range(len(term.theta))) for idx, chunk in ((cat.pe_idx[S.GRADED_EVENT], geo["chunk_pe"]), (cat.inj_idx, geo["chunk_inj"]))]
        assert min(spread) > 15.0, (spread, geo)
        # (a chain of two samples per lane rounds 256 up to its granule of 512: still two tiles per event, the last ragged)
        assert geo["tiles_per_event"] >= 2 and 700 % geo["chunk_pe"] != 0 and geo["n_inj_tiles"] >= 2, geo
        assert geo["tiles_per_event"] == 3 or geo["chunk_pe"] == 512, geo
        yield cat
    monkeypatch.delenv("GWI_SAMPLES_PER_BLOCK")


def _single(term, path, monkeypatch, tail_ok, worst, failures, kernel_ok=None, marginalised=False, tiles=True, repeat=False):
    conv = {}
    for cat in _catalogs(term, monkeypatch, tiles):
        eng = cat.ev.eng
        if kernel_ok:
            assert kernel_ok(eng.scan_kernel_name()), eng.scan_kernel_name()

        def evaluate(theta, total_inj, nobs, flags):
            r = eng.evaluate(theta, total_inj, nobs=nobs, **flags)
            tail = eng.tail_path()
            assert tail_ok(tail), (path, tail)
            if repeat:
                again = eng.evaluate(theta, total_inj, nobs=nobs, **flags)
                if not (again.log_likelihood == r.log_likelihood and np.array_equal(again.grad, r.grad) and np.array_equal(again.log_bfs, r.log_bfs, equal_nan=True)):
                    failures.append(f"{term.name} [{path}] {cat.cat_name}: a second evaluation differs")
            return _got(r)

        S.check_catalog(cat, path, worst, failures, evaluate, marginalised=marginalised, conv=conv)
        cat.close()


@pytest.mark.parametrize("name", NAMES)
def test_host_final(terms, name, monkeypatch):
    worst, failures = U.Worst(), []
    _single(terms[name], "host-final", monkeypatch, lambda t: t["host_final"] and t["publish_events"], worst, failures, kernel_ok=lambda k: not k.startswith("jit:") and (name == "plzspline7" or not k.startswith("generic")))
    _finish(worst, failures)


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_device_final(terms, name, G, monkeypatch):
    monkeypatch.setenv("GWI_HOST_FINAL", "0")
    monkeypatch.setenv("GWI_FINAL_GROUPS", str(G))
    worst, failures = U.Worst(), []
    _single(terms[name], f"device-final G={G}", monkeypatch, lambda t: not t["host_final"] and t["final_groups"] == G and t["publish_events"], worst, failures)
    _finish(worst, failures)


@pytest.mark.parametrize("name", NAMES)
def test_host_final_with_the_other_combine_workgroup_size(terms, name, monkeypatch):
    probe = S.sites_small(terms[name], EngineEvaluator)
    default = probe.ev.eng.tail_path()["combine_threads"]
    probe.close()
    other = 256 if default == 64 else 64
    monkeypatch.setenv("GWI_COMBINE_THREADS", str(other))
    worst, failures = U.Worst(), []
    _single(terms[name], f"host-final combine_threads={other}", monkeypatch, lambda t: t["host_final"] and t["combine_threads"] == other, worst, failures)
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["plpeak_ratio", "logy17", "plzspline7"])
def test_replay_mode(terms, name, monkeypatch):
    monkeypatch.setenv("GWI_DETERMINISTIC", "1")
    worst, failures = U.Worst(), []
    _single(terms[name], "replay", monkeypatch, lambda t: t["publish_events"], worst, failures, repeat=True)
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["truncnorm", "logxlogy17"])
def test_generic_kernel(terms, name, monkeypatch):
    monkeypatch.setenv("GWI_FORCE_GENERIC", "1")
    worst, failures = U.Worst(), []
    _single(terms[name], "generic", monkeypatch, lambda t: t["publish_events"], worst, failures, kernel_ok=lambda k: k.startswith("generic"))
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["plpeak_ratio", "logy17", "plzspline7"])
def test_marginalised_selection_host_final(terms, name, monkeypatch):
    worst, failures = U.Worst(), []
    _single(terms[name], "marginalised/host-final", monkeypatch, lambda t: t["host_final"], worst, failures, marginalised=True)
    _finish(worst, failures)


def _batched(term, K, path, monkeypatch, worst, failures, marginalised=False, records=False):
    """Every evaluation of ``plan(cat)`` grouped by (N_obs, flags): each group in launches of K points (padded by repeating its
    first), every point against the referee and against its own single evaluation."""
    conv = {}
    for cat in _catalogs(term, monkeypatch):
        eng = cat.ev.eng
        if not records:
            assert eng.batch_path(K) in (("rows-per-point", "pbatch") if term.name in ("plpeak_ratio", "truncnorm") else ("taps",)), eng.batch_path(K)
        if cat.cat_name == "sites_small" and not marginalised:  # the convention shifts, from a batched launch of their own
            n1 = cat.pe_idx.shape[0] + 1.0
            for at in range(0, len(term.theta), K):
                hs = list(range(at, min(at + K, len(term.theta))))
                thetas = np.stack([cat.theta(h) for h in hs + [hs[0]] * (K - len(hs))])
                res = eng.combine_batch(thetas, eng.eval_batch_partial(thetas)[0][None], cat.total_inj, nobs=n1, **S.FLAGS_OFF) if records else eng.evaluate_batch(thetas, cat.total_inj, nobs=n1, **S.FLAGS_OFF)
                for h, b in zip(hs, res):
                    conv[h] = S.convention_shift(cat, h, lambda *a, b=b: _got(b))
        groups = {}
        for h, label, nobs, flags, values_only in S.plan(cat, marginalised):
            groups.setdefault((nobs, tuple(sorted(flags.items()))), []).append((h, label, values_only))
        # (one N_obs per launch: the decisions of different points have different N_obs, so their launches hold one point K times)
        for (nobs, fl), entries in groups.items():
            flags = dict(fl)
            for at in range(0, len(entries), K):
                chunk = entries[at:at + K]
                pts = [c[0] for c in chunk] + [chunk[0][0]] * (K - len(chunk))
                thetas = np.stack([cat.theta(h) for h in pts])
                if records:
                    rec = eng.eval_batch_partial(thetas)[0]
                    res = eng.combine_batch(thetas, rec[None], cat.total_inj, nobs=nobs, **flags)
                else:
                    res = eng.evaluate_batch(thetas, cat.total_inj, nobs=nobs, **flags)
                    tail = eng.tail_path()
                    assert (not tail["host_final"] and tail["publish_events"]) if K >= 4 else True, tail
                for (h, label, values_only), b in zip(chunk, res):
                    ref = S.sites_reference(cat, h, nobs, flags)
                    S.check_point(cat, h, _got(b), ref, path, label, worst, failures, values_only=values_only, nobs=nobs, conv=conv)
                    if records:
                        continue
                    one = eng.evaluate(cat.theta(h), cat.total_inj, nobs=nobs, **flags)
                    where = f"{term.name} [{path}] {cat.cat_name} {term.tags[h]} {label}"
                    live = ref["live"]
                    same = b.log_likelihood == one.log_likelihood or abs(b.log_likelihood - one.log_likelihood) < 1e-12 * max(abs(one.log_likelihood), ref["scale"] if U.is_cancelled(term, h) else 0.0)
                    if not (same and np.allclose(b.log_bfs[live], one.log_bfs[live], rtol=1e-12, atol=1e-12) and np.allclose(b.log_neffs[live], one.log_neffs[live], rtol=1e-10, atol=1e-13)
                            and np.allclose(b.grad, one.grad, rtol=1e-10, atol=1e-11) and np.array_equal(np.isnan(b.variances), np.isnan(one.variances))
                            and np.allclose(b.variances[live], one.variances[live], rtol=1e-10, atol=1e-13) and np.allclose(b.norms, one.norms, rtol=1e-13)
                            and (b.summary.log_nEff_inj == one.summary.log_nEff_inj or abs(b.summary.log_nEff_inj - one.summary.log_nEff_inj) < 1e-10 * abs(one.summary.log_nEff_inj))):
                        failures.append(f"{where}: the batched point differs from its own single evaluation")
        cat.close()


@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("name", NAMES)
def test_batches(terms, name, K, monkeypatch):
    worst, failures = U.Worst(), []
    _batched(terms[name], K, f"batch K={K}", monkeypatch, worst, failures)
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["plpeak_ratio", "plzspline7"])
def test_marginalised_selection_batch_of_4(terms, name, monkeypatch):
    worst, failures = U.Worst(), []
    _batched(terms[name], 4, "marginalised/batch K=4", monkeypatch, worst, failures, marginalised=True)
    _finish(worst, failures)


@pytest.mark.parametrize("name", ["truncnorm", "logy17"])
def test_records_then_combine(terms, name, monkeypatch):
    """eval_partial + combine and eval_batch_partial + combine_batch: the summary and the gradient (the per-event arrays are None)."""
    worst, failures = U.Worst(), []
    term = terms[name]
    conv = {}
    for cat in _catalogs(term, monkeypatch):
        eng = cat.ev.eng

        def evaluate(theta, total_inj, nobs, flags):
            rec = eng.eval_partial(theta)[0]
            return _got(eng.combine(rec, total_inj, nobs=nobs, **flags))

        conv = S.check_catalog(cat, "records", worst, failures, evaluate, conv=conv if cat.cat_name != "sites_small" else {})
        cat.close()
    _batched(term, 4, "records/batch K=4", monkeypatch, worst, failures, records=True)
    _finish(worst, failures)
