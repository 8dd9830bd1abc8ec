#!/usr/bin/env python3
"""Injection recovery on a mock catalog: 69 events x 1000 posterior samples drawn FROM PL+Peak m1 x PL q x PL z at a stated theta
through the observation model of gwinferno_amd.mock_catalog, then the library's NUTS (gwi_nuts_engine, four
chains) under the priors of the reference's example.  Prints split R-hat per parameter and whether each true value lies inside its
90 % interval.
    python examples/mock_recovery_plpeak.py [n_events n_pe n_generated]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gwinferno_amd import mock_catalog as MC  # noqa: E402
from gwinferno_amd.compositions import COMPOSITIONS  # noqa: E402
from gwinferno_amd.sampling import Bijector, GaussianSmoothingPrior, nuts_engine, split_rhat  # noqa: E402

TRUE = {"alpha": -2.5, "beta": 1.0, "mpp": 35.0, "sigpp": 4.0, "lam": 0.08, "lamb": 2.0}
n_ev, n_pe, n_gen = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (69, 1000, 400_000)
model = MC.default_model(rho_ref=8.0, mc_ref=25.0, dl_ref=4000.0, rho_th=8.0)
grids = {k: np.linspace(model.lo[c], model.hi[c], 800) for c, k in enumerate(model.names)}
tables = {"mass_1": grids["mass_1"] ** -1.8, "mass_ratio": np.minimum(1.0, 0.05 + grids["mass_ratio"] / 0.1), "redshift": grids["redshift"] ** 1.5 * (1 + grids["redshift"])}
tables = {k: (float(grids[k][0]), float(grids[k][-1]), v) for k, v in tables.items()}
pe, inj, total, truth = MC.make_mock_catalog(MC.plpeak_population(**TRUE), tables, model, n_ev, n_pe, n_gen, seed=2026)
print(f"{n_ev} events found among {truth['n_drawn']} sources; {inj['prior'].size} of {total} injections found")
inj = {k: v for k, v in inj.items() if k != "snr"}
n_chains = 4
comps = [COMPOSITIONS["plpeak"](pe, inj) for _ in range(n_chains)]
engines = [c.engine() for c in comps]
comp, eng = comps[0], engines[0]
names = [n for n, _ in comp._theta_map()]
idx = {n: i for i, n in enumerate(names)}
prior = GaussianSmoothingPrior(eng.n_theta)  # examples/simple_powerlaw_peak_example.py:52-77
for n in ("alpha", "beta", "lamb"):
    prior.sigmas[idx[n]] = 5.0
prior.sigmas[idx["sigpp"]] = 10.0
bij = Bijector(eng.n_theta).interval(idx["mpp"], 5.0, 100.0).interval(idx["lam"], 0.0, 1.0).positive(idx["sigpp"])
theta0 = comp.theta({"alpha": -2.0, "beta": 0.5, "mpp": 30.0, "sigpp": 6.0, "lam": 0.15, "lamb": 2.7})
rng = np.random.default_rng(0)
starts = np.stack([bij.forward(bij.inverse(theta0) + 0.05 * rng.normal(size=eng.n_theta))[0] for _ in range(n_chains)])
res = nuts_engine(engines, total, prior, bij, starts, n_warmup=300, n_samples=300, seed=1, min_neff_cut=True)
chains = np.stack([r["samples"] for r in res])  # (chains, samples, theta)
print(f"divergences: {[int(r['n_divergent']) for r in res]}")
rhat = split_rhat(chains)
print("| parameter | true | 5 % | median | 95 % | inside 90 % | split R-hat |\n|---|---|---|---|---|---|---|")
for i, n in enumerate(names):
    lo, med, hi = np.percentile(chains[:, :, i], [5, 50, 95])
    print(f"| {n} | {TRUE[n]:g} | {lo:.3f} | {med:.3f} | {hi:.3f} | {'yes' if lo <= TRUE[n] <= hi else 'no'} | {rhat[i]:.3f} |")
