"""GPU: the edges of the per-point entries' staged copy back (gwinferno_amd/csrc/gwi_engine.hip: StagedRows).  The rows of 64 points are
staged on the device and copied to the caller when the stage is full or the call ends; the entries' own tests cross the stage once, at
K = 70.  Here: a call that ends exactly on a full stage (K = 64), one point past it (65) and two full stages (128), for gwi_point_cdfs,
gwi_point_pits, gwi_point_pits_exact and gwi_point_moments.

Three distinct points are evaluated once, in one call of K = 3: the reference rows.  The long calls repeat them cyclically, and since a
point's row is a function of the point alone (the entries' own tests: bits do not depend on how the points are split over calls), row p
of every output must hold the bits of reference row p % 3, NaNs in the same places.

Shapes: 3 events x 100 PE samples, 300 injections, 2 columns, 8 grid points -- the stage's arithmetic does not depend on the catalog."""
import hist_util as HU
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_EV, N_PE, N_INJ, N_GRID = 3, 100, 300, 8
COLUMNS = ("mass_1", "mass_ratio")
ENTRIES = ("point_cdfs", "point_pits", "point_pits_exact", "point_moments")
_STATE = {}


def _engine():
    """One engine with the bins and the columns of every entry set, its three points and their reference rows per entry: made once, shared."""
    if not _STATE:
        from gwinferno_amd import draws as D
        from gwinferno_amd.compositions import COMPOSITIONS
        from gwinferno_amd.synthetic import make_catalog

        pe, inj, _ = make_catalog(N_EV, N_PE, N_INJ, seed=53)
        comp = COMPOSITIONS["plpeak"](pe, inj)
        eng = comp.engine()
        x_pe, x_inj = (np.stack([np.asarray(d[c], dtype=np.float64) for c in COLUMNS]) for d in (pe, inj))
        grids = [np.linspace(*np.quantile(np.concatenate([x_pe[c].ravel(), x_inj[c]]), [0.05, 0.95]), N_GRID) for c in range(len(COLUMNS))]
        eng.set_histogram_bins(np.stack([D.cdf_codes(x_pe[c], g) for c, g in enumerate(grids)]), np.stack([D.cdf_codes(x_inj[c], g) for c, g in enumerate(grids)]), n_bins=N_GRID)
        eng.set_rank_columns(x_pe, x_inj)
        eng.set_kde_columns(x_pe, x_inj)
        thetas = HU.points(comp, "plpeak", 3)
        assert len({t.tobytes() for t in thetas}) == 3
        reference = {e: getattr(eng, e)(thetas) for e in ENTRIES}
        for rows in reference.values():
            for a in rows:
                a.setflags(write=False)
        _STATE.update(eng=eng, thetas=thetas, reference=reference)
    return _STATE["eng"], _STATE["thetas"], _STATE["reference"]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    if _STATE:
        _STATE["eng"].close()
    _STATE.clear()


@pytest.mark.parametrize("k", (64, 65, 128))
@pytest.mark.parametrize("entry", ENTRIES)
def test_rows_of_full_stages_are_the_rows_of_their_points(entry, k):
    eng, thetas, reference = _engine()
    cycle = np.arange(k) % 3
    got = getattr(eng, entry)(thetas[cycle])
    assert len(got) == len(reference[entry])
    for g, want in zip(got, reference[entry]):
        assert g.dtype == want.dtype and g.shape == (k, *want.shape[1:])
        differ = [p for p in range(k) if not np.array_equal(g[p], want[cycle[p]], equal_nan=g.dtype.kind == "f")]
        assert not differ, f"{entry}, K = {k}: rows {differ[:8]} ... differ from the rows of their points"
    # the three reference rows are not all alike: a row copied to the wrong place would show
    assert any(not np.array_equal(want[0], want[1], equal_nan=want.dtype.kind == "f") for want in reference[entry])
