"""CPU side of the structured response designs: the generator keeps its promises (asserted on the matrices themselves, so a
later edit cannot quietly turn a design back into near-uniform data), and for every (engine family, design) pair of
tests/test_gpu_response_designs.py the float64 oracle is finite and no observed cell sits on the Bernoulli clamp -- the
condition under which the GPU comparison leaves nothing out.  The engines are built on the numpy backend exactly as the GPU
tests build them on the device, so the parameters are the same bits."""
import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import design_cases as dc
from tests import response_designs as rd
from tests.oracle_backend import OracleBackend

CPU = torch.device("cpu")


def _check_edges(y, f):
    """Every named edge of with_edges, on the matrix."""
    obs = y != 255
    d = rd.describe(y)
    assert set(np.unique(y).tolist()) <= {0, 1, 255}
    if "empty_person" in f:
        assert not obs[f["empty_person"]].any()
    if "empty_block" in f:
        assert not obs[f["empty_block"]:f["empty_block"] + 64].any()
    if "complete_case" in f:
        assert obs[f["complete_case"]].all() and len(d["unanswered_items"]) == 0
    if "unanswered_item" in f:
        assert not obs[:, f["unanswered_item"]].any()
    if "all_one_item" in f:
        j1, j0 = f["all_one_item"], f["all_zero_item"]
        assert obs[:, j1].sum() >= 2 and (y[obs[:, j1], j1] == 1).all()
        assert obs[:, j0].sum() >= 2 and (y[obs[:, j0], j0] == 0).all()
        assert j1 in d["all_one_items"] and j0 in d["all_zero_items"]
    if "all_one_person" in f:
        i1, i0 = f["all_one_person"], f["all_zero_person"]
        assert obs[i1].any() and (y[i1, obs[i1]] == 1).all()
        assert obs[i0].any() and (y[i0, obs[i0]] == 0).all()
    for k in ("missing", "n_missing", "min_obs", "max_obs"):
        assert f[k] == d[k], k
    assert np.array_equal(f["empty_persons"], d["empty_persons"])
    assert np.array_equal(f["unanswered_items"], d["unanswered_items"])
    want_empty = (1 if "empty_person" in f else 0) + (64 if "empty_block" in f else 0)
    if f.get("design") == "booklets":
        assert len(d["empty_persons"]) == want_empty


def test_booklets_are_contiguous_and_of_very_different_length():
    for sorted_rows in (True, False):
        y, f = rd.booklets(3000, 500, (10, 40, 150), sorted_rows, seed=3)
        obs = y != 255
        cnt = obs.sum(1)
        assert sorted(set(cnt.tolist())) == [10, 40, 150] and (f["min_obs"], f["max_obs"]) == (10, 150)
        assert [int((cnt == v).sum()) for v in (10, 40, 150)] == [1000, 1000, 1000]
        for i in range(0, 3000, 97):                          # one contiguous run of observed cells per person
            j = np.flatnonzero(obs[i])
            assert j[-1] - j[0] + 1 == len(j)
        assert np.array_equal(f["unanswered_items"], np.arange(200, 500)) and not obs[:, 200:].any()
        assert f["missing"] == pytest.approx(1 - 200 / 3.0 / 500) and f["missing"] == (y == 255).mean() and f["missing"] > 0.5
        changes = int((np.diff(f["booklet_of"]) != 0).sum())
        if sorted_rows:
            assert changes == 2 and np.array_equal(cnt, np.repeat([10, 40, 150], 1000))
        else:
            assert changes > 1000                             # shuffled: every 64-person group mixes the lengths
            assert all(len(set(cnt[g:g + 64].tolist())) == 3 for g in range(0, 3000 - 64, 64))
        assert set(np.unique(y[obs]).tolist()) == {0, 1}
    y1, _ = rd.booklets(300, 50, (5, 20), True, seed=9)
    y2, _ = rd.booklets(300, 50, (5, 20), True, seed=9)
    assert np.array_equal(y1, y2)                             # seeded
    # responses follow the latent: persons' mean scores on a common booklet spread far more than coin flips would
    y, f = rd.booklets(2000, 60, (60,), True, seed=4)
    assert y.mean(1).std() > 2 * np.sqrt(0.25 / 60)
    # overlapping booklets where they do not fit one behind the other
    y, f = rd.booklets(3000, 500, (350, 300, 250), False, seed=5)
    assert f["starts"] == [0, 100, 250] and len(f["unanswered_items"]) == 0 and 0.39 < (y == 255).mean() < 0.41


def test_with_edges_adds_what_it_names():
    y0, f0 = rd.booklets(1000, 120, (6, 20, 60), False, seed=1)
    keep = y0.copy()
    y, f = rd.with_edges(y0, f0, seed=2, empty_block=256)
    assert np.array_equal(y0, keep)                           # a copy
    _check_edges(y, f)
    assert len(f["empty_persons"]) == 65 and f["unanswered_item"] in f["unanswered_items"]
    y, f = rd.with_edges(y0, f0, seed=2, complete_case=True, unanswered_item=False)
    _check_edges(y, f)
    assert f["max_obs"] == 120
    with pytest.raises(ValueError):
        rd.with_edges(y0, f0, complete_case=True, unanswered_item=True)


def test_near_switch_sets_the_fraction_by_count():
    N, J = 200, 64
    half = N * J // 2
    ys = {}
    for n in (half - 1, half, half + 1):
        y, f = rd.near_switch(N, J, n / float(N * J), seed=31)
        assert int((y == 255).sum()) == n == f["n_missing"]
        assert ((y == 255).sum() / float(N * J) < 0.5) == (n < half)      # the engine's rule, on the engine's arithmetic
        assert f["min_obs"] < 8 and f["max_obs"] > 56                     # nothing like equal-length persons
        ys[n] = y
    for a, b in ((half - 1, half), (half, half + 1)):                     # the same persons: one cell apart, holes nested
        diff = ys[a] != ys[b]
        assert diff.sum() == 1 and (ys[b][diff] == 255).all()


def test_degenerate_ends():
    y, f = rd.all_missing(200, 37)
    assert (y == 255).all() and f["missing"] == 1.0 and len(f["empty_persons"]) == 200
    y, f = rd.single_cell(200, 37)
    assert int((y != 255).sum()) == 1 and y[f["cell"]] == 1 and f["max_obs"] == 1 and f["min_obs"] == 0
    assert len(f["empty_persons"]) == 199 and len(f["unanswered_items"]) == 36


DESIGN_NAMES = sorted({c[1] for c in dc.IRT1D_SPARSE + dc.IRT1D_DENSE + dc.IRT1D_AMORT + dc.MVN_AMORT + [dc.MVN_LARGE] + dc.MVN_BBVI
                       + dc.HODINA + dc.CCDM + dc.VAECCDM + dc.CDM_SF} | {"hetero_shards"})


@pytest.mark.parametrize("name", DESIGN_NAMES)
def test_named_designs_keep_their_promises(name):
    y, f = dc.design(name)
    d = rd.describe(y)
    if f["design"] == "booklets":
        _check_edges(y, f)
    assert f["missing"] == d["missing"] and np.array_equal(f["empty_persons"], d["empty_persons"])
    cnt = d["obs_per_person"]
    if name.startswith("complete"):
        assert f["missing"] == 0.0 and "all_one_item" in f
        return
    if f["design"] == "booklets":
        assert len(f["unanswered_items"]) >= 1 or "complete_case" in f
        assert len(f["empty_persons"]) >= 1 and f["max_obs"] >= 4 * max(1, int(np.min(cnt[cnt > 0])))       # very unequal persons
    side = {"dense3000": False, "hetero_shards": True}.get(name, True)
    assert (f["missing"] >= 0.5) == side, (name, f["missing"])
    if name == "sorted9000":
        assert len(y) > 2 * 4096 and f["sorted_rows"] and len(f["unanswered_items"]) == 301
    if name in ("shuffled3000", "amort640"):
        assert not f["sorted_rows"]
    if name == "j1024_complete":
        assert y.shape[1] == 1024 and f["max_obs"] == 1024 and f["missing"] > 0.93
    if name == "hetero_shards":
        half = len(y) // 2
        assert (y[:half] == 255).mean() < 0.3 and (y[half:] == 255).mean() > 0.85


def _irt_case_on_the_oracle(tag, eng, y, idx, spec, seed):
    params = dc.params_of(eng)
    eps = vo.philox_normals(seed, 0, 0, idx, spec["D"])
    loss, g = vo.loss_and_grads(spec, params, y, [idx], [eps])
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in g.values()), tag
    assert sorted(g) == sorted(eng.all_names())
    on, below, above, n_obs, zmax = dc.band(spec, params, y, idx, eps)
    assert on == 0, (tag, "observed cells on the clamp", on)
    return below, above, n_obs, zmax, g


@pytest.mark.parametrize("case", dc.IRT1D_SPARSE + dc.IRT1D_DENSE, ids=[c[0] for c in dc.IRT1D_SPARSE + dc.IRT1D_DENSE])
def test_irt1d_cases_on_the_oracle(case):
    tag, dname, model, B = case[:4]
    eng, y, idx = dc.irt1d_engine(case, CPU, OracleBackend())
    facts = dc.design(dname)[1]
    below, above, n_obs, zmax, g = _irt_case_on_the_oracle(tag, eng, y, idx, dc.irt_spec(model, 1, len(y), y.shape[1], False),
                                                           dc.IRT1D_SEED)
    if dname == "single_cell":
        assert n_obs == 1                                     # (the subsample holds the one observed cell)
    if tag in dc.BEYOND_CLAMP:                                # cells BEYOND the clamp are wanted: zero gradient, constant log-probability
        assert below + above >= 100 and (model != "irt_3pl" or below == 0), (tag, below, above)
    if tag in dc.NONE_BEYOND:
        assert below + above == 0
    for j in facts["unanswered_items"]:
        assert all((g[n][..., j] == 0.0).all() for n in ("a", "b", "c", "d") if n in g)
    # every model of each row of the table has its saturated design
    for row in (dc.IRT1D_SPARSE, dc.IRT1D_DENSE):
        have = {c[2] for c in row if c[0] in dc.BEYOND_CLAMP}
        assert have == {"irt_1pl", "irt_2pl", "irt_3pl"}
        assert any(c[2] == "irt_4pl" and c[0] in dc.NONE_BEYOND for c in row)


@pytest.mark.parametrize("model", ["irt_2pl", "irt_3pl", "irt_4pl"])
def test_near_switch_and_shard_cases_on_the_oracle(model):
    N, J = 200, 64
    half = N * J // 2
    if model != "irt_4pl":
        for n_missing in (half - 1, half, half + 1):
            y, _ = rd.near_switch(N, J, n_missing / float(N * J), seed=31)
            case = ("near_switch", None, model, None, 161, 0, 0.0)
            eng, y, idx = dc.irt1d_engine(case, CPU, OracleBackend(), y=y)
            _irt_case_on_the_oracle("near_switch", eng, y, idx, dc.irt_spec(model, 1, N, J, False), dc.IRT1D_SEED)
    if model != "irt_3pl":
        y = dc.design("hetero_shards")[0]
        case = ("hetero", "hetero_shards", model, None, 171, 0, 0.0)
        eng, y, idx = dc.irt1d_engine(case, CPU, OracleBackend())
        _irt_case_on_the_oracle("hetero", eng, y, idx, dc.irt_spec(model, 1, len(y), y.shape[1], False), dc.IRT1D_SEED)


@pytest.mark.parametrize("case", dc.IRT1D_AMORT, ids=[c[0] for c in dc.IRT1D_AMORT])
def test_irt1d_amortized_cases_on_the_oracle(case):
    tag, dname, model, B, _ = case
    eng, y, idx = dc.irt1d_amort_engine(case, CPU, OracleBackend())
    _irt_case_on_the_oracle(tag, eng, y, idx, dc.irt_spec(model, 1, len(y), y.shape[1], True), dc.IRT1D_SEED)


@pytest.mark.parametrize("case", dc.MVN_AMORT, ids=[c[0] for c in dc.MVN_AMORT])
def test_mvn_amortized_cases_on_the_oracle(case):
    tag, dname, D, H, model, B, slopes, _ = case
    eng, y, idx = dc.mvn_amort_engine(case, CPU, OracleBackend())
    zmax = _irt_case_on_the_oracle(tag, eng, y, idx, dc.irt_spec(model, D, len(y), y.shape[1], True), dc.MVN_SEED)[3]
    assert slopes != "small" or zmax < 15.0


@pytest.mark.parametrize("case", dc.MVN_BBVI, ids=[c[0] for c in dc.MVN_BBVI])
def test_mvn_bbvi_cases_on_the_oracle(case):
    tag, dname, D, share, B, _ = case
    eng, y, idx = dc.mvn_bbvi_engine(case, CPU, OracleBackend())
    _irt_case_on_the_oracle(tag, eng, y, idx, dc.irt_spec("irt_2pl", D, len(y), y.shape[1], False, share), dc.BBVI_SEED)


def _cdm_probabilities_clear_of_the_clamp(params):
    """The CDMs' response probabilities are 1 - s or g: far from eps32 and 1 - eps32 whatever the pattern."""
    for n in ("g", "s"):
        p = vo.sigmoid(params[n])
        assert p.min() > 1e-3 and p.max() < 1 - 1e-3


@pytest.mark.parametrize("case", dc.HODINA + dc.CCDM + dc.VAECCDM, ids=[c[0] for c in dc.HODINA + dc.CCDM + dc.VAECCDM])
def test_enumerated_cdm_cases_on_the_oracle(case):
    builder = dc.hodina_engine if case in dc.HODINA else (dc.ccdm_engine if case in dc.CCDM else dc.vaeccdm_engine)
    eng, y, idx, spec = builder(case, CPU, OracleBackend())
    params = dc.params_of(eng)
    _cdm_probabilities_clear_of_the_clamp(params)
    eps = vo.philox_normals(dc.HODINA_SEED, 0, 0, idx, 1) if case in dc.HODINA else None
    loss, g = vo.loss_and_grads(spec, params, y, [idx], [eps])
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in g.values())
    if case not in dc.VAECCDM:        # (VaeCCDM keeps the reference's -1 of a missing cell as an OBSERVATION, vi.py:882-891)
        for j in dc.design(case[1])[1]["unanswered_items"]:
            assert g["g"][..., j] == 0.0 and g["s"][..., j] == 0.0


@pytest.mark.parametrize("case", dc.CDM_SF, ids=[c[0] for c in dc.CDM_SF])
def test_cdm_sf_cases_on_the_oracle(case):
    tag, dname, K, cdm, B, amort, H, baseline, _ = case
    eng, y, idx, spec = dc.cdm_sf_engine(case, CPU, OracleBackend())
    params, attr, near = dc.cdm_sf_draws(eng, y, idx, K, amort)
    assert not near.any()                                     # no draw on its threshold: nothing needs to be left out
    _cdm_probabilities_clear_of_the_clamp(params)
    loss, g, lr = vo.cdm_sf_particle(spec, params, y, idx, attr)
    assert np.isfinite(loss) and np.isfinite(lr).all() and all(np.isfinite(v).all() for v in g.values())
