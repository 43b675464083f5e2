"""pair_tables / ld_x2, the parts that need no GPU: the declarations and the argument gate of vx_pair_tables, the host formulas
of pair_x2_host against a pair-by-pair restatement, its symmetry, NaN and ordering rules, the planted pair on tables made by
numpy, the share of pairs each case keeps under the comparison condition, and the operand phase said again in numpy against the
float64 oracle of tests/x2_cases.py -- which must stay below half the constant the GPU is held to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ld_cases as ld
from tests import x2_cases as xc
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("x2", "g2", "z", "p", "sign", "phi_obs", "phi_exp")


# ---- declarations and the gate ---------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9 and _hip.lib().vx_abi_version() == 9
    for name, nargs, res in (("vx_pair_tables_workspace_ints", 2, ctypes.c_int64), ("vx_pair_tables_chunks", 2, ctypes.c_int64),
                             ("vx_pair_tables", 11, ctypes.c_int)):
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")) == nargs, name
        assert len(_hip.SIGNATURES[name][1]) == nargs and _hip.SIGNATURES[name][0] is res, name
        assert (m.group(1) == "int64_t") == (res is ctypes.c_int64), name
    # pointers go through as void*: the ABI fuzz hands every entry null and host pointers
    args = _hip.SIGNATURES["vx_pair_tables"][1]
    assert args == [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    assert "2^31 - 1" in header                                     # how far the counts are exact


def test_size_queries_answer_without_a_gpu():
    """No workspace as built; the chunks of a call are those of the plan: stages of 128 persons, at most 256 workgroups over the
    pairs of 128-item groups; shapes beyond the limits answer -1."""
    from vipsy_amd import _hip
    L = _hip.lib()
    for J in (1, 31, 32, 33, 70, 128, 129, 500, 1024):
        groups = (J + 127) // 128
        n_bp = groups * (groups + 1) // 2
        for nb in (1, 127, 128, 129, 200, 5000, 1000000, 2 ** 24 + 3, 2 ** 31 - 1):
            assert L.vx_pair_tables_workspace_ints(nb, J) == 0
            stages = (nb + 127) // 128
            want = min(stages, max(1, 256 // n_bp))
            per = (stages + want - 1) // want
            assert L.vx_pair_tables_chunks(nb, J) == (stages + per - 1) // per, (nb, J)
    assert L.vx_pair_tables_chunks(128, 70) == 1 and L.vx_pair_tables_chunks(129, 70) == 2
    for J in (0, -1, 1025, 1 << 20):
        assert L.vx_pair_tables_workspace_ints(100, J) == -1 and L.vx_pair_tables_chunks(100, J) == -1
    for nb in (0, -7, 2 ** 31, 1 << 40):
        assert L.vx_pair_tables_workspace_ints(nb, 37) == -1 and L.vx_pair_tables_chunks(nb, 37) == -1


def test_the_gate_refuses_one_wrong_argument_at_a_time():
    """Host buffers, no GPU: every call must come back with -1 before the HIP runtime is touched."""
    from vipsy_amd import _hip
    L = _hip.lib()
    host = (ctypes.c_int32 * 4096)()
    p = ctypes.cast(host, ctypes.c_void_p)
    good = dict(y=p, rows=None, nb=100, J=37, n11=p, n10=p, n01=p, n00=p, ws=None, ws_ints=0, stream=None)
    order = ("y", "rows", "nb", "J", "n11", "n10", "n01", "n00", "ws", "ws_ints", "stream")
    wrong = [("y", None), ("n11", None), ("n10", None), ("n01", None), ("n00", None), ("nb", 0), ("nb", -1), ("nb", 2 ** 31),
             ("nb", 1 << 40), ("J", 0), ("J", -3), ("J", 1025), ("ws_ints", -1)]
    for key, value in wrong:
        a = dict(good)
        a[key] = value
        assert L.vx_pair_tables(*[a[k] for k in order]) == -1, (key, value)


def test_model_classes_have_the_methods():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, HipBackend, IrtEngine, _EngineBase
    for name in ("pair_tables", "ld_x2"):
        assert callable(getattr(vi.BasePsy, name))
        assert getattr(IrtEngine, name) is not getattr(_EngineBase, name) and getattr(CcdmEngine, name) is not getattr(_EngineBase, name)
    for doc in (vi.BasePsy.ld_x2.__doc__, IrtEngine.ld_x2.__doc__):
        doc = " ".join(doc.split())
        for words in ("as they stand", "ESTIMATED", "up to 3 degrees", "approximate in any case", "missing completely at random",
                      "Not built: polytomous tables, covariates= / at=, M2, more than one rank"):
            assert words in doc, words
    for name in ("pair_tables", "pair_tables_workspace", "pair_tables_chunks"):
        assert callable(getattr(HipBackend, name))


# ---- the host formulas -----------------------------------------------------------------------------------------------------
def _tiny(seed=3, J=6, G=7, n=60):
    """A tiny problem with every special cell: pair (0, 1) has a zero cell, item 2 was answered by 5 persons (below min_pairs),
    item 3 is nearly always right (an E below min_expected), item 4 is always right (phi undefined), item 5 nobody answered."""
    rng = np.random.RandomState(seed)
    p1 = rng.uniform(0.2, 0.8, size=(J, G))
    p1[3], p1[4] = 0.995, 0.97
    y = (rng.uniform(size=(n, J)) < p1[:, rng.randint(0, G, size=n)].T).astype(np.uint8)
    y[(y[:, 0] == 1) & (y[:, 1] == 0), 1] = 1                       # n10[0][1] = 0
    y[5:, 2] = 255
    y[:, 4] = 1
    y[:, 5] = 255
    y[rng.uniform(size=y.shape) < 0.1] = 255
    y[:5, 2] = rng.randint(0, 2, size=5)
    return y, p1, 1.0 - p1, np.log(rng.dirichlet(np.ones(G)))


@pytest.mark.parametrize("min_pairs,min_expected", [(8, 1.0), (1, 1e-9), (20, 3.0)])
def test_pair_x2_host_against_the_loop_over_pairs(min_pairs, min_expected):
    from vipsy_amd.grid import chi2_sf, pair_x2_host
    y, p1, p0, logw = _tiny()
    t = xc.tables(y)
    assert t["n10"][0, 1] == 0 and t["n11"][2, 2] + t["n00"][2, 2] == 5 and t["n00"][4, 4] == 0 and t["n11"][5].sum() == 0
    got = pair_x2_host(t["n11"], t["n10"], t["n01"], t["n00"], p1, p0, logw, min_pairs, min_expected)
    x2, g2, sign = xc.stats_loop(t, p1, p0, logw, min_pairs, min_expected)
    assert np.array_equal(np.isnan(got["x2"]), np.isnan(x2)) and np.array_equal(np.isnan(got["g2"]), np.isnan(x2))
    ok = ~np.isnan(x2)
    assert ok.sum() >= (2 if min_pairs > 1 else 10)
    assert np.allclose(got["x2"][ok], x2[ok], rtol=1e-12, atol=0) and np.allclose(got["g2"][ok], g2[ok], rtol=1e-11, atol=1e-13)
    assert np.array_equal(got["sign"], sign)
    assert np.allclose(got["z"][ok], (x2[ok] - 1) / np.sqrt(2), rtol=1e-12) and np.isnan(got["z"][~ok]).all()
    assert np.allclose(got["p"][ok], [chi2_sf(v, 1) for v in got["x2"][ok]], rtol=1e-12, atol=0) and np.isnan(got["p"][~ok]).all()
    N = t["n11"] + t["n10"] + t["n01"] + t["n00"]
    assert got["n_pairs"].dtype == np.int64 and np.array_equal(got["n_pairs"], N)
    assert got["expected"].shape == (2, 2, 6, 6) and np.allclose(got["expected"].sum((0, 1)), N, rtol=1e-13)
    if min_pairs == 8:
        # the rules, one by one: the diagonal, a pair below min_pairs, an E below min_expected, an item nobody answered
        assert np.isnan(np.diag(got["x2"])).all()
        assert N[0, 2] < 8 and np.isnan(got["x2"][0, 2]) and got["sign"][0, 2] == 0
        assert N[0, 3] >= 8 and got["expected"][:, :, 0, 3].min() < 1.0 and np.isnan(got["x2"][0, 3])
        assert np.isnan(got["x2"][5]).all() and np.isnan(got["phi_obs"][5]).all() and (got["sign"][5] == 0).all()
        assert np.isfinite(got["x2"][0, 1]) and np.isfinite(got["g2"][0, 1])                  # the zero cell: 0 ln 0 = 0
    if min_pairs == 1:
        # item 4 is always right: its observed phi is undefined and the sign is 0, with x2 finite
        assert np.isfinite(got["x2"][0, 4]) and np.isnan(got["phi_obs"][0, 4]) and got["sign"][0, 4] == 0
        assert np.isfinite(got["phi_exp"][0, 4])


def test_symmetry_bit_for_bit():
    from vipsy_amd.grid import pair_x2_host
    for kind, case in xc.ALL[:2] + xc.ALL[-1:]:
        cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
        p1, p0, logw = xc.restated_probs(kind, cs)
        got = pair_x2_host(o["n11"], o["n10"], o["n01"], o["n00"], p1, p0, logw)
        for k in STATS + ("n_pairs",):
            assert np.array_equal(got[k], got[k].T, equal_nan=True), (case[0], k)
        E = got["expected"]
        assert np.array_equal(E[1, 0], E[0, 1].T) and np.array_equal(E[1, 1], E[1, 1].T) and np.array_equal(E[0, 0], E[0, 0].T)


@pytest.mark.parametrize("key,value", [("min_pairs", 0), ("min_pairs", True), ("min_expected", 0.0), ("min_expected", float("nan"))])
def test_bad_thresholds_and_shapes_are_refused(key, value):
    from vipsy_amd.grid import pair_x2_host
    y, p1, p0, logw = _tiny()
    t = xc.tables(y)
    with pytest.raises(ValueError):
        pair_x2_host(t["n11"], t["n10"], t["n01"], t["n00"], p1, p0, logw, **{key: value})
    with pytest.raises(ValueError):
        pair_x2_host(t["n11"], t["n10"][:5], t["n01"], t["n00"], p1, p0, logw)
    with pytest.raises(ValueError):
        pair_x2_host(t["n11"], t["n10"], t["n01"], t["n00"], p1, p0[:, :6], logw)


def test_top_ordering_with_ties():
    from vipsy_amd.grid import pair_x2_top
    x2 = np.full((5, 5), np.nan)
    sign = np.zeros((5, 5))
    for (j, k), v, s in (((0, 1), 2.0, 1), ((0, 3), 7.0, -1), ((1, 2), 7.0, 1), ((2, 4), 0.5, -1), ((3, 4), 7.0, 1)):
        x2[j, k] = x2[k, j] = v
        sign[j, k] = sign[k, j] = s
    out = pair_x2_top(x2, sign, top=4)
    assert out["item_j"].dtype == np.int64 and out["item_k"].dtype == np.int64
    assert list(zip(out["item_j"], out["item_k"])) == [(0, 3), (1, 2), (3, 4), (0, 1)]          # ties: the lower pair first
    assert out["value"].tolist() == [7.0, 7.0, 7.0, 2.0] and out["sign"].tolist() == [-1, 1, 1, 1]
    assert len(pair_x2_top(x2, sign, top=20)["value"]) == 5 and len(pair_x2_top(x2, sign, top=0)["value"]) == 0
    assert len(pair_x2_top(np.full((3, 3), np.nan), np.zeros((3, 3)))["value"]) == 0


def test_the_planted_pair_comes_first_on_tables_made_by_numpy():
    from vipsy_amd.grid import pair_x2_host, pair_x2_top
    kind, case = "irt", ld.PLANTED
    cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
    got = pair_x2_host(o["n11"], o["n10"], o["n01"], o["n00"], *xc.probs(kind, cs))
    top = pair_x2_top(got["x2"], got["sign"], 20)
    print("planted: x2[0][1] %.1f sign %+d, next %.2f; phi_obs %.3f phi_exp %.3f" % (top["value"][0], top["sign"][0], top["value"][1],
                                                                                    got["phi_obs"][0, 1], got["phi_exp"][0, 1]))
    assert (top["item_j"][0], top["item_k"][0]) == (0, 1) and top["sign"][0] == 1
    assert top["value"][0] > 20 * top["value"][1] and got["p"][0, 1] < 1e-100
    assert got["phi_obs"][0, 1] > got["phi_exp"][0, 1] + 0.5


# ---- the cases: what the condition keeps, what the method costs ------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", xc.ALL, ids=xc.ALL_IDS)
def test_share_of_pairs_under_the_comparison_condition(kind, case):
    """A GPU comparison on the pairs of the condition compares something: at least KEEP_MIN of the off-diagonal pairs, or the
    case is listed as tables only -- and a case so listed is one the condition does cut below that."""
    o = xc.oracle(kind, case)
    J = case[2]
    assert o["keep"].sum() == int(round(o["share"] * J * (J - 1))) and not o["keep"][np.arange(J), np.arange(J)].any()
    assert np.array_equal(o["keep"], (o["N"] >= 8) & (o["E"] >= 1.0).all((0, 1)) & ~np.eye(J, dtype=bool))
    print("%s: the condition keeps %.3f of %d off-diagonal pairs" % (case[0], o["share"], J * (J - 1)))
    if case[0] in xc.TABLES_ONLY:
        assert o["share"] < xc.KEEP_MIN
    else:
        assert o["share"] >= xc.KEEP_MIN
    assert ld.LEFT_OUT_CAP.get("case4_3pl_j500_sparse", 0.0) is None and "case4_3pl_j500_sparse" in xc.TABLES_ONLY
    # the condition is the NaN rule of pair_x2_host at its defaults, on the oracle's own probabilities
    from vipsy_amd.grid import pair_x2_host
    got = pair_x2_host(o["n11"], o["n10"], o["n01"], o["n00"], *xc.probs(kind, xc.case_of(kind, case)))
    assert np.array_equal(~np.isnan(got["x2"]), o["keep"])


def _every_model_is_compared_on_x2():
    compared = {c[3] for k, c in xc.ALL if k == "irt" and c[0] not in xc.TABLES_ONLY}
    assert {"irt_1pl", "irt_2pl", "irt_4pl"} <= compared and {c[4] for k, c in xc.ALL if k == "irt" and c[0] not in xc.TABLES_ONLY} == {1, 2, 3}
    assert any(k == "cdm" for k, _ in xc.ALL) and ld.PLANTED in [c for _, c in xc.ALL]


@pytest.mark.parametrize("kind,case", xc.ALL, ids=xc.ALL_IDS)
def test_the_restated_operand_phase_meets_half_the_constant(kind, case):
    """The fp16-pair image said again in numpy, through pair_x2_host, against the float64 oracle: the relative error of E and
    the x2 ratio of the bound, in units of 2^-24, both below REL_E / 2 -- and no larger than what x2_cases records."""
    from vipsy_amd.grid import pair_x2_host
    cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
    p1, p0, logw = xc.restated_probs(kind, cs)
    got = pair_x2_host(o["n11"], o["n10"], o["n01"], o["n00"], p1, p0, logw)
    rel_e, ratio = xc.ratios(o, got["x2"], got["expected"])
    print("%s: restated E %.2f, x2 ratio %.2f units of 2^-24 on %d pairs (the constant: %.0f)"
          % (case[0], rel_e / xc.UNIT, ratio / xc.UNIT, o["keep"].sum(), xc.REL_E / xc.UNIT))
    assert o["keep"].any()
    assert rel_e <= 0.5 * xc.REL_E and ratio <= 0.5 * xc.REL_E
    assert rel_e <= xc.RESTATED_MEASURED[0] * 1.01 * xc.UNIT and ratio <= xc.RESTATED_MEASURED[1] * 1.01 * xc.UNIT


def test_the_host_formulas_on_the_oracle_probabilities():
    """pair_x2_host fed the oracle's own float64 probabilities gives the oracle's statistics to float64 rounding; and the cases
    on which that is asked of the GPU cover every model that has its own tables, x_feature 1 to 3, a CDM and the planted pair."""
    from vipsy_amd.grid import pair_x2_host
    _every_model_is_compared_on_x2()
    kind, case = xc.ALL[1]
    cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
    got = pair_x2_host(o["n11"], o["n10"], o["n01"], o["n00"], *xc.probs(kind, cs))
    keep = o["keep"]
    assert np.array_equal(np.isnan(got["x2"]), o["bad"])
    assert np.allclose(got["x2"][keep], o["x2"][keep], rtol=1e-11) and np.allclose(got["g2"][keep], o["g2"][keep], rtol=1e-10, atol=1e-12)
    assert np.array_equal(got["sign"], o["sign"])
    assert np.allclose(got["phi_exp"], o["phi_exp"], rtol=1e-11, equal_nan=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


def test_classes_without_grid_scores_refuse():
    from tests import score_cases as sc
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VCHoDina, vi.VaeCCDM, vi.VCDM):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        for call in (m.pair_tables, m.ld_x2):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert type(m.engine).__name__ in str(e.value)


def test_refusals_of_ld_x2_are_those_of_score():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", x_feature=4, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        m.engine.score()
    with pytest.raises(NotImplementedError) as e:
        m.ld_x2()
    assert str(e.value) == str(want.value) and "x_feature" in str(e.value)
    ok = vi.VIRT(data=_y(), model="irt_3pl", backend=OracleBackend())
    for kw in ({"min_pairs": 0}, {"min_pairs": 2.5}, {"min_expected": 0}, {"min_expected": "1"}, {"top": -1}, {"nodes": 1}):
        with pytest.raises(ValueError):
            ok.ld_x2(**kw)
    for kw in ({"covariates": np.zeros((24, 1))}, {"at": "wle"}):
        with pytest.raises(NotImplementedError):
            ok.ld_x2(**kw)
    with pytest.raises(ValueError):
        ok.ld_x2(data=_y(j=11))
    with pytest.raises(ValueError):
        ok.pair_tables(data=_y(j=11))
    with pytest.raises(IndexError):
        ok.engine.pair_tables(rows=[0, 24])
