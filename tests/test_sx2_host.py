"""The summed-score layer without a GPU: the declarations and limits of the vx_sumscore_* entries (VX_EINVAL before the HIP runtime
is touched), the refusals of sx2() / sumscore_tables() / score_table(), the host functions (chi2_sf, sx2_host, score_table_host,
grid_image_probs) against the oracle of tests/sx2_cases.py, and the conditions the cases must meet in the float64 oracle alone:
the rule's own consistency, the collapse margins of every end-to-end case, and the statistical claim of the planted case."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import score_cases as sc
from tests import sx2_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- declarations and limits ---------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    from vipsy_amd import _hip
    header = open(os.path.join(ROOT, "include", "vipsy_amd.h")).read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("vx_sumscore_model_workspace_floats", 2), ("vx_sumscore_model", 11), ("vx_sumscore_persons", 8),
                         ("vx_sumscore_observed", 9)):
        m = re.search(r"\b(?:int|int64_t) %s\((.*?)\);" % name, bare, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(_hip.lib(), name)


def test_workspace_query_and_limits():
    from vipsy_amd import _hip
    q = _hip.lib().vx_sumscore_model_workspace_floats
    for Js, G in [(1, 1), (5, 1024), (70, 61), (500, 61), (1023, 3), (1023, 1024)]:
        n = q(Js, G)
        assert n > 0 and n % (2 * Js * (Js + 1)) == 0 and n // (2 * Js * (Js + 1)) <= G, (Js, G, n)      # whole slabs, a chunk >= 1 node
    assert q(1023, 1024) * 4 < 1 << 28                                            # the largest call: under 256 MB
    for Js, G in [(0, 5), (-1, 5), (1024, 5), (5, 0), (5, -3), (5, 1025)]:
        assert q(Js, G) == -1, (Js, G)


def test_entries_refuse_every_limit_before_the_runtime():
    """Host buffers stand in for the device's: every call below has to come back with VX_EINVAL without a launch."""
    from vipsy_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_float * 8192)()
    P = ctypes.cast(buf, ctypes.c_void_p)

    def model(Js=5, G=4, ws_floats=1 << 20, null=None):
        a = {k: P for k in ("p1", "p0", "logw", "e1", "e0", "ws")}
        if null:
            a[null] = None
        return L.vx_sumscore_model(a["p1"], a["p0"], a["logw"], Js, G, a["e1"], a["e0"], None, a["ws"], ws_floats, None)

    for k in ("p1", "p0", "logw", "e1", "e0", "ws"):
        assert model(null=k) == -1, k
    assert model(Js=0) == -1 and model(Js=1024) == -1 and model(G=0) == -1 and model(G=1025) == -1 and model(Js=-4) == -1
    assert model(ws_floats=L.vx_sumscore_model_workspace_floats(5, 4) - 1) == -1 and model(ws_floats=-1) == -1

    def persons(nb=10, J=8, Js=8, y=P, score=P):
        return L.vx_sumscore_persons(y, None, nb, J, None, Js, score, None)

    assert persons(y=None) == -1 and persons(score=None) == -1
    assert persons(nb=-1) == -1 and persons(J=0) == -1 and persons(J=4097) == -1 and persons(Js=0) == -1 and persons(Js=9) == -1
    assert persons(J=2000, Js=1024) == -1

    def observed(nb=10, J=8, Js=8, y=P, rows=P, score=P, o1=P):
        return L.vx_sumscore_observed(y, rows, nb, J, None, Js, score, o1, None)

    assert observed(y=None) == -1 and observed(rows=None) == -1 and observed(score=None) == -1 and observed(o1=None) == -1
    assert observed(nb=-1) == -1 and observed(J=0) == -1 and observed(Js=0) == -1 and observed(Js=9) == -1
    assert observed(J=2000, Js=1024) == -1


# ---- the refusals of the public methods --------------------------------------------------------------------------------------
def _virt(model="irt_2pl", x_feature=1, n=24, J=12):
    from tests.oracle_backend import OracleBackend
    from vipsy_amd import vi
    vi.clear_param_store()
    y = torch.from_numpy((np.random.RandomState(2).uniform(size=(n, J)) < 0.5).astype(np.uint8))
    return vi.VIRT(data=y, model=model, x_feature=x_feature, backend=OracleBackend())


def test_refusals():
    from tests.oracle_backend import OracleBackend
    from vipsy_amd import vi
    m = _virt()
    for call in (m.sx2, m.sumscore_tables, m.score_table, m.engine.sx2, m.engine.sumscore_tables, m.engine.score_table):
        for bad in ([3, 2], [2, 2], [0, 12], [-1, 3], [], [0.5, 1.5], [[0, 1]]):
            with pytest.raises(ValueError, match="items must be"):
                call(items=bad)
        with pytest.raises(NotImplementedError, match="covariates"):
            call(covariates=np.zeros((24, 1)))
        with pytest.raises(NotImplementedError, match="rows=.*as data"):
            call(rows=[0, 1, 2])
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1", True):
        for call in (m.sx2, m.engine.sx2):
            with pytest.raises(ValueError, match="min_expected"):
                call(min_expected=bad)
    # more than 1 023 items: refused with the way out
    big = _virt(J=1030, n=8)
    with pytest.raises(NotImplementedError, match="at most 1023 items.*items="):
        big.sx2()
    with pytest.raises(NotImplementedError, match="at most 1023 items"):
        big.score_table()
    # x_feature > 3 and the classes score() refuses: score()'s own words
    m4 = _virt(x_feature=4)
    with pytest.raises(NotImplementedError) as want:
        m4.engine.score()
    for call in (m4.sx2, m4.sumscore_tables, m4.score_table):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == str(want.value)
    rng = np.random.RandomState(2)
    q = torch.from_numpy(sc.cdm_q(3, 12, rng))
    y = torch.from_numpy((rng.uniform(size=(24, 12)) < 0.5).astype(np.uint8))
    vi.clear_param_store()
    h = vi.VCHoDina(data=y, q=q, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        h.score()
    for call in (h.sx2, h.sumscore_tables, h.score_table):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == str(want.value)
    # more than one rank
    m = _virt()
    m.world = 2
    for call in (m.sx2, m.sumscore_tables, m.score_table):
        with pytest.raises(NotImplementedError, match="2 ranks"):
            call()
    for name in ("sx2", "sumscore_tables", "score_table"):
        assert getattr(vi.BasePsy, name).__doc__ and "rank" in getattr(vi.BasePsy, name).__doc__


def test_free_parameters_of_an_item():
    for model, D, want in (("irt_1pl", 1, 1), ("irt_2pl", 1, 2), ("irt_3pl", 1, 3), ("irt_4pl", 1, 4)):
        m = _virt(model=model, x_feature=D)
        assert m.engine._sx2_params(np.arange(12)).tolist() == [want] * 12, model
    m = _virt(x_feature=2)                                                      # the default a_free of two dimensions
    free = (m.engine.unconstrained("a", m.engine.free).cpu().numpy() != 0).sum(0)
    assert free.min() == 1 and free.max() == 2
    assert m.engine._sx2_params(np.array([0, 5, 11])).tolist() == (1 + free[[0, 5, 11]]).tolist()


# ---- the host functions --------------------------------------------------------------------------------------------------
def test_chi2_sf():
    from vipsy_amd.grid import chi2_sf
    # the 5 % points of the tables, and the exponential of df = 2
    for x, df in ((3.841458820694124, 1), (5.991464547107979, 2), (7.814727903251179, 3), (16.918977604620448, 9),
                  (18.307038053275146, 10), (124.34211340400407, 100), (125.4584, 101)):
        assert abs(chi2_sf(x, df) - 0.05) < 2e-7, (x, df)
    assert chi2_sf(0.0, 1) == 1.0 and chi2_sf(0.0, 4) == 1.0 and chi2_sf(3.0, 2) == math.exp(-1.5)
    for x in (0.0, 1e-3, 0.7, 5.0, 28.0, 120.0, 908.0):
        for df in list(range(1, 13)) + [57, 58, 499, 500]:
            got, want = chi2_sf(x, df), xc.chi2_tail(x, df)
            assert abs(got - want) <= 1e-12 * want + 1e-300, (x, df, got, want)
    assert 0.0 < chi2_sf(908.0, 9) < 1e-180
    # a large statistic over many cells: the finite sum passes the range of float64 while exp(-x / 2) leaves it at the other end;
    # the tail is tiny or 0, never 1 and never NaN
    for x, df in ((1e4, 400), (1e4, 401), (4.5e5, 402), (4.5e5, 401), (5300.0, 400), (2e4, 1001), (2e4, 1000)):
        assert chi2_sf(x, df) == 0.0 == xc.chi2_tail(x, df), (x, df)
    for x, df in ((1400.0, 400), (1400.0, 401), (3000.0, 1000), (3000.0, 1001), (600.0, 500), (600.0, 499)):
        got, want = chi2_sf(x, df), xc.chi2_tail(x, df)
        assert 0.0 < got < 1.0 and abs(got - want) <= 1e-11 * want, (x, df, got, want)
    for df in (400, 401, 1000, 1001):                                            # far below the mean: the tail is 1 to the last bit or so
        assert 1.0 - 1e-12 <= chi2_sf(0.3 * df, df) <= 1.0, df
    for x, df in ((1.0, 0), (1.0, -2), (-1.0, 3), (float("nan"), 3), (float("inf"), 3)):
        assert math.isnan(chi2_sf(x, df)), (x, df)


def test_the_oracles_tables_rounded_to_float32_meet_the_rule_at_a_third():
    """What the rule asks is at least three times what float32 storage alone costs, on every case; and the identities of the
    definitions hold in the oracle."""
    for case in xc.MODEL_CASES:
        cs = xc.model_case(case)
        o, Js, G = cs["oracle"], cs["Js"], cs["G"]
        for k in ("e1", "e0", "dist"):
            assert xc.table_ratio(o[k].astype(np.float32), o[k], Js, G) <= xc.SX2_C / 3.0, (case[0], k)
        tot = o["e1"] + o["e0"]
        assert np.allclose(tot, tot[0][None, :], rtol=1e-12, atol=1e-300), case[0]           # P(score = s), whichever item is left out
        assert np.allclose(tot[0], o["w"] @ o["dist"], rtol=1e-12, atol=1e-300), case[0]
        assert (o["e1"][:, 0] == 0).all() and (o["e0"][:, Js] == 0).all(), case[0]
        if cs["binomial"] is not None:
            want = xc.binomial_row(Js, xc.BINOMIAL_P, 1.0 - xc.BINOMIAL_P)
            assert np.allclose(o["dist"][cs["binomial"]], want, rtol=1e-9, atol=1e-250), case[0]    # (0.3^1023 leaves float64)
        if cs["sure"] is not None:
            rest = np.arange(G) != cs["binomial"]
            assert (o["dist"][rest, 0] == 0).all() and (o["dist"][rest, Js] == 0).all(), case[0]
    assert 2 * xc.SX2_MEASURED <= xc.SX2_C < 4 * xc.SX2_MEASURED                  # the next power of two above twice the measured
    assert math.log2(xc.SX2_C) == int(math.log2(xc.SX2_C))


def _end_to_end_tables():
    """(tag, e1, e0, o1, n, n_params) of every end-to-end case of tests/test_gpu_sx2.py, from float64 probabilities."""
    cs = xc.planted_case()
    p1, p0, _, logw = xc.irt_probs(cs)
    lw, o1, n, _ = xc.host_tables(cs["y"], None, p1, p0, logw)
    yield "planted", lw["e1"], lw["e0"], o1, n, cs["n_params"]
    cs = xc.booklet_case()
    for b, items in enumerate(cs["booklets"]):
        p1, p0, _, logw = xc.irt_probs(cs, items)
        lw, o1, n, _ = xc.host_tables(cs["y"], items, p1, p0, logw)
        yield "booklet %d" % b, lw["e1"], lw["e0"], o1, n, cs["n_params"][items]
    cs = sc.cdm_case(xc.DINA_CASE)
    from oracle import vi_oracle as vo
    eta, _ = vo.dina_eta(cs["K"], cs["q"].astype(np.float64))                                # [2^K][J]
    g, s = vo.sigmoid(cs["params"]["g"].astype(np.float64)), vo.sigmoid(cs["params"]["s"].astype(np.float64))
    p1 = np.where(eta > 0, 1.0 - s, g).T
    logw = np.full(2 ** cs["K"], -math.log(2 ** cs["K"]))
    lw, o1, n, _ = xc.host_tables(cs["y"], None, p1, 1.0 - p1, logw)
    yield "dina", lw["e1"], lw["e0"], o1, n, np.full(cs["J"], 2, np.int64)


def test_sx2_host_against_the_oracle_and_the_cases_conditions():
    """sx2_host equals the cell-by-cell oracle on every end-to-end case; in the oracle no sweep decision of any item of any case
    hangs on a count within 1e-3 of min_expected; the planted item stands out by more than 20 times."""
    from vipsy_amd.grid import sx2_host
    for tag, e1, e0, o1, n, k in _end_to_end_tables():
        for min_expected in (1.0, 5.0):
            want = xc.sx2_oracle(e1, e0, o1, n, k, min_expected)
            got = sx2_host(e1, e0, o1, n, k, min_expected)
            assert np.array_equal(got["n_cells"], want["n_cells"]) and np.array_equal(got["df"], want["df"]), (tag, min_expected)
            assert np.allclose(got["sx2"], want["sx2"], rtol=1e-11, atol=0), (tag, min_expected)
            assert np.allclose(got["p"], want["p"], rtol=1e-9, atol=1e-300, equal_nan=True), (tag, min_expected)
            assert (want["n_cells"] >= 1).all() and n.sum() > 0, tag
            if min_expected == 1.0:                                             # the setting the GPU tests use
                print("%s: smallest collapse margin %.3g, S-X2 %s" % (tag, want["margin"].min(), np.round(want["sx2"], 1)))
                assert (want["margin"] > xc.COLLAPSE_MARGIN).all(), (tag, want["margin"])
        keep = n > 0
        assert np.allclose(got["observed"][:, keep], o1[:, keep] / n[keep]) and np.isnan(got["observed"][:, ~keep]).all(), tag
        assert np.isnan(got["expected"][:, ~keep]).all(), tag
        pos = keep[None, :] & (e1 + e0 > 0)
        assert np.allclose(got["expected"][pos], (e1 / np.where(e1 + e0 > 0, e1 + e0, 1.0))[pos], rtol=1e-13, atol=0), tag
        assert (got["expected"][keep[None, :] & ~(e1 + e0 > 0)] == 0).all(), tag
    cs = xc.planted_case()
    tag, e1, e0, o1, n, k = next(_end_to_end_tables())
    want = xc.sx2_oracle(e1, e0, o1, n, k, 1.0)
    clean = np.delete(want["sx2"], xc.PLANTED_ITEM)
    print("planted item: S-X2 %.1f on %d df; the clean items at most %.1f" % (want["sx2"][xc.PLANTED_ITEM], want["df"][xc.PLANTED_ITEM],
                                                                            clean.max()))
    assert want["sx2"][xc.PLANTED_ITEM] > 20.0 * clean.max()
    assert want["p"][xc.PLANTED_ITEM] < 1e-20
    assert cs["y"].max() <= 1


def test_sx2_host_edges():
    from vipsy_amd.grid import sx2_host
    # one item: no score group between 0 and Js, no cell, no test
    out = sx2_host(np.array([[0.0, 0.4]]), np.array([[0.6, 0.0]]), np.array([[0, 7]]), np.array([5, 7]), [1])
    assert out["n_cells"].tolist() == [0] and out["sx2"].tolist() == [0.0] and out["df"].tolist() == [-1] and np.isnan(out["p"]).all()
    # two items: one group, the only cell, closed or not
    e1 = np.array([[0.0, 0.2, 0.3], [0.0, 0.1, 0.3]])
    e0 = np.array([[0.2, 0.3, 0.0], [0.2, 0.4, 0.0]])
    out = sx2_host(e1, e0, np.array([[0, 3, 4], [0, 1, 4]]), np.array([2, 10, 4]), [1, 1], min_expected=100.0)
    assert out["n_cells"].tolist() == [1, 1] and out["df"].tolist() == [0, 0] and np.isnan(out["p"]).all()
    assert np.allclose(out["sx2"], [(3 - 4.0) ** 2 / 4 + (3 - 4.0) ** 2 / 6, (1 - 2.0) ** 2 / 2 + (1 - 2.0) ** 2 / 8])
    with pytest.raises(ValueError):
        sx2_host(e1, e0, np.zeros((2, 3)), np.zeros(3), [1, 1], min_expected=0.0)
    with pytest.raises(ValueError):
        sx2_host(e1, e0, np.zeros((2, 3)), np.zeros(3), [1, 1], min_expected=True)


def test_a_gross_misfit_on_many_cells_gets_p_zero_not_one():
    """A million persons, 420 items: item 0 is answered right by everybody where the model expects a half -- a statistic of the
    order of 1e6 on some 400 df, whose tail has left float64: p is 0 (and not 1, and not NaN); a fitting item keeps a p inside (0, 1)."""
    from vipsy_amd.grid import sx2_host
    Js = 420
    rng = np.random.RandomState(9)
    prob = np.exp(-0.5 * ((np.arange(Js + 1) - Js / 2) / 30.0) ** 2)
    prob /= prob.sum()
    E = np.clip(np.arange(Js + 1) / Js, 0.0, 1.0)
    e1 = np.tile(prob * E, (Js, 1))
    e0 = np.tile(prob * (1.0 - E), (Js, 1))
    e1[:, 0], e0[:, Js] = 0.0, 0.0
    n = np.round(1e6 * prob)
    o1 = np.tile(rng.binomial(n.astype(np.int64), E), (Js, 1)).astype(np.float64)
    o1[0] = n                                                                  # everybody right on item 0
    out = sx2_host(e1, e0, o1, n, np.full(Js, 2), 1.0)
    assert out["sx2"][0] > 1e5 and out["df"][0] > 200 and out["p"][0] == 0.0, (out["sx2"][0], out["df"][0], out["p"][0])
    assert 0.0 < out["p"][1] < 1.0 and np.isfinite(out["p"]).all()
    with pytest.raises(ValueError):
        sx2_host(e1, e0, np.zeros((2, 2)), np.zeros(3), [1, 1])


def test_score_table_host_against_the_oracle():
    from vipsy_amd.grid import score_table_host
    cs = xc.planted_case()
    p1, p0, theta, logw = xc.irt_probs(cs)
    dist = xc.lord_wingersky(p1, p0, logw)["dist"]
    got, want = score_table_host(dist, logw, theta), xc.score_table_oracle(dist, logw, theta)
    for k in ("prob", "eap", "psd"):
        assert np.allclose(got[k], want[k], rtol=1e-11, atol=1e-13), k
    assert abs(got["prob"].sum() - 1.0) < 1e-12 and got["score"].tolist() == list(range(13))
    assert (np.diff(got["eap"][:, 0]) > 0).all()                                 # positive slopes: a higher score, a higher estimate


def test_grid_image_probs_reads_both_tables():
    """An image written element by element from the layout of vx_grid_table_* (k_grid_post.hip: [node tile][item chunk][T1 head, T1
    low, T0 head, T0 low][64 lanes][8 fp16], lane = node % 32 + 32 * (item % 16 // 8), element = item % 8, values T * 2^10): p1 is
    exp(T1) and equals grid_image_prob's, p0 is exp(T0) -- read from its own slots, with its low part, and not 1 - p1."""
    from vipsy_amd.grid import grid_image_prob, grid_image_probs
    J, G = 21, 37
    KC, NT = (J + 15) // 16, (G + 31) // 32
    rng = np.random.RandomState(4)
    img = np.zeros((NT, KC, 4, 64, 8), np.float16)
    parts = np.zeros((4, J, G))
    for j in range(J):
        for g in range(G):
            for slot in range(4):
                v = np.float16(rng.uniform(-8.0, 0.0) * 1024.0 if slot % 2 == 0 else rng.uniform(-0.25, 0.25))
                img[g // 32, j // 16, slot, g % 32 + 32 * (j % 16 // 8), j % 8] = v
                parts[slot, j, g] = float(v)
    p1, p0 = grid_image_probs(torch.from_numpy(img.reshape(-1)).view(torch.uint8), J, G)
    want1 = np.exp((parts[0] + parts[1]) / 1024.0).astype(np.float32)
    want0 = np.exp((parts[2] + parts[3]) / 1024.0).astype(np.float32)
    assert torch.equal(p1, grid_image_prob(torch.from_numpy(img.reshape(-1)).view(torch.uint8), J, G))
    assert np.array_equal(p1.numpy(), want1) and np.array_equal(p0.numpy(), want0) and p0.dtype == torch.float32
    assert not np.array_equal(want0, np.exp(parts[2] / 1024.0).astype(np.float32))       # (the low parts matter at float32)
    assert not np.allclose(p0.numpy(), 1.0 - p1.numpy())
