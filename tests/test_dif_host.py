"""The DIF layer without a GPU: the limits of vx_grid_counts_cond and its workspace query (VX_EINVAL before the HIP runtime is
touched), the refusals of dif() / group_counts(), the host functions (group_labels, group_fit_stats, group_fit_top) against the
oracle's, the conditions the cases of tests/dif_cases.py must meet, and the statistical claim in the float64 oracle alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import count_cases as cc
from tests import dif_cases as dc
from tests import em_cases as ec
from tests import score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- declarations and limits ---------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    from vipsy_amd import _hip
    header = open(os.path.join(ROOT, "include", "vipsy_amd.h")).read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("vx_grid_counts_cond_workspace_floats", 4), ("vx_grid_counts_cond", 18)):
        m = re.search(r"\b(?:int|int64_t) %s\((.*?)\);" % name, bare, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(_hip.lib(), name)
    assert "seg_start is HOST memory" in header                              # the contract of the segment table is stated


def test_workspace_query_limits_and_one_segment_is_the_unconditioned_plan():
    from vipsy_amd import _hip
    L = _hip.lib()
    q, q0 = L.vx_grid_counts_cond_workspace_floats, L.vx_grid_counts_workspace_floats
    for nb, J, G in [(1, 1, 1), (64, 37, 61), (2500, 37, 61), (100, 530, 61), (1 << 20, 500, 61)]:
        assert q(nb, 1, J, G) == q0(nb, J, G) + 8, (nb, J, G)                # gc_plan's slabs and the table of one segment: 4 int64
    slab = 2 * 37 * 61 + 61
    # every further segment may add two chunks, and its two table entries
    assert q(2500, 3, 37, 61) == q0(2500, 37, 61) + 4 * slab + 16
    assert q(1 << 20, 80, 500, 61) <= (256 + 2 * 79) * (2 * 500 * 61 + 61) + 4 * 81
    assert q(1 << 40, 4096, 1024, 1024) > 0                                   # int64 arithmetic
    for nb, S, J, G in [(0, 1, 37, 61), (-5, 1, 37, 61), (64, 0, 37, 61), (64, -1, 37, 61), (64, 4097, 37, 61), (64, 1, 1025, 61),
                        (64, 1, 37, 1025), (64, 1, 0, 61), (64, 1, 37, 0)]:
        assert q(nb, S, J, G) == -1, (nb, S, J, G)
    assert q(64, 4096, 37, 61) > 0


def test_entry_refuses_every_limit_before_the_runtime():
    """Host buffers stand in for the device's: every call below has to come back with VX_EINVAL without a launch."""
    from vipsy_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_float * 8192)()
    P = ctypes.cast(buf, ctypes.c_void_p)

    def call(nb=100, J=8, G=5, D=1, n_seg=2, seg=(0, 40, 100), null=None):
        s = np.asarray(seg, np.int64)
        ptrs = {k: P for k in ("y", "img", "logw", "coord", "tilt", "logjoint", "n1", "n0", "mass", "ws")}
        ptrs["seg"] = s.ctypes.data_as(ctypes.c_void_p)
        if null:
            ptrs[null] = None
        return L.vx_grid_counts_cond(ptrs["y"], None, nb, J, G, D, ptrs["img"], ptrs["logw"], ptrs["coord"], ptrs["tilt"],
                                     ptrs["logjoint"], ptrs["seg"], n_seg, ptrs["n1"], ptrs["n0"], ptrs["mass"], ptrs["ws"], None)

    for k in ("y", "img", "logw", "coord", "tilt", "logjoint", "seg", "n1", "n0", "mass", "ws"):
        assert call(null=k) == -1, k
    assert call(nb=0, seg=(0, 0, 0)) == -1 and call(nb=-1) == -1
    assert call(J=0) == -1 and call(J=1025) == -1 and call(G=0) == -1 and call(G=1025) == -1
    assert call(D=0) == -1 and call(D=4) == -1
    assert call(n_seg=0, seg=(0,)) == -1 and call(n_seg=-2) == -1
    assert call(n_seg=4097, seg=np.minimum(np.arange(4098), 100)) == -1
    assert call(seg=(1, 40, 100)) == -1                                       # seg_start[0] != 0
    assert call(seg=(0, 40, 99)) == -1 and call(seg=(0, 40, 101)) == -1       # seg_start[n_seg] != nb
    assert call(n_seg=3, seg=(0, 60, 40, 100)) == -1                          # decreasing
    assert call(n_seg=3, seg=(0, -1, 40, 100)) == -1


# ---- the refusals of dif() -----------------------------------------------------------------------------------------------
def _virt(model="irt_2pl", x_feature=1, n=24, J=12):
    from tests.oracle_backend import OracleBackend
    from vipsy_amd import vi
    vi.clear_param_store()
    y = torch.from_numpy((np.random.RandomState(2).uniform(size=(n, J)) < 0.5).astype(np.uint8))
    return vi.VIRT(data=y, model=model, x_feature=x_feature, backend=OracleBackend())


def test_dif_refusals():
    from tests.oracle_backend import OracleBackend
    from vipsy_amd import vi
    g = np.arange(24) % 2
    m = _virt()
    for call in (m.dif, m.group_counts, m.engine.dif, m.engine.group_counts):
        with pytest.raises(ValueError, match="integer labels"):
            call(g.astype(np.float64))
        with pytest.raises(ValueError, match="integer labels"):
            call(g.astype(bool))
        with pytest.raises(ValueError, match="2 .. 4096 groups"):
            call(np.zeros(24, np.int64))
        with pytest.raises(ValueError, match="labels, the scored rows"):
            call(g[:23])
        with pytest.raises(ValueError, match="impact must then be None or False"):
            call(g, covariates=np.zeros((24, 1)), impact=True)
        with pytest.raises(ValueError, match="fit_population"):
            call(g, covariates=np.zeros((24, 1)))
        with pytest.raises(ValueError, match="impact must be"):
            call(g, impact="yes")
    with pytest.raises(ValueError, match="min_obs"):
        m.dif(g, min_obs=0)
    with pytest.raises(ValueError, match="top"):
        m.dif(g, top=-1)
    with pytest.raises(ValueError, match="newton"):
        m.dif(g, refit=True, newton=0)
    # the refit is fit_em's M-step: 1PL / 2PL only, with its wording
    m3 = _virt(model="irt_3pl")
    with pytest.raises(NotImplementedError) as e:
        m3.dif(g, refit=True)
    with pytest.raises(NotImplementedError) as want:
        m3.fit_em()
    assert str(e.value).split(": ", 1)[1] == str(want.value).split(": ", 1)[1] and "irt_3pl" in str(e.value)
    # x_feature > 3 and the classes score() refuses: score()'s own words
    m4 = _virt(x_feature=4)
    with pytest.raises(NotImplementedError) as want:
        m4.engine.score()
    for call in (m4.dif, m4.group_counts):
        with pytest.raises(NotImplementedError) as e:
            call(g)
        assert str(e.value) == str(want.value)
    rng = np.random.RandomState(2)
    q = torch.from_numpy(sc.cdm_q(3, 12, rng))
    y = torch.from_numpy((rng.uniform(size=(24, 12)) < 0.5).astype(np.uint8))
    # VCCDM: no latent regression for patterns, no Newton refit (the classes without score(): tests/test_gpu_dif.py)
    vi.clear_param_store()
    c = vi.VCCDM(data=y, q=q, backend=OracleBackend())
    for kw in ({"impact": True}, {"covariates": np.zeros((24, 1))}, {"refit": True}):
        with pytest.raises(NotImplementedError, match="VCCDM|CcdmEngine"):
            c.dif(g, **kw)
    assert "reads" in vi.BasePsy.dif.__doc__ or "impact" in vi.BasePsy.dif.__doc__


# ---- the host functions --------------------------------------------------------------------------------------------------
def test_group_labels():
    from vipsy_amd.grid import group_labels
    g = np.array([7, -2, 7, 30, -2, 7, 30, 30, 30])
    labels, order, seg = group_labels(g, 9)
    assert labels.tolist() == [-2, 7, 30] and seg.tolist() == [0, 2, 5, 9] and order.dtype == np.int64 and seg.dtype == np.int64
    assert order.tolist() == [1, 4, 0, 2, 5, 3, 6, 7, 8]                      # stable: the persons of a group keep their order
    assert group_labels(torch.from_numpy(g), 9)[1].tolist() == order.tolist()
    assert group_labels(g.astype(np.uint8).tolist(), 9)[0].tolist() == [7, 30, 254]
    with pytest.raises(ValueError):
        group_labels(np.arange(4097), 4097)
    assert len(group_labels(np.arange(4096), 4096)[0]) == 4096


def test_group_statistics_match_the_oracle_formulas():
    from vipsy_amd.grid import group_fit_stats, group_fit_top, item_fit_stats
    want = dc.planted_oracle(False, min_obs=dc.PLANT_MIN_OBS)
    n1, n0 = want["n1"].copy(), want["n0"].copy()
    n1[1, 5] = 0.0
    n0[1, 5] = 0.0                                                           # an item nobody of group 1 answered
    ref = dc.group_stats(n1, n0, want["prob"], dc.PLANT_MIN_OBS)
    got = group_fit_stats(torch.from_numpy(n1), torch.from_numpy(n0), torch.from_numpy(want["prob"]), dc.PLANT_MIN_OBS)
    assert np.array_equal(np.rint(got["n_obs"].numpy()).astype(np.int64), ref["n_obs"]) and ref["n_obs"][1, 5] == 0
    for k in ("md", "rmsd", "observed"):
        assert got[k].dtype == torch.float64
        np.testing.assert_allclose(got[k].numpy(), ref[k], rtol=1e-12, atol=1e-15, equal_nan=True)
    few = ref["n_obs"] < dc.PLANT_MIN_OBS
    assert few.any() and (~few).any() and np.array_equal(np.isnan(ref["rmsd"]), few) and np.array_equal(np.isnan(got["md"].numpy()), few)
    # a group's statistics are item_fit_stats of its tables: the same bits
    one = item_fit_stats(torch.from_numpy(n1[0]), torch.from_numpy(n0[0]), torch.from_numpy(want["prob"]))
    assert torch.equal(one["observed"].nan_to_num(nan=-1.0), got["observed"][0].nan_to_num(nan=-1.0))
    top = group_fit_top(ref["rmsd"], 3)
    flat = np.where(np.isnan(ref["rmsd"]), -1.0, ref["rmsd"]).reshape(-1)
    best = np.argsort(-flat, kind="stable")[:3]
    assert (top["group"] * dc.PLANT_J + top["item"]).tolist() == best.tolist() and np.array_equal(top["value"], flat[best])
    assert len(group_fit_top(ref["rmsd"], 0)["value"]) == 0 and len(group_fit_top(ref["rmsd"], 99)["value"]) == int((~few).sum())


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_kernel_case_conditions():
    from vipsy_amd import _hip
    sizes = set()
    for key in dc.KCASES:
        cs = dc.kcase(key)
        seg = cs["seg_start"]
        assert seg[0] == 0 and seg[-1] == cs["N"] and (np.diff(seg) >= 0).all()
        assert sorted(cs["rows"].tolist()) == list(range(cs["N"])) and not np.array_equal(cs["rows"], np.arange(cs["N"]))
        assert cs["tilt"].shape == (cs["N"], cs["D"]) and cs["tilt"].dtype == np.float32 and np.abs(cs["tilt"]).max() > 0.5
        sizes |= set(np.diff(seg).tolist())
    assert {1, 31, 33, 255, 257, 600, 0} <= sizes
    k1 = dc.kcase("K1")["seg_start"]
    d = np.diff(k1)
    assert any(d[i] == 0 and 0 < i < len(d) - 1 and d[i - 1] > 0 and d[i + 1] > 0 for i in range(len(d)))     # empty, between two others
    assert any(0 < s % 32 and s // 32 == (s - 1) // 32 for s in k1[1:-1])                                   # a boundary inside a unit
    assert any(0 < s % 256 for s in k1[1:-1])                                                               # ... and inside a round
    # the last segment of K1 takes two chunks: the plan's rounds a chunk are the unconditioned plan's
    slab = 2 * 37 * 61 + 61
    chunks = _hip.lib().vx_grid_counts_workspace_floats(int(k1[-1]), 37, 61) // slab
    rpc = -(-(-(-int(k1[-1]) // 256)) // chunks)
    assert -(-1100 // 256) > rpc
    assert {dc.kcase(k)["D"] for k in dc.KCASES} == {1, 2, 3}
    assert {dc.kcase(k)["theta"].shape[0] for k in dc.KCASES} == {61, 33, 529}
    assert {dc.kcase(k)["J"] for k in dc.KCASES} == {1, 37, 300, 530}
    assert [-(-dc.kcase(k)["J"] // 32) for k in dc.BITWISE] == [2, 10, 17]                                  # IT = 1, 2, 4
    cs = dc.kcase("K1")
    assert (cs["y"][cs["rows"][dc.NO_RESPONSE["K1"]]] == 255).all()
    miss = {k: float((dc.kcase(k)["y"] == 255).mean()) for k in dc.KCASES}
    assert 0.85 < miss["K4"] < 0.95 and 0.25 < miss["K1"] < 0.35


@pytest.mark.parametrize("key", list(dc.KCASES))
def test_restatement_is_within_a_third_of_the_rule(key):
    err, rule = dc.krestated_error(key), dc.krule(key)
    print("%s: the method's own error %.3e, the rule %.3e" % (key, err, rule))
    assert 0 < err <= rule / 3.0
    want = dc.koracle(key)
    n = np.diff(dc.kcase(key)["seg_start"])
    assert np.abs(want["mass"].sum(1) - n).max() <= 1e-9 * max(n.max(), 1)    # the oracle's mass of a segment: its persons
    assert (want["n1"][n == 0] == 0).all() and (want["mass"][n == 0] == 0).all()


def test_planted_case_and_the_claim_in_the_oracle():
    cs = dc.planted()
    assert cs["y"].shape == (4096, 8) and set(np.unique(cs["groups"])) == set(dc.PLANT_LABELS.tolist())
    assert 0.18 < (cs["y"] == 255).mean() < 0.22 and 0.45 < cs["group"].mean() < 0.55
    a, b = dc.planted_oracle(True), dc.planted_oracle(False)
    clean = dc.clean_cells()
    figs = (a["rmsd"][clean].max(), a["rmsd"][dc.PLANT_GROUP, dc.PLANT_ITEM], b["rmsd"][clean].max(), b["rmsd"][dc.PLANT_GROUP, dc.PLANT_ITEM])
    print("clean max / planted with the groups' own priors: %.4f / %.4f; under N(0, I): %.4f / %.4f; t = %.3f" % (figs + (dc.PLANT_T,)))
    assert figs[0] < dc.PLANT_T < figs[2] and figs[1] > dc.PLANT_T
    assert dc.claim(a["rmsd"], b["rmsd"]) == (True, True, True)
    # t sits well inside the gap: no nearer than 0.015 to either clean maximum
    assert dc.PLANT_T - figs[0] > 0.015 and figs[2] - dc.PLANT_T > 0.015
    # the fitted private population finds the groups
    assert np.abs(a["group_mean"].ravel() - np.array([-0.75, 0.75])).max() < 0.06 and abs(a["sigma"][0, 0] - 0.64) < 0.05
    # min_obs: cells on both sides of PLANT_MIN_OBS, one of them exactly on it
    n_obs = a["n_obs"]
    assert (n_obs < dc.PLANT_MIN_OBS).any() and (n_obs > dc.PLANT_MIN_OBS).any() and (n_obs == dc.PLANT_MIN_OBS).any()
    assert np.array_equal(n_obs, np.stack([(cs["y"][cs["group"] == h] != 255).sum(0) for h in range(2)]))
    # the method's own error on this case, and of the refit through it in float32, against the rules the GPU is held to
    for o in (a, b):
        err = dc.restated_error(o, o["theta"], o["lw"], o["tilt"], o["y"], o["seg_start"])
        assert err <= dc.rule_of(err) / 3.0
    r = dc.restated(a["prob"], a["theta"], a["lw"], a["tilt"], a["y"], a["seg_start"])
    for newton in (1, 8):
        want = dc.planted_oracle(True, newton=newton)
        worst = 0.0
        for h in range(2):
            a32, b32 = ec.newton_mstep(cs["model"], a["theta"], cs["Dc"], r["n1"][h], r["n0"][h], cs["params"]["a"], cs["params"]["b"],
                                       np.ones((1, 8), bool), newton, dtype=np.float32)
            worst = max(worst, np.abs(a32 - want["a_group"][h]).max(), np.abs(b32[0] - want["b_group"][h]).max())
        print("refit, newton %d: the float32 restatement %.2e against the rule %.1e" % (newton, worst, dc.ROW_TOL))
        assert worst <= dc.ROW_TOL / 3.0
    # the planted shift comes back in delta_b of group 1 and nowhere else
    db = dc.planted_oracle(True, newton=8)["delta_b"]
    assert db[dc.PLANT_GROUP, dc.PLANT_ITEM] > 0.5 and np.abs(db[dc.clean_cells()]).max() < 0.25


def test_cdm_case():
    cs, want = dc.cdm_oracle(sc.CDM_CASES[0])
    assert want["labels"].tolist() == [-2, 3, 8] and np.diff(want["seg_start"]).tolist() == [34, 33, 33]
    assert want["n1"].shape == (3, cs["J"], 1 << cs["K"]) and np.isfinite(want["rmsd"]).any()
    whole = cc.cdm_oracle(cs)
    np.testing.assert_allclose(want["n1"].sum(0), whole["n1"], rtol=1e-12, atol=1e-12)     # the groups add up to everybody
    np.testing.assert_allclose(want["mass"].sum(0), whole["mass"], rtol=1e-12, atol=1e-12)
