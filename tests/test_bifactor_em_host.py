"""The bifactor E-step and fit (expected_counts_bifactor / fit_em_bifactor), the parts that need no GPU: the two float64 oracles
against each other, the count identities, the float32 restatement against the rule the GPU test applies, the gather and
scatter of the two-dimensional M-step's operands, every refusal, the new symbols of the C ABI and its launch plan (GbcPlan of
vipsy_amd/csrc/grid_plan.h, printed by tests/helpers/bifactor_counts_plan.cpp under AddressSanitizer + UBSan)."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import bifactor_cases as bc
from tests import bifactor_em_cases as be
from tests import corner_cases as cn
from tests import map_cases as mc
from vipsy_amd import grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracles and the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.BRUTE)
def test_brute_force_equals_the_reduction(name):
    o = be.oracle_of(name)
    brute = be.brute_counts(o["cs"])
    for k in be.TABLES + ("post",):
        assert np.abs(brute[k] - o["want"][k]).max() <= 1e-12, (name, k, np.abs(brute[k] - o["want"][k]).max())
    # (loglik: the pseudo-testlet's bracket carries log sum_h v_h, 5e-9 with float32 log-weights, which this grid does not have;
    # tests/test_bifactor_host.py holds the two logliks together on the grid that carries the empty dimension)
    assert np.abs(brute["loglik"] - o["want"]["loglik"]).max() <= 1e-7


@pytest.mark.parametrize("name", be.COUNT_CASES + (be.CUT[0], be.GROUPS[0]))
def test_the_count_identities_hold_for_the_oracle(name):
    o = be.oracle_of(name)
    cs, want = o["cs"], o["want"]
    Gg, Gh = cs["nodes"]
    total, rows, answered = be.identities(want, cs, Gg, Gh)
    assert total <= 1e-12 and rows <= 1e-12 and answered <= 1e-12, (name, total, rows, answered)
    n = (want["n1"] + want["n0"]).reshape(cs["J"], Gg, Gh).sum(2)
    assert np.abs(n - be.answered_mass(cs, want["post"])).max() <= 1e-10 * len(cs["y"])
    # an item nobody answered correctly has no n1, and the other way round
    for k, v in (("n1", 1), ("n0", 0)):
        none = ~(cs["y"] == v).any(0)
        assert (want[k][none] == 0).all()


@pytest.mark.parametrize("name", be.COUNT_CASES + (be.CUT[0], be.GROUPS[0]))
def test_restatement_meets_a_third_of_the_row_rule(name):
    o = be.oracle_of(name)
    print(name, {k: "%.1e" % v for k, v in o["e"].items()}, "cap %.1e" % o["cap"])
    for k in be.TABLES:
        assert o["e"][k] <= o["tol"][k] / 3.0, (name, k, o["e"][k], o["tol"][k])
        assert cn.ROW_TOL <= o["tol"][k] <= max(cn.ROW_TOL, o["cap"])
    Gg, Gh = o["cs"]["nodes"]
    for e in be.identities(o["r"], o["cs"], Gg, Gh):
        assert e <= cn.ROW_TOL / 3.0


def test_the_restatement_takes_the_hosts_slabs_in_person_order():
    """Two host slabs of 768 and 332 persons: other chunks, other sums, the same tables within the restatement's own error."""
    o = be.oracle_of(be.CUT[0])
    two = be.restated_counts(o["cs"], slab_persons=768)
    for k in be.TABLES:
        assert be.row_error(two[k], o["want"][k]) <= o["tol"][k] / 3.0, k
    assert any(not np.array_equal(two[k], o["r"][k]) for k in be.TABLES)


def test_the_cut_case_cuts_the_persons():
    name, N, sizes = be.CUT[0], be.CUT[1], be.CUT[2]
    cs = bc.case_of(be.CUT)
    plan = be.oracle_of(name)["plan"]
    p = be.gbc_plan(N, plan["KC"], cs["nodes"][0], len(plan["tl_column"]))
    assert N <= 4096 and N % 64 != 0 and p["n_chunks"] >= 2 and p["units_per_chunk"] > be.GBC_WAVES
    assert plan["KC"] == 3 and be.gbc_groups(plan["tl_start"]) == 2 and p["n_gpairs"] == 1


def test_the_groups_case_takes_two_chunk_groups_and_has_items_without_an_answer():
    o = be.oracle_of(be.GROUPS[0])
    cs, plan = o["cs"], o["plan"]
    assert list(np.diff(plan["tl_start"])) == [3, 1] and be.gbc_groups(plan["tl_start"]) == 3
    assert cs["nodes"][0] % be.GBC_NG == 1                            # a ragged last pair of general nodes
    no1, no0 = (int(plan["col"][s]) for s in be.ZERO_ITEMS[be.GROUPS[0]])
    assert be.ZERO_ITEMS[be.GROUPS[0]][0] // 16 == 2                  # the third chunk: the second group's own
    assert not (cs["y"][:, no1] == 1).any() and (cs["y"][:, no1] == 0).any()
    assert not (cs["y"][:, no0] == 0).any() and (cs["y"][:, no0] == 1).any()
    assert (o["want"]["n1"][no1] == 0).all() and (o["want"]["n0"][no0] == 0).all() and (o["r"]["n1"][no1] == 0).all()


# ---- the EM oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [be.EM_2PL[0], be.EM_3PL[0]])
def test_the_float64_em_rises_and_the_restated_em_follows_it(name):
    ps, lks, lps = be.em(name)
    for k in range(len(lps) - 1):
        assert lps[k + 1] >= lps[k] - 1e-6 * abs(lps[k]), (name, k)
    assert lps[-1] - lps[0] > 100.0                                   # (the start is far from the maximum)
    d = be.em_distance(name)
    print("%s: float64 EM against the EM on the float32 restatement after %d iterations: %.2e; the GPU rule is %g times that"
          % (name, be.EM_ITERS, d, be.EM_MARGIN))
    assert 0 < d <= 1e-5
    cs = be.case_by_name(name)
    sd, has, _ = be.em_operands(cs)
    a = ps[-1]["a"]
    others = np.ones_like(a, bool)
    others[cs["general"]] = False
    others[sd[has], np.arange(cs["J"])[has]] = False
    assert (a[others] == 0).all()


# ---- gather and scatter --------------------------------------------------------------------------------------------------
def test_gather_and_scatter_by_hand():
    """Four dimensions, the general one at index 2; items 0 and 3 on dimension 0, item 1 on dimension 3, item 2 general only,
    item 4 on dimension 1."""
    free = np.array([[1, 0, 0, 1, 0], [0, 0, 0, 0, 1], [1, 1, 1, 1, 1], [0, 1, 0, 0, 0]], np.float32)
    a = np.arange(1, 21, dtype=np.float32).reshape(4, 5) * free
    st = grid.bifactor_structure(free, a, "irt_2pl", general=2)
    assert list(st["specific_dims"]) == [0, 1, 3] and list(st["testlet"]) == [0, 2, -1, 0, 1]
    sd, has = grid.bifactor_em_index(st)
    assert list(sd) == [0, 3, 2, 0, 1] and list(has) == [True, True, False, True, True]
    ta, tf, tsd, th = torch.from_numpy(a.copy()), torch.from_numpy(free), torch.from_numpy(sd), torch.from_numpy(has)
    a2 = grid.bifactor_gather(ta, 2, tsd, th)
    assert a2.tolist() == [[11, 12, 13, 14, 15], [1, 17, 0, 4, 10]]
    assert grid.bifactor_gather(tf, 2, tsd, th).tolist() == [[1, 1, 1, 1, 1], [1, 1, 0, 1, 1]]
    new = torch.tensor([[-1., -2., -3., -4., -5.], [-6., -7., 99., -8., -9.]])
    out = grid.bifactor_scatter(ta, new, 2, tsd, th)
    want = np.zeros((4, 5), np.float32)
    want[2] = [-1, -2, -3, -4, -5]
    want[0, 0], want[3, 1], want[0, 3], want[1, 4] = -6, -7, -8, -9
    assert out is ta and np.array_equal(ta.numpy(), want)              # (the 99 of the general-only item goes nowhere)
    # the prior: scalars pass, leaf-shaped arrays are gathered like the loadings
    mean, sdv = np.arange(20, dtype=np.float64).reshape(4, 5) / 10, np.full((4, 5), 2.0)
    sdv[3, 1] = np.inf
    pr = grid.bifactor_em_prior({"a": (mean, sdv), "b": (0.5, 1.0)}, "irt_2pl", 4, 5, 2, sd, has)
    assert pr.shape == (2, 6, 5)
    assert np.allclose(pr[0, 1], mean[2]) and np.allclose(pr[1, 1], 0.25)
    assert np.allclose(pr[0, 2], [0.0, 0.0, 0.0, 0.3, 0.9]) and np.allclose(pr[1, 2], [0.25, 0.0, 0.0, 0.25, 0.25])
    assert np.allclose(pr[0, 0], 0.5) and np.allclose(pr[1, 0], 1.0) and (pr[:, 3:] == 0).all()
    flat = grid.bifactor_em_prior({"a": (1.0, 2.0)}, "irt_2pl", 4, 5, 2, sd, has)
    assert np.array_equal(flat, grid.em_prior({"a": (1.0, 2.0)}, "irt_2pl", 2, 5))
    for bad in ({"a": (np.zeros((2, 5)), 1.0)}, {"a": (0.0, np.zeros((4, 5)))}, {"a": (0.0,)}, {"q": (0.0, 1.0)}):
        with pytest.raises(ValueError):
            grid.bifactor_em_prior(bad, "irt_2pl", 4, 5, 2, sd, has)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _model(cs, model=None, cls=None):
    from vipsy_amd import vi
    vi.clear_param_store()
    return vi.VIRT(data=torch.from_numpy(cs["y"]), model=model or cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=3,
                   a_free=torch.from_numpy(cs["free"]), a0=torch.from_numpy(cs["free"].copy()), backend=mc.MapOracleBackend())


def test_every_refusal(monkeypatch):
    cs = bc.case_of(bc.by_name("s2_2pl"))
    m = _model(cs)
    before = {n: m.engine.unconstrained(n).clone() for n in ("a", "b")}
    for call in (m.fit_em_bifactor, m.engine.fit_em_bifactor):
        with pytest.raises(ValueError, match=r"1024.*\(41, 21\)"):
            call(nodes=(61, 21))
        for kw in (dict(max_iter=0), dict(newton=0), dict(newton=65), dict(nodes=(1, 5)), dict(nodes=(41, 33)), dict(span=6.0),
                   dict(general=7), dict(prior="c"), dict(prior={"c": (-1.4, 1.0)}), dict(prior={"a": (np.zeros((2, 3)), 1.0)})):
            with pytest.raises(ValueError):
                call(**kw)
    for kw in (dict(nodes=(257, 5)), dict(nodes=(21, 0)), dict(general=-1)):
        with pytest.raises(ValueError):
            m.engine.expected_counts_bifactor(**kw)
    # a testlet of one item: named by its dimension, unless a prior holds its loading
    one = bc.case_of(bc.by_name("s5_3pl"))
    m2 = _model(one, model="irt_2pl")
    dim = int(one["specific_dims"][[s for s in range(len(one["specific_dims"])) if (one["testlet"] == s).sum() == 1][0]])
    with pytest.raises(ValueError, match="dimension %d has ONE item" % dim):
        m2.fit_em_bifactor(max_iter=1)
    sd = np.full((one["D"], one["J"]), np.inf)
    with pytest.raises(ValueError, match="dimension %d has ONE item" % dim):
        m2.fit_em_bifactor(max_iter=1, prior={"a": (0.0, sd)})
    # 3PL without a prior, in fit_em's words; with one that lacks c, in em_prior's
    m3 = _model(one)
    with pytest.raises(NotImplementedError, match="not concave") as e:
        m3.fit_em_bifactor(max_iter=1)
    assert "prior=" in str(e.value)
    with pytest.raises(ValueError, match="finite sd on 'c'"):
        m3.fit_em_bifactor(max_iter=1, prior={"a": (1.0, 1.0)})
    # the other classes, in the words score_bifactor uses
    from tests import score_cases as sc
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, cs["J"], np.random.RandomState(2)))
    v = vi.VCCDM(data=torch.from_numpy(cs["y"]), q=q, backend=mc.MapOracleBackend())
    with pytest.raises(NotImplementedError) as e0:
        v.engine.score_bifactor()
    for name in ("expected_counts_bifactor", "fit_em_bifactor"):
        for obj in (v, v.engine):
            with pytest.raises(NotImplementedError) as e:
                getattr(obj, name)()
            assert str(e.value) == str(e0.value)
    # a process group of two
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    m.engine.group = object()
    for call in (m.engine.expected_counts_bifactor, m.engine.fit_em_bifactor):
        with pytest.raises(NotImplementedError, match="process group"):
            call()
    m.engine.group = None
    m.world = 2
    for call in (m.expected_counts_bifactor, m.fit_em_bifactor):
        with pytest.raises(NotImplementedError, match="group of 2 ranks"):
            call()
    for n, t in before.items():
        assert torch.equal(m.engine.unconstrained(n), t)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW = {"vx_grid_bifactor_counts_workspace_floats": 4, "vx_grid_bifactor_counts": 21}


def test_new_symbols_are_declared_bound_and_refuse_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from vipsy_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "vipsy_amd.h")).read()
    L = _hip.lib()
    for name, n_args in NEW.items():
        m = re.search(r"\nint(?:64_t)? %s\((.*?)\);" % name, hdr, flags=re.S)
        assert m and hasattr(L, name), name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
    assert _hip.ABI_VERSION == 9 and L.vx_abi_version() == 9                     # entries were only added
    query = L.vx_grid_bifactor_counts_workspace_floats
    for nb, KC, Gg, n_tl in ((100, 3, 21, 2), (1100, 3, 2, 2), (167680, 100, 41, 100), (1 << 40, 1024, 128, 1024)):
        p = be.gbc_plan(nb, KC, Gg, n_tl)
        assert query(nb, KC, Gg, n_tl) == p["n_chunks"] * p["slab_len"], (nb, KC, Gg, n_tl)
    assert query(1100, 3, 2, 2) == 3 * (2 * 16 * 3 * 2 * 32 + 2 * 2 * 32 + 2)
    for nb, KC, Gg, n_tl in ((0, 3, 21, 2), (-7, 3, 21, 2), ((1 << 48) + 1, 3, 21, 2), (100, 0, 21, 2), (100, 1025, 21, 2),
                             (100, 3, 1, 2), (100, 3, 257, 2), (100, 3, 21, 0), (100, 3, 21, 4), (100, 1024, 129, 2)):
        assert query(nb, KC, Gg, n_tl) == -1, (nb, KC, Gg, n_tl)
    # one wrong argument at a time, refused before any HIP call (there is no GPU here)
    host = (ctypes.c_float * 4096)()
    hp = ctypes.cast(host, ctypes.c_void_p)
    odd = ctypes.c_void_p(hp.value + 4)
    tl_ok = (ctypes.c_int32 * 3)(0, 1, 3)
    ok = dict(y=hp, nb=100, KC=3, Gg=21, Gh=11, tl=tl_ok, n_tl=2, tl_dev=hp, col=hp, J=23, img=hp, logv=hp, loglik=hp, fws=hp,
              accumulate=0, n1=hp, n0=hp, mass=hp, mass_s=hp, ws=hp)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vx_grid_bifactor_counts(a["y"], a["nb"], a["KC"], a["Gg"], a["Gh"], a["tl"], a["n_tl"], a["tl_dev"], a["col"], a["J"],
                                         a["img"], a["logv"], a["loglik"], a["fws"], a["accumulate"], a["n1"], a["n0"], a["mass"],
                                         a["mass_s"], a["ws"], None)

    for k in ("y", "tl", "tl_dev", "col", "img", "logv", "loglik", "fws", "n1", "n0", "mass", "ws"):
        assert call(**{k: None}) == -1, k
    assert call(img=odd) == -1 and call(ws=odd) == -1
    for kw in (dict(nb=0), dict(nb=-7), dict(KC=0), dict(KC=1025), dict(Gg=1), dict(Gg=257), dict(Gh=0), dict(Gh=33), dict(n_tl=0),
               dict(n_tl=4), dict(KC=1024, Gg=129), dict(J=0), dict(J=1025), dict(accumulate=2), dict(accumulate=-1)):
        assert call(**kw) == -1, kw
    for tl in ((1, 2, 3), (0, 1, 2), (0, 0, 3), (0, 3, 3), (0, 2, 1)):
        assert call(tl=(ctypes.c_int32 * 3)(*tl)) == -1, tl


def test_the_launch_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler"
    exe = str(tmp_path / "bifactor_counts_plan")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "vipsy_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "bifactor_counts_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    got = json.loads(r.stdout)
    assert len(got["plans"]) == 14 * 8 * 7
    import __graft_entry__ as g
    g.build()
    from vipsy_amd import _hip
    L = _hip.lib()
    for nb, KC, Gg, n_tl, n_gpairs, n_units, upc, n_chunks, off_ms, off_mass, slab_len in got["plans"]:
        p = be.gbc_plan(nb, KC, Gg, n_tl)
        assert (n_gpairs, n_units, upc, n_chunks, slab_len) == (p["n_gpairs"], p["n_units"], p["units_per_chunk"], p["n_chunks"],
                                                                p["slab_len"]), (nb, KC, Gg, n_tl)
        assert off_ms == 1024 * KC * Gg and off_mass == off_ms + 32 * n_tl * Gg and slab_len == off_mass + Gg
        # the workspace query: chunks x slab length where the shape is one the entry takes, VX_EINVAL where not
        ok = n_tl <= KC and Gg * KC * 4096 <= 512 << 20
        assert L.vx_grid_bifactor_counts_workspace_floats(nb, KC, Gg, n_tl) == (n_chunks * slab_len if ok else -1), (nb, KC, Gg, n_tl)
    for row in got["groups"]:
        assert row[-1] == be.gbc_groups(row[:-1]), row
    assert [row[-1] for row in got["groups"]] == [1, 2, 4, 7, 512]
