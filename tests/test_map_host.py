"""fit_em(prior=) and vx_grid_mstep_irt_map, the parts that need no GPU: the declarations, the gate, the one checker of `prior`,
the refusals, fit_em(prior=) through _em_loop on a numpy backend, and the conditions under which the rules of
tests/test_gpu_map.py and tests/test_gpu_map_paths.py are fair -- checked on the float64 oracle and on the kernel's method said
again in float32 numpy (tests/map_cases.py), which must meet rules 1, 2 and 3 at HALF their constants, while four wrong step
controls said the same way must break rule 3."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import map_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(mc.CASES)


def _build():
    import __graft_entry__ as g
    g.build()


# ---- declarations --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_symbol_agree():
    _build()
    from vipsy_amd import _hip
    from vipsy_amd.engine import HipBackend
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+vx_grid_mstep_irt_map\s*\(([^;]*)\)\s*;", header)
    assert m, "include/vipsy_amd.h does not declare vx_grid_mstep_irt_map"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    want = ["const vx_irt_cfg* cfg", "const float* theta", "int32_t G", "const float* n1", "const float* n0", "const float* a_free",
            "float* a", "float* b", "float* c_un", "float* d_un", "const float* prior", "int32_t newton", "float* lprior",
            "void* hip_stream"]
    assert [" ".join(p.split()) for p in params] == want
    res, args = _hip.SIGNATURES["vx_grid_mstep_irt_map"]
    assert res is ctypes.c_int and len(args) == len(want)
    for p, a in zip(want, args):
        assert (a is _hip._I32) == p.startswith("int32_t") and (a is _hip._CFG) == ("vx_irt_cfg" in p), (p, a)
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "vx_grid_mstep_irt_map")
    assert callable(HipBackend.grid_mstep_irt_map)
    assert _hip.lib().vx_abi_version() == _hip.ABI_VERSION             # (an added entry: the version stays)


def test_every_gate_row_refuses_before_the_runtime():
    _build()
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import map_gates as mg
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "map_gates.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [l for l, _ in got] == [l for l, _ in mg.ROWS] and len(got) >= 20
    assert not [(l, rc) for l, rc in got if rc != -1]
    labels = {l for l, _ in got}
    assert {"3PL without c_un", "4PL without d_un", "no prior", "newton 0", "newton 65"} <= labels


# ---- the one checker of `prior` -------------------------------------------------------------------------------------------------
def test_em_prior_layout():
    from vipsy_amd.grid import EM_PRIOR_ROWS, em_prior
    J, D = 5, 2
    sd_b = np.full((1, J), np.inf)
    sd_b[0, 3] = 2.0
    mean_a = np.arange(D * J, dtype=np.float64).reshape(D, J)
    out = em_prior({"a": (mean_a, 0.5), "b": (7.0, sd_b), "c": (-1.4, 1.0), "d": (2.2, np.full((1, J), 0.25))}, "irt_4pl", D, J)
    assert out.shape == (2, EM_PRIOR_ROWS, J) == (2, 6, J) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
    assert np.array_equal(out[0, 1:3], mean_a.astype(np.float32)) and (out[1, 1:3] == 4.0).all()
    assert (out[:, 3] == 0).all()                                      # a_2: the model has two dimensions
    assert np.array_equal(out[1, 0], [0, 0, 0, 0.25, 0]) and np.array_equal(out[0, 0], [0, 0, 0, 7, 0])    # sd inf: no prior, mean 0
    assert (out[0, 4] == np.float32(-1.4)).all() and (out[1, 4] == 1).all() and (out[1, 5] == 16).all()
    # absent keys: nothing; 1PL and 2PL take an empty dict
    assert not em_prior({}, "irt_2pl", 1, J).any() and not em_prior({}, "irt_1pl", 1, J).any()
    assert em_prior({"c": (-1.4, 1.0)}, "irt_3pl", 1, J)[1].sum() == J


BAD_PRIORS = [
    ("not a dict", "irt_2pl", [("a", (1.0, 1.0))], "dict"),
    ("unknown key", "irt_2pl", {"g": (0.0, 1.0)}, "unknown"),
    ("1PL has no a", "irt_1pl", {"a": (1.0, 1.0)}, "no such"),
    ("2PL has no c", "irt_2pl", {"c": (-1.4, 1.0)}, "no such"),
    ("3PL has no d", "irt_3pl", {"c": (-1.4, 1.0), "d": (2.2, 1.0)}, "no such"),
    ("not a pair", "irt_2pl", {"a": 1.0}, "pair"),
    ("a triple", "irt_2pl", {"a": (1.0, 1.0, 1.0)}, "pair"),
    ("bad shape", "irt_2pl", {"b": (np.zeros(5), 1.0)}, "shape"),
    ("bad shape of a", "irt_2pl", {"a": (1.0, np.ones((5, 1)))}, "shape"),
    ("sd 0", "irt_2pl", {"b": (0.0, 0.0)}, "sd"),
    ("sd negative", "irt_2pl", {"b": (0.0, -1.0)}, "sd"),
    ("sd NaN", "irt_2pl", {"b": (0.0, float("nan"))}, "sd"),
    ("one sd 0", "irt_2pl", {"b": (0.0, np.array([[1.0, 1.0, 0.0, 1.0, 1.0]]))}, "sd"),
    ("sd too small for float32", "irt_2pl", {"b": (0.0, 1e-30)}, "float32"),
    ("mean inf", "irt_2pl", {"b": (float("inf"), 1.0)}, "finite"),
    ("mean NaN", "irt_2pl", {"a": (float("nan"), 1.0)}, "finite"),
    ("3PL without c", "irt_3pl", {"a": (1.0, 1.0)}, "asymptote"),
    ("3PL with sd inf on c", "irt_3pl", {"c": (-1.4, float("inf"))}, "asymptote"),
    ("3PL with one sd inf on c", "irt_3pl", {"c": (-1.4, np.array([[1.0, 1.0, np.inf, 1.0, 1.0]]))}, "asymptote"),
    ("4PL without d", "irt_4pl", {"c": (-1.4, 1.0)}, "asymptote"),
    ("4PL without c", "irt_4pl", {"d": (2.2, 1.0)}, "asymptote"),
]


@pytest.mark.parametrize("label,model,prior,says", BAD_PRIORS, ids=[b[0].replace(" ", "_") for b in BAD_PRIORS])
def test_em_prior_value_errors(label, model, prior, says):
    from vipsy_amd.grid import em_prior
    with pytest.raises(ValueError) as e:
        em_prior(prior, model, 1, 5)
    assert says in str(e.value), (label, str(e.value))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("model", ["irt_3pl", "irt_4pl"])
def test_without_prior_the_asymptote_models_still_refuse_and_say_how(model):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model=model, backend=mc.MapOracleBackend())
    for call in (m.fit_em, m.engine.fit_em):
        with pytest.raises(NotImplementedError) as e:
            call(max_iter=2)
        assert "prior=" in str(e.value) and "not concave" in str(e.value)


def test_fit_em_raises_the_value_errors_before_anything_runs():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_3pl", backend=mc.MapOracleBackend())
    before = {n: m.engine.unconstrained(n).clone() for n in ("a", "b", "c")}
    for prior in ({}, {"c": (-1.4, 0.0)}, {"c": (-1.4, 1.0), "d": (2.2, 1.0)}, {"c": (-1.4, 1.0), "x": (0.0, 1.0)},
                  {"c": (np.zeros((1, 11)), 1.0)}, "c"):
        with pytest.raises(ValueError):
            m.fit_em(max_iter=1, prior=prior)
    for kw in (dict(max_iter=0), dict(newton=0), dict(newton=65)):
        with pytest.raises(ValueError):
            m.fit_em(prior={"c": (-1.4, 1.0)}, **kw)
    for n, v in before.items():
        assert torch.equal(m.engine.unconstrained(n), v)
    vi.clear_param_store()
    m4 = vi.VIRT(data=_y(), model="irt_2pl", x_feature=4, backend=mc.MapOracleBackend())
    with pytest.raises(NotImplementedError):
        m4.fit_em(max_iter=1, prior={})


def test_ccdm_refuses_a_prior():
    from tests import score_cases as sc
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    m = vi.VCCDM(data=_y(), q=q, backend=mc.MapOracleBackend())
    for call in (m.fit_em, m.engine.fit_em):
        with pytest.raises(ValueError) as e:
            call(max_iter=1, prior={"b": (0.0, 1.0)})
        assert "prior" in str(e.value)


def test_two_ranks_refuse(tmp_path):
    """A gloo group of two: the model class and the engine both refuse fit_em(prior=), before anything is computed."""
    worker = os.path.join(ROOT, "tests", "_map_dist_worker.py")
    out = str(tmp_path / "map_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29653", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            assert f.read().split() == ["NotImplementedError", "NotImplementedError"]


# ---- fit_em(prior=) through _em_loop on the numpy backend ------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.EM_CASES)
def test_fit_em_with_prior_runs_through_the_em_loop(name):
    """The engine's host path on CPU tensors: the compact copies of c and d reach the tables and the M-step and come back into
    the leaves, logpost = loglik + the summed lprior, and the leaves after three iterations are the oracle trajectory's (the
    backend computes with the same functions: float32 storage of the leaves is all that differs)."""
    from vipsy_amd import vi
    cs = mc.case(name)
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]), model=cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=3, backend=mc.MapOracleBackend())
    eng = m.engine
    if cs["a_free"] is not None:                                       # (the engine's own mask is the case's)
        assert np.array_equal(eng.unconstrained("a", eng.free).numpy() != 0, cs["a_free"])
    for k, v in mc.em_start(cs).items():
        eng.unconstrained(k).copy_(torch.from_numpy(v))
    t0, P0 = eng.t, eng.P.clone()
    out = m.fit_em(max_iter=3, tol=0, prior=mc.em_prior_of(cs), nodes=cs["nodes"], span=cs["span"])
    ps, lks, lps, _ = mc.trajectory(name, 3)
    assert sorted(out) == ["converged", "iterations", "loglik", "logpost"] and out["iterations"] == 3 and out["converged"] is False
    assert np.allclose(out["loglik"], lks, rtol=1e-5, atol=0) and np.allclose(out["logpost"], lps, rtol=1e-5, atol=0)
    assert out["logpost"][0] == out["loglik"][0]                       # (the start sits on every prior mean)
    assert out["logpost"][2] < out["loglik"][2] and out["logpost"][2] > out["logpost"][1] > out["logpost"][0]
    for k, w in ps[3].items():
        got = eng.unconstrained(k).numpy().astype(np.float64)
        assert np.abs(got - w).max() <= 1e-4, (k, np.abs(got - w).max())
    assert eng.t == t0 and not torch.equal(eng.P, P0)
    # the unanswered item kept its bits, and so did the masked loadings
    for k, v in mc.em_start(cs).items():
        assert eng.unconstrained(k).numpy()[:, mc.UNANSWERED].tobytes() == v[:, mc.UNANSWERED].tobytes()
    if cs["a_free"] is not None:
        assert not eng.unconstrained("a").numpy()[~cs["a_free"]].any()


def test_the_entry_by_entry_prior_of_the_end_to_end_case():
    """em_prior_of: full [D][J] arrays, no prior (precision 0, mean 0) at the masked loadings and at two free ones, the case's
    own prior everywhere else."""
    cs = mc.case(mc.EM_ENTRY_CASE)
    pr, own = mc.prior_rows(cs, mc.em_prior_of(cs)), mc.prior_rows(cs)
    off = ~cs["a_free"]
    off[0, 2] = off[1, 3] = True
    assert cs["a_free"][0, 2] and cs["a_free"][1, 3] and (~cs["a_free"]).sum() == 3
    D = cs["D"]
    assert not pr[:, 1:1 + D][:, off].any() and np.array_equal(pr[:, 1:1 + D][:, ~off], own[:, 1:1 + D][:, ~off])
    assert np.array_equal(pr[:, [0, 4, 5]], own[:, [0, 4, 5]]) and own[1, 1:1 + D].all()
    for n in mc.EM_CASES:
        if n != mc.EM_ENTRY_CASE:
            assert mc.em_prior_of(mc.case(n)) is mc.case(n)["prior"]


def test_every_model_takes_the_new_entry_and_converges_on_logpost():
    from vipsy_amd import vi
    cs = mc.case("map4_2pl_j8_g61")
    calls = []

    class Spy(mc.MapOracleBackend):
        def grid_mstep_irt_map(self, *a, **kw):
            calls.append("map")
            return super().grid_mstep_irt_map(*a, **kw)

    for model, prior in (("irt_1pl", {"b": (0.0, 2.0)}), ("irt_2pl", {"a": (1.0, 0.5), "b": (0.0, 2.0)}), ("irt_2pl", {})):
        vi.clear_param_store()
        m = vi.VIRT(data=torch.from_numpy(cs["y"][:200]), model=model, D=cs["Dc"], seed=3, backend=Spy())
        del calls[:]
        out = m.fit_em(max_iter=30, tol=1e-4, prior=prior, nodes=21)
        assert calls == ["map"] * out["iterations"] and out["converged"] and 2 <= out["iterations"] < 30
        lp = out["logpost"]
        assert lp[-1] - lp[-2] <= 1e-4 * abs(lp[-2]) and all(lp[k + 1] - lp[k] > 1e-4 * abs(lp[k]) for k in range(len(lp) - 2))
        assert np.isfinite(lp).all() and all(p <= l for p, l in zip(lp, out["loglik"]))


# ---- the rules' conditions, and the method against them --------------------------------------------------------------------------
def test_cases_are_as_documented():
    shapes = {n: (mc.case(n)["model"], mc.case(n)["D"], mc.case(n)["J"], mc.case(n)["G"]) for n in NAMES}
    assert shapes == {"map1_3pl_j14_g41": ("irt_3pl", 1, 14, 41), "map2_4pl_j14_g41": ("irt_4pl", 1, 14, 41),
                      "map3_3pl_d2_j7_g441": ("irt_3pl", 2, 7, 441), "map4_2pl_j8_g61": ("irt_2pl", 1, 8, 61),
                      "map5_3pl_j5_g1024": ("irt_3pl", 1, 5, 1024), "map6_3pl_j6_g1": ("irt_3pl", 1, 6, 1),
                      "map7_1pl_j7_g61": ("irt_1pl", 1, 7, 61), "map8_4pl_d2_j6_g225": ("irt_4pl", 2, 6, 225),
                      "map9_2pl_d3_j7_g343": ("irt_2pl", 3, 7, 343), "map10_4pl_d3_j9_g729": ("irt_4pl", 3, 9, 729)}
    assert {n: mc.case(n)["N"] for n in NAMES[6:]} == {"map7_1pl_j7_g61": 500, "map8_4pl_d2_j6_g225": 1000,
                                                       "map9_2pl_d3_j7_g343": 800, "map10_4pl_d3_j9_g729": 1500}
    assert {n: mc.case(n)["Dc"] for n in NAMES} == {n: (1.0 if n == "map10_4pl_d3_j9_g729" else 1.702) for n in NAMES}
    for n in NAMES:
        cs, L = mc.case(n), mc.launch(n)
        y = cs["y"]
        assert 0.07 < (y[:, [j for j in range(cs["J"]) if j != mc.UNANSWERED]] == 255).mean() < 0.13
        assert (y[:, mc.UNANSWERED] == 255).all() and not (y[:, -1] == 0).any() and (y[:, -1] == 1).sum() > 100
        assert list(mc.answered(L)) == [j != mc.UNANSWERED for j in range(cs["J"])]
        assert L["prior"][1, 0, -1] > 0                                 # the constant item has a prior on b
        for k, v in cs["start"].items():
            assert np.abs(v - cs["truth"][k]).max() <= 0.5 + 1e-6
    assert mc.case("map1_3pl_j14_g41")["N"] == 2048 and mc.case("map2_4pl_j14_g41")["N"] == 2048
    free = mc.case("map3_3pl_d2_j7_g441")["a_free"]
    assert not free.all() and free[0].all()                             # triangular: a masked loading
    assert not mc.launch("map4_2pl_j8_g61")["prior"][1, 0, :-1].any() and mc.launch("map4_2pl_j8_g61")["prior"][1, 1].all()
    # default_a_free leaves masked loadings in both multi-dimensional shapes: triangular, the last D - 1 items
    f2, f3 = mc.case("map8_4pl_d2_j6_g225")["a_free"], mc.case("map9_2pl_d3_j7_g343")["a_free"]
    assert f2.shape == (2, 6) and f2[0].all() and list(f2[1]) == [True] * 5 + [False]
    assert f3.shape == (3, 7) and f3[0].all() and list(f3[1]) == [True] * 6 + [False] and list(f3[2]) == [True] * 5 + [False] * 2
    assert np.array_equal(mc.case("map10_4pl_d3_j9_g729")["a_free"][:, -3:], [[True] * 3, [True, True, False], [True, False, False]])
    assert mc.case("map7_1pl_j7_g61")["a_free"] is None
    for n in ("map8_4pl_d2_j6_g225", "map9_2pl_d3_j7_g343", "map10_4pl_d3_j9_g729"):
        cs, L = mc.case(n), mc.launch(n)
        assert not cs["start"]["a"][~cs["a_free"]].any() and not mc.em_start(cs)["a"][~cs["a_free"]].any()
        assert (mc.em_start(cs)["a"][cs["a_free"]] == 1).all()
        assert L["prior"][1, 1:1 + cs["D"]].all() and L["prior"][1, 4].all() == (cs["model"] == "irt_4pl")
    assert not mc.launch("map7_1pl_j7_g61")["prior"][:, 1:].any()


@pytest.mark.parametrize("name", NAMES)
def test_the_method_meets_rule_1_at_half_the_constant(name):
    """One launch of 64 steps in float32 numpy from the start; the float64 maximiser started at its output."""
    cs, L = mc.case(name), mc.launch(name)
    st = {}
    p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0"], L["prior"], 64, np.float32, stats=st)
    gain, dev, last = mc.rule1(cs, L, p)
    print("%s: float32 restatement gains at most %.3g of 1e-6 |Q| (C_Q / 2 = %g), parameters at most %.3g of their bound; the "
          "maximiser's last step %.1e; %s" % (name, gain.max(), mc.C_Q / 2, dev.max(), last, st))
    assert last <= 1e-6
    assert gain.min() >= 0 and gain.max() <= mc.C_Q / 2 and dev.max() <= np.sqrt(0.5)
    assert st["stopped"] == 0
    assert p[:, mc.UNANSWERED].tobytes() == L["p0"][:, mc.UNANSWERED].tobytes()
    assert p[~L["free"]].tobytes() == L["p0"][~L["free"]].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_method_meets_rule_2_at_half_the_constant(name):
    """One step from p0_near: the float64 full step (capped where the cap applies, never halved) is accepted by more than 100
    times the acceptance tolerance on every item, so float32 takes the same decision; and the float32 step is the float64 one
    to half of C_STEP eps32 |H^-1| S."""
    cs, L = mc.case(name), mc.launch(name)
    p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0_near"], L["prior"], 1, np.float32)
    ratio, p64, st = mc.rule2(cs, L, p)
    print("%s: float32 restatement at most %.3g (C_STEP / 2 = %g); smallest margin %.0f tolerances" %
          (name, ratio.max(), mc.C_STEP / 2, st["margin"] / mc.QTOL))
    assert st["halvings"] == 0 and st["stopped"] == 0 and st["margin"] >= 100 * mc.QTOL
    assert ratio.max() <= mc.C_STEP / 2
    assert np.abs(p64 - L["p0_near"])[:, mc.answered(L)].max() > 1e-3      # (a step was taken)


@pytest.mark.parametrize("name", mc.EM_CASES)
def test_em_conditions(name):
    """25 iterations at newton = 4 in the float64 oracle and with the float32 M-step: logpost rises at every iteration, no item
    stops, and the two end within 1e-4 of a posterior standard deviation of each other -- the end-to-end rule (a hundredth of
    one) is not a rule about rounding."""
    cs = mc.case(name)
    ps, lks, lps, st = mc.trajectory(name, 25)
    ps32, _, lps32, st32 = mc.trajectory(name, 25, dtype=np.float32)
    for tag, l, s in (("float64", lps, st), ("float32", lps32, st32)):
        rises = np.diff(l)
        print("%s %s: smallest rise of logpost %.2e; %s" % (name, tag, rises.min(), s))
        assert rises.min() > 0 and s["stopped"] == 0
    sd, _ = mc.posterior_sd(cs, ps[25])
    for k in ps[25]:
        assert np.nanmax(np.abs(ps32[25][k] - ps[25][k]) / sd[k]) <= 1e-4
        assert np.isfinite(ps[25][k]).all()


# ---- far starts: the step control on the penalised Q_j ---------------------------------------------------------------------------
FAR_IDS = [mc.far_id(f) for f in mc.FAR]


def _far32(far, newton=1, **kn):
    cs, L = mc.case(far[0]), mc.far_launch(far)
    tr, st = {}, {}
    p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0"], L["prior"], newton, np.float32, stats=st, trace=tr, **kn)
    return p, tr, st


def test_far_launches_are_as_documented():
    assert sorted({f[0] for f in mc.FAR}) == sorted(["map1_3pl_j14_g41", "map7_1pl_j7_g61", "map8_4pl_d2_j6_g225",
                                                     "map9_2pl_d3_j7_g343", "map10_4pl_d3_j9_g729"])
    for name in {f[0] for f in mc.FAR}:
        assert sorted(f[1] for f in mc.FAR if f[0] == name and len(f) == 3) == [1.5, 3.0, 5.0]
    assert sorted(f[0][:4] for f in mc.FAR if len(f) == 4) == ["map1", "map8", "map9"]
    cand = dropped = 0
    for far in mc.FAR:
        L, L0 = mc.far_launch(far), mc.launch(far[0])
        move = L["p0"].astype(np.float64) - L0["p0"]
        assert not move[~L["free"]].any() and np.abs(move).max() <= far[1] + 1e-6 and np.abs(move[L["free"]]).max() > 0.8 * far[1]
        assert L["p0"].dtype == np.float32 and L["n1"] is L0["n1"]
        assert np.array_equal(L["prior"][0], L0["prior"][0]) and np.array_equal(L["prior"][1], L0["prior"][1] * (far[3] if len(far) > 3 else 1))
        assert set(mc.FAR_DROPPED.get(far, {})) <= set(mc.far_candidates(far))
        cand += len(mc.far_candidates(far))
        dropped += len(mc.FAR_DROPPED.get(far, {}))
    print("far starts: %d item-starts with clear float64 decisions, %d dropped" % (cand, dropped))
    assert cand >= 100 and 10 * dropped <= cand
    assert not (set(mc.FAR_DROPPED) | set(mc.FAR_NOT_TO_THE_END)) - set(mc.FAR)


def test_far_starts_cover_the_paths():
    """Every path of the step control is walked, with clear decisions, by item-starts rule 3 is held on: all four by the
    launches of a 3PL / 4PL case (the 3PL D = 1 case) and by those of a 1PL / 2PL case (the 2PL D = 3 case).  The 1PL case has
    no two halvings in one step in any of seeds 1 .. 8 at the three amplitudes (one unknown: the capped Newton step of a
    concave function of b seldom overshoots twice); it walks the other three.  The 4PL cases at D = 2 and 3 walk the first three."""
    have = {}
    for far in mc.FAR[:15]:                                            # (the launches under the cases' own priors)
        _, tr = mc.far_step(far)
        for j in mc.far_items(far):
            have.setdefault(far[0], set()).update(mc.path_of(tr[j][0]))
    print({k: sorted(v) for k, v in have.items()})
    assert have["map1_3pl_j14_g41"] == set(mc.PATHS) and have["map9_2pl_d3_j7_g343"] == set(mc.PATHS)
    for n in ("map7_1pl_j7_g61", "map8_4pl_d2_j6_g225", "map10_4pl_d3_j9_g729"):
        assert have[n] >= set(mc.PATHS[:3]), (n, have[n])


@pytest.mark.parametrize("far", mc.FAR, ids=FAR_IDS)
def test_far_one_step_conditions(far):
    """Of every item-start rule 3 is held on: each trial of the float64 step is decided by 100 tolerances or more (the rejected
    trials below the threshold, the accepted one above), the float32 restatement walks the same path, and it lands within HALF
    of rule 3's bound."""
    _, tr = mc.far_step(far)
    p32, tr32, _ = _far32(far)
    items = mc.far_items(far)
    assert len(items) >= 4
    for j in items:
        r, r32 = tr[j][0], tr32[j][0]
        assert mc.is_clear(r) and min(abs(x) for x in r["margins"]) >= mc.CLEAR * mc.QTOL, (far, j, r["margins"])
        assert (r32["capped"], r32["halvings"], r32["stop"]) == (r["capped"], r["halvings"], None), (far, j)
        assert r["t"] == (min(1.0, mc.STEP_CAP / np.abs(r["delta"]).max()) if r["capped"] else 1.0) * 0.5 ** r["halvings"]
    ratio = mc.rule3(far, p32)
    print("%s: float32 restatement at most %.3g (C_STEP / 2 = %g) over items %s; smallest |margin| %.0f tolerances" %
          (mc.far_id(far), max(ratio.values()), mc.C_STEP / 2, items, min(abs(x) for j in items for x in tr[j][0]["margins"]) / mc.QTOL))
    assert max(ratio.values()) <= mc.C_STEP / 2, ratio
    L = mc.far_launch(far)
    assert p32[~L["free"]].tobytes() == L["p0"][~L["free"]].tobytes()


FAR_MUTANTS = {"halving factor 0.25": dict(halving=0.25), "cap 2": dict(cap=2.0), "cap clips each component": dict(cap_rescales=False),
               "acceptance on the unpenalised Q": dict(accept_unpenalised=True)}


def _far_failures(kn):
    out = []
    for far in mc.FAR:
        ratio = mc.rule3(far, _far32(far, **kn)[0])
        out += [(mc.far_id(far), j) for j, r in ratio.items() if not r <= mc.C_STEP]
    return out


def test_far_stand_in_passes_everywhere():
    assert _far_failures({}) == []


@pytest.mark.parametrize("mutant", list(FAR_MUTANTS), ids=[m.replace(" ", "_") for m in FAR_MUTANTS])
def test_far_mutants(mutant):
    """A wrong step control, said in float32 numpy, breaks rule 3 of tests/test_gpu_map_paths.py on some item-start it is held
    on (the kernel's own method breaks it on none: test_far_stand_in_passes_everywhere)."""
    bad = _far_failures(FAR_MUTANTS[mutant])
    print(mutant, "breaks", len(bad), "item-starts, first", bad[:3])
    assert bad, mutant
    if "unpenalised" in mutant:                                        # (only where the prior weighs: see map_cases.FAR)
        assert {f for f, _ in bad} == {mc.far_id(f) for f in mc.FAR if len(f) == 4}


@pytest.mark.parametrize("far", mc.FAR, ids=FAR_IDS)
def test_far_to_the_end_conditions(far):
    """64 steps from the far start: the float64 method stops no item, the float64 maximiser converges from the float32
    restatement's output, and that output meets rule 1 at half its constant -- or the launch is listed in FAR_NOT_TO_THE_END
    and left out of the GPU test.  (The float32 restatement MAY stop an item: on the constant item of the 4PL D = 2 case at amp
    5 it rejects all nine trials by one to two tolerances each, the rounding of its Q_j, 0.2 tolerances short of the maximum.
    Rule 1 is what is asked of the end, not the way there.)"""
    cs, L = mc.case(far[0]), mc.far_launch(far)
    st = {}
    mc.map_mstep(cs, L["n1"], L["n0"], L["p0"].astype(np.float64), L["prior"].astype(np.float64), 64, stats=st)
    p32, _, st32 = _far32(far, 64)
    gain, dev, last = mc.rule1(cs, L, p32)
    print("%s: float32 restatement gains at most %.3g of 1e-6 |Q| (C_Q / 2 = %g), parameters at most %.3g of their bound; float64 %s, "
          "float32 %s" % (mc.far_id(far), gain.max(), mc.C_Q / 2, dev.max(), st, st32))
    ok = st["stopped"] == 0 and last <= 1e-6 and gain.min() >= 0 and gain.max() <= mc.C_Q / 2 and dev.max() <= np.sqrt(0.5)
    assert ok == (far not in mc.FAR_NOT_TO_THE_END), (far, st, last, gain, dev)
    assert 10 * len(mc.FAR_NOT_TO_THE_END) <= len(mc.FAR)


# ---- the conditions of the header's promises -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["map9_2pl_d3_j7_g343", "map8_4pl_d2_j6_g225", "map7_1pl_j7_g61"])
def test_scaling_by_four_keeps_the_restatements_bits(name):
    """n1, n0 and every precision times 4: Q_j, its gradient and the matrix are exactly 4 times what they were (a power of two
    commutes with every rounding, and nothing here is near the ends of the exponent range), the Cholesky factor exactly twice,
    the step and every accept / reject decision the same -- so the float32 restatement returns the same bits, and the log prior
    exactly 4 times its value."""
    cs, L = mc.case(name), mc.launch(name)
    L4 = mc.scaled4(L)
    for newton in (1, 64):
        p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0"], L["prior"], newton, np.float32)
        p4 = mc.map_mstep(cs, L4["n1"], L4["n0"], L4["p0"], L4["prior"], newton, np.float32)
        assert p.tobytes() == p4.tobytes() and not np.array_equal(p, L["p0"])
    assert np.array_equal(mc.log_prior(L["p0"], L["free"], L4["prior"]), 4 * mc.log_prior(L["p0"], L["free"], L["prior"]))
    assert np.array_equal(L4["prior"][0], L["prior"][0]) and np.array_equal(L4["n1"], 4 * L["n1"])


def test_pivot_stop_premise():
    """Every node of the pivot item is clamped at the start, in float64 and in float32; its matrix is diag(prec_b, 0, 0, 0); the
    method, in either precision, stops it with all its bits and moves every other answered item."""
    cs, L = mc.case(mc.PIVOT_CASE), mc.pivot_launch()
    j = mc.PIVOT_ITEM
    assert cs["model"] == "irt_2pl" and L["free"][:4, j].all() and j != mc.UNANSWERED and mc.answered(L)[j]
    assert L["prior"][1, 0, j] > 0 and not L["prior"][1, 1:, j].any()
    U = mc.design(np.asarray(cs["theta"], np.float64))
    for dtype in (np.float64, np.float32):
        z, inside = mc.node_masks(cs, L["p0"][:, j], dtype)
        assert not inside.any() and np.abs(z).min() > mc.ZL + 1
        _, g, H, _ = mc.item_eval(cs["model"], U, cs["Dc"], L["n1"][j], L["n0"][j], L["p0"][:, j], L["free"][:, j], L["prior"][0, :, j],
                                  L["prior"][1, :, j], dtype)
        assert np.array_equal(H, np.diag([0.25, 0, 0, 0, 0, 0])) and g[0] == -0.25 * 20 and not g[1:].any()
        st, tr = {}, {}
        p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0"].astype(dtype), L["prior"], 64, dtype, stats=st, trace=tr)
        assert st["stopped"] == 1 and tr[j][0]["stop"] == "pivot" and len(tr[j]) == 1
        assert p[:, j].astype(np.float32).tobytes() == L["p0"][:, j].tobytes()
        others = [k for k in np.flatnonzero(mc.answered(L)) if k != j]
        assert (p[:, others][L["free"][:, others]] != L["p0"][:, others][L["free"][:, others]]).all()


def test_steep_and_falling_start_conditions():
    """The steep 3PL start has nodes that are not `inside` at every answered item, the same nodes in float64 and float32, none
    of them within 1e-3 (relative) of the eps32 that decides; the falling 4PL start has d < c; and from both the float64 method
    stops no item in 64 steps and the float32 restatement meets rule 1 at half the constant."""
    cs, L = mc.case(mc.STEEP_CASE), mc.steep_launch()
    assert cs["model"] == "irt_3pl" and cs["span"] == 6.0 and (L["p0"][1] == mc.STEEP_A).all()
    for j in np.flatnonzero(mc.answered(L)):
        z, in64 = mc.node_masks(cs, L["p0"][:, j], np.float64)
        _, in32 = mc.node_masks(cs, L["p0"][:, j], np.float32)
        assert np.array_equal(in64, in32) and 0 < (~in64).sum() < cs["G"], (j, (~in64).sum())
        Q = (1 - mc._sig(np.float64(L["p0"][4, j]))) * mc._sig(-z)
        assert (np.abs(Q / mc.EPS32 - 1) > 1e-3).all()
    cf, Lf = mc.case(mc.FALLING_CASE), mc.falling_launch()
    assert cf["model"] == "irt_4pl" and Lf["p0"][5, mc.FALLING_ITEM] < Lf["p0"][4, mc.FALLING_ITEM] and mc.answered(Lf)[mc.FALLING_ITEM]
    for tag, c, l in (("steep", cs, L), ("falling", cf, Lf)):
        st, st32 = {}, {}
        mc.map_mstep(c, l["n1"], l["n0"], l["p0"].astype(np.float64), l["prior"].astype(np.float64), 64, stats=st)
        p32 = mc.map_mstep(c, l["n1"], l["n0"], l["p0"], l["prior"], 64, np.float32, stats=st32)
        gain, dev, last = mc.rule1(c, l, p32)
        print("%s start: float32 restatement gains at most %.3g (C_Q / 2 = %g), parameters at most %.3g; %s / %s"
              % (tag, gain.max(), mc.C_Q / 2, dev.max(), st, st32))
        assert st["stopped"] == 0 and st32["stopped"] == 0 and np.isfinite(p32).all()
        assert last <= 1e-6 and gain.min() >= 0 and gain.max() <= mc.C_Q / 2 and dev.max() <= np.sqrt(0.5)


def test_unread_rows_are_where_the_header_says():
    """unread_nan: NaN exactly at the masked loadings, the a rows at or beyond D (all three for 1PL) and the c / d rows the model
    lacks, of means and precisions alike -- and at nothing the float64 oracle reads."""
    want = {"map9_2pl_d3_j7_g343": 3 + 2 * 7, "map8_4pl_d2_j6_g225": 1 + 6, "map7_1pl_j7_g61": 5 * 7}
    for name, n in want.items():
        cs, L = mc.case(name), mc.launch(name)
        pr = mc.unread_nan(cs, L)
        assert np.isnan(pr[0]).sum() == n and np.array_equal(np.isnan(pr[0]), np.isnan(pr[1])) and np.array_equal(np.isnan(pr[0]), ~L["free"])
        p = mc.map_mstep(cs, L["n1"], L["n0"], L["p0"], np.where(np.isnan(pr), 1e30, pr), 1, np.float32)
        assert p.tobytes() == mc.map_mstep(cs, L["n1"], L["n0"], L["p0"], L["prior"], 1, np.float32).tobytes()
