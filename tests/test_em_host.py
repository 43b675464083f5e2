"""fit_em, the parts that need no GPU: the conditions under which the float64 oracle of tests/em_cases.py is a fair yardstick
(checked on the oracle alone), the kernel's method said again in float32 numpy against it, the declarations, and the refusals.

The stand-in figures are the stand-in's, not a kernel's: float32 Newton on float32 tables, and the float32 + fp16-pair tables of
count_cases.restated_f32 through the float64 M-step, each against the float64 maximiser of the float64 tables."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import count_cases as cc
from tests import em_cases as ec
from tests import score_cases as sc
from tests.oracle_backend import OracleBackend
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ec.ALL_EM, ids=[c[0] for c in ec.ALL_EM])
def test_oracle_conditions(case):
    """Both responses observed on every compared IRT item (a constant item has its maximiser at infinity), no halving, no
    capped step and no stopped item in the oracle's Newton on these starts, and a log-likelihood that rises in each of the
    first six iterations."""
    cs, kind, ps, lks, stats = ec.trajectory(case, 7)
    if kind == "irt":
        y = cs["y"]
        minority = np.minimum((y == 1).sum(0), (y == 0).sum(0))
        assert minority.min() >= 1, (cs["name"], minority)
        if case == ec.ONEPL:
            assert minority.min() >= 35, minority.min()
        assert stats == {"halvings": 0, "capped": 0, "stopped": 0}, (cs["name"], stats)
    rises = [(lks[k + 1] - lks[k]) / abs(lks[k]) for k in range(6)]
    print(cs["name"], "smallest relative rise of the first six iterations: %.2e" % min(rises))
    assert min(rises) > 0, (cs["name"], rises)
    for p in ps:
        for v in p.values():
            assert np.isfinite(v).all()


def test_the_1pl_case_is_drawn_as_documented():
    cs = ec.onepl_case()
    assert cs["y"].shape == (300, 50) and cs["Dc"] == 1.702 and cs["nodes"] == 41
    assert np.abs(cs["params"]["b"]).max() <= 1.5
    assert 0.07 < (cs["y"] == 255).mean() < 0.13


def test_the_design_case():
    cs = ec.design_case()
    y = cs["y"]
    assert (y[:, ec.DESIGN_UNANSWERED] == 255).all()
    col = y[:, ec.DESIGN_CONSTANT]
    assert (col[col != 255] == 1).all() and (col != 255).sum() >= 10
    # the oracle leaves the unanswered item alone and every value finite
    p0 = {k: v.astype(np.float64) for k, v in ec.start_of(cs, "irt").items()}
    p1, _ = ec.em_iteration(cs, "irt", p0, y=y)
    assert p1["a"][0, ec.DESIGN_UNANSWERED] == p0["a"][0, ec.DESIGN_UNANSWERED] and p1["b"][0, ec.DESIGN_UNANSWERED] == 0
    assert np.isfinite(p1["a"]).all() and np.isfinite(p1["b"]).all()


@pytest.mark.parametrize("case", ec.IRT_EM, ids=[c[0] for c in ec.IRT_EM])
def test_the_method_leaves_a_wide_margin_under_the_row_rule(case):
    """The M-step's arithmetic in float32 numpy against the float64 maximiser (25 Newton steps from the case's start on the tables
    of the start): float32 Newton on the float32-rounded tables, and the restated float32 + fp16-pair tables through the float64
    M-step.  Printed; asserted at an eighth of the rule the GPU test uses."""
    cs, kind = ec.case_of(case)
    theta, logw = ec.grid_of(cs)
    start = ec.start_of(cs, kind)
    free = ec.a_free_of(cs)
    ll = sc.irt_grid_loglik(cs["model"], theta, start, cs["Dc"], cs["y"])
    t64 = cc.counts(ll, logw, cs["y"])
    a64, b64 = ec.newton_mstep(cs["model"], theta, cs["Dc"], t64["n1"], t64["n0"], start.get("a"), start["b"], free, 25)
    a32, b32 = ec.newton_mstep(cs["model"], theta, cs["Dc"], t64["n1"].astype(np.float32), t64["n0"].astype(np.float32),
                               start.get("a"), start["b"], free, 25, dtype=np.float32)
    t32 = cc.restated_f32(ll, logw, cs["y"])
    at, bt = ec.newton_mstep(cs["model"], theta, cs["Dc"], t32["n1"], t32["n0"], start.get("a"), start["b"], free, 25)
    errs = {"b newton32": np.abs(b32 - b64).max(), "b tables32": np.abs(bt - b64).max()}
    if a64 is not None:
        errs["a newton32"], errs["a tables32"] = np.abs(a32 - a64).max(), np.abs(at - a64).max()
        assert np.array_equal(a32[~free], start["a"][~free]) and np.array_equal(a64[~free], start["a"][~free].astype(np.float64))
    print(cs["name"], "  ".join("%s %.2e" % kv for kv in sorted(errs.items())))
    for k, e in errs.items():
        assert e <= ROW_TOL / 8, (cs["name"], k, e)


def test_cdm_closed_form_is_the_maximiser():
    """The closed form against a grid search of Q on one item, and the DINO rule: single-attribute items keep s."""
    cs, kind = ec.case_of(sc.CDM_CASES[2])
    start = {k: v.astype(np.float64) for k, v in ec.start_of(cs, kind).items()}
    n1, n0, _ = ec.cdm_estep(cs, start)
    g, s = ec.cdm_mstep(cs["cdm"], cs["K"], cs["q"], n1, n0, start["g"], start["s"])
    single = cs["q"].sum(0) == 1
    assert single.any() and np.array_equal(s[0, single], start["s"][0, single]) and (s[0, ~single] != start["s"][0, ~single]).all()
    from oracle import vi_oracle as vo
    eta, _ = vo.dino_eta(cs["K"], cs["q"].astype(np.float64))
    j = int(np.flatnonzero(~single)[0])
    e1 = eta[:, j] > 0
    grid = np.linspace(0.001, 0.999, 999)
    Q = n1[j, ~e1].sum() * np.log(grid) + n0[j, ~e1].sum() * np.log1p(-grid)
    assert abs(grid[Q.argmax()] - vo.sigmoid(g[0, j])) <= 1e-3


# ---- the M-step's step control: conditions of the synthetic cases, and what they tell apart ----------------------------------
STEP_IDS = [c["name"] for c in ec.STEP_CASES]


@pytest.mark.parametrize("spec", ec.STEP_CASES, ids=STEP_IDS)
def test_step_case_conditions(spec):
    """The conditions under which the float64 oracle is a fair yardstick for a launch of STEP_CASES, on the oracle alone.
    Each item takes the path it is named for and full Newton steps after it.  No node comes within 1e-3 of +-ZL in any
    evaluation.  The float32 run takes the same decisions in all 64 steps and stays within an eighth of the GPU test's rule at
    every budget.

    |margin| >= 1e-4 = 100 QTOL is asserted for the finite items only, and for the steps the budgets tell apart (up to one
    past the item's last capped or halved step): it cannot hold for every decision.  A converged finite item (budget 25) and
    the last steps of a constant item to the clamp leave Q unchanged, so their margin is QTOL itself (1.0e-6 in float64,
    9.8e-7 in float32).  A constant item is held to this instead: Q never falls on the way to the clamp (each node's term
    rises), in float32 as in float64, so every step is accepted at once in both, and the item stops on a pivot of exactly
    zero with every node clamped."""
    c = ec.step_case(spec)
    assert c["J"] % 4 != 0, c["J"]
    _, _, tr = ec.step_run(spec, ec.STEP_MAX)
    _, _, tr32 = ec.step_run(spec, ec.STEP_MAX, np.float32)
    assert [r["item"] for r in tr] == list(range(c["J"]))
    smallest, edge = np.inf, np.inf
    for r, r32, it in zip(tr, tr32, spec["items"]):
        tag = (spec["name"], it["name"])
        dec, stop, at = ec.step_decisions(r)
        assert dec == [tuple(map(bool, p[:1])) + (p[1],) for p in it["path"]] + [(False, 0)] * (len(dec) - len(it["path"])), (tag, dec)
        assert ec.step_decisions(r32) == (dec, stop, at), (tag, ec.step_decisions(r32))
        if it["kind"] == "finite":
            assert stop is None and len(dec) == ec.STEP_MAX, tag
            margins = [abs(m) for s_ in r["steps"][:ec.step_last_special(r) + 1] for m in s_["margins"]]
            assert min(margins) >= 1e-4, (tag, min(margins))
            smallest = min(smallest, min(margins))
        else:
            assert stop == "pivot" and at < ec.STEP_LATE + (ec.STEP_MAX - ec.STEP_LATE) * (ec.STEP_MAX in ec.step_budgets(spec)), (tag, stop, at)
            assert r["stop_pivots"] == [0.0] and r32["stop_pivots"] == [0.0], (tag, r["stop_pivots"])
            assert r["clamped"][-1] == c["G"] and r32["clamped"][-1] == c["G"], tag
            for rr in (r, r32):
                for s_ in rr["steps"]:
                    assert len(s_["rises"]) == 1 and s_["rises"][0] >= 0, (tag, s_["rises"])
                    assert s_["m_over_cap"] <= 1.0 or s_["capped"]
        if "clamped_start" in it["name"]:
            assert r["clamped"][0] >= 1 and len(set(r["clamped"])) > 1, (tag, r["clamped"])
        assert min(r["edge"], r32["edge"]) >= 1e-3, (tag, r["edge"], r32["edge"])
        edge = min(edge, r["edge"], r32["edge"])
    worst = 0.0
    for n in ec.step_budgets(spec):
        a64, b64, _ = ec.step_run(spec, n)
        a32, b32, _ = ec.step_run(spec, n, np.float32)
        e = [x for x in ec.step_errors(spec, a32, b32, a64, b64, ROW_TOL / 8) if x is not None]
        assert max(e) <= 1.0, (spec["name"], n, e)
        worst = max(worst, max(e))
        if a64 is not None:                                              # masked loadings keep their bits in both
            assert np.array_equal(a64[~c["free"]], c["a0"][~c["free"]].astype(np.float64))
            assert np.array_equal(a32[~c["free"]], c["a0"][~c["free"]])
    print("%s budgets %s: smallest |margin| %.1e, nearest approach to the clamp %.1e, float32 at most %.3f of ROW_TOL / 8"
          % (spec["name"], ec.step_budgets(spec), smallest, edge, worst))


def test_step_cases_cover_the_paths():
    """Every path of the kernel's step control that an input can reach is taken by some item (all halvings exhausted is not:
    see the docstring of test_step_mutants)."""
    have = set()
    for spec in ec.STEP_CASES:
        c = ec.step_case(spec)
        _, _, tr = ec.step_run(spec, ec.STEP_MAX)
        have.add("G%d" % c["G"])
        for r, it in zip(tr, spec["items"]):
            dec, stop, at = ec.step_decisions(r)
            one, D = spec["model"] == "irt_1pl", spec["D"]
            masked = it["free"] is not None and 0 in it["free"]
            if (True, 0) in dec and it["kind"] == "finite":
                have.add("cap accepted 1pl" if one else "cap accepted 2pl")
            if any(cp and h for cp, h in dec):
                have.add("capped and halved")
            if max(h for _, h in dec) >= 2:
                have.add("two halvings in a step")
            if sum(h > 0 for _, h in dec) >= 2:
                have.add("halvings in two steps")
            if r["clamped"][0] >= 1 and len(set(r["clamped"])) > 1 and it["kind"] == "finite":
                have.add("clamped at the start")
            if masked and (dec[0][0] or dec[0][1]):
                have.add("masked D%d" % D)
            if it["kind"] == "clamp":
                have.add("1pl %s%s" % (it["truth"], " capped first" if dec[0][0] else ""))
            if it["kind"] == "contract":
                have.add("2pl %s" % it["truth"])
            assert max(h for _, h in dec) < ec.HALVINGS and stop != "halvings"
    want = {"cap accepted 1pl", "cap accepted 2pl", "capped and halved", "two halvings in a step", "halvings in two steps",
            "clamped at the start", "masked D2", "masked D3", "1pl correct", "1pl wrong", "1pl correct capped first",
            "1pl wrong capped first", "2pl correct", "2pl wrong", "G64", "G65", "G961", "G1000", "G1024"}
    assert want <= have, want - have


STEP_MUTANTS = {"halving factor 0.25": dict(halving=0.25), "cap 2": dict(cap=2.0), "cap clips each component": dict(cap_rescales=False),
                "clamped nodes in the gradient": dict(leak=True), "one Newton step more": 1, "one Newton step fewer": -1}


def _step_failures(kn, tol):
    """(launch, budget, item) of every comparison of the float32 stand-in, changed by `kn`, that breaks the GPU test's rule."""
    out = []
    for spec in ec.STEP_CASES:
        for n in ec.step_budgets(spec):
            a64, b64, _ = ec.step_run(spec, n)
            if isinstance(kn, int):                                      # (n + kn is not always a budget: not kept)
                a32, b32, _ = ec.step_run(spec, n + kn, np.float32, cache=False)
            else:
                a32, b32, _ = ec.step_run(spec, n, np.float32, **kn)
            e = ec.step_errors(spec, a32, b32, a64, b64, tol)
            out += [(spec["name"], n, ec.step_case(spec)["names"][j]) for j, x in enumerate(e) if x is not None and x > 1]
    return out


def test_step_stand_in_passes_everywhere():
    """The kernel's own method, said in float32 numpy, breaks the rule of the GPU test on no launch, budget or item."""
    assert _step_failures({}, ROW_TOL) == []


@pytest.mark.parametrize("mutant", list(STEP_MUTANTS), ids=[m.replace(" ", "_") for m in STEP_MUTANTS])
def test_step_mutants(mutant):
    """A wrong kernel, said in float32 numpy, breaks the rule of tests/test_gpu_em.py::test_step_control on some launch and
    budget (the kernel's own method breaks it nowhere: test_step_stand_in_passes_everywhere).

    Two wrong variants no reachable input exposes, and none is asserted for them.  One halving fewer (hv < GM_HALVINGS)
    differs only where the eighth halving is tried: in 9 000 random starts (2PL, D = 1 .. 3, Dc = 1 and 1.702, a from -6 to
    15, b from -20 to 20, constant items among them) the float64 oracle and the float32 run halve at most twice in a step and
    never reject all nine trials -- Q is concave and the Newton direction ascends.  qtol = 0 differs only where a trial's Q
    falls by less than 1e-6 |Q|: a decision the conditions above exclude, since the two precisions need not agree on it; at
    convergence, where such trials do occur, the outcome moves the result by less than the rule."""
    bad =_step_failures(STEP_MUTANTS[mutant], ROW_TOL)
    print(mutant, "breaks", len(bad), "comparisons, first", bad[:3])
    assert bad, mutant


@pytest.mark.parametrize("case,tol", ec.CONVERGED, ids=[c[0][0] for c in ec.CONVERGED])
def test_converged_cases_are_decided(case, tol):
    """The tol of tests/test_gpu_em.py::test_converged separates two consecutive relative rises of the oracle that differ by a
    factor >= 4, every rise up to the stop at least 5 ROW_TOL away from it."""
    cs, kind, ps, lks, _ = ec.trajectory(case, 8)
    n = ec.stop_iteration(lks, tol)
    assert n is not None and n >= 3, n
    rises = [(lks[k + 1] - lks[k]) / abs(lks[k]) for k in range(n - 1)]
    print(cs["name"], "tol %.0e stops after %d iterations; rises %s" % (tol, n, ["%.2e" % r for r in rises]))
    assert rises[-2] >= 4 * rises[-1] > 0
    assert all(r - tol >= 5 * ROW_TOL for r in rises[:-1]) and tol - rises[-1] >= 5 * ROW_TOL
    assert ec.stop_iteration(lks, 1e30) == 2


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+vx_grid_mstep_irt\s*\(\s*const vx_irt_cfg\*", header)
    assert re.search(r"\bint\s+vx_grid_mstep_cdm\s*\(\s*const vx_hodina_cfg\*", header)
    assert len(_hip.SIGNATURES["vx_grid_mstep_irt"][1]) == 10 and len(_hip.SIGNATURES["vx_grid_mstep_cdm"][1]) == 8


def test_model_classes_have_the_method():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, IrtEngine, _EngineBase
    assert callable(vi.BasePsy.fit_em) and IrtEngine.fit_em is not _EngineBase.fit_em and CcdmEngine.fit_em is not _EngineBase.fit_em
    assert "loglik[0]" in vi.BasePsy.fit_em.__doc__ and "clamp" in IrtEngine.fit_em.__doc__


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("kw", [dict(model="irt_3pl"), dict(model="irt_4pl"), dict(model="irt_2pl", x_feature=4)],
                         ids=["3pl", "4pl", "d4"])
def test_irt_models_out_of_scope_refuse(kw):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), backend=OracleBackend(), **kw)
    with pytest.raises(NotImplementedError) as e:
        m.fit_em(max_iter=2)
    assert len(str(e.value)) > 20


def test_classes_without_grid_scores_refuse():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VaeCCDM, vi.VCDM, vi.VCHoDina):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        with pytest.raises(NotImplementedError) as e:
            m.fit_em()
        assert type(m.engine).__name__ in str(e.value)


def test_bad_arguments_are_value_errors():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", backend=OracleBackend())
    for kw in (dict(max_iter=0), dict(newton=0), dict(newton=65), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            m.fit_em(**kw)


def test_two_ranks_refuse(tmp_path):
    """A gloo group of two: the model class and the engine both refuse, before anything is computed."""
    worker = os.path.join(ROOT, "tests", "_em_dist_worker.py")
    out = str(tmp_path / "em_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29651", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29651", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            assert f.read().split() == ["NotImplementedError", "NotImplementedError"]
