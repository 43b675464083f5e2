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
