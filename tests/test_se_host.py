"""item_information / item_se, the parts that need no GPU: the conditions under which the float64 oracle of tests/se_cases.py is a
fair yardstick (checked on the oracle alone), the kernels' arithmetic said again in float32 + fp16 pairs against it, the host
layer of item_se on oracle matrices, the declarations, and the refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import count_cases as cc
from tests import score_cases as sc
from tests import se_cases as se
from tests.oracle_backend import OracleBackend
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("entry", se.SE_CASES, ids=se.SE_IDS)
def test_oracle_conditions(entry):
    """A condition on the INPUTS: the kept block of every SE case is positive definite with a 2-norm condition number of at most
    1e3 in the float64 oracle -- the bound of the GPU test is 3e-5 times this number."""
    cs, kind, params, o = se.se_oracle(entry)
    P = len(o["free"])
    print("%s: P %d, kept %d, condition %.1f, largest |gradient| on the kept columns %.2e"
          % (cs["name"], P, len(o["kept"]), o["condition"], np.abs(o["gradient"][o["kept"]]).max()))
    assert "se" in o and o["condition"] <= se.CONDITION_MAX
    assert np.isfinite(o["se"][o["kept"]]).all() and np.isnan(np.delete(o["se"], o["kept"])).all()
    dropped = np.setdiff1d(np.flatnonzero(o["free"]), o["kept"])
    if cs["name"] == "se_dino_k4":
        # the s of a DINO single-attribute item: nobody is in its eta = 1 class
        single = np.flatnonzero(cs["q"].sum(0) == 1)
        assert len(single) == 4 and np.array_equal(dropped, 2 * single + 1)
        assert (o["info"][dropped] == 0).all() and (o["info"][:, dropped] == 0).all() and (o["gradient"][dropped] == 0).all()
    else:
        assert len(dropped) == 0
    if kind == "irt" and cs["D"] > 1:
        assert (~o["free"]).sum() == cs["D"] * (cs["D"] - 1) // 2 and not np.isin(np.flatnonzero(~o["free"]), o["kept"]).any()


@pytest.mark.parametrize("entry", se.SE_CASES, ids=se.SE_IDS)
def test_the_method_leaves_a_wide_margin_under_the_row_rule(entry):
    """The kernels' arithmetic in float32 + fp16 pairs (se_cases.restated_f32) against the float64 oracle: info within 1e-5 of
    max |info|, a third of the rule of the GPU test; the gradient and n likewise; the standard errors out of the restated matrix
    within a third of the GPU test's bound.  Printed."""
    cs, kind, params, o = se.se_oracle(entry)
    r = se.restated_f32(cs, kind, params)
    top = np.abs(o["info"]).max()
    e_info = np.abs(r["info"] - o["info"]).max() / top
    e_grad = np.abs(r["gradient"] - o["gradient"]).max() / np.sqrt(top * o["n"])
    k = o["kept"]
    cov = np.linalg.inv(r["info"].astype(np.float64)[np.ix_(k, k)])
    e_se = np.abs(np.sqrt(np.diag(cov)) / o["se"][k] - 1).max()
    print("%s: info %.2e of max |info|, gradient %.2e of its floor, se %.2e relative (condition %.1f)"
          % (cs["name"], e_info, e_grad, e_se, o["condition"]))
    assert e_info <= 1e-5 and e_grad <= 1e-5
    assert r["n"] == o["n"]
    assert e_se <= 1e-5 * o["condition"]


@pytest.mark.parametrize("entry", se.SE_CASES, ids=se.SE_IDS)
def test_oracle_gradient_is_the_m_steps(entry):
    """sum_i S[i] equals Dc sum_g (n1 (1 - P) - n0 P) u_g of the tables of count_cases.counts, to 1e-9 of the size of the sum's
    terms: the gradient of the information is the gradient the M-step climbs."""
    cs, kind, params, o = se.se_oracle(entry)
    J, K = cs["J"], o["K"]
    u = (o["W1"] + o["W0"]).reshape(-1, J, K)                       # (1 - P) u + P u
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(u != 0, o["W0"].reshape(-1, J, K) / u, 0.0)    # the oracle's own P, where the parameter acts
    n1, n0 = o["n1"].T[:, :, None], o["n0"].T[:, :, None]
    want = ((n1 * (1 - P) - n0 * P) * u).sum(0).reshape(-1)
    size = ((n1 * (1 - P) + n0 * P) * np.abs(u)).sum(0).reshape(-1)
    err = np.abs(o["gradient"] - want) / np.maximum(size, 1.0)
    print("%s: %.2e" % (cs["name"], err.max()))
    assert err.max() <= 1e-9
    # ... and so is what the GPU test forms from expected_counts(): the same sum with the P of the counts' own table
    again = se.mstep_gradient(cs, kind, o["n1"], o["n0"], _prob_of(cs, kind, params), params)
    assert (np.abs(again - want) / np.maximum(size, 1.0)).max() <= 1e-9


def _prob_of(cs, kind, params):
    """P(y_j = 1 | node) [J][G] as count_cases has it, from single-item response rows."""
    J = cs["J"]
    return cc._prob_from(se.grid_loglik(cs, kind, params, cc._single_item_rows(J))[0], J)


@pytest.mark.parametrize("case", se.INFO_CASES, ids=se.INFO_IDS)
def test_the_method_on_the_matrix_only_cases(case):
    """The cases whose matrix and gradient alone are compared on the GPU (drawn parameters, mostly fewer persons than
    parameters): the restated arithmetic stays within 1e-5 of max |info| there too, and the oracle's matrix is symmetric."""
    cs, kind, o = se.info_oracle(case)
    r = se.restated_f32(cs, kind, cs["params"])
    top = np.abs(o["info"]).max()
    e_info = np.abs(r["info"] - o["info"]).max() / top
    e_grad = np.abs(r["gradient"] - o["gradient"]).max() / np.sqrt(top * o["n"])
    print("%s: N %d, P %d, info %.2e of max |info|, gradient %.2e of its floor" % (cs["name"], o["n"], len(o["free"]), e_info, e_grad))
    assert e_info <= 1e-5 and e_grad <= 1e-5 and r["n"] == o["n"]
    assert np.abs(o["info"] - o["info"].T).max() <= 1e-12 * top


def test_golden_parameters_are_oracle_em_iterates():
    """tests/golden/se/se_params.npz holds, for every SE case, the oracle's parameters after iters - 1 and after iters EM iterations
    (python -m tests.se_cases writes it: two minutes of float64 numpy that the GPU suite should not repeat on every run).  One
    oracle iteration from the first gives the second, and the cheap cases are recomputed from the start."""
    from tests import em_cases as ec
    for case, iters in se.SE_CASES:
        cs, kind = se.case_of(case)
        prev, last = se.golden_params(case, iters - 1), se.golden_params(case, iters)
        assert prev is not None and last is not None, case[0]
        p, _ = ec.em_iteration(cs, kind, {k: v.astype(np.float64) for k, v in prev.items()})
        for k, v in last.items():
            # (prev was rounded to float32 when it was written: one iteration contracts that rounding, it does not grow it)
            assert np.abs(p[k] - v).max() <= 4e-7 * max(1.0, np.abs(v).max()), (case[0], k, np.abs(p[k] - v).max())
        if cs["N"] * cs["J"] <= 20000 or kind == "cdm":
            again = se.compute_params(case, iters)
            for k, v in last.items():
                assert np.array_equal(again[k], v), (case[0], k)


# ---- the host layer of item_se on oracle matrices ------------------------------------------------------------------------
def _host(o, **kw):
    from vipsy_amd.grid import item_se_host
    return item_se_host(o["info"], o["gradient"], o["free"], **kw)


@pytest.mark.parametrize("entry", se.SE_CASES, ids=se.SE_IDS)
def test_host_layer_on_oracle_matrices(entry):
    cs, kind, params, o = se.se_oracle(entry)
    got = _host(o)
    assert np.array_equal(got["kept"], o["kept"])
    assert np.array_equal(np.isnan(got["se"]), np.isnan(o["se"]))                               # fixed or dropped: NaN
    assert np.abs(got["se"][o["kept"]] / o["se"][o["kept"]] - 1).max() <= 1e-9 * o["condition"]
    assert got["cov"].shape == (len(o["kept"]),) * 2 and got["cov"].dtype == np.float64
    assert np.abs(got["cov"] - o["cov"]).max() <= 1e-9 * o["condition"] * np.abs(o["cov"]).max()
    assert abs(got["condition"] / o["condition"] - 1) <= 1e-9
    assert got["gradient_max"] == np.abs(o["gradient"][o["kept"]]).max()


def test_host_layer_follows_the_free_mask():
    """Taking a free column out of the mask takes it out of the kept block: its SE is NaN and the others are those of the smaller
    block, which are never larger."""
    cs, kind, params, o = se.se_oracle(se.SE_CASES[2])
    full = _host(o)
    free = o["free"].copy()
    free[[3, 10]] = False
    from vipsy_amd.grid import item_se_host
    part = item_se_host(o["info"], o["gradient"], free)
    assert np.array_equal(part["kept"], np.setdiff1d(o["kept"], [3, 10]))
    assert np.isnan(part["se"][[3, 10]]).all()
    rest = part["kept"]
    assert (part["se"][rest] <= full["se"][rest] * (1 + 1e-12)).all()
    want = np.sqrt(np.diag(np.linalg.inv(o["info"][np.ix_(rest, rest)])))
    assert np.abs(part["se"][rest] / want - 1).max() <= 1e-9


def test_host_layer_refuses_a_singular_block():
    """case1: 33 persons, 74 parameters.  No pseudo-inverse: ValueError, with the parameter of the smallest pivot in it."""
    cs, kind, o = se.info_oracle(sc.IRT_CASES[0])
    with pytest.raises(ValueError) as e:
        _host(o, names=lambda c: "item %d, parameter %d" % (c // 2, c % 2))
    assert re.search(r"pivot -?\d\.\d+e[-+]\d+ at item \d+, parameter [01]", str(e.value)), str(e.value)
    with pytest.raises(ValueError) as e:
        _host(o)
    assert "column" in str(e.value)
    from vipsy_amd.grid import item_se_host
    with pytest.raises(ValueError):
        item_se_host(np.eye(3), np.zeros(2), np.ones(3, bool))


def test_engine_shapes_and_the_delta_method():
    """Dense standard errors -> the leaves' shapes, through the engines (an OracleBackend: nothing is computed on a device)."""
    from vipsy_amd import vi
    cs, kind, params, o = se.se_oracle(se.SE_CASES[6])                          # DINO: four NaN among the s
    vi.clear_param_store()
    m = vi.VCCDM(data=torch.from_numpy(cs["y"]), q=torch.from_numpy(cs["q"]), model=cs["cdm"], backend=OracleBackend())
    for name, v in params.items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v))
    out = m.engine._se_leaves(o["se"].copy())
    J = cs["J"]
    assert set(out) == {"g_un", "s_un", "g", "s"} and all(v.shape == (1, J) for v in out.values())
    assert np.array_equal(out["g_un"][0], o["se"][0::2]) and np.array_equal(out["s_un"][0], o["se"][1::2], equal_nan=True)
    from oracle import vi_oracle as vo
    for k in ("g", "s"):
        x = vo.sigmoid(params[k].astype(np.float64))
        assert np.allclose(out[k], out[k + "_un"] * x * (1 - x), rtol=1e-6, atol=0, equal_nan=True)
    assert np.isnan(out["s"]).sum() == 4 and np.isfinite(out["g"]).all()
    cs, kind, params, o = se.se_oracle(se.SE_CASES[3])                          # 2PL, two dimensions: one loading is fixed
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]), model="irt_2pl", x_feature=2, backend=OracleBackend())
    out = m.engine._se_leaves(o["se"].copy())
    assert set(out) == {"a", "b"} and out["a"].shape == (2, cs["J"]) and out["b"].shape == (1, cs["J"])
    from tests import em_cases as ec
    assert np.array_equal(np.isnan(out["a"]), ~ec.a_free_of(cs)) and np.isnan(out["a"]).sum() == 1 and np.isfinite(out["b"]).all()
    assert np.array_equal(out["a"][0], o["se"][1::3]) and np.array_equal(out["b"][0], o["se"][0::3])


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    for name, nargs in (("vx_grid_wimage_bytes", 2), ("vx_grid_wtable_irt", 7), ("vx_grid_wtable_cdm", 7),
                        ("vx_grid_info_workspace_floats", 3), ("vx_grid_info_workspace_min_floats", 2), ("vx_grid_info", 15)):
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        assert len(_hip.SIGNATURES[name][1]) == nargs, name


def test_workspace_queries_answer_without_a_gpu():
    """The size queries are host arithmetic: the minimum holds one slab of 256 persons and one chunk, the preferred size is never
    below it and never above 512 MB where the minimum is below that; bad shapes are refused."""
    from vipsy_amd import _hip
    L = _hip.lib()
    for P, G in ((74, 61), (1000, 61), (160, 729), (4096, 1024), (1, 1)):
        lo = L.vx_grid_info_workspace_min_floats(P, G)
        PT = (P + 32) // 32
        assert lo == (8 * PT + 3 * PT * (PT + 1) // 2) * 1024
        for nb in (1, 256, 2500, 1000000):
            pref = L.vx_grid_info_workspace_floats(nb, P, G)
            assert lo <= pref <= max(lo, 128 << 20), (P, G, nb, lo, pref)
        assert L.vx_grid_info_workspace_floats(256, P, G) == lo
        assert L.vx_grid_wimage_bytes(P, G) == ((G + 31) // 32) * 2 * PT * 4096 + 16
    for P, G in ((0, 61), (4097, 61), (74, 0), (74, 1025)):
        assert L.vx_grid_info_workspace_min_floats(P, G) == -1 and L.vx_grid_wimage_bytes(P, G) == -1
        assert L.vx_grid_info_workspace_floats(100, P, G) == -1
    assert L.vx_grid_info_workspace_floats(0, 74, 61) == -1


def test_model_classes_have_the_methods():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, IrtEngine, _EngineBase
    for name in ("item_information", "item_se"):
        assert callable(getattr(vi.BasePsy, name))
        assert getattr(IrtEngine, name) is not getattr(_EngineBase, name) and getattr(CcdmEngine, name) is not getattr(_EngineBase, name)
        for doc in (getattr(vi.BasePsy, name).__doc__, getattr(IrtEngine, name).__doc__):
            assert "AS THEY STAND" in doc and "fit_em()" in doc and "maximum" in doc


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("kw", [dict(model="irt_3pl"), dict(model="irt_4pl"), dict(model="irt_2pl", x_feature=4)],
                         ids=["3pl", "4pl", "d4"])
def test_irt_models_out_of_scope_refuse(kw):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), backend=OracleBackend(), **kw)
    for call in (m.item_information, m.item_se):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert len(str(e.value)) > 20 and (kw["model"] in str(e.value) or "x_feature" in str(e.value))


def test_classes_without_grid_scores_refuse():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VaeCCDM, vi.VCDM, vi.VCHoDina):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        for call in (m.item_information, m.item_se):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert type(m.engine).__name__ in str(e.value)


def test_bad_data_is_refused_before_anything_is_computed():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", backend=OracleBackend())
    with pytest.raises(ValueError):
        m.item_se(data=_y(j=11))
    with pytest.raises(IndexError):
        m.engine.item_information(rows=[0, 24])
    with pytest.raises(ValueError):
        m.item_se(nodes=1)


def test_two_ranks_refuse(tmp_path):
    """A gloo group of two: the model class and the engine both refuse, before anything is computed."""
    worker = os.path.join(ROOT, "tests", "_se_dist_worker.py")
    out = str(tmp_path / "se_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29653", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            assert f.read().split() == ["NotImplementedError"] * 4
