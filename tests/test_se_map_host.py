"""item_information(prior=) / item_se(prior=) and vx_grid_wtable_irt_map, the parts that need no GPU: the declarations, the gates,
the refusals, the host layer with a precision, the float64 oracle of tests/se_map_cases.py against itself (central differences
of the log posterior), the float32 + fp16-pair restatement of the kernels' arithmetic against the rules the GPU tests hold the
kernels to, what the cases promise, and the whole path on a numpy backend."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import score_cases as sc
from tests import se_cases as se
from tests import se_map_cases as sm
from tests.oracle_backend import OracleBackend
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BOTH = [(name, n) for name in sm.IDS for n in (sm.N_INFO, sm.N_SE)]
BOTH_IDS = ["%s_n%d" % c for c in BOTH]


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
    m = re.search(r"\bint\s+vx_grid_wtable_irt_map\s*\(([^;]*)\)\s*;", header)
    assert m, "include/vipsy_amd.h does not declare vx_grid_wtable_irt_map"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 9 and args[0].startswith("const vx_irt_cfg*") and args[-1] == "void* hip_stream"
    assert [a.split()[-1] for a in args[3:8]] == ["a", "b", "c_un", "d_un", "wimg"]
    res, sig = _hip.SIGNATURES["vx_grid_wtable_irt_map"]
    assert res is ctypes.c_int and len(sig) == 9
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "vx_grid_wtable_irt_map") and callable(HipBackend.grid_wtable_irt_map)
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9 and _hip.lib().vx_abi_version() == 9
    assert "K <= 6" in header


def test_every_gate_row_refuses_before_the_runtime():
    _build()
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import se_map_gates as sg
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "se_map_gates.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [l for l, _ in got] == [l for l, _ in sg.TABLE_ROWS + sg.INFO_ROWS]
    assert not [(l, rc) for l, rc in got if rc != -1]
    assert {"model 0", "model 5", "D 4", "1PL with D 2", "2PL without a", "3PL without c_un", "4PL without d_un", "J 1025", "G 1025",
            "wimg off by 4 bytes", "no theta", "vx_grid_info with K 7", "vx_grid_info with K 6, J 683"} <= {l for l, _ in got}


def test_the_new_k_limit_in_the_size_queries():
    """682 items of six unknowns fit, 683 do not; the plans depend on P alone."""
    from vipsy_amd import _hip
    L = _hip.lib()
    assert L.vx_grid_wimage_bytes(682 * 6, 125) > 0 and L.vx_grid_wimage_bytes(683 * 6, 125) == -1
    assert L.vx_grid_info_workspace_min_floats(682 * 6, 125) > 0 and L.vx_grid_info_workspace_min_floats(683 * 6, 125) == -1


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


BAD_PRIORS = [
    ("irt_3pl", [("c", (-1.4, 1.0))], "dict"),                                               # not a dict
    ("irt_3pl", {"c": (-1.4, 1.0), "e": (0.0, 1.0)}, "unknown key"),
    ("irt_3pl", {"c": (-1.4, 1.0), "d": (2.2, 1.0)}, "no such parameter"),
    ("irt_2pl", {"c": (-1.4, 1.0)}, "no such parameter"),
    ("irt_3pl", {"c": (-1.4, 1.0, 2.0)}, "pair"),
    ("irt_3pl", {"c": -1.4}, "pair"),
    ("irt_3pl", {"c": (np.zeros((1, 11)), 1.0)}, "shaped like the leaf"),
    ("irt_3pl", {"c": (np.nan, 1.0)}, "finite"),
    ("irt_3pl", {"c": (-1.4, 0.0)}, "sd must be > 0"),
    ("irt_3pl", {"c": (-1.4, -1.0)}, "sd must be > 0"),
    ("irt_3pl", {"c": (-1.4, 1e-30)}, "finite float32"),
    ("irt_3pl", {"a": (1.0, 1.0)}, "guessing"),                                              # 3PL without a finite sd on c
    ("irt_3pl", {"c": (-1.4, np.inf)}, "guessing"),
    ("irt_4pl", {"c": (-1.4, 1.0)}, "slipping"),                                             # 4PL without one on d
    ("irt_4pl", {"d": (2.2, 1.0)}, "guessing"),
]


@pytest.mark.parametrize("model,prior,word", BAD_PRIORS, ids=["%s-%s-%d" % (m, w.split()[0], i) for i, (m, _, w) in enumerate(BAD_PRIORS)])
def test_every_value_error_of_prior(model, prior, word):
    """The rules and ValueErrors of fit_em's `prior` (grid.em_prior), raised by both methods before anything is computed: the
    backend here has no grid entry at all."""
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model=model, backend=OracleBackend())
    for call in (m.item_information, m.item_se):
        with pytest.raises(ValueError) as e:
            call(prior=prior)
        assert word in str(e.value), str(e.value)


def test_vccdm_refuses_a_prior_and_the_old_refusals_stand():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    m = vi.VCCDM(data=_y(), q=q, backend=OracleBackend())
    for call in (m.item_information, m.item_se):
        with pytest.raises(ValueError) as e:
            call(prior={"b": (0.0, 1.0)})
        assert "CcdmEngine" in str(e.value) and "prior" in str(e.value)
    # without a prior: irt_3pl / irt_4pl refuse as before, and the message says what opens them
    for model in ("irt_3pl", "irt_4pl"):
        v = vi.VIRT(data=_y(), model=model, backend=OracleBackend())
        for call in (v.item_information, v.item_se):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert model in str(e.value) and "prior=" in str(e.value)
    # x_feature > 3 and the classes score() refuses: a prior changes nothing
    v = vi.VIRT(data=_y(), model="irt_3pl", x_feature=4, backend=OracleBackend())
    for cls_m in (v, vi.VCDM(data=_y(), q=q, backend=OracleBackend()), vi.VCHoDina(data=_y(), q=q, backend=OracleBackend())):
        for call in (cls_m.item_information, cls_m.item_se):
            with pytest.raises(NotImplementedError):
                call(prior={"c": (-1.4, 1.0)})


def test_model_classes_take_the_argument_and_say_what_the_matrix_is():
    import inspect
    from vipsy_amd import vi
    from vipsy_amd.engine import IrtEngine
    from vipsy_amd.grid import item_se_host
    for obj in (vi.BasePsy, IrtEngine):
        for name in ("item_information", "item_se"):
            f = getattr(obj, name)
            assert inspect.signature(f).parameters["prior"].default is None
            assert "prior" in f.__doc__
        doc = " ".join(obj.item_se.__doc__.split())
        assert "precision" in doc and "posterior covariance" in doc and "posterior mode" in doc and "AS THEY STAND" in doc
    assert inspect.signature(item_se_host).parameters["precision"].default is None


# ---- the host layer ------------------------------------------------------------------------------------------------------------
def test_host_layer_without_a_precision_is_the_former_one():
    """precision=None: the outputs of the call without the argument, bit for bit, and those of the inverse of the kept block."""
    from vipsy_amd.grid import item_se_host
    cs, o = sm.oracle_of(sm.IDS[0], sm.N_SE)
    a = item_se_host(o["info"], o["gradient"], o["free"])
    b = item_se_host(o["info"], o["gradient"], o["free"], precision=None)
    z = item_se_host(o["info"], o["gradient"], o["free"], precision=np.zeros(len(o["free"])))
    for other in (b, z):
        assert set(a) == set(other) == {"se", "cov", "kept", "gradient_max", "condition"}
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(other[k]), equal_nan=True), k
    k = o["kept"]
    want = np.sqrt(np.diag(np.linalg.inv(o["info"][np.ix_(k, k)])))
    assert np.array_equal(a["kept"], k) and np.allclose(a["se"][k], want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", sm.IDS)
def test_host_layer_with_a_precision(name):
    """On the oracle's matrix: its se, cov, kept and condition; kept follows the likelihood's diagonal -- the unanswered item
    has a prior on every unknown and stays NaN --; the gradient is taken as handed over."""
    from vipsy_amd.grid import item_se_host
    cs, o = sm.oracle_of(name, sm.N_SE)
    K = o["K"]
    dead = sm.UNANSWERED * K + np.arange(K)
    assert (o["prior_precision"][dead][[0, K - 1]] >= 0).all() and o["prior_precision"][dead[-1]] > 0
    g = o["gradient"] + o["prior_gradient"]
    h = item_se_host(o["info"], g, o["free"], precision=o["prior_precision"])
    assert np.array_equal(h["kept"], o["kept"]) and not set(dead) & set(h["kept"])
    assert np.isnan(h["se"][dead]).all() and np.array_equal(np.isnan(h["se"]), np.isnan(o["se"]))
    assert np.allclose(h["se"][o["kept"]], o["se"][o["kept"]], rtol=1e-9, atol=0) and np.allclose(h["cov"], o["cov"], rtol=1e-7, atol=1e-12)
    assert abs(h["condition"] / o["condition"] - 1) < 1e-9 and h["gradient_max"] == float(np.abs(g[o["kept"]]).max())
    alone = item_se_host(o["info"], o["gradient"], o["free"])
    assert (h["se"][o["kept"]] < alone["se"][o["kept"]]).all()
    for bad in (np.ones(3), -o["prior_precision"] - 1, np.full(len(g), np.nan)):
        with pytest.raises(ValueError):
            item_se_host(o["info"], g, o["free"], precision=bad)


# ---- the oracle against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.IDS)
def test_oracle_gradient_is_the_central_difference_of_the_log_posterior(name):
    """gradient + prior_gradient (Fisher's identity through the tables) against central differences of the float64 marginal
    log-likelihood plus log prior, which never sees a derivative: the error falls about fourfold when the step halves (it is
    the h^2 term), and the finer step meets the row rule with the gradient's floor."""
    cs, o = sm.oracle_of(name, sm.N_INFO)
    v = sm.dense(cs, cs["params"])
    ana = o["gradient"] + o["prior_gradient"]
    cols = np.flatnonzero(np.diag(o["info"]) != 0)                              # (masked loadings have a likelihood gradient too)
    floor = np.sqrt(np.abs(np.diag(o["info"])).max() * o["n"])
    errs = []
    for h in (4e-2, 2e-2):
        num = np.zeros(len(v))
        for c in cols:
            e = np.zeros(len(v))
            e[c] = h
            num[c] = (sm.logpost(cs, v + e, cs["y"]) - sm.logpost(cs, v - e, cs["y"])) / (2 * h)
        want = np.where(o["free"], ana, o["gradient"])                          # (no prior on what is not free)
        errs.append(float(np.abs(num[cols] - want[cols]).max()) / floor)
    print("%s: central differences against the analytic gradient: %.2e at h = 0.04, %.2e at h = 0.02 (floor %.1f)" % (name, errs[0], errs[1], floor))
    assert 3.0 <= errs[0] / errs[1] <= 5.0, errs
    assert errs[1] <= ROW_TOL, errs


@pytest.mark.parametrize("name", sm.IDS)
def test_oracle_gradient_is_the_penalised_m_steps(name):
    """... and what map_cases.item_eval, which says the cell on its own, forms from the oracle's own n1 / n0."""
    cs, o = sm.oracle_of(name, sm.N_INFO)
    want = sm.mstep_gradient(cs, o["n1"], o["n0"])
    got = np.where(o["free"], o["gradient"] + o["prior_gradient"], o["gradient"])
    assert np.abs(got - want).max() <= 1e-9 * np.sqrt(np.abs(np.diag(o["info"])).max() * o["n"])
    ll = sc.irt_grid_loglik(cs["model"], cs["theta"], cs["params"], cs["Dc"], cs["y"])
    # the oracle's log-likelihood is the cell's but for the reference's constant of a missing cell, -log1p(eps32) each: the same
    # at every node and every parameter, so neither the posterior nor a derivative sees it
    miss = (cs["y"] == 255).sum(1) * -np.log1p(sm.EPS32)
    assert np.allclose(sm.grid_loglik(cs, cs["params"], cs["y"]) + miss[:, None], ll, rtol=1e-10, atol=1e-10)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", BOTH, ids=BOTH_IDS)
def test_the_method_leaves_a_wide_margin_under_the_rules(name, n):
    """The kernels' arithmetic in numpy meets a third of ROW_TOL on info and gradient and a third of ROW_TOL x condition on the
    standard errors, on every case: the rules of tests/test_gpu_se_map.py are not fitted to the kernels."""
    from vipsy_amd.grid import item_se_host
    cs, o = sm.oracle_of(name, n)
    r = sm.restated_f32(cs)
    e_i, row, e_g = sm.info_errors(r["info"], r["gradient"], o["info"], o["gradient"], o["n"])
    h = item_se_host(r["info"], r["gradient"].astype(np.float64) + o["prior_gradient"], o["free"], precision=o["prior_precision"])
    e_se = float(np.nanmax(np.abs(h["se"] / o["se"] - 1)))
    print("%s, %d persons: restated info %.2e gradient %.2e (rule / 3: %.1e), se %.2e (rule / 3: %.2e); largest |W| %.3f, scale 2^%d"
          % (name, n, e_i, e_g, ROW_TOL / 3, e_se, ROW_TOL * o["condition"] / 3, r["top"], int(np.log2(r["scale"]))))
    assert e_i <= ROW_TOL / 3 and e_g <= ROW_TOL / 3, (e_i, row, e_g)
    assert np.array_equal(h["kept"], o["kept"]) and e_se <= ROW_TOL * o["condition"] / 3
    assert r["top"] * r["scale"] < 2.0 ** 15 <= 2 * r["top"] * r["scale"]        # the image's bound, and no bit given away


# ---- what the cases promise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.IDS)
def test_cases_keep_their_promises(name):
    cs, o = sm.oracle_of(name, sm.N_SE)
    spec = sm.CASES[name]
    K, J, D = o["K"], cs["J"], cs["D"]
    assert K == D + (2 if cs["model"] == "irt_3pl" else 3) and len(o["free"]) == J * K and cs["G"] == spec["nodes"] ** D
    t = sm.cell(cs, cs["params"])
    assert min(t["P"].min(), t["Q"].min()) >= sm.PQ_MIN and t["inside"].all()
    t32 = sm.cell(cs, cs["params"], np.float32)
    assert t32["inside"].all()
    assert o["condition"] <= se.CONDITION_MAX, o["condition"]
    y = cs["y"]
    assert y.shape == (sm.N_SE, J) and (y[:, sm.UNANSWERED] == 255).all() and sm.case(name, sm.N_INFO)["y"].shape == (sm.N_INFO, J)
    rest = np.delete(y, sm.UNANSWERED, axis=1)
    assert 0.17 <= (rest == 255).mean() <= 0.23 and ((rest != 255).sum(0) > 0).all()
    assert (~o["free"]).sum() == D * (D - 1) // 2 and o["free"].reshape(J, K)[sm.UNANSWERED].all()
    assert len(o["kept"]) == o["free"].sum() - K                                # the unanswered item's columns, and only they
    assert set(cs["prior"]) == ({"a", "c"} if cs["model"] == "irt_3pl" else {"a", "c", "d"})


def test_the_shapes_sit_where_the_code_can_go_wrong():
    P = {name: sm.CASES[name]["J"] * sm.K_of(sm.case(name)) for name in sm.IDS}
    assert P == {"sm1_3pl_d1_j11": 33, "sm2_4pl_d1_j8": 32, "sm3_3pl_d2_j13": 52, "sm4_4pl_d3_j7": 42}
    assert sm.K_of(sm.case("sm4_4pl_d3_j7")) == 6 and sm.case("sm4_4pl_d3_j7")["G"] == 125 and sm.case("sm3_3pl_d2_j13")["G"] == 49
    assert sm.N_INFO == se.SLAB + 44


def test_the_falling_item_is_one():
    cs = sm.case(sm.FALLING_CASE)
    j = sm.FALLING_ITEM
    assert cs["params"]["d"][0, j] < cs["params"]["c"][0, j] and j != sm.UNANSWERED
    t = sm.cell(cs, cs["params"])
    assert t["d"][j] < t["c"][j] and (np.diff(t["P"][:, j]) < 0).all()                # theta ascends along the grid: P falls
    others = [i for i in range(cs["J"]) if i != j]
    assert (t["d"][others] > t["c"][others]).all()
    W1, W0, top = sm.tables(cs, cs["params"])
    K = sm.K_of(cs)
    assert (W1[:, j * K] < 0).all() and (W1[:, j * K + K - 2:j * K + K] > 0).all()   # dP/db < 0; the asymptotes still push P up
    assert (cs["y"][:, j] != 255).sum() > 1500


# ---- end to end on a numpy backend -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sm1_3pl_d1_j11", "sm4_4pl_d3_j7"])
def test_the_whole_path_on_a_numpy_backend(name):
    """vi.VIRT.item_information(prior=) / item_se(prior=) through GridMixin, IrtEngine._info_call / _info_prior / _se_leaves and
    item_se_host, the backend's entries in float64 numpy (its matrix goes through float32 tensors)."""
    from vipsy_amd import vi
    cs, o = sm.oracle_of(name, sm.N_INFO)
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]), model=cs["model"], x_feature=cs["D"], D=cs["Dc"], backend=sm.SeMapOracleBackend())
    for k, v in cs["params"].items():
        m.engine.unconstrained(k).copy_(torch.from_numpy(v))
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    got = m.item_information(prior=cs["prior"], **kw)
    assert set(got) == {"info", "gradient", "n", "free", "index", "prior_precision", "prior_gradient"}
    e_i, _, e_g = sm.info_errors(got["info"].numpy(), got["gradient"].numpy(), o["info"], o["gradient"], o["n"])
    assert e_i <= 1e-6 and e_g <= 1e-6
    assert np.array_equal(got["free"].numpy(), o["free"]) and got["n"] == sm.N_INFO
    assert np.array_equal(got["index"]["k"], np.arange(len(o["free"])) % o["K"])
    for k in ("prior_precision", "prior_gradient"):
        assert got[k].dtype == np.float64 and np.allclose(got[k], o[k], rtol=1e-12, atol=0)
    out = m.item_se(prior=cs["prior"], **kw)
    J, D, K = cs["J"], cs["D"], o["K"]
    names = {"a", "b", "c_un", "c"} | ({"d_un", "d"} if cs["model"] == "irt_4pl" else set())
    assert set(out) == names | {"cov", "kept", "gradient_max", "condition"}
    dense = o["se"].reshape(J, K)
    assert out["b"].shape == out["c_un"].shape == out["c"].shape == (1, J) and out["a"].shape == (D, J)
    tol = 1e-6 * o["condition"]
    assert np.allclose(out["b"][0], dense[:, 0], rtol=tol, atol=0, equal_nan=True)
    assert np.allclose(out["a"], dense[:, 1:1 + D].T, rtol=tol, atol=0, equal_nan=True)
    assert np.allclose(out["c_un"][0], dense[:, D + 1], rtol=tol, atol=0, equal_nan=True)
    c = 1.0 / (1.0 + np.exp(-cs["params"]["c"].astype(np.float64)))
    assert np.allclose(out["c"], out["c_un"] * c * (1 - c), rtol=1e-12, atol=0, equal_nan=True)
    if cs["model"] == "irt_4pl":
        d = 1.0 / (1.0 + np.exp(-cs["params"]["d"].astype(np.float64)))
        assert np.allclose(out["d_un"][0], dense[:, D + 2], rtol=tol, atol=0, equal_nan=True)
        assert np.allclose(out["d"], out["d_un"] * d * (1 - d), rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(out["kept"], o["kept"]) and np.isnan(out["b"][0, sm.UNANSWERED]) and np.isnan(out["c"][0, sm.UNANSWERED])
    gmax = float(np.abs((o["gradient"] + o["prior_gradient"])[o["kept"]]).max())
    assert abs(out["gradient_max"] - gmax) <= 1e-5 * gmax and abs(out["condition"] / o["condition"] - 1) <= tol
    # without a prior this model still refuses
    with pytest.raises(NotImplementedError):
        m.item_se(**kw)
