"""point_estimates(), the parts that need no GPU: the declarations, the oracle's formulas against finite differences of the
log-likelihood, the caps the cases are chosen to satisfy, the method said again in float32 against the rules, the host layer on
hand-made input, the statistical sanity case in the oracle, and the refusals."""
import os
import re

import numpy as np
import pytest
import torch

from tests import point_cases as pc
from tests import score_cases as sc
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_entry_point():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9 and _hip.lib().vx_abi_version() == 9
    m = re.search(r"\bint\s+vx_grid_point_irt\s*\(([^;]*)\);", header)
    assert m
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 19
    assert len(_hip.SIGNATURES["vx_grid_point_irt"][1]) == 19
    assert hasattr(_hip.lib(), "vx_grid_point_irt")
    from vipsy_amd import grid
    for k, name in enumerate(pc.STATUS):
        assert re.search(r"#define VX_POINT_%s %d\b" % (name.upper(), k), header) and grid.POINT_STATUS[k] == name
    for name, k in grid.POINT_METHODS.items():
        assert re.search(r"#define VX_POINT_%s %d\b" % (name.upper(), k), header)
    assert (grid.POINT_CONVERGED, grid.POINT_AT_BOUND, grid.POINT_MAX_ITER, grid.POINT_SINGULAR, grid.POINT_EMPTY) == (0, 1, 2, 3, 4)


def test_entry_refuses_bad_arguments_without_a_gpu():
    """Every limit of the header, one at a time, on host pointers nothing may be read through: -1 before the runtime is touched."""
    import ctypes
    from vipsy_amd import _hip
    L = _hip.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)

    def call(model=2, D=1, J=37, nb=10, method=2, max_iter=32, tol=1e-6, bound=6.0, cap=1.0, null=None):
        cfg = _hip.IrtCfg(model, D, J, 0, 1.0, 1.0, 0, 0, 0)
        ptrs = {k: p for k in ("y", "rows", "theta0", "a", "b", "c", "d", "theta_hat", "info", "status", "iters")}
        if null:
            ptrs[null] = None
        return L.vx_grid_point_irt(ctypes.byref(cfg), ptrs["y"], ptrs["rows"], nb, ptrs["theta0"], ptrs["a"], ptrs["b"], ptrs["c"],
                                   ptrs["d"], method, max_iter, tol, bound, cap, ptrs["theta_hat"], ptrs["info"], ptrs["status"],
                                   ptrs["iters"], None)

    bad = [dict(model=0), dict(model=5), dict(D=0), dict(D=4), dict(J=0), dict(J=1025), dict(nb=0), dict(nb=-3), dict(method=-1),
           dict(method=3), dict(method=2, D=2), dict(model=1, D=2, method=0), dict(max_iter=0), dict(max_iter=256)]
    for name in ("tol", "bound", "cap"):
        bad += [{name: v} for v in (0.0, -1.0, float("inf"), float("nan"))]
    bad += [dict(null=k) for k in ("y", "theta0", "b", "a", "theta_hat", "info", "status", "iters")]
    bad += [dict(model=3, null="c"), dict(model=4, null="d")]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_model_classes_have_the_method():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, HipBackend, IrtEngine, _EngineBase
    assert callable(vi.BasePsy.point_estimates) and callable(HipBackend.grid_point_irt)
    assert IrtEngine.point_estimates is not _EngineBase.point_estimates and CcdmEngine.point_estimates is not _EngineBase.point_estimates
    doc = " ".join(IrtEngine.point_estimates.__doc__.split())
    assert "Warm" in doc and "reliability" in doc and "at_bound" in doc


# ---- the formulas ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[2], pc.CASES[3], pc.CASES[6], pc.CASES[8]], ids=[pc.IDS[k] for k in (0, 2, 3, 6, 8)])
def test_g_is_the_gradient_of_the_loglik_and_info_its_expected_curvature(case):
    """g against central differences of vo.irt_loglik (1e-6 relative to the sum of |terms|), and I against the expectation over
    y of the outer product of the per-item scores, which for a Bernoulli cell is a_d a_e P_z^2 / (P Q)."""
    from oracle import vi_oracle as vo
    cs = pc.case_of(case)
    a, b, lo, hi = pc._params(cs)
    th = np.clip(pc.eap_of(case), -3, 3)
    e = pc.evaluate(cs, th, "ml")
    four, three = cs["model"] == "irt_4pl", cs["model"] in ("irt_3pl", "irt_4pl")

    def ll(x):
        return vo.irt_loglik(cs["model"], x, a if cs["model"] != "irt_1pl" else None, b, lo if three else None, hi if four else None,
                             cs["Dc"], cs["y"])[0]                   # (a missing cell carries a constant: no slope)

    h = 1e-5
    for d in range(cs["D"]):
        step = np.zeros_like(th)
        step[:, d] = h
        fd = (ll(th + step) - ll(th - step)) / (2 * h)
        scale = np.maximum(np.abs(e["g"][:, d]), 1.0)
        assert np.abs(fd - e["g"][:, d]).max() <= 1e-6 * scale.max() * cs["J"], (case[0], d)
    # a second way to I: the derivative of the EXPECTED score, -d/dtheta sum_j (P_j(theta) - P_j(theta0)) P_z / (P Q) a, at theta0
    z = cs["Dc"] * (th @ a + b)
    P = lo + (hi - lo) * vo.sigmoid(z)
    pz = (hi - lo) * vo.sigmoid(z) * vo.sigmoid(-z)
    m = cs["y"] < 2
    want = cs["Dc"] ** 2 * np.einsum("nj,dj,ej->nde", np.where(m, pz * pz / (P * (1 - P)), 0.0), a, a)
    assert np.abs(want - e["info"]).max() <= 1e-10 * max(1.0, np.abs(want).max())
    assert (e["info_abs"] >= np.abs(e["info"]) - 1e-12).all()


def test_wle_of_a_rasch_test_is_finite_where_ml_is_not_and_solves_warms_equation():
    """Five 1PL items, every score 0 .. 5: ml runs to the bound for 0 and 5, the wle is finite, antisymmetric on a symmetric test
    and solves g + J / (2 I) = 0; the map lies between the wle's sign and zero."""
    J = 5
    cs = {"name": "rasch5", "N": 6, "J": J, "model": "irt_1pl", "D": 1, "Dc": 1.0,
          "params": {"b": np.array([[-1.0, -0.5, 0.0, 0.5, 1.0]], np.float32)},
          "y": np.array([[1] * k + [0] * (J - k) for k in range(J + 1)], np.uint8)}
    ml = pc.fisher64(cs, "ml", np.zeros((6, 1)))
    wle = pc.fisher64(cs, "wle", np.zeros((6, 1)))
    mp = pc.fisher64(cs, "map", np.zeros((6, 1)))
    assert list(ml["status"]) == [pc.AT_BOUND] + [pc.CONVERGED] * 4 + [pc.AT_BOUND]
    assert ml["theta_hat"][0, 0] == -sc.SPAN and ml["theta_hat"][5, 0] == sc.SPAN
    assert (wle["status"] == pc.CONVERGED).all() and (mp["status"] == pc.CONVERGED).all()
    w = wle["theta_hat"][:, 0]
    assert np.abs(w + w[::-1]).max() <= 1e-9 and (np.diff(w) > 0).all() and abs(w[5]) < 4.0
    assert (np.abs(w[1:5]) < np.abs(ml["theta_hat"][1:5, 0]) + 1e-12).all()          # Warm's correction pulls inward
    assert (np.abs(mp["theta_hat"][:, 0]) < np.abs(w) + 1e-12).all()                  # the prior pulls further
    e = pc.evaluate(cs, wle["theta_hat"], "wle")
    assert np.abs(e["g"]).max() <= 1e-9


# ---- the cases: chosen to satisfy the caps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case,method", pc.CASE_METHODS, ids=pc.CASE_METHOD_IDS)
def test_float64_fisher_scoring_stays_inside_the_caps(case, method):
    """tol = 1e-6, max_iter = 64 from the oracle's EAP: at most 1 % of the persons with >= 5 answers end in max_iter, nobody ends
    singular on a 2PL case, the planted persons end as planted, and the 60-step root agrees."""
    cs = pc.case_of(case)
    r = pc.fisher64(cs, method, pc.eap_of(case), max_iter=pc.MAX_ITER, tol=pc.TOL)
    n_obs = (cs["y"] < 2).sum(1)
    many = n_obs >= pc.MIN_ITEMS
    share = float((r["status"][many] == pc.MAX_ITERS).mean()) if many.any() else 0.0
    counts = {pc.STATUS[k]: int((r["status"] == k).sum()) for k in range(5)}
    print("%s %s: %s; iterations max %d, mean %.1f; max_iter share among >= 5 answers %.3f"
          % (case[0], method, counts, r["iterations"].max(), r["iterations"][r["iterations"] > 0].mean(), share))
    assert share <= pc.MAX_ITER_CAP
    if cs["model"] == "irt_2pl":
        assert counts["singular"] == 0
    assert r["status"][pc.NOBODY] == pc.EMPTY and np.isnan(r["theta_hat"][pc.NOBODY]).all()
    assert np.array_equal(r["status"] == pc.EMPTY, n_obs == 0)
    if method == "ml" and cs["D"] == 1 and cs["model"] in ("irt_1pl", "irt_2pl"):
        assert r["status"][pc.ALL_CORRECT] == pc.AT_BOUND and r["theta_hat"][pc.ALL_CORRECT, 0] == sc.SPAN
        assert r["status"][pc.ALL_WRONG] == pc.AT_BOUND and r["theta_hat"][pc.ALL_WRONG, 0] == -sc.SPAN
    root = pc.root_of(case, method)
    both = (r["status"] == pc.CONVERGED) & (root["status"] == pc.CONVERGED)
    if both.any() and pc.concave(cs):
        assert np.abs(r["theta_hat"][both] - root["theta_hat"][both]).max() <= 1e-6
    if method == "ml":
        assert np.array_equal(r["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND)


@pytest.mark.parametrize("case,method", pc.CASE_METHODS, ids=pc.CASE_METHOD_IDS)
def test_float32_restatement_meets_the_rules(case, method):
    """The method in float32 numpy (point_cases.restated_f32) from the float32 EAP, held to the rules of tests/point_cases.py:
    what the method costs by itself, printed, has to come out below POINT_C."""
    cs = pc.case_of(case)
    got = pc.restated_f32(cs, method, pc.eap_of(case).astype(np.float32))
    r = pc.ratios(cs, method, got, root=pc.root_of(case, method), tag=case[0])
    print("%s %s: s %.2f root %.2f info %.2f  (C = %g)" % (case[0], method, r["s"], r["root"], r["info"], pc.POINT_C))
    assert max(r.values()) <= pc.POINT_C, r
    if method == "ml":
        assert np.array_equal(got["status"] == pc.AT_BOUND, pc.root_of(case, method)["status"] == pc.AT_BOUND)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def test_host_layer_on_hand_made_input():
    from vipsy_amd.grid import point_estimates_host
    th = np.array([[0.5, -0.5], [1.5, 0.0], [np.nan, np.nan], [6.0, 1.0], [0.0, 0.0]], np.float32)
    tri = np.array([[4.0, 1.0, 0.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0, 1.0], [1.0, 4.0, 0.0, 0.5, 1.0]], np.float32)      # 00, 01, 11
    status = np.array([0, 0, 4, 1, 3], np.int32)
    out = point_estimates_host(th, tri, status, np.array([3, 4, 0, 9, 1], np.int32), "ml")
    assert set(out) == {"theta_hat", "se", "cov", "info", "status", "iterations", "n_converged", "reliability"}
    assert out["info"].shape == (5, 2, 2) and out["info"].dtype == np.float64 and out["info"][4, 0, 1] == 1.0 == out["info"][4, 1, 0]
    assert np.allclose(out["se"][0], [0.5, 1.0]) and np.allclose(out["se"][1], [1.0, 0.5]) and np.allclose(out["se"][3], [2 ** -0.5, 2 ** 0.5])
    assert np.isnan(out["se"][2]).all() and np.isnan(out["se"][4]).all() and np.isnan(out["cov"][2]).all() and np.isnan(out["cov"][4]).all()
    assert out["n_converged"] == 2
    assert np.allclose(out["reliability"], [1 - ((0.25 + 1.0) / 2) / 0.5, 1 - ((1.0 + 0.25) / 2) / 0.125])
    mp = point_estimates_host(th, tri, status, np.zeros(5, np.int32), "map")
    assert np.allclose(mp["se"][0], [5 ** -0.5, 2 ** -0.5]) and np.array_equal(mp["info"], out["info"])
    one = point_estimates_host(th[:1], tri[:, :1], status[:1], np.ones(1, np.int32), "ml")
    assert np.isnan(one["reliability"]).all() and one["n_converged"] == 1


def test_sanity_case_in_the_oracle():
    """4 096 x 40, 2PL, in float64 (point_cases.sanity_stats, which the GPU test applies to the kernel's results): over the
    persons with |theta| > 1.5 and status converged -- each estimate's own -- the mean of theta_hat_wle - theta is smaller in
    absolute value than that of theta_hat_ml - theta (Warm's point; measured -0.015 against +0.043), the outward bias likewise on
    the persons both converged for, and the reliability of the host layer is 1 - mean(se^2) / var.  The figures are printed."""
    from vipsy_amd.grid import point_estimates_host
    cs = pc.sanity_case()
    eap = pc.eap_of(pc.SANITY)
    assert np.corrcoef(eap[:, 0], cs["theta"][:, 0])[0, 1] > 0.85
    ml = pc.fisher64(cs, "ml", eap, max_iter=pc.MAX_ITER, tol=pc.TOL)
    wle = pc.fisher64(cs, "wle", eap, max_iter=pc.MAX_ITER, tol=pc.TOL)
    st = pc.sanity_stats(cs, ml, wle)
    print("sanity: mean error beyond 1.5: ml %.4f (%d persons) wle %.4f (%d); outward bias ml %.4f wle %.4f; wle reliability %.4f "
          "(%d converged)" % (st["mean_ml"], st["n_ml"], st["mean_wle"], st["n_wle"], st["out_ml"], st["out_wle"],
                              st["reliability"], st["n_converged"]))
    assert min(st["n_ml"], st["n_wle"]) > 300
    assert abs(st["mean_wle"]) < abs(st["mean_ml"]) and abs(st["out_wle"]) < abs(st["out_ml"])
    tri = wle["info"][:, 0, 0][None, :].astype(np.float32)
    host = point_estimates_host(np.nan_to_num(wle["theta_hat"]).astype(np.float32), tri, wle["status"], wle["iterations"], "wle")
    assert abs(host["reliability"][0] - st["reliability"]) <= 1e-4 and 0.5 < st["reliability"] < 0.95


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


def test_classes_without_grid_scores_refuse():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VCHoDina, vi.VaeCCDM, vi.VCDM):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        with pytest.raises(NotImplementedError) as e:
            m.point_estimates()
        assert type(m.engine).__name__ in str(e.value)
        with pytest.raises(NotImplementedError) as w:
            m.engine.score()
        assert str(e.value) == str(w.value)
    m = vi.VCCDM(data=_y(), q=q, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as e:
        m.point_estimates()
    assert "MAP pattern" in str(e.value) and "score()" in str(e.value)
    for call in (m.person_fit, m.fit_sums, m.item_msq, m.local_dependence, m.residual_sums):
        with pytest.raises(ValueError) as v:
            call(at="wle")
        assert "eap" in str(v.value)


def test_irt_refusals_come_before_anything_is_computed():
    from vipsy_amd import vi
    vi.clear_param_store()
    m4 = vi.VIRT(data=_y(), model="irt_2pl", x_feature=4, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        m4.engine.score()
    for method in ("wle", "ml", "map"):
        with pytest.raises(NotImplementedError) as e:
            m4.point_estimates(method=method)
        assert str(e.value) == str(want.value) and "x_feature" in str(e.value)
    m2 = vi.VIRT(data=_y(), model="irt_2pl", x_feature=2, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as e:
        m2.point_estimates()
    assert "Firth" in str(e.value) and "x_feature" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        m2.person_fit(at="wle")
    assert "Firth" in str(e.value)
    m = vi.VIRT(data=_y(), model="irt_3pl", backend=OracleBackend())
    with pytest.raises(NotImplementedError) as e:
        m.point_estimates(covariates=np.zeros((24, 1)))
    assert "covariates" in str(e.value)
    for kw in (dict(method="eap"), dict(method=None), dict(max_iter=0), dict(max_iter=256), dict(max_iter=2.5), dict(tol=0.0),
               dict(tol=float("nan")), dict(bound=-1.0), dict(bound=float("inf")), dict(tol="small")):
        with pytest.raises(ValueError):
            m.point_estimates(**kw)
    with pytest.raises(ValueError):
        m.point_estimates(data=_y(j=11))
    with pytest.raises(IndexError):
        m.engine.point_estimates(rows=[0, 24])
    for call in (m.person_fit, m.local_dependence):
        with pytest.raises(ValueError) as v:
            call(at="mle")
        assert "at must be one of" in str(v.value)
