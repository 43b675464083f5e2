"""Grid scores, the parts that need no GPU: the quadrature grid of IrtEngine.score (vipsy_amd.engine.score_grid), and the float64
oracle the GPU tests hold the kernel to (tests/score_cases.py) -- checked here on facts that need no kernel: a person without
a response gets the prior back, equal responses get equal scores, 61 nodes agree with 2 001; and the drawn cases meet the
conditions tests/test_gpu_score.py relies on (oracle PSD >= half the node spacing, at most 2 % of the persons with a tied MAP
node)."""
import os

import numpy as np
import pytest

from oracle import vi_oracle as vo
from tests import score_cases as sc
from vipsy_amd.engine import score_grid

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the grid builder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,nodes", [(1, 61), (1, 2), (2, 21), (3, 9), (2, 32), (3, 10)])
def test_grid_weights_sum_to_one_and_follow_the_normal_prior(D, nodes):
    theta, logw = score_grid(D, nodes, 6.0)
    assert theta.dtype == np.float32 and logw.dtype == np.float32
    assert theta.shape == (nodes ** D, D) and logw.shape == (nodes ** D,)
    assert abs(np.exp(logw.astype(np.float64)).sum() - 1.0) < 1e-6
    # proportional to exp(-|theta|^2 / 2): log-weight differences are the differences of the exponent
    t = theta.astype(np.float64)
    d = (logw.astype(np.float64) - logw[0]) - (-0.5 * (t ** 2).sum(1) + 0.5 * (t[0] ** 2).sum())
    assert np.abs(d).max() < 2e-5
    assert theta.min() == -6.0 and theta.max() == 6.0


def test_grid_tensor_product_order_matches_the_coordinates():
    n, D = 5, 3
    theta, logw = score_grid(D, n, 2.0)
    p = np.linspace(-2.0, 2.0, n).astype(np.float32)
    for g in (0, 1, n, n * n, 37, n ** D - 1):
        i0, i1, i2 = g // (n * n), (g // n) % n, g % n                # dimension 0 slowest
        assert tuple(theta[g]) == (p[i0], p[i1], p[i2])
    # D = 1: increasing
    t1, _ = score_grid(1, 61, 6.0)
    assert (np.diff(t1[:, 0]) > 0).all() and t1[30, 0] == 0.0


def test_grid_accepts_explicit_nodes():
    th = np.array([-1.0, 0.0, 2.0])
    lw = np.log(np.array([0.2, 0.5, 0.3]))
    theta, logw = score_grid(1, (th, lw))
    assert theta.shape == (3, 1) and np.allclose(theta[:, 0], th) and np.allclose(logw, lw)
    theta2, _ = score_grid(2, (np.zeros((4, 2)), np.full(4, np.log(0.25))))
    assert theta2.shape == (4, 2)


@pytest.mark.parametrize("D,nodes,span", [
    (0, 61, 6.0), (4, 3, 6.0), (1, 1, 6.0), (1, 0, 6.0), (1, -5, 6.0), (1, 61.5, 6.0), (1, True, 6.0), (1, 1025, 6.0),
    (2, 33, 6.0), (3, 11, 6.0), (1, 61, 0.0), (1, 61, -6.0), (1, 61, float("nan")), (1, 61, float("inf")), (1, 61, "6"),
    (2, (np.zeros(3), np.zeros(3)), 6.0), (1, (np.zeros((3, 1)), np.zeros(4)), 6.0), (1, (np.zeros((1025, 1)), np.zeros(1025)), 6.0),
    (1, (np.array([0.0, np.nan]), np.zeros(2)), 6.0), (1, (np.zeros(2),), 6.0),
])
def test_grid_refuses_bad_arguments(D, nodes, span):
    with pytest.raises(ValueError) as e:
        score_grid(D, nodes, span)
    assert len(str(e.value)) > 10                                    # says why


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def test_oracle_returns_the_prior_for_a_person_without_a_response():
    cs = sc.irt_case(sc.IRT_CASES[0])
    assert (cs["y"][5] == 255).all()
    want = sc.irt_oracle(cs)
    theta, logw = score_grid(1, cs["nodes"], cs["span"])
    w = np.exp(logw.astype(np.float64))
    mean = (w * theta[:, 0]).sum()
    sd = np.sqrt((w * (theta[:, 0] - mean) ** 2).sum())
    # (to the float32 rounding of the 61 log-weights, which the oracle renormalises and this line does not)
    assert abs(want["mean"][5, 0] - mean) < 1e-7 and abs(want["sd"][5, 0] - sd) < 1e-7
    assert abs(sd - 1.0) < 1e-3                                      # N(0, 1) on [-6, 6]
    # J cells of the reference's constant; the float32 log-weights sum to 1 within 1e-8, whose log is added
    assert want["loglik"][5] == pytest.approx(cs["J"] * np.log1p(-vo.EPS32), abs=1e-7)
    assert want["node"][5] == 30


# LSAT-6 under the 2PL estimates every textbook prints (Bock & Lieberman 1970: slopes, intercepts)
LSAT_A = np.array([[0.83, 0.72, 0.89, 0.69, 0.66]])
LSAT_B = np.array([[2.77, 0.99, 0.25, 1.28, 2.05]])


def test_oracle_on_lsat6_equal_responses_equal_scores_and_61_nodes_agree_with_2001():
    y = np.load(os.path.join(HERE, "golden", "lsat6.npz"))["y"]
    cs = {"D": 1, "nodes": 61, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "y": y, "params": {"a": LSAT_A, "b": LSAT_B}}
    w61 = sc.irt_oracle(cs)
    key = (y.astype(np.int64) * (1 << np.arange(5))).sum(1)
    assert len(np.unique(key)) <= 32
    for k in np.unique(key):
        rows = np.flatnonzero(key == k)
        for name in ("loglik", "mean", "sd", "node"):
            assert (w61[name][rows] == w61[name][rows[0]]).all(), (k, name)
    # 2 001 nodes: an explicit grid (beyond the kernel's limit, so built here), the same rule for the weights
    p = np.linspace(-6.0, 6.0, 2001)
    lw = -0.5 * p ** 2
    lw -= np.log(np.exp(lw).sum())
    ll = sc.irt_grid_loglik("irt_2pl", p[:, None], cs["params"], 1.0, y)
    w2001 = sc.grid_posterior(ll, lw, p[:, None])
    d_eap = float(np.abs(w61["mean"] - w2001["mean"]).max())
    d_psd = float(np.abs(w61["sd"] - w2001["sd"]).max())
    d_ll = float(np.abs(w61["loglik"] - w2001["loglik"]).max())
    print("lsat6: 61 against 2001 nodes: |d eap| %.3e  |d psd| %.3e  |d loglik| %.3e" % (d_eap, d_psd, d_ll))
    # found: |d eap| 6.0e-7, |d psd| 1.5e-6, |d loglik| 1.4e-7 -- asserted at ten times that
    assert d_eap <= 6.0e-6 and d_psd <= 1.5e-5 and d_ll <= 1.4e-6


@pytest.mark.parametrize("case", sc.IRT_CASES, ids=[c[0] for c in sc.IRT_CASES])
def test_irt_cases_meet_the_conditions_of_the_gpu_test(case):
    cs = sc.irt_case(case)
    want = sc.irt_oracle(cs)
    lo, need = sc.irt_condition(cs, want)
    out = sc.left_out(want)
    print("%s: smallest oracle PSD %.3f (needs >= %.3f), %.1f %% of the persons with a tied MAP node"
          % (cs["name"], lo, need, 100 * out))
    assert lo >= need
    assert out <= sc.ARGMAX_LEFT_OUT
    assert np.isfinite(want["loglik"]).all()


@pytest.mark.parametrize("case", sc.CDM_CASES, ids=[c[0] for c in sc.CDM_CASES])
def test_cdm_cases_meet_the_conditions_of_the_gpu_test(case):
    cs = sc.cdm_case(case)
    want = sc.cdm_oracle(cs)
    out = sc.left_out(want)
    print("%s: %.1f %% of the persons with a tied MAP pattern" % (cs["name"], 100 * out))
    assert out <= sc.ARGMAX_LEFT_OUT
    assert ((want["mean"] >= 0) & (want["mean"] <= 1)).all()
    if cs["cdm"] == "dino":
        assert (cs["q"].sum(0) == 1).any()                           # single-attribute items are part of the case
