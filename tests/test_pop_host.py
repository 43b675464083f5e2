"""The latent regression on the CPU: the conditions the float64 oracle of tests/pop_cases.py has to meet before the GPU is held to
it (tests/test_gpu_pop.py), the tolerance of the EM comparison, measured, the host pieces of vipsy_amd/grid.py, and the two
new entries of the C ABI as the header and the binding declare them."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pop_cases as pc
from tests import score_cases as sc
from tests.test_gpu_response_designs import ROW_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frozen_estep(key):
    theta, ll = pc.grid_ll(key)
    gamma, sigma = pc.frozen(key)
    return pc.estep(ll, theta, pc.case(key)["X"], gamma, sigma)


@pytest.mark.parametrize("key", ["P1", "P2", "P3"])
def test_oracle_psd_is_above_half_the_node_spacing_under_the_conditioned_prior(key):
    cs, want = pc.case(key), _frozen_estep(key)
    lo, need = sc.irt_condition(cs, want)
    print("%s: smallest oracle PSD %.3f, half the node spacing %.3f" % (cs["name"], lo, need))
    assert lo >= need
    gamma, sigma = pc.frozen(key)
    assert np.abs(gamma).max() <= 0.6 and (cs["D"] == 1 or np.abs(sigma - np.diag(np.diag(sigma))).max() > 0.05)
    assert np.linalg.eigvalsh(sigma).min() > 0.3


def test_the_left_out_caps_hold_for_the_oracle_alone():
    for key in ("P1", "P2", "P3"):
        out = sc.left_out(_frozen_estep(key))
        print("%s: %.1f %% of the persons left out of the argmax rule" % (key, 100 * out))
        assert out <= sc.ARGMAX_LEFT_OUT
    cs, want = pc.second_unit(1)
    assert sc.left_out(want) <= sc.ARGMAX_LEFT_OUT
    for key in ("P1", "P2"):
        f = _frozen_estep(key)["f"]
        _, gap = pc.oracle_draws(f, np.arange(len(f)), pc.PV_DRAWS, pc.PV_SEED)
        out = float((gap <= pc.DRAW_GAP).mean())
        print("%s: %.3f %% of the (person, draw) pairs left out" % (key, 100 * out))
        assert out <= sc.ARGMAX_LEFT_OUT


@pytest.mark.parametrize("key,iters", [("P1", 60), ("P2", 30), ("P5", 50)])
def test_the_oracle_log_likelihood_never_falls(key, iters):
    out = pc.em_oracle(key, iters)
    h = np.array(out["loglik"])
    print("%s: %d iterations, converged %s, loglik %.4f -> %.4f, gamma[:, 0] %s, diag sigma %s"
          % (key, out["iterations"], out["converged"], h[0], h[-1], out["gamma"][:, 0], np.diag(out["sigma"])))
    assert (np.diff(h) >= -1e-9 * np.abs(h[:-1])).all()
    cs = pc.case(key)
    half = 0.5 * (2.0 * cs["span"] / (cs["nodes"] - 1))
    assert (np.diag(out["sigma"]) >= half ** 2).all()
    assert (np.abs(cs["X"] @ out["gamma"]).max(0) + 4 * np.sqrt(np.diag(out["sigma"])) <= cs["span"]).all()


def test_recovery_holds_for_the_oracle_alone():
    """P5: the OLS coefficients of the mean of 16 conditioned oracle draws a person lie within 5 Monte-Carlo standard errors of
    gamma; the dummy's slope from draws under N(0, 1) for everybody falls short of gamma's by more than those 5."""
    from vipsy_amd.grid import score_grid
    cs = pc.case("P5")
    theta, ll = pc.grid_ll("P5")
    fit = pc.em_oracle("P5", 50)
    cond = pc.estep(ll, theta, cs["X"], fit["gamma"], fit["sigma"])
    _, logw = score_grid(1, cs["nodes"], cs["span"])
    rows = np.arange(cs["N"])
    node_c, _ = pc.oracle_draws(cond["f"], rows, 16, pc.PV_SEED)
    node_u, _ = pc.oracle_draws(ll + logw.astype(np.float64)[None, :], rows, 16, pc.PV_SEED)
    t = theta[:, 0].astype(np.float64)
    z, short = pc.recovery_holds(cs["X"], fit["gamma"], t[node_c].mean(1), t[node_u].mean(1), cond["cov"][:, 0, 0])
    print("P5 oracle: gamma %s, conditioned z %s, unconditioned dummy slope short by %.1f standard errors" % (fit["gamma"][:, 0], z, short))
    assert (z <= 5.0).all()
    assert short > 5.0
    assert abs(fit["gamma"][1, 0] - 0.5) < 0.15                               # the true slope, within its sampling error


@pytest.mark.parametrize("key", ["P1", "P2"])
def test_em_tolerance_measured(key):
    """What E-step outputs inside the row rule can move Gamma, Sigma and the history by: the GPU comparison allows twice this."""
    for iters in (1, 6):
        dev = pc.em_tolerance(key, iters)
        print("%s, max_iter %d: perturbing every E-step output by +-%.0e max(|row|, 1) moves gamma by %.2e, sigma by %.2e, the "
              "loglik history by %.2e of its size" % (key, iters, ROW_TOL, dev["gamma"], dev["sigma"], dev["loglik"]))
        assert 0 < dev["gamma"] < 1e-2 and 0 < dev["sigma"] < 1e-2 and 0 < dev["loglik"] < 1e-3


def test_population_logw():
    from vipsy_amd.grid import population_logw, score_grid
    theta, logw = score_grid(2, 21, 6.0)
    lw = population_logw(theta, np.eye(2))
    assert lw.dtype == np.float32 and lw.shape == (441,) and lw.max() == 0.0
    assert np.allclose(lw - lw[0], logw - logw[0], atol=2e-6)                 # Sigma = I: the N(0, I) weights up to a shift
    sigma = np.array([[0.9, 0.3], [0.3, 0.6]])
    want = -0.5 * np.einsum("gd,de,ge->g", theta.astype(np.float64), np.linalg.inv(sigma), theta.astype(np.float64))
    assert np.abs(population_logw(theta, sigma) - (want - want.max())).max() <= 1e-5
    with pytest.raises(ValueError):
        population_logw(theta, np.eye(3))


def test_population_mstep_and_design_cholesky():
    from vipsy_amd.grid import design_cholesky, population_mstep, tri_to_full
    rng = np.random.RandomState(3)
    n, p, D = 200, 4, 3
    X = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, p - 1))], 1)
    m = rng.normal(size=(n, D))
    A = rng.normal(size=(n, D, D))
    C = A @ np.transpose(A, (0, 2, 1))
    iu = np.triu_indices(D)
    tri = C[:, iu[0], iu[1]]
    assert np.array_equal(tri_to_full(tri, D), C) or np.allclose(tri_to_full(tri, D), C, atol=1e-15)
    Xt = torch.from_numpy(X)
    L = design_cholesky(Xt)
    assert np.allclose(L @ L.T, X.T @ X)
    gamma, sigma = population_mstep(Xt, L, torch.from_numpy(m.astype(np.float32)), torch.from_numpy(tri.astype(np.float32)))
    g_want, s_want = pc.mstep(X, m.astype(np.float32).astype(np.float64), tri_to_full(tri.astype(np.float32).astype(np.float64), D))
    assert gamma.dtype == np.float64 and gamma.shape == (p, D) and sigma.shape == (D, D)
    assert np.abs(gamma - g_want).max() <= 1e-12 and np.abs(sigma - s_want).max() <= 1e-12
    assert np.array_equal(sigma, sigma.T)
    bad = np.concatenate([X, 2.0 * X[:, 2:3]], 1)                              # column 4 repeats column 2
    with pytest.raises(ValueError, match="column 4"):
        design_cholesky(torch.from_numpy(bad))
    with pytest.raises(ValueError):
        population_mstep(Xt.float(), L, torch.from_numpy(m), torch.from_numpy(tri))


def test_sigma_refusals_on_the_host():
    """A diagonal entry below (half the node spacing)^2, and a Sigma whose diagonal is healthy but which is singular through a
    correlation of +-1: both the documented ValueError, before Sigma is inverted."""
    from vipsy_amd.grid import GridMixin
    GridMixin._population_check(np.array([[1.0, 0.9], [0.9, 1.0]]), 0.6)
    GridMixin._population_check(np.eye(1), 0.2)
    for sigma in (np.array([[1.0, 0.0], [0.0, 0.08]]), np.array([[1.0, 1.0], [1.0, 1.0]]), np.array([[1.0, -1.0 + 1e-9], [-1.0 + 1e-9, 1.0]]),
                  np.array([[1.0, np.nan], [np.nan, 1.0]])):
        with pytest.raises(ValueError, match="node spacing"):
            GridMixin._population_check(sigma, 0.6)
    GridMixin._population_reach(np.array([1.5]), np.array([[1.0]]), 6.0)
    with pytest.raises(ValueError, match="raise span"):
        GridMixin._population_reach(np.array([2.5]), np.array([[1.0]]), 6.0)


def test_the_collapse_case_collapses_part_way_through_the_fit():
    cs, k0 = pc.collapse_case()
    print("%s: min diag(Sigma) by iteration %s, limit %.4f" % (cs["name"], np.round(cs["diags"], 3), cs["limit"]))
    assert 5 <= k0 < 59 and (cs["diags"][:k0] >= cs["limit"] + 0.01).all() and cs["diags"][k0] < cs["limit"] - 0.01
    assert (np.diff(cs["diags"]) < 0).all()


def test_fit_population_refuses_two_ranks(tmp_path):
    """A gloo group of two: fit_population refuses through the model class and on the engine, before anything is computed, and
    no population is stored."""
    import subprocess
    import sys
    worker = os.path.join(ROOT, "tests", "_pop_dist_worker.py")
    out = str(tmp_path / "pop_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29661", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29661", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            lines = f.read().splitlines()
        assert lines[0] == "NotImplementedError NotImplementedError population=None"
        assert lines[1] == "fit_population with a group of 2 ranks: the M-step's sums are the local shard's; the cross-rank sum is not built"
        assert lines[2].startswith("fit_population over a process group: ") and lines[2].endswith("the cross-rank sum is not built")


def test_four_dimensions_refuse_with_the_wording_of_score():
    from tests.oracle_backend import OracleBackend
    from vipsy_amd import vi
    vi.clear_param_store()
    y = torch.from_numpy((np.random.RandomState(2).uniform(size=(24, 12)) < 0.5).astype(np.uint8))
    m = vi.VIRT(data=y, model="irt_2pl", x_feature=4, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        m.engine.score()
    for call in (m.fit_population, m.engine.fit_population):
        with pytest.raises(NotImplementedError) as e:
            call(np.zeros((24, 2)))
        assert str(e.value) == str(want.value) and "x_feature" in str(e.value)
    assert m.engine.population is None


def test_header_and_binding_declare_the_conditioned_entries():
    from vipsy_amd import _hip
    header = open(os.path.join(ROOT, "include", "vipsy_amd.h")).read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    for name, n_args in (("vx_grid_posterior_cond", 16), ("vx_grid_draw_cond", 17)):
        m = re.search(r"\bint %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
    assert _hip.lib().vx_abi_version() == 9
    for name in ("vx_grid_posterior_cond", "vx_grid_draw_cond"):
        assert hasattr(_hip.lib(), name)
