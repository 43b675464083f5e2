"""The latent regression on the GPU (vx_grid_posterior_cond / vx_grid_draw_cond behind IrtEngine.fit_population and the conditioned
score() / plausible_values()) against the float64 oracle of tests/pop_cases.py.

Item parameters are drawn and set through the engine's views, as tests/test_gpu_score.py does.  Per-person outputs are held to the
oracle by the project's row rule, _row_errors(got, want, floor = 1) <= ROW_TOL; nodes and draws must equal the oracle's wherever
its best two values differ by more than 1e-4, with at most 2 % left out (tests/test_pop_host.py checks on the CPU that the oracle
alone stays inside those caps).  The EM comparison allows twice what an E-step inside the row rule can move the result by, as
pop_cases.em_tolerance measures it.  The errors found are printed.

Shapes: one person tile + 1 row with ragged J and G (P1), 14 and 23 node tiles with D = 2 and 3 (P2, P3), a wave's second unit
(P4), and 2 048 persons for the statistical property the feature exists for (P5)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pop_cases as pc
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_pv import _hold_draws
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import SCHED2, _irt_engine, _np, _want

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = np.array([99, 3, 3, 64, 31, 32, 0, 98, 17, 5, 50, 63, 65, 3, 77, 12, 40, 41, 42, 96, 2, 1, 88, 70, 33, 34, 35, 36, 9, 8, 7,
                66, 67, 68, 69, 20, 21], dtype=np.int64)


def _engine(key, population=None):
    cs = pc.case(key)
    eng = _irt_engine(cs)
    if population is not None:
        eng.population = {"gamma": population[0], "sigma": population[1], "intercept": True}
    return cs, eng, {"nodes": cs["nodes"], "span": cs["span"]}


def _hold_rows(tag, pairs):
    """The row rule on every (name, got, want); prints what it finds."""
    errs = [(name,) + _row_errors(np.asarray(got, np.float64), np.asarray(want, np.float64), floor=1.0) for name, got, want in pairs]
    print("%s: %s (row rule: %.1e)" % (tag, "  ".join("%s %.2e (row %d)" % e for e in errs), ROW_TOL))
    for name, e, worst in errs:
        assert e <= ROW_TOL, (tag, name, "person", worst, e)


def _hold_nodes(tag, got, want):
    sure = want["gap"] > sc.ARGMAX_GAP
    out = 1.0 - float(sure.mean())
    wrong = np.flatnonzero(sure & (np.asarray(got, np.int64) != want["node"]))
    print("%s: %.1f %% of the persons left out of the argmax rule, %d wrong nodes" % (tag, 100 * out, len(wrong)))
    assert out <= sc.ARGMAX_LEFT_OUT, (tag, out)
    assert len(wrong) == 0, (tag, wrong[:10])


# ---- 1. a zero tilt gives today's bits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [sc.IRT_CASES[0], sc.IRT_CASES[4], sc.IRT_CASES[5]], ids=lambda c: c[0])
def test_zero_tilt_gives_the_unconditioned_bits(case):
    cs, _ = _want(case)
    eng = _irt_engine(cs)
    call = eng._grid_call(None, None, cs["nodes"], cs["span"])                  # score_grid's logw
    tilt = torch.zeros(cs["N"], cs["D"], dtype=torch.float32, device=_dev())
    old = eng._grid_posterior(call)
    new = eng._grid_posterior_cond(call, tilt)
    torch.cuda.synchronize()
    assert new["cov"].shape == (cs["N"], cs["D"] * (cs["D"] + 1) // 2)
    assert torch.equal(new["logjoint"], old["loglik"]) and torch.equal(new["mean"], old["mean"]) and torch.equal(new["node"], old["node"])
    diag = [0] if cs["D"] == 1 else ([0, 2] if cs["D"] == 2 else [0, 3, 5])
    assert np.array_equal(np.sqrt(_np(new["cov"])[:, diag]), _np(old["sd"]))       # (IEEE square roots on both sides)
    # the prior alone: the weights of score_grid sum to 1
    assert float(new["lognorm"].abs().max()) <= 1e-5
    for draws in (5, 21):
        a, _ = eng._grid_draws(call, draws, 7, 0)
        b, _ = eng._grid_draws_cond(call, tilt, draws, 7, 0)
        torch.cuda.synchronize()
        assert a.shape == (cs["N"], draws) and torch.equal(a, b), draws


# ---- 2. frozen (Gamma, Sigma) against the oracle ----------------------------------------------------------------------------
_FROZEN = {}


def _frozen_want(key):
    if key not in _FROZEN:
        theta, ll = pc.grid_ll(key)
        gamma, sigma = pc.frozen(key)
        _FROZEN[key] = pc.estep(ll, theta, pc.case(key)["X"], gamma, sigma)
    return _FROZEN[key]


@pytest.mark.parametrize("key", ["P1", "P2", "P3"])
def test_frozen_population_vs_oracle(key):
    want = _frozen_want(key)
    cs, eng, kw = _engine(key, pc.frozen(key))
    lo, need = sc.irt_condition(cs, want)
    assert lo >= need, (cs["name"], "oracle PSD below half the node spacing", lo, need)
    cov_t = torch.from_numpy(cs["cov"])
    got = eng.score(covariates=cov_t, **kw)
    call, tilt, _ = eng._population_call(None, None, cs["nodes"], cs["span"], cov_t)
    raw = eng._grid_posterior_cond(call, tilt)
    total = eng.marginal_loglik(covariates=cov_t, **kw)
    torch.cuda.synchronize()
    N, D = cs["N"], cs["D"]
    assert got["eap"].shape == (N, D) and got["psd"].shape == (N, D) and got["cov"].shape == (N, D, D)
    assert got["loglik"].shape == (N,) and got["node"].shape == (N,) and got["prior_mean"].shape == (N, D)
    _hold_rows(cs["name"], [("loglik", _np(got["loglik"]), want["loglik"]), ("eap", _np(got["eap"]), want["mean"]),
                            ("psd", _np(got["psd"]), want["sd"]), ("cov", _np(got["cov"]), want["cov"]),
                            ("lognorm", _np(raw["lognorm"]), want["lognorm"]), ("logjoint", _np(raw["logjoint"]), want["logjoint"]),
                            ("prior_mean", _np(got["prior_mean"]), want["prior_mean"])])
    _hold_nodes(cs["name"], _np(got["node"]), want)
    assert torch.equal(got["cov"], got["cov"].transpose(1, 2))
    assert torch.equal(got["loglik"], raw["logjoint"] - raw["lognorm"]) and torch.equal(got["eap"], raw["mean"])
    assert total == pytest.approx(float(want["loglik"].sum()), rel=2 * ROW_TOL)


def test_a_waves_second_unit_starts_clean():
    """P4: the tail rows behind 2 * CUs * 256 head rows whose tilt is +2 give the bits they give alone, and hold to the oracle of
    the tail alone: neither the missing count nor the tilt of a wave's first unit reaches its second."""
    cs, want = pc.second_unit(torch.cuda.get_device_properties(_dev()).multi_processor_count)
    eng = _irt_engine(cs)
    call = eng._grid_call(None, None, cs["nodes"], cs["span"])
    call = call._replace(logw=torch.from_numpy(want["lw"].astype(np.float32)).to(_dev()))
    tilt = torch.from_numpy(want["tilt"]).to(_dev())
    tail = torch.from_numpy(cs["tail"]).to(_dev())
    full = eng._grid_posterior_cond(call, tilt)
    alone_call = eng._grid_call(torch.from_numpy(cs["y_tail"]), None, cs["nodes"], cs["span"])._replace(logw=call.logw)
    alone = eng._grid_posterior_cond(alone_call, tilt[tail].contiguous())
    d_full = eng._grid_draws_cond(call, tilt, 5, pc.PV_SEED, 0)[0]
    d_rows = eng._grid_draws_cond(call._replace(rows=tail), tilt[tail].contiguous(), 5, pc.PV_SEED, 0)[0]
    torch.cuda.synchronize()
    for k in ("logjoint", "lognorm", "mean", "cov", "node"):
        assert torch.equal(full[k][tail], alone[k]), k
    assert torch.equal(d_full[tail], d_rows)
    _hold_rows(cs["name"], [("loglik", _np(alone["logjoint"] - alone["lognorm"]), want["loglik"]), ("eap", _np(alone["mean"]), want["mean"]),
                            ("cov", _np(alone["cov"]), want["cov"][:, 0, :]), ("lognorm", _np(alone["lognorm"]), want["lognorm"])])
    _hold_nodes(cs["name"], _np(alone["node"]), want)
    node, gap = pc.oracle_draws(want["f"], cs["tail"], 5, pc.PV_SEED)
    _hold_draws(cs["name"], _np(d_rows), node, gap)


def test_frozen_population_under_a_second_schedule():
    """P2 and the zero-tilt comparisons again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
           "(test_frozen_population_vs_oracle and P2) or test_zero_tilt", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail


# ---- 3. rows ----------------------------------------------------------------------------------------------------------------
def test_rows_pick_the_full_calls_rows():
    """The tilt goes by batch position and the noise key by row: an unsorted index with repeats tells the two apart."""
    cs, eng, kw = _engine("P2", pc.frozen("P2"))
    assert len(np.unique(IDX)) < len(IDX) and (np.diff(IDX) < 0).any() and len(IDX) % 32 != 0
    cov_t, idx = torch.from_numpy(cs["cov"]), torch.from_numpy(IDX).to(_dev())
    one, two = eng.score(covariates=cov_t, **kw), eng.score(covariates=cov_t, **kw)
    sub = eng.score(rows=idx, covariates=cov_t, **kw)
    pv_full = eng.plausible_values(draws=pc.PV_DRAWS, seed=pc.PV_SEED, covariates=cov_t, **kw)
    pv_sub = eng.plausible_values(rows=idx, draws=pc.PV_DRAWS, seed=pc.PV_SEED, covariates=cov_t, **kw)
    torch.cuda.synchronize()
    for k in ("eap", "psd", "loglik", "node", "cov", "prior_mean"):
        assert torch.equal(one[k], two[k]), k
        assert torch.equal(sub[k], one[k][idx]), k
    for k in ("theta", "node"):
        assert torch.equal(pv_sub[k], pv_full[k][idx]), k
    # the covariates matter: other people's covariates give other scores
    other = eng.score(covariates=torch.from_numpy(cs["cov"][::-1].copy()), **kw)
    assert not torch.equal(other["eap"], one["eap"])


# ---- 4. conditioned draws against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["P1", "P2"])
def test_conditioned_draws_vs_oracle(key):
    want = _frozen_want(key)
    cs, eng, kw = _engine(key, pc.frozen(key))
    got = eng.plausible_values(draws=pc.PV_DRAWS, seed=pc.PV_SEED, covariates=torch.from_numpy(cs["cov"]), **kw)
    torch.cuda.synchronize()
    node, gap = pc.oracle_draws(want["f"], np.arange(cs["N"]), pc.PV_DRAWS, pc.PV_SEED)
    assert got["node"].shape == (cs["N"], pc.PV_DRAWS) and got["theta"].shape == (cs["N"], pc.PV_DRAWS, cs["D"])
    _hold_draws(cs["name"], _np(got["node"]), node, gap)
    theta, _ = pc.grid_ll(key)
    assert np.array_equal(_np(got["theta"]), theta[_np(got["node"])])


# ---- 5. EM against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["P1", "P2"])
@pytest.mark.parametrize("iters", [1, 6])
def test_fit_population_vs_oracle(key, iters):
    cs, eng, kw = _engine(key)
    want, tol = pc.em_oracle(key, iters), pc.em_tolerance(key, iters)
    got = eng.fit_population(torch.from_numpy(cs["cov"]), max_iter=iters, **kw)
    p, D = cs["X"].shape[1], cs["D"]
    assert got["gamma"].shape == (p, D) and got["gamma"].dtype == np.float64 and got["sigma"].shape == (D, D)
    assert got["iterations"] == want["iterations"] == iters and got["converged"] is False and len(got["loglik"]) == iters
    assert eng.population["gamma"] is got["gamma"] and eng.population["intercept"] is True
    err = {"gamma": float(np.abs(got["gamma"] - want["gamma"]).max()), "sigma": float(np.abs(got["sigma"] - want["sigma"]).max()),
           "loglik": float(np.max(np.abs(np.array(got["loglik"]) - np.array(want["loglik"])) / np.abs(np.array(want["loglik"]))))}
    print("%s, max_iter %d: %s" % (cs["name"], iters, "  ".join("%s %.2e (allowed %.2e)" % (k, err[k], 2 * tol[k]) for k in err)))
    for k in err:
        assert err[k] <= 2 * tol[k], (key, iters, k, err[k], 2 * tol[k])
    # loglik[0] is the log-likelihood under Gamma = 0, Sigma = I: what marginal_loglik() gives without covariates
    assert got["loglik"][0] == pytest.approx(eng.marginal_loglik(**kw), rel=2 * ROW_TOL)


# ---- 6. recovery ------------------------------------------------------------------------------------------------------------
def test_conditioned_draws_recover_the_regression_and_unconditioned_ones_do_not():
    cs, eng, kw = _engine("P5")
    cov_t = torch.from_numpy(cs["cov"])
    fit = eng.fit_population(cov_t, max_iter=50, **kw)
    cond = eng.plausible_values(draws=16, seed=pc.PV_SEED, covariates=cov_t, **kw)
    unc = eng.plausible_values(draws=16, seed=pc.PV_SEED, **kw)
    post = eng.score(covariates=cov_t, **kw)
    torch.cuda.synchronize()
    z, short = pc.recovery_holds(cs["X"], fit["gamma"], _np(cond["theta"]).astype(np.float64)[:, :, 0].mean(1),
                                 _np(unc["theta"]).astype(np.float64)[:, :, 0].mean(1), _np(post["psd"]).astype(np.float64)[:, 0] ** 2)
    print("P5: %d iterations (converged %s), gamma %s, sigma %.4f; conditioned coefficients at %s standard errors of gamma; the "
          "unconditioned dummy slope falls short by %.1f" % (fit["iterations"], fit["converged"], fit["gamma"][:, 0],
                                                            fit["sigma"][0, 0], np.round(z, 2), short))
    assert fit["converged"] and (np.diff(fit["loglik"]) >= -2 * ROW_TOL * np.abs(fit["loglik"][:-1])).all()
    assert (z <= 5.0).all(), z
    assert short > 5.0, short


# ---- 7. nothing else moves --------------------------------------------------------------------------------------------------
def test_fit_population_changes_nothing_else():
    from vipsy_amd import vi
    cs = pc.case("P1")
    data = cs["y"].astype(np.float32)
    data[cs["y"] == 255] = np.nan
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(data).to(_dev()), model="irt_2pl", x_feature=1, seed=7)
    m.fit(optim=vi.Adam({"lr": 1e-2}), max_iter=4, progress=False)
    eng = m.engine
    state = lambda: [t.clone() for t in (eng.P, eng.PP, eng.M, eng.V, eng.MP, eng.VP)]      # noqa: E731
    before, t_before, s_before = state(), eng.t, m.score(nodes=cs["nodes"])
    assert eng.population is None
    fit = m.fit_population(cs["cov"], max_iter=3, nodes=cs["nodes"])
    after, s_after = state(), m.score(nodes=cs["nodes"])
    torch.cuda.synchronize()
    assert fit["iterations"] == 3 and eng.population is not None and eng.t == t_before
    for u, v in zip(before, after):
        assert torch.equal(u, v)
    for k in s_before:
        assert torch.equal(s_before[k], s_after[k]), k
    assert set(s_after) == {"eap", "psd", "loglik", "node"}
    cond = m.score(covariates=cs["cov"], nodes=cs["nodes"])
    assert set(cond) == {"eap", "psd", "loglik", "node", "cov", "prior_mean"}
    # a refused fit leaves the stored population alone
    kept = eng.population
    with pytest.raises(ValueError):
        m.fit_population(cs["cov"], nodes=cs["nodes"], span=3.0)
    assert eng.population is kept


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vipsy_amd import vi
    cs, eng, kw = _engine("P1")
    cov = cs["cov"]
    with pytest.raises(ValueError, match="fit_population"):
        eng.score(covariates=cov, **kw)                                          # no population yet
    with pytest.raises(ValueError, match="column 3"):                            # a constant column beside the intercept
        eng.fit_population(np.concatenate([cov, np.full((cs["N"], 1), 2.0)], 1), **kw)
    with pytest.raises(ValueError, match="node spacing"):                        # 5 nodes: half the spacing is 1.5 > sqrt(Sigma) = 1
        eng.fit_population(cov, nodes=5, span=6.0)
    with pytest.raises(ValueError, match="raise span"):                          # 4 sqrt(1) > 3
        eng.fit_population(cov, nodes=cs["nodes"], span=3.0)
    with pytest.raises(ValueError, match="persons"):
        eng.fit_population(cov, rows=np.array([0, 1, 2, 3]), **kw)               # p + D + 1 = 5
    with pytest.raises(ValueError):
        eng.fit_population(cov[:50], **kw)
    with pytest.raises(ValueError, match="finite"):
        eng.fit_population(np.where(np.arange(cs["N"])[:, None] == 4, np.nan, cov), **kw)
    with pytest.raises(ValueError):
        eng.fit_population(cov, max_iter=0, **kw)
    assert eng.population is None
    eng.fit_population(cov, max_iter=2, **kw)
    with pytest.raises(ValueError, match="design columns"):
        eng.score(covariates=cov[:, :1], **kw)                                   # the wrong p
    with pytest.raises(ValueError, match="design columns"):
        eng.plausible_values(covariates=np.concatenate([cov, cov], 1), **kw)
    with pytest.raises(ValueError):
        eng.score(covariates=cov[:50], **kw)
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    x = rng.normal(size=(64, 2))
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)), vi.VCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCCDM(data=yd, q=torch.from_numpy(q))):
        with pytest.raises(NotImplementedError) as e:
            m.fit_population(x)
        assert type(m.engine).__name__ in str(e.value)
    m = vi.VIRT(data=yd, model="irt_2pl", x_feature=4)                           # D > 3: the wording of score()
    with pytest.raises(NotImplementedError) as want:
        m.engine.score()
    for call in (m.fit_population, m.engine.fit_population):
        with pytest.raises(NotImplementedError) as e:
            call(x)
        assert str(e.value) == str(want.value) and "x_feature" in str(e.value)
    assert m.engine.population is None


def test_a_sigma_that_collapses_during_the_fit_is_refused_and_the_stored_population_stays():
    """pop_cases.collapse_case: D = 3 on a test that barely measures its dimensions.  The M-step of iteration k0 is the first whose
    Sigma falls below (half the node spacing)^2: a fit of k0 iterations returns, a longer one is refused part-way through --
    the in-loop check on the M-step's Sigma -- and leaves the population of the earlier fit where it was."""
    cs, k0 = pc.collapse_case()
    eng = _irt_engine(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    cov_t = torch.from_numpy(cs["cov"])
    short = eng.fit_population(cov_t, max_iter=k0, **kw)
    assert short["iterations"] == k0 and not short["converged"]
    print("%s: after %d iterations min diag(Sigma) = %.4f (oracle %.4f, limit %.4f)"
          % (cs["name"], k0, np.diag(short["sigma"]).min(), cs["diags"][k0 - 1], cs["limit"]))
    assert abs(np.diag(short["sigma"]).min() - cs["diags"][k0 - 1]) < 1e-3
    kept = eng.population
    assert kept["sigma"] is short["sigma"]
    with pytest.raises(ValueError, match="node spacing"):
        eng.fit_population(cov_t, **kw)
    with pytest.raises(ValueError, match="node spacing"):
        eng.fit_population(cov_t, max_iter=k0 + 1, **kw)                          # the check on what would be returned
    assert eng.population is kept


def test_the_binding_refuses_bad_dimensions_and_null_pointers():
    from vipsy_amd import _hip
    L = _hip.lib()
    dev = _dev()
    y = torch.zeros(4, 8, dtype=torch.uint8, device=dev)
    img = torch.zeros(int(L.vx_grid_image_bytes(8, 5)), dtype=torch.uint8, device=dev)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)                                   # noqa: E731
    logw, coord, tilt, lj, ln, mean, cov = f(5), f(5, 3), f(4, 3), f(4), f(4), f(4, 3), f(4, 6)
    node = torch.zeros(4, 8, dtype=torch.int32, device=dev)
    P = _hip.ptr

    def post(D, **null):
        a = dict(y=y, img=img, logw=logw, coord=coord, tilt=tilt, lj=lj, ln=ln, mean=mean, cov=cov, node=node)
        a.update(null)
        return L.vx_grid_posterior_cond(P(a["y"]), None, 4, 8, 5, D, P(a["img"]), P(a["logw"]), P(a["coord"]), P(a["tilt"]), P(a["lj"]),
                                        P(a["ln"]), P(a["mean"]), P(a["cov"]), P(a["node"]), None)

    def draw(D, **null):
        a = dict(y=y, img=img, logw=logw, coord=coord, tilt=tilt, node=node)
        a.update(null)
        return L.vx_grid_draw_cond(P(a["y"]), None, 4, 8, 5, D, P(a["img"]), P(a["logw"]), P(a["coord"]), P(a["tilt"]),
                                   ctypes.c_uint64(1), 0, 0, 8, 8, P(a["node"]), None)

    for D in (0, 4, -1):
        assert post(D) == -1 and draw(D) == -1, D
    for k in ("y", "img", "logw", "coord", "tilt", "lj", "ln", "mean", "cov", "node"):
        assert post(1, **{k: None}) == -1, k
    for k in ("y", "img", "logw", "coord", "tilt", "node"):
        assert draw(1, **{k: None}) == -1, k
