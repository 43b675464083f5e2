"""The float64 oracle and the cases of the latent-regression tests (tests/test_pop_host.py on the CPU, tests/test_gpu_pop.py on the
GPU): IrtEngine.fit_population and the conditioned score() / plausible_values() behind vx_grid_posterior_cond / vx_grid_draw_cond.

The oracle is a few lines over tests/score_cases.py (irt_grid_loglik: ll[i][g]) and tests/pv_cases.py (the Philox words, the Gumbel
noise, draw): the E-step under a prior of each person's own, theta_i ~ N(Gamma^T x_i, Sigma), which on the grid is the shared
log-weight lw[g] = -1/2 theta_g^T Lambda theta_g (max-shifted, as grid.population_logw shifts it) plus the tilt (Lambda Gamma^T x_i)
. theta_g; lognorm, mean, the full covariance, the MAP node and the gap of the best two; the M-step
    Gamma' = (X^T X)^-1 X^T m,      Sigma' = (1 / n) sum_i [C_i + (m_i - Gamma'^T x_i)(m_i - Gamma'^T x_i)^T];
and the loop from Gamma = 0, Sigma = I that stops when |dL| <= tol |L_prev|.

Item parameters, covariates and responses are DRAWN (seeded), not trained; the latent of a simulated person is Gamma_true^T x_i +
N(0, 0.8^2 I), so that the population stays well inside the grid.  Everything here is computed once and shared; callers must not
modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import pv_cases as pv
from tests import score_cases as sc
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

DRAW_GAP = 1e-4              # a draw must equal the oracle's where its best two perturbed values differ by more
PV_DRAWS, PV_SEED = 8, 11    # the conditioned draws against the oracle
RESID_SD = 0.8

# name, N, J, D, nodes per dimension, missing rate, slope range or the score case whose parameters it takes, p (with intercept), seed
CASES = {
    "P1": ("p1_d1_n97_j17", 97, 17, 1, 41, 0.30, (0.5, 1.5), 3, 41),
    "P2": ("p2_d2_441", 100, 40, 2, 21, 0.0, "case5_2pl_d2_441", 3, 42),
    "P3": ("p3_d3_729", 100, 40, 3, 9, 0.0, "case5_2pl_d3_729", 3, 43),
    "P5": ("p5_recovery_n2048", 2048, 30, 1, 61, 0.20, (0.5, 1.5), 3, 45),
}
TRUE_GAMMA_1D = np.array([0.0, 0.5, 0.3])                    # intercept, the 0/1 dummy (the slope test 6 recovers), the normal column


def covariates(N, rng):
    """[N][2]: one 0/1 column, one standard normal column (the design adds the intercept)."""
    return np.stack([(rng.uniform(size=N) < 0.5).astype(np.float64), rng.normal(size=N)], axis=1)


def design(cov, intercept=True):
    cov = np.asarray(cov, np.float64)
    return np.concatenate([np.ones((len(cov), 1)), cov], 1) if intercept else cov


_CASE = {}


def case(key):
    """The drawn case: name, N, J, model, D, Dc, nodes, span, params (float32 leaves), cov [N][p - 1], X [N][p], y u8 [N][J]."""
    if key not in _CASE:
        name, N, J, D, nodes, missing, slopes, p, seed = CASES[key]
        rng = np.random.RandomState(seed)
        if isinstance(slopes, str):
            base = sc.irt_case([c for c in sc.IRT_CASES if c[0] == slopes][0])
            assert (base["J"], base["D"], base["nodes"]) == (J, D, nodes)
            params = base["params"]
        else:
            params = {"a": rng.uniform(slopes[0], slopes[1], size=(D, J)).astype(np.float32),
                      "b": rng.normal(0.0, 1.0, size=(1, J)).astype(np.float32)}
        cov = covariates(N, rng)
        X = design(cov)
        g_true = np.zeros((p, D))
        g_true[:, 0] = TRUE_GAMMA_1D
        for d in range(1, D):
            g_true[:, d] = rng.uniform(-0.4, 0.4, size=p)
        x = X @ g_true + RESID_SD * rng.normal(size=(N, D))
        z = x @ params["a"].astype(np.float64) + params["b"].astype(np.float64)
        y = (rng.uniform(size=(N, J)) < vo.sigmoid(z)).astype(np.uint8)
        if missing > 0:
            y[rng.uniform(size=(N, J)) < missing] = 255
        _CASE[key] = {"name": name, "N": N, "J": J, "model": "irt_2pl", "D": D, "Dc": 1.0, "nodes": nodes, "span": sc.SPAN,
                      "params": params, "cov": cov, "X": X, "y": y, "gamma_true": g_true}
    return _CASE[key]


def frozen(key):
    """(Gamma [p][D] with entries up to 0.6, Sigma [D][D], non-diagonal for D > 1) of the comparisons at fixed parameters.  Sigma
    = L L^T with a diagonal of L in [0.95, 1.1]: a population as wide as N(0, I), so that the oracle's PSD stays above half the
    node spacing on the coarse grid of P3 (9 nodes a dimension) too -- test_pop_host.py checks it."""
    cs = case(key)
    rng = np.random.RandomState(1000 + CASES[key][8])
    p, D = cs["X"].shape[1], cs["D"]
    gamma = rng.uniform(-0.6, 0.6, size=(p, D))
    L = np.diag(rng.uniform(0.95, 1.1, size=D)) + np.tril(rng.uniform(-0.3, 0.3, size=(D, D)), -1)
    return gamma, L @ L.T


_LL = {}


def grid_ll(key):
    """(theta float32 [G][D], ll float64 [N][G]) of a case."""
    if key not in _LL:
        from vipsy_amd.grid import score_grid
        cs = case(key)
        theta, _ = score_grid(cs["D"], cs["nodes"], cs["span"])
        _LL[key] = (theta, sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y"]))
    return _LL[key]


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def _lse(f):
    m = f.max(1)
    return m + np.log(np.exp(f - m[:, None]).sum(1))


def population_prior(theta, X, gamma, sigma):
    """(lw [G] = -1/2 theta^T Lambda theta, max-shifted; tilt [n][D] = X Gamma Lambda; mu [n][D]) in float64."""
    theta = np.asarray(theta, np.float64)
    lam = np.linalg.inv(np.asarray(sigma, np.float64))
    lw = -0.5 * np.einsum("gd,de,ge->g", theta, lam, theta)
    mu = np.asarray(X, np.float64) @ np.asarray(gamma, np.float64)
    return lw - lw.max(), mu @ lam, mu


def estep_tilt(ll, theta, lw, tilt):
    """The E-step under log prior lw[g] + tilt_i . theta_g (unnormalised): f = ll + that, loglik = lse f - lse h."""
    theta = np.asarray(theta, np.float64)
    h = np.asarray(lw, np.float64)[None, :] + np.asarray(tilt, np.float64) @ theta.T
    f = ll + h
    logjoint, lognorm = _lse(f), _lse(h)
    p = np.exp(f - logjoint[:, None])
    mean = p @ theta
    dev = theta[None, :, :] - mean[:, None, :]
    cov = np.einsum("ng,ngd,nge->nde", p, dev, dev)
    top = np.sort(f, axis=1)
    gap = top[:, -1] - top[:, -2] if f.shape[1] > 1 else np.full(len(f), np.inf)
    sd = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    return {"f": f, "logjoint": logjoint, "lognorm": lognorm, "loglik": logjoint - lognorm, "mean": mean, "cov": cov, "sd": sd,
            "node": f.argmax(1), "gap": gap}


def estep(ll, theta, X, gamma, sigma):
    lw, tilt, mu = population_prior(theta, X, gamma, sigma)
    out = estep_tilt(ll, theta, lw, tilt)
    out["prior_mean"] = mu
    return out


SECOND_SIGMA = np.array([[0.8]])
_SECOND = {}


def second_unit(cus):
    """P4: sc.second_unit_case(cus) -- two waves of a launch take a second unit -- under Sigma = 0.8, with tilt +2 for every head
    row (the waves' first units) and a drawn tilt of their own for the 97 tail rows.  What a unit leaves behind, the tilt
    included, must not reach the next: the oracle is that of the tail alone.  Returns (case, oracle), the oracle with `tilt`
    float32 [N][1] of the whole batch and `lw` float64 [G]."""
    if cus not in _SECOND:
        from vipsy_amd.grid import score_grid
        cs, _ = sc.second_unit_case(cus)
        theta, _ = score_grid(cs["D"], cs["nodes"], cs["span"])
        ll = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y_tail"])
        tilt = np.full((cs["N"], 1), 2.0, dtype=np.float32)
        tilt[cs["tail"]] = np.random.RandomState(19).uniform(-0.75, 0.75, size=(len(cs["tail"]), 1)).astype(np.float32)
        lw = population_prior(theta, np.zeros((1, 1)), np.zeros((1, 1)), SECOND_SIGMA)[0]
        want = estep_tilt(ll, theta, lw, tilt[cs["tail"]].astype(np.float64))
        want.update(tilt=tilt, lw=lw, theta=theta)
        _SECOND[cus] = (cs, want)
    return _SECOND[cus]


_COLLAPSE = {}


def collapse_case():
    """The case in which Sigma collapses DURING the fit (the Sigma refusal's case): 300 persons, 30 items, D = 3 with slopes 0.2 ..
    0.5, 9 nodes a dimension -- the test barely measures its dimensions, and EM shrinks Sigma_22 iteration by iteration until it
    falls below (half the node spacing)^2 = 0.5625.  Returns (case, k0): the M-step of iteration k0 (counted from 0) is the first
    whose Sigma is refused, so a fit of k0 iterations returns and a longer one raises."""
    if not _COLLAPSE:
        from vipsy_amd.grid import score_grid
        rng = np.random.RandomState(47)
        N, J, D, nodes = 300, 30, 3, 9
        a = (rng.uniform(0.2, 0.5, size=(D, J)) * vo.default_a_free(D, J)).astype(np.float32)
        b = rng.normal(size=(1, J)).astype(np.float32)
        cov = covariates(N, rng)
        x = rng.normal(size=(N, D))
        y = (rng.uniform(size=(N, J)) < vo.sigmoid(x @ a.astype(np.float64) + b)).astype(np.uint8)
        cs = {"name": "p6_collapse_d3", "N": N, "J": J, "model": "irt_2pl", "D": D, "Dc": 1.0, "nodes": nodes, "span": sc.SPAN,
              "params": {"a": a, "b": b}, "cov": cov, "X": design(cov), "y": y}
        theta, _ = score_grid(D, nodes, sc.SPAN)
        ll = sc.irt_grid_loglik("irt_2pl", theta, cs["params"], 1.0, y)
        lim = (0.5 * 2.0 * sc.SPAN / (nodes - 1)) ** 2
        gamma, sigma, diags = np.zeros((cs["X"].shape[1], D)), np.eye(D), []
        for k in range(60):
            e = estep(ll, theta, cs["X"], gamma, sigma)
            gamma, sigma = mstep(cs["X"], e["mean"], e["cov"])
            diags.append(np.diag(sigma).min())
            if diags[-1] < lim:
                break
        cs["diags"], cs["limit"] = np.array(diags), lim
        _COLLAPSE["c"] = (cs, len(diags) - 1)
    return _COLLAPSE["c"]


def mstep(X, mean, cov):
    X = np.asarray(X, np.float64)
    gamma = np.linalg.solve(X.T @ X, X.T @ mean)
    r = mean - X @ gamma
    return gamma, (cov.sum(0) + r.T @ r) / len(X)


def _perturb(v, sign, tol):
    """Every row of v moved by sign * tol * max(|row|_inf, 1): the largest error the row rule lets through."""
    flat = v.reshape(len(v), -1)
    return v + sign.reshape(v.shape) * (tol * np.maximum(np.abs(flat).max(1), 1.0)).reshape((-1,) + (1,) * (v.ndim - 1))


def em(ll, theta, X, max_iter, tol=1e-7, signs=None, row_tol=ROW_TOL):
    """The loop of fit_population.  signs: None, or a function (iteration, name, shape) -> an array of +-1 by which loglik, mean
    and cov of that iteration's E-step are perturbed (the tolerance measurement of the EM comparison)."""
    p, D = X.shape[1], theta.shape[1]
    gamma, sigma = np.zeros((p, D)), np.eye(D)
    hist, converged = [], False
    for k in range(max_iter):
        e = estep(ll, theta, X, gamma, sigma)
        loglik, mean, cov = e["loglik"], e["mean"], e["cov"]
        if signs is not None:
            loglik = _perturb(loglik, signs(k, "loglik", loglik.shape), row_tol)
            mean = _perturb(mean, signs(k, "mean", mean.shape), row_tol)
            s = np.triu(signs(k, "cov", cov.shape))                        # (a symmetric perturbation: the kernel gives a triangle)
            cov = _perturb(cov, s + np.transpose(np.triu(s, 1), (0, 2, 1)), row_tol)
        hist.append(float(loglik.sum()))
        gamma, sigma = mstep(X, mean, cov)
        if len(hist) > 1 and abs(hist[-1] - hist[-2]) <= tol * abs(hist[-2]):
            converged = True
            break
    return {"gamma": gamma, "sigma": sigma, "loglik": hist, "iterations": len(hist), "converged": converged}


_EM = {}


def em_oracle(key, max_iter):
    if (key, max_iter) not in _EM:
        theta, ll = grid_ll(key)
        _EM[(key, max_iter)] = em(ll, theta, case(key)["X"], max_iter)
    return _EM[(key, max_iter)]


_TOL = {}


def em_tolerance(key, max_iter):
    """What an E-step that meets the row rule can move: the largest deviation of Gamma, Sigma (absolute) and of the log-likelihood
    history (relative to its size) from the clean oracle, over 16 sign patterns of the perturbation -- all +, all -, 14 seeded
    random ones.  The GPU comparison allows twice these (second-order terms)."""
    if (key, max_iter) not in _TOL:
        theta, ll = grid_ll(key)
        X = case(key)["X"]
        clean = em_oracle(key, max_iter)
        dev = {"gamma": 0.0, "sigma": 0.0, "loglik": 0.0}
        for pat in range(16):
            if pat < 2:
                signs = lambda k, name, shape, s=(1.0 if pat == 0 else -1.0): np.full(shape, s)       # noqa: E731
            else:
                def signs(k, name, shape, pat=pat):
                    rng = np.random.RandomState(7000 + 97 * pat + 13 * k + {"loglik": 0, "mean": 1, "cov": 2}[name])
                    return np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)
            got = em(ll, theta, X, max_iter, tol=0.0, signs=signs)
            n = min(len(got["loglik"]), len(clean["loglik"]))
            dev["gamma"] = max(dev["gamma"], float(np.abs(got["gamma"] - clean["gamma"]).max()))
            dev["sigma"] = max(dev["sigma"], float(np.abs(got["sigma"] - clean["sigma"]).max()))
            dev["loglik"] = max(dev["loglik"], float(np.max(np.abs(np.array(got["loglik"][:n]) - np.array(clean["loglik"][:n]))
                                                            / np.abs(np.array(clean["loglik"][:n])))))
        _TOL[(key, max_iter)] = dev
    return _TOL[(key, max_iter)]


# ---- draws ----------------------------------------------------------------------------------------------------------------
def oracle_draws(f, rows, draws, seed):
    """(node [n][draws], gap) of the posteriors f [n][G] for the persons with noise keys `rows`."""
    return pv.draw(f, pv.gumbel(seed, np.asarray(rows, np.int64), f.shape[1], draws))


def ols(X, v):
    X = np.asarray(X, np.float64)
    return np.linalg.solve(X.T @ X, X.T @ np.asarray(v, np.float64))


def recovery_se(X, post_var, draws):
    """The Monte-Carlo standard error of the OLS coefficients of the mean of `draws` draws a person: sqrt(diag((X^T X)^-1) *
    mean posterior variance / draws)."""
    X = np.asarray(X, np.float64)
    return np.sqrt(np.diag(np.linalg.inv(X.T @ X)) * float(np.mean(post_var)) / draws)


def recovery_holds(X, gamma, cond_mean_theta, unc_mean_theta, post_var, draws=16, dummy=1):
    """Test 6, both halves, on the per-person means of the draws: (z of the conditioned coefficients against gamma, the shortfall
    of the unconditioned dummy slope in standard errors)."""
    se = recovery_se(X, post_var, draws)
    z = np.abs(ols(X, cond_mean_theta) - np.asarray(gamma)[:, 0]) / se
    short = (np.asarray(gamma)[dummy, 0] - ols(X, unc_mean_theta)[dummy]) / se[dummy]
    return z, float(short)
