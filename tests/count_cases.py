"""The float64 oracle and the cases of the expected-count tests (tests/test_counts_host.py on the CPU, tests/test_gpu_counts.py
on the GPU).  A few lines over tests/score_cases.py: its irt_grid_loglik / cdm_grid_loglik, a max-shifted softmax over the
nodes and two indicator matmuls,

    n1[j][g] = sum_i p_i(g) [y_ij == 1]      n0[j][g] = sum_i p_i(g) [y_ij == 0]      mass[g] = sum_i p_i(g).

prob[j][g] = P(y_j = 1 | node g) comes from single-item response rows through the same functions, and the item-fit statistics
follow their definition: with n = n1 + n0, N_j = sum_g n[j][g] and every sum over the nodes with n[j][g] > 0,

    n_obs = N_j     md = sum (n1 - n prob) / N_j     rmsd = sqrt(sum (n1 - n prob)^2 / n / N_j)     observed = n1 / n.

Cases: every case of score_cases (ragged J and G, 32 item chunks, 14 / 23 / 32 node tiles, a person without a response, 90 %
missing, K = 10), COUNT_BIG (2 500 persons: several units a workgroup, several slabs, a ragged last unit), its misfit
variant, in which the observed cells of item 3 are seeded coin flips, and COUNT_WIDE (530 items: the kernel's form for more
than 512)."""
import numpy as np

from tests import score_cases as sc

COUNT_BIG = ("counts_2pl_n2500", 2500, 37, "irt_2pl", 1, 1.0, 61, 0.30, (0.5, 1.5), 31)
# beyond 512 items a wave holds four item tiles and a workgroup one node tile: the third form of the kernel (100 persons, sparse as case 4)
COUNT_WIDE = ("counts_2pl_j530", 100, 530, "irt_2pl", 1, 1.0, 41, 0.90, (0.3, 0.8), 41)
MISFIT_NAME = "counts_2pl_n2500_misfit"
MISFIT_ITEM = 3
IRT_CASES = list(sc.IRT_CASES) + [COUNT_BIG, COUNT_WIDE]
CDM_CASES = list(sc.CDM_CASES)


def big_case():
    return sc.irt_case(COUNT_BIG)


def misfit_case():
    """COUNT_BIG with the observed cells of item 3 replaced by coin flips: the item no longer follows its curve."""
    cs = dict(big_case())
    y = cs["y"].copy()
    rng = np.random.RandomState(99)
    obs = y[:, MISFIT_ITEM] != 255
    y[obs, MISFIT_ITEM] = (rng.uniform(size=int(obs.sum())) < 0.5)
    cs["y"], cs["name"] = y, MISFIT_NAME
    return cs


def _single_item_rows(J):
    """J rows that answer one item each correctly, and a last row that answers none."""
    Y = np.full((J + 1, J), 255, np.uint8)
    Y[np.arange(J), np.arange(J)] = 1
    return Y


def _prob_from(ll, J):
    # row j holds log P(y_j = 1 | g) and J - 1 cells of the missing constant, row J holds J of them
    return np.exp(ll[:J] - ll[J:J + 1] * ((J - 1.0) / J))


def fit_stats(n1, n0, prob):
    n = n1 + n0
    pos = n > 0
    safe = np.where(pos, n, 1.0)
    n_obs = np.where(pos, n, 0.0).sum(1)
    resid = np.where(pos, n1 - n * prob, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        md = resid.sum(1) / n_obs
        rmsd = np.sqrt((resid ** 2 / safe).sum(1) / n_obs)
        observed = np.where(pos, n1 / safe, np.nan)
    return {"n_obs": n_obs, "md": md, "rmsd": rmsd, "observed": observed}


def counts(ll, logw, y):
    """The tables from ll [n][G], logw [G] and the responses [n][J]; `p` [n][G] is the posterior they were summed from."""
    f = ll + np.asarray(logw, np.float64)[None, :]
    w = np.exp(f - f.max(1, keepdims=True))
    p = w / w.sum(1, keepdims=True)
    return {"n1": (y == 1).astype(np.float64).T @ p, "n0": (y == 0).astype(np.float64).T @ p, "mass": p.sum(0), "p": p}


def irt_oracle(cs, rows=None):
    """n1, n0, mass, prob, p and the fit statistics of an IRT case (cs as sc.irt_case makes it; rows: a subset of its persons)."""
    from vipsy_amd.engine import score_grid
    theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
    y = cs["y"] if rows is None else cs["y"][np.asarray(rows)]
    J = y.shape[1]
    out = counts(sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], y), logw, y)
    out["prob"] = _prob_from(sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], _single_item_rows(J)), J)
    out.update(fit_stats(out["n1"], out["n0"], out["prob"]))
    out["logw"] = logw.astype(np.float64)
    return out


def cdm_oracle(cs, rows=None):
    y = cs["y"] if rows is None else cs["y"][np.asarray(rows)]
    J = y.shape[1]
    ll, logw, attrs = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], y)
    out = counts(ll, logw, y)
    out["prob"] = _prob_from(sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], _single_item_rows(J))[0], J)
    out.update(fit_stats(out["n1"], out["n0"], out["prob"]))
    out["logw"], out["patterns"] = logw, attrs
    return out


def restated_f32(ll, logw, y, scale=16384.0):
    """The kernel's arithmetic said again in numpy: float32 ll and log-sum-exp, p = exp(f - loglik) in float32, p 2^14 as an
    fp16 head and an fp16 remainder, float32 sums over the persons in their order.  What is left against counts() is the
    error of the METHOD, whatever the code does."""
    f = (ll.astype(np.float32) + np.asarray(logw, np.float32)[None, :]).astype(np.float32)
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp(f - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    p = np.exp((f - lk).astype(np.float32)).astype(np.float32) * np.float32(scale)
    h = p.astype(np.float16)
    lo = (p - h.astype(np.float32)).astype(np.float16)
    p2 = h.astype(np.float32) + lo.astype(np.float32)
    n1 = np.zeros((y.shape[1], p.shape[1]), np.float32)
    n0 = n1.copy()
    mass = np.zeros(p.shape[1], np.float32)
    for i in range(y.shape[0]):
        n1 += np.outer((y[i] == 1).astype(np.float32), p2[i])
        n0 += np.outer((y[i] == 0).astype(np.float32), p2[i])
        mass += p2[i]
    s = np.float32(1.0 / scale)
    return {"n1": n1 * s, "n0": n0 * s, "mass": mass * s}
