"""The float64 oracle and the cases of the standard-error tests (tests/test_se_host.py on the CPU, tests/test_gpu_se.py on the GPU).
A few lines over tests/score_cases.py, tests/count_cases.py and tests/em_cases.py: with p the posterior of count_cases.counts,

    W1[g][(j,k)] = (1 - P_j(g)) u_jgk      W0[g][(j,k)] = P_j(g) u_jgk
    S[i][(j,k)]  = sum_g p_i(g) ( [y_ij == 1] W1[g][(j,k)] - [y_ij == 0] W0[g][(j,k)] )      info = S^T S      gradient = sum_i S[i]

P from vo.sigmoid at z clamped as em_cases._item_eval clamps it (a node where the clamp is active contributes nothing), u_g =
Dc (1, theta_g) for the IRT links; for DINA / DINO P = g or 1 - s by eta (vo.dina_eta / vo.dino_eta) and u = ([eta = 0],
-[eta = 1]) on the unconstrained scale.  Dense layout: column c = j K + k; K = D + 1 (b, a_0 ..) for 2PL, 1 for 1PL, 2 (g_un,
s_un) for the CDMs.  The standard errors are the square roots of the diagonal of the inverse of the kept block: the free
columns whose diagonal is not exactly zero.

restated_f32 says the kernels' arithmetic again in numpy: p 2^14, W 2^s and S 2^s as fp16 heads and fp16 remainders (the
low x low products left out), float32 sums, the persons in slabs of 256 added in their order.

SE cases: the parameters are those after a fixed number of ORACLE EM iterations from em_cases.start_of -- near the marginal
maximum, where the matrix means something -- never trained on the GPU.  They are recorded in tests/golden/se/se_params.npz
(python -m tests.se_cases writes it; two minutes of float64 numpy) and checked against the oracle by tests/test_se_host.py.  INFO cases: the drawn parameters of the score / count
cases; N < P there or the design is degenerate, the matrix is singular by design and only it and the gradient are compared."""
import os

import numpy as np

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import em_cases as ec
from tests import score_cases as sc

# (case, oracle EM iterations)
SE_CASES = [
    (cc.COUNT_BIG, 60),
    (ec.ONEPL, 40),
    (("se_2pl_d1_small", 400, 12, "irt_2pl", 1, 1.702, 41, 0.2, (0.5, 1.5), 41), 40),
    (("se_2pl_d2", 1500, 20, "irt_2pl", 2, 1.0, 21, 0.10, (0.6, 1.4), 37), 40),
    (("se_2pl_d3", 1500, 18, "irt_2pl", 3, 1.0, 9, 0.0, (0.6, 1.2), 39), 60),
    (("se_dina_k3", 1500, 20, "dina", 3, 0.10, 31), 30),
    (("se_dino_k4", 2000, 24, "dino", 4, 0.0, 33), 30),
]
SE_IDS = [c[0][0] for c in SE_CASES]
INFO_CASES = [c for c in sc.IRT_CASES if c[3] in ("irt_1pl", "irt_2pl")] + list(sc.CDM_CASES) + [cc.COUNT_WIDE]
INFO_IDS = [c[0] for c in INFO_CASES]
CONDITION_MAX = 1e3
SLAB = 256                       # GRID_SLAB (vipsy_amd/csrc/grid_plan.h)


def case_of(case):
    """The case and its kind; the CDM tuples have seven entries, the IRT ones ten."""
    if case == ec.ONEPL:
        return ec.onepl_case(), "irt"
    if len(case) == 7:
        return sc.cdm_case(case), "cdm"
    return sc.irt_case(case), "irt"


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se", "se_params.npz")
_PARAMS, _GOLDEN = {}, []


def compute_params(case, iters, also=()):
    """The float32 leaves after `iters` oracle EM iterations (em_cases.em_iteration) from the engine's start; also: earlier
    iteration counts whose leaves are wanted too -- then a dict {count: leaves}."""
    cs, kind = case_of(case)
    p = {k: v.astype(np.float64) for k, v in ec.start_of(cs, kind).items()}
    out = {}
    for it in range(1, iters + 1):
        p, _lk = ec.em_iteration(cs, kind, p)
        if it == iters or it in also:
            out[it] = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    return out if also else out[iters]


def golden_params(case, iters):
    """The recorded leaves of (case, iters), or None."""
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) else {})
    keys = [k for k in _GOLDEN[0] if k.startswith("%s/%d/" % (case[0], iters))]
    return {k.rsplit("/", 1)[1]: _GOLDEN[0][k] for k in keys} or None


def write_golden():
    out = {}
    for case, iters in SE_CASES:
        for it, leaves in compute_params(case, iters, also=(iters - 1,)).items():
            for k, v in leaves.items():
                out["%s/%d/%s" % (case[0], it, k)] = v
    np.savez_compressed(GOLDEN, **out)


def params_after(case, iters):
    """(cs, kind, float32 leaves after `iters` oracle EM iterations from the engine's start): the recorded ones
    (tests/golden/se/se_params.npz; tests/test_se_host.py checks them against the oracle), else computed; shared, never modified."""
    key = (case[0], iters)
    if key not in _PARAMS:
        cs, kind = case_of(case)
        _PARAMS[key] = (cs, kind, golden_params(case, iters) or compute_params(case, iters))
    return _PARAMS[key]


def layout(cs, kind):
    """K and the free mask over the dense layout."""
    J = cs["J"]
    if kind == "cdm":
        return 2, np.ones(2 * J, bool)
    if cs["model"] == "irt_1pl":
        return 1, np.ones(J, bool)
    free = np.ones((J, cs["D"] + 1), bool)
    free[:, 1:] = ec.a_free_of(cs).T
    return cs["D"] + 1, free.reshape(-1)


def tables(cs, kind, params):
    """(W1 [G][P], W0 [G][P], the bound on |W| the kernels scale by) in float64."""
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    J = cs["J"]
    if kind == "cdm":
        eta, _ = (vo.dino_eta if cs["cdm"] == "dino" else vo.dina_eta)(cs["K"], f8(cs["q"]))
        e1 = eta > 0                                                # [C][J]
        gu, su = f8(params["g"]).reshape(1, J), f8(params["s"]).reshape(1, J)
        g, s = vo.sigmoid(gu), vo.sigmoid(su)
        ok_g = (g <= 1 - vo.EPS32) & (vo.sigmoid(-gu) >= vo.EPS32)
        ok_s = (s <= 1 - vo.EPS32) & (vo.sigmoid(-su) >= vo.EPS32)
        C = e1.shape[0]
        W1, W0 = np.zeros((C, J, 2)), np.zeros((C, J, 2))
        W1[:, :, 0] = np.where(~e1 & ok_g, 1 - g, 0.0)              # eta = 0: P = g, u = 1
        W0[:, :, 0] = np.where(~e1 & ok_g, g, 0.0)
        W1[:, :, 1] = np.where(e1 & ok_s, -s, 0.0)                  # eta = 1: P = 1 - s, u = -1
        W0[:, :, 1] = np.where(e1 & ok_s, -(1 - s), 0.0)
        return W1.reshape(C, -1), W0.reshape(C, -1), 1.0
    theta, _ = ec.grid_of(cs)
    theta = f8(theta)
    G, D = theta.shape
    Dc = float(cs["Dc"])
    U = np.concatenate([np.ones((G, 1)), theta], axis=1)            # [G][D + 1]
    b = f8(params["b"]).reshape(1, J)
    if cs["model"] == "irt_1pl":
        z = Dc * (theta + b)
        U = U[:, :1]
    else:
        z = Dc * (theta @ f8(params["a"]).reshape(D, J) + b)
    zc = np.clip(z, -ec.ZL, ec.ZL)
    inside = zc == z
    om = np.where(inside, vo.sigmoid(-zc), 0.0)                     # 1 - P
    pr = np.where(inside, vo.sigmoid(zc), 0.0)                      # P
    W1 = (om[:, :, None] * (Dc * U)[:, None, :]).reshape(G, -1)
    W0 = (pr[:, :, None] * (Dc * U)[:, None, :]).reshape(G, -1)
    return W1, W0, abs(Dc) * max(1.0, float(np.abs(theta).max()))


def grid_loglik(cs, kind, params, y):
    """(ll [n][G], logw [G]) of the rows y."""
    if kind == "cdm":
        ll, logw, _ = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], params, y)
        return ll, np.asarray(logw, np.float64)
    theta, logw = ec.grid_of(cs)
    return sc.irt_grid_loglik(cs["model"], theta, params, cs["Dc"], y), np.asarray(logw, np.float64)


def scores(p, W1, W0, y, K):
    """S [n][P] from the posterior p [n][G], the tables and the responses."""
    y1 = np.repeat((y == 1), K, axis=1)
    y0 = np.repeat((y == 0), K, axis=1)
    return np.where(y1, p @ W1, 0.0) - np.where(y0, p @ W0, 0.0)


def kept_of(info, free):
    return np.flatnonzero(np.asarray(free, bool) & (np.diag(info) != 0))


def oracle(cs, kind, params, y=None):
    """info, gradient, n, K, free, kept, and -- where the kept block is positive definite -- cov, se [P] (NaN off the kept
    columns) and the block's 2-norm condition number; also p, the tables and S for the tests that need them."""
    y = cs["y"] if y is None else y
    K, free = layout(cs, kind)
    ll, logw = grid_loglik(cs, kind, params, y)
    t = cc.counts(ll, logw, y)
    W1, W0, bound = tables(cs, kind, params)
    S = scores(t["p"], W1, W0, y, K)
    info = S.T @ S
    out = {"info": info, "gradient": S.sum(0), "n": len(y), "K": K, "free": free, "kept": kept_of(info, free), "S": S, "p": t["p"],
           "W1": W1, "W0": W0, "bound": bound, "n1": t["n1"], "n0": t["n0"], "ll": ll, "logw": logw}
    A = info[np.ix_(out["kept"], out["kept"])]
    w = np.linalg.eigvalsh(A) if A.size else np.zeros(0)
    if A.size and w[0] > 0:
        cov = np.linalg.inv(A)
        se = np.full(len(free), np.nan)
        se[out["kept"]] = np.sqrt(np.diag(cov))
        out.update(cov=cov, se=se, condition=float(w[-1] / w[0]))
    return out


_SE = {}


def se_oracle(entry):
    """(cs, kind, params, oracle) of an SE_CASES entry, computed once and shared (never modified)."""
    case, iters = entry
    if case[0] not in _SE:
        cs, kind, params = params_after(case, iters)
        _SE[case[0]] = (cs, kind, params, oracle(cs, kind, params))
    return _SE[case[0]]


_INFO = {}


def info_oracle(case):
    """(cs, kind, oracle) of an INFO_CASES entry at its drawn parameters."""
    if case[0] not in _INFO:
        cs, kind = case_of(case)
        _INFO[case[0]] = (cs, kind, oracle(cs, kind, cs["params"]))
    return _INFO[case[0]]


def mstep_gradient(cs, kind, n1, n0, prob, params):
    """The gradient the M-step forms from the expected counts, in float64: for IRT Dc sum_g (n1 (1 - P) - n0 P) u_g with P = prob
    where the clamp is not active (the oracle's tables say where it is), for the CDMs the same sum over the class of each
    parameter with u = +-1."""
    W1, W0, _ = tables(cs, kind, params)
    J = cs["J"]
    K = W1.shape[1] // J
    # W1 = (1 - P) u, W0 = P u  ->  u = W1 + W0 (zero where the clamp is active); the P of the counts' own table replaces the oracle's
    u = (W1 + W0).reshape(-1, J, K)                                 # [G][J][K]
    P = np.asarray(prob, np.float64).T[:, :, None]                  # [G][J][1]
    r = np.asarray(n1, np.float64).T[:, :, None] * (1 - P) - np.asarray(n0, np.float64).T[:, :, None] * P
    return (r * u).sum(0).reshape(-1)


def _split16(v):
    """float32 -> (fp16 head, fp16 remainder) as float32."""
    h = v.astype(np.float16)
    lo = (v - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float32), lo.astype(np.float32)


def scale_exp(bound):
    """f16_scale_exp of vx_common.h: the power of two that brings |v| <= bound under 2^15."""
    _, e = np.frexp(np.float32(bound))
    return 15 - int(e)


def restated_f32(cs, kind, params, y=None, slab=SLAB):
    """info and gradient by the kernels' arithmetic in numpy (see the module docstring)."""
    y = cs["y"] if y is None else y
    K, _ = layout(cs, kind)
    ll, logw = grid_loglik(cs, kind, params, y)
    f = (ll.astype(np.float32) + logw.astype(np.float32)[None, :]).astype(np.float32)
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp(f - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    p = np.exp((f - lk).astype(np.float32)).astype(np.float32) * np.float32(16384.0)
    ph, pl = _split16(p)
    W1, W0, bound = tables(cs, kind, params)
    sc_ = np.float32(2.0 ** scale_exp(bound))
    un = np.float32(1.0) / sc_
    parts = []
    for W in (W1, W0):
        wh, wl = _split16(W.astype(np.float32) * sc_)
        parts.append(((ph @ wh + ph @ wl).astype(np.float32) + pl @ wh).astype(np.float32) * np.float32(1.0 / 16384.0))
    y1, y0 = np.repeat(y == 1, K, axis=1), np.repeat(y == 0, K, axis=1)
    S = (np.where(y1, parts[0], np.float32(0)) - np.where(y0, parts[1], np.float32(0))).astype(np.float32)
    S = np.concatenate([S, np.full((len(y), 1), sc_, np.float32)], axis=1)          # the constant column
    sh, sl = _split16(S)
    acc = np.zeros((S.shape[1], S.shape[1]), np.float32)
    for i0 in range(0, len(y), slab):
        h, lo = sh[i0:i0 + slab], sl[i0:i0 + slab]
        acc = acc + ((h.T @ h + h.T @ lo).astype(np.float32) + lo.T @ h).astype(np.float32)
    acc = acc * (un * un)
    return {"info": acc[:-1, :-1], "gradient": acc[:-1, -1], "n": float(acc[-1, -1])}


if __name__ == "__main__":
    write_golden()
