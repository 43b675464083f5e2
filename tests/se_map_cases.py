"""The cases, the float64 oracle and the float32 restatement of item_information(prior=) / item_se(prior=): the information of
the 3PL / 4PL item parameters at the Bayes-modal fit (vx_grid_wtable_irt_map, k_grid_wtable_irt_asym in
vipsy_amd/csrc/k_grid_info.hip).  tests/test_se_map_host.py on the CPU, tests/test_gpu_se_map.py on the GPU.

Dense layout: column c = j K + k; k = 0: b, k = 1 + d: a_d, k = D + 1: c_un, k = D + 2: d_un (4PL); K = D + 2 for 3PL, D + 3 for 4PL.
With the cell of the penalised M-step (tests/map_cases.item_eval says it too, independently of this file),

    P = c + (d - c) s(z),  Q = (1 - d) + (d - c) s(-z),  v = dP / d(unknown),  W1 = v / P,  W0 = v / Q   (0 where P or Q < eps32),
    S[i][(j,k)] = sum_g p_i(g) ([y_ij == 1] W1 - [y_ij == 0] W0),   info = S^T S,   gradient = sum_i S[i],

and the prior's share prior_precision = 1 / sd^2, prior_gradient = -precision (p - mean) over the free unknowns.  The standard
errors are the square roots of the diagonal of (info[kept, kept] + diag(precision[kept]))^-1, kept = the free columns whose
LIKELIHOOD diagonal is not exactly zero.

Cases: the smallest shapes at which the new code can go wrong (CASES); every one with an item nobody answered (UNANSWERED), 20 %
missing cells, priors of the README's kind and a weak one on a; 2 500 persons for the standard errors, the first 300 of them (one
slab of 256 and a ragged one) for the matrix alone.  The priors' means are the README's (c_un -1.4, d_un 2.2); their sd is 0.5, and
1.0 on a: at the README's sd of 1.0 (a: 2.0) the float64 condition number of the inverted block at 2 500 persons is 496, 2 413,
1 037 and 1 032 for the four cases -- above CONDITION_MAX = 1e3 (tests/se_cases.py), the smallest eigenvalue being the prior's
own where the data say little -- and with these it is 224, 830, 304 and 261.  The cap was not raised; the priors were tightened.
The engine stands at the generating values, copied in; nothing is trained.  FALLING: an item of the 4PL D = 1 case with d_un < c_un, a falling curve.  Spans and
slopes keep every P and Q above 1e-6 at every node, so no `inside` decision sits near its threshold (the host test asserts it).

restated_f32 says the kernels' arithmetic again in numpy, in the manner of se_cases.restated_f32: the tables in float32, their
power of two from their own largest magnitude, p 2^14, W 2^s and S 2^s as fp16 heads and remainders, float32 sums in slabs of 256."""
import numpy as np
import torch

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import map_cases as mc
from tests import score_cases as sc
from tests import se_cases as se

EPS32 = float(np.finfo(np.float32).eps)
MODEL_NO = mc.MODEL_NO
UNANSWERED = 2
N_SE, N_INFO = 2500, 300
PRIOR_A = (1.0, 1.0)
PRIOR_C, PRIOR_D = (mc.PRIOR_C[0], 0.5), (mc.PRIOR_D[0], 0.5)
PQ_MIN = 1e-6
FALLING_CASE, FALLING_ITEM = "sm2_4pl_d1_j8", 5

# name -> model, D, J, nodes a dimension, span, Dc, seed
CASES = {
    "sm1_3pl_d1_j11": dict(model="irt_3pl", D=1, J=11, nodes=61, span=6.0, Dc=1.0, seed=51),      # P = 33: one column past a tile
    "sm2_4pl_d1_j8": dict(model="irt_4pl", D=1, J=8, nodes=61, span=6.0, Dc=1.0, seed=52),        # P = 32: column P opens tile 2
    "sm3_3pl_d2_j13": dict(model="irt_3pl", D=2, J=13, nodes=7, span=4.0, Dc=1.0, seed=53),       # P = 52, G = 49, masked loadings
    "sm4_4pl_d3_j7": dict(model="irt_4pl", D=3, J=7, nodes=5, span=3.0, Dc=1.0, seed=54),         # K = 6, P = 42, G = 125
}
IDS = list(CASES)
SCHED2_IDS = ("sm1_3pl_d1_j11", "sm4_4pl_d3_j7")
# for the bit rules: (score_cases.irt_case tuples) 1PL at D = 1 and 2PL at D = 2, and the prior each is called with
BIT_CASES = [(("smb_1pl_d1", 300, 9, "irt_1pl", 1, 1.0, 61, 0.2, (1.0, 1.0), 61), {"b": (0.0, 2.0)}),
             (("smb_2pl_d2", 300, 10, "irt_2pl", 2, 1.0, 9, 0.2, (0.6, 1.3), 62), {"a": PRIOR_A})]
BIT_IDS = [c[0][0] for c in BIT_CASES]


def _logit(p):
    return np.log(p) - np.log1p(-p)


def K_of(cs):
    return cs["D"] + MODEL_NO[cs["model"]] - 1


_CASE = {}


def case(name, n=N_SE):
    """The case with its first n persons, built once and never modified: y [n][J] u8, theta [G][D], logw [G], params (float32
    unconstrained leaves a [D][J], b, c, d [1][J]: the generating values), a_free [D][J] bool, prior (what item_se takes)."""
    if name not in _CASE:
        from vipsy_amd.grid import score_grid
        spec = CASES[name]
        model, D, J = spec["model"], spec["D"], spec["J"]
        m = MODEL_NO[model]
        rng = np.random.RandomState(spec["seed"])
        free = vo.default_a_free(D, J)
        free = np.ones((D, J), bool) if free is None else np.asarray(free, bool)
        a = rng.uniform(0.7, 1.2, size=(D, J)) * free
        b = rng.uniform(-1.5, 1.5, size=(1, J))
        c = rng.uniform(0.1, 0.3, size=(1, J))
        d = rng.uniform(0.85, 0.97, size=(1, J)) if m == 4 else np.ones((1, J))
        if name == FALLING_CASE:
            c[0, FALLING_ITEM], d[0, FALLING_ITEM] = 0.62, 0.38
        x = rng.normal(size=(N_SE, D))
        y = (rng.uniform(size=(N_SE, J)) < c + (d - c) * vo.sigmoid(spec["Dc"] * (x @ a + b))).astype(np.uint8)
        y[rng.uniform(size=(N_SE, J)) < 0.20] = 255
        y[:, UNANSWERED] = 255
        theta, logw = score_grid(D, spec["nodes"], spec["span"])
        params = {"a": a, "b": b, "c": _logit(c)}
        if m == 4:
            params["d"] = _logit(d)
        prior = {"a": PRIOR_A, "c": PRIOR_C}
        if m == 4:
            prior["d"] = PRIOR_D
        _CASE[name] = {"name": name, "model": model, "D": D, "J": J, "N": N_SE, "Dc": spec["Dc"], "G": theta.shape[0], "y": y,
                       "theta": theta, "logw": logw, "nodes": spec["nodes"], "span": spec["span"],
                       "params": {k: v.astype(np.float32) for k, v in params.items()}, "a_free": free, "prior": prior}
    cs = _CASE[name]
    return cs if n == N_SE else dict(cs, y=cs["y"][:n], N=n)


def layout(cs):
    """K and the free mask over the dense layout: b, c_un, d_un always, the loadings by a_free."""
    K, D = K_of(cs), cs["D"]
    free = np.ones((cs["J"], K), bool)
    free[:, 1:1 + D] = cs["a_free"].T
    return K, free.reshape(-1)


def dense(cs, params):
    """The leaves as the dense vector [P], float64."""
    J = cs["J"]
    cols = [np.asarray(params["b"], np.float64).reshape(1, J), np.asarray(params["a"], np.float64).reshape(cs["D"], J),
            np.asarray(params["c"], np.float64).reshape(1, J)]
    if "d" in params:
        cols.append(np.asarray(params["d"], np.float64).reshape(1, J))
    return np.concatenate(cols, 0).T.reshape(-1)


def undense(cs, v):
    """The dense vector [P] as leaves."""
    J, D = cs["J"], cs["D"]
    m = np.asarray(v).reshape(J, -1).T
    out = {"b": m[0:1].copy(), "a": m[1:1 + D].copy(), "c": m[D + 1:D + 2].copy()}
    if m.shape[0] > D + 2:
        out["d"] = m[D + 2:D + 3].copy()
    return out


def prior_terms(cs, params, prior=None):
    """(prior_precision, prior_gradient) [P] float64 through the product's own checker of `prior` (grid.em_prior)."""
    from vipsy_amd.grid import em_prior
    pr = em_prior(cs["prior"] if prior is None else prior, cs["model"], cs["D"], cs["J"]).astype(np.float64)
    K, free = layout(cs)
    rows = [0] + list(range(1, 1 + cs["D"])) + [4] + ([5] if MODEL_NO[cs["model"]] == 4 else [])
    prec = np.where(free.reshape(cs["J"], K), pr[1, rows].T, 0.0).reshape(-1)
    mean = pr[0, rows].T.reshape(-1)
    return prec, -prec * (dense(cs, params) - mean)


def cell(cs, params, dtype=np.float64):
    """sg, sn, P, Q, inside [G][J] and the capped c, d, 1 - d [J] in `dtype`, as gm_eval<3 | 4> forms them."""
    dt = np.dtype(dtype).type
    J, D = cs["J"], cs["D"]
    eps = dt(EPS32)
    sig = lambda v: (dt(1) / (dt(1) + np.exp(-v))).astype(dtype)     # noqa: E731
    theta = np.asarray(cs["theta"], dtype)
    a, b = np.asarray(params["a"], dtype).reshape(D, J), np.asarray(params["b"], dtype).reshape(1, J)
    cu = np.asarray(params["c"], dtype).reshape(J)
    c = np.minimum(sig(cu), dt(1) - eps)
    if "d" in params:
        du = np.asarray(params["d"], dtype).reshape(J)
        d, omd = np.minimum(sig(du), dt(1) - eps), np.maximum(sig(-du), eps)
    else:
        d, omd = np.ones(J, dtype), np.zeros(J, dtype)
    z = (dt(cs["Dc"]) * (theta @ a + b)).astype(dtype)
    e = np.exp(-np.abs(z))
    sg = np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
    sn = np.where(z >= 0, e / (1 + e), 1 / (1 + e)).astype(dtype)
    P, Q = (c + (d - c) * sg).astype(dtype), (omd + (d - c) * sn).astype(dtype)
    return {"sg": sg, "sn": sn, "P": P, "Q": Q, "inside": (P >= eps) & (Q >= eps), "c": c, "d": d, "omd": omd}


def tables(cs, params, dtype=np.float64):
    """(W1 [G][P], W0 [G][P], the largest magnitude of both) in `dtype`."""
    dt = np.dtype(dtype).type
    D, J, K = cs["D"], cs["J"], K_of(cs)
    t = cell(cs, params, dtype)
    theta = np.asarray(cs["theta"], dtype)
    G = theta.shape[0]
    eps = dt(EPS32)
    U = dt(cs["Dc"]) * np.concatenate([np.ones((G, 1), dtype), theta], axis=1)       # [G][D + 1]
    V = np.zeros((G, J, K), dtype)
    V[:, :, :D + 1] = ((t["d"] - t["c"]) * t["sg"] * t["sn"])[:, :, None] * U[:, None, :]
    V[:, :, D + 1] = t["sn"] * (t["c"] * (dt(1) - t["c"]))
    if K == D + 3:
        V[:, :, D + 2] = t["sg"] * (t["d"] * t["omd"])
    Pc, Qc = np.clip(t["P"], eps, dt(1) - eps), np.clip(t["Q"], eps, dt(1) - eps)
    W1 = np.where(t["inside"][:, :, None], V / Pc[:, :, None], 0).astype(dtype).reshape(G, -1)
    W0 = np.where(t["inside"][:, :, None], V / Qc[:, :, None], 0).astype(dtype).reshape(G, -1)
    return W1, W0, float(max(np.abs(W1).max(), np.abs(W0).max()))


def grid_loglik(cs, params, y):
    """ll [n][G] in float64 from the cell's own P and Q (no clamp is active: P, Q >= PQ_MIN); the host test holds it against
    score_cases.irt_grid_loglik."""
    t = cell(cs, params)
    return (y == 1).astype(np.float64) @ np.log(t["P"]).T + (y == 0).astype(np.float64) @ np.log(t["Q"]).T


def logpost(cs, v, y, prior=None):
    """The float64 marginal log-likelihood of the rows y plus the log prior (constants dropped) at the dense vector v."""
    from vipsy_amd.grid import em_prior
    params = undense(cs, v)
    f = grid_loglik(cs, params, y) + np.asarray(cs["logw"], np.float64)[None, :]
    m = f.max(1)
    lik = float((m + np.log(np.exp(f - m[:, None]).sum(1))).sum())
    pr = em_prior(cs["prior"] if prior is None else prior, cs["model"], cs["D"], cs["J"]).astype(np.float64)
    K, free = layout(cs)
    rows = [0] + list(range(1, 1 + cs["D"])) + [4] + ([5] if MODEL_NO[cs["model"]] == 4 else [])
    prec, mean = np.where(free.reshape(cs["J"], K), pr[1, rows].T, 0.0).reshape(-1), pr[0, rows].T.reshape(-1)
    return lik - 0.5 * float((prec * (np.asarray(v, np.float64) - mean) ** 2).sum())


def oracle(cs, params=None, y=None, prior=None):
    """info, gradient, the prior terms, n, K, free, kept, cov, se [P] (NaN off the kept columns), the condition number of the
    block that is inverted; also p, n1, n0 and S."""
    params = cs["params"] if params is None else params
    y = cs["y"] if y is None else y
    K, free = layout(cs)
    ll = sc.irt_grid_loglik(cs["model"], cs["theta"], params, cs["Dc"], y)
    t = cc.counts(ll, cs["logw"], y)
    W1, W0, top = tables(cs, params)
    S = se.scores(t["p"], W1, W0, y, K)
    info = S.T @ S
    prec, pgrad = prior_terms(cs, params, prior)
    kept = se.kept_of(info, free)
    out = {"info": info, "gradient": S.sum(0), "prior_precision": prec, "prior_gradient": pgrad, "n": len(y), "K": K, "free": free,
           "kept": kept, "S": S, "p": t["p"], "n1": t["n1"], "n0": t["n0"], "top": top}
    A = info[np.ix_(kept, kept)] + np.diag(prec[kept])
    w = np.linalg.eigvalsh(A)
    cov = np.linalg.inv(A)
    sd = np.full(len(free), np.nan)
    sd[kept] = np.sqrt(np.diag(cov))
    out.update(cov=cov, se=sd, condition=float(w[-1] / w[0]))
    return out


_ORACLE = {}


def oracle_of(name, n=N_SE):
    """(cs, oracle) of a case at its first n persons, computed once and shared (never modified)."""
    if (name, n) not in _ORACLE:
        cs = case(name, n)
        _ORACLE[(name, n)] = (cs, oracle(cs))
    return _ORACLE[(name, n)]


def mstep_gradient(cs, n1, n0, params=None, prior=None):
    """The gradient of the penalised Q the M-step forms from n1 / n0 [J][G] (map_cases.item_eval in float64, which says the cell
    on its own), over the dense layout.  Every unknown the model has is taken as free in the likelihood part; the penalty is that
    of the free unknowns."""
    from vipsy_amd.grid import em_prior
    params = cs["params"] if params is None else params
    pr = em_prior(cs["prior"] if prior is None else prior, cs["model"], cs["D"], cs["J"]).astype(np.float64)
    D, J = cs["D"], cs["J"]
    rows = [0] + list(range(1, 1 + D)) + [4] + ([5] if MODEL_NO[cs["model"]] == 4 else [])
    fr = np.zeros(mc.ROWS, bool)
    fr[rows] = True
    _, free = layout(cs)
    free = free.reshape(J, -1)
    p = mc.pack(cs, params)
    U = mc.design(np.asarray(cs["theta"], np.float64))
    out = np.zeros((J, len(rows)))
    for j in range(J):
        pp = np.zeros(mc.ROWS)
        pp[rows] = np.where(free[j], pr[1, rows, j], 0.0)
        g = mc.item_eval(cs["model"], U, cs["Dc"], np.asarray(n1, np.float64)[j], np.asarray(n0, np.float64)[j], p[:, j], fr,
                         pr[0, :, j], pp)[1]
        out[j] = g[rows]
    return out.reshape(-1)


def restated_f32(cs, params=None, y=None, slab=se.SLAB):
    """info and gradient by the kernels' arithmetic in numpy (see the module docstring)."""
    params = cs["params"] if params is None else params
    y = cs["y"] if y is None else y
    K = K_of(cs)
    ll = sc.irt_grid_loglik(cs["model"], cs["theta"], params, cs["Dc"], y)
    f = (ll.astype(np.float32) + np.asarray(cs["logw"], np.float32)[None, :]).astype(np.float32)
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp(f - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    p = np.exp((f - lk).astype(np.float32)).astype(np.float32) * np.float32(16384.0)
    ph, pl = se._split16(p)
    W1, W0, top = tables(cs, params, np.float32)
    sc_ = np.float32(2.0 ** se.scale_exp(top))
    un = np.float32(1.0) / sc_
    parts = []
    for W in (W1, W0):
        wh, wl = se._split16(W * sc_)
        parts.append(((ph @ wh + ph @ wl).astype(np.float32) + pl @ wh).astype(np.float32) * np.float32(1.0 / 16384.0))
    y1, y0 = np.repeat(y == 1, K, axis=1), np.repeat(y == 0, K, axis=1)
    S = (np.where(y1, parts[0], np.float32(0)) - np.where(y0, parts[1], np.float32(0))).astype(np.float32)
    S = np.concatenate([S, np.full((len(y), 1), sc_, np.float32)], axis=1)          # the constant column
    sh, sl = se._split16(S)
    acc = np.zeros((S.shape[1], S.shape[1]), np.float32)
    for i0 in range(0, len(y), slab):
        h, lo = sh[i0:i0 + slab], sl[i0:i0 + slab]
        acc = acc + ((h.T @ h + h.T @ lo).astype(np.float32) + lo.T @ h).astype(np.float32)
    acc = acc * (un * un)
    return {"info": acc[:-1, :-1], "gradient": acc[:-1, -1], "scale": float(sc_), "top": top}


def info_errors(got_info, got_grad, want_info, want_grad, n):
    """The row rule's two figures (tests/test_gpu_se.py): info with floor = its largest diagonal entry, gradient as one row with
    floor = (largest diagonal x n)^0.5."""
    from tests.test_gpu_response_designs import _row_errors
    f8 = lambda t: np.asarray(t, np.float64)                        # noqa: E731
    top = float(np.abs(np.diag(want_info)).max())
    e_i, row = _row_errors(f8(got_info), f8(want_info), floor=top)
    e_g, _ = _row_errors(f8(got_grad)[None, :], f8(want_grad)[None, :], floor=np.sqrt(top * n))
    return e_i, row, e_g


# ---- a backend for the host tests --------------------------------------------------------------------------------------------
class SeMapOracleBackend(mc.MapOracleBackend):
    """MapOracleBackend (an OracleBackend) with the entries item_information(prior=) calls, in float64 numpy on CPU tensors: the
    derivative tables are kept as the parameters they were asked for (the image is never read), vx_grid_info is oracle()'s sum."""

    def grid_wimage_bytes(self, P, G):
        return 16

    def grid_info_workspace(self, nb, P, G):
        return 1

    def grid_wtable_irt_map(self, cfg, theta, G, a, b, c_un, d_un, wimg):
        f8 = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
        model, D, J = mc.CODE_MODEL[cfg.model], cfg.D, cfg.J
        assert MODEL_NO[model] >= 3, "the host backend tabulates the asymptote models only"
        params = {k: v for k, v in (("a", f8(a)), ("b", f8(b)), ("c", f8(c_un)), ("d", f8(d_un))) if v is not None}
        self._wtab = ({"model": model, "D": D, "J": J, "Dc": cfg.Dc, "theta": f8(theta)}, params)

    def grid_info(self, y, rows, nb, J, G, K, img, wimg, logw, loglik, info, gradient, ws, ws_floats):
        assert rows is None
        cs, params = self._wtab
        yy = y.cpu().numpy()
        t = cc.counts(self._ll(y), logw.cpu().numpy(), yy)
        W1, W0, _ = tables(cs, params)
        S = se.scores(t["p"], W1, W0, yy, K)
        info.copy_(torch.from_numpy((S.T @ S).astype(np.float32)))
        gradient.copy_(torch.from_numpy(S.sum(0).astype(np.float32)))
