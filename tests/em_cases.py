"""The float64 oracle and the cases of the EM tests (tests/test_em_host.py on the CPU, tests/test_gpu_em.py on the GPU).  Built on
tests/score_cases.py and tests/count_cases.py: one oracle EM iteration is

    1. the float64 tables of count_cases.counts over score_cases.irt_grid_loglik / cdm_grid_loglik (the marginal log-likelihood
       of the parameters the iteration starts from falls out of score_cases.grid_posterior);
    2. the M-step of vipsy_amd/csrc/k_grid_mstep.hip said in numpy: for IRT `newton` Newton steps an item on
           Q_j = sum_g n1 log P + n0 log(1 - P),   z = Dc (theta_g . a_j + b_j) clamped to +-ZL,
       a clamped node adding nothing to gradient or curvature, the same mask, the same acceptance rule (Q may fall by 1e-6 |Q|,
       else halve, at most 8 times, else stop), the same cap of 4 on a step's largest component; for DINA / DINO the closed
       form  g_un = log R0 - log W0,  s_un = log W1 - log R1  clamped to +-ZL, a class without mass left alone.

newton_mstep runs in the dtype it is handed: float64 is the oracle, float32 the stand-in of the kernel's arithmetic.

Cases and starts (em_cases()): IRT_CASES[0] (2PL, N = 33, J = 37: ragged everything, a person without answers, one all-correct)
and COUNT_BIG (N = 2 500) from a = 1, b = 0; case5_2pl_d2_441 and case5_2pl_d3_729 (masked loadings) from a = 0.5 a_free, b = 0;
a 1PL case of its own (ONEPL: N = 300, J = 50, thresholds in +-1.5 -- case3 of the score tests draws them over +-4 and has
constant items, whose maximiser is at infinity, where no two arithmetics agree) from b = 0; the three CDM cases from the engine's
g = s = 0.1."""
import numpy as np

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import score_cases as sc

ZL = 15.942384719848633          # logit(1 - eps32) as the kernels hold it
QTOL = 1e-6
HALVINGS = 8
STEP_CAP = 4.0
ONEPL = ("em_1pl_n300_j50", 300, 50, "irt_1pl", 1, 1.702, 41, 0.10, None, 51)
IRT_EM = [sc.IRT_CASES[0], sc.IRT_CASES[4], sc.IRT_CASES[5], cc.COUNT_BIG, ONEPL]
CDM_EM = list(sc.CDM_CASES)
ALL_EM = IRT_EM + CDM_EM
G_S_START = float(np.float32(np.log(np.float32(0.1)) - np.log1p(-np.float32(0.1))))     # engine._init_g_s


def onepl_case():
    name, N, J, model, D, Dc, nodes, missing, _, seed = ONEPL
    rng = np.random.RandomState(seed)
    b = rng.uniform(-1.5, 1.5, size=(1, J))
    x = rng.normal(0.0, 1.0, size=(N, 1))
    y = (rng.uniform(size=(N, J)) < vo.sigmoid(Dc * (x + b))).astype(np.uint8)
    y[rng.uniform(size=(N, J)) < missing] = 255
    return {"name": name, "N": N, "J": J, "model": model, "D": D, "Dc": Dc, "nodes": nodes, "span": sc.SPAN, "y": y,
            "params": {"b": b.astype(np.float32)}}


def case_of(case):
    """The case (responses and shapes) and kind ('irt' / 'cdm')."""
    if case == ONEPL:
        return onepl_case(), "irt"
    if case in sc.CDM_CASES:
        return sc.cdm_case(case), "cdm"
    return sc.irt_case(case), "irt"


def a_free_of(cs):
    """The engine's mask over a ([D][J] bool; all free for one dimension), None for 1PL."""
    if cs["model"] == "irt_1pl":
        return None
    f = vo.default_a_free(cs["D"], cs["J"])
    return np.ones((cs["D"], cs["J"]), bool) if f is None else f


def start_of(cs, kind):
    """The start of the case as float32 unconstrained leaves -- what the engine holds before fit_em."""
    if kind == "cdm":
        return {"g": np.full((1, cs["J"]), G_S_START, np.float32), "s": np.full((1, cs["J"]), G_S_START, np.float32)}
    p = {"b": np.zeros((1, cs["J"]), np.float32)}
    if cs["model"] != "irt_1pl":
        free = a_free_of(cs)
        p["a"] = ((0.5 if cs["D"] > 1 else 1.0) * free).astype(np.float32)
    return p


def grid_of(cs):
    from vipsy_amd.engine import score_grid
    return score_grid(cs["D"], cs["nodes"], cs["span"])


# ---- the E-step ----------------------------------------------------------------------------------------------------------
def irt_estep(cs, params, y=None):
    """float64 tables and the marginal log-likelihood of `params`: (n1 [J][G], n0 [J][G], loglik)."""
    y = cs["y"] if y is None else y
    theta, logw = grid_of(cs)
    ll = sc.irt_grid_loglik(cs["model"], theta, params, cs["Dc"], y)
    t = cc.counts(ll, logw, y)
    return t["n1"], t["n0"], float(sc.grid_posterior(ll, logw, theta)["loglik"].sum())


def cdm_estep(cs, params, y=None):
    y = cs["y"] if y is None else y
    ll, logw, attrs = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], params, y)
    t = cc.counts(ll, logw, y)
    return t["n1"], t["n0"], float(sc.grid_posterior(ll, logw, attrs)["loglik"].sum())


# ---- the M-step ----------------------------------------------------------------------------------------------------------
def _item_eval(U, c1, c0, p, Dc, zl):
    z = Dc * (U @ p)
    zc = np.clip(z, -zl, zl)
    inside = zc == z
    e = np.exp(-np.abs(zc))
    sp = np.maximum(zc, 0) + np.log1p(e)
    sg = np.where(zc >= 0, 1 / (1 + e), e / (1 + e)).astype(U.dtype)
    q = (c1 * (zc - sp) - c0 * sp).sum(dtype=U.dtype)
    r = np.where(inside, c1 * (1 - sg) - c0 * sg, 0).astype(U.dtype)
    w = np.where(inside, (c1 + c0) * sg * (1 - sg), 0).astype(U.dtype)
    return q, Dc * (U.T @ r), Dc * Dc * ((U * w[:, None]).T @ U)


def newton_mstep(model, theta, Dc, n1, n0, a, b, free, newton, dtype=np.float64, stats=None):
    """New (a [D][J] or None, b [1][J]) in `dtype`; stats (a dict, optional) counts halvings, capped steps, stopped items."""
    dt = np.dtype(dtype).type
    theta = np.asarray(theta, dtype)
    G, D = theta.shape
    n1, n0 = np.asarray(n1, dtype), np.asarray(n0, dtype)
    J = n1.shape[0]
    U = np.concatenate([np.ones((G, 1), dtype), theta], axis=1)
    b = np.array(b, dtype).reshape(1, J)
    a = None if model == "irt_1pl" else np.array(a, dtype).reshape(D, J)
    Dc, zl, qtol, cap = dt(Dc), dt(ZL), dt(QTOL), dt(STEP_CAP)
    st = {"halvings": 0, "capped": 0, "stopped": 0} if stats is None else stats
    for k in ("halvings", "capped", "stopped"):
        st.setdefault(k, 0)
    for j in range(J):
        c1, c0 = n1[j], n0[j]
        if not (c1 + c0).sum() > 0:
            continue
        if model == "irt_1pl":
            p, fr = np.array([b[0, j], 1], dtype), np.array([True, False])
        else:
            p, fr = np.concatenate([b[:, j], a[:, j]]).astype(dtype), np.concatenate([[True], np.asarray(free)[:, j] != 0])
        q, g, H = _item_eval(U, c1, c0, p, Dc, zl)
        for _ in range(newton):
            try:
                L = np.linalg.cholesky(H[np.ix_(fr, fr)])
            except np.linalg.LinAlgError:
                st["stopped"] += 1
                break
            d = np.zeros_like(p)
            d[fr] = np.linalg.solve(L.T, np.linalg.solve(L, g[fr])).astype(dtype)
            m = np.abs(d).max()
            if not np.isfinite(m):
                st["stopped"] += 1
                break
            t = dt(1)
            if m > cap:
                t = cap / m
                st["capped"] += 1
            moved = False
            for _h in range(HALVINGS + 1):
                pt = (p + t * d).astype(dtype)
                qt, gt, Ht = _item_eval(U, c1, c0, pt, Dc, zl)
                if qt >= q - qtol * abs(q):
                    p, q, g, H, moved = pt, qt, gt, Ht, True
                    break
                st["halvings"] += 1
                t = t * dt(0.5)
            if not moved:
                st["stopped"] += 1
                break
        b[0, j] = p[0]
        if a is not None:
            a[fr[1:], j] = p[1:][fr[1:]]
    return a, b


def cdm_mstep(cdm, K, q, n1, n0, g_un, s_un):
    """The closed form on the unconstrained scale (float64), clamped to +-ZL; a class without mass keeps its value."""
    eta, _ = (vo.dino_eta if cdm == "dino" else vo.dina_eta)(K, np.asarray(q, np.float64))
    e1 = (eta > 0).T                                                    # [J][C]
    R1, W1 = (n1 * e1).sum(1), (n0 * e1).sum(1)
    R0, W0 = (n1 * ~e1).sum(1), (n0 * ~e1).sum(1)
    g = np.array(g_un, np.float64).reshape(1, -1)
    s = np.array(s_un, np.float64).reshape(1, -1)
    with np.errstate(divide="ignore", invalid="ignore"):          # (a class without mass: log 0 - log 0, not used)
        gn = np.clip(np.log(R0) - np.log(W0), -ZL, ZL)
        sn = np.clip(np.log(W1) - np.log(R1), -ZL, ZL)
    g[0, R0 + W0 > 0] = gn[R0 + W0 > 0]
    s[0, R1 + W1 > 0] = sn[R1 + W1 > 0]
    return g, s


# ---- EM ------------------------------------------------------------------------------------------------------------------
def em_iteration(cs, kind, params, newton=4, y=None, stats=None):
    """(parameters after one oracle iteration from `params`, the marginal log-likelihood of `params`)."""
    if kind == "cdm":
        n1, n0, lk = cdm_estep(cs, params, y)
        g, s = cdm_mstep(cs["cdm"], cs["K"], cs["q"], n1, n0, params["g"], params["s"])
        return {"g": g, "s": s}, lk
    n1, n0, lk = irt_estep(cs, params, y)
    theta, _ = grid_of(cs)
    a, b = newton_mstep(cs["model"], theta, cs["Dc"], n1, n0, params.get("a"), params["b"], a_free_of(cs), newton, stats=stats)
    out = {"b": b}
    if a is not None:
        out["a"] = a
    return out, lk


_TRAJ = {}


def trajectory(case, iters, newton=4):
    """The oracle's EM from the case's start, computed once and shared (never modified): (cs, kind, params after 0 .. iters
    iterations, loglik[0 .. iters - 1], stats)."""
    key = (case[0], newton)
    if key not in _TRAJ:
        cs, kind = case_of(case)
        _TRAJ[key] = (cs, kind, [{k: v.astype(np.float64) for k, v in start_of(cs, kind).items()}], [], {})
    cs, kind, ps, lks, stats = _TRAJ[key]
    while len(lks) < iters:
        p, lk = em_iteration(cs, kind, ps[-1], newton, stats=stats)
        ps.append(p)
        lks.append(lk)
    return cs, kind, ps[:iters + 1], lks[:iters], stats


def design_case():
    """IRT_CASES[0] with item 4 answered by nobody and the observed answers of item 9 all 1."""
    cs = dict(sc.irt_case(sc.IRT_CASES[0]))
    y = cs["y"].copy()
    y[:, 4] = 255
    y[y[:, 9] != 255, 9] = 1
    cs["y"], cs["name"] = y, "em_design_n33_j37"
    return cs


DESIGN_UNANSWERED, DESIGN_CONSTANT = 4, 9
