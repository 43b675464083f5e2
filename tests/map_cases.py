"""The cases, the float64 oracle and the float32 restatement of the penalised M-step (vx_grid_mstep_irt_map,
vipsy_amd/csrc/k_grid_mstep_map.hip) and of fit_em(prior=): tests/test_map_host.py on the CPU, tests/test_gpu_map.py on the GPU.

Unknowns of an item, everywhere in this file, as the kernel orders them: p = (b, a_0, a_1, a_2, c_un, d_un) -- six rows whatever
the model; `free` [6][J] says which of them the item has (b; a_d for d < D where a_free allows; c_un from 3PL; d_un for 4PL).

item_eval is the kernel's evaluation in numpy, in the dtype it is handed (float64: the oracle; float32: the stand-in of the
kernel's arithmetic): the penalised Q_j, its gradient, the Fisher matrix plus diag(prec), and the sums of the absolute gradient
terms the one-step rule is scaled by.  map_mstep is the kernel's step control around it (em_cases.newton_mstep's, on the
penalised Q_j).

Cases (CASES): the smallest shapes at which the kernel can go wrong -- J no multiple of 4, G no multiple of 64, sixteen nodes a
lane, one node, masked loadings, every model -- each with 10 % missing, generating values a in [0.7, 1.8], b in [-1.5, 1.5], c in
[0.1, 0.3], d in [0.85, 0.98], the priors c_un ~ N(-1.4, 1), d_un ~ N(2.2, 1), and two more items: one nobody answered (UNANSWERED)
and one everybody answered correctly (the last), which has a prior on b so that its maximum is finite.

The rules and their constants.  A float32 sum of at most 16 terms a lane and six tree levels carries a relative error of at most
22 u = 11 eps32 of the sum of its absolute terms (u = eps32 / 2), and the terms themselves (exp, rcp, log of the hardware, a few
ulp each) about 4 eps32 more: 15 eps32.
  C_Q = 16    rule 1: the penalised Q_j the float64 maximiser can still gain from the kernel's output is at most C_Q 1e-6 |Q_j|.
              1e-6 |Q_j| is what the acceptance rule cannot see, and every accepted step may LOSE that much: `newton` times it in
              the worst case.  A run of such steps needs a direction that overshoots -- where the Fisher matrix understates the
              curvature, as for an item everybody answers alike (no n0: expected and observed information part ways), only a
              quarter step is accepted, and falls of just under the tolerance are accepted until the next halving is forced.
              That is a limit cycle of the step control itself, in exact arithmetic too: on the 4PL case's constant item the
              float64 restatement cycles between 0.02 and 5.3 times 1e-6 |Q_j| short of the maximum (float32: 6.2 at step 64);
              every other item of every case ends below 1e-8.  C_Q is twice the next power of two above that cycle.
  C_STEP = 32 rule 2: the output of one accepted full step equals the float64 step to C_STEP eps32 |H^-1| S, S_l = the sum of the
              absolute terms of gradient entry l: 15 eps32 S for the gradient's own rounding, and as much again for the rounding
              of the matrix (its entries are sums of the same length; the step is at most of size one here), rounded up to 2^5.
tests/test_map_host.py asserts that the method alone, said in float32 numpy, meets both at HALF the constant."""
import numpy as np
import torch

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import score_cases as sc
from tests.oracle_backend import CODE_MODEL, OracleBackend

EPS32 = float(np.finfo(np.float32).eps)
ZL = 15.942384719848633          # logit(1 - eps32), the clamp of gm_cell
QTOL, HALVINGS, STEP_CAP = 1e-6, 8, 4.0
ROWS = 6
MODEL_NO = {"irt_1pl": 1, "irt_2pl": 2, "irt_3pl": 3, "irt_4pl": 4}
C_Q = 16.0
C_STEP = 32.0
UNANSWERED = 1                   # the index of the item nobody answered; the constant item is the last
PRIOR_C, PRIOR_D = (-1.4, 1.0), (2.2, 1.0)

# name -> model, D, regular items (two more are added), nodes a dimension (or "one": the explicit one-node grid), span, persons,
# seed, priors beside those on c and d and the constant item's b.  D, J + 2, G:
CASES = {
    "map1_3pl_j14_g41": dict(model="irt_3pl", D=1, J=12, nodes=41, span=6.0, N=2048, seed=11, prior={}),
    "map2_4pl_j14_g41": dict(model="irt_4pl", D=1, J=12, nodes=41, span=6.0, N=2048, seed=12, prior={}),
    "map3_3pl_d2_j7_g441": dict(model="irt_3pl", D=2, J=5, nodes=21, span=5.0, N=600, seed=13, prior={}),
    "map4_2pl_j8_g61": dict(model="irt_2pl", D=1, J=6, nodes=61, span=6.0, N=500, seed=14, prior={"a": (1.0, 0.5)}),
    "map5_3pl_j5_g1024": dict(model="irt_3pl", D=1, J=3, nodes=1024, span=6.0, N=400, seed=15, prior={}),
    "map6_3pl_j6_g1": dict(model="irt_3pl", D=1, J=4, nodes="one", span=6.0, N=300, seed=16,
                           prior={"a": (1.0, 0.5), "b": (0.0, 2.0)}),
}
EM_CASES = ("map1_3pl_j14_g41", "map2_4pl_j14_g41")
EM_START = {"a": 1.0, "b": 0.0, "c": -1.4, "d": 2.2}           # the start of the end-to-end runs, every item alike


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _logit(p):
    return np.log(p) - np.log1p(-p)


def names_of(model):
    return [n for n, lo in (("a", 2), ("b", 1), ("c", 3), ("d", 4)) if MODEL_NO[model] >= lo]


_CASE = {}


def case(name):
    """The case, built once and never modified: y [N][J] u8, theta [G][D], logw [G], truth and start (unconstrained float32
    leaves: a [D][J], b, c, d [1][J]), a_free [D][J] bool (None for 1PL), prior (the dict fit_em takes), nodes (what fit_em takes)."""
    if name in _CASE:
        return _CASE[name]
    from vipsy_amd.engine import score_grid
    spec = CASES[name]
    model, D, N = spec["model"], spec["D"], spec["N"]
    J = spec["J"] + 2
    rng = np.random.RandomState(spec["seed"])
    free = vo.default_a_free(D, J)
    free = np.ones((D, J), bool) if free is None else np.asarray(free, bool)
    a = rng.uniform(0.7, 1.8, size=(D, J)) * free
    b = rng.uniform(-1.5, 1.5, size=(1, J))
    c = rng.uniform(0.1, 0.3, size=(1, J))
    d = rng.uniform(0.85, 0.98, size=(1, J))
    Dc = 1.702
    x = rng.normal(size=(N, D))
    z = Dc * (x @ a + b)
    m = MODEL_NO[model]
    lo = c if m >= 3 else 0.0
    hi = d if m == 4 else 1.0
    y = (rng.uniform(size=(N, J)) < lo + (hi - lo) * _sig(z)).astype(np.uint8)
    y[rng.uniform(size=(N, J)) < 0.10] = 255
    y[:, UNANSWERED] = 255
    y[y[:, J - 1] != 255, J - 1] = 1
    nodes = (np.array([[0.3]], np.float32), np.array([0.0], np.float32)) if spec["nodes"] == "one" else spec["nodes"]
    theta, logw = score_grid(D, nodes, spec["span"])
    truth = {"a": a, "b": b, "c": _logit(c), "d": _logit(d)}
    truth = {k: truth[k].astype(np.float32) for k in names_of(model)}
    start = {k: (v + rng.uniform(-0.5, 0.5, size=v.shape)).astype(np.float32) for k, v in truth.items()}
    if "a" in start:
        start["a"] = (start["a"] * free).astype(np.float32)
    prior = dict(spec["prior"])
    if "b" not in prior:                                            # the constant item alone has a prior on b
        sd = np.full((1, J), np.inf)
        sd[0, J - 1] = 2.0
        prior["b"] = (0.0, sd)
    if m >= 3:
        prior["c"] = PRIOR_C
    if m == 4:
        prior["d"] = PRIOR_D
    _CASE[name] = {"name": name, "model": model, "D": D, "J": J, "N": N, "Dc": Dc, "G": theta.shape[0], "y": y, "theta": theta,
                   "logw": logw, "nodes": nodes, "span": spec["span"], "truth": truth, "start": start,
                   "a_free": free if m >= 2 else None, "prior": prior}
    return _CASE[name]


# ---- six rows an item ------------------------------------------------------------------------------------------------------
def pack(cs, params, dtype=np.float64):
    """The leaves {a [D][J], b, c, d [1][J]} as p [6][J]; rows the model does not have: a = 1 for 1PL (z = Dc (theta + b)), else 0."""
    J, D = cs["J"], cs["D"]
    p = np.zeros((ROWS, J), dtype)
    p[0] = np.asarray(params["b"], dtype).reshape(J)
    if "a" in params:
        p[1:1 + D] = np.asarray(params["a"], dtype).reshape(D, J)
    else:
        p[1] = 1.0
    for k, row in (("c", 4), ("d", 5)):
        if k in params:
            p[row] = np.asarray(params[k], dtype).reshape(J)
    return p


def unpack(cs, p):
    J, D = cs["J"], cs["D"]
    out = {"b": p[0].reshape(1, J).copy()}
    if MODEL_NO[cs["model"]] >= 2:
        out["a"] = p[1:1 + D].reshape(D, J).copy()
    if MODEL_NO[cs["model"]] >= 3:
        out["c"] = p[4].reshape(1, J).copy()
    if MODEL_NO[cs["model"]] == 4:
        out["d"] = p[5].reshape(1, J).copy()
    return out


def free_rows(cs):
    """bool [6][J]: the unknowns of every item."""
    m, J, D = MODEL_NO[cs["model"]], cs["J"], cs["D"]
    fr = np.zeros((ROWS, J), bool)
    fr[0] = True
    if m >= 2:
        fr[1:1 + D] = cs["a_free"]
    fr[4] = m >= 3
    fr[5] = m == 4
    return fr


def prior_rows(cs, prior=None):
    """[2][6][J] float32 as the kernel takes it, through the product's own checker (tests/test_map_host.py tests that one)."""
    from vipsy_amd.grid import em_prior
    return em_prior(cs["prior"] if prior is None else prior, cs["model"], cs["D"], cs["J"])


def design(theta):
    """U [G][4]: (1, theta_g), zero beyond D."""
    theta = np.asarray(theta)
    U = np.zeros((theta.shape[0], 4), theta.dtype)
    U[:, 0] = 1
    U[:, 1:1 + theta.shape[1]] = theta
    return U


# ---- the kernel's evaluation -------------------------------------------------------------------------------------------------
def item_eval(model, U, Dc, c1, c0, p, fr, pm, pp, dtype=np.float64):
    """(Q_j penalised, gradient [6], matrix [6][6], S [6] = the sums of the absolute terms of the gradient) at p [6] in `dtype`;
    rows that are not free are zero in the gradient and the matrix."""
    dt = np.dtype(dtype).type
    m = MODEL_NO[model]
    U, c1, c0, p = np.asarray(U, dtype), np.asarray(c1, dtype), np.asarray(c0, dtype), np.asarray(p, dtype)
    pm, pp = np.asarray(pm, dtype), np.asarray(pp, dtype)
    Dc, eps = dt(Dc), dt(EPS32)
    z = Dc * (U @ p[:4])
    V = np.zeros((U.shape[0], ROWS), dtype)
    if m <= 2:
        zc = np.clip(z, dt(-ZL), dt(ZL))
        inside = zc == z
        e = np.exp(-np.abs(zc))
        lse = np.log1p(e)
        sg = np.where(zc >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
        sn = np.where(zc >= 0, e / (1 + e), 1 / (1 + e)).astype(dtype)
        lp1, lp0 = np.minimum(zc, 0) - lse, np.minimum(-zc, 0) - lse
        t1, t0 = np.where(inside, c1 * sn, 0).astype(dtype), np.where(inside, c0 * sg, 0).astype(dtype)
        ww = np.where(inside, (c1 + c0) * sg * sn, 0).astype(dtype)
        V[:, :4] = Dc * U
    else:
        c = min(dt(_sig(p[4])), dt(1) - eps)
        d = min(dt(_sig(p[5])), dt(1) - eps) if m == 4 else dt(1)
        omd = max(dt(_sig(-p[5])), eps) if m == 4 else dt(0)
        e = np.exp(-np.abs(z))
        sg = np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
        sn = np.where(z >= 0, e / (1 + e), 1 / (1 + e)).astype(dtype)
        P, Q = c + (d - c) * sg, omd + (d - c) * sn
        inside = (P >= eps) & (Q >= eps)
        Pc, Qc = np.clip(P, eps, dt(1) - eps), np.clip(Q, eps, dt(1) - eps)
        small = np.minimum(Pc, Qc)                                     # log of the larger one as log1p(-the smaller): gmm_log1m
        ls, lb = np.log(small), np.log1p(-small)
        lp1, lp0 = np.where(Pc >= Qc, lb, ls).astype(dtype), np.where(Pc >= Qc, ls, lb).astype(dtype)
        inv = np.where(inside, 1 / (Pc * Qc), 0).astype(dtype)
        t1, t0 = c1 * Qc * inv, c0 * Pc * inv
        ww = (c1 + c0) * inv
        V[:, :4] = (Dc * (d - c) * sg * sn)[:, None] * U
        V[:, 4] = sn * c * (dt(1) - c)
        if m == 4:
            V[:, 5] = sg * d * omd
    V = V * fr[None, :]
    pen = fr * pp * (p - pm)
    q = (c1 * lp1 + c0 * lp0).sum(dtype=dtype) - dt(0.5) * (pen * (p - pm)).sum(dtype=dtype)
    g = (V.T @ (t1 - t0)).astype(dtype) - pen
    H = ((V * ww[:, None]).T @ V).astype(dtype) + np.diag(fr * pp).astype(dtype)
    S = np.abs(V).T @ (np.abs(t1) + np.abs(t0)) + np.abs(pen)
    return q, g, H, S


def log_prior(p, fr, prior):
    """-1/2 sum prec (p - mean)^2 over the free unknowns of every item: [J], float64."""
    p, pr = np.asarray(p, np.float64), np.asarray(prior, np.float64)
    return -0.5 * (fr * pr[1] * (p - pr[0]) ** 2).sum(0)


def map_mstep(cs, n1, n0, p0, prior, newton, dtype=np.float64, stats=None, fr=None, theta=None):
    """`newton` steps of the kernel's method on every item from p0 [6][J]: the new p [6][J] in `dtype`.  stats (a dict,
    optional) counts halvings, capped steps, stopped items and keeps "margin": the smallest (Q_trial - (Q - 1e-6 |Q|)) / |Q|
    of any accepted FIRST trial (how clearly the full step was accepted)."""
    dt = np.dtype(dtype).type
    fr = free_rows(cs) if fr is None else fr
    U = design(np.asarray(cs["theta"] if theta is None else theta, dtype))
    n1, n0 = np.asarray(n1, dtype), np.asarray(n0, dtype)
    pr = np.asarray(prior, dtype)
    p = np.array(p0, dtype)
    st = {} if stats is None else stats
    for k in ("halvings", "capped", "stopped"):
        st.setdefault(k, 0)
    st.setdefault("margin", np.inf)
    for j in range(p.shape[1]):
        c1, c0, f = n1[j], n0[j], fr[:, j]
        if not (c1 + c0).sum() > 0:
            continue
        pj = p[:, j].copy()
        ev = lambda v: item_eval(cs["model"], U, cs["Dc"], c1, c0, v, f, pr[0, :, j], pr[1, :, j], dtype)    # noqa: E731
        q, g, H, _ = ev(pj)
        for _ in range(newton):
            try:
                L = np.linalg.cholesky(H[np.ix_(f, f)])
            except np.linalg.LinAlgError:
                st["stopped"] += 1
                break
            d = np.zeros(ROWS, dtype)
            d[f] = np.linalg.solve(L.T, np.linalg.solve(L, g[f])).astype(dtype)
            mx = np.abs(d).max()
            if not np.isfinite(mx):
                st["stopped"] += 1
                break
            t = dt(1)
            if mx > STEP_CAP:
                t = dt(STEP_CAP) / mx
                st["capped"] += 1
            moved = False
            for h in range(HALVINGS + 1):
                pt = np.where(f, pj + t * d, pj).astype(dtype)          # (what is not free keeps its bits)
                qt, gt, Ht, _ = ev(pt)
                if qt >= q - dt(QTOL) * abs(q):
                    if h == 0:
                        st["margin"] = min(st["margin"], float((qt - (q - dt(QTOL) * abs(q))) / abs(q)))
                    pj, q, g, H, moved = pt, qt, gt, Ht, True
                    break
                st["halvings"] += 1
                t = t * dt(0.5)
            if not moved:
                st["stopped"] += 1
                break
        p[:, j] = pj
    return p


# ---- the rules -----------------------------------------------------------------------------------------------------------------
def tables(cs, params=None):
    """The float64 E-step at `params` (default: the case's start): (n1, n0 [J][G], the marginal log-likelihood)."""
    params = cs["start"] if params is None else params
    ll = sc.irt_grid_loglik(cs["model"], cs["theta"], params, cs["Dc"], cs["y"])
    t = cc.counts(ll, cs["logw"], cs["y"])
    return t["n1"], t["n0"], float(sc.grid_posterior(ll, cs["logw"], cs["theta"])["loglik"].sum())


_LAUNCH = {}


def launch(name):
    """What one launch of a case is fed, built once: the float32 tables at the start, p0 [6][J] float32 (the start: within 0.5 of
    the generating values), p0_near (half as far: the start of the one-step rule), free, prior."""
    if name not in _LAUNCH:
        cs = case(name)
        n1, n0, _ = tables(cs)
        p0, pt = pack(cs, cs["start"], np.float32), pack(cs, cs["truth"], np.float32)
        _LAUNCH[name] = {"n1": n1.astype(np.float32), "n0": n0.astype(np.float32), "p0": p0, "p0_near": (pt + (p0 - pt) / 2).astype(np.float32),
                         "free": free_rows(cs), "prior": prior_rows(cs)}
    return _LAUNCH[name]


def answered(L):
    return (L["n1"] + L["n0"]).sum(1) > 0


def maximise(ev, p, f, iters=400):
    """The float64 maximiser of one item's penalised Q_j from p [6] (ev = item_eval at a point, f = its free rows): Newton
    with the observed Hessian (central differences of the analytic gradient), the Fisher matrix where that is not positive
    definite, strict ascent by halving.  Path-independent on purpose: nothing of the kernel's step control is in it.
    Returns (p_end, the largest component of the last step tried)."""
    p = np.array(p, np.float64)
    idx = np.flatnonzero(f)
    step = np.inf
    for _ in range(iters):
        q, g, H, _ = ev(p)
        Ho = np.zeros((len(idx), len(idx)))
        for n, k in enumerate(idx):
            e = np.zeros(ROWS)
            e[k] = 1e-5
            Ho[n] = -(ev(p + e)[1][idx] - ev(p - e)[1][idx]) / 2e-5
        Ho = 0.5 * (Ho + Ho.T)
        try:
            np.linalg.cholesky(Ho)
        except np.linalg.LinAlgError:
            Ho = H[np.ix_(idx, idx)]
        d = np.zeros(ROWS)
        d[idx] = np.linalg.solve(Ho, g[idx])
        step = float(np.abs(d).max())
        if step < 1e-11:
            break
        t, moved = min(1.0, STEP_CAP / step), False
        for _h in range(40):
            qt = ev(p + t * d)[0]
            if qt > q:
                p, moved = p + t * d, True
                break
            t *= 0.5
        if not moved:
            break
    return p, step


def rule1(cs, L, p_out, prior=None):
    """Rule 1 for an output p_out [6][J] of a launch on L's tables: the float64 maximiser is started AT p_out.  Returns, an
    answered item, gain / (1e-6 |Q_j|) (to be held against C_Q) and the largest |p_out - p_end|_k / sqrt(2 C_Q 1e-6 |Q_j|
    (H^-1)_kk) over its free unknowns (against 1), H the matrix of the method at p_end; and the largest component of the
    maximiser's last step (its own convergence)."""
    pr = np.asarray(L["prior"] if prior is None else prior, np.float64)
    fr = L["free"]
    U = design(np.asarray(cs["theta"], np.float64))
    p_out = np.asarray(p_out, np.float64)
    gain, dev, last = [], [], 0.0
    for j in np.flatnonzero(answered(L)):
        f = fr[:, j]
        ev = lambda v: item_eval(cs["model"], U, cs["Dc"], L["n1"][j], L["n0"][j], v, f, pr[0, :, j], pr[1, :, j])   # noqa: E731
        q0 = ev(p_out[:, j])[0]
        p_end, step = maximise(ev, p_out[:, j], f)
        q1, g1, H1, _ = ev(p_end)
        Hi = np.linalg.inv(H1[np.ix_(f, f)])
        last = max(last, step)
        res = QTOL * abs(q1)
        gain.append(float((q1 - q0) / res))
        dev.append(float((np.abs(p_out[f, j] - p_end[f]) / np.sqrt(2 * C_Q * res * np.diag(Hi))).max()))
    return np.array(gain), np.array(dev), last


def rule2(cs, L, p_out):
    """Rule 2 for the output of ONE step from the launch's p0_near: |p_out - p64|_k / (eps32 (|H^-1| S)_k) an answered item and
    free unknown (against C_STEP), p64 the float64 one-step result; and the smallest acceptance margin of the float64 steps in
    units of the acceptance tolerance (>= 100 asserted on the CPU)."""
    pr = np.asarray(L["prior"], np.float64)
    fr = L["free"]
    U = design(np.asarray(cs["theta"], np.float64))
    st = {}
    p0 = np.asarray(L["p0_near"], np.float64)
    p64 = map_mstep(cs, L["n1"], L["n0"], p0, pr, 1, stats=st)
    out = []
    for j in np.flatnonzero(answered(L)):
        f = fr[:, j]
        _, _, H, S = item_eval(cs["model"], U, cs["Dc"], L["n1"][j], L["n0"][j], p0[:, j], f, pr[0, :, j], pr[1, :, j])
        scale = EPS32 * (np.abs(np.linalg.inv(H[np.ix_(f, f)])) @ S[f])
        out.append(float((np.abs(np.asarray(p_out, np.float64)[f, j] - p64[f, j]) / scale).max()))
    return np.array(out), p64, st


# ---- EM ----------------------------------------------------------------------------------------------------------------------
def em_start(cs):
    return {k: np.full(v.shape, EM_START[k], np.float32) for k, v in cs["start"].items()}


def em_iteration(cs, params, prior, newton=4, dtype=np.float64, stats=None):
    """(the leaves after one iteration from `params`, loglik, log prior) -- both of `params`; the M-step runs in `dtype`."""
    n1, n0, lk = tables(cs, params)
    p0 = pack(cs, params)
    p = map_mstep(cs, n1.astype(dtype), n0.astype(dtype), p0.astype(dtype), prior, newton, dtype, stats=stats)
    return unpack(cs, p.astype(np.float64)), lk, float(log_prior(p0, free_rows(cs), prior).sum())


_TRAJ = {}


def trajectory(name, iters, newton=4, dtype=np.float64):
    """The EM of a case from em_start, computed once and shared: (params after 0 .. iters iterations, loglik and logpost
    [0 .. iters - 1], stats)."""
    key = (name, newton, np.dtype(dtype).name)
    cs = case(name)
    if key not in _TRAJ:
        _TRAJ[key] = ([{k: v.astype(np.float64) for k, v in em_start(cs).items()}], [], [], {})
    ps, lks, lps, stats = _TRAJ[key]
    prior = prior_rows(cs)
    while len(lks) < iters:
        p, lk, lp = em_iteration(cs, ps[-1], prior, newton, dtype, stats)
        ps.append(p)
        lks.append(lk)
        lps.append(lk + lp)
    return ps[:iters + 1], lks[:iters], lps[:iters], stats


def posterior_sd(cs, params):
    """sqrt((H^-1)_kk) of every free unknown at `params` on the tables of `params`, as leaves (NaN where fixed or unanswered),
    and |Q_j| [J]: the scales of the end-to-end comparisons."""
    n1, n0, _ = tables(cs, params)
    pr = np.asarray(prior_rows(cs), np.float64)
    fr, p = free_rows(cs), pack(cs, params)
    U = design(np.asarray(cs["theta"], np.float64))
    sd, qs = np.full((ROWS, cs["J"]), np.nan), np.zeros(cs["J"])
    for j in np.flatnonzero((n1 + n0).sum(1) > 0):
        f = fr[:, j]
        q, _, H, _ = item_eval(cs["model"], U, cs["Dc"], n1[j], n0[j], p[:, j], f, pr[0, :, j], pr[1, :, j])
        sd[f, j] = np.sqrt(np.diag(np.linalg.inv(H[np.ix_(f, f)])))
        qs[j] = abs(q)
    return unpack(cs, sd), qs


# ---- a backend for the host tests --------------------------------------------------------------------------------------------
class MapOracleBackend(OracleBackend):
    """OracleBackend with the five grid entries fit_em(prior=) calls, in float64 numpy on CPU tensors: the tables are kept as the
    parameters they were built from (the image is never read), the posterior and the counts come from score_cases and
    count_cases, the M-step is map_mstep."""

    def grid_image_bytes(self, J, G):
        return 16

    def grid_counts_workspace(self, nb, J, G):
        return 1

    def grid_table_irt(self, cfg, theta, G, a, b, c_un, d_un, img):
        f8 = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
        params = {k: v for k, v in (("a", f8(a)), ("b", f8(b)), ("c", f8(c_un)), ("d", f8(d_un))) if v is not None}
        self._tab = (CODE_MODEL[cfg.model], f8(theta), params, cfg.Dc)

    def _ll(self, y):
        model, theta, params, Dc = self._tab
        return sc.irt_grid_loglik(model, theta, params, Dc, y.cpu().numpy())

    def grid_posterior(self, y, rows, nb, J, G, D, img, logw, coord, loglik, mean, sd, argmax):
        assert rows is None
        post = sc.grid_posterior(self._ll(y), logw.cpu().numpy(), coord.cpu().numpy())
        loglik.copy_(torch.from_numpy(post["loglik"].astype(np.float32)))

    def grid_counts(self, y, rows, nb, J, G, img, logw, loglik, n1, n0, mass, ws):
        t = cc.counts(self._ll(y), logw.cpu().numpy(), y.cpu().numpy())
        for dst, k in ((n1, "n1"), (n0, "n0"), (mass, "mass")):
            dst.copy_(torch.from_numpy(t[k].astype(np.float32)))

    def grid_mstep_irt_map(self, cfg, theta, G, n1, n0, a_free, a, b, c_un, d_un, prior, newton, lprior=None):
        model, D, J = CODE_MODEL[cfg.model], cfg.D, cfg.J
        cs = {"model": model, "D": D, "J": J, "Dc": cfg.Dc, "theta": theta.cpu().numpy(),
              "a_free": None if a is None else (np.ones((D, J), bool) if a_free is None else a_free.cpu().numpy() != 0)}
        leaves = {k: t for k, t in (("a", a), ("b", b), ("c", c_un), ("d", d_un)) if t is not None}
        p0 = pack(cs, {k: t.cpu().numpy() for k, t in leaves.items()})
        pr = prior.cpu().numpy().astype(np.float64)
        if lprior is not None:
            lprior.copy_(torch.from_numpy(log_prior(p0, free_rows(cs), pr).astype(np.float32)))
        out = unpack(cs, map_mstep(cs, n1.cpu().numpy(), n0.cpu().numpy(), p0, pr, newton))
        for k, t in leaves.items():
            t.copy_(torch.from_numpy(out[k].astype(np.float32)).reshape(t.shape))
