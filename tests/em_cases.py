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
g = s = 0.1.

On all of these the oracle's Newton takes full steps only.  STEP_CASES are the inputs that leave that path: synthetic tables
(step_tables: closed form, no seed, no training) from starts far from the maximiser -- capped steps, halved steps, both, two
halvings in a step, halvings in two steps, nodes clamped at the start, masked loadings in two and three dimensions, constant
items that walk to the clamp and stop on the zero pivot -- and ordinary items on grids either side of the kernel's lane
boundaries.  A converged result hides a wrong path, so every launch is compared at every Newton budget of step_budgets().
newton_mstep's trace records what was decided and by what margin, and its keywords build the wrong variants the cases must
tell apart (tests/test_em_host.py).

"All nine trials rejected" was searched for and not found: in 9 000 random starts (2PL, D = 1 .. 3, Dc = 1 and 1.702, a in
[-6, 15], b in [-20, 20], truths with a in [-1, 6] and b in [-6, 6], constant items among them) the oracle and its float32 run
halve at most twice in a step -- Q is concave and the Newton direction ascends.  (With log P formed as z - softplus(z), as
_item_eval and the kernel had it before gm_cell, the float32 run did reject all nine, on items with Dc |b| >= 7 at the
maximiser: rounding, not step control.  The launch step_2pl_easy_items keeps those inputs; docs/NOTEBOOK.md.)"""
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
def _item_eval(U, c1, c0, p, Dc, zl, leak=False, info=None):
    z = Dc * (U @ p)
    zc = np.clip(z, -zl, zl)
    inside = zc == z
    if info is not None:                                                # (the trace: clamped nodes, nearest approach to +-ZL)
        info["clamped"].append(int((~inside).sum()))
        info["edge"] = min(info["edge"], float(np.abs(np.abs(z.astype(np.float64)) - ZL).min()))
    if leak:                                                            # a wrong variant: clamped nodes enter gradient and curvature
        inside = np.ones_like(inside)
    e = np.exp(-np.abs(zc))                                             # log P, log(1 - P), P and 1 - P from positive terms:
    lse = np.log1p(e)                                                   # no z - softplus(z), no 1 - P (gm_cell of the kernel)
    sg = np.where(zc >= 0, 1 / (1 + e), e / (1 + e)).astype(U.dtype)
    sn = np.where(zc >= 0, e / (1 + e), 1 / (1 + e)).astype(U.dtype)
    q = (c1 * (np.minimum(zc, 0) - lse) + c0 * (np.minimum(-zc, 0) - lse)).sum(dtype=U.dtype)
    r = np.where(inside, c1 * sn - c0 * sg, 0).astype(U.dtype)
    w = np.where(inside, (c1 + c0) * sg * sn, 0).astype(U.dtype)
    return q, Dc * (U.T @ r), Dc * Dc * ((U * w[:, None]).T @ U)


def _pivots(A):
    """The pivots of the Cholesky factorisation of A in A's dtype, up to and including the first that is not positive."""
    n = A.shape[0]
    L = np.zeros_like(A)
    out = []
    for i in range(n):
        for l in range(i + 1):
            v = A[i, l] - (L[i, :l] * L[l, :l]).sum(dtype=A.dtype)
            if l == i:
                out.append(float(v))
                if not v > 0:
                    return out
                L[i, i] = np.sqrt(v)
            else:
                L[i, l] = v / L[l, l]
    return out


def newton_mstep(model, theta, Dc, n1, n0, a, b, free, newton, dtype=np.float64, stats=None, trace=None, halving=0.5,
                 cap=STEP_CAP, halvings=HALVINGS, qtol=QTOL, leak=False, cap_rescales=True):
    """New (a [D][J] or None, b [1][J]) in `dtype`; stats (a dict, optional) counts halvings, capped steps, stopped items.
    trace (a list, optional) receives one record for every item that somebody answered: {"item", "steps": [{"capped",
    "m_over_cap", "margins": (qt - (q - qtol |q|)) / |q| of every trial, the last one the accepted, "rises": qt - q of the same,
    "pivots", "p": the unknowns after the step}], "stop": None / "pivot" / "nonfinite" / "halvings", "stop_step": the step it
    happened in, "clamped": the number of clamped nodes of every evaluation, "edge": the smallest | |z| - ZL | of any node in
    any evaluation}.
    The keywords after it are the constants of the kernel; other values build the wrong variants of test_em_host.py (leak: the
    clamped nodes enter gradient and curvature; cap_rescales = False: every component is clipped to the cap on its own)."""
    dt = np.dtype(dtype).type
    theta = np.asarray(theta, dtype)
    G, D = theta.shape
    n1, n0 = np.asarray(n1, dtype), np.asarray(n0, dtype)
    J = n1.shape[0]
    U = np.concatenate([np.ones((G, 1), dtype), theta], axis=1)
    b = np.array(b, dtype).reshape(1, J)
    a = None if model == "irt_1pl" else np.array(a, dtype).reshape(D, J)
    Dc, zl, qtol, cap, halving = dt(Dc), dt(ZL), dt(qtol), dt(cap), dt(halving)
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
        rec = None
        if trace is not None:
            rec = {"item": j, "steps": [], "stop": None, "stop_step": None, "clamped": [], "edge": np.inf}
            trace.append(rec)
        q, g, H = _item_eval(U, c1, c0, p, Dc, zl, leak, rec)
        for it in range(newton):
            A = H[np.ix_(fr, fr)]
            step = None
            if rec is not None:
                step = {"capped": False, "m_over_cap": 0.0, "margins": [], "rises": [], "pivots": _pivots(A), "p": None}
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                st["stopped"] += 1
                if rec is not None:
                    rec["stop"], rec["stop_step"], rec["stop_pivots"] = "pivot", it, step["pivots"]
                break
            d = np.zeros_like(p)
            d[fr] = np.linalg.solve(L.T, np.linalg.solve(L, g[fr])).astype(dtype)
            m = np.abs(d).max()
            if not np.isfinite(m):
                st["stopped"] += 1
                if rec is not None:
                    rec["stop"], rec["stop_step"] = "nonfinite", it
                break
            t = dt(1)
            if m > cap:
                if cap_rescales:
                    t = cap / m
                else:
                    d = np.clip(d, -cap, cap)
                st["capped"] += 1
            if step is not None:
                step["capped"], step["m_over_cap"] = bool(m > cap), float(m / cap)
                rec["steps"].append(step)
            moved = False
            for _h in range(halvings + 1):
                pt = (p + t * d).astype(dtype)
                qt, gt, Ht = _item_eval(U, c1, c0, pt, Dc, zl, leak, rec)
                if step is not None:
                    step["margins"].append(float((qt - (q - qtol * abs(q))) / abs(q)))  # (q < 0: log1p(eps32) a node at the clamp)
                    step["rises"].append(float(qt - q))
                if qt >= q - qtol * abs(q):
                    p, q, g, H, moved = pt, qt, gt, Ht, True
                    break
                st["halvings"] += 1
                t = t * halving
            if step is not None:
                step["p"] = p.copy()
            if not moved:
                st["stopped"] += 1
                if rec is not None:
                    rec["stop"], rec["stop_step"] = "halvings", it
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


# ---- the M-step's step control: synthetic tables -----------------------------------------------------------------------------
def step_tables(theta, logw, Dc, N, truth):
    """The tables of one synthetic item in float64: n1 = N w sigma(z), n0 = N w sigma(-z) with z = Dc (theta . a + b) of
    truth = (a, b), or everything in n1 / n0 for truth = "correct" / "wrong".  w is the grid's prior weight times
    1 + 0.25 sin(1.7 sum(theta) + 0.4), normalised: no table is symmetric about theta = 0, and so none about b = 0."""
    theta = np.asarray(theta, np.float64)
    w = np.exp(np.asarray(logw, np.float64)) * (1 + 0.25 * np.sin(1.7 * theta.sum(1) + 0.4))
    w = N * w / w.sum()
    if truth == "correct":
        return w, np.zeros_like(w)
    if truth == "wrong":
        return np.zeros_like(w), w
    a, b = truth
    z = Dc * (theta @ np.asarray(a, np.float64).reshape(-1) + b)
    return w * vo.sigmoid(z), w * vo.sigmoid(-z)


def _it(name, truth, a0, b0, free=None, kind="finite", path=()):
    return {"name": name, "truth": truth, "a0": a0, "b0": b0, "free": free, "kind": kind, "path": list(path)}


# One entry = one launch: the items share model, D, Dc and grid.  kind: "finite" (a finite maximiser: a and b compared
# absolutely), "clamp" (a constant 1PL item: walks until every node is clamped and the pivot is zero; b compared relative to
# its size), "contract" (a constant 2PL item: near-singular on the way, no two arithmetics agree; the documented contract is
# asserted instead of values).  J is never a multiple of 4: waves that stop early share a workgroup with waves that go on.
# path: (capped, halvings) of the item's first Newton steps in the float64 oracle, the path its name stands for; every later
# step is a full Newton step accepted at once (tests/test_em_host.py::test_step_case_conditions asserts both).
STEP_CASES = [
    {"name": "step_2pl_dc1", "model": "irt_2pl", "D": 1, "Dc": 1.0, "nodes": 41, "span": 6.0, "items": [
        _it("ordinary", ([1.2], 0.3), [1.0], 0.0),
        _it("cap", ([1.2], 0.3), [0.2], -3.0, path=[(1, 0)]),
        _it("halve", ([1.2], 0.3), [3.0], 0.0, path=[(0, 1)]),
        _it("cap_and_halve_clamped_start", ([2.0], 1.0), [4.0], 0.0, path=[(1, 1)]),      # a = 4 on [-6, 6]: clamped nodes at the start
        _it("cap_then_halve", ([1.2], 0.3), [6.0], -4.0, path=[(1, 0), (0, 1)]),
        _it("cap3", ([1.2], 0.3), [12.0], -8.0, path=[(1, 0), (1, 0), (1, 0)]),
        _it("all_correct", "correct", [1.0], 0.0, kind="contract"),
        _it("all_wrong_cap", "wrong", [2.0], 2.0, kind="contract", path=[(1, 0)]),
        _it("cap_b", ([0.8], -0.7), [0.1], 4.0, path=[(1, 0)]),
    ]},
    {"name": "step_2pl_dc1702", "model": "irt_2pl", "D": 1, "Dc": 1.702, "nodes": 41, "span": 6.0, "items": [
        _it("ordinary", ([1.0], 0.9), [1.0], 0.0),
        _it("cap_halve2", ([1.7], -2.2), [-0.8], -1.9, path=[(1, 2)]),
        _it("cap_then_halve2", ([1.0], -2.1), [-2.4], -6.3, path=[(1, 0), (0, 2)]),
        _it("halve_in_two_steps", ([1.2], -1.0), [-0.3], -1.8, path=[(1, 1), (0, 1)]),
        _it("cap_halve_twice", ([1.4], -3.3), [-0.3], -6.6, path=[(1, 1), (1, 1)]),
        _it("halve2", ([0.9], -3.9), [-0.1], -4.0, path=[(0, 2)]),
    ]},
    # very easy and very hard items: Dc |b| of 8 to 10 at the maximiser, P > 0.9997 or < 0.0003 at theta = 0.  With log P formed as
    # z - softplus(z) the float32 Q of such an item is rounded at 1e-4 of its size, every trial near the maximiser looks like a
    # fall, and the item stopped on its halvings up to 1.5e-2 short (the first item: a 6.9e-3, b 1.5e-2 on an MI355X)
    {"name": "step_2pl_easy_items", "model": "irt_2pl", "D": 1, "Dc": 1.702, "nodes": 41, "span": 6.0, "items": [
        _it("easy_from_far", ([0.64], 5.88), [-2.78], -7.18, path=[(1, 0), (1, 0)]),
        _it("easy_negative_a", ([-0.33], 5.56), [7.31], -8.11, path=[(1, 0), (1, 0)]),
        _it("easy_from_one", ([1.0], 5.5), [1.0], 0.0),
        _it("hard_from_one", ([0.8], -5.0), [1.0], 0.0),
        _it("easy_steep", ([1.06], 4.77), [-5.69], 5.34, path=[(1, 0)]),
    ]},
    {"name": "step_1pl_dc1702", "model": "irt_1pl", "D": 1, "Dc": 1.702, "nodes": 41, "span": 6.0, "items": [
        _it("ordinary", ([1.0], 0.4), None, 0.0),
        _it("cap", ([1.0], 0.4), None, -4.0, path=[(1, 0)]),
        _it("cap3", ([1.0], 0.4), None, 12.0, path=[(1, 0), (1, 0), (1, 0)]),
        _it("all_correct", "correct", None, 0.0, kind="clamp"),
        _it("all_correct_cap3", "correct", None, -12.0, kind="clamp", path=[(1, 0), (1, 0), (1, 0)]),       # stops past step 25
        _it("all_wrong_cap", "wrong", None, 5.0, kind="clamp", path=[(1, 0)]),
        _it("all_wrong_clamped_start", "wrong", None, -4.0, kind="clamp"),
        _it("all_correct_clamped_start", "correct", None, 12.0, kind="clamp"),
        _it("cap2", ([1.0], 0.4), None, 8.0, path=[(1, 0), (1, 0)]),
    ]},
    {"name": "step_1pl_dc1", "model": "irt_1pl", "D": 1, "Dc": 1.0, "nodes": 41, "span": 6.0, "items": [
        _it("ordinary", ([1.0], 0.4), None, 0.0),
        _it("all_correct", "correct", None, 0.0, kind="clamp"),
        _it("cap", ([1.0], 0.4), None, 5.0, path=[(1, 0)]),
        _it("all_wrong_cap2", "wrong", None, 8.0, kind="clamp", path=[(1, 0), (1, 0)]),
        _it("cap3", ([1.0], 0.4), None, -12.0, path=[(1, 0), (1, 0), (1, 0)]),
    ]},
    {"name": "step_2pl_d2_masked", "model": "irt_2pl", "D": 2, "Dc": 1.0, "nodes": 11, "span": 4.0, "items": [
        _it("ordinary", ([1.0, 0.6], 0.2), [0.5, 0.5], 0.0, [1, 1]),
        _it("cap_halve_fixed_0.7", ([1.4, 0.7], 1.1), [3.3, 0.7], 3.2, [1, 0], path=[(1, 1)]),
        _it("halve_fixed_0.7", ([0.7, 1.7], 1.9), [0.7, 0.0], 2.9, [0, 1], path=[(0, 1)]),
        _it("cap_halve_fixed_0", ([0.0, 1.7], 1.5), [0.0, 3.4], 4.1, [0, 1], path=[(1, 1)]),
        _it("cap_fixed_0.7", ([0.7, 1.9], -0.2), [0.7, -0.7], 3.7, [0, 1], path=[(1, 0)]),
        _it("halve_fixed_0", ([1.6, 0.0], -1.2), [0.5, 0.0], -2.9, [1, 0], path=[(0, 1)]),
    ]},
    {"name": "step_2pl_d3_masked", "model": "irt_2pl", "D": 3, "Dc": 1.0, "nodes": 5, "span": 4.0, "items": [
        _it("ordinary", ([1.0, 0.6, 0.8], 0.2), [0.5, 0.5, 0.5], 0.0, [1, 1, 1]),
        _it("cap_halve_one_fixed", ([1.9, 0.7, 1.3], 0.9), [3.8, 0.7, 3.6], 2.6, [1, 0, 1], path=[(1, 1)]),
        _it("halve_one_fixed", ([0.7, 1.8, 1.5], 1.9), [0.7, 0.8, 2.8], 2.3, [0, 1, 1], path=[(0, 1)]),
        _it("cap_halve_two_fixed", ([1.9, 0.7, 0.7], 1.5), [3.9, 0.7, 0.7], 1.1, [1, 0, 0], path=[(1, 1)]),
        _it("cap_one_fixed_0", ([1.4, 1.7, 0.0], -1.2), [3.7, 3.9, 0.0], 1.9, [1, 1, 0], path=[(1, 0)]),
    ]},
]
# Ordinary converging items on grids either side of the lane boundaries of the kernel (64 lanes, at most GM_NK = 16 nodes a lane)
for _D, _nodes, _span in ((1, 64, 6.0), (1, 65, 6.0), (2, 31, 5.0), (3, 10, 4.0), (2, 32, 5.0)):
    STEP_CASES.append({"name": "lanes_d%d_g%d" % (_D, _nodes ** _D), "model": "irt_2pl", "D": _D, "Dc": 1.0, "nodes": _nodes,
                       "span": _span, "items": [
        _it("ordinary_a", ([1.2, 0.6, 0.9][:_D], 0.3), [0.5] * _D, 0.0, [1] * _D),
        _it("ordinary_b", ([0.7, 1.1, 0.5][:_D], -0.8), [0.5] * _D, 0.0, [1] * _D),
        _it("ordinary_c", ([1.5, 0.4, 0.8][:_D], 1.0), [1.0] * _D, 0.5, [1] * _D),
    ]})
STEP_LATE = 25                      # the budget at which a finite item has converged
STEP_MAX = 64                       # GM_MAX_NEWTON: run where an item stops later than step 25

_STEP = {}


def step_case(spec):
    """The launch of a STEP_CASES entry, built once: theta, the float32 tables [J][G] (what the kernel is fed, and the oracle),
    the float32 start a0 [D][J] (None for 1PL) and b0 [1][J], free [D][J] bool (None for 1PL), the items' kinds."""
    key = spec["name"]
    if key not in _STEP:
        from vipsy_amd.engine import score_grid
        theta, logw = score_grid(spec["D"], spec["nodes"], spec["span"])
        tabs = [step_tables(theta, logw, spec["Dc"], 2000.0, it["truth"]) for it in spec["items"]]
        one = spec["model"] == "irt_1pl"
        D = spec["D"]
        _STEP[key] = {
            "theta": theta, "J": len(tabs), "G": theta.shape[0],
            "n1": np.stack([t[0] for t in tabs]).astype(np.float32), "n0": np.stack([t[1] for t in tabs]).astype(np.float32),
            "a0": None if one else np.array([it["a0"] for it in spec["items"]], np.float32).T.reshape(D, -1).copy(),
            "b0": np.array([[it["b0"] for it in spec["items"]]], np.float32),
            "free": None if one else np.array([[1] * D if it["free"] is None else it["free"] for it in spec["items"]], bool).T.copy(),
            "kinds": [it["kind"] for it in spec["items"]], "names": [it["name"] for it in spec["items"]]}
    return _STEP[key]


_STEP_RUN = {}


def step_run(spec, newton, dtype=np.float64, cache=True, **knobs):
    """(a, b, trace) of newton_mstep on the launch; the unmutated runs are computed once and shared (never modified), unless
    cache = False; a run with knobs is never kept."""
    key = (spec["name"], newton, np.dtype(dtype).name)
    keep = cache and not knobs
    if keep and key in _STEP_RUN:
        return _STEP_RUN[key]
    c = step_case(spec)
    tr = []
    a, b = newton_mstep(spec["model"], c["theta"], spec["Dc"], c["n1"], c["n0"], c["a0"], c["b0"], c["free"], newton,
                        dtype=dtype, trace=tr, **knobs)
    if keep:
        _STEP_RUN[key] = (a, b, tr)
    return a, b, tr


def step_decisions(rec, upto=None):
    """What the step control decided for one item: ((capped, halvings) of each Newton step, stop, the step it stopped in)."""
    steps = rec["steps"] if upto is None else rec["steps"][:upto]
    return [(s["capped"], len(s["margins"]) - 1) for s in steps], rec["stop"], rec["stop_step"]


def step_last_special(rec):
    """The number of Newton steps up to and including the item's last capped or halved one (0: none)."""
    return max([i + 1 for i, (c, h) in enumerate(step_decisions(rec)[0]) if c or h] or [0])


def step_budgets(spec):
    """The `newton` of the launches of an entry: every budget from 1 to one past the last capped or halved step of any of its
    items, then 25 -- and 64 where an item of the oracle stops later than that."""
    _, _, tr = step_run(spec, STEP_MAX)
    last = max(step_last_special(r) for r in tr)
    out = list(range(1, last + 2)) + [STEP_LATE]
    if any(r["stop_step"] is not None and r["stop_step"] >= STEP_LATE for r in tr):
        out.append(STEP_MAX)
    return sorted(set(out))


def step_errors(spec, a, b, a64, b64, tol):
    """The rule of the comparisons of a launch, as error / tolerance an item (> 1 fails): `tol` absolutely on a and b of a
    finite item, tol * max(1, |b|) on a clamp item; None for a contract item (no values compared)."""
    out = []
    for j, kind in enumerate(step_case(spec)["kinds"]):
        if kind == "contract":
            out.append(None)
            continue
        e = abs(float(b[0, j]) - b64[0, j])
        if a64 is not None:
            e = max(e, float(np.abs(np.asarray(a, np.float64)[:, j] - a64[:, j]).max()))
        out.append(e / (tol * (max(1.0, abs(b64[0, j])) if kind == "clamp" else 1.0)))
    return out


# ---- fit_em's stopping rule ----------------------------------------------------------------------------------------------------
# (case, tol): tol lies between two consecutive relative rises of the oracle's trajectory that differ by a factor >= 4, each at
# least 5 ROW_TOL from it (tests/test_em_host.py::test_converged_cases_are_decided checks it): the loglik the GPU returns is
# held to ROW_TOL relatively, so its rises cannot fall on the other side of tol.
CONVERGED = [(IRT_EM[0], 3e-2), (CDM_EM[0], 3e-4)]


def stop_iteration(lks, tol):
    """The number of iterations after which fit_em's rule stops on the log-likelihoods lks (None: not within them)."""
    for k in range(1, len(lks)):
        if lks[k] - lks[k - 1] <= tol * abs(lks[k - 1]):
            return k + 1
    return None
