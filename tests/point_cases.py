"""The float64 oracle, the cases and the rules of the point-estimate tests (tests/test_point_host.py on the CPU,
tests/test_gpu_point.py on the GPU): the ML, MAP and Warm's WLE estimate of a person by Fisher scoring.

The oracle holds the formulas and nothing of the kernel's path.  With z = Dc (theta . a + b) (1PL: a = 1), P = c + (d - c)
sigmoid(z), Q = 1 - P (float64: harmless), P_z = (d - c) sigmoid(z) sigmoid(-z), over the observed cells (y < 2):

    g_d  = Dc   sum_j a_jd (y_j ? Q_j : -P_j) P_z / (P_j Q_j)
    I_de = Dc^2 sum_j a_jd a_je P_z^2 / (P_j Q_j)
    J    = sum_j P'_j P''_j / (P_j Q_j),  P' = Dc a P_z,  P'' = Dc^2 a^2 (d - c) sigmoid(z) sigmoid(-z) (sigmoid(-z) - sigmoid(z))

ml: g, M = I;  map: g - theta, M = I + 1;  wle (D = 1): g + J / (2 I), M = I.  For a theta_hat handed to it, evaluate() gives g, M,
s = M^-1 g and the yardstick u_d = 2^-23 (sum_e |M^-1|_de sum_j |t_je| + |theta_hat_d|), t_je the terms summed into g_e (with |J / 2 I|
for wle and |theta_e| for map among them).  fisher64() is the method in float64 (the step M^-1 g capped at 1 a coordinate, theta
clamped to +-bound, the five ways to stop): the oracle's own root is what it reaches from the oracle's EAP in 60 steps.

The rules (C: POINT_C), for a float32 theta_hat TAKEN AS IT IS and evaluated in float64 -- they do not depend on the path:
  converged   |s_d| <= tol + C u_d for every d; where the objective is concave (1PL / 2PL) and the oracle converged too, also
              |theta_hat_d - root_d| <= tol + C u_d;
  info        |I - I64(theta_hat)| <= C 2^-23 sum |terms|, every status but empty;
  at_bound    a coordinate of theta_hat sits on +-bound exactly and the float64 s points outward there; under ml these are exactly
              the persons the oracle's own run ends at the bound;
  empty       theta_hat NaN, info 0, iterations 0, exactly on the persons without an observed cell (checked against y).
Caps (conditions on the cases, not measurements; tests/test_point_host.py holds the float64 method to them on the CPU): with
tol = 1e-6 and max_iter = 64 at most MAX_ITER_CAP of a case's persons with >= 5 answers may end in max_iter, and none may end
singular on a 2PL case."""
import numpy as np

from oracle import vi_oracle as vo
from tests import score_cases as sc

U = 2.0 ** -23
# The constant of the rules: the next power of two above twice the largest ratio measured on one MI355X (the convention of
# fit_cases.FIT_C: the factor two covers another summation order on another build).  Over every case, method and shape of
# tests/test_gpu_point.py, at the ABI and end to end, under both instruction schedules, the largest ratio is 1.97 (the information
# of a person of pt_3pl_n257_j33 under wle: |I - I64| against 2^-23 times the sum of its 33 terms); the largest of the s and root
# rules is 0.23 -- a converged theta_hat sits within tol of the float64 root of the estimating function almost everywhere.
# 2 x 1.97 < 4.  The float32 numpy restatement of the method (restated_f32, tests/test_point_host.py) costs 2.27 by itself (the
# information again, pt_2pl_d3_n97_j130 under ml; numpy's pairwise float32 sum against the kernel's lane-and-butterfly order).
POINT_C = 4.0
MEASURED_MAX_RATIO = 1.97
RESTATED_MAX_RATIO = 2.27
TOL, MAX_ITER, STEP_CAP = 1e-6, 64, 1.0
MAX_ITER_CAP = 0.01
MIN_ITEMS = 5
METHODS = ("ml", "map", "wle")
STATUS = ("converged", "at_bound", "max_iter", "singular", "empty")
CONVERGED, AT_BOUND, MAX_ITERS, SINGULAR, EMPTY = range(5)

# name, N, J, model, D, Dc, nodes per dimension, missing rate, slope range, seed  (score_cases.irt_case draws them).
# Items: 1, 31 (a partial tile of 64), 33, 130 (three tiles), 1 024 (the limit, 64 persons, 95 % missing); persons 1 .. 97 of the
# first case go through `rows` (tests/test_gpu_point.py).  The asymptote cases are as large as the caps ask: the capped step has no
# halving, and the planted all-wrong / all-correct row of a 3PL / 4PL case can alternate between two points for ever (float64 and
# kernel alike) -- one person of a case, so a case has more than a hundred persons; a 31-item 4PL case loses 1.2 - 1.4 % of its
# persons that way whatever its size and is not among them (its 4PL items are the 130 of pt_4pl_n129_j130).
CASES = [
    ("pt_2pl_n97_j31", 97, 31, "irt_2pl", 1, 1.0, 61, 0.20, (0.5, 1.5), 51),
    ("case3_1pl_j130", 100, 130, "irt_1pl", 1, 1.702, 41, 0.10, None, 13),            # score_cases' own: Dc = 1.702
    ("pt_3pl_n257_j33", 257, 33, "irt_3pl", 1, 1.0, 61, 0.0, (0.5, 1.5), 53),
    ("pt_4pl_n129_j130", 129, 130, "irt_4pl", 1, 1.0, 61, 0.20, (0.5, 1.5), 54),
    ("pt_2pl_n33_j1", 33, 1, "irt_2pl", 1, 1.0, 61, 0.20, (0.5, 1.5), 55),
    ("pt_2pl_n64_j1024_sparse", 64, 1024, "irt_2pl", 1, 1.0, 61, 0.95, (0.5, 1.5), 56),
    ("pt_2pl_d2_n32_j40", 32, 40, "irt_2pl", 2, 1.0, 21, 0.0, (0.5, 1.5), 57),
    ("pt_2pl_d3_n97_j130", 97, 130, "irt_2pl", 3, 1.0, 9, 0.20, (0.5, 1.5), 58),
    ("pt_3pl_d2_n129_j130", 129, 130, "irt_3pl", 2, 1.0, 21, 0.20, (0.5, 1.5), 59),
]
IDS = [c[0] for c in CASES]
CASE_METHODS = [(c, m) for c in CASES for m in METHODS if m != "wle" or c[4] == 1]
CASE_METHOD_IDS = ["%s-%s" % (c[0], m) for c, m in CASE_METHODS]
SANITY = ("pt_sanity_2pl_n4096_j40", 4096, 40, "irt_2pl", 1, 1.0, 61, 0.0, (0.5, 1.5), 60)
SANITY_SHIFT = 1.0                                      # the mean of its thresholds: an easy test (see sanity_case)
NOBODY, ALL_CORRECT, ALL_WRONG = 0, 1, 2                # the planted persons of every case

_CASES, _EAP, _ROOT = {}, {}, {}


def case_of(case):
    """The case, built once and shared (callers must not modify it): score_cases.irt_case's draw with three planted persons -- 0
    answered nothing, 1 answered everything correctly, 2 everything wrongly (the one-item case keeps its missing cells)."""
    key = case[0]
    if key not in _CASES:
        cs = sc.irt_case(case)
        y = cs["y"]
        y[NOBODY] = 255
        y[ALL_CORRECT] = 1
        y[ALL_WRONG] = 0
        _CASES[key] = cs
    return _CASES[key]


def sanity_case():
    """4 096 persons x 40 items, 2PL, nothing missing, with `theta` [N][1], the values the responses were simulated from.  The
    thresholds are drawn around SANITY_SHIFT, not 0: on a test centred on the population the outward biases of the ML estimate
    in the two tails cancel in the plain mean of theta_hat - theta over |theta| > 1.5, and the comparison of that mean between
    ml and wle would be a coin flip; on an easy test the upper tail, where the information runs out, does not cancel."""
    key = SANITY[0]
    if key not in _CASES:
        name, N, J, model, D, Dc, nodes, missing, slopes, seed = SANITY
        rng = np.random.RandomState(seed)
        p = {"a": rng.uniform(slopes[0], slopes[1], size=(D, J)).astype(np.float32),
             "b": rng.normal(SANITY_SHIFT, 1.0, size=(1, J)).astype(np.float32)}
        theta = rng.normal(size=(N, D))
        y = (rng.uniform(size=(N, J)) < vo.sigmoid(Dc * (theta @ p["a"].astype(np.float64) + p["b"]))).astype(np.uint8)
        _CASES[key] = {"name": name, "N": N, "J": J, "model": model, "D": D, "Dc": Dc, "nodes": nodes, "span": sc.SPAN, "y": y,
                       "params": p, "theta": theta}
    return _CASES[key]


def sanity_stats(cs, ml, wle):
    """The figures of the sanity case from two results {theta_hat, status, info as (n, 1, 1)}: the mean of theta_hat - theta over
    the persons with |theta| > 1.5 and status converged, for ml and for wle (each over its own such persons); the mean OUTWARD
    error (theta_hat - theta) sign(theta) over the persons both converged for; and the wle's 1 - mean(1 / I) / var(theta_hat) over
    its converged persons (var with n - 1), in float64."""
    th = cs["theta"][:, 0]
    far = np.abs(th) > 1.5
    cm, cw = far & (np.asarray(ml["status"]) == CONVERGED), far & (np.asarray(wle["status"]) == CONVERGED)
    em, ew = np.asarray(ml["theta_hat"], np.float64)[:, 0] - th, np.asarray(wle["theta_hat"], np.float64)[:, 0] - th
    both = cm & cw
    conv = np.asarray(wle["status"]) == CONVERGED
    se2 = 1.0 / np.asarray(wle["info"], np.float64)[conv, 0, 0]
    return {"mean_ml": float(em[cm].mean()), "mean_wle": float(ew[cw].mean()), "n_ml": int(cm.sum()), "n_wle": int(cw.sum()),
            "out_ml": float((em * np.sign(th))[both].mean()), "out_wle": float((ew * np.sign(th))[both].mean()),
            "reliability": float(1.0 - se2.mean() / np.asarray(wle["theta_hat"], np.float64)[conv, 0].var(ddof=1)),
            "n_converged": int(conv.sum())}


def eap_of(case):
    """The oracle's EAP of a case (score_cases.irt_oracle), float64 [N][D], computed once."""
    if case[0] not in _EAP:
        _EAP[case[0]] = sc.irt_oracle(sanity_case() if case[0] == SANITY[0] else case_of(case))["mean"]
    return _EAP[case[0]]


def concave(cs):
    return cs["model"] in ("irt_1pl", "irt_2pl")


# ---- the formulas ------------------------------------------------------------------------------------------------------------
def _params(cs, params=None):
    p = cs["params"] if params is None else params
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    J = cs["J"]
    a = f8(p["a"]).reshape(cs["D"], J) if cs["model"] != "irt_1pl" else np.ones((1, J))
    b = f8(p["b"]).reshape(1, J)
    lo = vo.sigmoid(f8(p["c"])).reshape(1, J) if cs["model"] in ("irt_3pl", "irt_4pl") else np.zeros((1, J))
    hi = vo.sigmoid(f8(p["d"])).reshape(1, J) if cs["model"] == "irt_4pl" else np.ones((1, J))
    return a, b, lo, hi


def evaluate(cs, theta, method, y=None, params=None):
    """g, M, I (and s = M^-1 g, the yardstick u, the sums of the absolute terms) at theta [n][D], float64.  `pd`: M is positive
    definite (s, u and minv are NaN where it is not)."""
    y = cs["y"] if y is None else y
    th = np.asarray(theta, np.float64).reshape(len(y), cs["D"])
    a, b, lo, hi = _params(cs, params)
    Dc, D = float(cs["Dc"]), cs["D"]
    z = Dc * (th @ a + b)
    sg, sn = vo.sigmoid(z), vo.sigmoid(-z)
    dmc = hi - lo
    P = lo + dmc * sg
    Q = (1.0 - hi) + dmc * sn
    pz = dmc * sg * sn
    m, one = y < 2, y == 1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.where(m, np.where(one, Q, -P) * pz / (P * Q), 0.0)                  # [n][J]
        w = np.where(m, pz * pz / (P * Q), 0.0)
    g = Dc * t @ a.T
    g_abs = Dc * np.abs(t) @ np.abs(a).T
    info = Dc * Dc * np.einsum("nj,dj,ej->nde", w, a, a)
    info_abs = Dc * Dc * np.einsum("nj,dj,ej->nde", w, np.abs(a), np.abs(a))
    M = info.copy()
    if method == "map":
        g = g - th
        g_abs = g_abs + np.abs(th)
        M = M + np.eye(D)[None]
    elif method == "wle":
        assert D == 1
        p1 = Dc * a * pz
        p2 = Dc * Dc * a * a * pz * (sn - sg)
        with np.errstate(divide="ignore", invalid="ignore"):
            Jw = np.where(m, p1 * p2 / (P * Q), 0.0).sum(1)
            half = np.where(info[:, 0, 0] > 0, Jw / (2.0 * info[:, 0, 0]), np.nan)
        g = g + half[:, None]
        g_abs = g_abs + np.abs(half)[:, None]
    n = len(y)
    pd = np.isfinite(M).all((1, 2)) & np.isfinite(g).all(1)
    for d in range(D):
        pd &= np.linalg.det(np.where(pd[:, None, None], M, np.eye(D))[:, :d + 1, :d + 1]) > 0
    minv = np.full((n, D, D), np.nan)
    if pd.any():
        minv[pd] = np.linalg.inv(M[pd])
    s = np.einsum("nde,ne->nd", minv, g)
    u = U * (np.einsum("nde,ne->nd", np.abs(minv), g_abs) + np.abs(th))
    return {"g": g, "M": M, "info": info, "info_abs": info_abs, "s": s, "u": u, "pd": pd, "minv": minv, "n_obs": m.sum(1)}


def fisher64(cs, method, theta0, y=None, params=None, max_iter=60, tol=1e-12, bound=sc.SPAN, cap=STEP_CAP, dtype=np.float64,
             evaluate_fn=None):
    """The method in float64 from theta0 [n][D]: returns theta (the last point evaluated), status, iterations and the info at
    theta.  A person stops as the kernel's documentation says: converged (max |s| <= tol, the step not taken), at_bound (two
    consecutive evaluations on +-bound with s pointing outward), max_iter, singular, empty."""
    y = cs["y"] if y is None else y
    ev = evaluate if evaluate_fn is None else evaluate_fn
    n, D = len(y), cs["D"]
    th = np.clip(np.asarray(theta0, dtype).reshape(n, D), -bound, bound).astype(dtype)
    status = np.full(n, EMPTY, np.int32)
    iters = np.zeros(n, np.int32)
    live = (y < 2).any(1)
    out_before = np.zeros(n, bool)
    info = np.zeros((n, D, D))
    for it in range(1, max_iter + 1):
        if not live.any():
            break
        e = ev(cs, th, method, y, params)
        s = e["s"].astype(dtype)
        iters[live] = it
        info[live] = e["info"][live]
        with np.errstate(invalid="ignore"):
            mx = np.abs(s).max(1)
            bad = live & ~(e["pd"] & np.isfinite(mx))
            conv = live & ~bad & (mx <= tol)
            outward = (((th >= bound) & (s > 0)) | ((th <= -bound) & (s < 0))).any(1)
        atb = live & ~bad & ~conv & outward & out_before
        status[bad], status[conv], status[atb] = SINGULAR, CONVERGED, AT_BOUND
        live = live & ~bad & ~conv & ~atb
        if it == max_iter:
            status[live] = MAX_ITERS
            break
        scale = np.where(mx > cap, cap / np.where(mx > 0, mx, 1.0), 1.0).astype(dtype)
        step = np.where(live[:, None], s * scale[:, None], 0).astype(dtype)
        th = np.where(live[:, None], np.clip((th + step).astype(dtype), -bound, bound), th).astype(dtype)
        out_before = np.where(live, outward, out_before)
    return {"theta_hat": np.where((status == EMPTY)[:, None], np.nan, th), "status": status, "iterations": iters, "info": info}


def root_of(case, method):
    """The oracle's own root of a case: fisher64 from the oracle's EAP, 60 steps, tol 1e-12.  Computed once."""
    key = (case[0], method)
    if key not in _ROOT:
        _ROOT[key] = fisher64(case_of(case), method, eap_of(case))
    return _ROOT[key]


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def ratios(cs, method, got, tol=TOL, bound=sc.SPAN, y=None, root=None, tag=""):
    """The rules on a result {theta_hat (n, D) float32, info (n, D, D), status, iterations} for the rows y (default: the case's):
    asserts what is exact (empty, at_bound, the shape of things) and returns the largest ratios found, {"s": (|s_d| - tol) / u_d over
    the converged persons, "root": (|theta_hat - root| - tol) / u_d where `root` (fisher64's result for the same rows) is given,
    the model is concave and both converged, "info": |I - I64| / (2^-23 sum |terms|)} -- each to be held against POINT_C."""
    y = cs["y"] if y is None else y
    th = np.asarray(got["theta_hat"])
    status, iters = np.asarray(got["status"]), np.asarray(got["iterations"])
    n, D = len(y), cs["D"]
    assert th.shape == (n, D) and th.dtype == np.float32 and status.shape == (n,) and iters.shape == (n,), tag
    assert ((status >= 0) & (status <= EMPTY)).all(), tag
    nobody = ~(y < 2).any(1)
    assert np.array_equal(status == EMPTY, nobody), tag
    assert np.isnan(th[nobody]).all() and (iters[nobody] == 0).all() and (np.asarray(got["info"])[nobody] == 0).all(), tag
    assert np.isfinite(th[~nobody]).all() and (iters[~nobody] >= 1).all(), tag
    e = evaluate(cs, np.where(nobody[:, None], 0.0, th.astype(np.float64)), method, y)
    out = {"s": 0.0, "root": 0.0, "info": 0.0}
    conv = status == CONVERGED
    if conv.any():
        assert e["pd"][conv].all(), tag
        out["s"] = float((np.maximum(np.abs(e["s"][conv]) - tol, 0.0) / e["u"][conv]).max())
        if root is not None and concave(cs):
            both = conv & (root["status"] == CONVERGED)
            if both.any():
                out["root"] = float((np.maximum(np.abs(th[both].astype(np.float64) - root["theta_hat"][both]) - tol, 0.0)
                                     / e["u"][both]).max())
    some = ~nobody
    ia, ig = e["info_abs"][some], np.asarray(got["info"], np.float64)[some]
    dead = ia == 0
    assert (ig[dead] == 0).all(), tag
    if (~dead).any():
        out["info"] = float((np.abs(ig - e["info"][some])[~dead] / (U * ia[~dead])).max())
    atb = status == AT_BOUND
    if atb.any():
        on_hi, on_lo = th[atb] == np.float32(bound), th[atb] == np.float32(-bound)
        with np.errstate(invalid="ignore"):
            outward = (on_hi & (e["s"][atb] > 0)) | (on_lo & (e["s"][atb] < 0))
        assert outward.any(1).all(), tag
    return out


def restated_f32(cs, method, theta0, y=None, max_iter=MAX_ITER, tol=TOL, bound=sc.SPAN):
    """The method said again in float32 numpy: theta, the item parameters, z, both sigmoids and every term of a cell in float32
    (Q formed on its own), the asymptotes of 3PL / 4PL from float64, a person's sums by numpy's float32 sum, the solve in
    float32; the same step control and ways to stop."""
    f4, f8 = np.float32, np.float64
    y = cs["y"] if y is None else y
    a8, b8, lo8, hi8 = _params(cs)
    a, b = a8.astype(f4), b8.astype(f4)
    Dc, D = f4(cs["Dc"]), cs["D"]
    dmc8, omd8 = hi8 - lo8, 1.0 - hi8
    if cs["model"] == "irt_3pl":
        dmc8 = vo.sigmoid(-np.asarray(cs["params"]["c"], f8)).reshape(1, -1)
    if cs["model"] == "irt_4pl":
        omd8 = vo.sigmoid(-np.asarray(cs["params"]["d"], f8)).reshape(1, -1)
    m, one = y < 2, y == 1

    def ev(cs_, th, method_, y_, params_):
        th = th.astype(f4)
        z = (Dc * (th @ a + b).astype(f4)).astype(f4)
        ez = np.exp(-np.abs(z)).astype(f4)
        r = (f4(1) / (f4(1) + ez)).astype(f4)
        er = (ez * r).astype(f4)
        sg, sn = np.where(z >= 0, r, er), np.where(z >= 0, er, r)
        if concave(cs):
            t = np.where(one, sn, -sg).astype(f4)
            w = (er * r).astype(f4)
        else:
            P = (lo8 + dmc8 * sg.astype(f8)).astype(f4)
            Q = (omd8 + dmc8 * sn.astype(f8)).astype(f4)
            pz = (dmc8.astype(f4) * (er * r).astype(f4)).astype(f4)
            u1, u0 = (pz / P).astype(f4), (pz / Q).astype(f4)
            t = np.where(one, u1, -u0).astype(f4)
            w = (u1 * u0).astype(f4)
        t, w = np.where(m, t, f4(0)).astype(f4), np.where(m, w, f4(0)).astype(f4)
        g = np.stack([(t * a[d]).astype(f4).sum(1, dtype=f4) for d in range(D)], 1) * Dc
        info = np.zeros((len(y), D, D), f4)
        for d in range(D):
            for k in range(d, D):
                info[:, d, k] = info[:, k, d] = (w * (a[d] * a[k]).astype(f4)).astype(f4).sum(1, dtype=f4) * (Dc * Dc)
        M = info.copy()
        if method == "map":
            g = (g - th).astype(f4)
            M = (M + np.eye(D, dtype=f4)[None]).astype(f4)
        elif method == "wle":
            Jw = ((w * (a[0] * a[0] * a[0]).astype(f4)).astype(f4) * (sn - sg).astype(f4)).astype(f4).sum(1, dtype=f4) * (Dc * Dc * Dc)
            with np.errstate(divide="ignore", invalid="ignore"):
                g = (g + (Jw / (f4(2) * info[:, 0, 0]))[:, None]).astype(f4)
        pd = np.isfinite(M).all((1, 2)) & np.isfinite(g).all(1)
        for d in range(D):
            pd &= np.linalg.det(np.where(pd[:, None, None], M, np.eye(D, dtype=f4)).astype(f8)[:, :d + 1, :d + 1]) > 0
        s = np.full((len(y), D), np.nan, f4)
        if pd.any():
            s[pd] = np.linalg.solve(M[pd].astype(f4), g[pd].astype(f4)[:, :, None])[:, :, 0].astype(f4)
        return {"s": s, "pd": pd, "info": info.astype(f8)}

    out = fisher64(cs, method, np.asarray(theta0, f4), y, None, max_iter, f4(tol), f4(bound), f4(STEP_CAP), dtype=f4, evaluate_fn=ev)
    out["theta_hat"] = out["theta_hat"].astype(f4)
    return out
