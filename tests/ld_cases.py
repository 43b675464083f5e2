"""The float64 oracle and the cases of the local-dependence tests (tests/test_ld_host.py on the CPU, tests/test_gpu_ld.py on the
GPU): the pairwise-complete residual sums n, s, ss, sp and Yen's Q3.

The oracle: the point estimate of every person comes from score_cases.irt_oracle / cdm_oracle (`mean`, `node`), P from it and the
case parameters, the residuals r = m (y - P) with m = [y < 2], and the four tables by plain float64 matrix products.  q3 is
computed twice: by the closed form over the tables (q3_of_tables) and, pair by pair, as np.corrcoef over the persons who answered
both items (q3_corrcoef) -- the second checks the formula, not only the arithmetic.

Cases: all of score_cases.IRT_CASES and CDM_CASES, and one planted case, q3_2pl_n5000_j70_ld: item 1 has the a and b of item 0
and, where both are observed, copies item 0's answer with probability 0.8.

The comparison condition of q3 (COND_*): off-diagonal pairs with oracle n >= 8 and both oracle variances v / n > 0.01.  It is a
condition on the oracle, not a measurement; LEFT_OUT_CAP says how much of a case it may leave out."""
import numpy as np

from oracle import vi_oracle as vo
from tests import score_cases as sc

SCALE = 1024.0                   # PP_SCALE (vipsy_amd/csrc/k_grid_pairs.hip): 2^10 into the fp16 split of r and r^2
COND_MIN_PAIRS = 8
COND_MIN_VAR = 0.01

PLANTED = ("q3_2pl_n5000_j70_ld", 5000, 70, "irt_2pl", 1, 1.0, 61, 0.20, (0.5, 1.5), 31)
PLANTED_RATE, PLANTED_SEED = 0.8, 32

IRT = list(sc.IRT_CASES) + [PLANTED]
CDM = list(sc.CDM_CASES)
ALL = [("irt", c) for c in IRT] + [("cdm", c) for c in CDM]
ALL_IDS = [c[0] for _, c in ALL]
# the share of the off-diagonal pairs the comparison condition may leave out; None: tables only, no q3 comparison
LEFT_OUT_CAP = {"case3_1pl_j130": 0.40, "case4_3pl_j500_sparse": None}
CORRCOEF_MAX_J = 130             # q3_corrcoef is a Python loop over the pairs: the small cases

_CASES, _ORACLES = {}, {}


def planted_case():
    cs = sc.irt_case(PLANTED)
    p = cs["params"]
    p["a"][:, 1] = p["a"][:, 0]
    p["b"][:, 1] = p["b"][:, 0]
    y = cs["y"]
    copy = np.random.RandomState(PLANTED_SEED).uniform(size=cs["N"]) < PLANTED_RATE
    both = (y[:, 0] < 2) & (y[:, 1] < 2) & copy
    y[both, 1] = y[both, 0]
    return cs


def case_of(kind, case):
    """The case, built once and shared; callers must not modify it."""
    key = case[0]
    if key not in _CASES:
        _CASES[key] = planted_case() if case is PLANTED or key == PLANTED[0] else (sc.irt_case(case) if kind == "irt" else sc.cdm_case(case))
    return _CASES[key]


def irt_prob(cs, theta_hat, params=None):
    """P [N][J] at theta_hat [N][D], float64: c + (d - c) sigmoid(Dc (theta_hat . a + b)), 1PL with a = 1."""
    p = cs["params"] if params is None else params
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    th = f8(theta_hat).reshape(len(theta_hat), -1)
    b = f8(p["b"]).reshape(1, -1)
    z = cs["Dc"] * ((th + b) if cs["model"] == "irt_1pl" else (th @ f8(p["a"]) + b))
    lo = vo.sigmoid(f8(p["c"])).reshape(1, -1) if cs["model"] in ("irt_3pl", "irt_4pl") else 0.0
    hi = vo.sigmoid(f8(p["d"])).reshape(1, -1) if cs["model"] == "irt_4pl" else 1.0
    return lo + (hi - lo) * vo.sigmoid(z)


def cdm_prob(cs, pattern, params=None):
    """P [N][J] at the patterns [N]: eta ? 1 - s : g, eta from the oracle's dina_eta / dino_eta."""
    p = cs["params"] if params is None else params
    eta_all, _ = (vo.dino_eta if cs["cdm"] == "dino" else vo.dina_eta)(cs["K"], np.asarray(cs["q"], np.float64))
    g = vo.sigmoid(np.asarray(p["g"], np.float64)).reshape(1, -1)
    s = vo.sigmoid(np.asarray(p["s"], np.float64)).reshape(1, -1)
    return np.where(eta_all[np.asarray(pattern, np.int64)] > 0, 1 - s, g)


def tables(y, prob):
    """n, s, ss, sp [J][J] in float64, and the residuals r and the mask m [N][J]."""
    m = (y < 2).astype(np.float64)
    r = m * (y.astype(np.float64) * m - prob)
    return {"n": m.T @ m, "s": r.T @ m, "ss": (r * r).T @ m, "sp": r.T @ r, "r": r, "m": m}


def q3_of_tables(t, min_pairs=COND_MIN_PAIRS):
    """cov = sp - s s^T / n, v = ss - s^2 / n, q3 = cov / sqrt(v v^T); NaN where n < min_pairs or either v <= 0; diagonal 1."""
    n, s, ss, sp = t["n"], t["s"], t["ss"], t["sp"]
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = sp - s * s.T / n
        v = ss - s * s / n
        q3 = cov / np.sqrt(v * v.T)
    bad = ~((n >= min_pairs) & (v > 0) & (v.T > 0))
    q3[bad] = np.nan
    d = np.arange(len(n))
    q3[d, d] = np.where(bad[d, d], np.nan, 1.0)
    return q3, v


def q3_corrcoef(t, min_pairs=COND_MIN_PAIRS):
    """q3 pair by pair: np.corrcoef of the two items' residuals over the persons who answered both."""
    r, m = t["r"], t["m"] > 0
    J = r.shape[1]
    q3 = np.full((J, J), np.nan)
    for j in range(J):
        for k in range(j, J):
            both = m[:, j] & m[:, k]
            if both.sum() < min_pairs:
                continue
            a, b = r[both, j], r[both, k]
            if a.std() == 0 or b.std() == 0:
                continue
            q3[j, k] = q3[k, j] = 1.0 if j == k else np.corrcoef(a, b)[0, 1]
    return q3


def condition(o):
    """The off-diagonal pairs on which q3 is compared: oracle n >= 8 and both oracle variances v / n > 0.01."""
    n, v = o["n"], o["v"]
    with np.errstate(divide="ignore", invalid="ignore"):
        vn = np.where(n > 0, v / n, 0.0)
    keep = (n >= COND_MIN_PAIRS) & (vn > COND_MIN_VAR) & (vn.T > COND_MIN_VAR)
    keep[np.arange(len(n)), np.arange(len(n))] = False
    return keep


def summary(q3):
    """mean of the finite off-diagonal entries and the largest off-diagonal q3 - mean."""
    off = ~np.eye(len(q3), dtype=bool) & np.isfinite(q3)
    mean = q3[off].mean()
    return float(mean), float((q3[off] - mean).max())


def oracle(kind, case, params=None, y=None):
    """The oracle of a case, computed once and shared (never modified): the point estimates (`theta_hat` float64 [N][D] or `pattern`
    [N]), the tables, `q3`, `v`, `keep` (condition) and `mean`, `max`.  params / y: other parameters or rows (not cached)."""
    key = case[0]
    if params is None and y is None and key in _ORACLES:
        return _ORACLES[key]
    cs = case_of(kind, case)
    yy = cs["y"] if y is None else y
    if kind == "irt":
        est = sc.irt_oracle(cs, params=params, y=yy)["mean"]
        prob = irt_prob(cs, est, params)
    else:
        est = sc.cdm_oracle(cs, params=params, y=yy)["node"]
        prob = cdm_prob(cs, est, params)
    o = tables(yy, prob)
    o["theta_hat" if kind == "irt" else "pattern"] = est
    o["q3"], o["v"] = q3_of_tables(o)
    o["keep"] = condition(o)
    o["mean"], o["max"] = summary(o["q3"]) if np.isfinite(o["q3"][~np.eye(len(o["q3"]), dtype=bool)]).any() else (np.nan, np.nan)
    if params is None and y is None:
        _ORACLES[key] = o
    return o


def row_error(got, want):
    """The row rule: max over the rows of |got - want|_inf / max(1, |want|_inf of the row)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), 1.0)).max())


def _split16(v):
    """v (float32, already scaled) -> fp16 head and fp16 remainder, as float32."""
    h = v.astype(np.float16).astype(np.float32)
    return h, (v - h).astype(np.float16).astype(np.float32)


def restated_f32(kind, case):
    """The kernels' arithmetic said again in numpy: theta_hat and the parameters in float32, P and r in float32, r and r^2 times
    2^10 as fp16 pairs, m exact, the products in float32 (hh + hl + lh for sp; head and low against m for s and ss), the scales
    taken off, the host formulas of pair_q3_host in float64."""
    from vipsy_amd.grid import pair_q3_host
    cs, o = case_of(kind, case), oracle(kind, case)
    f4 = np.float32
    y = cs["y"]
    m = (y < 2).astype(f4)
    if kind == "irt":
        p = cs["params"]
        th = o["theta_hat"].astype(f4)
        b = p["b"].astype(f4).reshape(1, -1)
        z = f4(cs["Dc"]) * ((th + b) if cs["model"] == "irt_1pl" else (th @ p["a"].astype(f4) + b)).astype(f4)
        sig = lambda v: (f4(1) / (f4(1) + np.exp(-v.astype(f4)))).astype(f4)                  # noqa: E731
        lo = sig(p["c"].reshape(1, -1)) if cs["model"] in ("irt_3pl", "irt_4pl") else f4(0)
        hi = sig(p["d"].reshape(1, -1)) if cs["model"] == "irt_4pl" else f4(1)
        prob = (lo + (hi - lo) * sig(z)).astype(f4)
    else:
        prob = cdm_prob(cs, o["pattern"]).astype(f4)
    r = (m * (y.astype(f4) * m - prob)).astype(f4)
    rh, rl = _split16(r * f4(SCALE))
    qh, ql = _split16((r * r).astype(f4) * f4(SCALE))
    un = f4(1.0 / SCALE)
    t = {"n": m.T @ m,
         "s": ((rh.T @ m + rl.T @ m) * un).astype(f4),
         "ss": ((qh.T @ m + ql.T @ m) * un).astype(f4),
         "sp": ((rh.T @ rh + rh.T @ rl + rl.T @ rh) * (un * un)).astype(f4)}
    t["q3"] = pair_q3_host(t["n"], t["s"], t["ss"], t["sp"], COND_MIN_PAIRS)
    return t
