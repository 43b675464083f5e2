"""The float64 oracle and the cases of the LD X2 tests (tests/test_x2_host.py on the CPU, tests/test_gpu_x2.py on the GPU): the
pairwise 2 x 2 tables n11, n10, n01, n00 and Chen & Thissen's LD X2 / G2.

The oracle computes everything from the case parameters and nothing from the code under test: the nodes and log-weights of the
grid (corner_cases.grid_of), the probabilities P(y_j = 1 | node) in float64 as ld_cases has them (ld_cases.irt_prob at the nodes,
ld_cases.cdm_prob at the patterns), p0 = 1 - p1 in float64, the tables as int64 numpy products of the 0 / 1 indicators, and the
statistics by plain float64 formulas (stats) -- and, for tiny J, pair by pair in a Python loop (stats_loop).

Cases: the IRT cases of ld_cases (1PL to 4PL, x_feature 1, 2 and 3, the planted pair among them), a second 1PL case
(ONEPL) and one DINA case.

The comparison condition of x2 (condition): off-diagonal pairs with oracle N_jk >= 8 and all four oracle E_ab >= 1.  A case must
keep at least KEEP_MIN of its off-diagonal pairs, or it is compared on its tables only (TABLES_ONLY; tests/test_x2_host.py asserts
the share of every case, on both sides of the line).

The bound.  The tables are exact integers; the only rounding that reaches x2 is that of the fp16-pair operand image, through E.
A relative error eps of every E_ab moves x2 by at most eps * sum_ab E |d x2 / d E| = eps * sum_ab (2 |O - E| + (O - E)^2 / E) to
first order, so the measure is  ratio = |x2 - x2_oracle| / sum_ab (2 |O - E| + (O - E)^2 / E)  over the pairs of the condition,
beside the relative error of E itself.  REL_E is the constant both are held to on the GPU; the operand phase said again in numpy
(restated_probs: the oracle's log-probabilities rounded to float32, times 2^10, as an fp16 head and the fp16 of the remainder --
corner_cases._split16 -- and the exponential of their sum rounded to float32, as grid_image_probs returns it) must stay below
HALF of it on the CPU (tests/test_x2_host.py, which prints what it measures)."""
import numpy as np

from tests import corner_cases as cc
from tests import ld_cases as ld

COND_MIN_PAIRS = 8
COND_MIN_EXPECTED = 1.0
KEEP_MIN = 0.60
# REL_E, as the project derives such constants (sx2_cases.SX2_C): in units of 2^-24, half a float32 ulp.  The restatement alone
# costs 2.97 units on E and 1.49 on the x2 ratio on these cases (RESTATED_MEASURED, case6_dina_k3 the largest; test_x2_host.py
# prints them all).  The image on the GPU is not filled from float64 tables rounded once, as the restatement's is, but from
# float32 response functions: T = log P with |T| < 16 at every node that carries weight is then right to a float32 ulp of 16 at
# best, 2^-20 = 16 units as half an ulp; a product p_a p_b has two such factors, 32 units; and the evaluation of the response
# function in float32 is granted as much again: 64 units.  The restatement must meet half of it (it stays 10 times below).
UNIT = 2.0 ** -24
RESTATED_MEASURED = (2.97, 1.49)
REL_E = 64 * UNIT
X2_FLOOR = 1e-10                 # float64 rounding of the statistic itself, where O = E to the last bit

# the 1PL case of ld_cases spreads its thresholds over [-4, 4] and keeps 22 % of its pairs: tables only.  A 1PL case of this
# module's own, thresholds over [-1.4, 1.4], so that the 1PL tables are compared on x2 too
ONEPL = ("x2_1pl_n600_j45", 600, 45, "irt_1pl", 1, 1.0, 41, 0.10, None, 71)
IRT = list(ld.IRT) + [ONEPL]
CDM = [c for c in ld.CDM if c[0] == "case6_dina_k3"]
ALL = [("irt", c) for c in IRT] + [("cdm", c) for c in CDM]
ALL_IDS = [c[0] for _, c in ALL]
TABLES_ONLY = ("case3_1pl_j130", "case4_3pl_j500_sparse")

_O, _CASES = {}, {}


def onepl_case():
    """score_cases.irt_case with the thresholds shrunk to 0.35 of their draw and the responses simulated again from them."""
    from oracle import vi_oracle as vo
    from tests import score_cases as sc
    cs = sc.irt_case(ONEPL)
    cs["params"]["b"] = (cs["params"]["b"] * np.float32(0.35)).astype(np.float32)
    rng = np.random.RandomState(ONEPL[-1] + 1)
    x = rng.normal(size=(cs["N"], 1))
    y = (rng.uniform(size=(cs["N"], cs["J"])) < vo.sigmoid(cs["Dc"] * (x + cs["params"]["b"].astype(np.float64)))).astype(np.uint8)
    y[rng.uniform(size=y.shape) < ONEPL[7]] = 255
    cs["y"] = y
    return cs


def case_of(kind, case):
    """The case, built once and shared; callers must not modify it."""
    if case[0] != ONEPL[0]:
        return ld.case_of(kind, case)
    if case[0] not in _CASES:
        _CASES[case[0]] = onepl_case()
    return _CASES[case[0]]


def tables(y):
    """n11, n10, n01, n00 [J][J] int64: products of the indicators [y == 1] and [y == 0]; every other byte is not observed."""
    u, z = (y == 1).astype(np.int64), (y == 0).astype(np.int64)
    return {"n11": u.T @ u, "n10": u.T @ z, "n01": z.T @ u, "n00": z.T @ z}


def probs(kind, cs):
    """(p1, p0 [J][G] float64, logw [G] float64): the model at the nodes of score(), from the case parameters."""
    coord, logw = cc.grid_of(cs, kind)
    if kind == "cdm":
        p1 = ld.cdm_prob(cs, np.arange(coord.shape[0])).T
    else:
        p1 = ld.irt_prob(cs, coord).T
    return np.ascontiguousarray(p1), 1.0 - p1, np.asarray(logw, np.float64)


def restated_probs(kind, cs):
    """(p1, p0 float32 [J][G], logw) by the arithmetic of the operand image (module docstring)."""
    coord, logw = cc.grid_of(cs, kind)
    out = []
    for T in cc.item_tables(cs, kind, coord):
        h, lo = cc._split16(T.astype(np.float32) * np.float32(1024.0))
        out.append(np.exp((h.astype(np.float64) + lo.astype(np.float64)) / 1024.0).astype(np.float32))
    return out[0], out[1], np.asarray(logw, np.float32)


def _phi(t):
    den = (t[1, 1] + t[1, 0]) * (t[0, 1] + t[0, 0]) * (t[1, 1] + t[0, 1]) * (t[1, 0] + t[0, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (t[1, 1] * t[0, 0] - t[1, 0] * t[0, 1]) / np.sqrt(den), np.nan)


def stats(t, p1, p0, logw, min_pairs=COND_MIN_PAIRS, min_expected=COND_MIN_EXPECTED):
    """x2, g2, sign, phi_obs, phi_exp, N, E [2][2][J][J] (indexed [a][b]) and bad, in float64 from int64 tables."""
    w = np.exp(logw - logw.max())
    w = w / w.sum()
    P = (p0, p1)
    e = np.array([[np.einsum("g,jg,kg->jk", w, P[a], P[b]) for b in (0, 1)] for a in (0, 1)])
    e = e / e.sum((0, 1))
    O = np.array([[t["n00"], t["n01"]], [t["n10"], t["n11"]]], np.float64)
    N = O.sum((0, 1))
    E = N * e
    with np.errstate(divide="ignore", invalid="ignore"):
        x2 = np.where(O != E, (O - E) ** 2 / E, 0.0).sum((0, 1))
        g2 = 2.0 * np.where(O > 0, O * np.log(np.where(O > 0, O, 1.0) / E), 0.0).sum((0, 1))
    J = len(N)
    bad = np.eye(J, dtype=bool) | (N < min_pairs) | ~(E >= min_expected).all((0, 1))
    po, pe = _phi(O), _phi(e)
    with np.errstate(invalid="ignore"):
        sign = np.where(bad | np.isnan(po) | np.isnan(pe), 0.0, np.sign(po - pe))
    return {"x2": np.where(bad, np.nan, x2), "g2": np.where(bad, np.nan, g2), "x2_all": x2, "sign": sign, "phi_obs": po,
            "phi_exp": pe, "N": N, "E": E, "O": O, "bad": bad}


def stats_loop(t, p1, p0, logw, min_pairs, min_expected):
    """The same, pair by pair and cell by cell in Python floats: x2, g2, sign [J][J] (tiny J)."""
    import math
    J, G = p1.shape
    lw = [float(v) for v in logw]
    mx = max(lw)
    w = [math.exp(v - mx) for v in lw]
    sw = sum(w)
    w = [v / sw for v in w]
    x2, g2, sign = np.full((J, J), np.nan), np.full((J, J), np.nan), np.zeros((J, J))
    P = (p0, p1)
    for j in range(J):
        for k in range(J):
            O = {(1, 1): int(t["n11"][j, k]), (1, 0): int(t["n10"][j, k]), (0, 1): int(t["n01"][j, k]), (0, 0): int(t["n00"][j, k])}
            e = {(a, b): sum(w[g] * float(P[a][j, g]) * float(P[b][k, g]) for g in range(G)) for a in (0, 1) for b in (0, 1)}
            tot = sum(e.values())
            N = sum(O.values())
            E = {ab: N * e[ab] / tot for ab in e}

            def phi(c):
                den = (c[1, 1] + c[1, 0]) * (c[0, 1] + c[0, 0]) * (c[1, 1] + c[0, 1]) * (c[1, 0] + c[0, 0])
                return (c[1, 1] * c[0, 0] - c[1, 0] * c[0, 1]) / math.sqrt(den) if den > 0 else None
            if j == k or N < min_pairs or min(E.values()) < min_expected:
                continue
            x2[j, k] = sum((O[ab] - E[ab]) ** 2 / E[ab] for ab in O)
            g2[j, k] = 2.0 * sum(O[ab] * math.log(O[ab] / E[ab]) for ab in O if O[ab] > 0)
            po, pe = phi(O), phi(e)
            if po is not None and pe is not None:
                sign[j, k] = (po > pe) - (po < pe)
    return x2, g2, sign


def condition(o):
    """The off-diagonal pairs on which x2 is compared: oracle N >= 8 and all four oracle E >= 1."""
    return ~o["bad"]


def oracle(kind, case):
    """The oracle of a case, computed once and shared (never modified): the tables, the statistics, `keep` and `share`."""
    key = case[0]
    if key not in _O:
        cs = case_of(kind, case)
        t = tables(cs["y"])
        o = stats(t, *probs(kind, cs))
        o.update(t)
        o["keep"] = condition(o)
        J = cs["J"]
        o["share"] = float(o["keep"].sum()) / max(1, J * (J - 1))
        _O[key] = o
    return _O[key]


def ratios(o, x2, E):
    """(max relative error of E, max |x2 - oracle| / sum_ab (2 |O - E| + (O - E)^2 / E)) over the pairs of the condition."""
    keep = o["keep"]
    if not keep.any():
        return 0.0, 0.0
    Eo, O = o["E"], o["O"]
    Eo = np.where(Eo > 0, Eo, 1.0)                                  # (pairs nobody answered both items of are not kept)
    rel_e = float((np.abs(np.asarray(E, np.float64) - Eo) / Eo)[:, :, keep].max())
    den = (2.0 * np.abs(O - Eo) + (O - Eo) ** 2 / Eo).sum((0, 1))[keep]
    r = float((np.maximum(np.abs(x2[keep] - o["x2"][keep]) - X2_FLOOR, 0.0) / den).max())
    return rel_e, r
