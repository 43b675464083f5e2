"""The float64 oracle, the cases and the rules of the summed-score tests (tests/test_sx2_host.py on the CPU, tests/test_gpu_sx2.py on
the GPU): the Lord-Wingersky tables of vx_sumscore_model, the integer tables of vx_sumscore_persons / vx_sumscore_observed, and
S-X2 and the score table out of them.  Everything is seeded numpy: every case is the same on every machine.

Definitions (restated from include/vipsy_amd.h).  Over Js items and G nodes with p1[j][g] = P(y_j = 1 | g), p0[j][g] = P(y_j = 0 | g)
and w_g = exp(logw[g]):  S(s | g): S = delta_0, then for every item in ascending order S'[s] = p0 S[s] + p1 S[s - 1];  S_-j the same
without item j;  e1[j][s] = sum_g w_g p1[j][g] S_-j(s - 1 | g),  e0[j][s] = sum_g w_g p0[j][g] S_-j(s | g),  dist[g][s] = S(s | g).

Rule for e1, e0, dist (the oracle is given the kernel's own float32 p1, p0, logw):

    |e - e64| <= C (Js + G) 2^-24 e64 + 2^-100

relative because no term is negative; the floor covers products that underflow at one node while another node carries the entry.
C = SX2_C, by the project's convention the next power of two above twice the largest ratio measured on one MI355X over all the
cases below (written beside the constant).

Rule for the statistic.  The host forms S-X2 in float64 from the device tables, so its error is that of the tables, propagated to
first order.  With rho = C (Js + G) 2^-24 the relative error of e1 and e0: E_s = e1 / (e1 + e0) moves by at most 2 rho E_s (1 - E_s); a
cell's expected count Ehat = sum n[s] E_s by dE = sum n[s] 2 rho E_s (1 - E_s), and its term t = d^2 / Ehat + d^2 / F with d = O - Ehat,
F = N - Ehat by |dt/dEhat| dE <= (2 |d| / Ehat + d^2 / Ehat^2 + 2 |d| / F + d^2 / F^2) dE.  The rule is the sum of that over the cells
(sx2_tolerance).  df and n_cells must equal the oracle's exactly -- which needs the collapse, a discrete thing, to be decided the
same way: in the float64 oracle no running expected count may sit within 1e-3 relative of min_expected where the decision of a
sweep step hangs on it (collapse_margin; asserted on the oracle alone in tests/test_sx2_host.py).  No item is left out."""
import math

import numpy as np

# the largest (|e - e64| - 2^-100) / ((Js + G) 2^-24 e64) found on one MI355X over MODEL_CASES (e1, e0 and dist) and the tables of
# the end-to-end cases was 0.358 (model_j2_g3, e1; the long cases stay below 0.11: the errors of the steps do not line up); twice
# that, and the next power of two above
SX2_MEASURED = 0.358
SX2_C = 1.0
FLOOR = 2.0 ** -100
COLLAPSE_MARGIN = 1e-3

# name, Js, G
MODEL_CASES = [
    ("model_j1_g4", 1, 4), ("model_j2_g3", 2, 3), ("model_j9_g1", 9, 1), ("model_j63_g5", 63, 5), ("model_j64_g5", 64, 5),
    ("model_j65_g5", 65, 5), ("model_j127_g3", 127, 3), ("model_j128_g3", 128, 3), ("model_j1023_g3", 1023, 3),
    ("model_j5_g1024", 5, 1024), ("model_j70_g61", 70, 61),
]
MODEL_IDS = [c[0] for c in MODEL_CASES]
BINOMIAL_P = 0.3

_MODEL = {}


def model_case(case):
    """p1, p0 [Js][G] and logw [G] as float32, and the float64 oracle over them; computed once, never modified.  Logistic
    probabilities spread over |z| <= 12 (p1 = sigmoid(z) and p0 = sigmoid(-z), each rounded on its own); from three items on, item 1
    is certain (p1 = 1, p0 = 0 exactly) and the last item impossible (p1 = 0, p0 = 1): exact shifts and exact zeros; from two nodes
    on, at the last node (`binomial`) ALL items share p1 = 0.3f, p0 = 0.7f: the binomial, in closed form."""
    name, Js, G = case
    if name not in _MODEL:
        rng = np.random.RandomState(1000 + 7 * Js + G)
        z = rng.uniform(-12.0, 12.0, size=(Js, G))
        p1 = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
        p0 = (1.0 / (1.0 + np.exp(z))).astype(np.float32)
        sure, never = (1, Js - 1) if Js >= 3 else (None, None)
        if sure is not None:
            p1[sure], p0[sure] = 1.0, 0.0
            p1[never], p0[never] = 0.0, 1.0
        binomial = G - 1 if G >= 2 else None
        if binomial is not None:
            p1[:, binomial], p0[:, binomial] = np.float32(BINOMIAL_P), np.float32(1.0 - BINOMIAL_P)
        w = rng.uniform(0.05, 1.0, size=G)
        logw = np.log(w / w.sum()).astype(np.float32)
        cs = {"name": name, "Js": Js, "G": G, "p1": p1, "p0": p0, "logw": logw, "sure": sure, "never": never, "binomial": binomial}
        cs["oracle"] = lord_wingersky(p1, p0, logw)
        _MODEL[name] = cs
    return _MODEL[name]


def _fold(S, p1k, p0k):
    """One recursion step over every node: S [G][len] -> S'[s] = p0 S[s] + p1 S[s - 1]."""
    out = p0k[:, None] * S
    out[:, 1:] += p1k[:, None] * S[:, :-1]
    return out


def lord_wingersky(p1, p0, logw):
    """The float64 tables over the given p1, p0 [Js][G] and logw [G] (taken as they are): e1, e0 [Js][Js + 1], dist [G][Js + 1]."""
    p1, p0 = np.asarray(p1, np.float64), np.asarray(p0, np.float64)
    w = np.exp(np.asarray(logw, np.float64))
    Js, G = p1.shape
    e1, e0 = np.zeros((Js, Js + 1)), np.zeros((Js, Js + 1))
    # prefix[k] = the first k items folded; the items after j are folded onto prefix[j]: O(Js^2) steps of [G][Js + 1]
    S = np.zeros((G, Js + 1))
    S[:, 0] = 1.0
    for j in range(Js):
        T = S.copy()
        for k in range(j + 1, Js):
            T = _fold(T, p1[k], p0[k])
        e1[j, 1:] = ((w * p1[j])[:, None] * T[:, :-1]).sum(0)
        e0[j] = ((w * p0[j])[:, None] * T).sum(0)
        S = _fold(S, p1[j], p0[j])
    return {"e1": e1, "e0": e0, "dist": S, "w": w}


def table_ratio(got, want, Js, G):
    """The largest (|e - e64| - 2^-100) / ((Js + G) 2^-24 e64) (0 where the floor alone covers the difference, inf where e64 = 0
    and it does not): the rule holds where this is <= C."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    over = np.maximum(np.abs(got - want) - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(over > 0, over / ((Js + G) * 2.0 ** -24 * want), 0.0)
    return float(r.max())


def binomial_row(Js, p1, p0):
    """C(Js, s) p1^s p0^(Js - s) in float64 from the float32 p1, p0 as given; through logarithms, since p1^s alone leaves the
    range of float64 long before the product does."""
    l1, l0 = math.log(float(np.float32(p1))), math.log(float(np.float32(p0)))
    return np.array([math.exp(math.lgamma(Js + 1) - math.lgamma(s + 1) - math.lgamma(Js - s + 1) + s * l1 + (Js - s) * l0)
                     for s in range(Js + 1)])


# ---- the integer tables -------------------------------------------------------------------------------------------------
def persons_oracle(y, rows, items):
    """score int32 [nb] (-1: not complete) of y[rows][:, items] (rows / items None: all)."""
    sub = y if rows is None else y[rows]
    sub = sub if items is None else sub[:, items]
    complete = (sub <= 1).all(1)
    return np.where(complete, (sub == 1).sum(1), -1).astype(np.int32)


def observed_oracle(y, items, score):
    """(o1 int32 [Js][Js + 1], n int64 [Js + 1]) over the complete persons of y (score >= 0), score by row of y."""
    sub = y if items is None else y[:, items]
    Js = sub.shape[1]
    o1, n = np.zeros((Js, Js + 1), np.int32), np.zeros(Js + 1, np.int64)
    keep = score >= 0
    np.add.at(n, score[keep], 1)
    for j in range(Js):
        np.add.at(o1[j], score[keep], (sub[keep, j] == 1).astype(np.int32))
    return o1, n


def integer_data(nb_total, J, seed, kind):
    """Responses uint8 [nb_total][J] for the integer kernels.  kind: 'mixed' (about a sixth of the persons with a 255 or a 254
    somewhere), 'one_score' (everybody complete with the same score), 'gaps' (complete, the scores 0, 1 and J only: empty score
    groups between), 'nobody' (everybody with a 255 in item 0)."""
    rng = np.random.RandomState(seed)
    y = (rng.uniform(size=(nb_total, J)) < rng.uniform(0.1, 0.9, size=(nb_total, 1))).astype(np.uint8)
    if kind == "mixed":
        hit = rng.uniform(size=nb_total) < 1.0 / 6.0
        col = rng.randint(0, J, size=nb_total)
        code = np.where(rng.uniform(size=nb_total) < 0.5, 255, 254).astype(np.uint8)
        y[hit, col[hit]] = code[hit]
    elif kind == "one_score":
        y[:] = 0
        y[:, : max(1, J // 3)] = 1
    elif kind == "gaps":
        pick = rng.randint(0, 3, size=nb_total)
        y[:] = 0
        y[pick == 1, J // 2] = 1
        y[pick == 2] = 1
    elif kind == "nobody":
        y[:, 0] = 255
    else:
        raise KeyError(kind)
    return y


# ---- S-X2 in float64, written out cell by cell ----------------------------------------------------------------------------
def chi2_tail(x, df):
    """The chi-square upper tail by numerical integration-free closed forms, written independently of vipsy_amd.grid.chi2_sf:
    the regularised upper incomplete gamma function Q(df / 2, x / 2) by its recurrence Q(a + 1, h) = Q(a, h) + h^a e^-h / Gamma(a + 1)
    from Q(1, h) = e^-h (even df) or Q(1 / 2, h) = erfc(sqrt(h)) (odd df)."""
    if df <= 0:
        return float("nan")
    h = 0.5 * x
    a, q = (1.0, math.exp(-h)) if df % 2 == 0 else (0.5, math.erfc(math.sqrt(h)))
    while a < 0.5 * df - 1e-9:
        q += math.exp(a * math.log(h) - h - math.lgamma(a + 1.0)) if h > 0 else 0.0
        a += 1.0
    return min(1.0, q)


def sx2_oracle(e1, e0, o1, n, n_params, min_expected=1.0, rho=0.0):
    """S-X2 of every item from float64 tables, one item and one score group at a time.  Returns sx2, df, p, n_cells [Js], `tol`
    [Js]: the first-order rule of the docstring above for a relative table error rho, and `margin` [Js]: the smallest relative
    distance of a running expected count from min_expected at a sweep step whose decision hangs on it (inf: none does)."""
    e1, e0, o1, n = (np.asarray(t, np.float64) for t in (e1, e0, o1, n))
    Js = e1.shape[0]
    out = {k: np.zeros(Js) for k in ("sx2", "p", "tol")}
    out["df"], out["n_cells"], out["margin"] = np.zeros(Js, np.int64), np.zeros(Js, np.int64), np.full(Js, np.inf)
    for j in range(Js):
        cells, run = [], [0.0, 0.0, 0.0, 0.0]                               # O, Ehat, F, dE
        for s in range(1, Js):
            tot = e1[j, s] + e0[j, s]
            E, Q = (e1[j, s] / tot, e0[j, s] / tot) if tot > 0 else (0.0, 0.0)
            run = [run[0] + o1[j, s], run[1] + n[s] * E, run[2] + n[s] * Q, run[3] + n[s] * 2.0 * rho * E * Q]
            lo, hi = min(run[1], run[2]), max(run[1], run[2])
            if hi >= min_expected * (1.0 - COLLAPSE_MARGIN):                # the decision hangs on the smaller count (or on both)
                for v in ((lo,) if hi >= min_expected * (1.0 + COLLAPSE_MARGIN) else (lo, hi)):
                    out["margin"][j] = min(out["margin"][j], abs(v - min_expected) / min_expected)
            if run[1] >= min_expected and run[2] >= min_expected:
                cells.append(run)
                run = [0.0, 0.0, 0.0, 0.0]
        if Js >= 2:
            if cells:
                cells[-1] = [a + b for a, b in zip(cells[-1], run)]
            else:
                cells = [run]
        stat = tol = 0.0
        for O, Eh, F, dE in cells:
            d = O - Eh
            if d != 0.0:
                stat += d * d / Eh + d * d / F if Eh > 0 and F > 0 else float("inf")
                if Eh > 0 and F > 0:
                    tol += (2 * abs(d) / Eh + d * d / Eh ** 2 + 2 * abs(d) / F + d * d / F ** 2) * dE
        out["sx2"][j], out["tol"][j], out["n_cells"][j] = stat, tol + 1e-12 * (1.0 + stat), len(cells)
        out["df"][j] = len(cells) - int(n_params[j])
        out["p"][j] = chi2_tail(stat, out["df"][j]) if math.isfinite(stat) else float("nan")
    return out


def score_table_oracle(dist, logw, theta):
    """prob [Js + 1], eap, psd [Js + 1][D] in float64, one score at a time."""
    dist, theta = np.asarray(dist, np.float64), np.asarray(theta, np.float64)
    w = np.exp(np.asarray(logw, np.float64))
    S, D = dist.shape[1], theta.shape[1]
    prob, eap, psd = np.zeros(S), np.zeros((S, D)), np.zeros((S, D))
    for s in range(S):
        joint = w * dist[:, s]
        prob[s] = joint.sum()
        post = joint / prob[s]
        eap[s] = post @ theta
        psd[s] = np.sqrt(post @ (theta - eap[s]) ** 2)
    return {"prob": prob, "eap": eap, "psd": psd}


def prob_ratio(got, want, other):
    """The largest |p - p64| / ((|z| + 1) 2^-21 p64), z = log(p64 / other64) the logit, of probabilities read back from the operand
    image against float64 ones made from the item parameters without it (`other`: the float64 probability of the other answer):
    must be <= 1.  The image holds T = log p; exp carries the ABSOLUTE error of T into p as a relative one.  What T carries, in
    units of 2^-24: the float32 z = Dc (theta a + b) from a float32 theta, |theta a| + |z| <= 2 |z| + |b|; the cell forms T = y z -
    softplus(z) in float32, so where p is near 1 and T small the roundings of z and of softplus(z), |z| each, stay in T
    though |T| does not show them; the two fp16 terms of T 2^10, 2^-22 |T| = 4 |T| with |T| <= |z| + 0.7; the hardware log2 and
    the float32 p, a few more.  Together below 8 (|z| + 1): the error follows |z|, not |log p|."""
    got, want, other = (np.asarray(t, np.float64) for t in (got, want, other))
    z = np.abs(np.log(want) - np.log(other))
    return float((np.abs(got - want) / ((z + 1.0) * 2.0 ** -21 * want)).max())


# ---- the models of the end-to-end cases -----------------------------------------------------------------------------------
def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def grid_1d(nodes=61, span=6.0):
    """The nodes and normalised log-weights of score_grid(1, nodes, span), in float64."""
    th = np.linspace(-span, span, nodes)
    lw = -0.5 * th * th
    lw = lw - (lw.max() + np.log(np.exp(lw - lw.max()).sum()))
    return th[:, None], lw


PLANTED_SEED = 5
PLANTED_ITEM = 5
PLANTED_ASYMPTOTE = 0.35
_PLANTED = {}


def planted_case():
    """4 096 persons x 12 items, 2PL, complete; the fitted parameters are the generating ones, except that item 5 was generated
    with a lower asymptote of 0.35 the model lacks.  Computed once, never modified."""
    if not _PLANTED:
        rng = np.random.RandomState(PLANTED_SEED)
        N, J = 4096, 12
        a = rng.uniform(0.8, 2.0, size=(1, J))
        b = rng.normal(0.0, 1.0, size=(1, J))
        x = rng.normal(size=(N, 1))
        p = sigmoid(x @ a + b)
        p[:, PLANTED_ITEM] = PLANTED_ASYMPTOTE + (1.0 - PLANTED_ASYMPTOTE) * p[:, PLANTED_ITEM]
        y = (rng.uniform(size=(N, J)) < p).astype(np.uint8)
        _PLANTED.update({"name": "planted_2pl_n4096_j12", "N": N, "J": J, "model": "irt_2pl", "D": 1, "Dc": 1.0, "nodes": 61,
                         "span": 6.0, "y": y, "params": {"a": a.astype(np.float32), "b": b.astype(np.float32)},
                         "n_params": np.full(J, 2, np.int64)})
    return _PLANTED


def irt_probs(cs, items=None):
    """(p1, p0 [Js][G], theta [G][1], logw [G]) in float64 from the float32 parameters of a 1PL / 2PL case with D = 1."""
    theta, logw = grid_1d(cs["nodes"], cs["span"])
    a = cs["params"]["a"].astype(np.float64) if "a" in cs["params"] else np.ones((1, cs["J"]))
    z = cs["Dc"] * (theta @ a + cs["params"]["b"].astype(np.float64))           # [G][J]
    p1, p0 = sigmoid(z).T, sigmoid(-z).T
    if items is not None:
        p1, p0 = p1[items], p0[items]
    return p1, p0, theta, logw


def host_tables(y, items, p1, p0, logw):
    """The float64 model tables and the integer tables of y over `items` (None: all)."""
    lw = lord_wingersky(p1, p0, logw)
    score = persons_oracle(y, None, items)
    o1, n = observed_oracle(y, items, score)
    return lw, o1, n, score


BOOKLET_SEED = 38
_BOOKLETS = {}


def booklet_case():
    """Two booklets over 20 items of a 2PL: booklet 0 = items 0 .. 13, booklet 1 = items 6 .. 19 (8 shared); each of 1 500 persons
    took one, the other booklet's own 6 items are 255: 30 % of the cells are missing by design and nobody is complete."""
    if not _BOOKLETS:
        rng = np.random.RandomState(BOOKLET_SEED)
        N, J = 1500, 20
        a = rng.uniform(0.7, 1.8, size=(1, J))
        b = rng.normal(0.0, 1.0, size=(1, J))
        x = rng.normal(size=(N, 1))
        y = (rng.uniform(size=(N, J)) < sigmoid(x @ a + b)).astype(np.uint8)
        took = rng.randint(0, 2, size=N)
        books = [np.arange(0, 14), np.arange(6, 20)]
        y[took == 0, 14:] = 255
        y[took == 1, :6] = 255
        _BOOKLETS.update({"name": "booklets_2pl_n1500_j20", "N": N, "J": J, "model": "irt_2pl", "D": 1, "Dc": 1.0, "nodes": 41,
                          "span": 6.0, "y": y, "took": took, "booklets": books,
                          "params": {"a": a.astype(np.float32), "b": b.astype(np.float32)}, "n_params": np.full(J, 2, np.int64)})
    return _BOOKLETS


DINA_CASE = ("sx2_dina_k3", 2000, 14, "dina", 3, 0.0, 41)             # a tests.score_cases.cdm_case: complete data
