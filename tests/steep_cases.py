"""The cases, the oracle and the rules of the steep-parameter tests (tests/test_steep_host.py on the CPU, tests/test_gpu_steep.py
on the GPU): the grid family on item parameters as an unpenalised fit_em() leaves them -- slopes of 2.5 to 4.5 at Dc = 1.702,
asymptote logits of -12 / -20 (c = 6e-6 / 2e-9, the latter below eps32) and +12 / +20, guess / slip logits of -9, -14 and -20.
Tuples as in tests/score_cases.py; parameters are drawn, never trained.

Three things happen there that the mild cases never meet.  (1) The tables of k_grid_table_* sit on their clamp (z at +-15.94, P
and Q at eps32) on a large share of their cells and a posterior lives on two or three nodes: irt_condition is WAIVED for this
whole file on purpose (CONDITION_WAIVED) -- it is about what the quadrature means, not about what the kernels compute -- and
test_steep_host.py asserts the opposite, that the cases are saturated.  (2) The diagnostics (k_fit_irt, k_pair_*, k_point_irt)
do not clamp: at a person on the bound +-6 |z| reaches 41 in one dimension and passes 110 in three, and the rounding of z
itself, which the yardstick 2^-23 sum |t| of fit_cases / point_cases does not contain, becomes the largest error.  (3) Beyond
|z| = 87 sigmoid(-|z|) is no float32 any more (steep_3pl_d3 and its twins).

The oracle forms Q on its own (Q = (1 - d) + (d - c) sigmoid(-z), 1 - d = sigmoid(-d_un)): fit_cases.cell_terms' Q = 1 - P is
harmless in float64 only up to |z| = 30 or so.

The extended yardstick.  The kernels form z as b, then D fmas, then the product with Dc: D + 1 roundings (1PL: 2), each at most
2^-24 of a partial that z_abs = Dc (|b| + sum_d |theta_d a_jd|) bounds, so |dz| <= (D + 1) 2^-24 z_abs.  With P' = dP/dz = P_z =
(d - c) sigmoid(z) sigmoid(-z), Q' = -P_z and lambda = log P - log Q the terms move by

    l     y ? P_z / P : -P_z / Q                     r2    y ? -2 Q P_z : 2 P P_z             w   P_z (Q - P)
    zeta  y ? -P_z / P^2 : P_z / Q^2                 eps   P_z lambda                          nu  P_z ((Q - P) lambda^2 + 2 lambda)
    w_pt = P_z^2 / (P Q)   (the information's cell)        w_pt (2 (sigmoid(-z) - sigmoid(z)) - P_z (Q - P) / (P Q))

a unit of z (for 1PL / 2PL: Q or P, zeta itself, 2 w Q or 2 w P, w lambda), all from the oracle's own float64 P and Q, and
    Y = sum |t| + 2^23 sum |dt/dz| |dz|
takes the place of sum |t| in |S - S64| <= C 2^-23 Y.  Two more roundings belong to it, found when the float32 restatement missed
C / 2 under the above alone (tests/test_steep_host.py holds it to that).  The kernels take Dc as a float: (float)Dc differs from
Dc by up to 2^-24 of it (1.702: 0.22 x 2^-24), a relative error of z itself, added to |dz|.  And the 3PL / 4PL cell takes the
logarithm of a P (a Q) that was rounded to float32 in two fmas: log P and log Q carry an ABSOLUTE 2^-23, whatever their size --
a person on the bound has sum |l| = 2e-7 over 34 answers and a float32 P = 1 - k 2^-24 -- so a 3PL / 4PL cell adds 2^-23 to the
yardsticks of l and of eps (P + Q = 1 times it) and 4 w |lambda| 2^-23 to that of nu (lambda carries both).  The 1PL / 2PL cell
forms its logarithms from exp(-|z|) directly and has no such term.  C stays FIT_C / POINT_C.  The DINA / DINO cells have no z to round (their
terms are made in double once an item): Y is sum |t| there.

Every case and oracle is computed once and shared; callers must not modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import corner_cases as co
from tests import fit_cases as fc
from tests import ld_cases as ld
from tests import point_cases as pc
from tests import score_cases as sc

U = 2.0 ** -23
F32_MAX = float(np.finfo(np.float32).max)
# What float32 cannot hold at all: a term below the smallest normal float is lost (the hardware exp2, rcp and log2 flush, and a
# product of two small factors underflows), whatever its size relative to the sum.  A cell goes through at most four such
# operations, so every observed cell adds 4 x 1.18e-38 to Y (in units of 2^-23: times 2^23).  It matters only where a whole sum
# is that small -- the information of a person on the bound of steep_4pl_d3 is 1e-58 in float64 and 0 in float32.
FLOOR23 = 4.0 * float(np.finfo(np.float32).tiny) * 2.0 ** 23
LOG_EPS32 = float(np.log(vo.EPS32))                   # -15.94: the clamp of the tables
NOBODY, ALL_CORRECT, ALL_WRONG, ABERRANT = 0, 1, 2, 3  # the planted persons of every IRT case (the first three as point_cases)

# name, N, J, model, D, Dc, nodes per dimension, missing rate, slope range, seed
TABLE_IRT = [
    ("sat_2pl_steep", 100, 40, "irt_2pl", 1, 1.702, 61, 0.1, (2.5, 4.0), 401),
    # (seed 412, not 402: under 402 one person with one correct answer of 40 alternates under the capped step in float64 and
    # ends in max_iter, 1 of 99 -- above MAX_ITER_CAP, which a 2PL case is held to; under 412 nobody does)
    ("sat_2pl_steep_d2", 100, 40, "irt_2pl", 2, 1.702, 21, 0.0, (2.0, 3.0), 412),
    ("sat_3pl_asym", 129, 40, "irt_3pl", 1, 1.702, 61, 0.1, (1.5, 3.0), 403),
    # (slopes of 2.0 to 3.5, not 1.5 to 3.0: a 4PL item whose asymptotes are both above eps32 never meets the clamp, and at 1.5 to
    # 3.0 only 13 % of the case's table positions are on it; test_steep_host.py asks for 15 %)
    ("sat_4pl_asym", 129, 40, "irt_4pl", 1, 1.702, 61, 0.1, (2.0, 3.5), 404),
]
# name, N, J, cdm, K, missing rate, seed.  (Seed 416: 0 % of the persons are left out by the node rule; the cap is 2 %.)
DINA = ("sat_dina_k5", 100, 30, "dina", 5, 0.1, 416)
TABLE_CASES = TABLE_IRT + [DINA]
TABLE_IDS = [c[0] for c in TABLE_CASES]
# fit, pairs and point only: beyond float32.  The slopes put the all-correct person at (6, 6, 6) past z = 110 on most items.
D3 = ("steep_3pl_d3", 129, 40, "irt_3pl", 3, 1.702, 9, 0.0, (3.0, 4.5), 406)
D3_TWINS = [("steep_2pl_d3",) + D3[1:3] + ("irt_2pl",) + D3[4:], D3, ("steep_4pl_d3",) + D3[1:3] + ("irt_4pl",) + D3[4:]]
IRT_CASES = TABLE_IRT + D3_TWINS
IRT_IDS = [c[0] for c in IRT_CASES]
CONDITION_WAIVED = tuple(IRT_IDS)                     # irt_condition: waived for every case of this file, see above
ASYM_LOGITS = (12.0, 20.0)                            # |c_un|, d_un of the items in turn
DINA_LOGITS = (-9.0, -14.0, -20.0)
Z_BEYOND = 110.0                                      # steep_3pl_d3: z of the all-correct person at the bound, on >= 4 items
ESTIMATES = ("eap", "ml")
# The D = 3 twins a third time: fisher64 (and the kernel) stop a person as at_bound as soon as ONE coordinate sits on the bound, so
# from the EAP nobody reaches the corner, where the likelihood of the all-correct person has its supremum and z passes 110.
# "corner" is the ml estimate with the all-correct and the aberrant person put at (6, 6, 6) and the all-wrong one at (-6, -6, -6):
# the aberrant person's wrong answers there have odds beyond the largest float32.
CORNER = "corner"
BAND = (87.0, 88.8)                                   # exp(-|z|) is subnormal, the odds not yet beyond float32: no wrong answer may sit here

_MADE, _EST, _RUN = {}, {}, {}


def _plant(y):
    """Nobody, all correct, all wrong, and one aberrant person whose observed answers are the complement of the row simulated
    for them."""
    y[ABERRANT] = np.where(y[ABERRANT] < 2, 1 - y[ABERRANT], y[ABERRANT])
    y[NOBODY], y[ALL_CORRECT], y[ALL_WRONG] = 255, 1, 0


def _irt(case):
    name, N, J, model, D, Dc, nodes, missing, slopes, seed = case
    src = D3 if case in D3_TWINS else case
    cs = sc.irt_case(src)                                           # the draw of a, b (and of mild asymptotes)
    p = {k: v.copy() for k, v in cs["params"].items()}
    rng = np.random.RandomState(seed + 1000 + {"irt_2pl": 0, "irt_3pl": 1, "irt_4pl": 2}[model])
    if case in D3_TWINS:
        if model == "irt_2pl":
            p.pop("c")
        if model == "irt_4pl":
            p["d"] = sc._logit(rng.uniform(0.85, 0.98, size=(1, J))).astype(np.float32)
    else:
        turn = np.where(np.arange(J) % 2 == 0, ASYM_LOGITS[0], ASYM_LOGITS[1]).astype(np.float32)[None, :]
        if "c" in p:
            p["c"] = -turn
        if "d" in p:
            p["d"] = turn.copy()
    cs = dict(cs, name=name, model=model, params=p)
    # the responses again, from the final parameters
    x = rng.normal(size=(N, D))
    y = (rng.uniform(size=(N, J)) < probs(cs, x)[0]).astype(np.uint8)
    if missing > 0:
        y[rng.uniform(size=(N, J)) < missing] = 255
    _plant(y)
    cs["y"] = y
    return cs


def _dina(case):
    name, N, J, cdm, K, missing, seed = case
    cs = sc.cdm_case(case)                                          # its Q-matrix
    rng = np.random.RandomState(seed + 1000)
    p = {"g": rng.choice(DINA_LOGITS, size=(1, J)).astype(np.float32), "s": rng.choice(DINA_LOGITS, size=(1, J)).astype(np.float32)}
    eta_all, _ = vo.dina_eta(K, cs["q"].astype(np.float64))
    eta = eta_all[rng.randint(0, 2 ** K, size=N)]
    g, s = vo.sigmoid(p["g"].astype(np.float64)), vo.sigmoid(p["s"].astype(np.float64))
    y = (rng.uniform(size=(N, J)) < np.where(eta > 0, 1 - s, g)).astype(np.uint8)
    y[:, K:][rng.uniform(size=(N, J - K)) < missing * J / (J - K)] = 255       # (sc.cdm_case: the identifying items stay)
    return dict(cs, params=p, y=y)


def made(case):
    """(cs, kind) of a case, as corner_cases.oracle_of takes it ready-made."""
    if case[0] not in _MADE:
        _MADE[case[0]] = (_dina(case), "cdm") if len(case) == 7 else (_irt(case), "irt")
    return _MADE[case[0]]


def table_oracle(case):
    return co.oracle_of(case, made(case))


def clamp_share(o):
    """The share of the (item, node) positions whose T1 or T0 lies within 1e-3 of the clamp log eps32."""
    return float(((np.abs(o["T1"] - LOG_EPS32) <= 1e-3) | (np.abs(o["T0"] - LOG_EPS32) <= 1e-3)).mean())


# ---- P and Q, each on its own ----------------------------------------------------------------------------------------------
def probs(cs, theta):
    """P, Q, P_z, sigmoid(z) - sigmoid(-z) ... of an IRT case at theta [n][D] in float64: (P, Q, pz, sg, sn, z, z_abs, k) with k the
    number of roundings of z."""
    a, b, lo, hi = pc._params(cs)
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    omd = vo.sigmoid(-f8(cs["params"]["d"])).reshape(1, -1) if cs["model"] == "irt_4pl" else 0.0
    dmc = hi - lo
    if cs["model"] == "irt_3pl":
        dmc = vo.sigmoid(-f8(cs["params"]["c"])).reshape(1, -1)
    th = f8(theta).reshape(len(theta), cs["D"])
    Dc = float(cs["Dc"])
    z = Dc * (th @ a + b)
    z_abs = Dc * (np.abs(th) @ np.abs(a) + np.abs(b))
    with np.errstate(over="ignore"):
        sg, sn = vo.sigmoid(z), vo.sigmoid(-z)
    return lo + dmc * sg, omd + dmc * sn, dmc * sg * sn, sg, sn, z, z_abs, (2 if cs["model"] == "irt_1pl" else cs["D"] + 1)


def dz23(cs, z, z_abs, k):
    """2^23 |dz|: k roundings of 2^-24 z_abs, and the float32 the kernels take Dc as, a relative error of z itself."""
    Dc = float(cs["Dc"])
    return k * 0.5 * z_abs + np.abs(z) * (abs(float(np.float32(Dc)) - Dc) / Dc * 2.0 ** 23)


def cdm_probs(cs, pattern):
    p = cs["params"]
    eta_all, _ = (vo.dino_eta if cs["cdm"] == "dino" else vo.dina_eta)(cs["K"], np.asarray(cs["q"], np.float64))
    on = eta_all[np.asarray(pattern, np.int64)] > 0
    g_un, s_un = np.asarray(p["g"], np.float64).reshape(1, -1), np.asarray(p["s"], np.float64).reshape(1, -1)
    return np.where(on, vo.sigmoid(-s_un), vo.sigmoid(g_un)), np.where(on, vo.sigmoid(s_un), vo.sigmoid(-g_un))


def fit_sums(kind, cs, est, y=None):
    """fit_cases.sums with Q on its own and the extended yardstick: `person`, `item`, `person_abs` / `item_abs` (Y as the module
    docstring has it), `plain_abs` (sum |t| alone, persons), the statistics, `keep`, and `over_person` / `over_item`: who holds an
    answer whose float64 odds exceed the largest float32."""
    y = cs["y"] if y is None else y
    m, one = y < 2, y == 1
    if kind == "irt":
        P, Q, pz, sg, sn, z, z_abs, k = probs(cs, est)
        dz = dz23(cs, z, z_abs, k)
        rho = 1.0 if cs["model"] in ("irt_3pl", "irt_4pl") else 0.0
    else:
        P, Q = cdm_probs(cs, est)
        pz, dz, rho = np.zeros_like(P), 0.0, 0.0
    # (the logarithm of the larger of P and Q through log1p of the other: np.log(1 - 1e-11) is good to 1e-5 of itself only)
    with np.errstate(divide="ignore", invalid="ignore"):            # (the branch np.where does not take)
        lp, lq = np.where(P > 0.5, np.log1p(-Q), np.log(P)), np.where(Q > 0.5, np.log1p(-P), np.log(Q))
    lam = lp - lq
    t = {"l0": np.where(one, lp, lq), "e": P * lp + Q * lq, "v": P * Q * lam * lam, "sr2": np.where(one, Q * Q, P * P), "sw": P * Q,
         "sz2": np.where(one, Q / P, P / Q)}
    d = {"l0": np.where(one, pz / P, pz / Q), "e": pz * lam, "v": pz * ((Q - P) * lam * lam + 2.0 * lam),
         "sr2": np.where(one, 2.0 * Q * pz, 2.0 * P * pz), "sw": pz * (Q - P), "sz2": np.where(one, pz / (P * P), pz / (Q * Q))}
    over = m & (t["sz2"] > F32_MAX)
    t = {k_: np.where(m, v, 0.0) for k_, v in t.items()}
    ext = {k_: np.where(m, np.abs(v) * dz, 0.0) for k_, v in d.items()}
    for k_, v in (("l0", 1.0), ("e", 1.0), ("v", 4.0 * P * Q * np.abs(lam))):
        ext[k_] = ext[k_] + np.where(m, rho * v, 0.0)
    ext = {k_: v + np.where(m, FLOOR23, 0.0) for k_, v in ext.items()}
    t["n"], ext["n"] = m.astype(np.float64), np.zeros(y.shape)
    o = {"person": {k_: t[k_].sum(1) for k_ in fc.PERSON}, "item": {k_: t[k_].sum(0) for k_ in fc.ITEM},
         "plain_abs": {k_: np.abs(t[k_]).sum(1) for k_ in fc.PERSON},
         "person_abs": {k_: (np.abs(t[k_]) + ext[k_]).sum(1) for k_ in fc.PERSON},
         "item_abs": {k_: (np.abs(t[k_]) + ext[k_]).sum(0) for k_ in fc.ITEM},
         "over_person": over.any(1), "over_item": over.any(0)}
    o.update(fc.stats(o["person"]))
    o["item_infit"], o["item_outfit"] = fc.msq(o["item"])
    o["keep"] = fc.lz_condition(o)
    return o


def fit_ratios(person, item, o):
    """The rules of tests/test_gpu_fit.py under the extended yardstick, for sums {name: float64 numpy}: n exactly; every sum
    |S - S64| / (2^-23 Y); where a person or an item holds an answer whose float64 odds exceed the largest float32, sz2 (and
    nothing else) must be +inf and is not compared; lz against 2^-23 (Y_l0 + Y_e) / sqrt(v) on the persons of the condition;
    infit and outfit relative to 2^-23 (Y_sr2 / sr2 + Y_sw / sw) and 2^-23 Y_sz2 / sz2.  Returns {name: largest ratio}, every one
    to be held against FIT_C."""
    from vipsy_amd.grid import item_msq_host, person_fit_host
    out = {}
    for tag, got, want, Y, over, names in (("", person, o["person"], o["person_abs"], o["over_person"], fc.PERSON),
                                           ("item ", item, o["item"], o["item_abs"], o["over_item"], fc.ITEM)):
        assert np.array_equal(got["n"], want["n"]), tag
        for k in names[1:]:
            g = np.asarray(got[k], np.float64)
            skip = over if k == "sz2" else np.zeros(len(g), bool)
            assert (g[skip] == np.inf).all(), (tag, k, "odds beyond float32 must come back as +inf", g[skip])
            assert np.isfinite(g[~skip]).all(), (tag, k, np.flatnonzero(~np.isfinite(g) & ~skip)[:10])
            dead = Y[k] == 0
            assert (g[dead] == 0).all(), (tag, k)
            ok = ~dead & ~skip
            out[tag + k] = float((np.abs(g - want[k])[ok] / (U * Y[k][ok])).max()) if ok.any() else 0.0
    clean = ~o["over_person"]
    pf = person_fit_host({k: np.where(clean, v, 0.0) if k == "sz2" else v for k, v in person.items()})
    keep = o["keep"]
    assert np.array_equal(np.isnan(pf["lz"]), np.isnan(o["lz"]))
    assert np.isfinite(pf["lz"][keep]).all()
    u = U * (o["person_abs"]["l0"] + o["person_abs"]["e"])[keep] / np.sqrt(o["person"]["v"][keep])
    out["lz"] = float((np.abs(pf["lz"][keep] - o["lz"][keep]) / u).max()) if keep.any() else 0.0
    im = item_msq_host({k: np.where(o["over_item"], 0.0, v) if k == "sz2" else v for k, v in item.items()})
    for tag, got, want, s, Y, skip in (("", pf, o, o["person"], o["person_abs"], ~clean),
                                       ("item ", {"infit": im["infit"], "outfit": im["outfit"]},
                                        {"infit": o["item_infit"], "outfit": o["item_outfit"]}, o["item"], o["item_abs"], o["over_item"])):
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = {"infit": U * (Y["sr2"] / s["sr2"] + Y["sw"] / s["sw"]), "outfit": U * Y["sz2"] / s["sz2"]}
        for k in ("infit", "outfit"):
            g, w = np.asarray(got[k], np.float64), want[k]
            ok = np.isfinite(w) & (w > 0) & ~(skip if k == "outfit" else np.zeros(len(w), bool))
            assert np.array_equal(np.isnan(g[ok]), np.isnan(w[ok])) and np.isnan(g[np.isnan(w)]).all(), (tag, k)
            out[tag + k] = float((np.abs(g - w)[ok] / (w[ok] * rel[k][ok])).max()) if ok.any() else 0.0
    return out


def point_info_ratio(cs, got, y=None):
    """|I - I64| / (2^-23 Y) of a point result (as point_cases.ratios takes it) under the extended yardstick, the largest over the
    persons with an answer; and the same under the plain yardstick sum |terms|."""
    y = cs["y"] if y is None else y
    some = (y < 2).any(1)
    th = np.where(some[:, None], np.asarray(got["theta_hat"], np.float64), 0.0)
    P, Q, pz, sg, sn, z, z_abs, k = probs(cs, th)
    a = pc._params(cs)[0]
    m = y < 2
    w = np.where(m, pz * pz / (P * Q), 0.0)
    dw = np.where(m, np.abs(w * (2.0 * (sn - sg) - pz * (Q - P) / (P * Q))) * dz23(cs, z, z_abs, k), 0.0)
    Dc2 = float(cs["Dc"]) ** 2
    info = Dc2 * np.einsum("nj,dj,ej->nde", w, a, a)
    plain = Dc2 * np.einsum("nj,dj,ej->nde", w, np.abs(a), np.abs(a))
    Y = plain + Dc2 * np.einsum("nj,dj,ej->nde", dw + np.where(m, FLOOR23, 0.0), np.abs(a), np.abs(a))
    ig = np.asarray(got["info"], np.float64)
    assert np.isfinite(ig[some]).all()
    err = np.abs(ig - info)[some]
    ok = Y[some] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return (float((err[ok] / (U * Y[some][ok])).max()) if ok.any() else 0.0,
                float(np.where(plain[some] > 0, err / (U * plain[some]), 0.0).max()))


# ---- the estimates the diagnostics are fed ---------------------------------------------------------------------------------
def eap_of(case):
    if case[0] not in _EST:
        cs, _ = made(case)
        _EST[case[0]] = table_oracle(case)["post"]["mean"] if case in TABLE_IRT else sc.irt_oracle(cs)["mean"]
    return _EST[case[0]]


def fisher(case, method, exact=True):
    """point_cases.fisher64 from the oracle's EAP: exact, the oracle's own root (60 steps, tol 1e-12, as point_cases.root_of); not
    exact, the method as the kernel is asked to run it (MAX_ITER evaluations, tol TOL) -- the status counts a kernel is held to."""
    key = (case[0], method, exact)
    if key not in _RUN:
        cs, _ = made(case)
        kw = {} if exact else {"max_iter": pc.MAX_ITER, "tol": pc.TOL}
        _RUN[key] = pc.fisher64(cs, method, eap_of(case), **kw)
    return _RUN[key]


def estimate(case, which):
    """float32 [N][D]: the oracle's EAP, or fisher64's ml estimate with the EAP where it has none (empty, singular), as at=
    documents it."""
    eap = eap_of(case)
    if which == "eap":
        return np.ascontiguousarray(eap, np.float32)
    r = fisher(case, "ml")
    bad = (r["status"] == pc.EMPTY) | (r["status"] == pc.SINGULAR)
    est = np.ascontiguousarray(np.where(bad[:, None], eap, r["theta_hat"]), np.float32)
    if which == CORNER:
        est[[ALL_CORRECT, ABERRANT]], est[ALL_WRONG] = sc.SPAN, -sc.SPAN
    return est


def corner_start(case):
    """The oracle's EAP with the all-correct person started at (6, 6, 6) and the all-wrong one at (-6, -6, -6): the first
    evaluation of vx_grid_point_irt is at the corner."""
    th0 = np.ascontiguousarray(eap_of(case), np.float32)
    th0[ALL_CORRECT], th0[ALL_WRONG] = sc.SPAN, -sc.SPAN
    return th0


def estimates_of(case):
    return ESTIMATES + ((CORNER,) if case in D3_TWINS else ())


def pairs_oracle(cs, est):
    """ld_cases' tables, q3 and condition at the estimates given (float32 taken as they are)."""
    o = ld.tables(cs["y"], probs(cs, np.asarray(est, np.float64))[0])
    o["q3"], o["v"] = ld.q3_of_tables(o)
    o["keep"] = ld.condition(o)
    return o


# ---- whose status a float32 method is held to ------------------------------------------------------------------------------
# STATUS_WAIVED, the one exemption of the status rules on the D = 3 twins, named as CONDITION_WAIVED is.  A person's status is not
# compared with fisher64's where, by the oracle alone,
#   - fisher64 itself ends the person max_iter (the capped step alternates; where it stands after 64 evaluations is not a
#     property of the method), or
#   - the float64 information at fisher64's own last point has a condition number above 2^23: a float32 Cholesky factor cannot
#     resolve such a matrix, and beyond 2^53 fisher64's verdict is rounding noise itself, or
#   - fisher64's own status changes when its start is rounded to float32 or moved by one float32 spacing (x (1 +- 2^-23)): two
#     persons of steep_2pl_d3 walk 34 capped steps to the bound and end at_bound or max_iter depending on that rounding.
# Off the waiver the twins are held to the issue's rules: under ml the at_bound persons are exactly fisher64's, nobody is singular
# whom fisher64 is not, the converged count is not below fisher64's by more than fisher64's own max_iter count.  (Which persons
# end max_iter is not compared: a person fisher64 converges at its 59th or 64th evaluation with |s| = 0.99 tol -- there are such
# -- may need a 65th in float32; the count condition is the issue's answer to that.)
STATUS_COND_LIMIT = 2.0 ** 23


def status_waived(cs, asked, method="ml", start=None):
    """bool [N]: the persons STATUS_WAIVED exempts, from fisher64 alone.  asked: its result from `start` (float64 [N][D]; None:
    the stability clause is not evaluated) with MAX_ITER evaluations and tol TOL."""
    th = np.where(np.isfinite(asked["theta_hat"]), asked["theta_hat"], 0.0)
    info = pc.evaluate(cs, th, method)["info"]
    if method == "map":
        info = info + np.eye(cs["D"])[None]
    ev = np.linalg.eigvalsh(np.where(np.isfinite(info), info, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
    out = (asked["status"] == pc.MAX_ITERS) | ((cond > STATUS_COND_LIMIT) & (asked["status"] != pc.EMPTY))
    if start is not None:
        s0 = np.asarray(start, np.float64)
        for th0 in (s0.astype(np.float32).astype(np.float64), s0 * (1.0 + U), s0 * (1.0 - U)):
            out |= pc.fisher64(cs, method, th0, max_iter=pc.MAX_ITER, tol=pc.TOL)["status"] != asked["status"]
    return out


def status_differences(got_status, asked, waived, method="ml"):
    """The persons, not waived, on whom a result breaks the rules above: at_bound other than in fisher64 (ml), or singular where
    fisher64 is not."""
    g, a = np.asarray(got_status), asked["status"]
    bad = (g == pc.SINGULAR) & (a != pc.SINGULAR)
    if method == "ml":
        bad |= (g == pc.AT_BOUND) != (a == pc.AT_BOUND)
    return np.flatnonzero(bad & ~waived)
