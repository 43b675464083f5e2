"""The float64 oracle and the cases of the person-fit tests (tests/test_fit_host.py on the CPU, tests/test_gpu_fit.py on the GPU):
the seven sums per person and the four per item behind lz and the infit / outfit mean squares.

The oracle: the point estimate of every person comes from score_cases.irt_oracle / cdm_oracle (`mean`, `node`), P from
ld_cases.irt_prob / cdm_prob, Q = 1 - P (float64: harmless), and per observed cell (y < 2)

    lambda = log P - log Q    l = y ? log P : log Q    eps = P log P + Q log Q    nu = P Q lambda^2
    r2 = y ? Q^2 : P^2        w = P Q                  zeta = y ? Q / P : P / Q

summed over a person's answered items (n, l0, e, v, sr2, sw, sz2) and over an item's persons (n, sr2, sw, sz2), with the sums
of the absolute terms beside them (`abs`): the yardstick of the comparison rules.  lz = (l0 - e) / sqrt(v), outfit = sz2 / n,
infit = sr2 / sw.

Cases: all of ld_cases.ALL and one planted case, pf_2pl_n5000_j70_aberrant: 250 of its 5 000 persons, chosen with
RandomState(42), have their observed cells replaced by coin flips from the same generator.

The rules (C: FIT_C).  n exactly.  Every other sum S = sum t: |S - S64| <= C 2^-23 sum |t|.  lz: |lz - lz64| <= C u with
u = 2^-23 (sum |l| + sum |eps|) / sqrt(v), on the persons with oracle n >= 5 and v > 0.25 (lz_condition), which may leave out at
most LEFT_OUT_CAP of a case's persons.  infit and outfit, being quotients of sums of non-negative terms: relative error
<= C 2^-23 (terms summed), i.e. 2 C 2^-23 for infit (two sums) and C 2^-23 for outfit."""
import numpy as np

from tests import ld_cases as ld
from tests import score_cases as sc

U = 2.0 ** -23
# The constant of the rules: the next power of two above twice the largest ratio measured on one MI355X.  Over the eleven cases,
# at the ABI and end to end, the largest |S - S64| / (2^-23 sum |t|) is 3.16 (a person's sz2 in case3_1pl_j130, where Dc = 1.702
# and |z| reaches 13: a float32 z carries |z| 2^-24 into exp(z)) and the largest |lz - lz64| / u is 1.16; over the shape limits
# of tests/test_gpu_fit.py it is 3.74 (a person's sr2 over three items, the largest of 98 403 such sums).  2 x 3.74 < 8.
FIT_C = 8.0
MEASURED_MAX_RATIO = 3.74
COND_MIN_ITEMS = 5
COND_MIN_VAR = 0.25
LEFT_OUT_CAP = 0.05

PLANTED = ("pf_2pl_n5000_j70_aberrant", 5000, 70, "irt_2pl", 1, 1.0, 61, 0.20, (0.5, 1.5), 41)
PLANTED_SEED, PLANTED_PERSONS = 42, 250

ALL = list(ld.ALL) + [("irt", PLANTED)]
ALL_IDS = [c[0] for _, c in ALL]
PERSON = ("n", "l0", "e", "v", "sr2", "sw", "sz2")
ITEM = ("n", "sr2", "sw", "sz2")

_CASES, _ORACLES, _WHO = {}, {}, {}


def planted_persons():
    """The 250 planted persons (sorted indices)."""
    case_of("irt", PLANTED)
    return _WHO["who"]


def planted_case():
    cs = sc.irt_case(PLANTED)
    rng = np.random.RandomState(PLANTED_SEED)
    who = np.sort(rng.choice(cs["N"], size=PLANTED_PERSONS, replace=False))
    flips = (rng.uniform(size=(PLANTED_PERSONS, cs["J"])) < 0.5).astype(np.uint8)
    y = cs["y"]
    y[who] = np.where(y[who] < 2, flips, y[who])
    _WHO["who"] = who
    return cs


def case_of(kind, case):
    """The case, built once and shared; callers must not modify it."""
    if case[0] == PLANTED[0]:
        if PLANTED[0] not in _CASES:
            _CASES[PLANTED[0]] = planted_case()
        return _CASES[PLANTED[0]]
    return ld.case_of(kind, case)


def cell_terms(y, prob):
    """The per-cell terms [N][J] in float64, zero where the cell is not observed, and the mask."""
    m = y < 2
    one = y == 1
    P = np.asarray(prob, np.float64)
    Q = 1.0 - P
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lp, lq = np.log(P), np.log(Q)
        lam = lp - lq
        t = {"l0": np.where(one, lp, lq), "e": P * lp + Q * lq, "v": P * Q * lam * lam, "sr2": np.where(one, Q * Q, P * P),
             "sw": P * Q, "sz2": np.where(one, Q / P, P / Q)}
    t = {k: np.where(m, v, 0.0) for k, v in t.items()}
    t["n"] = m.astype(np.float64)
    return t, m


def sums(y, prob):
    """`person` and `item` sums, the sums of the absolute terms (`person_abs`, `item_abs`), and the statistics out of them."""
    t, _ = cell_terms(y, prob)
    o = {"person": {k: t[k].sum(1) for k in PERSON}, "person_abs": {k: np.abs(t[k]).sum(1) for k in PERSON},
         "item": {k: t[k].sum(0) for k in ITEM}, "item_abs": {k: np.abs(t[k]).sum(0) for k in ITEM}}
    o.update(stats(o["person"]))
    o["item_infit"], o["item_outfit"] = msq(o["item"])
    o["keep"] = lz_condition(o)
    return o


def msq(s):
    with np.errstate(divide="ignore", invalid="ignore"):
        infit = np.where((s["n"] > 0) & (s["sw"] > 0), s["sr2"] / s["sw"], np.nan)
        outfit = np.where(s["n"] > 0, s["sz2"] / s["n"], np.nan)
    return infit, outfit


def stats(p):
    """lz, infit, outfit of the persons from their sums (the formulas said independently of vipsy_amd.grid)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lz = np.where((p["n"] > 0) & (p["v"] > 0), (p["l0"] - p["e"]) / np.sqrt(p["v"]), np.nan)
    infit, outfit = msq(p)
    return {"lz": lz, "infit": infit, "outfit": outfit}


def lz_condition(o):
    """The persons on whom lz is compared: oracle n >= 5 and v > 0.25."""
    return (o["person"]["n"] >= COND_MIN_ITEMS) & (o["person"]["v"] > COND_MIN_VAR)


def prob_at(kind, cs, est, params=None):
    return ld.irt_prob(cs, est, params) if kind == "irt" else ld.cdm_prob(cs, est, params)


def oracle(kind, case):
    """The oracle of a case, computed once and shared (never modified): the point estimates (`theta_hat` float64 [N][D] or
    `pattern` [N]) and sums() at them."""
    key = case[0]
    if key not in _ORACLES:
        cs = case_of(kind, case)
        est = sc.irt_oracle(cs)["mean"] if kind == "irt" else sc.cdm_oracle(cs)["node"]
        o = sums(cs["y"], prob_at(kind, cs, est))
        o["theta_hat" if kind == "irt" else "pattern"] = est
        _ORACLES[key] = o
    return _ORACLES[key]


# ---- the rules -------------------------------------------------------------------------------------------------------------
def sum_ratios(got, want, want_abs, names):
    """{name: the largest |S - S64| / (2^-23 sum |t|)} over the entries with sum |t| > 0; where sum |t| = 0 the sum must be an
    exact zero (AssertionError otherwise).  n is not in it: it is compared exactly."""
    out = {}
    for k in names:
        if k == "n":
            continue
        g, w, a = np.asarray(got[k], np.float64), want[k], want_abs[k]
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.isfinite(g).all(), k
        dead = a == 0
        assert (g[dead] == 0).all(), k
        out[k] = float((np.abs(g - w)[~dead] / (U * a[~dead])).max()) if (~dead).any() else 0.0
    return out


def lz_ratio(lz, o):
    """The largest |lz - lz64| / u over the persons of the condition, u = 2^-23 (sum |l| + sum |eps|) / sqrt(v)."""
    keep = o["keep"]
    if not keep.any():
        return 0.0
    u = U * (o["person_abs"]["l0"] + o["person_abs"]["e"])[keep] / np.sqrt(o["person"]["v"][keep])
    assert np.isfinite(np.asarray(lz)[keep]).all()
    return float((np.abs(np.asarray(lz, np.float64)[keep] - o["lz"][keep]) / u).max())


def msq_ratios(infit, outfit, want_infit, want_outfit):
    """The largest relative errors of infit and outfit in units of 2^-23, over the finite oracle values; NaN must sit where the
    oracle has it."""
    out = []
    for g, w in ((infit, want_infit), (outfit, want_outfit)):
        g = np.asarray(g, np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w))
        ok = np.isfinite(w) & (w > 0)
        out.append(float((np.abs(g - w)[ok] / (U * w[ok])).max()) if ok.any() else 0.0)
    return out[0], out[1]




# ---- the sums said again in float32 ----------------------------------------------------------------------------------------
def restated_f32(kind, case, made=None):
    """A plain float32 numpy restatement of what the kernels do: the estimates and the item parameters in float32; z, exp, log and
    every term of a cell in float32, Q formed on its own (sigmoid of the negated argument; (1 - d) + (d - c) sigmoid(-z)); what
    belongs to an ITEM alone -- the asymptotes c, d - c and 1 - d of 3PL / 4PL, the two sets of terms of a DINA / DINO item --
    from float64 (a float's rounding of them is the same in every cell of the item and adds up in its sums instead of averaging
    out); a person's sums by numpy's float32 sum over the items, an item's as float32 partials over 32 persons added in
    float64 and rounded once.  Returns `person`, `item` (float32) and the statistics in float64 out of them.  made: a ready-made
    (cs, estimates) in place of the case's own and its oracle's (tests/steep_cases.py)."""
    if made is None:
        cs, o = case_of(kind, case), oracle(kind, case)
    else:
        cs, o = made[0], {"theta_hat" if kind == "irt" else "pattern": made[1]}
    f4, f8 = np.float32, np.float64
    y = cs["y"]
    m, one = y < 2, y == 1
    p = cs["params"]
    sig = lambda v: (f4(1) / (f4(1) + np.exp(-v.astype(f4)))).astype(f4)                      # noqa: E731
    sig8 = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, f8)))                                 # noqa: E731
    if kind == "irt":
        th = o["theta_hat"].astype(f4)
        b = p["b"].astype(f4).reshape(1, -1)
        z = (f4(cs["Dc"]) * ((th + b) if cs["model"] == "irt_1pl" else (th @ p["a"].astype(f4) + b)).astype(f4)).astype(f4)
        if cs["model"] in ("irt_3pl", "irt_4pl"):
            four = cs["model"] == "irt_4pl"
            c = sig8(p["c"].reshape(1, -1))
            omd = sig8(-p["d"].reshape(1, -1)) if four else 0.0
            dmc = sig8(p["d"].reshape(1, -1)) - c if four else sig8(-p["c"].reshape(1, -1))
            P = (c + dmc * sig(z).astype(f8)).astype(f4)
            Q = (omd + dmc * sig(-z).astype(f8)).astype(f4)
            lp, lq = np.log(P).astype(f4), np.log(Q).astype(f4)
            lam = (lp - lq).astype(f4)
        else:
            P, Q = sig(z), sig(-z)
            sp = lambda v: (np.maximum(v, f4(0)) + np.log1p(np.exp(-np.abs(v)))).astype(f4)   # noqa: E731
            lp, lq = (-sp(-z)).astype(f4), (-sp(z)).astype(f4)
            lam = z
        with np.errstate(over="ignore"):
            t = {"l0": np.where(one, lp, lq), "e": (P * lp + Q * lq).astype(f4), "v": (P * Q * lam * lam).astype(f4),
                 "sr2": np.where(one, Q * Q, P * P).astype(f4), "sw": (P * Q).astype(f4), "sz2": np.where(one, Q / P, P / Q).astype(f4)}
    else:
        t8, _ = cell_terms(y, ld.cdm_prob(cs, o["pattern"]))
        t = {k: v.astype(f4) for k, v in t8.items()}
    t["n"] = m.astype(f4)
    t = {k: np.where(m, v, f4(0)).astype(f4) for k, v in t.items()}
    pad = (-len(y)) % 32
    units = lambda v: np.concatenate([v, np.zeros((pad, v.shape[1]), f4)]).reshape(-1, 32, v.shape[1])     # noqa: E731
    out = {"person": {k: t[k].sum(1, dtype=f4) for k in PERSON},
           "item": {k: units(t[k]).sum(1, dtype=f4).astype(f8).sum(0).astype(f4) for k in ITEM}}
    out.update(stats({k: v.astype(f8) for k, v in out["person"].items()}))
    out["item_infit"], out["item_outfit"] = msq({k: v.astype(f8) for k, v in out["item"].items()})
    return out

