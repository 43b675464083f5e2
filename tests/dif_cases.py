"""The float64 oracle and the cases of the DIF tests (tests/test_dif_host.py on the CPU, tests/test_gpu_dif.py on the GPU):
vx_grid_counts_cond -- the expected counts under a tilt a person, a table set a segment of the persons -- behind
expected_counts(covariates=), group_counts() and dif().

The oracle is a few lines over its neighbours: the conditioned E-step of tests/pop_cases.py (estep_tilt: f = ll + lw + tilt . theta,
logjoint), a segment at a time through tests/count_cases.py (counts: the max-shifted softmax and the two indicator products), its
fit_stats a group against the pooled prob, pop_cases.em for the private latent regression of dif(impact=True) on group dummies,
and the Newton M-step of tests/em_cases.py a group for dif(refit=True).

THE RULE.  Tables are held to the float64 oracle by the project's row metric (_row_errors, floor 1: one row = one item of one
segment; mass one row a segment), the proportions (rmsd, md, observed where the cell has mass) absolutely.  The bound is not a
round number: restated() says the METHOD again in numpy -- the operand image as fp16 pairs of T 2^10, float32 ll, f and
log-sum-exp, p 2^14 split into an fp16 head and remainder, float32 sums over the persons of a segment in their order -- and its
worst row error against float64 ON THE CASE AT HAND is what float32 and the fp16 pairs cost there whatever the code does (it
grows with the cells a person answered: 2e-7 on one item, 8e-6 on 300 dense ones).  The rule of a case is rule_of(that) = C_RULE
times it, the restatement counted as no better than RULE_FLOOR = 2^-20.  observed = n1 / n is held to the rule as it reaches a
ratio (ratio_errors).  C_RULE = 8: the restatement rounds exp and log correctly and adds in the written order, where the
kernel uses the hardware's exp2 / log2 (1 ulp each, and the product with log2 e before them), a hardware sum order inside an
MFMA and across slabs, and a logjoint that comes from another kernel's log-sum-exp -- each of the size of the terms the
restatement already has, so a small multiple of it; the row rule of the unconditioned kernel (3e-5 over a restatement of 3.4e-6)
keeps the same margin.  tests/test_dif_host.py checks that the restatement stays within a third of RULE on every case.

Kernel cases (K*): drawn 2PL items and responses, a drawn tilt (a segment's own offset plus person noise), Sigma = 0.64 I for
the log-weights; the rows of every case are a permutation, so the segments hold shuffled rows.  Shapes: segments of 1, 31, 33,
255, 0 (empty, between two others), 257, 600 and 1 100 persons in one call (boundaries inside a 32-person unit and inside a
256-person round; the last segment takes two chunks), D = 1, 2, 3, G = 61, 33, 529 (17 node tiles: nine node groups), J = 1, 37,
300 (two item tiles a wave) and 530 (four, one node tile a workgroup), 30 % and 90 % missing, a person with no response.

The planted case: 4 096 persons, 8 2PL items, two groups at -0.75 / +0.75 with sd 0.8, 20 % missing, item PLANT_ITEM of group 1
shifted by 0.8 in b, fixed seed.  Everything here is computed once and shared; callers must not modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import em_cases as ec
from tests import pop_cases as pc
from tests import score_cases as sc
from tests.test_gpu_response_designs import ROW_TOL, _row_errors       # noqa: F401  (3e-5: the rule of the refit comparison)

C_RULE = 8.0
RULE_FLOOR = 2.0 ** -20       # sixteen float32 ulp: no case's method counts as better than this (a one-item case rounds almost nothing)
KSIGMA = 0.64                 # the population variance behind the kernel cases' log-weights
LOGP_MISSING = np.float32(-1.1920928244535389e-07)       # VX_LOGP_MISSING (vipsy_amd/csrc/vx_common.h)

# name: segment sizes, J, D, nodes a dimension (or ("explicit", G)), missing rate, seed
KCASES = {
    "K1": ((1, 31, 33, 255, 0, 257, 600, 1100), 37, 1, 61, 0.30, 71),
    "K2": ((40, 300, 7), 37, 2, 23, 0.30, 72),
    "K3": ((33, 0, 95), 37, 3, ("explicit", 33), 0.30, 73),
    "K4": ((100, 60), 530, 1, 61, 0.90, 74),
    "K5": ((300, 1, 212), 300, 1, 33, 0.30, 75),
    "K6": ((31, 33), 1, 1, 33, 0.30, 76),
}
BITWISE = ("K1", "K5", "K4")          # one case for each template instance: IT = 1, 2, 4
NO_RESPONSE = {"K1": 400}             # a batch position (in the segment of 257) whose row answers nothing

_K = {}


def kcase(key):
    """The drawn kernel case: an engine case (name, N, J, model, D, Dc, nodes, span, y, params) with theta [G][D], lw [G] float32,
    tilt [N][D] float32 by batch position, rows int64 [N] (a permutation) and seg_start int64 [S + 1]."""
    if key not in _K:
        from vipsy_amd.grid import population_logw, score_grid
        segs, J, D, nodes, missing, seed = KCASES[key]
        rng = np.random.RandomState(seed)
        N = int(sum(segs))
        a = rng.uniform(0.5, 1.5, size=(D, J))
        if D > 1:
            a = a * vo.default_a_free(D, J)
        params = {"a": a.astype(np.float32), "b": rng.normal(0.0, 1.0, size=(1, J)).astype(np.float32)}
        x = rng.normal(size=(N, D))
        y = (rng.uniform(size=(N, J)) < vo.sigmoid(x @ a + params["b"])).astype(np.uint8)
        y[rng.uniform(size=(N, J)) < missing] = 255
        if isinstance(nodes, tuple):
            theta = rng.uniform(-3.0, 3.0, size=(nodes[1], D)).astype(np.float32)
            nodes = (theta, np.zeros(nodes[1], np.float32))
        else:
            theta, _ = score_grid(D, nodes, sc.SPAN)
        rows = rng.permutation(N).astype(np.int64)
        seg_start = np.concatenate([[0], np.cumsum(segs)]).astype(np.int64)
        if key in NO_RESPONSE:
            y[rows[NO_RESPONSE[key]]] = 255
        off = rng.uniform(-1.2, 1.2, size=(len(segs), D))
        tilt = (np.repeat(off, segs, axis=0) + 0.1 * rng.normal(size=(N, D))).astype(np.float32)
        _K[key] = {"name": "dif_%s" % key.lower(), "N": N, "J": J, "model": "irt_2pl", "D": D, "Dc": 1.0, "nodes": nodes,
                   "span": sc.SPAN, "y": y, "params": params, "theta": theta,
                   "lw": population_logw(theta, KSIGMA * np.eye(D)), "tilt": tilt, "rows": rows, "seg_start": seg_start}
    return _K[key]


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def segment_counts(ll, theta, lw, tilt, y, seg_start):
    """The conditioned E-step a segment: ll [n][G] and y [n][J] by batch position -> n1, n0 [S][J][G], mass [S][G], logjoint [n]."""
    e = pc.estep_tilt(ll, theta, lw, tilt)
    lt = e["f"] - np.asarray(lw, np.float64)[None, :]                     # ll + tilt . theta: count_cases.counts adds lw back
    S, J, G = len(seg_start) - 1, y.shape[1], ll.shape[1]
    out = {"n1": np.zeros((S, J, G)), "n0": np.zeros((S, J, G)), "mass": np.zeros((S, G)), "logjoint": e["logjoint"],
           "lognorm": e["lognorm"]}
    for s in range(S):
        lo, hi = int(seg_start[s]), int(seg_start[s + 1])
        if hi > lo:
            t = cc.counts(lt[lo:hi], lw, y[lo:hi])
            out["n1"][s], out["n0"][s], out["mass"][s] = t["n1"], t["n0"], t["mass"]
    return out


def prob_of(cs, theta):
    J = cs["J"]
    return cc._prob_from(sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cc._single_item_rows(J)), J)


_KO = {}


def koracle(key):
    if key not in _KO:
        cs = kcase(key)
        y = cs["y"][cs["rows"]]
        ll = sc.irt_grid_loglik(cs["model"], cs["theta"], cs["params"], cs["Dc"], y)
        out = segment_counts(ll, cs["theta"], cs["lw"], cs["tilt"].astype(np.float64), y, cs["seg_start"])
        out["prob"] = prob_of(cs, cs["theta"])
        _KO[key] = out
    return _KO[key]


def _pair(T):
    """T 2^10 as an fp16 head and an fp16 remainder, back in float32: what the operand image holds of a table."""
    s = (np.asarray(T, np.float64) * 1024.0).astype(np.float32)
    h = s.astype(np.float16)
    lo = (s - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float32) + lo.astype(np.float32)


def restated(prob, theta, lw, tilt, y, seg_start, scale=16384.0):
    """The method in numpy float32 (see the module's header): n1, n0 [S][J][G] and mass [S][G]."""
    f32 = np.float32
    with np.errstate(divide="ignore"):
        t1, t0 = _pair(np.log(prob)), _pair(np.log1p(-prob))                # [J][G]
    acc = (y == 1).astype(f32) @ t1 + (y == 0).astype(f32) @ t0             # float32 products and sums
    ll = (acc * f32(2.0 ** -10) + (y == 255).sum(1, keepdims=True).astype(f32) * LOGP_MISSING).astype(f32)
    th, tl = np.asarray(theta, f32), np.asarray(tilt, f32)
    dot = (tl[:, :1] * th[None, :, 0]).astype(f32)
    for d in range(1, th.shape[1]):
        dot = (tl[:, d:d + 1] * th[None, :, d] + dot).astype(f32)
    f = ((ll + np.asarray(lw, f32)[None, :]).astype(f32) + dot).astype(f32)
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp(f - m).sum(1, keepdims=True, dtype=f32))).astype(f32)
    p = np.exp((f - lk).astype(f32)).astype(f32) * f32(scale)
    h = p.astype(np.float16)
    lo = (p - h.astype(f32)).astype(np.float16)
    p2 = h.astype(f32) + lo.astype(f32)
    S, J, G = len(seg_start) - 1, y.shape[1], p.shape[1]
    n1, n0, mass = np.zeros((S, J, G), f32), np.zeros((S, J, G), f32), np.zeros((S, G), f32)
    for s in range(S):
        for i in range(int(seg_start[s]), int(seg_start[s + 1])):
            n1[s] += np.outer((y[i] == 1).astype(f32), p2[i])
            n0[s] += np.outer((y[i] == 0).astype(f32), p2[i])
            mass[s] += p2[i]
    inv = f32(1.0 / scale)
    return {"n1": n1 * inv, "n0": n0 * inv, "mass": mass * inv}


def table_errors(got, want):
    """The row metric on the three tables: {name: (error, worst row)}; one row = one item of one segment, mass one row a segment."""
    G = want["mass"].shape[-1]
    f8 = lambda v: np.asarray(v, np.float64)                                # noqa: E731
    return {"n1": _row_errors(f8(got["n1"]).reshape(-1, G), want["n1"].reshape(-1, G), floor=1.0),
            "n0": _row_errors(f8(got["n0"]).reshape(-1, G), want["n0"].reshape(-1, G), floor=1.0),
            "mass": _row_errors(f8(got["mass"]).reshape(-1, G), want["mass"].reshape(-1, G), floor=1.0)}


_KR = {}


def krestated_error(key):
    """The largest row error of the restatement on a kernel case."""
    if key not in _KR:
        cs, want = kcase(key), koracle(key)
        r = restated(want["prob"], cs["theta"], cs["lw"], cs["tilt"], cs["y"][cs["rows"]], cs["seg_start"])
        _KR[key] = max(e for e, _ in table_errors(r, want).values())
    return _KR[key]


def rule_of(restated_error):
    """The rule of a case from its restatement's error: C_RULE times it, the restatement taken as no better than RULE_FLOOR."""
    return C_RULE * max(float(restated_error), RULE_FLOOR)


def krule(key):
    return rule_of(krestated_error(key))


def restated_error(want, theta, lw, tilt, y, seg_start):
    """The largest row error of the restatement against an oracle `want` (n1, n0, mass, prob) of any case."""
    return max(e for e, _ in table_errors(restated(want["prob"], theta, lw, tilt, y, seg_start), want).values())


def ratio_errors(got_obs, want_obs, want_n, want_rowmax):
    """observed = n1 / n where both tables meet a row rule r moves by at most 2 r max(rowmax, 1) / n: the largest
    |got - want| n / (2 max(rowmax, 1)) over the cells with n > 0, to be held to r.  want_rowmax: max(|n1|_inf, |n0|_inf) a row."""
    pos = want_n > 0
    d = np.abs(np.where(pos, got_obs - np.where(pos, want_obs, 0.0), 0.0)) * want_n / (2.0 * np.maximum(want_rowmax, 1.0)[..., None])
    return float(np.nanmax(d))


def group_stats(n1, n0, prob, min_obs):
    """count_cases.fit_stats a group: n_obs (rounded, int64), md, rmsd [H][J] (NaN below min_obs) and observed [H][J][G]."""
    st = [cc.fit_stats(n1[h], n0[h], prob) for h in range(len(n1))]
    out = {k: np.stack([s[k] for s in st]) for k in ("n_obs", "md", "rmsd", "observed")}
    out["n_obs"] = np.rint(out["n_obs"]).astype(np.int64)
    few = out["n_obs"] < min_obs
    out["md"], out["rmsd"] = np.where(few, np.nan, out["md"]), np.where(few, np.nan, out["rmsd"])
    return out


# ---- the planted case -----------------------------------------------------------------------------------------------------
PLANT_N, PLANT_J, PLANT_ITEM, PLANT_GROUP, PLANT_SHIFT, PLANT_SEED = 4096, 8, 3, 1, 0.8, 20260
PLANT_LABELS = np.array([3, 11])      # the labels dif() is handed: group 0 carries 3, group 1 carries 11
PLANT_NODES = 61
# The threshold of the statistical claim, between the oracle's two clean maxima on the committed seed: with the fitted private
# population (impact=True: group means -0.780 / +0.794, Sigma 0.634 after 21 EM iterations) the largest RMSD of a clean (group,
# item) cell is 0.0313 and the planted cell reads 0.1125; under N(0, I) for everybody (impact=False) the largest clean cell reads
# 0.0863 and the planted one 0.1846 (tests/test_dif_host.py prints and checks them)
PLANT_T = 0.05
# group_mean and sigma of dif(impact=True) against the oracle's fit, absolutely.  The oracle stops after 21 iterations with the
# log-likelihood moving by 0.99e-7 of itself -- at the tolerance, so a float32 sum may stop a few iterations either side; from the
# oracle's stop to its fixed point (40 iterations) gamma moves by 0.9e-3 and sigma by 2.1e-3, two iterations earlier by 0.4e-3 / 1.0e-3
POP_TOL = 5e-3
# dif(min_obs=PLANT_MIN_OBS) on the planted case: cells on either side of it (about 0.8 * 2 048 persons of a group answer an item)
PLANT_MIN_OBS = 1640

_P = {}


def planted():
    """The planted case: an engine case with `groups` int64 [N] (PLANT_LABELS by person, interleaved) and the pooled params."""
    if not _P:
        rng = np.random.RandomState(PLANT_SEED)
        N, J = PLANT_N, PLANT_J
        a = np.linspace(0.8, 1.6, J)[None, :]
        b = np.linspace(-1.2, 1.2, J)[None, ::-1].copy()
        g = (rng.uniform(size=N) < 0.5).astype(np.int64)                        # (about half the persons each, interleaved)
        x =np.where(g == 1, 0.75, -0.75)[:, None] + 0.8 * rng.normal(size=(N, 1))
        bb = np.repeat(b, N, axis=0)
        bb[g == PLANT_GROUP, PLANT_ITEM] += PLANT_SHIFT
        y = (rng.uniform(size=(N, J)) < vo.sigmoid(x @ a + bb)).astype(np.uint8)
        y[rng.uniform(size=(N, J)) < 0.20] = 255
        _P["c"] = {"name": "dif_planted", "N": N, "J": J, "model": "irt_2pl", "D": 1, "Dc": 1.0, "nodes": PLANT_NODES, "span": sc.SPAN,
                   "y": y, "params": {"a": a.astype(np.float32), "b": b.astype(np.float32)}, "group": g,
                   "groups": PLANT_LABELS[g]}
    return _P["c"]


_PO = {}


def planted_oracle(impact, min_obs=8, newton=None, prior=None):
    """dif()'s outputs on the planted case in float64: labels, order, seg_start, n1, n0, mass, prob, rmsd, md, n_obs, observed,
    group_mean, sigma; with `newton` also b_group, a_group, delta_b (newton_mstep a group from the pooled values).
    prior: (group_mean [H][1], sigma [1][1]) to score under instead of the oracle's own fit -- both EM loops stop when the
    log-likelihood moves by less than 1e-7 of itself, not when the parameters stand, so the GPU's tables are compared under the
    population the GPU reports, and that population to the oracle's by POP_TOL."""
    key = (bool(impact), min_obs, newton, None if prior is None else (prior[0].tobytes(), prior[1].tobytes()))
    if key not in _PO:
        from vipsy_amd.grid import score_grid
        cs = planted()
        theta, logw0 = score_grid(1, cs["nodes"], cs["span"])
        labels, inv = np.unique(cs["groups"], return_inverse=True)
        order = np.argsort(inv, kind="stable")
        counts = np.bincount(inv)
        seg_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        y = cs["y"][order]
        if "ll" not in _P:
            _P["ll"] = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], y)
            _P["prob"] = prob_of(cs, theta)
        ll, H = _P["ll"], len(labels)
        gidx = np.repeat(np.arange(H), counts)
        if prior is not None:
            gm, sigma = np.asarray(prior[0], np.float64), np.asarray(prior[1], np.float64)
            lw, tilt, _ = pc.population_prior(theta, np.eye(H)[gidx], gm, sigma)
        elif impact:
            if "em" not in _P:
                X = np.zeros((len(y), H))
                X[np.arange(len(y)), gidx] = 1.0
                X[:, 0] = 1.0
                _P["em"] = pc.em(ll, theta, X, 200, tol=1e-7)
            gamma, sigma = _P["em"]["gamma"], _P["em"]["sigma"]
            gm = gamma.copy()
            gm[1:] += gamma[0]
            lw, tilt, _ = pc.population_prior(theta, np.eye(H)[gidx], gm, sigma)
        else:
            gm, sigma, lw, tilt = np.zeros((H, 1)), np.eye(1), logw0.astype(np.float64), np.zeros((len(y), 1))
        out = segment_counts(ll, theta, lw, tilt, y, seg_start)
        out.update(labels=labels, order=order, seg_start=seg_start, prob=_P["prob"], group_mean=gm, sigma=sigma, theta=theta,
                   lw=lw, tilt=tilt, y=y)
        out.update(group_stats(out["n1"], out["n0"], out["prob"], min_obs))
        if newton is not None:
            a0, b0 = cs["params"]["a"].astype(np.float64), cs["params"]["b"].astype(np.float64)
            ab = [ec.newton_mstep(cs["model"], theta, cs["Dc"], out["n1"][h], out["n0"][h], a0, b0, np.ones((1, cs["J"]), bool), newton)
                  for h in range(H)]
            out["a_group"], out["b_group"] = np.stack([t[0] for t in ab]), np.stack([t[1][0] for t in ab])
            out["delta_b"] = out["b_group"] - b0
        _PO[key] = out
    return _PO[key]


def clean_cells():
    """bool [2][J]: every (group, item) cell but the planted one."""
    m = np.ones((2, PLANT_J), bool)
    m[PLANT_GROUP, PLANT_ITEM] = False
    return m


def claim(rmsd_impact, rmsd_flat, t=None):
    """The three inequalities of the statistical claim on two [2][J] RMSD tables: (every clean cell below t with the groups' own
    priors, the planted cell above t, at least one clean cell above t under N(0, I))."""
    t = PLANT_T if t is None else t
    c = clean_cells()
    return (bool((rmsd_impact[c] < t).all()), bool(rmsd_impact[PLANT_GROUP, PLANT_ITEM] > t), bool((rmsd_flat[c] > t).any()))


def top_cells(rmsd, top, gap):
    """The oracle's `top` cells by descending rmsd as (group, item) pairs, cut before the first neighbours closer than `gap`."""
    flat = rmsd.reshape(-1)
    fin = np.flatnonzero(np.isfinite(flat))
    sel = fin[np.argsort(-flat[fin], kind="stable")]
    keep = []
    for k, c in enumerate(sel[:top]):
        if k + 1 < len(sel) and flat[c] - flat[sel[k + 1]] <= gap:
            break
        keep.append((int(c // rmsd.shape[1]), int(c % rmsd.shape[1])))
    return keep


# ---- VCCDM ----------------------------------------------------------------------------------------------------------------
def cdm_groups(N):
    return (np.arange(N) % 3).astype(np.int64) * 5 - 2                         # labels -2, 3, 8


_CO = {}


def cdm_oracle(case, min_obs=8):
    if case[0] not in _CO:
        cs = sc.cdm_case(case)
        groups = cdm_groups(cs["N"])
        labels, inv = np.unique(groups, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        seg_start = np.concatenate([[0], np.cumsum(np.bincount(inv))]).astype(np.int64)
        y = cs["y"][order]
        ll, logw, attrs = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], y)
        out = segment_counts(ll, np.zeros((ll.shape[1], 1)), logw, np.zeros((len(y), 1)), y, seg_start)
        J = cs["J"]
        out["prob"] = cc._prob_from(sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], cc._single_item_rows(J))[0], J)
        out.update(group_stats(out["n1"], out["n0"], out["prob"], min_obs))
        out.update(labels=labels, groups=groups, seg_start=seg_start)
        _CO[case[0]] = (cs, out)
    return _CO[case[0]]
