"""The grid family on structured response designs: the cases, the glue to the float64 oracles the calls already have, and the
conditions under which those oracles are a fair yardstick (tests/test_grid_designs_host.py on the CPU,
tests/test_gpu_grid_designs.py on the GPU).  Plain numpy, seeded: every case is the same on every machine.

Every other test of the grid family draws its holes as independent coin flips at one rate (tests/score_cases.py), so every
person answers about the same number of items and every item has about the same number of respondents.  The designs here are
those of tests/response_designs.py as it stands -- booklets of very different length, a block of 64 consecutive persons without a
response, items nobody saw, constant items and persons, a matrix without an observed cell and one with a single cell.  The
responses are the design's own (a 2PL with its own parameters); the item parameters of a case are DRAWN as
score_cases.irt_case / cdm_case draw them, never trained.  A case is a dict shaped like irt_case's / cdm_case's with `facts`, the
design's promises, beside it: the oracles of score_cases, count_cases, se_cases, ld_cases, fit_cases, point_cases, dif_cases,
sx2_cases, pop_cases and em_cases take it as it is (some through y= / params=).

What each case reaches:
  gd_sorted_j70          rows 128 .. 191 are one whole unit of empty persons (64 = GP_MT x 32) between two units of booklet 1; the 10
                         items behind the last booklet and the edge's extra item are unanswered; items of different booklets
                         share no respondent.  Also the sx2, the groups-are-booklets and the rows= case.
  gd_shuffled_j130_3pl   257 persons = four units and one person; every unit mixes 10-, 30- and 80-item persons.
  gd_short_j40_d2        3-item persons; the multidimensional kernels.
  gd_complete_j30        no hole at all, one all-one and one all-zero item.
  gd_all_missing, gd_single_cell
  gd_dina_k3, gd_dina_k6 the booklets fall on the items behind the K single-attribute ones, as cdm_case punches its holes (a person
                         who lacks the one item that identifies an attribute has two patterns exactly tied); rows 128 .. 191 are
                         empty and the last item is unanswered.  K = 6: two node tiles.  DINO is left out on purpose: under
                         booklets its patterns tie exactly in the float64 oracle alone, and no cap on the node rule could hold.

No new tolerance: every call keeps the rule and the constant of its own *_cases.py.  Two caps are conditions on the oracle, asserted
on the CPU: the node / draw rule may leave out at most score_cases.ARGMAX_LEFT_OUT of the persons with at least one answer
(an empty person's posterior is the prior, whose best two nodes are never tied); lz is compared on fit_cases.lz_condition's
persons, which may leave out at most fit_cases.LEFT_OUT_CAP of the persons with at least COND_MIN_ITEMS answers -- persons with
fewer are held by the sum rule on all seven sums.

Everything here is computed once and shared; callers must not modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import dif_cases as dc
from tests import fit_cases as fc
from tests import ld_cases as ld
from tests import pop_cases as pc
from tests import pv_cases as pv
from tests import response_designs as rd
from tests import score_cases as sc
from tests import se_cases as se

DRAWS, SEED = pv.DRAWS, pv.SEED
EDGE_SEED = 7

# name: (design, model, D, Dc, nodes a dimension, slope range, seed of the item parameters).  (gd_sorted_j70: seed 351, not 301 --
# under 301 a running expected count of S-X2's collapse sweep on the 40-item booklet sits within 3e-4 relative of min_expected,
# inside sx2_cases.COLLAPSE_MARGIN, where float32 tables may decide the cell otherwise; under 351 the closest is 1.8e-3.)
IRT = {
    "gd_sorted_j70": (lambda: rd.with_edges(*rd.booklets(333, 70, (5, 15, 40), True, seed=17), seed=EDGE_SEED, empty_block=128),
                      "irt_2pl", 1, 1.0, 61, (0.5, 1.5), 351),
    "gd_shuffled_j130_3pl": (lambda: rd.with_edges(*rd.booklets(257, 130, (10, 30, 80), False, seed=9), seed=EDGE_SEED),
                             "irt_3pl", 1, 1.0, 61, (0.4, 1.0), 302),
    "gd_short_j40_d2": (lambda: rd.with_edges(*rd.booklets(192, 40, (3, 8, 17), False, seed=4), seed=EDGE_SEED, empty_block=64),
                        "irt_2pl", 2, 1.0, 21, (0.4, 1.0), 303),
    "gd_complete_j30": (lambda: rd.with_edges(*rd.booklets(400, 30, (30,), False, seed=20), seed=EDGE_SEED, empty_person=False,
                                              unanswered_item=False, constant_persons=False),
                        "irt_2pl", 1, 1.0, 61, (0.5, 1.5), 304),
    "gd_all_missing": (lambda: rd.all_missing(200, 37), "irt_2pl", 1, 1.0, 61, (0.5, 1.5), 305),
    "gd_single_cell": (lambda: rd.single_cell(200, 37), "irt_2pl", 1, 1.0, 61, (0.5, 1.5), 306),
}
# name: (N, J, K, booklet lengths over the items behind the K single-attribute ones, first row of the empty block, seed)
CDM = {
    "gd_dina_k3": (300, 30, 3, (4, 9, 14), 128, 311),
    "gd_dina_k6": (300, 40, 6, (4, 9, 14), 128, 312),
}
DEGENERATE = ("gd_all_missing", "gd_single_cell")
MAIN = [n for n in IRT if n not in DEGENERATE] + list(CDM)           # the cases every call is compared on
ALL = list(IRT) + list(CDM)
SORTED = "gd_sorted_j70"
POP = {SORTED: 321, "gd_short_j40_d2": 322}                          # the conditioned-prior cases: seed of covariates and (Gamma, Sigma)

_CASES = {}


def kind_of(name):
    return "cdm" if name in CDM else "irt"


def _irt_params(model, D, J, slopes, rng):
    """The float32 leaves as score_cases.irt_case draws them (2PL / 3PL)."""
    a = rng.uniform(slopes[0], slopes[1], size=(D, J))
    if D > 1:
        a = a * vo.default_a_free(D, J)
    p = {"a": a.astype(np.float32), "b": rng.normal(0.0, 1.0, size=(1, J)).astype(np.float32)}
    if model == "irt_3pl":
        p["c"] = sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)
    return p


def _cdm_case(name):
    """score_cases.cdm_case's draw (Q-matrix, g, s, patterns, responses from the model) under a booklet design."""
    N, J, K, lens, block, seed = CDM[name]
    rng = np.random.RandomState(seed)
    q = sc.cdm_q(K, J, rng)
    p = {"g": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32),
         "s": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)}
    eta_all, _ = vo.dina_eta(K, q.astype(np.float64))
    eta = eta_all[rng.randint(0, 2 ** K, size=N)]
    g, s = vo.sigmoid(p["g"].astype(np.float64)), vo.sigmoid(p["s"].astype(np.float64))
    y = (rng.uniform(size=(N, J)) < np.where(eta > 0, 1 - s, g)).astype(np.uint8)
    holes, facts = rd.booklets(N, J - K, lens, False, seed=seed)
    y[:, K:][holes == rd.MISSING] = rd.MISSING
    y[block:block + 64] = rd.MISSING
    y[:, J - 1] = rd.MISSING                                             # a multi-attribute item nobody answered
    d = rd.describe(y)
    facts = dict(facts, design="cdm_booklets", empty_block=block, unanswered_item=J - 1,
                 **{k: d[k] for k in ("missing", "n_missing", "min_obs", "max_obs", "empty_persons", "unanswered_items")})
    facts["lens"] = [K + v for v in lens]                               # what a person of each booklet answers
    return {"name": name, "N": N, "J": J, "cdm": "dina", "K": K, "q": q, "y": y, "params": p, "facts": facts}


def case(name):
    """The case dict (with `facts`), built once."""
    if name not in _CASES:
        if name in CDM:
            _CASES[name] = _cdm_case(name)
        else:
            design, model, D, Dc, nodes, slopes, seed = IRT[name]
            y, facts = design()
            N, J = y.shape
            _CASES[name] = {"name": name, "N": N, "J": J, "model": model, "D": D, "Dc": Dc, "nodes": nodes, "span": sc.SPAN,
                            "y": y, "params": _irt_params(model, D, J, slopes, np.random.RandomState(seed)), "facts": facts}
        ld._CASES.setdefault(name, _CASES[name])                       # ld_cases / fit_cases look their cases up by name
    return _CASES[name]


def key(name):
    """What ld_cases.oracle / restated_f32 and fit_cases.oracle / restated_f32 take for a case: (kind, a tuple led by the name)."""
    case(name)
    return kind_of(name), (name,)


def grid_kw(name):
    cs = case(name)
    return {} if name in CDM else {"nodes": cs["nodes"], "span": cs["span"]}


def has_info(name):
    """item_information() / fit_em() exist for 1PL / 2PL and the CDMs."""
    return name in CDM or IRT[name][1] in ("irt_1pl", "irt_2pl")


# ---- what the designs promise -----------------------------------------------------------------------------------------------
def check_facts(name):
    """Every promise of `facts` on the matrix itself (AssertionError otherwise); returns rd.describe(y)."""
    cs = case(name)
    y, f = cs["y"], cs["facts"]
    d = rd.describe(y)
    assert y.dtype == np.uint8 and set(np.unique(y)) <= {0, 1, rd.MISSING}
    for k in ("n_missing", "min_obs", "max_obs"):
        assert d[k] == f[k], (name, k, d[k], f[k])
    assert abs(d["missing"] - f["missing"]) < 1e-12
    assert np.array_equal(d["empty_persons"], f["empty_persons"]) and np.array_equal(d["unanswered_items"], f["unanswered_items"])
    if "empty_block" in f:
        b = f["empty_block"]
        assert b % 64 == 0 and (y[b:b + 64] == rd.MISSING).all() and set(range(b, b + 64)) <= set(d["empty_persons"].tolist())
        assert (y[b - 1] != rd.MISSING).any() and (y[b + 64] != rd.MISSING).any()         # answering persons on both sides
    if "empty_person" in f:
        assert (y[f["empty_person"]] == rd.MISSING).all()
    if "unanswered_item" in f:
        assert (y[:, f["unanswered_item"]] == rd.MISSING).all()
    if "all_one_item" in f:
        for j, v in ((f["all_one_item"], 1), (f["all_zero_item"], 0)):
            col = y[:, j][y[:, j] != rd.MISSING]
            assert len(col) >= 2 and (col == v).all(), (name, j)
    if "all_one_person" in f:
        for i, v in ((f["all_one_person"], 1), (f["all_zero_person"], 0)):
            row = y[i][y[i] != rd.MISSING]
            assert len(row) >= 1 and (row == v).all(), (name, i)
    if f.get("design") == "booklets":
        # a person's observed cells lie inside the booklet's contiguous item range: whole 16-item chunks are empty
        for k, (s, v) in enumerate(zip(f["starts"], f["lens"])):
            mine = y[f["booklet_of"] == k]
            assert (np.delete(mine, np.arange(s, s + v), axis=1) == rd.MISSING).all(), (name, k)
    return d


def booklet_items(name, k):
    f = case(name)["facts"]
    return np.arange(f["starts"][k], f["starts"][k] + f["lens"][k])


def cross_pairs(name):
    """bool [J][J]: pairs of items from different booklets of a sorted design without overlap -- no person answered both."""
    cs = case(name)
    f = cs["facts"]
    book = np.full(cs["J"], -1)
    for k in range(len(f["lens"])):
        book[booklet_items(name, k)] = k
    m = (book[:, None] != book[None, :]) & (book[:, None] >= 0) & (book[None, :] >= 0)
    obs = (cs["y"] != rd.MISSING).astype(np.int64)
    assert ((obs.T @ obs)[m] == 0).all()
    return m


# ---- the oracles -------------------------------------------------------------------------------------------------------------
_GRID, _O = {}, {}


def grid_ll(name, y=None):
    """(coord float64 [G][D], logw [G] as the engine hands it to the kernels, ll float64 [n][G]) -- of the case's rows, kept; or of y."""
    if y is None and name in _GRID:
        return _GRID[name]
    cs = case(name)
    yy = cs["y"] if y is None else y
    if name in CDM:
        ll, logw, coord = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], yy)
        out = (np.asarray(coord, np.float64), np.asarray(logw, np.float64), ll)
    else:
        from vipsy_amd.engine import score_grid
        theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
        out = (theta.astype(np.float64), logw, sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], yy))
    if y is None:
        _GRID[name] = out
    return out


def missing_constant():
    """log p of a missing cell as the oracle has it."""
    return float(vo.bernoulli_logprob_probs(np.zeros((1, 1)), np.full((1, 1), 255, np.uint8))[0][0, 0])


def oracle(name):
    """`post` (score_cases.irt_oracle / cdm_oracle), `counts` (count_cases.irt_oracle / cdm_oracle), `f` = logw + ll, `draws`
    (pv_cases.draw over pv_cases.gumbel: node, gap), `answered` bool [N], `est` (the EAP [N][D] / the MAP pattern [N]),
    `pairs` (ld_cases: tables, q3, v, keep at est) and `fit` (fit_cases.sums at est)."""
    if name not in _O:
        cs, kind = case(name), kind_of(name)
        y = cs["y"]
        coord, logw, ll = grid_ll(name)
        post = sc.irt_oracle(cs) if kind == "irt" else sc.cdm_oracle(cs)
        f = ll + np.asarray(logw, np.float64)[None, :]
        est = post["mean"] if kind == "irt" else post["node"]
        prob = fc.prob_at(kind, cs, est)
        pairs = ld.tables(y, prob)
        pairs["q3"], pairs["v"] = ld.q3_of_tables(pairs)
        pairs["keep"] = ld.condition(pairs)
        _O[name] = {"post": post, "counts": cc.irt_oracle(cs) if kind == "irt" else cc.cdm_oracle(cs), "f": f, "coord": coord,
                    "draws": pv.draw(f, pv.gumbel(SEED, np.arange(len(y)), f.shape[1], DRAWS)),
                    "answered": (y != rd.MISSING).any(1), "est": est, "pairs": pairs, "fit": fc.sums(y, prob)}
    return _O[name]


def left_out(name):
    """The shares the node rule and the draw rule leave out, over the persons with at least one answer (and their draws)."""
    o = oracle(name)
    a = o["answered"]
    if not a.any():
        return 0.0, 0.0
    return float((o["post"]["gap"][a] <= sc.ARGMAX_GAP).mean()), float((o["draws"][1][a] <= sc.ARGMAX_GAP).mean())


def lz_left_out(name, sums=None):
    """The share of the persons with at least COND_MIN_ITEMS answers that fit_cases.lz_condition leaves out."""
    o = oracle(name)["fit"] if sums is None else sums
    many = o["person"]["n"] >= fc.COND_MIN_ITEMS
    return float((~o["keep"][many]).mean()) if many.any() else 0.0


_INFO = {}


def info_oracle(name):
    """se_cases.oracle at the drawn parameters (info, gradient, kept, free and -- where the kept block is positive definite -- se,
    cov, condition)."""
    if name not in _INFO:
        cs = case(name)
        _INFO[name] = se.oracle(cs, kind_of(name), cs["params"])
    return _INFO[name]


_GROUPS = {}


def group_oracle(name=SORTED, min_obs=8):
    """groups = booklets under N(0, I) for everybody (dif(impact=False)): dif_cases.segment_counts and group_stats, with `rule`
    (dif_cases.rule_of the restatement's error on this case) and what the restatement needs again (theta, lw, tilt, y, seg_start)."""
    if name not in _GROUPS:
        cs = case(name)
        coord, logw, ll = grid_ll(name)
        groups = np.asarray(cs["facts"]["booklet_of"], np.int64)
        labels, inv = np.unique(groups, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        seg = np.concatenate([[0], np.cumsum(np.bincount(inv))]).astype(np.int64)
        y = cs["y"][order]
        lw, tilt = np.asarray(logw, np.float64), np.zeros((len(y), cs["D"]))
        out = dc.segment_counts(ll[order], coord, lw, tilt, y, seg)
        out["prob"] = dc.prob_of(cs, coord.astype(np.float32))
        out.update(dc.group_stats(out["n1"], out["n0"], out["prob"], min_obs))
        out.update(labels=labels, groups=groups, order=order, seg_start=seg, theta=coord, lw=lw, tilt=tilt, y=y)
        out["restated_error"] = dc.restated_error(out, coord, lw, tilt, y, seg)
        out["rule"] = dc.rule_of(out["restated_error"])
        _GROUPS[name] = out
    return _GROUPS[name]


_POP = {}


def population(name):
    """(cov [N][2] as pop_cases.covariates draws them, X, Gamma [3][D], Sigma [D][D] drawn as pop_cases.frozen draws them, the
    oracle pop_cases.estep under them, its draws (node, gap) with PV_DRAWS / PV_SEED)."""
    if name not in _POP:
        cs = case(name)
        rng = np.random.RandomState(POP[name])
        cov = pc.covariates(cs["N"], rng)
        X, D = pc.design(cov), cs["D"]
        gamma = rng.uniform(-0.6, 0.6, size=(X.shape[1], D))
        L = np.diag(rng.uniform(0.95, 1.1, size=D)) + np.tril(rng.uniform(-0.3, 0.3, size=(D, D)), -1)
        sigma = L @ L.T
        coord, _, ll = grid_ll(name)
        want = pc.estep(ll, coord.astype(np.float32), X, gamma, sigma)
        _POP[name] = {"cov": cov, "X": X, "gamma": gamma, "sigma": sigma, "want": want,
                      "draws": pc.oracle_draws(want["f"], np.arange(cs["N"]), pc.PV_DRAWS, pc.PV_SEED)}
    return _POP[name]
