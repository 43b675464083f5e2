"""The cases, the restated operand phase and the rules of the grid family's corner tests (tests/test_grid_corners_host.py on the
CPU, tests/test_gpu_grid_corners.py on the GPU): score(), expected_counts() / item_fit(), plausible_values() and
item_information() at the shape limits the family accepts (J <= 1024 items, G <= 1024 nodes, D <= 10, P = J K <= 4096) and on
persons who answered up to 1 024 items.  Tuples as in tests/score_cases.py; parameters are drawn, never trained.

The oracle is float64 throughout.  ll comes from per-item tables T1[j][g] = log P(y_j = 1 | g), T0[j][g] = log P(y_j = 0 | g) --
vo.irt_loglik on single-item response rows (one column, every node a row), vo.bernoulli_logprob_probs for the CDMs -- and two
indicator matmuls: sc.irt_grid_loglik calls vo.irt_loglik once a node over the whole response matrix, 9 s at J 1024 x G 1024.
tests/test_grid_corners_host.py holds the shortcut to sc.irt_grid_loglik / sc.cdm_grid_loglik.

restated_f says the operand phase of the kernels (GP_PASS of vipsy_amd/csrc/k_grid_post.hip) again in numpy; what it gives
against the oracle is the error of the METHOD at a case, whatever the code does.  The rules are built on it:

    row rule    tol = max(ROW_TOL, 3 e_restated) for an output of a case, e_restated the restatement's own row error against
                the oracle (the method-only bound of the project is a third of the rule); tol never exceeds the cap 4 x 2^-23 x
                max_i |loglik_i| (four float32 spacings at the size of the accumulated log-likelihood): where 3 e_restated
                would pass it -- the count tables of the long one-dimensional cases, whose relative error is the absolute error
                of f -- the cap is the tolerance.  tol is ROW_TOL itself for every case whose persons answered at most 130
                items.  Both asserted on the CPU.
    node rule   the gap below which a person's node (a draw) is left out is max(ARGMAX_GAP, 4 d_f), d_f the largest
                |f_restated - f_oracle| over the nodes within 20 of a person's maximum; at most ARGMAX_LEFT_OUT may be left out
                in the oracle alone.

Every oracle is computed once and shared; callers must not modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import pv_cases as pv
from tests import score_cases as sc
from tests import se_cases as se

ROW_TOL = 3e-5                   # the project's row rule (tests/test_gpu_response_designs.py)
DRAWS, SEED = 16, 7
NEAR = 20.0                      # d_f looks at the nodes within this of a person's maximum: exp(-20) = 2e-9 of its weight
SHORT = 130                      # answered items up to which the row rule must come out as ROW_TOL itself

# name, N, J, model, D, Dc, nodes per dimension, missing rate, slope range, seed
IRT_CASES = [
    ("corner_j1", 100, 1, "irt_2pl", 1, 1.0, 61, 0.0, (0.5, 1.5), 201),                  # one item, P = 2
    ("corner_j16_g33", 100, 16, "irt_2pl", 1, 1.0, 33, 0.1, (0.5, 1.5), 202),            # one full item chunk; one node in the second tile
    ("corner_j17_g32_1pl", 100, 17, "irt_1pl", 1, 1.702, 32, 0.1, None, 203),            # chunk + 1 item; exactly one node tile
    # two nodes.  irt_condition is waived: it is about what the quadrature means, not about what the kernel computes
    ("corner_g2", 100, 20, "irt_2pl", 1, 1.0, 2, 0.1, (0.5, 1.5), 210),
    # NT 16, the largest one-phase k_grid_pscores.  irt_condition is waived (8 nodes a dimension): it is about what the
    # quadrature means, not about what the kernel computes
    ("corner_g512_d3", 100, 40, "irt_2pl", 3, 1.0, 8, 0.0, (0.2, 0.5), 208),
    ("corner_g529_d2", 100, 40, "irt_2pl", 2, 1.0, 23, 0.0, (0.4, 1.0), 207),            # NT 17: the first two-phase launch
    ("corner_g1000_d3", 100, 30, "irt_2pl", 3, 1.0, 10, 0.0, (0.2, 0.5), 211),           # NT 32, ragged last tile
    # 1 024 answered items.  (Seed 214, not 204: under 204 four of the 100 persons have their best two nodes within the widened
    # gap of 1.6e-3 -- 4 % left out, above the cap of 2 %; under 214 it is one.)
    ("long_j1024_d1", 100, 1024, "irt_2pl", 1, 1.0, 61, 0.0, (0.1, 0.3), 214),
    ("long_j1024_g1024_d2", 64, 1024, "irt_2pl", 2, 1.0, 32, 0.1, (0.1, 0.3), 205),      # both limits at once, P = 3 072
    # P = 4 096.  irt_condition is waived (8 nodes a dimension): it is about what the quadrature means, not about what the
    # kernel computes
    ("long_j1024_g512_d3", 64, 1024, "irt_2pl", 3, 1.0, 8, 0.0, (0.1, 0.3), 206),
    ("long_j1024_4pl", 100, 1024, "irt_4pl", 1, 1.702, 61, 0.1, (0.1, 0.3), 209),        # score, counts and draws only
]
CONDITION_WAIVED = ("corner_g2", "corner_g512_d3", "long_j1024_g512_d3")
# name, N, J, cdm, K, missing rate, seed.  DINO with K <= 3 is left out on purpose: the reference's single-attribute rule ties
# patterns exactly there, and the argmax rule would leave 51-70 % of the persons out.
CDM_CASES = ([("corner_dina_k%d" % K, 100, J, "dina", K, 0.1, 100 + K)
              for K, J in ((1, 17), (2, 12), (5, 30), (6, 33), (7, 40), (8, 48), (9, 60))]
             + [("corner_dino_k%d" % K, 100, J, "dino", K, 0.0, 100 + K) for K, J in ((5, 30), (8, 48), (9, 60))]
             + [("long_dina_k2_j1024", 100, 1024, "dina", 2, 0.0, 302), ("long_dina_k10_j1024", 100, 1024, "dina", 10, 0.0, 310),
                ("long_dino_k10_j1024", 100, 1024, "dino", 10, 0.0, 310)])
ALL_CASES = IRT_CASES + CDM_CASES
ALL_IDS = [c[0] for c in ALL_CASES]


def by_name(name):
    return ALL_CASES[ALL_IDS.index(name)]


def has_info(case):
    """item_information() exists for 1PL / 2PL and the CDMs."""
    return len(case) == 7 or case[3] in ("irt_1pl", "irt_2pl")


def case_of(case):
    return (sc.cdm_case(case), "cdm") if len(case) == 7 else (sc.irt_case(case), "irt")


# ---- the float64 oracle --------------------------------------------------------------------------------------------------
def missing_constant():
    """log p of a missing cell as the oracle has it (vo.bernoulli_logprob_probs: y := 0, P := 0 under the clamp)."""
    return float(vo.bernoulli_logprob_probs(np.zeros((1, 1)), np.full((1, 1), 255, np.uint8))[0][0, 0])


def grid_of(cs, kind):
    """(coord float64 [G][D], logw float32 [G]) as the engines hand them to the kernels."""
    if kind == "cdm":
        C = 1 << cs["K"]
        pr = np.full(C, 1.0 / C)
        logw = np.log(np.clip(pr / pr.sum(), vo.EPS32, 1 - vo.EPS32))          # (sc.cdm_grid_loglik)
        return vo.all_attrs(cs["K"]), logw.astype(np.float32)
    from vipsy_amd.engine import score_grid
    theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
    return theta.astype(np.float64), logw


def item_tables(cs, kind, coord):
    """(T1, T0) float64 [J][G]: the log-probability of a correct / a wrong answer to item j at node g."""
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    J, G = cs["J"], coord.shape[0]
    p = cs["params"]
    if kind == "cdm":
        eta, _ = (vo.dino_eta if cs["cdm"] == "dino" else vo.dina_eta)(cs["K"], f8(cs["q"]))          # [C][J]
        g_, s_ = vo.sigmoid(f8(p["g"])).reshape(1, J), vo.sigmoid(f8(p["s"])).reshape(1, J)
        one, zero = np.ones((1, J), np.uint8), np.zeros((1, J), np.uint8)
        lp = {(e, v): vo.bernoulli_logprob_probs(P.copy(), yv)[0][0] for e, P in ((0, g_), (1, 1 - s_)) for v, yv in ((1, one), (0, zero))}
        on = (eta > 0).T                                            # [J][C]
        return np.where(on, lp[1, 1][:, None], lp[0, 1][:, None]), np.where(on, lp[1, 0][:, None], lp[0, 0][:, None])
    model = cs["model"]
    x = np.concatenate([coord, coord])                              # every node twice: answered 1, answered 0
    yv = np.concatenate([np.ones((G, 1), np.uint8), np.zeros((G, 1), np.uint8)])
    T1, T0 = np.empty((J, G)), np.empty((J, G))
    for j in range(J):
        a = f8(p["a"])[:, j:j + 1] if "a" in p else None
        c = vo.sigmoid(f8(p["c"]).reshape(1, J)[:, j:j + 1]) if model in ("irt_3pl", "irt_4pl") else None
        d = vo.sigmoid(f8(p["d"]).reshape(1, J)[:, j:j + 1]) if model == "irt_4pl" else None
        ll = vo.irt_loglik(model, x, a, f8(p["b"]).reshape(1, J)[:, j:j + 1], c, d, cs["Dc"], yv)[0]
        T1[j], T0[j] = ll[:G], ll[G:]
    return T1, T0


def loglik_from_tables(T1, T0, y):
    """ll [n][G] = [y == 1] T1 + [y == 0] T0 + (#missing) the missing constant."""
    return ((y == 1).astype(np.float64) @ T1 + (y == 0).astype(np.float64) @ T0
            + (y == 255).sum(1, keepdims=True) * missing_constant())


# ---- the operand phase said again ----------------------------------------------------------------------------------------
def _split16(v):
    h = v.astype(np.float16)
    return h, (v - h.astype(np.float32)).astype(np.float16)


def restated_f(cs, kind, tables=None):
    """f = logw + ll [n][G] float32 of a case by the arithmetic of the operand phase (vipsy_amd/csrc/k_grid_post.hip), step by
    step (tables: (T1, T0, logw) where the caller has them already):

      - the tables are the oracle's, rounded to float32 (k_grid_table_*: `float t1, t0`);
      - `split2h_bits(t * GP_SCALE, h, l)` in gp_put: T 2^10 as an fp16 head and the fp16 of the remainder;
      - GP_PASS, `for (int kc = 0; kc < KC; ++kc)`: the items in chunks of 16, in their order;
      - its four `acc[mt][t] = mfma_f16(a1h | a1l | a0h | a0l, f1 | f0, acc[mt][t])`: the sum of a chunk's 16 products of one
        table part and a 0/1 indicator is taken as exact (float64 holds it) and rounded into the float32 accumulator, T1 head,
        T1 low, T0 head, T0 low in turn -- four roundings a chunk;
      - `miss[mt] = (float)tot * VX_LOGP_MISSING`: one float32 product;
      - `f[r] = fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g]` in the consumers (k_grid_post, k_grid_draw, k_grid_counts,
        k_grid_pscores alike): the scale comes off exactly inside the fma, which rounds once, and the log-weight is added in float32.

    A model for a bound, not a bit-for-bit twin: the tables of the kernels come from their own float32 response functions, and
    the order of the 16 products inside one MFMA is the hardware's."""
    f32 = np.float32
    y = cs["y"]
    if tables is None:
        coord, logw = grid_of(cs, kind)
        tables = item_tables(cs, kind, coord) + (logw,)
    T1, T0, logw = tables
    parts = []
    for T in (T1, T0):
        h, lo = _split16(T.astype(f32) * f32(1024.0))
        parts += [h.astype(np.float64), lo.astype(np.float64)]
    ind = ((y == 1).astype(np.float64), (y == 0).astype(np.float64))
    acc = np.zeros((y.shape[0], T1.shape[1]), f32)
    for j0 in range(0, y.shape[1], 16):
        for k, part in enumerate(parts):
            acc = (acc.astype(np.float64) + ind[k >> 1][:, j0:j0 + 16] @ part[j0:j0 + 16]).astype(f32)
    miss = ((y == 255).sum(1).astype(f32) * f32(missing_constant())).astype(f32)[:, None]
    f = (acc.astype(np.float64) * 2.0 ** -10 + miss.astype(np.float64)).astype(f32)             # the fma: one rounding
    return (f + np.asarray(logw, f32)[None, :]).astype(f32)


def restated_posterior(f, coord):
    """loglik, mean, sd and node from a float32 f as k_grid_post forms them: weights about the maximum, moments about the
    coordinates of the best node, float32 sums."""
    f32 = np.float32
    f = np.asarray(f, f32)
    c32 = np.asarray(coord, f32)
    idx = f.argmax(1)
    m = f.max(1)
    w = np.exp((f - m[:, None]).astype(f32)).astype(f32)
    s0 = w.sum(1, dtype=f32)
    dl = (c32[None, :, :] - c32[idx][:, None, :]).astype(f32)
    m1 = ((w[:, :, None] * dl).sum(1, dtype=f32) / s0[:, None]).astype(f32)
    m2 = ((w[:, :, None] * dl * dl).sum(1, dtype=f32) / s0[:, None]).astype(f32)
    return {"loglik": (m + np.log(s0)).astype(f32), "mean": (c32[idx] + m1).astype(f32),
            "sd": np.sqrt(np.maximum(m2 - m1 * m1, f32(0))).astype(f32), "node": idx}


def _p_pairs(f):
    """p 2^14 of a float32 f as fp16 head + fp16 remainder (float32 values), the normaliser from the same f."""
    f32 = np.float32
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp((f - m).astype(f32)).sum(1, keepdims=True, dtype=f32))).astype(f32)
    p = np.exp((f - lk).astype(f32)).astype(f32) * f32(16384.0)
    h, lo = _split16(p)
    return h.astype(f32), lo.astype(f32)


def restated_counts(f, y):
    """n1, n0, mass from a float32 f by the arithmetic of count_cases.restated_f32: p = exp(f - loglik) in float32, p 2^14 as fp16
    pairs, float32 sums over the persons."""
    f32 = np.float32
    h, lo = _p_pairs(np.asarray(f, f32))
    p2 = (h + lo).astype(f32)
    s = f32(1.0 / 16384.0)
    return {"n1": ((y == 1).astype(f32).T @ p2).astype(f32) * s, "n0": ((y == 0).astype(f32).T @ p2).astype(f32) * s,
            "mass": p2.sum(0, dtype=f32) * s}


def restated_info(f, W1, W0, bound, y, K, slab=se.SLAB):
    """info and gradient by the chain of se_cases.restated_f32 (p 2^14, W 2^s and S 2^s as fp16 pairs without the low x low
    products, float32 sums, slabs of 256 persons) with the restated f in place of its once-rounded ll."""
    f32 = np.float32
    ph, pl = _p_pairs(np.asarray(f, f32))
    sc_ = f32(2.0 ** se.scale_exp(bound))
    un = f32(1.0) / sc_
    parts = []
    for W in (W1, W0):
        wh, wl = se._split16(W.astype(f32) * sc_)
        parts.append(((ph @ wh + ph @ wl).astype(f32) + pl @ wh).astype(f32) * f32(1.0 / 16384.0))
    y1, y0 = np.repeat(y == 1, K, axis=1), np.repeat(y == 0, K, axis=1)
    S = (np.where(y1, parts[0], f32(0)) - np.where(y0, parts[1], f32(0))).astype(f32)
    S = np.concatenate([S, np.full((len(y), 1), sc_, f32)], axis=1)
    sh, sl = se._split16(S)
    acc = np.zeros((S.shape[1], S.shape[1]), f32)
    for i0 in range(0, len(y), slab):
        h, lo = sh[i0:i0 + slab], sl[i0:i0 + slab]
        acc = acc + ((h.T @ h + h.T @ lo).astype(f32) + lo.T @ h).astype(f32)
    acc = acc * (un * un)
    return {"info": acc[:-1, :-1], "gradient": acc[:-1, -1]}


# ---- a case with everything the tests hold it to -------------------------------------------------------------------------
def _row_errors(got, want, floor):
    from tests.test_gpu_response_designs import _row_errors as rule
    return rule(np.asarray(got, np.float64), np.asarray(want, np.float64), floor)[0]


def row_tol(e_restated, cap):
    """max(ROW_TOL, 3 e_restated), and never above the cap (tol_cap): where three times the restatement's error would pass it, the
    cap is the tolerance -- the widening cannot hide more than the cap allows."""
    return min(max(ROW_TOL, 3.0 * e_restated), max(ROW_TOL, cap))


def tol_cap(loglik):
    """Four spacings of float32 at the size of the accumulated log-likelihood."""
    return 4.0 * 2.0 ** -23 * float(np.abs(loglik).max())


_O = {}


def oracle_of(case, made=None):
    """Everything score, counts and draws of a case are held to, computed once (made: a ready-made (cs, kind) in place of
    case_of(case) -- tests/steep_cases.py overrides leaves and plants persons; the cache goes by the case's name either way):

      cs, kind, coord, logw, T1, T0, f (float64 [N][G]), f_r (restated, float32), post (sc.grid_posterior), counts
      (cc.counts + prob + cc.fit_stats), draws (node, gap), answered (the largest number of answered items),
      d_f, gap_thr, e (the restatement's row errors by output) and tol (the row rule by output)."""
    if case[0] in _O:
        assert made is None or _O[case[0]]["cs"] is made[0], (case[0], "cached under this name from another case")
        return _O[case[0]]
    cs, kind = case_of(case) if made is None else made
    y = cs["y"]
    coord, logw = grid_of(cs, kind)
    T1, T0 = item_tables(cs, kind, coord)
    ll = loglik_from_tables(T1, T0, y)
    f = ll + logw.astype(np.float64)[None, :]
    post = sc.grid_posterior(ll, logw, coord)
    cnt = cc.counts(ll, logw, y)
    cnt["prob"] = np.exp(T1)
    cnt.update(cc.fit_stats(cnt["n1"], cnt["n0"], cnt["prob"]))
    f_r = restated_f(cs, kind, (T1, T0, logw))
    near = f >= f.max(1, keepdims=True) - NEAR
    d_f = float(np.abs(f_r.astype(np.float64) - f)[near].max())
    r_post, r_cnt = restated_posterior(f_r, coord), restated_counts(f_r, y)
    r_fit = cc.fit_stats(r_cnt["n1"].astype(np.float64), r_cnt["n0"].astype(np.float64), cnt["prob"])
    e = {"loglik": _row_errors(r_post["loglik"], post["loglik"], 1.0), "mean": _row_errors(r_post["mean"], post["mean"], 1.0),
         "sd": _row_errors(r_post["sd"], post["sd"], 1.0),
         "n1": _row_errors(r_cnt["n1"], cnt["n1"], 1.0), "n0": _row_errors(r_cnt["n0"], cnt["n0"], 1.0),
         "mass": _row_errors(r_cnt["mass"][None, :], cnt["mass"][None, :], 1.0)}
    for k in ("md", "rmsd"):
        assert np.array_equal(np.isnan(r_fit[k]), np.isnan(cnt[k]))
        e[k] = float(np.nanmax(np.abs(r_fit[k] - cnt[k]))) if np.isfinite(cnt[k]).any() else 0.0
    out = {"cs": cs, "kind": kind, "coord": coord, "logw": logw, "T1": T1, "T0": T0, "f": f, "f_r": f_r, "post": post,
           "counts": cnt, "draws": pv.draw(f, pv.gumbel(SEED, np.arange(f.shape[0]), f.shape[1], DRAWS)),
           "answered": int((y != 255).sum(1).max()), "d_f": d_f, "gap_thr": max(sc.ARGMAX_GAP, 4.0 * d_f),
           "e": e, "cap": tol_cap(post["loglik"])}
    out["tol"] = {k: row_tol(v, out["cap"]) for k, v in e.items()}
    _O[case[0]] = out
    return out


def left_out(o):
    """Shares of the persons and of the (person, draw) pairs that the node rule leaves out at the case's gap threshold."""
    return float((o["post"]["gap"] <= o["gap_thr"]).mean()), float((o["draws"][1] <= o["gap_thr"]).mean())


def info_oracle(case, made=None):
    """What item_information() of a case (made: as oracle_of takes it) is held to, in the keys of se_cases.oracle that test_gpu_se._hold_info reads (S, info and
    gradient in float64), with the restatement's row errors `e` and the row rule `tol` for info and gradient.  Not kept: the
    matrix of 4 096 parameters is 134 MB."""
    o = oracle_of(case, made)
    cs, kind, y = o["cs"], o["kind"], o["cs"]["y"]
    K, free = se.layout(cs, kind)
    W1, W0, bound = se.tables(cs, kind, cs["params"])
    S = se.scores(o["counts"]["p"], W1, W0, y, K)
    info = S.T @ S
    out = {"info": info, "gradient": S.sum(0), "n": len(y), "K": K, "free": free}
    r = restated_info(o["f_r"], W1, W0, bound, y, K)
    top = float(np.abs(np.diag(info)).max())
    out["e"] = {"info": _row_errors(r["info"], info, top),
                "gradient": _row_errors(r["gradient"][None, :], out["gradient"][None, :], np.sqrt(top * len(y)))}
    out["tol"] = {k: row_tol(v, o["cap"]) for k, v in out["e"].items()}
    return out
