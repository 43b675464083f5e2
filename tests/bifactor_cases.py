"""The cases, the two float64 oracles, the restated operand phase and the rules of the bifactor / testlet scores
(IrtEngine.score_bifactor on vipsy_amd/csrc/k_grid_bifactor.hip; tests/test_bifactor_host.py on the CPU, tests/test_gpu_bifactor.py
on the GPU).  Parameters are drawn and seeded, never trained; the item order is shuffled, so that no testlet is contiguous.

Oracles, float64 numpy over the public pieces of oracle/vi_oracle.py (through tests/corner_cases.item_tables, as the corner
cases take their tables):

    brute force   the full tensor grid Gg x Gh^S' with product weights over the general dimension and the S' specific
                  dimensions that HAVE items, then score_cases.grid_posterior: loglik, EAP and PSD of every dimension.  It does not
                  use the reduction identity.  The node of the general MARGINAL posterior and its gap come from the same table,
                  marginalised over the specific axes by a log-sum-exp.  (A specific dimension without items multiplies the grid
                  by Gh and changes nothing: its weights sum to 1.  `s2_2pl` carries it through the brute force all the same; the
                  larger cases leave it out and hold it to the moments of the grid prior.)
    reduced       the factorised formula of Gibbons & Hedeker, used where brute force is impossible (Gh^40).  The host test
                  asserts that the two agree to 1e-12 on every case small enough for both.

restated() says the operand phase of the kernels again in float32 numpy: per-testlet chunk order (grid.bifactor_plan), four
roundings a chunk, the fma that takes the scale off and adds log v_h, the float32 log-sum-exp over h, the float32 sum over the
testlets, the fold over g (corner_cases.restated_posterior), and for the specific moments the float32 sums E1, E2 of the
second kernel.  A model for a bound, not a bit-for-bit twin.  The rules are the project's (tests/corner_cases.py): the row rule
row_tol(e_restated, tol_cap(loglik)) an output, the node rule with the gap max(ARGMAX_GAP, 4 d_f).

Every case has one person with no answer (row 0), one all-correct person (row 1) and one specific dimension without items;
`s3_full_tile` has its general dimension at index 2, not 0.  Everything is computed once a case; callers must not modify it."""
import numpy as np

from oracle import vi_oracle as vo
from tests import corner_cases as cn
from tests import score_cases as sc

# name, N, testlet sizes, general-only items, model, Dc, (Gg, Gh), missing rate, seed, index of the general dimension
CASES = [
    ("s2_2pl", 100, (9, 11), 3, "irt_2pl", 1.0, (21, 11), 0.10, 11, 0),          # N no multiple of 64, pseudo-testlet, brute force
    ("s5_3pl", 64, (17, 16, 1, 12, 14), 0, "irt_3pl", 1.0, (15, 5), 0.10, 12, 0),  # two-chunk, one-chunk, one-item testlets; brute force
    ("s3_full_tile", 64, (5, 20, 8), 2, "irt_2pl", 1.0, (9, 32), 0.0, 13, 2),    # Gh = 32: no padded h row
    ("s40", 100, (3,) * 40, 0, "irt_2pl", 1.0, (61, 21), 0.20, 14, 0),           # many testlets, reduced oracle
    ("s100_j500", 64, (5,) * 100, 0, "irt_2pl", 1.0, (61, 21), 0.0, 15, 0),      # the headline's structure, reduced oracle
    ("s2_4pl_dc", 64, (7, 9), 0, "irt_4pl", 1.702, (21, 11), 0.10, 16, 0),       # both asymptotes
    ("gh1", 100, (9, 11), 3, "irt_2pl", 1.0, (41, 1), 0.10, 17, 0),              # Gh = 1
]
IDS = [c[0] for c in CASES]
SPAN = (6.0, 4.0)
BRUTE = ("s2_2pl", "s5_3pl", "s2_4pl_dc", "gh1")                                # small enough for the tensor grid (s3_full_tile: 9 x 32^3)
BRUTE_WITH_EMPTY = ("s2_2pl", "gh1")                                             # ... with the empty dimension carried along
# irt_condition (PSD >= half the node spacing) is waived for the coarse grids: it is about what the quadrature means, not about
# what the kernel computes
CONDITION_HELD = ("s2_2pl", "s40", "s100_j500")
EMPTY_AT = 1                                                                     # the column of specific_dims that has no item


def by_name(name):
    return CASES[IDS.index(name)]


def _logit(p):
    return np.log(p) - np.log1p(-p)


_CASES = {}


def case_of(case):
    """The drawn case: model, D, J, Dc, nodes, span, general, free / a [D][J], params (float32 leaves), y [N][J] u8, and the
    structure it was drawn from (testlet [J]: the column of specific_dims, -1: general only; specific_dims)."""
    name, N, sizes, n_gen, model, Dc, nodes, missing, seed, general = case
    if name in _CASES:
        return _CASES[name]
    rng = np.random.RandomState(seed)
    S = len(sizes) + 1                                              # one specific dimension without items, at column EMPTY_AT
    D, J = S + 1, int(sum(sizes)) + n_gen
    specific_dims = np.array([d for d in range(D) if d != general], np.int64)
    columns = [s for s in range(S) if s != EMPTY_AT]
    testlet = np.concatenate([np.full(k, columns[t], np.int64) for t, k in enumerate(sizes)] + [np.full(n_gen, -1, np.int64)])
    testlet = testlet[rng.permutation(J)]                           # no testlet is contiguous
    free = np.zeros((D, J), np.float32)
    free[general] = 1
    free[specific_dims[testlet[testlet >= 0]], np.flatnonzero(testlet >= 0)] = 1
    a = rng.uniform(0.4, 1.0, size=(D, J)) * free                   # the specific loadings; zero where not free
    a[general] = rng.uniform(0.6, 1.4, size=J)
    params = {"a": a.astype(np.float32), "b": rng.normal(size=J).astype(np.float32)}
    c = d = None
    if model in ("irt_3pl", "irt_4pl"):
        c = rng.uniform(0.05, 0.25, size=J)
        params["c"] = _logit(c).astype(np.float32)
    if model == "irt_4pl":
        d = 1.0 - rng.uniform(0.02, 0.15, size=J)
        params["d"] = _logit(d).astype(np.float32)
    x = rng.normal(size=(N, D))
    z = Dc * (x @ params["a"].astype(np.float64) + params["b"].astype(np.float64)[None, :])
    p = 1.0 / (1.0 + np.exp(-z))
    if c is not None:
        p = c[None, :] + ((d[None, :] if d is not None else 1.0) - c[None, :]) * p
    y = (rng.uniform(size=(N, J)) < p).astype(np.uint8)
    if missing > 0:
        y[rng.uniform(size=(N, J)) < missing] = 255
    y[0] = 255                                                      # nobody's answers
    y[1] = 1                                                        # all correct
    cs = {"name": name, "N": N, "J": J, "D": D, "model": model, "Dc": Dc, "nodes": nodes, "span": SPAN, "general": general,
          "free": free, "params": params, "y": y, "testlet": testlet, "specific_dims": specific_dims, "sizes": sizes}
    _CASES[name] = cs
    return cs


def grid_of(cs):
    from vipsy_amd.grid import bifactor_grid
    theta, logw, u, logv = bifactor_grid(cs["nodes"], cs["span"])
    return theta.astype(np.float64), logw, u.astype(np.float64), logv


def _sub(cs, items):
    """The case restricted to `items`, as corner_cases.item_tables reads one."""
    p = {k: (v[:, items] if k == "a" else v[items]) for k, v in cs["params"].items()}
    return {"J": len(items), "model": cs["model"], "Dc": cs["Dc"], "params": p}


# ---- brute force ---------------------------------------------------------------------------------------------------------
def brute_force(cs, with_empty=False):
    """The tensor grid over the general dimension and the specific dimensions with items (with_empty: and the one without).
    Returns loglik, eap_general, psd_general, eap_specific / psd_specific [N][S] (the prior's moments for a dimension that is not
    on the grid), node and gap of the general marginal, and F [N][Gg] = its log up to loglik."""
    theta, logw, u, logv = grid_of(cs)
    Gg, Gh, S = len(theta), len(u), len(cs["specific_dims"])
    on = [s for s in range(S) if with_empty or (cs["testlet"] == s).any()]
    axes = np.meshgrid(theta, *([u] * len(on)), indexing="ij")
    lws = np.meshgrid(logw.astype(np.float64), *([logv.astype(np.float64)] * len(on)), indexing="ij")
    G = axes[0].size
    coord = np.zeros((G, cs["D"]))
    coord[:, cs["general"]] = axes[0].reshape(-1)
    for k, s in enumerate(on):
        coord[:, cs["specific_dims"][s]] = axes[1 + k].reshape(-1)
    logw_full = sum(w.reshape(-1) for w in lws)
    T1, T0 = cn.item_tables(cs, "irt", coord)
    ll = cn.loglik_from_tables(T1, T0, cs["y"])
    post = sc.grid_posterior(ll, logw_full, coord)
    f = (ll + logw_full[None, :]).reshape(len(ll), Gg, -1)
    m = f.max(2)
    F = m + np.log(np.exp(f - m[:, :, None]).sum(2))
    out = _general(F, theta)
    out["loglik_joint"] = post["loglik"]
    v = np.exp(logv.astype(np.float64))
    v = v / v.sum()                                                 # (the float32 log-weights sum to 1 within 1e-7 only)
    pm = float((v * u).sum())
    out["eap_specific"] = np.full((len(ll), S), pm)
    out["psd_specific"] = np.full((len(ll), S), np.sqrt((v * u * u).sum() - pm * pm))
    for s in on:
        out["eap_specific"][:, s] = post["mean"][:, cs["specific_dims"][s]]
        out["psd_specific"][:, s] = post["sd"][:, cs["specific_dims"][s]]
    out["eap_general_joint"], out["psd_general_joint"] = post["mean"][:, cs["general"]], post["sd"][:, cs["general"]]
    return out


def _general(F, theta):
    """loglik, the moments of theta, node and gap from F [N][Gg] in float64."""
    p = sc.grid_posterior(F, np.zeros(F.shape[1]), theta[:, None])
    return {"loglik": p["loglik"], "eap_general": p["mean"][:, 0], "psd_general": p["sd"][:, 0], "node": p["node"], "gap": p["gap"],
            "F": F}


# ---- the reduction, in float64 -------------------------------------------------------------------------------------------
def testlet_logliks(cs):
    """For every testlet of grid.bifactor_plan (the pseudo-testlet last): (column of specific_dims or -1, items in slot order,
    T1, T0 float64 [items][Gg Gh], node g h at g Gh + h)."""
    from vipsy_amd.grid import bifactor_plan
    theta, _, u, _ = grid_of(cs)
    plan = bifactor_plan(cs["testlet"], cs["specific_dims"], len(theta))
    tg, uh = np.meshgrid(theta, u, indexing="ij")
    out = []
    for t, s in enumerate(plan["tl_column"]):
        slots = plan["col"][16 * plan["tl_start"][t]:16 * plan["tl_start"][t + 1]]
        items = slots[slots >= 0]
        coord = np.zeros((tg.size, cs["D"]))
        coord[:, cs["general"]] = tg.reshape(-1)
        if s >= 0:
            coord[:, cs["specific_dims"][s]] = uh.reshape(-1)
        T1, T0 = cn.item_tables(_sub(cs, items), "irt", coord)
        out.append((int(s), items, T1, T0))
    return plan, out


def reduced(cs, tl=None):
    """The factorised formula in float64; the outputs of brute_force."""
    theta, logw, u, logv = grid_of(cs)
    Gg, Gh, S, y = len(theta), len(u), len(cs["specific_dims"]), cs["y"]
    _, tl = testlet_logliks(cs) if tl is None else tl
    lv = logv.astype(np.float64)
    F = np.broadcast_to(logw.astype(np.float64)[None, :], (len(y), Gg)) + (y == 255).sum(1, keepdims=True) * cn.missing_constant()
    cond = {}
    for s, items, T1, T0 in tl:
        ys = y[:, items]
        ll = ((ys == 1).astype(np.float64) @ T1 + (ys == 0).astype(np.float64) @ T0).reshape(len(y), Gg, Gh) + lv[None, None, :]
        mx = ll.max(2)
        w = np.exp(ll - mx[:, :, None])
        F = F + mx + np.log(w.sum(2))
        if s >= 0:
            w = w / w.sum(2, keepdims=True)
            cond[s] = (w @ u, w @ (u * u))
    out = _general(F, theta)
    post = np.exp(F - out["loglik"][:, None])
    v = np.exp(lv) / np.exp(lv).sum()
    pm = float((v * u).sum())
    out["eap_specific"] = np.full((len(y), S), pm)
    out["psd_specific"] = np.full((len(y), S), np.sqrt((v * u * u).sum() - pm * pm))
    for s, (e1, e2) in cond.items():
        m1 = (post * e1).sum(1)
        out["eap_specific"][:, s] = m1
        out["psd_specific"][:, s] = np.sqrt(np.maximum((post * e2).sum(1) - m1 * m1, 0.0))
    return out


# ---- the operand phase said again ----------------------------------------------------------------------------------------
def restated(cs, tl=None):
    """The outputs by the arithmetic of k_grid_bifactor / k_grid_bifactor_spec, in float32 numpy, step by step:

      - the tables are the oracle's, rounded to float32, T 2^10 as an fp16 head and the fp16 of the remainder (gp_put);
      - GB_TESTLET: a testlet's slots in chunks of 16 in the plan's order, the sum of a chunk's products of one table part and
        a 0/1 indicator taken as exact and rounded into the float32 accumulator -- T1 head, T1 low, T0 head, T0 low: four
        roundings a chunk;
      - GB_ROWS: v = fmaf(acc, 2^-10, logv[h]), one rounding; the maximum over h; s = the float32 sum of exp(v - max);
      - F = (logw[g] + miss) + the testlets' max + log s, one after the other in float32;
      - the fold over g: corner_cases.restated_posterior (weights about the maximum, moments about its node, float32 sums);
      - the second kernel: pw = exp(F - loglik) / s, E1 += pw s1, E2 += pw s2 over g in float32, sd = sqrt(E2 - E1^2)."""
    f32 = np.float32
    theta, logw, u, logv = grid_of(cs)
    Gg, Gh, S, y = len(theta), len(u), len(cs["specific_dims"]), cs["y"]
    plan, tl = testlet_logliks(cs) if tl is None else tl
    u32, lv32 = u.astype(f32), logv.astype(f32)
    miss = ((y == 255).sum(1).astype(f32) * f32(cn.missing_constant())).astype(f32)
    F = (logw.astype(f32)[None, :] + miss[:, None]).astype(f32)
    kept = {}
    for s, items, T1, T0 in tl:
        parts = []
        for T in (T1, T0):
            h, lo = cn._split16(T.astype(f32) * f32(1024.0))
            parts += [h.astype(np.float64), lo.astype(np.float64)]
        ys = y[:, items]
        ind = ((ys == 1).astype(np.float64), (ys == 0).astype(np.float64))
        acc = np.zeros((len(y), Gg * Gh), f32)
        for j0 in range(0, len(items), 16):                         # (the padding slots of the last chunk add nothing)
            for k, part in enumerate(parts):
                acc = (acc.astype(np.float64) + ind[k >> 1][:, j0:j0 + 16] @ part[j0:j0 + 16]).astype(f32)
        v = (acc.astype(np.float64).reshape(len(y), Gg, Gh) * 2.0 ** -10 + lv32.astype(np.float64)[None, None, :]).astype(f32)
        mx = v.max(2)
        e = np.exp((v - mx[:, :, None]).astype(f32)).astype(f32)
        ssum = e.sum(2, dtype=f32)
        F = (F + (mx + np.log(ssum).astype(f32)).astype(f32)).astype(f32)
        if s >= 0:
            kept[s] = (ssum, (e * u32).sum(2, dtype=f32), (e * u32 * u32).sum(2, dtype=f32))
    r = cn.restated_posterior(F, theta[:, None])
    out = {"loglik": r["loglik"], "eap_general": r["mean"][:, 0], "psd_general": r["sd"][:, 0], "node": r["node"], "F": F}
    v64 = np.exp(logv.astype(np.float64))
    v64 = v64 / v64.sum()
    pm = float((v64 * u).sum())
    out["eap_specific"] = np.full((len(y), S), pm, f32)
    out["psd_specific"] = np.full((len(y), S), np.sqrt((v64 * u * u).sum() - pm * pm), f32)
    post = np.exp((F - r["loglik"][:, None]).astype(f32)).astype(f32)
    for s, (ssum, s1, s2) in kept.items():
        pw = (post / ssum).astype(f32)
        E1, E2 = (pw * s1).sum(1, dtype=f32), (pw * s2).sum(1, dtype=f32)
        out["eap_specific"][:, s] = E1
        out["psd_specific"][:, s] = np.sqrt(np.maximum(E2 - E1 * E1, f32(0)))
    return out


# ---- a case with everything the tests hold it to -------------------------------------------------------------------------
OUTPUTS = ("loglik", "eap_general", "psd_general", "eap_specific", "psd_specific")
_O = {}


def oracle_of(case):
    """cs, want (the reduced oracle: float64), brute (the brute force where the case is in BRUTE, else None), r (restated), e
    (the restatement's row errors by output), cap, tol (the row rule by output), d_f, gap_thr and left_out (the share of the
    persons the node rule leaves out in the oracle alone)."""
    if case[0] in _O:
        return _O[case[0]]
    cs = case_of(case)
    tl = testlet_logliks(cs)
    want = reduced(cs, tl)
    r = restated(cs, tl)
    brute = brute_force(cs, with_empty=cs["name"] in BRUTE_WITH_EMPTY) if cs["name"] in BRUTE else None
    near = want["F"] >= want["F"].max(1, keepdims=True) - cn.NEAR
    d_f = float(np.abs(r["F"].astype(np.float64) - want["F"])[near].max())
    e = {k: cn._row_errors(r[k], want[k], 1.0) for k in OUTPUTS}
    cap = cn.tol_cap(want["loglik"])
    gap_thr = max(sc.ARGMAX_GAP, 4.0 * d_f)
    out = {"cs": cs, "want": want, "brute": brute, "r": r, "e": e, "cap": cap, "tol": {k: cn.row_tol(v, cap) for k, v in e.items()},
           "d_f": d_f, "gap_thr": gap_thr, "left_out": float((want["gap"] <= gap_thr).mean())}
    _O[case[0]] = out
    return out


def condition(cs, want):
    """(the smallest oracle PSD of the general dimension and of the specific dimensions with items, half the general node
    spacing, half the specific one)."""
    on = [s for s in range(len(cs["specific_dims"])) if (cs["testlet"] == s).any()]
    Gg, Gh = cs["nodes"]
    return (float(want["psd_general"].min()), float(want["psd_specific"][:, on].min()) if on else np.inf,
            0.5 * 2.0 * cs["span"][0] / (Gg - 1), 0.5 * 2.0 * cs["span"][1] / max(Gh - 1, 1))


def shuffled(cs, seed=99):
    """The same model and data with the items in another order: (cs', perm), item k of cs' = item perm[k] of cs."""
    perm = np.random.RandomState(seed).permutation(cs["J"])
    out = dict(cs)
    out["params"] = {k: (v[:, perm] if k == "a" else v[perm]) for k, v in cs["params"].items()}
    out["free"], out["y"], out["testlet"] = cs["free"][:, perm], cs["y"][:, perm], cs["testlet"][perm]
    return out, perm
