"""The cases, the float64 oracles, the restated arithmetic and the float64 EM of the bifactor E-step and fit
(IrtEngine.expected_counts_bifactor / fit_em_bifactor on vipsy_amd/csrc/k_grid_bifactor_counts.hip; tests/test_bifactor_em_host.py
on the CPU, tests/test_gpu_bifactor_em.py on the GPU).  The cases are those of tests/bifactor_cases.py, by import, and two drawn
here for the EM; everything is computed once a case and callers must not modify it.

Oracles, float64 numpy:

    brute force   the joint posterior on the tensor grid Gg x Gh^S' (the specific dimensions that have items), marginalised to
                  (g, h_s) for every testlet -- for the pseudo-testlet to g, times the normalised v_h -- and contracted with the
                  indicators.  It does not use the reduction.  Possible for bifactor_cases.BRUTE.
    reduced       post_i(g) r_is(g, h) with r from the testlet's own log-sum-exp, usable for every case.

restated_counts() says the kernel's arithmetic again in float32: r from the restated rows of bifactor_cases.restated (v, its
maximum, e = exp(v - max), their float32 sum), p = e (post / s), p 2^14 as an fp16 head and low term, and float32 sums over
persons in the kernel's order -- a wave's units ascending, sixteen persons a k-step, the four waves, the person chunks of
gbc_plan (vipsy_amd/csrc/grid_plan.h, said again here), the host's slabs.  A model for a bound, not a bit-for-bit twin.

em() is Bock-Aitkin EM around an E-step of this file and the M-step oracle of tests/map_cases.py with D = 2."""
import numpy as np

from tests import bifactor_cases as bc
from tests import corner_cases as cn
from tests import map_cases as mc

COUNT_CASES = ("s2_2pl", "s5_3pl", "s3_full_tile", "s40", "s2_4pl_dc", "gh1")
TABLES = ("n1", "n0", "mass", "mass_s")

# ---- gbc_plan, said again ------------------------------------------------------------------------------------------------
GBC_CG, GBC_NG, GBC_WAVES, GBC_MIN_ROUNDS, GBC_MAX_BLOCKS, GBC_MIN_CHUNKS = 2, 2, 4, 2, 256, 4


def gbc_plan(nb, KC, Gg, n_tl):
    """(n_gpairs, n_units, units_per_chunk, n_chunks, slab_len) of vx_grid_bifactor_counts."""
    n_gpairs = (Gg + GBC_NG - 1) // GBC_NG
    n_units = (nb + 63) // 64
    rounds = (n_units + GBC_WAVES - 1) // GBC_WAVES
    chunks = min((rounds + GBC_MIN_ROUNDS - 1) // GBC_MIN_ROUNDS, max(GBC_MAX_BLOCKS // n_gpairs, GBC_MIN_CHUNKS))
    rpc = (rounds + chunks - 1) // chunks
    return {"n_gpairs": n_gpairs, "n_units": n_units, "units_per_chunk": rpc * GBC_WAVES, "n_chunks": (rounds + rpc - 1) // rpc,
            "slab_len": 2 * 16 * KC * Gg * 32 + n_tl * Gg * 32 + Gg}


def gbc_groups(tl_start):
    return int(sum((int(b) - int(a) + GBC_CG - 1) // GBC_CG for a, b in zip(tl_start[:-1], tl_start[1:])))


# ---- cases ---------------------------------------------------------------------------------------------------------------
# Gg = 2 and two testlets of 3 and 17 items: two workgroups a person chunk, so the plan cuts the persons.  N from the plan: 1 100
# persons are 18 units of 64 (the last one ragged: 12 persons), five rounds of four units, three chunks of two rounds.
CUT = ("cut_g2", 1100, (3, 17), 0, "irt_2pl", 1.0, (2, 5), 0.10, 31, 0)
# the two end-to-end cases of the EM
EM_2PL = ("em_2pl", 512, (6, 6, 6), 2, "irt_2pl", 1.0, (21, 11), 0.05, 32, 0)
EM_3PL = ("em_3pl", 512, (8, 8), 0, "irt_3pl", 1.0, (21, 11), 0.05, 33, 0)
EM_PRIOR = {"em_2pl": None, "em_3pl": {"c": (-1.4, 1.0)}}
EM_ITERS = 25


# A testlet of 35 items is three chunks: two chunk groups of GBC_CG = 2, the second one short -- its product 1 runs over all three
# chunks in both groups, and only the first group owns the testlet's mass_s (and, the testlet being the layout's first, mass).
# Gg = 3: a ragged last pair of general nodes.  ZERO_ITEMS: an item of it that nobody answered correctly and one that nobody
# answered wrongly (exact zeros in n1 / n0), made by case_by_name.
GROUPS = ("groups_35", 100, (35, 3), 0, "irt_2pl", 1.0, (3, 7), 0.10, 34, 0)
ZERO_ITEMS = {"groups_35": (34, 49)}         # layout SLOTS: (the item without a 1: third chunk of the 35; without a 0: of the 3)


def case_named(name):
    for c in (CUT, GROUPS, EM_2PL, EM_3PL):
        if c[0] == name:
            return c
    return bc.by_name(name)


_CS = {}


def case_by_name(name):
    """bifactor_cases.case_of of the named case; for the cases of ZERO_ITEMS with the answers 1 of the first item turned into 0
    and the answers 0 of the second into 1."""
    if name not in _CS:
        cs = bc.case_of(case_named(name))
        if name in ZERO_ITEMS:
            from vipsy_amd.grid import bifactor_plan
            col = bifactor_plan(cs["testlet"], cs["specific_dims"], cs["nodes"][0])["col"]
            no1, no0 = (int(col[s]) for s in ZERO_ITEMS[name])
            y = cs["y"].copy()
            y[y[:, no1] == 1, no1] = 0
            y[y[:, no0] == 0, no0] = 1
            cs = dict(cs, y=y)
        _CS[name] = cs
    return _CS[name]


# ---- the two oracles -----------------------------------------------------------------------------------------------------
def _indicators(y, items):
    ys = y[:, items]
    return (ys == 1).astype(np.float64), (ys == 0).astype(np.float64)


def reduced_counts(cs, tl=None):
    """n1, n0 [J][Gg Gh], mass [Gg], mass_s [n_tl][Gg Gh] (the plan's testlet order, the pseudo-testlet last), loglik [N], post
    [N][Gg] by the factorised formula in float64."""
    theta, logw, u, logv = bc.grid_of(cs)
    Gg, Gh, y = len(theta), len(u), cs["y"]
    tl = bc.testlet_logliks(cs) if tl is None else tl
    want = bc.reduced(cs, tl)
    post = np.exp(want["F"] - want["loglik"][:, None])
    lv = logv.astype(np.float64)
    out = {"n1": np.zeros((cs["J"], Gg * Gh)), "n0": np.zeros((cs["J"], Gg * Gh)), "mass": post.sum(0),
           "mass_s": np.zeros((len(tl[1]), Gg * Gh)), "loglik": want["loglik"], "post": post, "F": want["F"]}
    for t, (s, items, T1, T0) in enumerate(tl[1]):
        i1, i0 = _indicators(y, items)
        ll = (i1 @ T1 + i0 @ T0).reshape(len(y), Gg, Gh) + lv[None, None, :]
        mx = ll.max(2, keepdims=True)
        w = np.exp(ll - mx)
        p = (post[:, :, None] * (w / w.sum(2, keepdims=True))).reshape(len(y), Gg * Gh)
        out["n1"][items], out["n0"][items], out["mass_s"][t] = i1.T @ p, i0.T @ p, p.sum(0)
    return out


def brute_counts(cs):
    """The same tables from the joint posterior on the tensor grid (bifactor_cases.brute_force's grid), without the reduction."""
    theta, logw, u, logv = bc.grid_of(cs)
    Gg, Gh, S, y = len(theta), len(u), len(cs["specific_dims"]), cs["y"]
    plan, tls = bc.testlet_logliks(cs)
    on = [s for s in range(S) if (cs["testlet"] == s).any()]
    axes = np.meshgrid(theta, *([u] * len(on)), indexing="ij")
    lws = np.meshgrid(logw.astype(np.float64), *([logv.astype(np.float64)] * len(on)), indexing="ij")
    coord = np.zeros((axes[0].size, cs["D"]))
    coord[:, cs["general"]] = axes[0].reshape(-1)
    for k, s in enumerate(on):
        coord[:, cs["specific_dims"][s]] = axes[1 + k].reshape(-1)
    logw_full = sum(w.reshape(-1) for w in lws)
    T1, T0 = cn.item_tables(cs, "irt", coord)
    f = cn.loglik_from_tables(T1, T0, y) + logw_full[None, :]
    m = f.max(1, keepdims=True)
    lk = (m + np.log(np.exp(f - m).sum(1, keepdims=True)))[:, 0]
    joint = np.exp(f - lk[:, None]).reshape((len(y), Gg) + (Gh,) * len(on))
    post = joint.reshape(len(y), Gg, -1).sum(2)
    v = np.exp(logv.astype(np.float64))
    v = v / v.sum()
    out = {"n1": np.zeros((cs["J"], Gg * Gh)), "n0": np.zeros((cs["J"], Gg * Gh)), "mass": post.sum(0),
           "mass_s": np.zeros((len(tls), Gg * Gh)), "loglik": lk, "post": post}
    for t, (s, items, _, _) in enumerate(tls):
        if s >= 0:
            other = tuple(2 + k for k in range(len(on)) if on[k] != s)
            p = joint.sum(other) if other else joint
        else:
            p = post[:, :, None] * v[None, None, :]
        p = p.reshape(len(y), Gg * Gh)
        i1, i0 = _indicators(y, items)
        out["n1"][items], out["n0"][items], out["mass_s"][t] = i1.T @ p, i0.T @ p, p.sum(0)
    return out


# ---- the kernel's arithmetic said again ----------------------------------------------------------------------------------
def _tree32(x):
    """The sum over 32 lanes [32][...] by the xor steps 16, 8, 4, 2, 1 in float32, as lane 0 ends up with it."""
    idx = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        x = (x + x[idx ^ o]).astype(np.float32)
    return x[0]


def _units_of(n, Gg, slab_persons):
    """The kernel's order of the persons: for every host slab, every person chunk, every wave: the units (first person, count)."""
    out = []
    for s0 in range(0, n, slab_persons):
        nb = min(n, s0 + slab_persons) - s0
        p = gbc_plan(nb, 1, Gg, 1)
        chunks = []
        for c in range(p["n_chunks"]):
            lo, hi = c * p["units_per_chunk"], min(p["n_units"], (c + 1) * p["units_per_chunk"])
            chunks.append([[(s0 + 64 * k, min(64, nb - 64 * k)) for k in range(lo + w, hi, GBC_WAVES)] for w in range(GBC_WAVES)])
        out.append(chunks)
    return out


def _sum_f32(parts):
    s = np.zeros_like(parts[0], dtype=np.float32)
    for x in parts:
        s = (s + x).astype(np.float32)
    return s


def restated_counts(cs, tl=None, slab_persons=None):
    """The tables by the arithmetic of k_grid_bifactor_counts in float32 numpy (see the module's header); slab_persons: the
    host's slab (default: everybody in one)."""
    f32 = np.float32
    theta, logw, u, logv = bc.grid_of(cs)
    Gg, Gh, y, N = len(theta), len(u), cs["y"], len(cs["y"])
    tl = bc.testlet_logliks(cs) if tl is None else tl
    r = bc.restated(cs, tl)
    post = np.exp((r["F"] - r["loglik"][:, None]).astype(f32)).astype(f32)
    lv32 = logv.astype(f32)
    order = _units_of(N, Gg, N if slab_persons is None else slab_persons)
    kstep = [np.concatenate([np.arange(8 * s, 8 * s + 8), 32 + np.arange(8 * s, 8 * s + 8)]) for s in range(4)]

    def lanes(p):                                                   # [N][...] -> the sum a person chunk by lanes, waves; slabs
        slabs = []
        for chunks in order:
            cs_ = []
            for waves in chunks:
                ws = []
                for units in waves:
                    acc = np.zeros((32,) + p.shape[1:], f32)
                    for p0, cnt in units:
                        for half in (0, 32):
                            k = min(max(cnt - half, 0), 32)
                            acc[:k] = (acc[:k] + p[p0 + half:p0 + half + k]).astype(f32)
                    ws.append(_tree32(acc))
                cs_.append(_sum_f32(ws))
            slabs.append(_sum_f32(cs_))
        return _sum_f32(slabs)

    def mfma(ind, hp, lp):                                          # [N][k] x [N][GG] -> [k][GG]
        slabs = []
        for chunks in order:
            cs_ = []
            for waves in chunks:
                ws = []
                for units in waves:
                    acc = np.zeros((ind.shape[1], hp.shape[1]), f32)
                    for p0, cnt in units:
                        for ks in kstep:
                            idx = p0 + ks[ks < cnt]
                            if idx.size:
                                acc = (acc.astype(np.float64) + ind[idx].T @ hp[idx]).astype(f32)
                                acc = (acc.astype(np.float64) + ind[idx].T @ lp[idx]).astype(f32)
                    ws.append(acc)
                tot = ws[0]
                for x in ws[1:]:
                    tot = (tot + x).astype(f32)
                cs_.append((tot * f32(2.0 ** -14)).astype(f32))
            slabs.append(_sum_f32(cs_))
        return _sum_f32(slabs)

    out = {"n1": np.zeros((cs["J"], Gg * Gh), f32), "n0": np.zeros((cs["J"], Gg * Gh), f32), "mass": lanes(post),
           "mass_s": np.zeros((len(tl[1]), Gg * Gh), f32), "loglik": r["loglik"]}
    for t, (s, items, T1, T0) in enumerate(tl[1]):
        parts = []
        for T in (T1, T0):
            h, lo = cn._split16(T.astype(f32) * f32(1024.0))
            parts += [h.astype(np.float64), lo.astype(np.float64)]
        i1, i0 = _indicators(y, items)
        acc = np.zeros((N, Gg * Gh), f32)
        for j0 in range(0, len(items), 16):
            for k, part in enumerate(parts):
                acc = (acc.astype(np.float64) + (i1, i0)[k >> 1][:, j0:j0 + 16] @ part[j0:j0 + 16]).astype(f32)
        v = (acc.astype(np.float64).reshape(N, Gg, Gh) * 2.0 ** -10 + lv32.astype(np.float64)[None, None, :]).astype(f32)
        e = np.exp((v - v.max(2, keepdims=True)).astype(f32)).astype(f32)
        pw = (post / e.sum(2, dtype=f32)).astype(f32)
        p = (e * pw[:, :, None]).astype(f32).reshape(N, Gg * Gh)
        hp, lp = cn._split16((p * f32(16384.0)).astype(f32))
        hp, lp = hp.astype(np.float64), lp.astype(np.float64)
        out["n1"][items], out["n0"][items], out["mass_s"][t] = mfma(i1, hp, lp), mfma(i0, hp, lp), lanes(p)
    return out


# ---- what a case's tables are held to ------------------------------------------------------------------------------------
_O = {}


def oracle_of(name):
    """cs, plan, want (reduced), r (restated), e (the restatement's row errors by table), cap and tol (the row rule by table)."""
    if name in _O:
        return _O[name]
    cs = case_by_name(name)
    tl = bc.testlet_logliks(cs)
    want, r = reduced_counts(cs, tl), restated_counts(cs, tl)
    e = {k: row_error(r[k], want[k]) for k in TABLES}
    cap = cn.tol_cap(want["loglik"])
    _O[name] = {"cs": cs, "plan": tl[0], "want": want, "r": r, "e": e, "cap": cap, "tol": {k: cn.row_tol(v, cap) for k, v in e.items()}}
    return _O[name]


def row_error(got, want):
    """The project's row rule on a table: rows = items / testlets; mass is one row."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.ndim == 1:
        got, want = got[None, :], want[None, :]
    return cn._row_errors(got.reshape(len(got), -1), want.reshape(len(want), -1), 1.0)


def identities(t, cs, Gg, Gh):
    """The three count identities as relative errors: sum_h (n1 + n0)[j][g][h] against sum_{i answered j} post_i(g) needs the
    posterior and is taken by the caller's oracle; here what the tables alone give -- (sum_{g,h} mass_s[t] / N - 1,
    sum_h mass_s[t][g][h] against mass[g], sum_{g,h} (n1 + n0)[j] against the persons who answered j)."""
    ms = np.asarray(t["mass_s"], np.float64).reshape(-1, Gg, Gh)
    mass = np.asarray(t["mass"], np.float64)
    n = (np.asarray(t["n1"], np.float64) + np.asarray(t["n0"], np.float64)).reshape(-1, Gg, Gh)
    cnt = (cs["y"] != 255).sum(0).astype(np.float64)
    return (float(np.abs(ms.sum((1, 2)) / len(cs["y"]) - 1.0).max()),
            float((np.abs(ms.sum(2) - mass[None, :]).max(1) / np.maximum(np.abs(mass).max(), 1.0)).max()),
            float((np.abs(n.sum((1, 2)) - cnt) / np.maximum(cnt, 1.0)).max()))


def answered_mass(cs, post):
    """sum_{i answered j} post_i(g): [J][Gg]."""
    return (cs["y"] != 255).astype(np.float64).T @ post


# ---- the EM --------------------------------------------------------------------------------------------------------------
def em_operands(cs):
    """(sd int64 [J], has bool [J], fr bool [6][J]) of the two-dimensional M-step: the rows b, a_general, a_specific, -, c, d."""
    from vipsy_amd.grid import bifactor_em_index
    sd, has = bifactor_em_index({"testlet": cs["testlet"], "specific_dims": cs["specific_dims"], "general": cs["general"]})
    m = mc.MODEL_NO[cs["model"]]
    fr = np.zeros((mc.ROWS, cs["J"]), bool)
    fr[0], fr[1], fr[2], fr[4], fr[5] = True, cs["free"][cs["general"]] != 0, has, m >= 3, m == 4
    return sd, has, fr


def em_prior_rows(cs, prior):
    from vipsy_amd.grid import bifactor_em_prior
    sd, has, _ = em_operands(cs)
    if prior is None:
        return np.zeros((2, mc.ROWS, cs["J"]), np.float32)
    return bifactor_em_prior(prior, cs["model"], cs["D"], cs["J"], cs["general"], sd, has)


def em_start(cs):
    """Every item alike, the loadings that are not free zero: what the tests put on the engine before fit_em_bifactor."""
    out = {"a": (cs["free"] * 1.0).astype(np.float32), "b": np.zeros(cs["J"], np.float32)}
    if "c" in cs["params"]:
        out["c"] = np.full(cs["J"], -1.4, np.float32)
    if "d" in cs["params"]:
        out["d"] = np.full(cs["J"], 2.2, np.float32)
    return out


def em_iteration(cs, params, prior_rows, estep, dtype, newton=4):
    """(the leaves after one iteration from `params`, the tables' loglik sum, the log prior of `params`)."""
    sd, has, fr = em_operands(cs)
    J, g = cs["J"], cs["general"]
    theta, _, u, _ = bc.grid_of(cs)
    tg, uh = np.meshgrid(theta, u, indexing="ij")
    theta2 = np.stack([tg.reshape(-1), uh.reshape(-1)], 1)
    t = estep(dict(cs, params=params))
    p0 = np.zeros((mc.ROWS, J), np.float64)
    a = np.asarray(params["a"], np.float64)
    p0[0], p0[1], p0[2] = np.asarray(params["b"], np.float64).reshape(J), a[g], np.where(has, a[sd, np.arange(J)], 0.0)
    for k, row in (("c", 4), ("d", 5)):
        if k in params:
            p0[row] = np.asarray(params[k], np.float64).reshape(J)
    p = map_mstep2(cs, t["n1"], t["n0"], p0, prior_rows, newton, dtype, fr, theta2)
    new = {"a": a.copy(), "b": p[0].copy()}
    new["a"][g] = p[1]
    new["a"][sd[has], np.arange(J)[has]] = p[2][has]
    for k, row in (("c", 4), ("d", 5)):
        if k in params:
            new[k] = p[row].copy()
    if dtype == np.float32:
        new = {k: v.astype(np.float32) for k, v in new.items()}
    return new, float(np.asarray(t["loglik"], np.float64).sum()), float(mc.log_prior(p0, fr, prior_rows).sum())


def map_mstep2(cs, n1, n0, p0, prior_rows, newton, dtype, fr, theta2):
    return np.asarray(mc.map_mstep({"model": cs["model"], "Dc": cs["Dc"], "J": cs["J"], "D": 2}, np.asarray(n1, dtype),
                                   np.asarray(n0, dtype), p0.astype(dtype), prior_rows, newton, dtype, fr=fr, theta=theta2), np.float64)


_EM = {}


def em(name, iters=EM_ITERS, dtype=np.float64):
    """The EM of a case from em_start, computed once and shared: (leaves after 0 .. iters iterations, loglik, logpost [iters]);
    dtype float64: the reduced oracle's E-step and the float64 M-step; float32: the restated E-step and the float32 M-step."""
    key = (name, iters, np.dtype(dtype).name)
    if key not in _EM:
        cs = case_by_name(name)
        pr = em_prior_rows(cs, EM_PRIOR[name])
        estep = reduced_counts if dtype == np.float64 else restated_counts
        ps, lks, lps = [{k: np.asarray(v, dtype) for k, v in em_start(cs).items()}], [], []
        for _ in range(iters):
            new, lk, lp = em_iteration(cs, ps[-1], pr, estep, dtype)
            ps.append(new)
            lks.append(lk)
            lps.append(lk + lp)
        _EM[key] = (ps, lks, lps)
    return _EM[key]


# the margin of tests/test_gpu_map_paths.py: the GPU is held to a bound whose half the float32 restatement meets on the CPU
EM_MARGIN = 2.0


def em_distance(name):
    """The largest distance of any leaf entry between the float64 EM and the same EM on the float32 restatement, after EM_ITERS."""
    p64, p32 = em(name)[0][-1], em(name, dtype=np.float32)[0][-1]
    return max(float(np.abs(np.asarray(p32[k], np.float64) - p64[k]).max()) for k in p64)
