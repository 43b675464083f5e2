"""The bifactor E-step and fit on the GPU (vx_grid_bifactor_counts behind IrtEngine.expected_counts_bifactor / fit_em_bifactor and the
model classes' methods) against the float64 oracles of tests/bifactor_em_cases.py.

Item parameters are drawn and set on the engine through its views, not trained.  Every table -- n1, n0 (a row an item), mass (one
row), mass_s (a row a testlet) -- is held to the reduced oracle by the project's row rule, _row_errors(got, want, floor = 1) <=
row_tol(e_restated, tol_cap(loglik)) (tests/corner_cases.py; tests/test_bifactor_em_host.py asserts on the CPU that the
restatement itself meets a third of it), and the three count identities to the same tolerance.  The errors found are printed.

The EM end to end (test_em_end_to_end): 25 iterations from bifactor_em_cases.em_start end where the float64 EM oracle's own 25 end,
every leaf entry within EM_MARGIN = 2 times the distance, on the CPU, between that oracle and the same EM on the float32
restatement (test_the_float64_em_rises_and_the_restated_em_follows_it prints it) -- the margin of tests/test_gpu_map_paths.py, whose
bound the restatement meets at a half: 2 x 4.9e-7 = 9.7e-7 for em_2pl and 2 x 3.7e-7 = 7.4e-7 for em_3pl.

Shapes: the smallest at which the kernel can go wrong -- the cases of bifactor_cases.CASES the E-step is held on,
bifactor_em_cases.CUT, whose plan cuts 1 100 persons into three chunks with a ragged last unit, and bifactor_em_cases.GROUPS, whose
testlet of 35 items takes two chunk groups and two of whose items lack an answer 1 / an answer 0."""
import numpy as np
import pytest
import torch

from tests import bifactor_cases as bc
from tests import bifactor_em_cases as be
from tests import corner_cases as cn
from tests.test_gpu_bifactor import _cross_case, _engine, _np
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(_dev())


_GOT = {}


def _got(name):
    """The engine of a case and its expected_counts_bifactor(), computed once and shared (never modified)."""
    if name not in _GOT:
        cs = be.oracle_of(name)["cs"]
        eng = _engine(cs)
        got = eng.expected_counts_bifactor(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
        torch.cuda.synchronize()
        _GOT[name] = (eng, got)
    return _GOT[name]


def _direct(eng, cs, y=None, keep=None, scores=None, accumulate=False, into=None):
    """vx_grid_bifactor (unless scores = (loglik, fws) of an earlier call) and vx_grid_bifactor_counts called by hand on the
    persons `y` (default: the case's), into tables that start as NaN (or `into`).  keep: the testlets of the plan, by index,
    that stay in the LAYOUT -- columns, image and responses are cut down to them, F and loglik are whatever `scores` says.
    Returns (tables, (loglik, fws), (col, tl_start) of the layout used)."""
    bf = eng._bifactor_call(None if y is None else torch.from_numpy(y), None, cs["nodes"], cs["span"], cs["general"])
    bf.fill()
    b_, plan, dev = eng.be, bf.plan, _dev()
    (_, _, yp), = list(bf.slabs())
    n, Gg, Gh, J = bf.n, bf.Gg, bf.Gh, bf.J
    f32 = dict(dtype=torch.float32, device=dev)
    if scores is None:
        loglik, mean, sd = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)
        fws = torch.empty(b_.grid_bifactor_workspace(n, Gg), **f32)
        b_.grid_bifactor(yp, n, bf.KC, plan["tl_start"], bf.tl_dev, bf.img, bf.logw, bf.theta, bf.logv, bf.u, loglik, mean, sd,
                         torch.empty(n, dtype=torch.int32, device=dev), fws)
    else:
        loglik, fws = scores
    col_np, tl_start, KC, img, col, tl_dev = plan["col"], plan["tl_start"], bf.KC, bf.img, bf.col, bf.tl_dev
    if keep is not None:
        slots = np.concatenate([np.arange(16 * tl_start[t], 16 * tl_start[t + 1]) for t in keep])
        col_np = plan["col"][slots]
        tl_start = np.concatenate([[0], np.cumsum([tl_start[t + 1] - tl_start[t] for t in keep])]).astype(np.int32)
        KC = int(tl_start[-1])
        col, sdim, tl_dev = _t(col_np), _t(plan["sdim"][slots]), _t(tl_start)
        img = torch.empty(b_.grid_bifactor_image_bytes(Gg, KC), dtype=torch.uint8, device=dev)
        flat = lambda name: eng.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
        b_.grid_table_bifactor(b_.cfg(eng.model, eng.D_model, J, 0, eng.Dc, 1.0, 0, 0, 0), bf.theta, bf.u, cs["general"], col, sdim,
                               KC, eng.unconstrained("a").contiguous(), flat("b"),
                               flat("c") if eng.model in ("irt_3pl", "irt_4pl") else None,
                               flat("d") if eng.model == "irt_4pl" else None, img)
        yp = yp[:, _t(slots)].contiguous()
    n_tl = len(tl_start) - 1
    nan = lambda *shape: torch.full(shape, float("nan"), **f32)                   # noqa: E731
    t = into or {"n1": nan(J, Gg * Gh), "n0": nan(J, Gg * Gh), "mass": nan(Gg), "mass_s": nan(n_tl, Gg * Gh)}
    ws = nan(b_.grid_bifactor_counts_workspace(n, KC, Gg, n_tl))
    b_.grid_bifactor_counts(yp, n, KC, Gg, tl_start, tl_dev, col, J, img, bf.logv, loglik, fws, accumulate, t["n1"], t["n0"],
                            t["mass"], t["mass_s"], ws)
    torch.cuda.synchronize()
    return t, (loglik, fws), (col_np, tl_start)


def _hold(tag, t, o):
    """The row rule on n1, n0, mass, mass_s (numpy, the plan's testlet order) and the identities; prints what it finds."""
    cs, want = o["cs"], o["want"]
    Gg, Gh = cs["nodes"]
    errs = {k: be.row_error(t[k], want[k]) for k in be.TABLES}
    total, rows, answered = be.identities(t, cs, Gg, Gh)
    n = (np.asarray(t["n1"], np.float64) + np.asarray(t["n0"], np.float64)).reshape(cs["J"], Gg, Gh).sum(2)
    am = be.answered_mass(cs, want["post"])
    per_g = float((np.abs(n - am).max(1) / np.maximum(np.abs(am).max(1), 1.0)).max())
    print("%s: %s; identities: sum mass_s / N - 1 %.1e, sum_h mass_s against mass %.1e, sum n against the answers %.1e, sum_h n against "
          "the answered mass %.1e" % (tag, "  ".join("%s %.2e (tol %.1e)" % (k, errs[k], o["tol"][k]) for k in be.TABLES), total,
                                      rows, answered, per_g))
    for k in be.TABLES:
        assert np.isfinite(t[k]).all(), (tag, k)
        assert errs[k] <= o["tol"][k], (tag, k, errs[k], o["tol"][k])
    assert total <= o["tol"]["mass_s"] and rows <= o["tol"]["mass_s"], (tag, total, rows)
    assert answered <= o["tol"]["n1"] and per_g <= o["tol"]["n1"], (tag, answered, per_g)
    for k, v in (("n1", 1), ("n0", 0)):                                           # nobody gave that answer: exact zeros
        none = ~(cs["y"] == v).any(0)
        assert none.any() or cs["name"] not in be.ZERO_ITEMS, (tag, k, "the case was made to have such an item")
        assert (np.asarray(t[k])[none] == 0).all(), (tag, k)


def _public_tables(got, o):
    """expected_counts_bifactor()'s tables as the oracle has them: flat nodes, mass_s in the plan's testlet order."""
    plan = o["plan"]
    J = o["cs"]["J"]
    ms = _np(got["mass_specific"])
    return {"n1": _np(got["n1"]).reshape(J, -1), "n0": _np(got["n0"]).reshape(J, -1), "mass": _np(got["mass"]),
            "mass_s": np.stack([ms[s].reshape(-1) if s >= 0 else np.full(ms[0].size, np.nan) for s in plan["tl_column"]])}


# ---- 1. the tables against the reduced oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", be.COUNT_CASES)
def test_tables_vs_oracle(name):
    o = be.oracle_of(name)
    cs, want, plan = o["cs"], o["want"], o["plan"]
    eng, got = _got(name)
    J, S, (Gg, Gh) = cs["J"], len(cs["specific_dims"]), cs["nodes"]
    for k in ("n1", "n0", "prob"):
        assert tuple(got[k].shape) == (J, Gg, Gh) and got[k].dtype == torch.float32, k
    assert tuple(got["mass"].shape) == (Gg,) and tuple(got["mass_specific"].shape) == (S, Gg, Gh)
    assert tuple(got["theta"].shape) == (Gg,) and tuple(got["u"].shape) == (Gh,)
    # through the ABI, into tables that start as NaN: every entry is written, and the public path gives the same bits
    t, _, _ = _direct(eng, cs)
    pub = _public_tables(got, o)
    for k in be.TABLES:
        tk = _np(t[k])
        assert np.isfinite(tk).all(), (name, k)
        real = plan["tl_column"] >= 0 if k == "mass_s" else slice(None)
        assert np.array_equal(tk[real], pub[k][real]), (name, k)
    _hold(name, {k: _np(v) for k, v in t.items()}, o)
    # a specific dimension without items: the grid prior times mass
    v = np.exp(_np(got["logv"]).astype(np.float64))
    empty = _np(got["mass_specific"])[bc.EMPTY_AT]
    assert np.abs(empty - _np(got["mass"]).astype(np.float64)[:, None] * v[None, :]).max() <= cn.ROW_TOL
    # prob out of the image, loglik the device sum
    prob = np.zeros((J, Gg * Gh))
    for _, items, T1, _ in bc.testlet_logliks(cs)[1]:
        prob[items] = np.exp(T1)
    assert np.abs(_np(got["prob"]).reshape(J, -1) - prob).max() <= cn.ROW_TOL
    assert abs(float(got["loglik"]) - want["loglik"].sum()) <= cn.ROW_TOL * abs(want["loglik"].sum())
    # nobody's answers adds the prior: row 0 of every case
    assert (cs["y"][0] == 255).all()


# ---- 2. more than one wave round, more than one person chunk -------------------------------------------------------------
def test_the_plan_cuts_the_persons():
    name = be.CUT[0]
    o = be.oracle_of(name)
    cs, plan = o["cs"], o["plan"]
    eng, got = _got(name)
    N, Gg, n_tl = cs["N"], cs["nodes"][0], len(plan["tl_column"])
    p = be.gbc_plan(N, plan["KC"], Gg, n_tl)
    assert eng.be.grid_bifactor_counts_workspace(N, plan["KC"], Gg, n_tl) == p["n_chunks"] * p["slab_len"]
    assert p["n_chunks"] >= 2 and N % 64 != 0 and p["units_per_chunk"] > be.GBC_WAVES
    t, _, _ = _direct(eng, cs)
    _hold(name, {k: _np(v) for k, v in t.items()}, o)
    pub = _public_tables(got, o)
    for k in be.TABLES:
        assert np.array_equal(_np(t[k]), pub[k]), k


def test_a_testlet_of_more_than_two_chunks_takes_two_chunk_groups():
    """35 items are three chunks: the second chunk group of the testlet repeats product 1 over all three, accumulates the third
    chunk alone and leaves mass_s and mass to the first; three general nodes leave the last pair ragged.  An item of the third
    chunk has no answer 1 and an item of the other testlet no answer 0: exact zeros (_hold asserts that they exist)."""
    name = be.GROUPS[0]
    o = be.oracle_of(name)
    cs, plan = o["cs"], o["plan"]
    eng, got = _got(name)
    assert list(np.diff(plan["tl_start"])) == [3, 1] and be.gbc_groups(plan["tl_start"]) == 3 and cs["nodes"][0] % be.GBC_NG == 1
    t, _, _ = _direct(eng, cs)
    _hold(name, {k: _np(v) for k, v in t.items()}, o)
    pub = _public_tables(got, o)
    for k in be.TABLES:
        assert np.array_equal(_np(t[k]), pub[k]), k


# ---- 3. determinism and independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s2_2pl", "s40", be.CUT[0]])
def test_the_same_call_gives_the_same_bits(name):
    cs = be.oracle_of(name)["cs"]
    eng, got = _got(name)
    again = eng.expected_counts_bifactor(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass", "mass_specific", "prob", "loglik"):
        assert torch.equal(again[k], got[k]), k


def test_two_slabs_through_accumulate_are_added_in_that_order():
    cs = be.oracle_of(be.CUT[0])["cs"]
    eng, _ = _got(be.CUT[0])
    ya, yb = cs["y"][:768], cs["y"][768:]
    ta, _, _ = _direct(eng, cs, y=ya)
    tb, _, _ = _direct(eng, cs, y=yb)
    both = {k: v.clone() for k, v in ta.items()}
    _direct(eng, cs, y=yb, accumulate=True, into=both)
    for k in be.TABLES:
        assert torch.equal(both[k], ta[k] + tb[k]), k
        assert not torch.equal(both[k], ta[k])


def test_a_testlets_tables_do_not_depend_on_the_other_testlets_of_the_layout():
    """s5_3pl with the two-chunk testlet and the one-item testlet dropped from the LAYOUT, F and loglik kept: the other testlets'
    items, their mass_s rows and mass have the bits of the full call; the dropped items are not written."""
    name = "s5_3pl"
    o = be.oracle_of(name)
    cs, plan = o["cs"], o["plan"]
    eng, _ = _got(name)
    full, scores, _ = _direct(eng, cs)
    sizes = np.diff(plan["tl_start"])
    keep = [t for t in range(len(sizes)) if not (sizes[t] == 2 or (plan["col"][16 * plan["tl_start"][t]:16 * plan["tl_start"][t + 1]] >= 0).sum() == 1)]
    assert 0 < len(keep) < len(sizes) - 1 and 0 not in keep
    part, _, (col, _) = _direct(eng, cs, keep=keep, scores=scores)
    kept = col[col >= 0]
    gone = np.setdiff1d(np.arange(cs["J"]), kept)
    for k in ("n1", "n0"):
        assert torch.equal(part[k][_t(kept)], full[k][_t(kept)]), k
        assert bool(torch.isnan(part[k][_t(gone)]).all()), k
    assert torch.equal(part["mass_s"], full["mass_s"][_t(np.array(keep))]) and torch.equal(part["mass"], full["mass"])


def test_rows_and_new_data_give_the_tables_of_the_corresponding_full_call():
    name = "s40"
    cs = be.oracle_of(name)["cs"]
    eng, _ = _got(name)
    kw = dict(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
    rows = np.random.RandomState(4).permutation(cs["N"])[:71]
    sub = eng.expected_counts_bifactor(rows=torch.from_numpy(rows), **kw)
    new = eng.expected_counts_bifactor(torch.from_numpy(cs["y"][rows]), **kw)
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass", "mass_specific", "prob", "loglik"):
        assert torch.equal(sub[k], new[k]), k
    assert abs(float(sub["mass"].sum()) - len(rows)) <= cn.ROW_TOL * len(rows)


# ---- 4. consistency with what exists -------------------------------------------------------------------------------------
def _oracle_for(cs):
    tl = bc.testlet_logliks(cs)
    want, r = be.reduced_counts(cs, tl), be.restated_counts(cs, tl)
    cap = cn.tol_cap(want["loglik"])
    return want, {k: cn.row_tol(be.row_error(r[k], want[k]), cap) for k in be.TABLES}


def test_two_dimensions_are_the_tensor_grid_of_expected_counts():
    n = 21
    cs = dict(_cross_case(2, 20, 100, 42), nodes=(n, n), span=(6.0, 6.0), general=0, specific_dims=np.array([1]), name="cross2")
    cs["testlet"] = np.where(cs["free"][1] != 0, 0, -1).astype(np.int64)
    want, tol = _oracle_for(cs)
    eng = _engine(cs, own_mask=True)
    got = eng.expected_counts_bifactor(nodes=(n, n), span=(6.0, 6.0))
    full = eng.expected_counts(nodes=n, span=6.0)
    torch.cuda.synchronize()
    # an item on the general dimension alone has post(g) v_h here and the joint posterior of (theta, u) there: the same table
    # only after the sum over h (what its M-step sees, its specific loading being fixed at 0)
    on, alone = np.flatnonzero(cs["testlet"] >= 0), np.flatnonzero(cs["testlet"] < 0)
    assert len(alone) == 1

    def fold(v):
        v = np.asarray(v, np.float64).reshape(cs["J"], n, n)
        z = np.zeros((len(alone), n * n))
        z[:, :n] = v[alone].sum(2)
        return np.concatenate([v[on].reshape(len(on), -1), z])

    for k in ("n1", "n0", "mass"):
        g = fold(_np(got[k])) if k != "mass" else _np(got[k])
        f = fold(_np(full[k])) if k != "mass" else _np(full[k]).reshape(n, n).astype(np.float64).sum(1)
        w = fold(want[k]) if k != "mass" else want[k]
        eg, ef = be.row_error(g, w), be.row_error(f, w)
        print("x_feature = 2, %d nodes a dimension: %s bifactor %.2e, tensor grid %.2e (tol %.1e), between them %.2e"
              % (n, k, eg, ef, tol[k], be.row_error(g, f)))
        assert eg <= tol[k] and ef <= tol[k], (k, eg, ef)
    # the joint mass of (theta, u) is the tensor grid's own mass, node for node: one row, the rule of mass_s (testlet 0 of the plan)
    ms, fm, wm = _np(got["mass_specific"])[0].reshape(-1), _np(full["mass"]), want["mass_s"][0]
    eg, ef = be.row_error(ms, wm), be.row_error(fm, wm)
    print("x_feature = 2: mass_specific %.2e, the tensor grid's mass %.2e (tol %.1e), between them %.2e"
          % (eg, ef, tol["mass_s"], be.row_error(ms, fm)))
    assert eg <= tol["mass_s"] and ef <= tol["mass_s"], (eg, ef)
    assert np.abs(_np(got["prob"]).reshape(cs["J"], -1) - _np(full["prob"])).max() <= cn.ROW_TOL


def test_one_specific_node_is_the_unidimensional_model():
    name = "gh1"
    o = be.oracle_of(name)
    cs, want = o["cs"], o["want"]
    _, got = _got(name)
    one = _engine(cs, D=1, params={"a": cs["params"]["a"][cs["general"]:cs["general"] + 1], "b": cs["params"]["b"]})
    full = one.expected_counts(nodes=cs["nodes"][0], span=cs["span"][0])
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass"):
        g = _np(got[k]).reshape(_np(full[k]).shape)
        eg, ef = be.row_error(g, want[k]), be.row_error(_np(full[k]), want[k])
        print("gh1 against the 1-D expected_counts(): %s bifactor %.2e, 1-D %.2e (tol %.1e), between them %.2e"
              % (k, eg, ef, o["tol"][k], be.row_error(g, _np(full[k]))))
        assert eg <= o["tol"][k] and ef <= o["tol"][k], (k, eg, ef)


# ---- 5. one M-step through the public path -------------------------------------------------------------------------------
def _em_engine(name):
    cs = be.case_by_name(name)
    return cs, _engine(cs, params=be.em_start(cs))


@pytest.mark.parametrize("name", [be.EM_2PL[0], be.EM_3PL[0]])
def test_one_iteration_is_the_existing_mstep_on_the_returned_tables(name):
    from vipsy_amd import grid
    cs, eng = _em_engine(name)
    prior, kw = be.EM_PRIOR[name], dict(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
    J, (Gg, Gh) = cs["J"], cs["nodes"]
    start = {k: eng.unconstrained(k).clone() for k in be.em_start(cs)}
    t = eng.expected_counts_bifactor(**kw)
    out = eng.fit_em_bifactor(max_iter=1, newton=4, prior=prior, **kw)
    torch.cuda.synchronize()
    assert out["iterations"] == 1 and not out["converged"] and out["loglik"] == [float(t["loglik"])]
    sd_np, has_np = grid.bifactor_em_index(eng.bifactor_structure(cs["general"]))
    sd, has = _t(sd_np), _t(has_np)
    a2 = grid.bifactor_gather(start["a"].contiguous(), cs["general"], sd, has)
    free2 = grid.bifactor_gather(eng.unconstrained("a", eng.free).contiguous(), cs["general"], sd, has)
    b = start["b"].reshape(-1).contiguous().clone()
    theta2 = torch.stack([t["theta"][:, None].expand(Gg, Gh), t["u"][None, :].expand(Gg, Gh)], 2).reshape(Gg * Gh, 2).contiguous()
    cfg2 = eng.be.cfg(eng.model, 2, J, 0, eng.Dc, 1.0, 0, 0, 0)
    n1, n0 = t["n1"].reshape(J, -1).contiguous(), t["n0"].reshape(J, -1).contiguous()
    if prior is None:
        eng.be.grid_mstep_irt(cfg2, theta2, Gg * Gh, n1, n0, free2, a2, b, 4)
    else:
        c = start["c"].reshape(-1).contiguous().clone()
        pr = _t(grid.bifactor_em_prior(prior, cs["model"], cs["D"], J, cs["general"], sd_np, has_np))
        eng.be.grid_mstep_irt_map(cfg2, theta2, Gg * Gh, n1, n0, free2, a2, b, c, None, pr, 4, torch.zeros(J, device=_dev()))
        assert torch.equal(eng.unconstrained("c").reshape(-1), c) and not torch.equal(c, start["c"].reshape(-1))
    torch.cuda.synchronize()
    a = eng.unconstrained("a")
    j = torch.arange(J, device=_dev())
    assert torch.equal(a[cs["general"]], a2[0]) and torch.equal(a[sd[has], j[has]], a2[1][has])
    assert torch.equal(eng.unconstrained("b").reshape(-1), b) and not torch.equal(b, start["b"].reshape(-1))
    assert not torch.equal(a[cs["general"]], start["a"][cs["general"]])
    # what is not free keeps its bits: the specific rows of the other testlets, and the whole row of the empty dimension, stay 0
    free = eng.unconstrained("a", eng.free) != 0
    assert torch.equal(a[~free], start["a"][~free]) and bool((a[~free] == 0).all())


# ---- 6. the EM end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [be.EM_2PL[0], be.EM_3PL[0]])
def test_em_end_to_end(name):
    """25 iterations end where the float64 EM oracle's 25 end: every leaf entry within EM_MARGIN (2) times the CPU distance between
    that oracle and the EM on the float32 restatement -- 9.7e-7 (em_2pl), 7.4e-7 (em_3pl); see the module's header."""
    cs, eng = _em_engine(name)
    prior, kw = be.EM_PRIOR[name], dict(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
    s = eng.score_bifactor(**kw)["loglik"]
    total = torch.zeros(1, dtype=torch.float32, device=_dev())
    eng.be.sum_into(s, cs["N"], 1.0, total, torch.empty(1024, dtype=torch.float32, device=_dev()))
    t0, state = eng.t, {"P": eng.P.clone(), "M": eng.M.clone(), "V": eng.V.clone(), "G": eng.G.clone()}
    if eng.per_person:
        state.update({"PP": eng.PP.clone(), "MP": eng.MP.clone(), "VP": eng.VP.clone()})
    out = eng.fit_em_bifactor(max_iter=be.EM_ITERS, tol=-1.0, prior=prior, **kw)
    torch.cuda.synchronize()
    assert sorted(out) == (["converged", "iterations", "loglik"] + (["logpost"] if prior else [])) and out["iterations"] == be.EM_ITERS
    assert out["loglik"][0] == float(total[0])                          # bit for bit the summed score_bifactor loglik
    hist = out["logpost"] if prior else out["loglik"]
    for k in range(be.EM_ITERS - 1):
        assert hist[k + 1] >= hist[k] - 1e-6 * abs(hist[k]), (name, k, hist)
    ps, lks, lps = be.em(name)
    tol = be.EM_MARGIN * be.em_distance(name)
    errs = {k: float(np.abs(_np(eng.unconstrained(k)).astype(np.float64).reshape(ps[-1][k].shape) - ps[-1][k]).max()) for k in ps[-1]}
    errl = max(abs(g - w) / abs(w) for g, w in zip(hist, lps))
    print("%s: %.4f -> %.4f; leaves against the float64 EM %s (tol %.2e); history %.2e" % (name, hist[0], hist[-1], errs, tol, errl))
    assert errl <= cn.ROW_TOL
    for k, e in errs.items():
        assert e <= tol, (name, k, e, tol)
    # the guide, Adam's state and the step count are left alone
    assert eng.t == t0 and not torch.equal(eng.P, state["P"])
    for k in state:
        if k != "P":
            assert torch.equal(getattr(eng, k), state[k]), k


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_the_limits_are_value_errors_and_the_other_classes_refuse():
    from tests import score_cases as sc
    from vipsy_amd.engine import CcdmEngine, IrtEngine
    eng, _ = _got("s2_2pl")
    for kw in (dict(nodes=(1, 5)), dict(nodes=(257, 5)), dict(nodes=(21, 0)), dict(nodes=(21, 33)), dict(nodes=21),
               dict(span=(6.0, -1.0)), dict(general=4), dict(general=-1)):
        with pytest.raises(ValueError):
            eng.expected_counts_bifactor(**kw)
        with pytest.raises(ValueError):
            eng.fit_em_bifactor(**kw)
    with pytest.raises(ValueError, match=r"\(41, 21\)"):
        eng.fit_em_bifactor(nodes=(61, 21))
    y = torch.from_numpy(bc.case_of(bc.by_name("s2_2pl"))["y"]).to(_dev())
    one = IrtEngine(y, model="irt_1pl", D=1, seed=3)
    cdm = CcdmEngine(y, sc.cdm_q(3, int(y.shape[1]), np.random.RandomState(1)), cdm="dina")
    for e in (one, cdm):
        for call in (e.expected_counts_bifactor, e.fit_em_bifactor):
            with pytest.raises(NotImplementedError):
                call()
    three = IrtEngine(y, model="irt_2pl", D=3, seed=3)                 # the triangular default mask of x_feature = 3
    with pytest.raises(ValueError, match="item 0 is free on the specific dimensions"):
        three.fit_em_bifactor()
