"""The structured designs of the grid family (tests/grid_design_cases.py), the parts that need no GPU: every promise of a design's
`facts` on the matrix itself, and the conditions under which the rules of tests/test_gpu_grid_designs.py are sound -- checked on
the float64 oracles and on the numpy restatements the calls already have, never on what a kernel returned.

  - the node / draw rule leaves out at most ARGMAX_LEFT_OUT of the persons with at least one answer, and irt_condition holds;
  - fit_cases.lz_condition leaves out at most LEFT_OUT_CAP of the persons with at least COND_MIN_ITEMS answers;
  - each call's restatement (count_cases, se_cases, ld_cases, fit_cases, point_cases.restated_f32, dif_cases.restated) stays within
    that call's own rule on every design the call is run on: no design needs a constant of its own for the method's sake;
  - the discrete decisions the GPU test asserts exactly (who ends at the bound under ml, which booklet has no complete person,
    where S-X2's collapse is decided, where q3 is NaN) are clear-cut in the oracle.
The figures are printed per case; docs/NOTEBOOK.md has them beside what the GPU gave."""
import numpy as np
import pytest

from tests import count_cases as cc
from tests import dif_cases as dc
from tests import em_cases as ec
from tests import fit_cases as fc
from tests import grid_design_cases as gd
from tests import ld_cases as ld
from tests import point_cases as pc
from tests import pop_cases as pop
from tests import response_designs as rd
from tests import score_cases as sc
from tests import se_cases as se
from tests import sx2_cases as xc
from tests.test_gpu_response_designs import ROW_TOL, _row_errors

IRT_MAIN = [n for n in gd.MAIN if n in gd.IRT]
INFO = [n for n in gd.MAIN if gd.has_info(n)]


@pytest.mark.parametrize("name", gd.ALL)
def test_every_promise_of_the_facts_holds(name):
    cs = gd.case(name)
    d = gd.check_facts(name)
    f = cs["facts"]
    print("%s: %d x %d, %.1f %% missing, %d .. %d answered, %d empty persons, %d unanswered items"
          % (name, cs["N"], cs["J"], 100 * d["missing"], d["min_obs"], d["max_obs"], len(d["empty_persons"]), len(d["unanswered_items"])))
    if name == gd.SORTED:
        assert len(d["empty_persons"]) == 65 and len(d["unanswered_items"]) == 11 and f["empty_block"] == 128
        assert f["starts"] == [0, 5, 20] and f["lens"] == [5, 15, 40] and (np.diff(f["booklet_of"]) >= 0).all()
        assert gd.cross_pairs(name).sum() == 2 * (5 * 15 + 5 * 40 + 15 * 40)
        # the block lies inside booklet 1; the unit before it (booklets 0 and 1) and the unit after it (booklets 1 and 2) answer
        assert (f["booklet_of"][128:192] == 1).all() and len(np.unique(f["booklet_of"][64:128])) == 2
        assert len(np.unique(f["booklet_of"][192:256])) == 2
        assert (d["obs_per_person"][64:128] > 0).sum() >= 63 and (d["obs_per_person"][192:256] > 0).sum() >= 63
    if name == "gd_shuffled_j130_3pl":
        assert cs["N"] == 4 * 64 + 1
        for u in range(4):                                              # every unit mixes the three lengths
            assert len(np.unique(f["booklet_of"][64 * u:64 * u + 64])) == 3
    if name == "gd_short_j40_d2":
        assert d["min_obs"] == 0 and (d["obs_per_person"] == 3).sum() >= 32 and f["empty_block"] == 64
    if name == "gd_complete_j30":
        assert d["n_missing"] == 0 and len(d["all_one_items"]) == 1 and len(d["all_zero_items"]) == 1
    if name in gd.CDM:
        K = cs["K"]
        assert (cs["y"][d["obs_per_person"] > 0][:, :K] != rd.MISSING).all()      # every attribute's own item is answered
        assert f["empty_block"] == 128 and len(d["empty_persons"]) == 64 and cs["J"] - 1 in d["unanswered_items"]
        assert cs["q"][:, cs["J"] - 1].sum() >= 2
        assert set(d["obs_per_person"][d["obs_per_person"] > 0].tolist()) <= set(f["lens"]) | {v - 1 for v in f["lens"]}
    if name == "gd_dina_k6":
        assert (1 << cs["K"]) == 64                                      # two node tiles of 32


@pytest.mark.parametrize("name", gd.ALL)
def test_the_node_rule_and_the_quadrature_condition(name):
    cs, o = gd.case(name), gd.oracle(name)
    persons, draws = gd.left_out(name)
    print("%s: left out of the node rule %.2f %% of the answering persons, %.3f %% of their draws (cap %.0f %%)"
          % (name, 100 * persons, 100 * draws, 100 * sc.ARGMAX_LEFT_OUT))
    assert persons <= sc.ARGMAX_LEFT_OUT and draws <= sc.ARGMAX_LEFT_OUT
    empty = ~o["answered"]
    if empty.any():
        # an empty person's posterior is the prior: ll = J x the missing constant at every node, no tie among the best nodes
        assert np.allclose(o["f"][empty] - o["f"][empty][:, :1], (o["f"][empty][:1] - o["f"][empty][:1, :1]))
        assert np.abs(o["post"]["loglik"][empty] - cs["J"] * gd.missing_constant()).max() <= 1e-7       # (the float32 log-weights sum to 1 within 1e-8)
        if name in gd.IRT:
            assert (o["post"]["gap"][empty] > sc.ARGMAX_GAP).all() and (o["post"]["node"][empty] == (o["f"].shape[1] - 1) // 2).all()
            assert np.abs(o["post"]["mean"][empty]).max() <= 1e-9
        else:
            assert np.abs(o["post"]["mean"][empty] - 0.5).max() <= 1e-9 and (o["post"]["gap"][empty] == 0).all()
    if name in gd.IRT:
        lo, need = sc.irt_condition(cs, o["post"])
        print("    smallest oracle PSD %.2f against half the node spacing %.2f" % (lo, need))
        assert lo >= need
    # the tables: a row of an unanswered item is exactly zero in the oracle, and its statistics are NaN
    un = cs["facts"]["unanswered_items"]
    c = o["counts"]
    assert (c["n1"][un] == 0).all() and (c["n0"][un] == 0).all() and np.isnan(c["md"][un]).all() and (c["n_obs"][un] == 0).all()


@pytest.mark.parametrize("name", list(gd.POP))
def test_the_conditioned_oracle(name):
    cs, p = gd.case(name), gd.population(name)
    want = p["want"]
    lo, need = sc.irt_condition(cs, want)
    out = float((want["gap"] <= sc.ARGMAX_GAP).mean())
    dr = float((p["draws"][1] <= pop.DRAW_GAP).mean())
    print("%s under N(Gamma^T x, Sigma): PSD %.2f (need %.2f), %.2f %% of the persons and %.3f %% of the draws left out" % (name, lo, need, 100 * out, 100 * dr))
    assert lo >= need and out <= sc.ARGMAX_LEFT_OUT and dr <= sc.ARGMAX_LEFT_OUT
    empty = ~gd.oracle(name)["answered"]
    # an empty person returns the prior as the grid has it: near Gamma^T x and Sigma, up to what the grid's spacing and span cost
    assert np.abs(want["mean"][empty] - want["prior_mean"][empty]).max() < 0.05
    assert np.abs(want["cov"][empty] - p["sigma"][None]).max() < 0.05


@pytest.mark.parametrize("name", gd.MAIN)
def test_counts_restated(name):
    cs, o = gd.case(name), gd.oracle(name)["counts"]
    _, logw, ll = gd.grid_ll(name)
    r = cc.restated_f32(ll, logw, cs["y"])
    errs = {k: _row_errors(r[k].astype(np.float64), o[k], 1.0)[0] for k in ("n1", "n0")}
    errs["mass"] = _row_errors(r["mass"].astype(np.float64)[None], o["mass"][None], 1.0)[0]
    rs = cc.fit_stats(r["n1"].astype(np.float64), r["n0"].astype(np.float64), o["prob"])
    for k in ("md", "rmsd"):
        assert np.array_equal(np.isnan(rs[k]), np.isnan(o[k]))
        errs[k] = float(np.nanmax(np.abs(rs[k] - o[k])))
    print("%s counts restated: %s (rule %.1e)" % (name, "  ".join("%s %.2e" % kv for kv in errs.items()), ROW_TOL))
    assert max(errs.values()) <= ROW_TOL / 3
    un = cs["facts"]["unanswered_items"]
    assert (r["n1"][un] == 0).all() and (r["n0"][un] == 0).all()


@pytest.mark.parametrize("name", INFO)
def test_information_restated_and_what_item_se_can_be_asked(name):
    cs, o = gd.case(name), gd.info_oracle(name)
    r = se.restated_f32(cs, gd.kind_of(name), cs["params"])
    top = float(np.abs(np.diag(o["info"])).max())
    e_i = _row_errors(r["info"].astype(np.float64), o["info"], top)[0]
    e_g = _row_errors(r["gradient"].astype(np.float64)[None], o["gradient"][None], np.sqrt(top * o["n"]))[0]
    print("%s info restated: info %.2e gradient %.2e (rule %.1e); P %d, kept %d, condition %s"
          % (name, e_i, e_g, ROW_TOL, len(o["free"]), len(o["kept"]), "%.1f" % o["condition"] if "condition" in o else "not positive definite"))
    assert e_i <= ROW_TOL / 3 and e_g <= ROW_TOL / 3
    K = o["K"]
    dead = np.flatnonzero(np.diag(o["info"]) == 0)
    un = cs["facts"]["unanswered_items"]
    assert set(np.repeat(un * K, K) + np.tile(np.arange(K), len(un))) <= set(dead.tolist())
    assert (o["info"][dead] == 0).all() and (o["gradient"][dead] == 0).all() and not set(dead.tolist()) & set(o["kept"].tolist())
    if name == gd.SORTED:
        m = np.repeat(np.repeat(gd.cross_pairs(name), K, 0), K, 1)
        assert (o["info"][m] == 0).all() and (r["info"][m] == 0).all()


@pytest.mark.parametrize("name", INFO)
def test_one_oracle_em_iteration_leaves_unanswered_items_alone(name):
    cs, kind = gd.case(name), gd.kind_of(name)
    p0 = {k: v.astype(np.float64) for k, v in cs["params"].items()}
    p1, lk = ec.em_iteration(cs, kind, p0)
    un = cs["facts"]["unanswered_items"]
    for k in p1:
        assert np.array_equal(np.asarray(p1[k]).reshape(p0[k].shape)[:, un], p0[k][:, un]), k
        assert np.isfinite(p1[k]).all(), k
    assert np.isfinite(lk)


@pytest.mark.parametrize("name", gd.MAIN)
def test_pairs_restated(name):
    kind, k = gd.key(name)
    o = gd.oracle(name)["pairs"]
    assert np.array_equal(ld.oracle(kind, k)["n"], o["n"]) and np.array_equal(ld.oracle(kind, k)["sp"], o["sp"])
    r = ld.restated_f32(kind, k)
    e = {t: ld.row_error(r[t], o[t]) for t in ("s", "ss", "sp")}
    keep = o["keep"]
    q = float(np.abs(r["q3"][keep] - o["q3"][keep]).max()) if keep.any() else 0.0
    off = ~np.eye(len(keep), dtype=bool)
    print("%s pairs restated: s %.2e ss %.2e sp %.2e, q3 %.2e on %.1f %% of the off-diagonal pairs (rule %.1e)"
          % (name, e["s"], e["ss"], e["sp"], q, 100 * keep[off].mean(), ROW_TOL))
    assert np.array_equal(r["n"], o["n"]) and max(e.values()) <= ROW_TOL / 3 and q <= ROW_TOL / 3
    assert np.array_equal(np.isnan(r["q3"]), np.isnan(o["q3"]))          # where q3 is NaN is clear-cut
    # wherever q3 is defined (n >= 8) the variances are far from the sign change that decides it
    ok = o["n"] >= ld.COND_MIN_PAIRS
    assert (np.minimum(o["v"], o["v"].T)[ok] > 1e-3).all()
    un = gd.case(name)["facts"]["unanswered_items"]
    for t in ("n", "s", "ss", "sp"):
        assert (o[t][un] == 0).all() and (o[t][:, un] == 0).all() and (r[t][un] == 0).all() and (r[t][:, un] == 0).all()
    assert np.isnan(o["q3"][un]).all() and np.isnan(o["q3"][:, un]).all()
    if name == gd.SORTED:
        m = gd.cross_pairs(name)
        assert all((o[t][m] == 0).all() and (r[t][m] == 0).all() for t in ("n", "s", "ss", "sp")) and np.isnan(o["q3"][m]).all()


@pytest.mark.parametrize("name", gd.MAIN)
def test_person_fit_restated_and_the_lz_cap(name):
    kind, k = gd.key(name)
    o = gd.oracle(name)["fit"]
    assert np.array_equal(fc.oracle(kind, k)["person"]["l0"], o["person"]["l0"])
    r = fc.restated_f32(kind, k)
    rp = fc.sum_ratios(r["person"], o["person"], o["person_abs"], fc.PERSON)
    ri = fc.sum_ratios(r["item"], o["item"], o["item_abs"], fc.ITEM)
    rl = fc.lz_ratio(r["lz"], o)
    out = gd.lz_left_out(name)
    few = int((o["person"]["n"] < fc.COND_MIN_ITEMS).sum())
    print("%s fit restated: person %s | item %s | lz %.2f (C = %g); %.1f %% of the persons with >= %d answers left out of lz, %d persons below"
          % (name, " ".join("%s %.2f" % kv for kv in rp.items()), " ".join("%s %.2f" % kv for kv in ri.items()), rl, fc.FIT_C,
             100 * out, fc.COND_MIN_ITEMS, few))
    assert max(list(rp.values()) + list(ri.values()) + [rl]) <= fc.FIT_C
    assert out <= fc.LEFT_OUT_CAP
    assert np.array_equal(np.isnan(o["lz"]), ~gd.oracle(name)["answered"])


@pytest.mark.parametrize("name", IRT_MAIN)
def test_point_estimates_restated_and_who_ends_at_the_bound(name):
    cs = gd.case(name)
    eap = gd.oracle(name)["post"]["mean"]
    f = cs["facts"]
    many = (cs["y"] < 2).sum(1) >= pc.MIN_ITEMS
    for method in pc.METHODS:
        if method == "wle" and cs["D"] > 1:
            continue
        root = pc.fisher64(cs, method, eap)
        got = pc.restated_f32(cs, method, eap.astype(np.float32))
        r = pc.ratios(cs, method, got, root=root, tag=name)
        counts = {pc.STATUS[k]: int((got["status"] == k).sum()) for k in range(5)}
        # (point_cases.MAX_ITER_CAP is a condition on ITS cases and is not asked here: the capped step has no halving, and a 10-item
        # person of the 3PL design can alternate between two points under wle, in float64 and float32 alike -- printed, not bounded;
        # such a person is held by the info rule and by the bits of a second call)
        f64 = pc.fisher64(cs, method, eap, max_iter=pc.MAX_ITER, tol=pc.TOL)
        print("%s %s restated: s %.2f root %.2f info %.2f (C = %g); %s; max_iter among the persons with >= %d answers: %.1f %% (float64 "
              "method: %.1f %%)" % (name, method, r["s"], r["root"], r["info"], pc.POINT_C, counts, pc.MIN_ITEMS,
                                    100 * (got["status"][many] == pc.MAX_ITERS).mean(), 100 * (f64["status"][many] == pc.MAX_ITERS).mean()))
        assert max(r.values()) <= pc.POINT_C
        assert (got["status"] != pc.SINGULAR).all() or cs["model"] != "irt_2pl"
        if "all_one_person" in f:
            pair = [f["all_one_person"], f["all_zero_person"]]
            if method == "ml":
                assert (root["status"][pair] == pc.AT_BOUND).all() and (got["status"][pair] == pc.AT_BOUND).all()
                assert np.array_equal(got["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND)
                assert (np.abs(root["theta_hat"][pair]).max(1) == cs["span"]).all()
            else:
                assert np.isfinite(root["theta_hat"][pair]).all() and np.isfinite(got["theta_hat"][pair]).all()
                if method == "map":
                    assert (root["status"][pair] == pc.CONVERGED).all() and (np.abs(root["theta_hat"][pair]) < cs["span"]).all()


def test_groups_are_booklets_restated():
    o = gd.group_oracle()
    print("groups = booklets: restatement %.2e, rule %.2e" % (o["restated_error"], o["rule"]))
    assert dc.C_RULE * max(o["restated_error"], dc.RULE_FLOOR) == o["rule"] and o["restated_error"] <= ROW_TOL / 3
    cs = gd.case(gd.SORTED)
    for h in range(3):
        outside = np.delete(np.arange(cs["J"]), gd.booklet_items(gd.SORTED, h))
        assert (o["n1"][h][outside] == 0).all() and (o["n0"][h][outside] == 0).all() and (o["n_obs"][h][outside] == 0).all()
        assert np.isnan(o["rmsd"][h][outside]).all()
    assert np.array_equal(o["n_obs"], np.stack([(cs["y"][o["groups"] == h] != 255).sum(0) for h in range(3)]))
    whole = gd.oracle(gd.SORTED)["counts"]
    assert np.abs(o["n1"].sum(0) - whole["n1"]).max() <= 1e-9 and np.abs(o["mass"].sum(0) - whole["mass"]).max() <= 1e-9


def test_sx2_by_booklet_in_the_oracle():
    cs = gd.case(gd.SORTED)
    y, f = cs["y"], cs["facts"]
    assert (xc.persons_oracle(y, None, None) < 0).all()                  # nobody is complete: the default call must raise
    raised = []
    for k in range(3):
        items = gd.booklet_items(gd.SORTED, k)
        score = xc.persons_oracle(y, None, items)
        assert (score[f["booklet_of"] != k] == -1).all() and (score[f["empty_persons"]] == -1).all()
        if f["unanswered_item"] in items:
            assert (score < 0).all()
            raised.append(k)
            continue
        p1, p0, _, logw = xc.irt_probs(cs, items)
        lw, o1, n, _ = xc.host_tables(y, items, p1, p0, logw)
        want = xc.sx2_oracle(lw["e1"], lw["e0"], o1, n, np.full(len(items), 2), 1.0, rho=xc.SX2_C * (len(items) + len(logw)) * 2.0 ** -24)
        print("booklet %d: %d complete persons, smallest collapse margin %.2e, S-X2 %s" % (k, int((score >= 0).sum()), want["margin"].min(),
                                                                                         np.round(want["sx2"], 2)))
        assert (want["margin"] > xc.COLLAPSE_MARGIN).all() and (score >= 0).sum() > 30
    assert len(raised) == 1
