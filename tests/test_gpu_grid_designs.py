"""The grid family on the GPU on structured response designs (tests/grid_design_cases.py): score(), plausible_values(),
expected_counts() / item_fit(), item_information() / item_se(), fit_em(), the conditioned score() / plausible_values(),
residual_sums() / local_dependence(), fit_sums() / person_fit() / item_msq(), group_counts() / dif(), sumscore_tables() / sx2() and
point_estimates() of IrtEngine and CcdmEngine against the float64 oracle each call already has in its own *_cases.py.

Engines are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views, nothing trained.  No rule
and no constant is new: the row rule ROW_TOL for score, counts, info and the conditioned posterior, fit_cases.FIT_C,
point_cases.POINT_C, dif_cases.C_RULE, the Q3 and the S-X2 rules, the node / draw rule with ARGMAX_GAP -- whose cap is taken over
the persons with at least one answer, as the lz cap is taken over the persons with at least COND_MIN_ITEMS answers
(tests/test_grid_designs_host.py asserts both caps, and every restatement, on the CPU).  The errors found are printed beside
their rule; docs/NOTEBOOK.md has the table.

What is asserted EXACTLY is the reason for this file: an empty person -- every one of a whole unit of 64 -- returns the prior,
the centre node, exact zero sums and NaN statistics, and leaks nothing into the units beside it; an item nobody answered and a
pair of items no person shares have exact zeros in every table, in info and in the gradient, NaN where the host layers divide, and
parameters fit_em leaves bit-equal; a group holds exact zeros outside its booklet; rows= of one booklet gives the bits of the same
persons passed as data; a matrix without an observed cell, or with one, returns what the host layers document for empty tables."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

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
from tests.test_gpu_counts import _hold as _hold_counts
from tests.test_gpu_dif import _hold as _hold_group_tables
from tests.test_gpu_dif import _hold_dif
from tests.test_gpu_fit import _hold as _hold_fit
from tests.test_gpu_ld import TABLES, _hold_q3, _hold_tables
from tests.test_gpu_parity import _dev
from tests.test_gpu_pop import _hold_nodes, _hold_rows
from tests.test_gpu_pv import _hold_draws
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np
from tests.test_gpu_se import _hold_info
from tests.test_gpu_sx2 import _device_probs, _hold_probs, _hold_sx2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
IRT_MAIN = [n for n in gd.MAIN if n in gd.IRT]
INFO = [n for n in gd.MAIN if gd.has_info(n)]
POINT_KW = {"max_iter": pc.MAX_ITER, "tol": pc.TOL}


def _engine(name):
    cs = gd.case(name)
    return cs, (_ccdm_engine(cs) if name in gd.CDM else _irt_engine(cs)), gd.grid_kw(name)


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _dev_rows(idx):
    return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(_dev())


def _same_bits(tag, a, b, keys):
    for k in keys:
        ta, tb = a[k], b[k]
        if torch.is_tensor(ta):
            assert torch.equal(ta, tb) or (ta.is_floating_point() and np.array_equal(_np(ta), _np(tb), equal_nan=True)), (tag, k)
        else:
            assert np.array_equal(np.asarray(ta), np.asarray(tb), equal_nan=np.asarray(ta).dtype.kind == "f"), (tag, k)


def _finite(tag, out, keys):
    for k in keys:
        assert bool(torch.isfinite(out[k]).all()), (tag, k, "a device output is not finite")


# ---- score, counts, draws ------------------------------------------------------------------------------------------------
def _hold_post(name, got, o, cs):
    """The row rule on loglik and the moments (all persons); the node rule over the persons with at least one answer; an empty
    person's prior exactly."""
    kind, want, a = gd.kind_of(name), o["post"], o["answered"]
    N, (G, D) = cs["N"], o["coord"].shape
    mean_k, node_k = ("eap", "node") if kind == "irt" else ("attr_prob", "pattern")
    names = [("loglik", "loglik"), (mean_k, "mean")] + ([("psd", "sd")] if kind == "irt" else [])
    assert tuple(got[mean_k].shape) == (N, D) and tuple(got["loglik"].shape) == (N,) and got[node_k].dtype == torch.int32
    _finite(name, got, [g for g, _ in names])
    errs = {g: _row_errors(_f8(got[g]), np.asarray(want[w], np.float64), floor=1.0) for g, w in names}
    node = _np(got[node_k]).astype(np.int64)
    assert node.min() >= 0 and node.max() < G
    sure = a & (want["gap"] > sc.ARGMAX_GAP)
    out = 1.0 - float(sure[a].mean()) if a.any() else 0.0
    wrong = np.flatnonzero(sure & (node != want["node"]))
    print("%s score: %s; %.1f %% of the answering persons left out of the node rule, %d wrong nodes (row rule %.1e)"
          % (name, "  ".join("%s %.2e (row %d)" % (k, v[0], v[1]) for k, v in errs.items()), 100 * out, len(wrong), ROW_TOL))
    for k, (e, worst) in errs.items():
        assert e <= ROW_TOL, (name, k, "person", worst, e)
    assert out <= sc.ARGMAX_LEFT_OUT and len(wrong) == 0, (name, out, wrong[:10])
    empty = np.flatnonzero(~a)
    if len(empty):
        ll = _f8(got["loglik"])[empty]
        assert np.abs(ll - cs["J"] * gd.missing_constant()).max() <= ROW_TOL, name          # J cells of the missing constant
        if kind == "irt":
            prior_sd = want["sd"][empty[0]]
            assert np.abs(_f8(got["eap"])[empty]).max() <= ROW_TOL and np.abs(_f8(got["psd"])[empty] - prior_sd).max() <= ROW_TOL, name
            assert (node[empty] == (G - 1) // 2).all(), (name, "an empty person's node is not the centre node")
        else:
            assert np.abs(_f8(got["attr_prob"])[empty] - 0.5).max() <= ROW_TOL, name       # (all patterns tie: range-checked above)
        # every empty person has the bits of the first: nothing of a neighbour's reaches them
        for g, _ in names:
            assert (got[g][_dev_rows(empty)] == got[g][int(empty[0])]).all(), (name, g)


def _hold_pvs(name, got, o, cs):
    kind = gd.kind_of(name)
    coord_k, node_k = ("theta", "node") if kind == "irt" else ("attr", "pattern")
    G, D = o["coord"].shape
    node, val = _np(got[node_k]), _np(got[coord_k])
    assert node.dtype == np.int32 and node.shape == (cs["N"], gd.DRAWS) and val.shape == (cs["N"], gd.DRAWS, D)
    assert node.min() >= 0 and node.max() < G
    want_node, gap = o["draws"]
    _hold_draws(name, node, want_node, gap)
    assert np.array_equal(val, o["coord"].astype(np.float32)[node])              # the grid's own coordinates, bit for bit
    empty = ~o["answered"]
    if empty.any():                                                            # the prior's draws: the oracle's Gumbel draw
        sure = gap[empty] > sc.ARGMAX_GAP
        assert sure.mean() >= 1 - sc.ARGMAX_LEFT_OUT and np.array_equal(node[empty][sure], want_node[empty][sure]), name


@pytest.mark.parametrize("name", gd.MAIN)
def test_score_counts_and_draws(name):
    cs, eng, kw = _engine(name)
    o, f, y = gd.oracle(name), cs["facts"], cs["y"]
    got = eng.score(**kw)
    torch.cuda.synchronize()
    _hold_post(name, got, o, cs)
    if "empty_block" in f:
        # the unit before and the unit after the block are held to the oracle like everyone else: nothing leaks across units
        b = f["empty_block"]
        for tag, rows in (("before", np.arange(b - 64, b)), ("after", np.arange(b + 64, min(b + 128, cs["N"])))):
            for g, w in (("loglik", "loglik"), ("eap" if name in gd.IRT else "attr_prob", "mean")):
                e = _row_errors(_f8(got[g])[rows], np.asarray(o["post"][w], np.float64)[rows], floor=1.0)[0]
                assert e <= ROW_TOL, (name, "the unit %s the empty block" % tag, g, e)
    _same_bits(name, got, eng.score(**kw), list(got))
    cnt, fit = eng.expected_counts(**kw), eng.item_fit(**kw)
    torch.cuda.synchronize()
    _finite(name, cnt, ("n1", "n0", "mass", "prob"))
    _hold_counts(name, cnt, fit, o["counts"], y)
    un = f["unanswered_items"]
    assert (_np(cnt["n1"])[un] == 0).all() and (_np(cnt["n0"])[un] == 0).all(), name
    assert np.isnan(_np(fit["md"])[un]).all() and np.isnan(_np(fit["rmsd"])[un]).all() and (_np(fit["n_obs"])[un] == 0).all(), name
    assert np.isnan(_np(fit["observed"])[un]).all(), name
    # a cell nobody could fill is exactly zero: the all-one item has no n0, the all-zero item no n1
    assert (_np(cnt["n1"])[(y == 1).sum(0) == 0] == 0).all() and (_np(cnt["n0"])[(y == 0).sum(0) == 0] == 0).all(), name
    _same_bits(name, cnt, eng.expected_counts(**kw), ("n1", "n0", "mass", "prob"))
    pvs = eng.plausible_values(draws=gd.DRAWS, seed=gd.SEED, **kw)
    torch.cuda.synchronize()
    _hold_pvs(name, pvs, o, cs)
    _same_bits(name, pvs, eng.plausible_values(draws=gd.DRAWS, seed=gd.SEED, **kw), list(pvs))


# ---- information, standard errors, one EM iteration ----------------------------------------------------------------------
@pytest.mark.parametrize("name", INFO)
def test_information_and_item_se(name):
    cs, eng, kw = _engine(name)
    o, f = gd.info_oracle(name), cs["facts"]
    got = eng.item_information(**kw)
    torch.cuda.synchronize()
    _finite(name, got, ("info", "gradient"))
    _hold_info(name, got, o)                                                    # (symmetric bit for bit; dead parameters exact zeros)
    K = o["K"]
    gi, gg = _np(got["info"]), _np(got["gradient"])
    cols = (np.repeat(f["unanswered_items"] * K, K) + np.tile(np.arange(K), len(f["unanswered_items"]))).astype(np.int64)
    assert (gi[cols] == 0).all() and (gi[:, cols] == 0).all() and (gg[cols] == 0).all(), name
    if name == gd.SORTED:
        m = np.repeat(np.repeat(gd.cross_pairs(name), K, 0), K, 1)
        assert (gi[m] == 0).all(), "the info block between two items no person shares is not exactly zero"
    _same_bits(name, got, eng.item_information(**kw), ("info", "gradient"))
    # what item_se keeps: the oracle's kept columns exactly -- the unanswered items are dropped
    kept = se.kept_of(gi.astype(np.float64), _np(got["free"]))
    assert np.array_equal(kept, o["kept"]) and not set(cols.tolist()) & set(kept.tolist()), name
    fair = "condition" in o and ROW_TOL * o["condition"] <= 0.1
    print("%s: kept %d of %d; the oracle's kept block: %s" % (name, len(kept), len(o["free"]), "condition %.1f" % o["condition"]
                                                            if "condition" in o else "not positive definite"))
    try:
        out = eng.item_se(**kw)
    except ValueError as e:
        # drawn parameters on a design whose kept block is singular or nearly so: no pseudo-inverse, as documented
        assert not fair and "pivot" in str(e), (name, str(e))
        return
    assert np.array_equal(out["kept"], o["kept"])
    dense = np.full(len(o["free"]), 0.0)
    dense[np.setdiff1d(np.arange(len(o["free"])), o["kept"])] = np.nan
    for k, w in eng._se_leaves(dense).items():
        assert np.array_equal(np.isnan(out[k]), np.isnan(w)), (name, k, "se is NaN exactly off the kept columns")
    if fair:
        worst = max(float(np.nanmax(np.abs(out[k] / w - 1))) for k, w in eng._se_leaves(o["se"].copy()).items())
        print("%s: se %.2e relative (bound %.1e x condition = %.2e)" % (name, worst, ROW_TOL, ROW_TOL * o["condition"]))
        assert worst <= ROW_TOL * o["condition"]


@pytest.mark.parametrize("name", INFO)
def test_one_em_iteration(name):
    """fit_em(max_iter=1) from the drawn parameters against em_cases.em_iteration: ROW_TOL on the parameters (the CDM's on the
    probability scale) and on the log-likelihood, as tests/test_gpu_em.py holds them; the constant items, whose likelihood has
    no maximum, are held finite, as its constant-item test holds them; an unanswered item keeps its bits."""
    from oracle import vi_oracle as vo
    cs, eng, kw = _engine(name)
    kind, f = gd.kind_of(name), cs["facts"]
    start = {k: _np(eng.unconstrained(k)).copy() for k in cs["params"]}
    want, lk = ec.em_iteration(cs, kind, {k: v.astype(np.float64) for k, v in cs["params"].items()})
    out = eng.fit_em(max_iter=1, tol=0, **kw)
    torch.cuda.synchronize()
    skip = [f[k] for k in ("all_one_item", "all_zero_item") if k in f]
    errs = {"loglik": abs(out["loglik"][0] - lk) / abs(lk)}
    for k, w in want.items():
        g = _np(eng.unconstrained(k))
        assert np.isfinite(g).all(), (name, k)
        un = f["unanswered_items"]
        assert np.array_equal(g[:, un].view(np.uint32), start[k][:, un].view(np.uint32)), (name, k, "an unanswered item moved")
        g8, w8 = g.astype(np.float64), np.asarray(w, np.float64).reshape(g.shape)
        if kind == "cdm":
            g8, w8 = vo.sigmoid(g8), vo.sigmoid(w8)
        errs[k] = float(np.delete(np.abs(g8 - w8), skip, axis=1).max())
    print("%s after one EM iteration: %s (rule %.1e)" % (name, "  ".join("%s %.2e" % kv for kv in sorted(errs.items())), ROW_TOL))
    assert max(errs.values()) <= ROW_TOL, (name, errs)


# ---- pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gd.MAIN)
def test_residual_sums_and_q3(name):
    cs, eng, kw = _engine(name)
    kind, f = gd.kind_of(name), cs["facts"]
    o = gd.oracle(name)["pairs"]
    t = eng.residual_sums(**kw)
    torch.cuda.synchronize()
    if kind == "cdm":
        a = gd.oracle(name)["answered"]
        pat = _np(t["pattern"]).astype(np.int64)
        clear = a & (gd.oracle(name)["post"]["gap"] > sc.ARGMAX_GAP)
        assert np.array_equal(pat[clear], gd.oracle(name)["est"][clear]) and pat.min() >= 0 and pat.max() < (1 << cs["K"])
        if not np.array_equal(pat[a], gd.oracle(name)["est"][a]):               # (an empty person's pattern reaches no table)
            o = ld.tables(cs["y"], ld.cdm_prob(cs, pat))
            o["q3"], o["v"] = ld.q3_of_tables(o)
            o["keep"] = ld.condition(o)
    _hold_tables(name, t, o)                                                    # n exactly; n and sp symmetric bit for bit
    un = f["unanswered_items"]
    for k in TABLES:
        g = _np(t[k])
        assert (g[un] == 0).all() and (g[:, un] == 0).all(), (name, k, "an unanswered item's row or column is not exactly zero")
        if name == gd.SORTED:
            assert (g[gd.cross_pairs(name)] == 0).all(), (name, k, "two items no person shares")
    out = eng.local_dependence(**kw)
    assert np.array_equal(np.isnan(out["q3"]), np.isnan(o["q3"])), (name, "q3 is NaN where the oracle's is, and nowhere else")
    assert np.array_equal(out["n_pairs"], o["n"].astype(np.int64)) and np.array_equal(out["q3"], out["q3"].T, equal_nan=True)
    _hold_q3(name, out["q3"], o)
    _same_bits(name, t, eng.residual_sums(**kw), list(t))


# ---- person fit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gd.MAIN)
def test_person_fit_and_item_msq(name):
    cs, eng, kw = _engine(name)
    kind, f = gd.kind_of(name), cs["facts"]
    t = eng.fit_sums(**kw)
    torch.cuda.synchronize()
    est = _np(t["pattern" if kind == "cdm" else "theta_hat"])
    o = fc.sums(cs["y"], fc.prob_at(kind, cs, est.astype(np.float64) if kind == "irt" else est))
    person = {k: _np(v).astype(np.float64) for k, v in t["person"].items()}
    item = {k: _np(v).astype(np.float64) for k, v in t["item"].items()}
    _hold_fit(name, person, item, o)                                            # all seven sums of EVERY person, lz under its condition
    out = gd.lz_left_out(name, o)
    assert out <= fc.LEFT_OUT_CAP, (name, "lz leaves out too many of the persons with >= %d answers" % fc.COND_MIN_ITEMS, out)
    empty, un = f["empty_persons"], f["unanswered_items"]
    assert all((person[k][empty] == 0).all() for k in fc.PERSON) and all((item[k][un] == 0).all() for k in fc.ITEM), name
    pf, im = eng.person_fit(**kw), eng.item_msq(**kw)
    gone = np.zeros(cs["N"], bool)
    gone[empty] = True
    for k in ("lz", "infit", "outfit"):
        assert np.array_equal(np.isnan(pf[k]), gone), (name, k)
    dead = np.zeros(cs["J"], bool)
    dead[un] = True
    for k in ("infit", "outfit"):
        assert np.array_equal(np.isnan(im[k]), dead), (name, k)
    assert np.array_equal(pf["n_obs"], (cs["y"] < 2).sum(1)) and np.array_equal(im["n_obs"], (cs["y"] < 2).sum(0))
    again = eng.fit_sums(**kw)
    _same_bits(name, t["person"], again["person"], fc.PERSON)
    _same_bits(name, t["item"], again["item"], fc.ITEM)


# ---- point estimates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IRT_MAIN)
def test_point_estimates(name):
    cs, eng, kw = _engine(name)
    f, y = cs["facts"], cs["y"]
    eap = gd.oracle(name)["post"]["mean"]
    answered = (y < 2).sum(1)
    assert (answered == 3).any() or name != "gd_short_j40_d2"                   # 3-item persons are present
    for method in pc.METHODS:
        if method == "wle" and cs["D"] > 1:
            continue
        got = eng.point_estimates(method=method, **POINT_KW, **kw)
        root = pc.fisher64(cs, method, eap)
        r = pc.ratios(cs, method, got, root=root, tag=name)
        counts = {pc.STATUS[k]: int((got["status"] == k).sum()) for k in range(5)}
        print("%s %s: s %.2f root %.2f info %.2f (C = %g); %s; iterations max %d" % (name, method, r["s"], r["root"], r["info"], pc.POINT_C,
                                                                                  counts, got["iterations"].max()))
        assert max(r.values()) <= pc.POINT_C, (name, method, r)
        assert np.array_equal(got["status"] == pc.EMPTY, answered == 0) and counts["empty"] == len(f["empty_persons"])
        if cs["model"] == "irt_2pl":
            assert counts["singular"] == 0
        if method == "ml":
            assert np.array_equal(got["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND), (name, "ml's at_bound persons are the oracle's")
        if "all_one_person" in f:
            i1, i0 = f["all_one_person"], f["all_zero_person"]
            if method == "ml":
                assert got["status"][i1] == pc.AT_BOUND and got["status"][i0] == pc.AT_BOUND
                assert got["theta_hat"][i1].max() == np.float32(cs["span"]) and got["theta_hat"][i0].min() == np.float32(-cs["span"])
            else:
                assert np.isfinite(got["theta_hat"][[i1, i0]]).all() and np.isfinite(got["se"][[i1, i0]]).all()
            if method == "map":
                assert (np.abs(got["theta_hat"][[i1, i0]]) < cs["span"]).all() and (got["status"][[i1, i0]] == pc.CONVERGED).all()
        _same_bits(name, got, eng.point_estimates(method=method, **POINT_KW, **kw), ("theta_hat", "info", "status", "iterations"))


# ---- groups = booklets ---------------------------------------------------------------------------------------------------
def test_groups_are_booklets():
    name = gd.SORTED
    cs, eng, kw = _engine(name)
    want = gd.group_oracle(name)
    rule, groups = want["rule"], want["groups"]
    gc = eng.group_counts(groups, impact=False, **kw)
    torch.cuda.synchronize()
    _finite(name, gc, ("n1", "n0", "mass", "prob"))
    assert tuple(gc["n1"].shape) == (3, cs["J"], 61) and np.array_equal(gc["labels"], [0, 1, 2])
    _hold_group_tables(name + " group_counts", gc, want, rule)
    n1, n0 = _np(gc["n1"]), _np(gc["n0"])
    whole = eng.expected_counts(**kw)
    for h in range(3):
        outside = np.delete(np.arange(cs["J"]), gd.booklet_items(name, h))
        assert (n1[h][outside] == 0).all() and (n0[h][outside] == 0).all(), "group %d has mass on an item outside its booklet" % h
        mine = eng.expected_counts(rows=_dev_rows(np.flatnonzero(groups == h)), **kw)
        for k in ("n1", "n0"):
            e = _row_errors(_f8(gc[k][h]), _f8(mine[k]), floor=1.0)[0]
            assert e <= rule, (h, k, e, rule)
        assert _row_errors(_f8(gc["mass"][h])[None], _f8(mine["mass"])[None], floor=1.0)[0] <= rule
    for k in ("n1", "n0"):
        e = _row_errors(_f8(gc[k]).sum(0), _f8(whole[k]), floor=1.0)[0]
        print("groups = booklets: sum over the groups against expected_counts(): %s %.2e (row rule %.1e)" % (k, e, ROW_TOL))
        assert e <= ROW_TOL
    assert _row_errors(_f8(gc["mass"]).sum(0)[None], _f8(whole["mass"])[None], floor=1.0)[0] <= ROW_TOL
    got = eng.dif(groups, impact=False, **kw)
    _hold_dif(name + " dif(impact=False)", got, want, rule)                     # n_obs the integer counts; NaN where the oracle has it
    for h in range(3):
        outside = np.delete(np.arange(cs["J"]), gd.booklet_items(name, h))
        assert (got["n_obs"][h][outside] == 0).all() and np.isnan(got["rmsd"][h][outside]).all() and np.isnan(got["md"][h][outside]).all()
    _same_bits(name, gc, eng.group_counts(groups, impact=False, **kw), ("n1", "n0", "mass", "prob"))


# ---- rows= one booklet ---------------------------------------------------------------------------------------------------
def test_rows_of_one_booklet_are_the_same_persons_as_data():
    """The 5-item booklet of gd_sorted_j70: every item chunk but the first is empty for the whole call."""
    name = gd.SORTED
    cs, eng, kw = _engine(name)
    idx = np.flatnonzero(cs["facts"]["booklet_of"] == 0)
    assert len(idx) == 111 and (cs["y"][idx][:, 5:] == rd.MISSING).all()
    rows, data = _dev_rows(idx), torch.from_numpy(np.ascontiguousarray(cs["y"][idx]))
    _same_bits("score", eng.score(rows=rows, **kw), eng.score(data, **kw), ("eap", "psd", "loglik", "node"))
    _same_bits("expected_counts", eng.expected_counts(rows=rows, **kw), eng.expected_counts(data, **kw), ("n1", "n0", "mass", "prob"))
    _same_bits("item_information", eng.item_information(rows=rows, **kw), eng.item_information(data, **kw), ("info", "gradient"))
    a, b = eng.residual_sums(rows=rows, **kw), eng.residual_sums(data, **kw)
    _same_bits("residual_sums", a, b, TABLES + ("theta_hat",))
    assert (_np(a["n"])[5:] == 0).all() and (_np(a["sp"])[:, 5:] == 0).all()
    a, b = eng.fit_sums(rows=rows, **kw), eng.fit_sums(data, **kw)
    _same_bits("fit_sums", a["person"], b["person"], fc.PERSON)
    _same_bits("fit_sums", a["item"], b["item"], fc.ITEM)
    for method in pc.METHODS:
        _same_bits("point_estimates " + method, eng.point_estimates(rows=rows, method=method, **POINT_KW, **kw),
                   eng.point_estimates(data, method=method, **POINT_KW, **kw), ("theta_hat", "info", "status", "iterations"))
    # ... and the same persons' entries of the call over everybody
    full = eng.score(**kw)
    _same_bits("score against the full call", eng.score(rows=rows, **kw), {k: v[rows] for k, v in full.items()}, ("eap", "psd", "loglik", "node"))


# ---- the conditioned prior -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gd.POP))
def test_conditioned_prior(name):
    cs, eng, kw = _engine(name)
    p = gd.population(name)
    want = p["want"]
    eng.population = {"gamma": p["gamma"], "sigma": p["sigma"], "intercept": True}
    cov_t = torch.from_numpy(p["cov"])
    got = eng.score(covariates=cov_t, **kw)
    torch.cuda.synchronize()
    _finite(name, got, ("loglik", "eap", "psd", "cov", "prior_mean"))
    pairs = [("loglik", _np(got["loglik"]), want["loglik"]), ("eap", _np(got["eap"]), want["mean"]), ("psd", _np(got["psd"]), want["sd"]),
             ("cov", _np(got["cov"]), want["cov"]), ("prior_mean", _np(got["prior_mean"]), want["prior_mean"])]
    _hold_rows(name + " conditioned", pairs)
    _hold_nodes(name + " conditioned", _np(got["node"]), want)
    assert torch.equal(got["cov"], got["cov"].transpose(1, 2))
    empty = cs["facts"]["empty_persons"]
    # an empty person returns their own prior N(Gamma^T x, Sigma) as the grid has it: the oracle's rows, by the row rule
    _hold_rows(name + " conditioned, the empty persons", [(k, g[empty], w[empty]) for k, g, w in pairs])
    assert np.abs(_f8(got["loglik"])[empty] - cs["J"] * gd.missing_constant()).max() <= ROW_TOL
    pvs = eng.plausible_values(draws=pop.PV_DRAWS, seed=pop.PV_SEED, covariates=cov_t, **kw)
    torch.cuda.synchronize()
    node, gap = p["draws"]
    _hold_draws(name + " conditioned", _np(pvs["node"]), node, gap)
    assert np.array_equal(_np(pvs["theta"]), gd.oracle(name)["coord"].astype(np.float32)[_np(pvs["node"])])
    _same_bits(name, got, eng.score(covariates=cov_t, **kw), list(got))
    _same_bits(name, pvs, eng.plausible_values(draws=pop.PV_DRAWS, seed=pop.PV_SEED, covariates=cov_t, **kw), list(pvs))


# ---- S-X2 by booklet -----------------------------------------------------------------------------------------------------
def test_sx2_by_booklet():
    name = gd.SORTED
    cs, eng, kw = _engine(name)
    y, f = cs["y"], cs["facts"]
    with pytest.raises(ValueError, match="items="):
        eng.sx2(**kw)                                                           # nobody is complete on all 70 items
    n_params = np.full(cs["J"], 2, np.int64)
    raised = 0
    for k in range(3):
        items = gd.booklet_items(name, k)
        want_score = xc.persons_oracle(y, None, items)
        t = eng.sumscore_tables(items=items, **kw)
        score = _np(t["score"])
        assert np.array_equal(score, want_score), k
        assert (score[f["booklet_of"] != k] == -1).all() and (score[f["empty_persons"]] == -1).all()
        if f["unanswered_item"] in items:
            assert (score == -1).all()
            with pytest.raises(ValueError, match="items="):
                eng.sx2(items=items, **kw)
            raised += 1
            continue
        got = eng.sx2(items=items, **kw)
        p1, p0, _, logw = _device_probs(eng, items, **kw)
        _hold_probs("%s booklet %d" % (name, k), p1, p0, *xc.irt_probs(cs, items)[:2])
        _hold_sx2("%s booklet %d" % (name, k), got, t, y, items, p1, p0, logw, n_params[items])      # o1, n integer-exact; n_dropped
        assert got["n_dropped"] == int((want_score < 0).sum()) and got["items"].tolist() == items.tolist()
        again = eng.sumscore_tables(items=items, **kw)
        _same_bits(name, t, again, ("e1", "e0", "dist", "o1", "n", "score"))
    assert raised == 1


# ---- no observed cell, one observed cell ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gd.DEGENERATE)
def test_a_matrix_with_no_or_one_observed_cell(name):
    cs, eng, kw = _engine(name)
    o, y, N, J = gd.oracle(name), cs["y"], cs["N"], cs["J"]
    one = name == "gd_single_cell"
    cell = cs["facts"].get("cell")
    some = np.zeros(N, bool)
    if one:
        some[cell[0]] = True

    def calls():
        out = {"score": eng.score(**kw), "counts": eng.expected_counts(**kw), "info": eng.item_information(**kw),
               "pairs": eng.residual_sums(**kw), "fit": eng.fit_sums(**kw), "pvs": eng.plausible_values(draws=gd.DRAWS, seed=gd.SEED, **kw)}
        out["fit"] = dict(out["fit"]["person"], **{"item_" + k: v for k, v in out["fit"]["item"].items()}, theta_hat=out["fit"]["theta_hat"])
        out["info"] = {k: out["info"][k] for k in ("info", "gradient")}
        return out

    a, b = calls(), calls()
    torch.cuda.synchronize()
    for c in a:
        _finite(name + " " + c, a[c], [k for k, v in a[c].items() if torch.is_tensor(v) and v.is_floating_point()])
        _same_bits(name + " " + c, a[c], b[c], list(a[c]))
    _hold_post(name, a["score"], o, cs)
    _hold_pvs(name, a["pvs"], o, cs)
    # counts: exact zeros; mass = N x the prior weights (one person's posterior in their place)
    cnt, fit = a["counts"], eng.item_fit(**kw)
    n1, n0 = _np(cnt["n1"]), _np(cnt["n0"])
    filled = np.zeros((J, 1), bool)
    if one:
        filled[cell[1]] = True
    assert (n1[~filled[:, 0]] == 0).all() and (n0 == 0).all() and (not one or n1[cell[1]].sum() > 0.99), name
    assert _row_errors(_f8(cnt["mass"])[None], o["counts"]["mass"][None], floor=1.0)[0] <= ROW_TOL
    if not one:
        assert _row_errors(_f8(cnt["mass"])[None], N * np.exp(o["counts"]["logw"])[None], floor=1.0)[0] <= ROW_TOL
    for k in ("md", "rmsd"):
        assert np.array_equal(np.isnan(_np(fit[k])), np.isnan(o["counts"][k])) and np.isnan(_np(fit[k])).sum() == J - int(one), (name, k)
    assert (_np(fit["n_obs"])[~filled[:, 0]] == 0).all()
    # info: exact zeros but for the one item's own block; item_se keeps nothing (one cell: a rank-one block, no standard errors)
    gi, gg = _np(a["info"]["info"]), _np(a["info"]["gradient"])
    own = np.zeros(2 * J, bool)
    if one:
        own[2 * cell[1]:2 * cell[1] + 2] = True
    assert (gi[~own] == 0).all() and (gi[:, ~own] == 0).all() and (gg[~own] == 0).all(), name
    if not one:
        out = eng.item_se(**kw)
        assert len(out["kept"]) == 0 and np.isnan(out["a"]).all() and np.isnan(out["b"]).all() and out["cov"].shape == (0, 0)
    # pairs: no q3 is finite and the summary is NaN
    t = a["pairs"]
    for k in TABLES:
        g = _np(t[k])
        assert (np.delete(np.delete(g, cell[1], 0), cell[1], 1) == 0).all() if one else (g == 0).all(), (name, k)
    ldp = eng.local_dependence(**kw)
    assert not np.isfinite(ldp["q3"]).any() and np.isnan(ldp["mean"]) and np.isnan(ldp["max"]) and len(ldp["value"]) == 0
    # person fit: exact zero sums, NaN statistics, for everybody but the one person
    pf, im = eng.person_fit(**kw), eng.item_msq(**kw)
    for k in fc.PERSON:
        assert (_np(a["fit"][k])[~some] == 0).all(), (name, k)
    for k in ("lz", "infit", "outfit"):
        assert np.isnan(pf[k][~some]).all(), (name, k)
    assert not one or (np.isfinite(pf["outfit"][some]).all() and np.isfinite(pf["infit"][some]).all())
    assert np.isnan(im["infit"][~filled[:, 0]]).all() and np.isnan(im["outfit"][~filled[:, 0]]).all()
    # point estimates: every status is empty, but the one person's
    for method in pc.METHODS:
        pt = eng.point_estimates(method=method, **POINT_KW, **kw)
        assert np.array_equal(pt["status"] == pc.EMPTY, ~some) and np.isnan(pt["theta_hat"][~some]).all(), (name, method)
        r = pc.ratios(cs, method, pt, tag=name)
        assert max(r.values()) <= pc.POINT_C
    # S-X2 counts complete persons only: the documented error
    with pytest.raises(ValueError, match="items="):
        eng.sx2(**kw)


# ---- the other instruction schedule --------------------------------------------------------------------------------------
CHILD = "(gd_sorted_j70 or gd_dina_k3 or groups_are_booklets or rows_of_one_booklet or sx2_by_booklet) and not second_schedule"
CHILD_PASSED = 3 * 2 + 2 * 2 + 1 + 1 + 3                                        # MAIN tests, INFO tests, points, the conditioned prior, the three named


def test_designs_under_a_second_schedule():
    """gd_sorted_j70 and gd_dina_k3 again -- every call, group_counts among them -- in a child process on the library built under
    the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", CHILD, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "%d passed" % CHILD_PASSED in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
