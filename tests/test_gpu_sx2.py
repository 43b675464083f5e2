"""Summed-score tables, S-X2 and the score table on the GPU: vx_sumscore_model / _persons / _observed at the ABI, and
IrtEngine / CcdmEngine / the model classes' sumscore_tables(), sx2() and score_table() against the float64 oracle of
tests/sx2_cases.py.

Rules (tests/sx2_cases.py).  e1, e0, dist: |e - e64| <= C (Js + G) 2^-24 e64 + 2^-100 against the float64 recursion over the very
float32 p1, p0, logw the kernel read; C = sx2_cases.SX2_C, set from the largest ratio measured on one MI355X (written beside the
constant).  The integer tables equal numpy's exactly.  S-X2: the first-order propagation of the table rule through the cell terms
(sx2_oracle's `tol`); df and n_cells equal the oracle's exactly; every item of every case is compared.  The ratios found are
printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import score_cases as sc
from tests import sx2_cases as xc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
C = xc.SX2_C


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _model_call(be, cs, with_dist=True):
    """vx_sumscore_model on a HipBackend alone.  Outputs and workspace start as NaN: every entry has to be written."""
    Js, G = cs["Js"], cs["G"]
    nan = dict(dtype=torch.float32, device=_dev())
    e1, e0 = torch.full((Js, Js + 1), float("nan"), **nan), torch.full((Js, Js + 1), float("nan"), **nan)
    dist = torch.full((G, Js + 1), float("nan"), **nan) if with_dist else None
    ws_floats = be.sumscore_model_workspace(Js, G)
    ws = torch.full((ws_floats,), float("nan"), **nan)
    be.sumscore_model(_t(cs["p1"]), _t(cs["p0"]), _t(cs["logw"]), Js, G, e1, e0, dist, ws, ws_floats)
    torch.cuda.synchronize()
    return e1, e0, dist


@pytest.mark.parametrize("case", xc.MODEL_CASES, ids=xc.MODEL_IDS)
def test_model_tables_at_the_abi(case):
    """e1, e0 and dist by the rule; the exact zeros and exact shifts; the binomial node in closed form; the identities that need
    no oracle; the same call again, and the call without dist, give the same bits."""
    from vipsy_amd.engine import HipBackend
    be, cs = HipBackend(), xc.model_case(case)
    Js, G, o = cs["Js"], cs["G"], cs["oracle"]
    e1, e0, dist = _model_call(be, cs)
    got = {"e1": _np(e1).astype(np.float64), "e0": _np(e0).astype(np.float64), "dist": _np(dist).astype(np.float64)}
    ratios = {k: xc.table_ratio(got[k], o[k], Js, G) for k in ("e1", "e0", "dist")}
    print("%s: ratios %s  (C = %g)" % (case[0], "  ".join("%s %.3f" % kv for kv in ratios.items()), C))
    for k in got:
        assert np.isfinite(got[k]).all() and (got[k] >= 0).all(), (case[0], k)
    assert max(ratios.values()) <= C, (case[0], ratios)
    # exact zeros: no score 0 with item j right, no score Js with item j wrong; a certain and an impossible item
    assert (got["e1"][:, 0] == 0).all() and (got["e0"][:, Js] == 0).all(), case[0]
    if cs["sure"] is not None:
        rest = np.arange(G) != cs["binomial"]
        assert (got["dist"][rest, 0] == 0).all() and (got["dist"][rest, Js] == 0).all(), case[0]
        # leaving the certain item out is an exact shift: e1[sure][s] = w-sum of S_-sure(s - 1), and e0[sure] = 0 off the binomial node
        if G == 1:
            assert (got["e0"][cs["sure"]] == 0).all() and (got["e1"][cs["never"]] == 0).all(), case[0]
    if cs["binomial"] is not None:
        want = xc.binomial_row(Js, xc.BINOMIAL_P, 1.0 - xc.BINOMIAL_P)
        assert xc.table_ratio(got["dist"][cs["binomial"]], want, Js, G) <= C, case[0]
    # without an oracle: e1 + e0 is P(score = s) whichever item is left out; its sum is the sum of the weights; rows of dist sum to 1
    rho = C * (Js + G) * 2.0 ** -24
    tot = got["e1"] + got["e0"]
    assert (np.abs(tot - tot[0][None, :]) <= 2 * (rho * tot[0][None, :] + xc.FLOOR)).all(), case[0]
    wsum = np.exp(cs["logw"].astype(np.float64)).sum()
    assert (np.abs(tot.sum(1) - wsum) <= 2 * rho * wsum).all(), case[0]              # (the kernel's expf(logw) is inside the rule)
    assert (np.abs(got["dist"].sum(1) - 1.0) <= rho).all(), (case[0], np.abs(got["dist"].sum(1) - 1.0).max(), rho)
    again = _model_call(be, cs)
    bare = _model_call(be, cs, with_dist=False)
    assert torch.equal(e1, again[0]) and torch.equal(e0, again[1]) and torch.equal(dist, again[2]), case[0]
    assert torch.equal(e1, bare[0]) and torch.equal(e0, bare[1]) and bare[2] is None, case[0]


# ---- the integer kernels ---------------------------------------------------------------------------------------------------
def _integer_call(be, y, rows, items, J):
    """vx_sumscore_persons, the host's stable sort, vx_sumscore_observed: (score by batch position, o1), as numpy."""
    dev = _dev()
    y_d = _t(y)
    rows_d = None if rows is None else _t(rows.astype(np.int64))
    items_d = None if items is None else _t(items.astype(np.int32))
    nb = y.shape[0] if rows is None else len(rows)
    Js = J if items is None else len(items)
    score = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    be.sumscore_persons(y_d, rows_d, nb, J, items_d, Js, score)
    keep = torch.nonzero(score >= 0).reshape(-1)
    s_sorted, order = torch.sort(score[keep], stable=True)
    pos = keep[order]
    rows_sorted = (pos if rows_d is None else rows_d[pos]).contiguous()
    o1 = torch.full((Js, Js + 1), -7, dtype=torch.int32, device=dev)
    be.sumscore_observed(y_d, rows_sorted, int(rows_sorted.numel()), J, items_d, Js, s_sorted.contiguous(), o1)
    torch.cuda.synchronize()
    return _np(score), _np(o1)


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 5000])
def test_integer_tables_equal_numpy(nb):
    """score and o1 against numpy, exactly: rows NULL and a permutation with repeats, items NULL and a subset (a 255 / 254 in a
    listed item takes the person out, in an unlisted one it does not), one item, everybody with one score, empty score groups,
    nobody complete."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    rng = np.random.RandomState(nb)
    J = 37
    subset = np.sort(rng.choice(J, size=11, replace=False))
    perm = rng.randint(0, nb, size=nb + 3)                                     # with repeats, and longer than y
    seen = []
    for kind in ("mixed", "one_score", "gaps", "nobody"):
        y = xc.integer_data(nb, J, 100 + nb, kind)
        for rows in (None, perm):
            for items in (None, subset, np.array([4])):
                if kind == "nobody" and items is not None and 0 not in items:
                    continue                                                    # (item 0 carries the 255s: not listed, somebody is complete)
                score, o1 = _integer_call(be, y, rows, items, J)
                want = xc.persons_oracle(y, rows, items)
                sub = y if rows is None else y[rows]
                want_o1, want_n = xc.observed_oracle(sub, items, want)
                assert np.array_equal(score, want), (nb, kind, rows is None, items)
                assert np.array_equal(o1, want_o1), (nb, kind, rows is None, items)
                seen.append((kind, (want >= 0).sum(), (want_n > 0).sum()))
                if kind == "nobody":
                    assert (score == -1).all() and (o1 == 0).all()
                if kind == "one_score" and items is None:
                    assert (want_n > 0).sum() == 1
    if nb >= 255:                                                               # the cases are what they claim to be
        mixed = xc.integer_data(nb, J, 100 + nb, "mixed")
        full, part = xc.persons_oracle(mixed, None, None), xc.persons_oracle(mixed, None, subset)
        assert (full < 0).any() and ((part >= 0) & (full < 0)).any() and (part < 0).any()      # holes in listed and in unlisted items
        assert (mixed == 254).any() and (mixed == 255).any()
        gaps = xc.observed_oracle(xc.integer_data(nb, J, 100 + nb, "gaps"), None, xc.persons_oracle(
            xc.integer_data(nb, J, 100 + nb, "gaps"), None, None))[1]
        assert (gaps > 0).sum() == 3 and gaps[2:J].sum() == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _device_probs(eng, items=None, **kw):
    """The float32 p1, p0 the kernel reads (out of the engine's operand image), theta and logw, as numpy."""
    from vipsy_amd.grid import grid_image_probs
    call = eng._grid_call(None, None, **kw)
    p1, p0 = grid_image_probs(eng._grid_image(call), call.J, call.G)
    p1, p0 = _np(p1), _np(p0)
    if items is not None:
        p1, p0 = p1[items], p0[items]
    return p1, p0, _np(call.theta).astype(np.float64), _np(call.logw)


def _hold_probs(tag, p1, p0, want1, want0):
    """p1 and p0 out of the image against float64 probabilities made from the item parameters alone (tests/sx2_cases.py
    prob_ratio): p0 is P(y = 0), from its own table."""
    r1, r0 = xc.prob_ratio(p1, want1, want0), xc.prob_ratio(p0, want0, want1)
    print("%s: image probabilities against the parameters, in units of the rule: p1 %.3f  p0 %.3f" % (tag, r1, r0))
    assert p1.shape == want1.shape and p0.shape == want0.shape and max(r1, r0) <= 1.0, (tag, r1, r0)


def _hold_sx2(tag, got, tables, y, items, p1, p0, logw, n_params, min_expected=1.0, others=0):
    """sx2() and the sumscore_tables() behind it against the oracle over the device's own probabilities: the model tables by their
    rule, the integer tables exactly, the statistic by the propagated rule, df and n_cells exactly, the expected proportions by
    the rule propagated to them, every item.  others: scored persons who are not in y at all."""
    Js, G = p1.shape
    lw, o1, n, score = xc.host_tables(y, items, p1, p0, logw)
    rho = C * (Js + G) * 2.0 ** -24
    ratios = {k: xc.table_ratio(_np(tables[k]), lw[k], Js, G) for k in ("e1", "e0", "dist")}
    print("%s: table ratios %s  (C = %g)" % (tag, "  ".join("%s %.3f" % kv for kv in ratios.items()), C))
    assert max(ratios.values()) <= C, (tag, ratios)
    assert np.array_equal(_np(tables["o1"]), o1) and np.array_equal(_np(tables["n"]), n) and tables["n"].dtype == torch.int64, tag
    want = xc.sx2_oracle(lw["e1"], lw["e0"], o1, n, n_params, min_expected, rho=rho)
    assert (want["margin"] > xc.COLLAPSE_MARGIN).all(), (tag, want["margin"])
    err = np.abs(got["sx2"] - want["sx2"])
    print("%s: S-X2 %s, largest error / rule %.3f" % (tag, np.round(got["sx2"], 2), (err / want["tol"]).max()))
    assert np.array_equal(got["n_cells"], want["n_cells"]) and np.array_equal(got["df"], want["df"]), tag
    assert (err <= want["tol"]).all(), (tag, err, want["tol"])
    tail = np.array([xc.chi2_tail(x, d) for x, d in zip(got["sx2"], got["df"])])      # (p is the tail of the statistic as computed)
    assert np.allclose(got["p"], tail, rtol=1e-9, atol=1e-300, equal_nan=True), tag
    assert got["n_persons"] == int((score >= 0).sum()) and got["n_dropped"] == int((score < 0).sum()) + others, tag
    keep = n > 0
    assert np.array_equal(got["observed"][:, keep], o1[:, keep] / n[keep]) and np.isnan(got["observed"][:, ~keep]).all(), tag
    # expected = e1 / (e1 + e0): moves by at most 2 rho E (1 - E) (tests/sx2_cases.py), plus the floor's share
    tot = lw["e1"] + lw["e0"]
    E = lw["e1"] / np.where(tot > 0, tot, 1.0)
    assert np.isnan(got["expected"][:, ~keep]).all(), tag
    slack = 2 * rho * E * (1 - E) + 2 * xc.FLOOR / np.where(tot > 0, tot, 1.0) + 1e-15
    assert (np.abs(got["expected"] - E) <= slack)[:, keep].all(), tag
    return lw, o1, n, want


def test_planted_misfit_stands_out():
    """4 096 persons x 12 items under the generating 2PL parameters; item 5 was generated with a lower asymptote of 0.35 the model
    lacks: its S-X2 is more than ten times the largest of the eleven clean items.  The tables behind it hold their rules."""
    cs = xc.planted_case()
    eng = _irt_engine(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    got = eng.sx2(**kw)
    t = eng.sumscore_tables(**kw)
    p1, p0, theta, logw = _device_probs(eng, **kw)
    _hold_probs("planted", p1, p0, *xc.irt_probs(cs)[:2])
    lw, o1, n, want = _hold_sx2("planted", got, t, cs["y"], None, p1, p0, logw, cs["n_params"])
    clean = np.delete(got["sx2"], xc.PLANTED_ITEM)
    assert got["sx2"][xc.PLANTED_ITEM] > 10.0 * clean.max(), got["sx2"]
    assert got["n_dropped"] == 0 and got["items"].tolist() == list(range(12))
    assert np.array_equal(_np(t["score"]), xc.persons_oracle(cs["y"], None, None))
    again = eng.sumscore_tables(**kw)
    assert all(torch.equal(t[k], again[k]) for k in ("e1", "e0", "dist", "o1", "n", "score"))


def test_dina_sx2_and_score_table():
    """CcdmEngine (DINA, K = 3): S-X2 with two parameters an item, and attr_prob of the score table."""
    cs = sc.cdm_case(xc.DINA_CASE)
    eng = _ccdm_engine(cs)
    got = eng.sx2()
    p1, p0, theta, logw = _device_probs(eng)
    eta = vo.dina_eta(cs["K"], cs["q"].astype(np.float64))[0].T > 0               # [J][2^K]
    g_un, s_un = (cs["params"][k].astype(np.float64).reshape(-1, 1) for k in ("g", "s"))
    _hold_probs("dina", p1, p0, np.where(eta, xc.sigmoid(-s_un), xc.sigmoid(g_un)), np.where(eta, xc.sigmoid(s_un), xc.sigmoid(-g_un)))
    lw, o1, n, want = _hold_sx2("dina", got, eng.sumscore_tables(), cs["y"], None, p1, p0, logw, np.full(cs["J"], 2, np.int64))
    tab = eng.score_table()
    o = xc.score_table_oracle(lw["dist"], logw, theta)
    rho = C * (cs["J"] + len(logw)) * 2.0 ** -24
    assert set(tab) == {"score", "prob", "attr_prob", "items"} and tab["attr_prob"].shape == (cs["J"] + 1, 3)
    assert np.abs(tab["attr_prob"] - o["eap"]).max() <= 4 * rho and abs(tab["prob"].sum() - 1.0) <= rho + 2.0 ** -20


def test_booklets_through_items():
    """Two booklets, 30 % of the cells missing by design: nobody is complete on all items, so the default call raises and names
    items=; sx2(items=booklet) is S-X2 of that booklet's complete sub-matrix -- against the oracle over the sub-matrix alone, and
    bit for bit the call on that booklet's persons alone.  Through the model class."""
    from vipsy_amd import vi
    cs = xc.booklet_case()
    assert abs((cs["y"] == 255).mean() - 0.30) < 1e-12
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    with pytest.raises(ValueError, match="items="):
        m.sx2(**kw)
    for b, items in enumerate(cs["booklets"]):
        got = m.sx2(items=items, **kw)
        mine = cs["y"][cs["took"] == b]
        p1, p0, theta, logw = _device_probs(m.engine, items, **kw)
        _hold_probs("booklet %d" % b, p1, p0, *xc.irt_probs(cs, items)[:2])
        _hold_sx2("booklet %d" % b, got, m.sumscore_tables(items=items, **kw), mine[:, items], None, p1, p0, logw,
                  cs["n_params"][items], others=cs["N"] - len(mine))
        assert got["n_persons"] == len(mine) and got["n_dropped"] == cs["N"] - len(mine) and got["items"].tolist() == items.tolist()
        alone = m.sx2(data=torch.from_numpy(mine), items=items, **kw)
        for k in ("sx2", "df", "p", "n_cells", "observed", "expected"):
            assert np.array_equal(got[k], alone[k], equal_nan=True), (b, k)
        assert alone["n_dropped"] == 0


def test_score_table_against_the_oracle():
    """eap and psd of every summed score against the float64 oracle over the device's own probabilities; the probabilities of the
    scores sum to 1; with a subset of the items the table is that subset's."""
    cs = xc.planted_case()
    eng = _irt_engine(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    for items in (None, np.array([0, 3, 4, 9])):
        tab = eng.score_table(items=items, **kw)
        p1, p0, theta, logw = _device_probs(eng, items, **kw)
        Js, G = p1.shape
        o = xc.score_table_oracle(xc.lord_wingersky(p1, p0, logw)["dist"], logw, theta)
        rho = C * (Js + G) * 2.0 ** -24
        # post = w dist / prob moves by 2 rho relative; |theta - eap| <= 2 span
        assert np.abs(tab["eap"] - o["eap"]).max() <= 2 * rho * 2 * cs["span"], items
        assert (np.abs(tab["psd"] - o["psd"]) <= 2 * rho * (2 * cs["span"]) ** 2 / (2 * o["psd"])).all(), items
        assert np.abs(tab["prob"] - o["prob"]).max() <= rho and abs(tab["prob"].sum() - 1.0) <= rho + 2.0 ** -20, items
        assert tab["score"].tolist() == list(range(Js + 1)) and tab["eap"].shape == (Js + 1, 1) and tab["eap"].dtype == np.float64


def test_lsat6_score_table_is_increasing():
    """LSAT-6 (1 000 persons x 5 items) under a 1PL with positive Dc: a higher summed score, a higher EAP; and S-X2 runs on it."""
    from vipsy_amd.engine import IrtEngine
    y = np.load(os.path.join(HERE, "golden", "lsat6.npz"))["y"]
    eng = IrtEngine(torch.from_numpy(y).to(_dev()), model="irt_1pl", D=1, Dc=1.702, seed=3)
    p = y.mean(0)
    eng.unconstrained("b").copy_(torch.from_numpy((np.log(p / (1 - p)) / 1.702).astype(np.float32).reshape(1, -1)).to(_dev()))
    tab = eng.score_table()
    assert tab["eap"].shape == (6, 1) and (np.diff(tab["eap"][:, 0]) > 0).all() and (tab["psd"] > 0).all()
    assert abs(tab["prob"].sum() - 1.0) < 1e-5
    out = eng.sx2()
    assert out["n_persons"] == 1000 and out["df"].tolist() == (out["n_cells"] - 1).tolist() and np.isfinite(out["sx2"]).all()


def test_abi_comparisons_under_a_second_schedule():
    """The comparisons at the ABI again, every case, in a child process on the library built under the other instruction
    schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "at_the_abi or equal_numpy", "-p",
           "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "%d passed" % (len(xc.MODEL_CASES) + 5) in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
