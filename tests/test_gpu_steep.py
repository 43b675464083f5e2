"""The grid family on the GPU at steep slopes and at asymptotes near 0 and 1 (tests/steep_cases.py; tests/test_steep_host.py
checks the conditions of the cases and of the rules on the CPU).

1. score(), expected_counts() / item_fit(), plausible_values() and item_information() on tables of which 20 to 51 % sit on the
   clamp and on posteriors that live on two or three nodes (a DINA case: on one pattern), by the rules of
   tests/test_gpu_grid_corners.py as they stand -- the row rule (tol comes out as ROW_TOL on every output), the node rule, the
   count identities, symmetric info, dead parameters, the bits of a second call -- and: every output finite, the person
   without answers gets the prior back, attr_prob of a one-pattern posterior within ROW_TOL of 0 or 1.
2. vx_grid_fit_* and vx_grid_pairs_* at the ABI, fed the oracle's EAP and fisher64's ml estimate (the D = 3 twins also `corner`):
   |S - S64| <= FIT_C 2^-23 Y with the extended yardstick Y of steep_cases, lz / infit / outfit out of the same Y; the pairs by
   ld_cases' rules as they stand.
3. vx_grid_point_irt at the ABI from the oracle's EAP, and point_estimates() once end to end: s and root by point_cases.ratios
   with POINT_C, the information under the extended yardstick, ml's at_bound persons exactly fisher64's; the 2PL cases end nobody
   singular and at most MAX_ITER_CAP in max_iter; the asymptote cases are held to fisher64's own counts instead.
4. Beyond float32 (steep_3pl_d3 and its twins: |z| passes 110 at the corner): every sum finite but sz2 where an answer's float64
   odds exceed the largest float32, which is +inf, never NaN; ml's at_bound persons are fisher64's and nobody is singular whom fisher64 is not, off the persons
   steep_cases.STATUS_WAIVED names from the oracle alone; the converged count by the issue's count condition.
5. The tests at the ABI again in a child process on the library built under the other instruction schedule.

The ratios found are printed; docs/NOTEBOOK.md has the table."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import corner_cases as co
from tests import fit_cases as fc
from tests import point_cases as pc
from tests import score_cases as sc
from tests import steep_cases as st
from tests.test_gpu_fit import _abi_call as _fit_abi
from tests.test_gpu_fit import _rows_of
from tests.test_gpu_grid_corners import _f8, _hold_counts, _hold_draws, _hold_info, _hold_score, _same_bits
from tests.test_gpu_ld import TABLES, _hold_q3, _hold_tables
from tests.test_gpu_ld import _abi_call as _pairs_abi
from tests.test_gpu_parity import _dev
from tests.test_gpu_point import _abi as _point_abi
from tests.test_gpu_point import _host, _same
from tests.test_gpu_response_designs import ROW_TOL
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
_ENGINES = {}


def _engine(case):
    """The case and an engine holding its parameters, made once a case."""
    if case[0] not in _ENGINES:
        cs, kind = st.made(case)
        _ENGINES[case[0]] = (cs, kind, _ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs))
    return _ENGINES[case[0]]


def _kw(cs, kind):
    return {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}


# ---- 1. the tables on the clamp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", st.TABLE_CASES, ids=st.TABLE_IDS)
def test_saturated_tables(case):
    o = st.table_oracle(case)
    cs, kind, eng = _engine(case)
    tag = cs["name"]
    kw = _kw(cs, kind)
    assert all(t == ROW_TOL for t in o["tol"].values())
    got = eng.score(**kw)
    torch.cuda.synchronize()
    _hold_score(tag, got, o)
    _same_bits(tag, got, eng.score(**kw), list(got))
    if kind == "irt":
        # nobody's answers: the prior comes back
        logw, coord = o["logw"].astype(np.float64), o["coord"]
        w = np.exp(logw - logw.max())
        w /= w.sum()
        mean = w @ coord
        sd = np.sqrt(w @ (coord - mean) ** 2)
        assert np.abs(_f8(got["eap"])[st.NOBODY] - mean).max() <= ROW_TOL and np.abs(_f8(got["psd"])[st.NOBODY] - sd).max() <= ROW_TOL
        print("%s: smallest PSD %.4f (oracle %.4f)" % (tag, float(got["psd"].min()), o["post"]["sd"].min()))
    else:
        f = o["f"]
        p = np.exp(f - f.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        sure = p.max(1) > 1.0 - 1e-6
        ap = _f8(got["attr_prob"])[sure]
        assert sure.mean() >= 0.30 and np.minimum(ap, 1.0 - ap).max() <= ROW_TOL, np.minimum(ap, 1.0 - ap).max()
        assert np.array_equal(np.round(ap), o["coord"][o["post"]["node"][sure]])
    cnt, fit = eng.expected_counts(**kw), eng.item_fit(**kw)
    torch.cuda.synchronize()
    _hold_counts(tag, cnt, fit, o)
    _same_bits(tag, cnt, eng.expected_counts(**kw), ("n1", "n0", "mass", "prob"))
    pvs = eng.plausible_values(draws=co.DRAWS, seed=co.SEED, **kw)
    torch.cuda.synchronize()
    _hold_draws(tag, pvs, o)
    _same_bits(tag, pvs, eng.plausible_values(draws=co.DRAWS, seed=co.SEED, **kw), list(pvs))
    if co.has_info(case):
        i = co.info_oracle(case, st.made(case))
        assert all(t == ROW_TOL for t in i["tol"].values())
        inf = eng.item_information(**kw)
        torch.cuda.synchronize()
        _hold_info(tag, inf, i)
        _same_bits(tag, inf, eng.item_information(**kw), ("info", "gradient"))


# ---- 2. and 4. the diagnostics at the ABI ----------------------------------------------------------------------------------
FIT_RUNS = [(c, w) for c in st.IRT_CASES for w in st.estimates_of(c)]
FIT_IDS = ["%s-%s" % (c[0], w) for c, w in FIT_RUNS]


def _hold_fit(tag, person, item, o):
    rr = st.fit_ratios(_rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM), o)
    print("%s: %s  (C = %g; odds beyond float32: %d persons, %d items; left out of lz: %d)"
          % (tag, " ".join("%s %.2f" % kv for kv in rr.items()), fc.FIT_C, o["over_person"].sum(), o["over_item"].sum(), (~o["keep"]).sum()))
    assert max(rr.values()) <= fc.FIT_C, (tag, rr)


@pytest.mark.parametrize("case,which", FIT_RUNS, ids=FIT_IDS)
def test_fit_sums_at_the_abi(case, which):
    """vx_grid_fit_irt fed the estimate as float32, against the float64 sums at exactly that estimate; where an answer's odds are
    beyond float32 sz2 is +inf and everything else finite; the same call again gives the same bits."""
    cs, kind, eng = _engine(case)
    est32 = st.estimate(case, which)
    est = torch.from_numpy(est32).to(_dev())
    person, item = _fit_abi(eng, kind, cs, est)
    o = st.fit_sums(kind, cs, est32)
    _hold_fit("%s at %s" % (case[0], which), person, item, o)
    if which == st.CORNER:
        p = _rows_of(person, fc.PERSON)
        assert np.isfinite(p["l0"]).all() and np.isfinite(p["e"]).all() and np.isfinite(p["v"]).all()
        if case[3] != "irt_4pl":
            assert p["sz2"][st.ABERRANT] == np.inf and np.isfinite(np.delete(p["sz2"], st.ABERRANT)).all()
    again = _fit_abi(eng, kind, cs, est)
    assert torch.equal(person, again[0]) and torch.equal(item, again[1]), case[0]


def test_fit_sums_of_the_dina_case_at_the_abi():
    case = st.DINA
    cs, kind, eng = _engine(case)
    pat = st.table_oracle(case)["post"]["node"].astype(np.int32)
    est = torch.from_numpy(pat).to(_dev())
    person, item = _fit_abi(eng, kind, cs, est)
    _hold_fit(case[0], person, item, st.fit_sums(kind, cs, pat))
    again = _fit_abi(eng, kind, cs, est)
    assert torch.equal(person, again[0]) and torch.equal(item, again[1])


@pytest.mark.parametrize("case,which", FIT_RUNS, ids=FIT_IDS)
def test_pair_tables_at_the_abi(case, which):
    """vx_grid_pairs_irt by ld_cases' rules as they stand: the residuals are bounded by 1, nothing scales with z."""
    from vipsy_amd.grid import pair_q3_host
    cs, kind, eng = _engine(case)
    est32 = st.estimate(case, which)
    est = torch.from_numpy(est32).to(_dev())
    o = st.pairs_oracle(cs, est32)
    tag = "%s at %s" % (case[0], which)
    got = _pairs_abi(eng, kind, cs, est)
    _hold_tables(tag, got, o)
    _hold_q3(tag, pair_q3_host(*[_f8(got[k]) for k in TABLES], min_pairs=8), o)
    again = _pairs_abi(eng, kind, cs, est)
    for k in TABLES:
        assert torch.equal(got[k], again[k]), (tag, k)


# ---- 3. and 4. the point estimates -----------------------------------------------------------------------------------------
POINT_RUNS = [(c, m) for c in st.IRT_CASES for m in pc.METHODS if m != "wle" or c[4] == 1]
POINT_IDS = ["%s-%s" % (c[0], m) for c, m in POINT_RUNS]


def _hold_point(tag, case, cs, method, got, root, asked, start=None):
    """The rules on a point result; root and asked: fisher64 from the same start, to 1e-12 and as the kernel was asked to run.
    The cases scored from tables: the 2PL ones end nobody singular and at most MAX_ITER_CAP in max_iter; the asymptote ones are
    singular only where fisher64 is.  The D = 3 twins (MAX_ITER_CAP cannot be asked of them, 2PL included: fisher64 itself ends 4
    to 56 of 129 in max_iter, tests/test_steep_host.py asserts it): under ml the at_bound persons are exactly fisher64's and nobody
    is singular whom fisher64 is not, off the persons steep_cases.STATUS_WAIVED names from the oracle alone (start: fisher64's).
    Asymptote cases and twins: the converged count is not below fisher64's by more than fisher64's own max_iter count."""
    r = pc.ratios(cs, method, got, root=root, tag=tag)
    info, plain = st.point_info_ratio(cs, got)
    counts = {pc.STATUS[k]: int((got["status"] == k).sum()) for k in range(5)}
    want = {pc.STATUS[k]: int((asked["status"] == k).sum()) for k in range(5)}
    print("%s %s: s %.2f root %.2f info %.2f (under 2^-23 sum |t| alone: %.2f; C = %g); %s; fisher64 %s; iterations max %d"
          % (tag, method, r["s"], r["root"], info, plain, pc.POINT_C, counts, want, got["iterations"].max()))
    assert max(r["s"], r["root"], info) <= pc.POINT_C, (tag, r, info)
    if case in st.TABLE_IRT and pc.concave(cs):
        many = (cs["y"] < 2).sum(1) >= pc.MIN_ITEMS
        assert counts["singular"] == 0 and (got["status"][many] == pc.MAX_ITERS).mean() <= pc.MAX_ITER_CAP, (tag, counts)
    else:
        assert counts["converged"] >= want["converged"] - want["max_iter"], (tag, counts, want)
    if case in st.TABLE_IRT:
        _only_the_oracles_singular(tag, got, root, asked)
    else:
        waived = st.status_waived(cs, asked, method, start)
        differ = np.flatnonzero(got["status"] != asked["status"])
        print("%s %s: STATUS_WAIVED %d persons; status other than fisher64's: %s" % (tag, method, waived.sum(), [
            "%d%s %s (fisher64 %s)" % (i, " waived" if waived[i] else "", pc.STATUS[got["status"][i]], pc.STATUS[asked["status"][i]]) for i in differ]))
        bad = st.status_differences(got["status"], asked, waived, method)
        assert len(bad) == 0, (tag, method, "at_bound or singular other than in fisher64 on persons STATUS_WAIVED does not exempt", bad.tolist())
        if pc.concave(cs) and "corner" not in tag:
            assert counts["singular"] == 0, (tag, counts)
    return counts


def _only_the_oracles_singular(tag, got, root, asked):
    sing = (got["status"] == pc.SINGULAR) & (asked["status"] != pc.SINGULAR) & (root["status"] != pc.SINGULAR)
    assert not sing.any(), (tag, "singular here, not in fisher64", np.flatnonzero(sing))


@pytest.mark.parametrize("case,method", POINT_RUNS, ids=POINT_IDS)
def test_point_estimates_at_the_abi(case, method):
    cs, kind, eng = _engine(case)
    th0 = st.eap_of(case).astype(np.float32)
    out = _point_abi(eng, cs, method, th0)
    got = _host(out, cs["D"])
    root = st.fisher(case, method)
    _hold_point(case[0], case, cs, method, got, root, st.fisher(case, method, exact=False), st.eap_of(case))
    if method == "ml":
        if case in st.TABLE_IRT:
            assert np.array_equal(got["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND)
            assert got["status"][st.ALL_WRONG] == pc.AT_BOUND
        assert got["status"][st.ALL_CORRECT] == pc.AT_BOUND
    assert _same(out, _point_abi(eng, cs, method, th0))


D3_IDS = [c[0] for c in st.D3_TWINS]


@pytest.mark.parametrize("case", st.D3_TWINS, ids=D3_IDS)
def test_point_estimates_from_the_corner_at_the_abi(case):
    """ml with the all-correct person started at (6, 6, 6) and the all-wrong one at (-6, -6, -6): their first evaluation is at
    |z| > 110 on most items.  Everything that comes back is finite (the 3PL twin returned NaN information before
    gpt_cell took the limits of P_z / P and P_z / Q), the rules hold, and nobody else is touched by it: every other person has
    the bits of the call from the EAP."""
    cs, kind, eng = _engine(case)
    th0 = st.corner_start(case)
    out = _point_abi(eng, cs, "ml", th0)
    got = _host(out, cs["D"])
    assert np.isfinite(got["info"]).all() and np.isfinite(got["theta_hat"][1:]).all()
    root = pc.fisher64(cs, "ml", th0.astype(np.float64))
    asked = pc.fisher64(cs, "ml", th0.astype(np.float64), max_iter=pc.MAX_ITER, tol=pc.TOL)
    _hold_point(case[0] + " from the corner", case, cs, "ml", got, root, asked, th0.astype(np.float64))
    for who, sign in ((st.ALL_CORRECT, 1.0), (st.ALL_WRONG, -1.0)):
        # (not the corner itself: the one step taken between the two evaluations may move a coordinate inward -- fisher64 ends
        # the all-correct person of the 2PL and the 3PL twin at (6, 5.984, 6))
        assert (got["theta_hat"][who] == np.float32(sign * sc.SPAN)).any() and got["iterations"][who] <= 2
    plain = _host(_point_abi(eng, cs, "ml", st.eap_of(case).astype(np.float32)), cs["D"])
    rest = np.setdiff1d(np.arange(cs["N"]), [st.ALL_CORRECT, st.ALL_WRONG])
    assert all(np.array_equal(got[k][rest], plain[k][rest], equal_nan=True) for k in ("theta_hat", "status", "iterations", "info"))
    assert _same(out, _point_abi(eng, cs, "ml", th0))


@pytest.mark.parametrize("start", ["eap", st.CORNER])
@pytest.mark.parametrize("case", st.D3_TWINS, ids=D3_IDS)
def test_who_ends_singular_at_the_abi(case, start):
    """The D = 3 twins under ml: a person ends singular only where fisher64 ends them so or where STATUS_WAIVED applies -- the
    float64 information at fisher64's own last point has a condition number above 2^23.  The issue asked for `nobody singular
    whom fisher64 does not end so`; held that way the kernel fails five of the six instances (3PL from the EAP: persons 2, 3, 99,
    123; 4PL: 55, 90, 98, 107, 111, 122; from the corner the planted persons 1 and 2 as well, all three twins; fisher64: at_bound,
    one max_iter).  It is not the cell: at those points one item's a a^T carries the 3 x 3 information, whose float64 eigenvalues
    spread over 2^86 to 2^178 (5e-45, 8e-18, 2e-5 for person 2 of the 3PL twin), the other items' terms underflow float32 outright,
    and the second pivot of the Cholesky factor is an exact 0.  No float32 solve resolves that, and float64 (2^53) does not
    either: fisher64's `positive definite` there is the sign of rounding noise in np.linalg.det.  So the comparison leaves those
    persons out, by a condition read off the oracle alone; the persons found singular are printed and every one of them must
    be waived."""
    cs, kind, eng = _engine(case)
    th0 = st.corner_start(case) if start == st.CORNER else st.eap_of(case).astype(np.float32)
    got = _host(_point_abi(eng, cs, "ml", th0), cs["D"])
    asked = pc.fisher64(cs, "ml", th0.astype(np.float64), max_iter=pc.MAX_ITER, tol=pc.TOL)
    waived = st.status_waived(cs, asked, "ml", th0.astype(np.float64))
    sing = np.flatnonzero(got["status"] == pc.SINGULAR)
    print("%s from %s: singular %s; fisher64 ends them %s; waived %s" % (case[0], start, sing.tolist(), [pc.STATUS[k] for k in asked["status"][sing]],
                                                                       waived[sing].tolist()))
    assert ((asked["status"][sing] == pc.SINGULAR) | waived[sing]).all(), (case[0], start, sing[~waived[sing]])
    assert np.isfinite(got["info"]).all()


def test_a_person_who_lacks_a_dimension_ends_as_in_float64():
    """Exactly singular information is not what STATUS_WAIVED is about: persons of sat_2pl_steep_d2 and of steep_2pl_d3 who answered
    only the last item (which loads on the first dimension alone under the default a_free) or only the last two (no loading on the
    third) have a zero row in their information.  Their status is fisher64's -- singular --, beside ordinary rows whose status is
    fisher64's too."""
    for case, last in ((st.TABLE_IRT[1], (1,)), (st.D3_TWINS[0], (1, 2))):
        cs, kind, eng = _engine(case)
        J = cs["J"]
        y = np.ascontiguousarray(cs["y"][4:4 + 2 * len(last) + 4]).copy()
        for k, n in enumerate(last):
            y[2 * k], y[2 * k + 1] = 255, 255
            y[2 * k, J - n:], y[2 * k + 1, J - n:] = 1, 0
        th0 = np.zeros((len(y), cs["D"]), np.float32)
        got = _host(_point_abi(eng, cs, "ml", th0, y_u8=torch.from_numpy(y)), cs["D"])
        asked = pc.fisher64(cs, "ml", th0.astype(np.float64), y=y, max_iter=pc.MAX_ITER, tol=pc.TOL)
        print("%s: rows lacking a dimension and four ordinary ones: %s; fisher64 %s" % (case[0], [pc.STATUS[k] for k in got["status"]],
                                                                                       [pc.STATUS[k] for k in asked["status"]]))
        assert (asked["status"][:2 * len(last)] == pc.SINGULAR).all()
        assert np.array_equal(got["status"], asked["status"])


def test_point_estimates_end_to_end():
    """IrtEngine.point_estimates(method="ml") on sat_3pl_asym, from the posterior kernel's own EAP: the rules on what comes back."""
    case = st.TABLE_IRT[2]
    cs, kind, eng = _engine(case)
    out = eng.point_estimates(method="ml", max_iter=pc.MAX_ITER, tol=pc.TOL, nodes=cs["nodes"], span=cs["span"])
    got = {"theta_hat": out["theta_hat"], "info": out["info"], "status": out["status"], "iterations": out["iterations"]}
    root = st.fisher(case, "ml")
    _hold_point(case[0] + " end to end", case, cs, "ml", got, root, st.fisher(case, "ml", exact=False))
    assert np.array_equal(got["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND)
    ok = (out["status"] != pc.EMPTY) & (out["status"] != pc.SINGULAR)
    assert np.isfinite(out["se"][ok]).all() and np.isnan(out["se"][~ok]).all()
    again = eng.point_estimates(method="ml", max_iter=pc.MAX_ITER, tol=pc.TOL, nodes=cs["nodes"], span=cs["span"])
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)


# ---- 5. the other instruction schedule ---------------------------------------------------------------------------------------
def test_at_the_abi_under_a_second_schedule():
    """Every test at the ABI of this file again in a fresh child process, which runs nothing but pytest, on the library built
    under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "at_the_abi and not second",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    print("\n".join(line for line in r.stdout.splitlines() if "C = " in line))
    n = 2 * len(FIT_RUNS) + 1 + len(POINT_RUNS) + 3 * len(st.D3_TWINS)
    assert "%d passed" % n in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
