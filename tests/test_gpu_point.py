"""Point estimates on the GPU: vx_grid_point_irt at the ABI, IrtEngine.point_estimates, the model classes' method and at= on the
two diagnostics, against the float64 oracle of tests/point_cases.py.

The rules (tests/point_cases.py) are path-independent: the kernel's float32 theta_hat is taken as it is and the estimating
function evaluated at it in float64 -- |s_d| <= tol + C u_d for every converged person, |theta_hat - root| <= tol + C u_d where the
objective is concave, the information within C 2^-23 of the sum of its terms, at_bound persons on the bound with s pointing
outward, empty persons exactly where y has no observed cell.  C = point_cases.POINT_C, set from the largest ratio measured on one
MI355X (written beside the constant), not chosen in advance.  The ratios found are printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import point_cases as pc
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
C = pc.POINT_C
_ENGINES = {}


def _engine(case):
    """The case and an engine holding its drawn parameters, made once a case."""
    if case[0] not in _ENGINES:
        cs = pc.sanity_case() if case[0] == pc.SANITY[0] else pc.case_of(case)
        _ENGINES[case[0]] = (cs, _irt_engine(cs))
    return _ENGINES[case[0]]


def _abi(eng, cs, method, theta0, rows=None, y_u8=None, max_iter=pc.MAX_ITER, tol=pc.TOL, bound=sc.SPAN):
    """vx_grid_point_irt itself through the engine's call, from theta0 (float32 numpy [n][D]).  The outputs start as NaN / -1:
    every entry has to be written.  Returns device tensors."""
    call = eng._grid_call(y_u8, rows, cs["nodes"], cs["span"])
    n, D = call.n, call.D
    flat = lambda name: eng.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
    params = (eng.unconstrained("a").contiguous() if cs["model"] != "irt_1pl" else None, flat("b"),
              flat("c") if cs["model"] in ("irt_3pl", "irt_4pl") else None, flat("d") if cs["model"] == "irt_4pl" else None)
    out = {"theta_hat": torch.full((n, D), float("nan"), dtype=torch.float32, device=_dev()),
           "info": torch.full((D * (D + 1) // 2, n), float("nan"), dtype=torch.float32, device=_dev()),
           "status": torch.full((n,), -1, dtype=torch.int32, device=_dev()), "iters": torch.full((n,), -1, dtype=torch.int32, device=_dev())}
    from vipsy_amd.grid import POINT_METHODS
    eng.be.grid_point_irt(call.cfg, call.y, call.rows, n, torch.from_numpy(np.ascontiguousarray(theta0, np.float32)).to(_dev()),
                          *params, POINT_METHODS[method], max_iter, tol, bound, pc.STEP_CAP, out["theta_hat"], out["info"],
                          out["status"], out["iters"])
    torch.cuda.synchronize()
    return out


def _host(out, D):
    """Device results -> what point_cases.ratios takes."""
    from vipsy_amd.grid import tri_to_full
    return {"theta_hat": _np(out["theta_hat"]), "info": tri_to_full(_np(out["info"]).T.astype(np.float64), D),
            "status": _np(out["status"]), "iterations": _np(out["iters"])}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) or (k in ("theta_hat", "info") and np.array_equal(_np(a[k]), _np(b[k]), equal_nan=True))
               for k in ("theta_hat", "info", "status", "iters"))


@pytest.mark.parametrize("case,method", pc.CASE_METHODS, ids=pc.CASE_METHOD_IDS)
def test_estimates_at_the_abi(case, method):
    """Every case and method from the oracle's EAP (as float32), tol 1e-6, 64 evaluations at the most: the rules, the caps, ml's
    at_bound persons exactly the oracle's, and the same call again gives the same bits."""
    cs, eng = _engine(case)
    th0 = pc.eap_of(case).astype(np.float32)
    out = _abi(eng, cs, method, th0)
    got = _host(out, cs["D"])
    root = pc.root_of(case, method)
    r = pc.ratios(cs, method, got, root=root, tag=case[0])
    counts = {pc.STATUS[k]: int((got["status"] == k).sum()) for k in range(5)}
    print("%s %s: s %.2f root %.2f info %.2f (C = %g); %s; iterations max %d"
          % (case[0], method, r["s"], r["root"], r["info"], C, counts, got["iterations"].max()))
    assert max(r.values()) <= C, r
    many = (cs["y"] < 2).sum(1) >= pc.MIN_ITEMS
    assert not many.any() or (got["status"][many] == pc.MAX_ITERS).mean() <= pc.MAX_ITER_CAP
    if cs["model"] == "irt_2pl":
        assert counts["singular"] == 0
    if method == "ml":
        assert np.array_equal(got["status"] == pc.AT_BOUND, root["status"] == pc.AT_BOUND)
    assert _same(out, _abi(eng, cs, method, th0))


NB = (1, 31, 32, 33, 97)


@pytest.mark.parametrize("shuffled", [False, True], ids=["file_order", "shuffled"])
@pytest.mark.parametrize("nb", NB)
def test_units_straddled_through_rows(nb, shuffled):
    """nb persons of the 2PL case through `rows` -- one person, one short of a unit of 32, a unit, one past it, four units the last
    with one person -- in file order and shuffled: the rules on those rows, and every person's bits those of the call over all
    97 persons (a person's result does not depend on who is scored beside it)."""
    case = pc.CASES[0]
    cs, eng = _engine(case)
    th0 = pc.eap_of(case).astype(np.float32)
    rows = np.random.RandomState(nb).permutation(cs["N"])[:nb] if shuffled else np.arange(nb)
    for method in pc.METHODS:
        whole = _abi(eng, cs, method, th0)
        out = _abi(eng, cs, method, th0[rows], rows=torch.from_numpy(rows.astype(np.int64)).to(_dev()))
        r = pc.ratios(cs, method, _host(out, 1), y=cs["y"][rows], tag="%d rows" % nb)
        assert max(r.values()) <= C, (method, r)
        sel = torch.from_numpy(rows.astype(np.int64)).to(_dev())
        pick = {"theta_hat": whole["theta_hat"][sel], "info": whole["info"][:, sel], "status": whole["status"][sel],
                "iters": whole["iters"][sel]}
        assert _same(out, pick), (method, nb)


@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[7]], ids=[pc.IDS[0], pc.IDS[7]])
def test_halves_against_the_whole(case):
    """The persons split into two calls (as data, not rows) against one call: equal bits, 1-D wle and 3-D ml."""
    cs, eng = _engine(case)
    method = "wle" if cs["D"] == 1 else "ml"
    th0 = pc.eap_of(case).astype(np.float32)
    whole = _abi(eng, cs, method, th0)
    cut = 45
    a = _abi(eng, cs, method, th0[:cut], y_u8=torch.from_numpy(np.ascontiguousarray(cs["y"][:cut])))
    b = _abi(eng, cs, method, th0[cut:], y_u8=torch.from_numpy(np.ascontiguousarray(cs["y"][cut:])))
    joined = {"theta_hat": torch.cat([a["theta_hat"], b["theta_hat"]]), "info": torch.cat([a["info"], b["info"]], 1),
              "status": torch.cat([a["status"], b["status"]]), "iters": torch.cat([a["iters"], b["iters"]])}
    assert _same(whole, joined)


def test_a_slow_person_does_not_touch_its_stopped_neighbours():
    """The 3PL case under ml with bound = 24: the all-wrong row, answered below chance, walks to the bound one capped step at a
    time (>= 20 evaluations) while its neighbours in the wave stop after a few.  The unit's persons alone, one call each, and
    together: identical bits."""
    case = pc.CASES[2]
    cs, eng = _engine(case)
    th0 = pc.eap_of(case).astype(np.float32)
    unit = np.arange(32)
    rows = lambda idx: torch.from_numpy(np.asarray(idx, np.int64)).to(_dev())      # noqa: E731
    together = _abi(eng, cs, "ml", th0[unit], rows=rows(unit), bound=24.0)
    it = _np(together["iters"])
    print("evaluations of the unit: %s" % it.tolist())
    assert it[pc.ALL_WRONG] >= 20 and _np(together["status"])[pc.ALL_WRONG] == pc.AT_BOUND
    assert _np(together["theta_hat"])[pc.ALL_WRONG, 0] == -24.0
    near = [i for i in range(8) if i not in (pc.NOBODY, pc.ALL_CORRECT, pc.ALL_WRONG)]
    assert (it[near] <= 10).all() and (it[near] >= 1).all()
    for i in unit[:12]:
        alone = _abi(eng, cs, "ml", th0[i:i + 1], rows=rows([i]), bound=24.0)
        pick = {"theta_hat": together["theta_hat"][i:i + 1], "info": together["info"][:, i:i + 1],
                "status": together["status"][i:i + 1], "iters": together["iters"][i:i + 1]}
        assert _same(alone, pick), i


def test_max_iter_ends_where_it_is_told_to():
    """max_iter = 2 from a start far from the root: everybody with an answer has taken exactly two evaluations or stopped before,
    theta_hat is the second point evaluated and `info` is the information there."""
    case = pc.CASES[0]
    cs, eng = _engine(case)
    th0 = np.full((cs["N"], 1), 2.5, np.float32)
    out = _abi(eng, cs, "ml", th0, max_iter=2)
    got = _host(out, 1)
    assert (got["iterations"][got["status"] == pc.MAX_ITERS] == 2).all() and (got["status"] == pc.MAX_ITERS).sum() > 50
    r = pc.ratios(cs, "ml", got, tag="max_iter 2")
    assert r["info"] <= C
    one = pc.fisher64(cs, "ml", th0.astype(np.float64), max_iter=2, tol=pc.TOL)
    hit = got["status"] == pc.MAX_ITERS
    assert np.abs(got["theta_hat"][hit] - one["theta_hat"][hit]).max() <= 1e-4


# ---- the bare backend ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J,model,D,method", [(100, 1, "irt_2pl", 1, "map"), (33, 64, "irt_1pl", 1, "wle"), (70, 65, "irt_4pl", 2, "ml"),
                                                 (64, 1024, "irt_3pl", 3, "map"), (257, 37, "irt_2pl", 3, "ml")],
                         ids=["2pl_j1_map", "1pl_j64_wle", "4pl_j65_d2_ml", "3pl_j1024_d3_map", "2pl_n257_d3_ml"])
def test_entry_on_a_bare_backend(N, J, model, D, method):
    """vx_grid_point_irt on a HipBackend alone -- no engine, no grid -- on coin flips with drawn parameters from a drawn start:
    one item, one full tile of 64, one item into the second tile, the largest J, nine units; every model, one to three dimensions."""
    from vipsy_amd.engine import HipBackend
    from vipsy_amd.grid import POINT_METHODS
    from tests.test_gpu_fit import _coin_irt
    cs, th0 = _coin_irt(N, J, 0.2, 80 + J % 7 + N % 5, model, D)
    cs["y"][0] = 255
    be, dev = HipBackend(), _dev()
    p = {k: torch.from_numpy(np.ascontiguousarray(v if k == "a" else v.reshape(-1))).to(dev) for k, v in cs["params"].items()}
    out = {"theta_hat": torch.full((N, D), float("nan"), dtype=torch.float32, device=dev),
           "info": torch.full((D * (D + 1) // 2, N), float("nan"), dtype=torch.float32, device=dev),
           "status": torch.full((N,), -1, dtype=torch.int32, device=dev), "iters": torch.full((N,), -1, dtype=torch.int32, device=dev)}
    be.grid_point_irt(be.cfg(model, D, J, 0, cs["Dc"], 1.0, 0, 0, 0), torch.from_numpy(cs["y"]).to(dev), None, N,
                      torch.from_numpy(th0).to(dev), p.get("a"), p["b"], p.get("c"), p.get("d"), POINT_METHODS[method], pc.MAX_ITER,
                      pc.TOL, sc.SPAN, pc.STEP_CAP, out["theta_hat"], out["info"], out["status"], out["iters"])
    torch.cuda.synchronize()
    got = _host(out, D)
    root = pc.fisher64(cs, method, th0.astype(np.float64)) if pc.concave(cs) else None
    r = pc.ratios(cs, method, got, root=root, tag=cs["name"])
    print("%s %s: s %.2f root %.2f info %.2f (C = %g); %s" % (cs["name"], method, r["s"], r["root"], r["info"], C,
                                                            {pc.STATUS[k]: int((got["status"] == k).sum()) for k in range(5)}))
    assert max(r.values()) <= C, r
    assert got["status"][0] == pc.EMPTY


def test_bad_arguments_are_refused_on_the_device_too():
    from vipsy_amd import _hip
    case = pc.CASES[6]
    cs, eng = _engine(case)
    th0 = pc.eap_of(case).astype(np.float32)
    for kw in (dict(method="wle"), dict(method="ml", max_iter=0), dict(method="ml", max_iter=256), dict(method="ml", tol=0.0),
               dict(method="map", bound=float("inf"))):
        with pytest.raises(_hip.VxError):
            _abi(eng, cs, kw.pop("method"), th0, **kw)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _model(cs, cls=None, **kw):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = (cls or vi.VIRT)(data=torch.from_numpy(cs["y"]).to(_dev()), model=cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=7, **kw)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return m


@pytest.mark.parametrize("case,method", [(pc.CASES[0], "wle"), (pc.CASES[3], "map"), (pc.CASES[7], "ml")],
                         ids=["2pl-wle", "4pl-map", "2pl_d3-ml"])
def test_point_estimates_through_the_model_class(case, method):
    """VIRT.point_estimates on the posterior kernel's own EAP: the rules on what comes back, se and cov against the float64
    inverse of the returned information, NaN where there is no estimate, the reliability against the oracle's formula."""
    cs = pc.case_of(case)
    m = _model(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"], "max_iter": pc.MAX_ITER}
    out = m.point_estimates(method=method, **kw)
    assert set(out) == {"theta_hat", "se", "cov", "info", "status", "iterations", "n_converged", "reliability"}
    n, D = cs["N"], cs["D"]
    assert out["theta_hat"].shape == (n, D) and out["se"].shape == (n, D) and out["cov"].shape == (n, D, D) == out["info"].shape
    assert out["status"].shape == (n,) and out["iterations"].shape == (n,) and out["reliability"].shape == (D,)
    r = pc.ratios(cs, method, out, root=pc.root_of(case, method), tag=case[0])
    print("%s %s end to end: s %.2f root %.2f info %.2f (C = %g)" % (case[0], method, r["s"], r["root"], r["info"], C))
    assert max(r.values()) <= C, r
    ok = (out["status"] != pc.EMPTY) & (out["status"] != pc.SINGULAR)
    M = out["info"] + (np.eye(D) if method == "map" else 0.0)
    assert np.isnan(out["se"][~ok]).all() and np.isnan(out["cov"][~ok]).all() and (~ok).any()
    assert np.isfinite(out["se"][ok]).all()
    assert np.abs(np.einsum("nde,nef->ndf", out["cov"][ok], M[ok]) - np.eye(D)).max() <= 1e-9
    assert np.allclose(out["se"][ok] ** 2, np.diagonal(out["cov"][ok], axis1=1, axis2=2), rtol=1e-12)
    if method == "ml":
        atb = out["status"] == pc.AT_BOUND
        assert atb[pc.ALL_CORRECT] or cs["D"] > 1
        assert np.isfinite(out["se"][atb]).all()
    conv = out["status"] == pc.CONVERGED
    assert out["n_converged"] == conv.sum()
    want = 1.0 - (out["se"][conv] ** 2).mean(0) / out["theta_hat"][conv].astype(np.float64).var(0, ddof=1)
    assert np.allclose(out["reliability"], want, rtol=1e-12)
    again = m.engine.point_estimates(method=method, **kw)
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)
    new = cs["y"][:40].astype(np.float32)
    new[cs["y"][:40] == 255] = np.nan
    sub = m.point_estimates(data=torch.from_numpy(new), method=method, **kw)
    assert np.array_equal(sub["theta_hat"], out["theta_hat"][:40], equal_nan=True) and np.array_equal(sub["status"], out["status"][:40])
    by_rows = m.engine.point_estimates(rows=[5, 3, 70], method=method, **kw)
    assert np.array_equal(by_rows["theta_hat"], out["theta_hat"][[5, 3, 70]], equal_nan=True)


def test_vaeirt_is_served_and_defaults_are_those_documented():
    """A VaeIRT with 31 items and hidden_dim 24 (a padded engine: phantom items and hidden units): point_estimates() with its
    defaults -- wle, 32 evaluations, bound = span = 6 -- is that of the ABI fed the engine's own score()."""
    from vipsy_amd import vi
    case = pc.CASES[0]
    cs = pc.case_of(case)
    m = _model(cs, vi.VaeIRT, hidden_dim=24)
    out = m.point_estimates()
    eap = _np(m.engine.score()["eap"])
    by_hand = _abi(m.engine, dict(cs, nodes=61, span=6.0), "wle", eap, max_iter=32)
    assert np.array_equal(out["theta_hat"], _np(by_hand["theta_hat"]), equal_nan=True)
    assert np.array_equal(out["status"], _np(by_hand["status"])) and np.array_equal(out["iterations"], _np(by_hand["iters"]))
    r = pc.ratios(cs, "wle", out, tag="VaeIRT")
    assert max(r.values()) <= C, r


@pytest.mark.parametrize("amortized", [False, True], ids=["VIRT", "VaeIRT"])
def test_the_next_step_of_a_captured_engine_is_that_of_an_untouched_twin(amortized):
    """point_estimates() and the diagnostics at its estimates work in buffers of their own: after them the engine's state is
    untouched and its next (replayed) step is bit for bit that of a twin that never called them."""
    from vipsy_amd import vi
    from vipsy_amd.engine import LrSpec
    cs = pc.case_of(pc.CASES[0])
    kw = {"hidden_dim": 24} if amortized else {}
    A, B = (_twin(cs, vi.VaeIRT if amortized else vi.VIRT, kw) for _ in range(2))
    lr = LrSpec(1e-2)
    for m in (A, B):
        for _ in range(2):
            m.engine.step(lr)                                                   # the second step replays the captured graph
    if not amortized:
        assert A.engine._graphable() and A.engine._graph is not None
    state = {k: getattr(A.engine, k).clone() for k in ("P", "M", "V", "G")}
    for method in pc.METHODS:
        out = A.point_estimates(method=method)
        assert out["n_converged"] > 50
    A.person_fit(at="wle")
    A.local_dependence(at="ml")
    torch.cuda.synchronize()
    for k, v in state.items():
        assert torch.equal(getattr(A.engine, k), v), k
    la, lb = float(A.engine.step(lr)), float(B.engine.step(lr))
    torch.cuda.synchronize()
    assert la == lb
    for k in ("P", "M", "V") + (("PP", "MP", "VP") if A.engine.per_person else ()):
        assert torch.equal(getattr(A.engine, k), getattr(B.engine, k)), k


def _twin(cs, cls, kw):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = cls(data=torch.from_numpy(cs["y"]).to(_dev()), model=cs["model"], x_feature=1, seed=7, **kw)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return m


def test_refusals_on_the_device():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4),
              vi.VCCDM(data=yd, q=torch.from_numpy(q))):
        with pytest.raises(NotImplementedError) as e:
            m.point_estimates()
        assert len(str(e.value)) > 20
    c = vi.VCCDM(data=yd, q=torch.from_numpy(q))
    assert np.isfinite(c.person_fit(at="eap")["lz"]).any()
    for call in (c.person_fit, c.local_dependence):
        with pytest.raises(ValueError):
            call(at="wle")
    two = vi.VIRT(data=yd, model="irt_2pl", x_feature=2)
    with pytest.raises(NotImplementedError):
        two.point_estimates()
    with pytest.raises(NotImplementedError):
        two.person_fit(at="wle")
    assert np.isfinite(two.point_estimates(method="ml", nodes=21)["theta_hat"]).all()
    ok = vi.VIRT(data=yd, model="irt_3pl")
    with pytest.raises(NotImplementedError):
        ok.point_estimates(covariates=np.zeros((64, 1)))
    with pytest.raises(ValueError):
        ok.point_estimates(method="eap")
    with pytest.raises(ValueError):
        ok.point_estimates(max_iter=0)
    assert ok.point_estimates()["status"].shape == (64,)                        # 3PL is served


# ---- at= on the diagnostics ------------------------------------------------------------------------------------------------
def _estimates_by_hand(m, cs, method):
    """point_estimates()'s theta_hat as a device tensor, the EAP where there is no estimate (as the diagnostics document it)."""
    pt = m.point_estimates(method=method, nodes=cs["nodes"], span=cs["span"])
    eap = m.engine.score(nodes=cs["nodes"], span=cs["span"])["eap"]
    bad = (pt["status"] == pc.EMPTY) | (pt["status"] == pc.SINGULAR)
    est = torch.where(torch.from_numpy(bad).to(_dev())[:, None], eap, torch.from_numpy(pt["theta_hat"]).to(_dev())).contiguous()
    return est, bad, pt


@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[3]], ids=[pc.IDS[0], pc.IDS[3]])
def test_person_fit_at_the_wle_is_the_fit_kernel_fed_by_hand(case):
    """person_fit(at="wle") against vx_grid_fit_irt fed point_estimates()["theta_hat"] by hand: the same bits in every sum and
    statistic; NaN rows for the person without an estimate; and without at= the bits of at="eap"."""
    from vipsy_amd.grid import ITEM_SUMS, PERSON_SUMS, person_fit_host
    cs = pc.case_of(case)
    m = _model(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    est, bad, pt = _estimates_by_hand(m, cs, "wle")
    eng = m.engine
    call, _, _, run = eng._fit_call(None, None, **kw)
    f32 = dict(dtype=torch.float32, device=_dev())
    person, item = torch.full((len(PERSON_SUMS), cs["N"]), float("nan"), **f32), torch.full((len(ITEM_SUMS), cs["J"]), float("nan"), **f32)
    ws_floats = eng.be.grid_fit_workspace(call.n, call.J)
    run(est, person, item, torch.empty(ws_floats, **f32), ws_floats)
    torch.cuda.synchronize()
    t = m.fit_sums(at="wle", **kw)
    assert set(t) == {"person", "item", "theta_hat", "no_estimate"} and np.array_equal(_np(t["no_estimate"]), bad) and bad[pc.NOBODY]
    for i, k in enumerate(PERSON_SUMS):
        assert torch.equal(t["person"][k], person[i]), k
    for i, k in enumerate(ITEM_SUMS):
        assert torch.equal(t["item"][k], item[i]), k
    assert torch.equal(t["theta_hat"], est)
    pf = m.person_fit(at="wle", **kw)
    want = person_fit_host({k: _np(person[i]) for i, k in enumerate(PERSON_SUMS)})
    for k in ("lz", "infit", "outfit"):
        want[k][bad] = np.nan
        assert np.array_equal(pf[k], want[k], equal_nan=True), k
    assert np.isnan(pf["theta_hat"][bad]).all() and np.array_equal(pf["theta_hat"][~bad], pt["theta_hat"][~bad])
    assert np.isfinite(pf["lz"][~bad & (pf["n_obs"] >= 5)]).all()
    im = m.item_msq(at="wle", **kw)
    assert np.isfinite(im["infit"]).all()
    plain, eap = m.person_fit(**kw), m.person_fit(at="eap", **kw)
    assert set(plain) == set(eap) and all(np.array_equal(plain[k], eap[k], equal_nan=True) for k in plain)
    assert not np.array_equal(plain["lz"], pf["lz"], equal_nan=True)


def test_local_dependence_at_the_ml_is_the_pairs_kernel_fed_by_hand():
    """local_dependence(at="ml") against vx_grid_pairs_irt fed point_estimates(method="ml")["theta_hat"] by hand (the EAP for the
    person without an estimate): the same bits in the four tables and in q3; without at= the bits of at="eap"."""
    from vipsy_amd.grid import pair_q3_host
    case = pc.CASES[0]
    cs = pc.case_of(case)
    m = _model(cs)
    kw = {"nodes": cs["nodes"], "span": cs["span"]}
    est, bad, _ = _estimates_by_hand(m, cs, "ml")
    eng = m.engine
    call, _, _, run = eng._pairs_call(None, None, **kw)
    f32 = dict(dtype=torch.float32, device=_dev())
    tab = {k: torch.full((cs["J"], cs["J"]), float("nan"), **f32) for k in ("n", "s", "ss", "sp")}
    ws_floats = eng.be.grid_pairs_workspace(call.n, call.J)
    run(est, tab, torch.empty(ws_floats, **f32), ws_floats)
    torch.cuda.synchronize()
    t = m.residual_sums(at="ml", **kw)
    for k in tab:
        assert torch.equal(t[k], tab[k]), k
    assert torch.equal(t["theta_hat"], est)
    ld = m.local_dependence(at="ml", **kw)
    q3 = pair_q3_host(_np(tab["n"]), _np(tab["s"]), _np(tab["ss"]), _np(tab["sp"]), 8)
    assert np.array_equal(ld["q3"], q3, equal_nan=True)
    plain, eap = m.local_dependence(**kw), m.local_dependence(at="eap", **kw)
    assert all(np.array_equal(plain[k], eap[k], equal_nan=True) for k in plain)
    assert not np.array_equal(plain["q3"], ld["q3"], equal_nan=True)


# ---- a statistical sanity case ---------------------------------------------------------------------------------------------
def test_wle_is_less_biased_than_ml_in_the_tails_and_the_reliability_is_the_oracles():
    """4 096 persons x 40 items, 2PL, simulated theta (point_cases.sanity_case): over the persons with |theta| > 1.5 and status
    converged the mean of theta_hat_wle - theta is smaller in absolute value than that of theta_hat_ml - theta, and `reliability`
    lies within 0.05 of 1 - mean(se^2) / var computed by the oracle (tests/test_point_host.py checks both on the oracle first)."""
    cs, eng = _engine(pc.SANITY)
    ml = eng.point_estimates(method="ml", max_iter=pc.MAX_ITER)
    wle = eng.point_estimates(method="wle", max_iter=pc.MAX_ITER)
    st = pc.sanity_stats(cs, ml, wle)
    eap = pc.eap_of(pc.SANITY)
    o = pc.sanity_stats(cs, pc.fisher64(cs, "ml", eap, max_iter=pc.MAX_ITER, tol=pc.TOL), pc.fisher64(cs, "wle", eap, max_iter=pc.MAX_ITER, tol=pc.TOL))
    print("sanity on the device: mean error beyond 1.5: ml %.4f wle %.4f (oracle %.4f %.4f); reliability %.4f (oracle %.4f)"
          % (st["mean_ml"], st["mean_wle"], o["mean_ml"], o["mean_wle"], wle["reliability"][0], o["reliability"]))
    assert abs(st["mean_wle"]) < abs(st["mean_ml"])
    assert abs(wle["reliability"][0] - o["reliability"]) <= 0.05
    assert wle["n_converged"] == st["n_converged"] and (wle["status"] != pc.SINGULAR).all()


# ---- the other instruction schedule ------------------------------------------------------------------------------------------
def test_oracle_comparisons_under_a_second_schedule():
    """The comparisons at the ABI again, every case and method, in a child process on the library built under the other
    instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "estimates_at_the_abi", "-p",
           "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    print("\n".join(line for line in r.stdout.splitlines() if "(C = " in line))
    assert "%d passed" % len(pc.CASE_METHODS) in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
