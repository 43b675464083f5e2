"""Person fit on the GPU: vx_grid_fit_irt / vx_grid_fit_cdm at the ABI, IrtEngine / CcdmEngine.fit_sums, .person_fit, .item_msq
and the model classes' methods against the float64 oracle of tests/fit_cases.py.

Rules (tests/fit_cases.py).  n equals the oracle's exactly, for persons and items.  Every other sum S = sum t:
|S - S64| <= C 2^-23 sum |t|, sum |t| from the oracle.  lz: |lz - lz64| <= C u, u = 2^-23 (sum |l| + sum |eps|) / sqrt(v), on the
persons with oracle n >= 5 and v > 0.25 (at most 5 % of a case's persons may be left out; tests/test_fit_host.py checks the
oracle against that cap on the CPU).  infit and outfit: relative error <= C 2^-23 times the sums in them (two, one).  C =
fit_cases.FIT_C, set from the largest ratio measured on one MI355X (written beside the constant), not chosen in advance.  The
ratios found are printed.  Engines are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fit_cases as fc
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
C = fc.FIT_C


def _engine(kind, case):
    cs = fc.case_of(kind, case)
    return cs, (_ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs))


def _kw(cs, kind):
    return {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}


def _rows_of(t, names):
    """[len(names)][n] float32 on the device -> {name: float64 numpy}."""
    return {k: _np(t[i]).astype(np.float64) for i, k in enumerate(names)}


def _hold(tag, person, item, o, cap=None):
    """The rules on the two sets of sums ({name: float64 numpy}); prints and returns the largest ratio found.  cap: the share of
    the persons the lz condition may leave out (the cases; the shape limits have persons with fewer than five answers)."""
    from vipsy_amd.grid import item_msq_host, person_fit_host
    assert np.array_equal(person["n"], o["person"]["n"]) and np.array_equal(item["n"], o["item"]["n"]), tag
    rp = fc.sum_ratios(person, o["person"], o["person_abs"], fc.PERSON)
    ri = fc.sum_ratios(item, o["item"], o["item_abs"], fc.ITEM)
    pf = person_fit_host(person)
    rl = fc.lz_ratio(pf["lz"], o)
    assert np.array_equal(np.isnan(pf["lz"]), np.isnan(o["lz"])), tag
    fi, fo = fc.msq_ratios(pf["infit"], pf["outfit"], o["infit"], o["outfit"])
    im = item_msq_host(item)
    gi, go = fc.msq_ratios(im["infit"], im["outfit"], o["item_infit"], o["item_outfit"])
    worst = max(list(rp.values()) + list(ri.values()) + [rl])
    print("%s: person %s | item %s | lz %.2f | infit %.2f outfit %.2f, items %.2f %.2f  (C = %g, left out of lz: %d)"
          % (tag, " ".join("%s %.2f" % kv for kv in rp.items()), " ".join("%s %.2f" % kv for kv in ri.items()), rl, fi, fo, gi,
             go, C, (~o["keep"]).sum()))
    assert worst <= C, (tag, rp, ri, rl)
    assert max(fi, gi) <= 2 * C and max(fo, go) <= C, (tag, fi, fo, gi, go)
    assert cap is None or (~o["keep"]).mean() <= cap, tag
    return worst


def _buffers(n, J):
    f32 = dict(dtype=torch.float32, device=_dev())
    return torch.full((len(fc.PERSON), n), float("nan"), **f32), torch.full((len(fc.ITEM), J), float("nan"), **f32)


def _abi_call(eng, kind, cs, est, y_u8=None, rows=None):
    """vx_grid_fit_* itself, fed `est` (theta_hat [n][D] float32 / pattern [n] int32) in place of the posterior's.  Outputs and
    workspace start as NaN: every entry has to be written."""
    call, name, key, run = eng._fit_call(y_u8, rows, **_kw(cs, kind))
    person, item = _buffers(call.n, call.J)
    ws_floats = eng.be.grid_fit_workspace(call.n, call.J)
    ws = torch.full((ws_floats,), float("nan"), dtype=torch.float32, device=_dev())
    run(est, person, item, ws, ws_floats)
    torch.cuda.synchronize()
    return person, item


def _oracle_estimate(kind, o):
    if kind == "cdm":
        return torch.from_numpy(o["pattern"].astype(np.int32)).to(_dev())
    return torch.from_numpy(np.ascontiguousarray(o["theta_hat"], dtype=np.float32)).to(_dev())


def _oracle_at(kind, cs, est, y=None):
    """The float64 sums at the estimates the kernel was given (float32 theta_hat taken as it is)."""
    return fc.sums(cs["y"] if y is None else y, fc.prob_at(kind, cs, np.asarray(est, np.float64) if kind == "irt" else est))


@pytest.mark.parametrize("kind,case", fc.ALL, ids=fc.ALL_IDS)
def test_sums_at_the_abi(kind, case):
    """Fed the oracle's theta_hat / pattern (as float32 / int32): both sets of sums and lz, infit, outfit out of them by the rules
    above, against the float64 formulas at exactly those estimates; and the same call again gives the same bits."""
    cs, eng = _engine(kind, case)
    est = _oracle_estimate(kind, fc.oracle(kind, case))
    o = _oracle_at(kind, cs, _np(est))
    person, item = _abi_call(eng, kind, cs, est)
    _hold(case[0], _rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM), o, fc.LEFT_OUT_CAP)
    again = _abi_call(eng, kind, cs, est)
    assert torch.equal(person, again[0]) and torch.equal(item, again[1]), case[0]


# ---- shape limits: coin-flip responses, drawn parameters, a drawn theta_hat / pattern --------------------------------------
def _coin_irt(N, J, missing, seed, model, D):
    """The draws keep |z| below about 6: these cases are about indices, and a float32 z carries |z| 2^-24 into exp(z)."""
    rng = np.random.RandomState(seed)
    y = (rng.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    y[rng.uniform(size=(N, J)) < missing] = 255
    p = {"b": (0.7 * rng.normal(size=(1, J))).astype(np.float32)}
    if model != "irt_1pl":
        p["a"] = (rng.uniform(0.5, 1.5, size=(D, J)) / D).astype(np.float32)
    if model in ("irt_3pl", "irt_4pl"):
        p["c"] = rng.normal(-1.5, 0.3, size=(1, J)).astype(np.float32)
    if model == "irt_4pl":
        p["d"] = rng.normal(2.0, 0.3, size=(1, J)).astype(np.float32)
    th = rng.normal(size=(N, D)).astype(np.float32)
    return {"name": "coin_%s_n%d_j%d_d%d" % (model[4:], N, J, D), "N": N, "J": J, "model": model, "D": D, "Dc": 1.0, "y": y, "params": p}, th


def _coin_irt_abi(cs, th):
    """vx_grid_fit_irt on a HipBackend alone: no engine, no grid."""
    from vipsy_amd.engine import HipBackend
    be, dev, J, N = HipBackend(), _dev(), cs["J"], cs["N"]
    p = {k: torch.from_numpy(np.ascontiguousarray(v if k == "a" else v.reshape(-1))).to(dev) for k, v in cs["params"].items()}
    person, item = _buffers(N, J)
    ws_floats = be.grid_fit_workspace(N, J)
    ws = torch.full((ws_floats,), float("nan"), dtype=torch.float32, device=dev)
    be.grid_fit_irt(be.cfg(cs["model"], cs["D"], J, 0, cs["Dc"], 1.0, 0, 0, 0), torch.from_numpy(cs["y"]).to(dev), None, N,
                    torch.from_numpy(th).to(dev), p.get("a"), p["b"], p.get("c"), p.get("d"), person, item, ws, ws_floats)
    torch.cuda.synchronize()
    return person, item


IRT_SHAPES = [(100, 1, "irt_2pl", 1), (100, 32, "irt_1pl", 1), (100, 33, "irt_4pl", 2), (70, 1024, "irt_3pl", 3),
              (1, 37, "irt_2pl", 1), (31, 37, "irt_3pl", 1), (32, 37, "irt_2pl", 2), (33, 37, "irt_4pl", 1), (257, 37, "irt_2pl", 3)]


@pytest.mark.parametrize("N,J,model,D", IRT_SHAPES, ids=["%s_n%d_j%d_d%d" % (m[4:], n, j, d) for n, j, m, d in IRT_SHAPES])
def test_shape_limits_irt(N, J, model, D):
    """One item, one full tile, one item into the second tile, the largest J (32 tiles: eight a wave); one person, one short of,
    exactly and one past a unit of 32, and nine units (nine workgroups' partials); every model, one to three dimensions."""
    cs, th = _coin_irt(N, J, 0.2, 50 + J % 7 + N % 5, model, D)
    person, item = _coin_irt_abi(cs, th)
    _hold(cs["name"], _rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM), _oracle_at("irt", cs, th))


def test_a_workgroup_takes_a_second_unit():
    """32 801 persons x 3 items: 1 026 units over 513 workgroups of two units each -- the stride over units runs a second time,
    and 513 partials reach every item sum."""
    from vipsy_amd.engine import HipBackend
    N, J = 32 * 1024 + 33, 3
    assert HipBackend().grid_fit_workspace(N, J) == 513 * 4 * J
    cs, th = _coin_irt(N, J, 0.2, 61, "irt_2pl", 1)
    person, item = _coin_irt_abi(cs, th)
    _hold(cs["name"], _rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM), _oracle_at("irt", cs, th))


@pytest.mark.parametrize("cdm,K,N,J", [("dina", 1, 100, 5), ("dino", 1, 33, 40), ("dina", 10, 257, 33), ("dino", 10, 100, 64)],
                         ids=["dina_k1", "dino_k1", "dina_k10", "dino_k10"])
def test_shape_limits_cdm(cdm, K, N, J):
    """vx_grid_fit_cdm on a HipBackend alone, DINA and DINO with one and with ten attributes, drawn patterns."""
    from vipsy_amd.engine import HipBackend
    rng = np.random.RandomState(70 + K + J)
    y = (rng.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    y[rng.uniform(size=(N, J)) < 0.2] = 255
    q = (rng.uniform(size=(K, J)) < (1.0 if K == 1 else 0.3)).astype(np.float32)
    q[rng.randint(0, K, size=J), np.arange(J)] = 1
    p = {"g": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32),
         "s": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)}
    pattern = rng.randint(0, 1 << K, size=N).astype(np.int32)
    cs = {"name": "coin_%s_k%d" % (cdm, K), "N": N, "J": J, "cdm": cdm, "K": K, "q": q, "y": y, "params": p}
    be, dev = HipBackend(), _dev()
    person, item = _buffers(N, J)
    ws_floats = be.grid_fit_workspace(N, J)
    ws = torch.full((ws_floats,), float("nan"), dtype=torch.float32, device=dev)
    be.grid_fit_cdm(be.hodina_cfg(K, J, 0, 1.0, 0, 0, 0), cdm == "dino", torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), None,
                    N, torch.from_numpy(pattern).to(dev), torch.from_numpy(p["g"].reshape(-1)).to(dev),
                    torch.from_numpy(p["s"].reshape(-1)).to(dev), person, item, ws, ws_floats)
    torch.cuda.synchronize()
    _hold(cs["name"], _rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM), _oracle_at("cdm", cs, pattern))


def test_workspace_below_the_size_is_refused():
    from vipsy_amd import _hip
    from vipsy_amd.engine import HipBackend
    cs, th = _coin_irt(100, 37, 0.2, 3, "irt_2pl", 1)
    be, dev = HipBackend(), _dev()
    person, item = _buffers(100, 37)
    need = be.grid_fit_workspace(100, 37)
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    with pytest.raises(_hip.VxError):
        be.grid_fit_irt(be.cfg("irt_2pl", 1, 37, 0, 1.0, 1.0, 0, 0, 0), torch.from_numpy(cs["y"]).to(dev), None, 100,
                        torch.from_numpy(th).to(dev), torch.from_numpy(cs["params"]["a"]).to(dev),
                        torch.from_numpy(cs["params"]["b"].reshape(-1)).to(dev), None, None, person, item, ws, need - 1)


def test_nobody_answered_and_answered_nothing():
    """An item nobody answered and a person who answered nothing: exact zeros in every one of their sums, NaN in lz, infit and
    outfit; everything else is finite."""
    from vipsy_amd.grid import item_msq_host, person_fit_host
    cs, th = _coin_irt(200, 37, 0.1, 47, "irt_2pl", 1)
    cs["y"][:, 11] = 255
    cs["y"][77] = 255
    person, item = _coin_irt_abi(cs, th)
    p, it = _rows_of(person, fc.PERSON), _rows_of(item, fc.ITEM)
    _hold("item 11 and person 77 without answers", p, it, _oracle_at("irt", cs, th))
    assert all(p[k][77] == 0 for k in fc.PERSON) and all(it[k][11] == 0 for k in fc.ITEM)
    pf, im = person_fit_host(p), item_msq_host(it)
    gone = np.arange(200) == 77
    for k in ("lz", "infit", "outfit"):
        assert np.array_equal(np.isnan(pf[k]), gone), k
    for k in ("infit", "outfit"):
        assert np.array_equal(np.isnan(im[k]), np.arange(37) == 11), k
    assert all(np.isfinite(v).all() for v in p.values()) and all(np.isfinite(v).all() for v in it.values())


def test_rows_equal_the_same_rows_passed_as_data():
    """rows = a subset of the training responses against the same rows handed over as y_u8: the same bits in every sum and in
    theta_hat."""
    kind, case = "irt", fc.PLANTED
    cs, eng = _engine(kind, case)
    sub = np.random.RandomState(5).permutation(cs["N"])[:1300].astype(np.int64)
    a = eng.fit_sums(rows=torch.from_numpy(sub).to(_dev()), **_kw(cs, kind))
    b = eng.fit_sums(y_u8=torch.from_numpy(np.ascontiguousarray(cs["y"][sub])), **_kw(cs, kind))
    torch.cuda.synchronize()
    assert set(a) == {"person", "item", "theta_hat"} and tuple(a["theta_hat"].shape) == (1300, 1)
    assert tuple(a["person"]) == fc.PERSON and tuple(a["item"]) == fc.ITEM
    assert torch.equal(a["theta_hat"], b["theta_hat"])
    for k in fc.PERSON:
        assert tuple(a["person"][k].shape) == (1300,) and torch.equal(a["person"][k], b["person"][k]), k
    for k in fc.ITEM:
        assert tuple(a["item"][k].shape) == (cs["J"],) and torch.equal(a["item"][k], b["item"][k]), k
    assert float(a["item"]["n"][0]) == float((cs["y"][sub, 0] < 2).sum())


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _model(kind, cs):
    from vipsy_amd import vi
    vi.clear_param_store()
    data = torch.from_numpy(cs["y"]).to(_dev())
    if kind == "cdm":
        m = vi.VCCDM(data=data, q=torch.from_numpy(cs["q"]), model=cs["cdm"])
    else:
        m = vi.VIRT(data=data, model=cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=7)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return m


@pytest.mark.parametrize("kind,case", fc.ALL, ids=fc.ALL_IDS)
def test_person_fit_on_the_engines_own_scores(kind, case):
    """The model class and its engine on the posterior kernel's own estimates: fit_sums(), person_fit() and item_msq() against the
    float64 formulas evaluated at the theta_hat / pattern returned; the estimates themselves against the oracle's as
    tests/test_gpu_ld.py holds them."""
    cs = fc.case_of(kind, case)
    m = _model(kind, cs)
    kw = _kw(cs, kind)
    t = m.fit_sums(**kw)
    torch.cuda.synchronize()
    name = "pattern" if kind == "cdm" else "theta_hat"
    assert set(t) == {"person", "item", name} and all(v.is_cuda and v.dtype == torch.float32 for v in t["person"].values())
    est = _np(t[name])
    if kind == "cdm":
        assert t[name].dtype == torch.int32
        want = sc.cdm_oracle(cs)
        clear = want["gap"] > sc.ARGMAX_GAP
        assert np.array_equal(est[clear].astype(np.int64), want["node"][clear]) and (~clear).mean() <= sc.ARGMAX_LEFT_OUT
    else:
        assert tuple(est.shape) == (cs["N"], cs["D"])
        print("%s: theta_hat %.2e from the oracle's" % (case[0], np.abs(est - fc.oracle(kind, case)["theta_hat"]).max()))
    o = _oracle_at(kind, cs, est)
    person = {k: _np(v).astype(np.float64) for k, v in t["person"].items()}
    item = {k: _np(v).astype(np.float64) for k, v in t["item"].items()}
    _hold(case[0] + ", end to end", person, item, o, fc.LEFT_OUT_CAP)
    pf = m.person_fit(**kw)
    assert set(pf) == {"lz", "infit", "outfit", "n_obs", "loglik0", "expected", "variance", name}
    assert pf["n_obs"].dtype == np.int64 and np.array_equal(pf["n_obs"], o["person"]["n"].astype(np.int64))
    assert np.array_equal(pf[name], est)
    for k, s in (("loglik0", "l0"), ("expected", "e"), ("variance", "v")):
        assert pf[k].dtype == np.float64 and np.array_equal(pf[k], person[s]), k
    assert fc.lz_ratio(pf["lz"], o) <= C
    fi, fo = fc.msq_ratios(pf["infit"], pf["outfit"], o["infit"], o["outfit"])
    assert fi <= 2 * C and fo <= C
    im = m.item_msq(**kw)
    assert set(im) == {"infit", "outfit", "n_obs"} and im["n_obs"].dtype == np.int64
    assert np.array_equal(im["n_obs"], o["item"]["n"].astype(np.int64))
    gi, go = fc.msq_ratios(im["infit"], im["outfit"], o["item_infit"], o["item_outfit"])
    assert gi <= 2 * C and go <= C
    e = m.engine.person_fit(**kw)
    assert all(np.array_equal(e[k], pf[k], equal_nan=True) for k in pf)


def test_the_planted_persons_come_first_through_the_model_class():
    """pf_2pl_n5000_j70_aberrant through VIRT: at least 200 of the 250 lowest lz are planted persons (the float64 oracle finds
    the count tests/test_fit_host.py prints); new respondents as float data with NaN are served."""
    kind, case = "irt", fc.PLANTED
    cs, who = fc.case_of(kind, case), fc.planted_persons()
    m = _model(kind, cs)
    out = m.person_fit()
    planted = np.zeros(cs["N"], bool)
    planted[who] = True
    hits = int(planted[np.argsort(out["lz"])[:250]].sum())
    print("planted, VIRT.person_fit(): %d of the 250 lowest lz are planted persons; mean lz planted %.2f, rest %.2f"
          % (hits, out["lz"][planted].mean(), out["lz"][~planted].mean()))
    assert np.isfinite(out["lz"]).all() and hits >= 200
    data = cs["y"][:700].astype(np.float32)
    data[cs["y"][:700] == 255] = np.nan
    new = m.person_fit(data=torch.from_numpy(data))
    assert np.array_equal(new["lz"], out["lz"][:700]) and np.array_equal(new["n_obs"], out["n_obs"][:700])
    with pytest.raises(ValueError):
        m.person_fit(data=cs["y"][:, :69])


def test_padded_amortized_engine_after_training():
    """A VaeIRT with 37 items and hidden_dim 24 (padded engine: phantom persons, items and dimensions) trained a few steps: the
    sums are those of the oracle computed from param() values alone -- phantoms count nowhere -- and fit(8), person_fit(),
    fit(8) leaves the bits of fit(16)."""
    from vipsy_amd import vi
    rng = np.random.RandomState(33)
    J = 37
    y = (rng.uniform(size=(150, J)) < 0.55).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.15] = 255

    def run(interrupt):
        vi.clear_param_store()
        m = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=1, hidden_dim=24, seed=5)
        opt = vi.Adam({"lr": 1e-2})
        mid = None
        if interrupt:
            m.fit(optim=opt, max_iter=8, progress=False)
            params = {"a": _np(vi.param("a")), "b": _np(vi.param("b"))}
            mid = (params, m.engine.fit_sums(), m.person_fit(), m.item_msq())
            m.fit(optim=opt, max_iter=8, progress=False)
        else:
            m.fit(optim=opt, max_iter=16, progress=False)
        torch.cuda.synchronize()
        eng = m.engine
        return (eng.P.clone(), eng.M.clone(), eng.V.clone()), mid, eng

    a, mid, eng = run(True)
    b, _, _ = run(False)
    assert eng.J_items == J and eng.J > J
    for x, z in zip(a, b):
        assert torch.equal(x, z)
    params, t, pf, im = mid
    assert params["a"].shape == (1, J) and tuple(t["item"]["n"].shape) == (J,) and tuple(t["person"]["n"].shape) == (150,)
    cs = {"name": "padded", "N": 150, "J": J, "D": 1, "nodes": 61, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "y": y, "params": params}
    o = _oracle_at("irt", cs, _np(t["theta_hat"]))
    _hold("padded VaeIRT after 8 steps", {k: _np(v).astype(np.float64) for k, v in t["person"].items()},
          {k: _np(v).astype(np.float64) for k, v in t["item"].items()}, o)
    assert np.array_equal(pf["n_obs"], (y < 2).sum(1)) and np.array_equal(im["n_obs"], (y < 2).sum(0))
    assert fc.lz_ratio(pf["lz"], o) <= C


def test_classes_out_of_scope_refuse():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4)):
        for call in (m.fit_sums, m.person_fit, m.item_msq):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert len(str(e.value)) > 20
    ok = vi.VIRT(data=yd, model="irt_3pl")
    assert np.isfinite(ok.person_fit()["lz"]).all() and np.isfinite(ok.item_msq()["infit"]).all()      # 3PL is served


def test_oracle_comparisons_under_a_second_schedule():
    """The oracle comparisons at the ABI again, every case, in a child process on the library built under the other instruction
    schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "sums_at_the_abi", "-p",
           "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "%d passed" % len(fc.ALL) in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
