"""Local dependence on the GPU: vx_grid_pairs_irt / vx_grid_pairs_cdm at the ABI, IrtEngine / CcdmEngine.residual_sums and
.local_dependence and the model classes' methods against the float64 oracle of tests/ld_cases.py.

Rules.  n equals the oracle's exactly.  s, ss, sp: the project's row rule, |got - want|_inf of a row against max(1, |want|_inf of
the row), <= ROW_TOL (3e-5).  q3: absolutely <= ROW_TOL on the off-diagonal pairs of the comparison condition (oracle n >= 8, both
oracle v / n > 0.01; ld_cases.condition, whose caps tests/test_ld_host.py checks on the CPU); case4_3pl_j500_sparse is compared
on its tables only.  The bounds do not come from the kernels: the same float32 + fp16-pair arithmetic said again in numpy
(tests/test_ld_host.py) stays below 2e-6 on the tables and below 4e-7 on q3 on exactly these cases.  The errors found are
printed.  Engines are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ld_cases as ld
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

TABLES = ("n", "s", "ss", "sp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")


def _engine(kind, case):
    cs = ld.case_of(kind, case)
    return cs, (_ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs))


def _kw(cs, kind):
    return {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _hold_tables(tag, got, want):
    """n exactly, s / ss / sp by the row rule, n and sp symmetric bit for bit; prints and returns the errors."""
    J = len(want["n"])
    for k in TABLES:
        assert tuple(got[k].shape) == (J, J) and got[k].dtype == torch.float32 and got[k].is_cuda, (tag, k)
        assert torch.isfinite(got[k]).all(), (tag, k)
    assert np.array_equal(_f8(got["n"]), want["n"]), tag
    assert torch.equal(got["n"], got["n"].t()) and torch.equal(got["sp"], got["sp"].t()), tag
    e = {k: ld.row_error(_f8(got[k]), want[k]) for k in ("s", "ss", "sp")}
    print("%s: J %d, s %.2e ss %.2e sp %.2e by the row rule (%.1e)" % (tag, J, e["s"], e["ss"], e["sp"], ROW_TOL))
    assert max(e.values()) <= ROW_TOL, (tag, e)
    return e


def _hold_q3(tag, q3, want):
    """q3 under the comparison condition; NaN exactly where the oracle's n is below 8."""
    keep = want["keep"]
    err = float(np.abs(q3[keep] - want["q3"][keep]).max()) if keep.any() else 0.0
    print("%s: q3 %.2e on %d of %d off-diagonal pairs (%.1e)" % (tag, err, keep.sum(), keep.size - len(keep), ROW_TOL))
    assert np.isfinite(q3[keep]).all() and err <= ROW_TOL, (tag, err)
    assert np.isnan(q3[want["n"] < 8]).all(), tag
    return err


def _abi_call(eng, kind, cs, est, ws_floats=None, y_u8=None, rows=None):
    """vx_grid_pairs_* itself, fed `est` (theta_hat [n][D] float32 / pattern [n] int32) in place of the posterior's, with a
    workspace of ws_floats floats (None: the preferred size).  The tables start as NaN: every entry has to be written."""
    call, name, key, run = eng._pairs_call(y_u8, rows, **_kw(cs, kind))
    J, n = call.J, call.n
    f32 = dict(dtype=torch.float32, device=_dev())
    if ws_floats is None:
        ws_floats = eng.be.grid_pairs_workspace(n, J)
    out = {k: torch.full((J, J), float("nan"), **f32) for k in TABLES}
    ws = torch.full((ws_floats,), float("nan"), **f32)
    run(est, out, ws, ws_floats)
    torch.cuda.synchronize()
    return out


def _oracle_estimate(kind, o):
    if kind == "cdm":
        return torch.from_numpy(o["pattern"].astype(np.int32)).to(_dev())
    return torch.from_numpy(np.ascontiguousarray(o["theta_hat"], dtype=np.float32)).to(_dev())


@pytest.mark.parametrize("kind,case", ld.ALL, ids=ld.ALL_IDS)
def test_tables_at_the_abi(kind, case):
    """Fed the oracle's theta_hat / pattern: the four tables by the rules above, q3 out of them under the condition, and the same
    call again gives the same bits."""
    cs, eng = _engine(kind, case)
    o = ld.oracle(kind, case)
    est = _oracle_estimate(kind, o)
    got = _abi_call(eng, kind, cs, est)
    _hold_tables(case[0], got, o)
    if ld.LEFT_OUT_CAP.get(case[0], 0.0) is not None:
        from vipsy_amd.grid import pair_q3_host
        _hold_q3(case[0], pair_q3_host(*[_f8(got[k]) for k in TABLES], min_pairs=8), o)
    again = _abi_call(eng, kind, cs, est)
    for k in TABLES:
        assert torch.equal(got[k], again[k]), (case[0], k)


# ---- shape limits: coin-flip responses, drawn parameters, a drawn theta_hat --------------------------------------------------
def _coin_case(N, J, missing, seed, model="irt_2pl", D=1):
    rng = np.random.RandomState(seed)
    y = (rng.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    y[rng.uniform(size=(N, J)) < missing] = 255
    p = {"b": rng.normal(size=(1, J)).astype(np.float32)}
    if model != "irt_1pl":
        p["a"] = rng.uniform(0.5, 1.5, size=(D, J)).astype(np.float32)
    if model in ("irt_3pl", "irt_4pl"):
        p["c"] = rng.normal(-1.5, 0.3, size=(1, J)).astype(np.float32)
    if model == "irt_4pl":
        p["d"] = rng.normal(2.0, 0.3, size=(1, J)).astype(np.float32)
    th = rng.normal(size=(N, D)).astype(np.float32)
    return {"name": "coin_n%d_j%d" % (N, J), "N": N, "J": J, "model": model, "D": D, "Dc": 1.702, "y": y, "params": p}, th


def _coin_abi(cs, th, ws_floats=None):
    """vx_grid_pairs_irt on a HipBackend alone: no engine, no grid."""
    from vipsy_amd.engine import HipBackend
    be, dev, J, N = HipBackend(), _dev(), cs["J"], cs["N"]
    p = {k: torch.from_numpy(np.ascontiguousarray(v if k == "a" else v.reshape(-1))).to(dev) for k, v in cs["params"].items()}
    f32 = dict(dtype=torch.float32, device=dev)
    if ws_floats is None:
        ws_floats = be.grid_pairs_workspace(N, J)
    out = {k: torch.full((J, J), float("nan"), **f32) for k in TABLES}
    ws = torch.full((ws_floats,), float("nan"), **f32)
    be.grid_pairs_irt(be.cfg(cs["model"], cs["D"], J, 0, cs["Dc"], 1.0, 0, 0, 0), torch.from_numpy(cs["y"]).to(dev), None, N,
                      torch.from_numpy(th).to(dev), p.get("a"), p["b"], p.get("c"), p.get("d"), out["n"], out["s"], out["ss"],
                      out["sp"], ws, ws_floats)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,J,missing,model,D", [(100, 1, 0.2, "irt_2pl", 1), (100, 32, 0.2, "irt_1pl", 1), (100, 33, 0.2, "irt_4pl", 2),
                                                 (300, 1024, 0.7, "irt_3pl", 3), (1, 37, 0.2, "irt_2pl", 1), (255, 37, 0.2, "irt_2pl", 1),
                                                 (256, 37, 0.2, "irt_2pl", 2), (257, 37, 0.2, "irt_2pl", 3)],
                         ids=["j1", "j32", "j33", "j1024_n300", "n1", "n255", "n256", "n257"])
def test_shape_limits(N, J, missing, model, D):
    """One item, one full tile, one item into the second tile, the largest J (528 tile pairs, 136 workgroup blocks); one
    person, and one short of, exactly and one past a slab of 256 -- at the preferred workspace and, where there is more than
    one slab or J is large, at the smallest."""
    cs, th = _coin_case(N, J, missing, 40 + J % 7 + N % 5, model, D)
    want = ld.tables(cs["y"], ld.irt_prob(cs, th))
    _hold_tables(cs["name"], _coin_abi(cs, th), want)
    if N > 256 or J == 1024:
        from vipsy_amd.engine import HipBackend
        _hold_tables(cs["name"] + ", smallest workspace", _coin_abi(cs, th, HipBackend().grid_pairs_workspace_min(J)), want)


def test_an_item_nobody_answered():
    """Its row and column of n are exactly zero, and so are those of s, ss and sp; q3 is NaN there and nowhere else."""
    from vipsy_amd.grid import pair_q3_host
    cs, th = _coin_case(200, 37, 0.1, 47)
    cs["y"][:, 11] = 255
    want = ld.tables(cs["y"], ld.irt_prob(cs, th))
    got = _coin_abi(cs, th)
    _hold_tables("item 11 unanswered", got, want)
    for k in TABLES:
        g = _np(got[k])
        assert (g[11] == 0).all() and (g[:, 11] == 0).all(), k
    q3 = pair_q3_host(*[_f8(got[k]) for k in TABLES], min_pairs=8)
    dead = np.zeros((37, 37), bool)
    dead[11], dead[:, 11] = True, True
    assert np.array_equal(np.isnan(q3), dead)


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_rows_equal_the_same_rows_passed_as_data():
    """rows = subset of the training responses against the same rows handed over as y_u8: the same bits in every table and in
    theta_hat -- a person's residuals do not depend on where in memory the row lies or on its place in the batch order."""
    cs, eng = _engine("irt", ld.PLANTED)
    sub = np.random.RandomState(5).permutation(cs["N"])[:1300].astype(np.int64)
    a = eng.residual_sums(rows=torch.from_numpy(sub).to(_dev()), **_kw(cs, "irt"))
    b = eng.residual_sums(y_u8=torch.from_numpy(np.ascontiguousarray(cs["y"][sub])), **_kw(cs, "irt"))
    torch.cuda.synchronize()
    assert set(a) == set(TABLES) | {"theta_hat"} and tuple(a["theta_hat"].shape) == (1300, 1)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["n"].max()) <= 1300 and float(a["n"][0, 0]) == float((cs["y"][sub, 0] < 2).sum())


def test_slabs_of_the_smallest_workspace():
    """The planted case (5 000 persons) with the smallest workspace -- twenty slabs of 256 persons, one chunk each -- against the
    preferred one (one slab of twenty chunks): within ROW_TOL / 10 by the row rule, n the same; each against the oracle; the same
    bits again; a workspace below the minimum is refused."""
    from vipsy_amd import _hip
    kind, case = "irt", ld.PLANTED
    cs, eng = _engine(kind, case)
    o = ld.oracle(kind, case)
    est = _oracle_estimate(kind, o)
    lo, pref = eng.be.grid_pairs_workspace_min(cs["J"]), eng.be.grid_pairs_workspace(cs["N"], cs["J"])
    assert lo < pref and cs["N"] > 19 * 256
    one = _abi_call(eng, kind, cs, est)
    many = _abi_call(eng, kind, cs, est, lo)
    e = {k: ld.row_error(_f8(many[k]), _f8(one[k])) for k in ("s", "ss", "sp")}
    print("planted, 20 slabs against one: s %.2e ss %.2e sp %.2e (%.1e)" % (e["s"], e["ss"], e["sp"], ROW_TOL / 10))
    assert max(e.values()) <= ROW_TOL / 10 and torch.equal(many["n"], one["n"])
    _hold_tables("planted, one slab", one, o)
    _hold_tables("planted, 20 slabs", many, o)
    again = _abi_call(eng, kind, cs, est, lo)
    for k in TABLES:
        assert torch.equal(many[k], again[k]), k
    with pytest.raises(_hip.VxError):
        _abi_call(eng, kind, cs, est, lo - 1)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", ld.ALL, ids=ld.ALL_IDS)
def test_local_dependence_on_the_engines_own_scores(kind, case):
    """engine.residual_sums() / local_dependence() on the posterior kernel's own estimates.  IRT: against the oracle as it is.
    DINA / DINO: the pattern equals the oracle's wherever its best and second-best pattern are not tied (score_cases.ARGMAX_GAP),
    and the tables are held to the float64 formulas at the pattern returned."""
    cs, eng = _engine(kind, case)
    o = ld.oracle(kind, case)
    t = eng.residual_sums(**_kw(cs, kind))
    torch.cuda.synchronize()
    if kind == "cdm":
        assert set(t) == set(TABLES) | {"pattern"} and t["pattern"].dtype == torch.int32
        pat = _np(t["pattern"]).astype(np.int64)
        clear = sc.cdm_oracle(cs)["gap"] > sc.ARGMAX_GAP
        assert np.array_equal(pat[clear], o["pattern"][clear]) and (~clear).mean() <= sc.ARGMAX_LEFT_OUT
        if not np.array_equal(pat, o["pattern"]):
            o = ld.tables(cs["y"], ld.cdm_prob(cs, pat))
            o["q3"], o["v"] = ld.q3_of_tables(o)
            o["keep"] = ld.condition(o)
            o["mean"], o["max"] = ld.summary(o["q3"])
    else:
        assert set(t) == set(TABLES) | {"theta_hat"} and tuple(t["theta_hat"].shape) == (cs["N"], cs["D"])
        e_th = float(np.abs(_f8(t["theta_hat"]) - o["theta_hat"]).max())
        print("%s: theta_hat %.2e from the oracle's" % (case[0], e_th))
    _hold_tables(case[0] + ", end to end", t, o)
    out = eng.local_dependence(**_kw(cs, kind))
    J = cs["J"]
    assert set(out) == {"q3", "n_pairs", "mean", "max", "item_j", "item_k", "value"}
    assert out["q3"].shape == (J, J) and out["q3"].dtype == np.float64
    assert out["n_pairs"].dtype == np.int64 and np.array_equal(out["n_pairs"], o["n"].astype(np.int64))
    assert np.array_equal(out["q3"], out["q3"].T, equal_nan=True)
    if ld.LEFT_OUT_CAP.get(case[0], 0.0) is None:
        return                                                      # tables only
    _hold_q3(case[0] + ", end to end", out["q3"], o)
    if ld.LEFT_OUT_CAP.get(case[0], 0.0) == 0.0:
        # every pair is under the condition: the summary is the oracle's
        print("%s: mean %.6f (oracle %.6f), max %.6f (oracle %.6f)" % (case[0], out["mean"], o["mean"], out["max"], o["max"]))
        assert abs(out["mean"] - o["mean"]) <= ROW_TOL and abs(out["max"] - o["max"]) <= ROW_TOL
        assert len(out["value"]) == min(20, J * (J - 1) // 2) and (out["item_j"] < out["item_k"]).all()
        assert np.array_equal(out["value"], out["q3"][out["item_j"], out["item_k"]])


def test_the_planted_pair_comes_first_through_the_model_class():
    from vipsy_amd import vi
    kind, case = "irt", ld.PLANTED
    cs, o = ld.case_of(kind, case), ld.oracle(kind, case)
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1, seed=7)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    out = m.local_dependence()
    print("planted, VIRT.local_dependence(): q3[0][1] %.4f, next |q3 - mean| %.4f, mean %.5f, max %.4f"
          % (out["q3"][0, 1], abs(out["value"][1] - out["mean"]), out["mean"], out["max"]))
    assert (out["item_j"][0], out["item_k"][0]) == (0, 1) and abs(out["value"][0] - o["q3"][0, 1]) <= ROW_TOL
    assert abs(out["value"][0] - 0.80) <= 0.01 and np.abs(out["value"][1:]).max() < 0.1
    assert abs(out["mean"] - o["mean"]) <= ROW_TOL and abs(out["max"] - o["max"]) <= ROW_TOL
    _hold_q3("planted, VIRT", out["q3"], o)
    t = m.residual_sums()
    assert all(torch.is_tensor(v) and v.is_cuda for v in t.values())
    # new respondents as float data with NaN, and top / min_pairs reach the engine
    data = cs["y"][:700].astype(np.float32)
    data[cs["y"][:700] == 255] = np.nan
    new = m.local_dependence(data=torch.from_numpy(data), top=3, min_pairs=300)
    assert len(new["value"]) == 3 and (new["item_j"][0], new["item_k"][0]) == (0, 1)
    assert np.array_equal(np.isnan(new["q3"]), new["n_pairs"] < 300)
    with pytest.raises(ValueError):
        m.local_dependence(data=cs["y"][:, :69])


def test_padded_amortized_engine_after_training():
    """A VaeIRT with 37 items and hidden_dim 24 (padded engine: phantom items and dimensions) trained a few steps: the tables are
    those of the oracle computed from param() values alone, and fit(8), local_dependence(), fit(8) leaves the bits of fit(16)."""
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
            mid = (params, m.engine.residual_sums(), m.local_dependence())
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
    params, t, out = mid
    assert params["a"].shape == (1, J) and tuple(t["n"].shape) == (J, J)
    cs = {"name": "padded", "N": 150, "J": J, "D": 1, "nodes": 61, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "y": y, "params": params}
    th = sc.irt_oracle(cs)["mean"]
    want = ld.tables(y, ld.irt_prob(cs, th))
    want["q3"], want["v"] = ld.q3_of_tables(want)
    want["keep"] = ld.condition(want)
    _hold_tables("padded VaeIRT after 8 steps", t, want)
    assert want["keep"].mean() > 0.9
    _hold_q3("padded VaeIRT after 8 steps", out["q3"], want)


def test_classes_out_of_scope_refuse():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4)):
        for call in (m.residual_sums, m.local_dependence):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert len(str(e.value)) > 20
    ok = vi.VIRT(data=yd, model="irt_3pl")
    with pytest.raises(ValueError):
        ok.local_dependence(min_pairs=1)
    assert np.isfinite(ok.local_dependence()["mean"])              # 3PL is served: nothing is refitted


def test_oracle_comparisons_under_a_second_schedule():
    """The planted case, case2 (4PL) and case6_dina_k3 at the ABI again, in a child process on the library built under the other
    instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "tables_at_the_abi and (q3_2pl_n5000 or case2_4pl or case6_dina_k3)"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "3 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
