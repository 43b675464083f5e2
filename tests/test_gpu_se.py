"""Item-parameter information and standard errors on the GPU (vx_grid_wtable_* / vx_grid_info behind IrtEngine / CcdmEngine
.item_information and .item_se, and the model classes' methods) against the float64 oracle of tests/se_cases.py.

Engines are set up as tests/test_gpu_score.py does it: parameters copied into the engine's views, nothing trained on the GPU --
the SE cases stand at the oracle's own EM iterates (tests/golden/se/se_params.npz), the matrix-only cases at their drawn parameters.

Rules.  info: the project's row rule, _row_errors(got, want, floor = max diagonal) <= ROW_TOL (3e-5), one row = one parameter;
gradient as one row with floor = (max diagonal x n)^0.5, the Cauchy-Schwarz size of a column sum of S.  Standard errors:
relative error <= ROW_TOL x the oracle's condition number of the kept block (the perturbation bound of an inverse).  The
bounds do not come from the kernels: the same float32 + fp16-pair arithmetic said again in numpy (tests/test_se_host.py) stays
below 3.3e-6 for info and below 1.8e-6 for the standard errors on exactly these cases.  The errors found are printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import count_cases as cc
from tests import score_cases as sc
from tests import se_cases as se
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
ALL = [("se", e) for e in se.SE_CASES] + [("info", c) for c in se.INFO_CASES]
ALL_IDS = se.SE_IDS + se.INFO_IDS


def _case(tag, entry):
    """(cs with the parameters the engine is to stand at, kind, oracle)."""
    if tag == "se":
        cs, kind, params, o = se.se_oracle(entry)
        return dict(cs, params=params), kind, o
    cs, kind, o = se.info_oracle(entry)
    return cs, kind, o


def _engine(cs, kind):
    return _ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs)


def _kw(cs, kind):
    return {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _info_errors(got_info, got_grad, want_info, want_grad, n):
    top = float(np.abs(np.diag(want_info)).max())
    e_i, row = _row_errors(_f8(got_info), want_info, floor=top)
    e_g, _ = _row_errors(_f8(got_grad)[None, :], np.asarray(want_grad, np.float64)[None, :], floor=np.sqrt(top * n))
    return e_i, row, e_g


def _hold_info(tag, got, o):
    """The row rule on info and gradient, the exact structure, free and index; prints what it finds."""
    P = len(o["free"])
    info, grad = got["info"], got["gradient"]
    assert tuple(info.shape) == (P, P) and tuple(grad.shape) == (P,) and info.dtype == torch.float32 and info.is_cuda
    e_i, row, e_g = _info_errors(info, grad, o["info"], o["gradient"], o["n"])
    print("%s: P %d, info %.2e (row %d), gradient %.2e (rule: %.1e)" % (tag, P, e_i, row, e_g, ROW_TOL))
    assert e_i <= ROW_TOL and e_g <= ROW_TOL, (tag, e_i, row, e_g)
    assert torch.equal(info, info.t()), tag                                     # symmetric bit for bit
    assert got["n"] == o["n"] and isinstance(got["n"], int)
    assert np.array_equal(_np(got["free"]), o["free"]) and got["free"].dtype == torch.bool
    K = o["K"]
    assert np.array_equal(got["index"]["item"], np.arange(P) // K) and np.array_equal(got["index"]["k"], np.arange(P) % K)
    # a parameter without information in the oracle has exactly none here: its row, its column and its gradient are zeros
    dead = np.flatnonzero(np.diag(o["info"]) == 0)
    gi = _np(info)
    assert (gi[dead] == 0).all() and (gi[:, dead] == 0).all() and (_np(grad)[dead] == 0).all(), tag
    assert (np.diag(gi)[np.diag(o["info"]) > 0] > 0).all(), tag


@pytest.mark.parametrize("tag,entry", ALL, ids=ALL_IDS)
def test_info_vs_oracle(tag, entry):
    cs, kind, o = _case(tag, entry)
    eng = _engine(cs, kind)
    got = eng.item_information(**_kw(cs, kind))
    torch.cuda.synchronize()
    _hold_info(cs["name"], got, o)
    # two independent kernels against each other: the gradient the M-step would form from expected_counts() of this engine
    c = eng.expected_counts(**_kw(cs, kind))
    want = se.mstep_gradient(cs, kind, _f8(c["n1"]), _f8(c["n0"]), _f8(c["prob"]), cs["params"])
    top = float(np.abs(np.diag(o["info"])).max())
    e, _ = _row_errors(_f8(got["gradient"])[None, :], want[None, :], floor=np.sqrt(top * o["n"]))
    print("%s: gradient against the M-step's from expected_counts(): %.2e" % (cs["name"], e))
    assert e <= ROW_TOL, (cs["name"], e)
    # the same call twice: the same bits
    again = eng.item_information(**_kw(cs, kind))
    torch.cuda.synchronize()
    assert torch.equal(got["info"], again["info"]) and torch.equal(got["gradient"], again["gradient"])


@pytest.mark.parametrize("entry", se.SE_CASES, ids=se.SE_IDS)
def test_item_se_vs_oracle(entry):
    cs, kind, o = _case("se", entry)
    eng = _engine(cs, kind)
    got = eng.item_se(**_kw(cs, kind))
    want = eng._se_leaves(o["se"].copy())
    assert set(got) == set(want) | {"cov", "kept", "gradient_max", "condition"}
    assert np.array_equal(got["kept"], o["kept"])
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape == tuple(eng.unconstrained(k[0]).shape) and g.dtype == np.float64, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), (cs["name"], k)
        worst = max(worst, float(np.nanmax(np.abs(g / w - 1))))
    e_cov = np.abs(got["cov"] - o["cov"]).max() / np.abs(o["cov"]).max()
    print("%s: se %.2e relative, cov %.2e of its largest entry (bound: %.1e x condition %.1f = %.2e); condition %.1f, largest "
          "|gradient| %.2e (oracle %.2e)" % (cs["name"], worst, e_cov, ROW_TOL, o["condition"], ROW_TOL * o["condition"],
                                             got["condition"], got["gradient_max"], np.abs(o["gradient"][o["kept"]]).max()))
    assert worst <= ROW_TOL * o["condition"], (cs["name"], worst)
    assert abs(got["condition"] / o["condition"] - 1) <= ROW_TOL * o["condition"]
    assert got["cov"].shape == (len(o["kept"]),) * 2 and got["cov"].dtype == np.float64
    if cs["name"] == "se_dino_k4":
        assert len(o["free"]) - len(got["kept"]) == 4 and np.isnan(got["s_un"]).sum() == 4 and np.isnan(got["s"]).sum() == 4
        assert np.isfinite(got["g_un"]).all() and np.isfinite(got["g"]).all()
    if kind == "irt" and cs["D"] > 1:
        assert np.isnan(got["a"]).sum() == cs["D"] * (cs["D"] - 1) // 2 and np.isfinite(got["b"]).all()


def test_a_singular_block_is_a_value_error():
    """case1, 33 persons for 74 parameters: no pseudo-inverse."""
    cs, kind, o = _case("info", sc.IRT_CASES[0])
    with pytest.raises(ValueError) as e:
        _engine(cs, kind).item_se(**_kw(cs, kind))
    assert "item" in str(e.value) and "pivot" in str(e.value)


def test_second_unit_of_a_workgroup():
    """sc.second_unit_case: more persons than the launch has units in flight, so that a workgroup of k_grid_pscores takes a second
    unit (what the first leaves in the LDS must not reach it), the last unit ragged; the whole call against the oracle of all
    rows, and the tail's rows alone against the oracle of the tail."""
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    cs, _ = sc.second_unit_case(cus)
    eng = _irt_engine(cs)
    for tag, rows, y in (("all rows", None, cs["y"]), ("the tail", cs["tail"], cs["y_tail"])):
        o = se.oracle(cs, "irt", cs["params"], y=y)
        got = eng.item_information(rows=rows, nodes=cs["nodes"], span=cs["span"])
        torch.cuda.synchronize()
        _hold_info("second unit, " + tag, got, o)


def test_additivity_over_rows():
    """info(rows = A) + info(rows = B) = info() for a split at person 1 000 and for a shuffled `rows`: the row rule, not the bits
    (another order of the sums)."""
    cs, kind, o = _case("se", se.SE_CASES[0])
    eng = _engine(cs, kind)
    kw = _kw(cs, kind)
    whole = eng.item_information(**kw)
    N = cs["N"]
    perm = np.random.RandomState(6).permutation(N).astype(np.int64)
    for tag, parts in (("split at 1000", (np.arange(1000), np.arange(1000, N))), ("shuffled", (perm,)),
                       ("shuffled halves", (perm[:1234], perm[1234:]))):
        got = [eng.item_information(rows=torch.from_numpy(np.ascontiguousarray(r)).to(_dev()), **kw) for r in parts]
        torch.cuda.synchronize()
        assert sum(g["n"] for g in got) == N
        info = sum(_f8(g["info"]) for g in got)
        grad = sum(_f8(g["gradient"]) for g in got)
        e_i, row, e_g = _info_errors(info, grad, _f8(whole["info"]), _f8(whole["gradient"]), N)
        print("additivity, %s: info %.2e gradient %.2e" % (tag, e_i, e_g))
        assert e_i <= ROW_TOL and e_g <= ROW_TOL, (tag, e_i, row, e_g)


def _raw_info(eng, cs, kind, ws_floats):
    """vx_grid_info itself over all rows with a workspace of ws_floats floats (None: the preferred size)."""
    be = eng.be
    call, K, fill_wtable, _ = eng._info_call(None, None, **_kw(cs, kind))
    post = eng._grid_posterior(call)
    P, G, n = call.J * K, call.G, call.n
    f32 = dict(dtype=torch.float32, device=_dev())
    wimg = torch.empty(be.grid_wimage_bytes(P, G), dtype=torch.uint8, device=_dev())
    fill_wtable(wimg)
    if ws_floats is None:
        ws_floats = be.grid_info_workspace(n, P, G)
    info, grad, ws = torch.full((P, P), float("nan"), **f32), torch.full((P,), float("nan"), **f32), torch.empty(ws_floats, **f32)
    be.grid_info(call.y, call.rows, n, call.J, G, K, post["img"], wimg, call.logw, post["loglik"], info, grad, ws, ws_floats)
    torch.cuda.synchronize()
    return info, grad, (P, G, n)


@pytest.mark.parametrize("idx", [0, 5], ids=[se.SE_IDS[0], se.SE_IDS[5]])
def test_slabs_of_the_smallest_workspace(idx):
    """vx_grid_info with the smallest workspace it accepts (slabs of 256 persons: ten for the 2 500, six for the 1 500) against
    the preferred one (one slab): the row rule; each against the oracle; a workspace below the minimum is refused."""
    from vipsy_amd import _hip
    cs, kind, o = _case("se", se.SE_CASES[idx])
    eng = _engine(cs, kind)
    one, g_one, (P, G, n) = _raw_info(eng, cs, kind, None)
    lo = eng.be.grid_info_workspace_min(P, G)
    assert eng.be.grid_info_workspace(n, P, G) > lo and n > 5 * 256
    many, g_many, _ = _raw_info(eng, cs, kind, lo)
    e_i, row, e_g = _info_errors(many, g_many, _f8(one), _f8(g_one), n)
    print("%s: %d slabs against one: info %.2e gradient %.2e" % (cs["name"], -(-n // 256), e_i, e_g))
    assert e_i <= ROW_TOL and e_g <= ROW_TOL
    assert torch.equal(many, many.t())
    for inf, gr in ((one, g_one), (many, g_many)):
        a, _, b = _info_errors(inf, gr, o["info"], o["gradient"], n)
        assert a <= ROW_TOL and b <= ROW_TOL
    again, g_again, _ = _raw_info(eng, cs, kind, lo)
    assert torch.equal(many, again) and torch.equal(g_many, g_again)
    with pytest.raises(_hip.VxError):
        _raw_info(eng, cs, kind, lo - 1)


def _count_big_model(cls=None, **kw):
    from vipsy_amd import vi
    cs, kind, o = _case("se", se.SE_CASES[0])
    vi.clear_param_store()
    m = (cls or vi.VIRT)(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1, seed=7, **kw)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return m, cs, o


def test_unseen_respondents():
    """data = new rows, float with NaN and uint8 with 255: what the oracle gives for those rows under the model's parameters."""
    m, cs, _ = _count_big_model()
    rng = np.random.RandomState(12)
    new = sc.irt_case(("se_new_rows", 600, cs["J"], "irt_2pl", 1, 1.0, 61, 0.25, (0.5, 1.5), 31))["y"]      # (the items of COUNT_BIG: seed 31)
    new[rng.randint(0, 600, 5)] = 255                                           # five respondents without an answer
    o = se.oracle(cs, "irt", cs["params"], y=new)
    data = new.astype(np.float32)
    data[new == 255] = np.nan
    a = m.item_information(data=torch.from_numpy(data))
    b = m.item_information(data=new)
    torch.cuda.synchronize()
    _hold_info("600 unseen respondents", a, o)
    assert torch.equal(a["info"], b["info"]) and torch.equal(a["gradient"], b["gradient"])
    got = m.item_se(data=new)
    worst = max(float(np.abs(got[k] / w - 1).max()) for k, w in m.engine._se_leaves(o["se"].copy()).items())
    print("600 unseen respondents: se %.2e relative (condition %.1f)" % (worst, o["condition"]))
    assert o["condition"] <= se.CONDITION_MAX and worst <= ROW_TOL * o["condition"]
    with pytest.raises(ValueError):
        m.item_se(data=new[:, :36])


@pytest.mark.parametrize("amortized", [False, True], ids=["VIRT", "VaeIRT"])
def test_the_next_step_of_a_captured_engine_is_that_of_an_untouched_twin(amortized):
    from vipsy_amd import vi
    from vipsy_amd.engine import LrSpec
    cls = vi.VaeIRT if amortized else vi.VIRT
    A, cs, _ = _count_big_model(cls)
    B, _, _ = _count_big_model(cls)
    lr = LrSpec(1e-2)
    for m in (A, B):
        for _ in range(2):
            m.engine.step(lr)                                                   # the second step replays the captured graph
    if not amortized:
        assert A.engine._graphable() and A.engine._graph is not None
    state = {k: getattr(A.engine, k).clone() for k in ("P", "M", "V", "G")}
    out = A.item_se()
    assert np.isfinite(out["b"]).all()
    torch.cuda.synchronize()
    for k, v in state.items():
        assert torch.equal(getattr(A.engine, k), v), k
    la, lb = float(A.engine.step(lr)), float(B.engine.step(lr))
    torch.cuda.synchronize()
    assert la == lb
    for k in ("P", "M", "V") + (("PP", "MP", "VP") if A.engine.per_person else ()):
        assert torch.equal(getattr(A.engine, k), getattr(B.engine, k)), k


def test_public_surface():
    from vipsy_amd import vi
    m, cs, o = _count_big_model()
    inf = m.item_information()
    assert set(inf) == {"info", "gradient", "n", "free", "index"} and inf["info"].is_cuda and inf["n"] == cs["N"]
    out = m.item_se()
    assert set(out) == {"a", "b", "cov", "kept", "gradient_max", "condition"} and all(isinstance(out[k], np.ndarray) for k in ("a", "b", "cov", "kept"))
    assert out["a"].shape == out["b"].shape == (1, cs["J"])
    want = m.engine._se_leaves(o["se"].copy())
    assert max(np.abs(out[k] / want[k] - 1).max() for k in ("a", "b")) <= ROW_TOL * o["condition"]
    # the padded amortized engine: phantom items and dimensions are in nobody's matrix
    v, _, _ = _count_big_model(vi.VaeIRT, hidden_dim=32)
    print("VaeIRT engine: J %d (items %d), D %d (model %d)" % (v.engine.J, v.engine.J_items, v.engine.D, v.engine.D_model))
    got = v.item_information()
    assert tuple(got["info"].shape) == (2 * cs["J"],) * 2
    e_i, _, e_g = _info_errors(got["info"], got["gradient"], o["info"], o["gradient"], o["n"])
    assert e_i <= ROW_TOL and e_g <= ROW_TOL
    assert torch.equal(got["info"], inf["info"])                                # the guide plays no part
    # VCCDM
    cd, kind, od = _case("se", se.SE_CASES[5])
    vi.clear_param_store()
    c = vi.VCCDM(data=torch.from_numpy(cd["y"]).to(_dev()), q=torch.from_numpy(cd["q"]), model=cd["cdm"])
    for name, val in cd["params"].items():
        c.engine.unconstrained(name).copy_(torch.from_numpy(val).to(_dev()))
    out = c.item_se()
    assert set(out) == {"g_un", "s_un", "g", "s", "cov", "kept", "gradient_max", "condition"}
    wantc = c.engine._se_leaves(od["se"].copy())
    assert max(np.abs(out[k] / wantc[k] - 1).max() for k in ("g_un", "s_un", "g", "s")) <= ROW_TOL * od["condition"]


def test_classes_and_models_out_of_scope_refuse():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4),
              vi.VIRT(data=yd, model="irt_3pl")):
        for call in (m.item_information, m.item_se):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert len(str(e.value)) > 20


def test_oracle_comparisons_under_a_second_schedule():
    """The 2 500 persons and se_dina_k3 again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "(info_vs_oracle or item_se_vs_oracle) and (counts_2pl_n2500 or se_dina_k3)"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
