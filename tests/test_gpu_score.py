"""Grid scores on the GPU (vx_grid_table_irt / vx_grid_table_cdm / vx_grid_posterior behind IrtEngine.score, CcdmEngine.score
and the model classes' score() / marginal_loglik()) against the float64 oracle of tests/score_cases.py.

Item parameters are drawn and set on the engine through its views, not trained.  Every output is held to the oracle by the
project's row rule, _row_errors(got, want, floor = 1) <= ROW_TOL (imported from tests/test_gpu_response_designs.py: the bound
the per-person ELBO rows already meet): loglik by its own magnitude, eap / psd / attr_prob absolutely (the prior's scale is
1).  node / pattern must equal the oracle's argmax wherever the oracle's best and second-best logw + ll differ by more than
1e-4; at most 2 % of the persons may be left out by that rule (tests/test_score_host.py checks on the CPU that the oracle
alone stays inside that cap, and that every IRT case keeps the oracle's PSD above half the node spacing; both are checked
here again).  The errors found are printed.

Shapes: the smallest that reach every branch -- one person tile + 1 row, ragged J and G (case 1), J beyond one item chunk
(2, 3), 32 item chunks (4), several node tiles, odd and even in number (5: 14 and 23 tiles; 6: 1 and 32), a wave's second
person tile partly and wholly empty."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")


def _np(t):
    return t.detach().cpu().numpy()


def _hold(tag, got, want, names):
    """The row rule on every output, the argmax rule on the node; prints what it finds."""
    errs = {}
    for g_name, w_name in names:
        e, worst = _row_errors(_np(got[g_name]).astype(np.float64), np.asarray(want[w_name], np.float64), floor=1.0)
        errs[g_name] = (e, worst)
    node_g = "node" if "node" in got else "pattern"
    sure = want["gap"] > sc.ARGMAX_GAP
    out = float((~sure).sum()) / len(sure)
    wrong = np.flatnonzero(sure & (_np(got[node_g]).astype(np.int64) != want["node"]))
    print("%s: %s; %.1f %% of the persons left out of the argmax rule, %d wrong nodes (row rule: %.1e)"
          % (tag, "  ".join("%s %.2e (row %d)" % (k, v[0], v[1]) for k, v in errs.items()), 100 * out, len(wrong), ROW_TOL))
    for k, (e, worst) in errs.items():
        assert e <= ROW_TOL, (tag, k, "person", worst, e)
    assert out <= sc.ARGMAX_LEFT_OUT, (tag, out)
    assert len(wrong) == 0, (tag, node_g, wrong[:10], _np(got[node_g])[wrong[:10]], want["node"][wrong[:10]])


IRT_NAMES = [("loglik", "loglik"), ("eap", "mean"), ("psd", "sd")]
CDM_NAMES = [("loglik", "loglik"), ("attr_prob", "mean")]


def _irt_engine(cs):
    from vipsy_amd.engine import IrtEngine
    eng = IrtEngine(torch.from_numpy(cs["y"]).to(_dev()), model=cs["model"], D=cs["D"], Dc=cs["Dc"], seed=3)
    for name, v in cs["params"].items():
        eng.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    if cs["D"] > 1:                                                   # the drawn slopes are masked by the engine's default a_free
        free = _np(eng.unconstrained("a", eng.free))
        assert np.array_equal(free != 0, vo.default_a_free(cs["D"], cs["J"]))
        assert (cs["params"]["a"][free == 0] == 0).all()
    return eng


def _ccdm_engine(cs):
    from vipsy_amd.engine import CcdmEngine
    eng = CcdmEngine(torch.from_numpy(cs["y"]).to(_dev()), cs["q"], cdm=cs["cdm"])
    for name, v in cs["params"].items():
        eng.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return eng


_WANT = {}


def _want(case):
    """The case and its oracle, computed once and shared (never modified)."""
    if case[0] not in _WANT:
        if case in sc.IRT_CASES:
            cs = sc.irt_case(case)
            _WANT[case[0]] = (cs, sc.irt_oracle(cs))
        else:
            cs = sc.cdm_case(case)
            _WANT[case[0]] = (cs, sc.cdm_oracle(cs))
    return _WANT[case[0]]


@pytest.mark.parametrize("case", sc.IRT_CASES, ids=[c[0] for c in sc.IRT_CASES])
def test_irt_scores_vs_oracle(case):
    cs, want = _want(case)
    lo, need = sc.irt_condition(cs, want)
    assert lo >= need, (cs["name"], "oracle PSD below half the node spacing", lo, need)
    eng = _irt_engine(cs)
    got = eng.score(nodes=cs["nodes"], span=cs["span"])
    torch.cuda.synchronize()
    assert got["eap"].shape == (cs["N"], cs["D"]) and got["psd"].shape == (cs["N"], cs["D"])
    assert got["loglik"].shape == (cs["N"],) and got["node"].shape == (cs["N"],)
    _hold(cs["name"], got, want, IRT_NAMES)
    if cs["name"].startswith("case1"):
        # nobody's answers: the prior's moments and J cells of the reference's constant; the centre node
        assert abs(float(got["eap"][5, 0])) <= ROW_TOL and abs(float(got["psd"][5, 0]) - want["sd"][5, 0]) <= ROW_TOL
        assert int(got["node"][5]) == 30 and (cs["y"][7] == 1).all()
        assert float(got["eap"][7, 0]) > 1.0


@pytest.mark.parametrize("case", sc.CDM_CASES, ids=[c[0] for c in sc.CDM_CASES])
def test_cdm_scores_vs_oracle(case):
    cs, want = _want(case)
    eng = _ccdm_engine(cs)
    got = eng.score()
    torch.cuda.synchronize()
    assert got["attr_prob"].shape == (cs["N"], cs["K"]) and got["pattern"].shape == (cs["N"],)
    _hold(cs["name"], got, want, CDM_NAMES)


def test_explicit_nodes_vs_oracle():
    """Explicit (theta, logw): an uneven grid of 45 nodes with uneven weights."""
    cs, _ = _want(sc.IRT_CASES[0])
    rng = np.random.RandomState(5)
    theta = np.sort(rng.uniform(-5, 5, size=45)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=45) * np.exp(-0.5 * theta.astype(np.float64) ** 2)
    logw = np.log(w / w.sum()).astype(np.float32)
    ll = sc.irt_grid_loglik(cs["model"], theta[:, None], cs["params"], cs["Dc"], cs["y"])
    want = sc.grid_posterior(ll, logw, theta[:, None])
    got = _irt_engine(cs).score(nodes=(theta, logw))
    torch.cuda.synchronize()
    _hold("explicit nodes", got, want, IRT_NAMES)


def test_repeated_calls_and_row_subsets_give_the_same_bits():
    cs, _ = _want(sc.IRT_CASES[4])                                    # D = 2, 14 node tiles, 100 persons
    eng = _irt_engine(cs)
    one = eng.score(nodes=cs["nodes"])
    two = eng.score(nodes=cs["nodes"])
    idx = np.array([99, 3, 3, 64, 31, 32, 0, 98, 17, 5, 50, 63, 65, 3, 77, 12, 40, 41, 42, 96, 2, 1, 88, 70, 33, 34, 35,
                    36, 9, 8, 7, 66, 67, 68, 69, 20, 21], dtype=np.int64)
    assert len(idx) % 4 != 0 and len(idx) % 32 != 0 and len(np.unique(idx)) < len(idx)
    sub = eng.score(rows=torch.from_numpy(idx).to(_dev()), nodes=cs["nodes"])
    torch.cuda.synchronize()
    for k in ("eap", "psd", "loglik", "node"):
        assert torch.equal(one[k], two[k]), k
        assert torch.equal(sub[k], one[k][torch.from_numpy(idx).to(_dev())]), k
    cc, _ = _want(sc.CDM_CASES[1])
    ce = _ccdm_engine(cc)
    c1, c2 = ce.score(), ce.score(rows=idx)
    c3 = ce.score()
    torch.cuda.synchronize()
    for k in ("attr_prob", "pattern", "loglik"):
        assert torch.equal(c1[k], c3[k]), k
        assert torch.equal(c2[k], c1[k][torch.from_numpy(idx).to(_dev())]), k
    with pytest.raises(IndexError):
        eng.score(rows=np.array([0, 100]), nodes=cs["nodes"])


def test_a_waves_second_unit_starts_clean():
    """sc.second_unit_case: more persons than one launch has lanes for, so that two waves take a second unit.  The last 97 rows
    scored behind the others give the bits they give alone, and both hold to their oracle."""
    cs, want = sc.second_unit_case(torch.cuda.get_device_properties(_dev()).multi_processor_count)
    eng = _irt_engine(cs)
    full = eng.score(nodes=cs["nodes"], span=cs["span"])
    alone = eng.score(torch.from_numpy(cs["y_tail"]), nodes=cs["nodes"], span=cs["span"])
    torch.cuda.synchronize()
    assert full["loglik"].shape == (cs["N"],) and alone["loglik"].shape == (sc.SECOND_UNIT_TAIL,)
    tail = torch.from_numpy(cs["tail"]).to(_dev())
    behind = {k: v[tail] for k, v in full.items()}
    for k in ("eap", "psd", "loglik", "node"):
        assert torch.equal(behind[k], alone[k]), k
    _hold(cs["name"], behind, want, IRT_NAMES)
    empty = np.flatnonzero((cs["y_tail"] == 255).all(1))
    assert len(empty) == 8 and (np.abs(want["loglik"][empty]) < 1e-5).all() and (_np(behind["node"])[empty] == 2).all()


@pytest.mark.parametrize("cls,D", [("VIRT", 1), ("VaeIRT", 2)])
def test_score_between_two_fits_changes_nothing(cls, D):
    """fit(8), score(), fit(8) leaves the parameter bits of sixteen uninterrupted iterations from the same seed."""
    from vipsy_amd import vi
    rng = np.random.RandomState(9)
    y = (rng.uniform(size=(300, 24)) < 0.6).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.1] = 255

    def run(interrupt):
        vi.clear_param_store()
        m = getattr(vi, cls)(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=D, seed=7)
        opt = vi.Adam({"lr": 1e-2})
        if interrupt:
            m.fit(optim=opt, max_iter=8, progress=False)
            s = m.score(nodes=61 if D == 1 else 21)
            assert torch.isfinite(s["loglik"]).all()
            assert np.isfinite(m.marginal_loglik(nodes=61 if D == 1 else 21))
            m.fit(optim=opt, max_iter=8, progress=False)
        else:
            m.fit(optim=opt, max_iter=16, progress=False)
        torch.cuda.synchronize()
        eng = m.engine
        return eng.P.clone(), (eng.PP.clone() if eng.per_person else None), eng.M.clone(), eng.V.clone()

    a, b = run(True), run(False)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


def test_new_persons_on_a_padded_amortized_engine():
    """VaeIRT with hidden_dim 32 and 37 items runs on phantom items, dimensions and hidden units; scores of 50 respondents
    it has never seen go by its param() values alone."""
    from vipsy_amd import vi
    rng = np.random.RandomState(32)          # (a seed under which no new person's best two nodes tie within 1e-4 in float64)
    J, D = 37, 2
    y = (rng.uniform(size=(120, J)) < 0.5).astype(np.uint8)
    vi.clear_param_store()
    m = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=D, hidden_dim=32, subsample_size=60, seed=4)
    eng = m.engine
    assert (eng.J, eng.D, eng.H) == (40, 4, 64) and (eng.J_items, eng.D_model, eng.H_model) == (J, D, 32)
    a = rng.uniform(0.4, 1.0, size=(D, J)).astype(np.float32) * vo.default_a_free(D, J)
    b = rng.normal(size=(1, J)).astype(np.float32)
    eng.unconstrained("a").copy_(torch.from_numpy(a.astype(np.float32)).to(_dev()))
    eng.unconstrained("b").copy_(torch.from_numpy(b).to(_dev()))
    new = (rng.uniform(size=(50, J)) < 0.5).astype(np.float32)
    new[rng.uniform(size=new.shape) < 0.2] = np.nan                  # the reference's contract: float, NaN = missing
    got = m.score(data=torch.from_numpy(new), nodes=21)
    torch.cuda.synchronize()
    y_new = np.where(np.isnan(new), 255, new).astype(np.uint8)
    params = {"a": _np(vi.param("a")), "b": _np(vi.param("b"))}
    assert params["a"].shape == (D, J)
    cs = {"D": D, "nodes": 21, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "y": y_new, "params": params}
    want = sc.irt_oracle(cs)
    assert got["eap"].shape == (50, D)
    _hold("new persons, padded engine", got, want, IRT_NAMES)
    with pytest.raises(ValueError):
        m.score(data=torch.from_numpy(new[:, :36]))
    with pytest.raises(ValueError):
        m.score(data=torch.from_numpy(np.concatenate([new, new[:, :3]], 1)))


def test_vccdm_public_surface():
    from vipsy_amd import vi
    cs, want = _want(sc.CDM_CASES[0])
    vi.clear_param_store()
    data = cs["y"].astype(np.float32)
    data[cs["y"] == 255] = np.nan
    m = vi.VCCDM(data=torch.from_numpy(data).to(_dev()), q=torch.from_numpy(cs["q"]), model=cs["cdm"])
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    got = m.score()
    _hold("VCCDM.score", got, want, CDM_NAMES)
    ml = m.marginal_loglik()
    assert isinstance(ml, float)
    assert ml == pytest.approx(float(want["loglik"].sum()), rel=2e-5)
    # for this class the ELBO is the marginal likelihood: the full-batch loss of the step
    m.engine.loss_and_grads()
    torch.cuda.synchronize()
    loss = float(m.engine.G[m.engine.n_params].item())
    print("VCCDM: marginal_loglik %.6f, -loss %.6f, oracle %.6f" % (ml, -loss, float(want["loglik"].sum())))
    assert ml == pytest.approx(-loss / 1.0, rel=2e-5)                 # scale = N / N
    # new examinees through the public surface, u8 contract
    got2 = m.score(data=cs["y"][:37])
    torch.cuda.synchronize()
    for k in ("attr_prob", "pattern", "loglik"):
        assert torch.equal(got2[k], got[k][:37]), k
    with pytest.raises(ValueError):
        m.score(data=cs["y"][:, :29])


def test_classes_out_of_scope_refuse():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4)):
        with pytest.raises(NotImplementedError) as e:
            m.score()
        assert len(str(e.value)) > 20
        with pytest.raises(NotImplementedError):
            m.marginal_loglik()
    m = vi.VIRT(data=yd, model="irt_2pl", x_feature=2)
    with pytest.raises(ValueError):
        m.score(nodes=33)                                             # 33^2 > 1024 grid points


def test_oracle_comparisons_under_a_second_schedule():
    """Cases 1, 5 and 7 again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "scores_vs_oracle and (case1 or case5 or case7)"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
