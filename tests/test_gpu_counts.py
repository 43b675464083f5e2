"""Expected counts and item fit on the GPU (vx_grid_counts behind IrtEngine / CcdmEngine.expected_counts, Engine.item_fit and
the model classes' expected_counts() / item_fit()) against the float64 oracle of tests/count_cases.py.

Engines are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views, nothing trained.
Every table is held to the oracle by the project's row rule, _row_errors(got, want, floor = 1) <= ROW_TOL (3e-5, imported
from tests/test_gpu_response_designs.py), one row = one item; mass as one row; prob, md and rmsd absolutely -- they are
proportions.  The bound does not come from the kernel: the same float32 + fp16-pair arithmetic said again in numpy
(tests/test_counts_host.py) stays at <= 3.4e-6 for the tables and <= 6.6e-7 for md / rmsd on exactly these cases.  The errors
found are printed.

Shapes: those of the score tests (ragged J and G, 32 item chunks, 1 to 32 node tiles, more item tiles than a wave holds at
once) and 2 500 persons (several rounds a workgroup, several slabs, a ragged last unit)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import count_cases as cc
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")

_WANT = {}


def _want(case):
    """The case and its oracle, computed once and shared (never modified)."""
    name = case if isinstance(case, str) else case[0]
    if name not in _WANT:
        if name == cc.MISFIT_NAME:
            cs = cc.misfit_case()
            _WANT[name] = (cs, cc.irt_oracle(cs))
        elif case in cc.IRT_CASES:
            cs = sc.irt_case(case)
            _WANT[name] = (cs, cc.irt_oracle(cs))
        else:
            cs = sc.cdm_case(case)
            _WANT[name] = (cs, cc.cdm_oracle(cs))
    return _WANT[name]


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _hold(tag, got, fit, want, y):
    """The row rule on the tables, the absolute rule on the proportions, the count identities; prints what it finds."""
    J, G = want["n1"].shape
    assert tuple(got["n1"].shape) == (J, G) and tuple(got["n0"].shape) == (J, G) and tuple(got["prob"].shape) == (J, G)
    assert tuple(got["mass"].shape) == (G,) and got["n1"].dtype == torch.float32 and got["prob"].dtype == torch.float32
    errs = {}
    for k in ("n1", "n0"):
        errs[k] = _row_errors(_f8(got[k]), want[k], floor=1.0)
    errs["mass"] = _row_errors(_f8(got["mass"])[None, :], want["mass"][None, :], floor=1.0)
    errs["prob"] = (float(np.abs(_f8(got["prob"]) - want["prob"]).max()), -1)
    for k in ("md", "rmsd"):
        g, w = _f8(fit[k]), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, k)
        errs[k] = (float(np.nanmax(np.abs(g - w))) if np.isfinite(w).any() else 0.0, -1)
    # observed = n1 / n, NaN exactly where the returned tables have n = 0 (a far node's mass may round to 0 in float32)
    n_got = _f8(got["n1"]) + _f8(got["n0"])
    obs = _f8(fit["observed"])
    assert obs.shape == (J, G) and np.array_equal(np.isnan(obs), n_got == 0), tag
    assert ((obs[n_got > 0] >= 0) & (obs[n_got > 0] <= 1)).all(), tag
    # the count identities on what the GPU returned
    for k, v in (("n1", 1), ("n0", 0)):
        cnt = (y == v).sum(0).astype(np.float64)
        errs["sum " + k] = (float((np.abs(_f8(got[k]).sum(1) - cnt) / np.maximum(cnt, 1.0)).max()), -1)
    cnt = (y != 255).sum(0).astype(np.float64)
    errs["n_obs"] = (float((np.abs(_f8(fit["n_obs"]) - cnt) / np.maximum(cnt, 1.0)).max()), -1)
    errs["sum mass"] = (abs(float(_f8(got["mass"]).sum()) - len(y)) / len(y), -1)
    print("%s: %s (rule: %.1e)" % (tag, "  ".join("%s %.2e" % (k, v[0]) for k, v in errs.items()), ROW_TOL))
    for k, (e, worst) in errs.items():
        assert e <= ROW_TOL, (tag, k, "item", worst, e)


@pytest.mark.parametrize("case", cc.IRT_CASES + [cc.MISFIT_NAME], ids=[c[0] for c in cc.IRT_CASES] + [cc.MISFIT_NAME])
def test_irt_counts_vs_oracle(case):
    cs, want = _want(case)
    eng = _irt_engine(cs)
    got = eng.expected_counts(nodes=cs["nodes"], span=cs["span"])
    fit = eng.item_fit(nodes=cs["nodes"], span=cs["span"])
    torch.cuda.synchronize()
    G = want["mass"].shape[0]
    assert tuple(got["theta"].shape) == (G, cs["D"]) and tuple(got["logw"].shape) == (G,)
    assert set(fit) == {"n_obs", "md", "rmsd", "observed", "prob"} and fit["md"].dtype == torch.float64
    _hold(cs["name"], got, fit, want, cs["y"])
    if cs["name"].startswith("case1"):
        # the person without a response adds exactly their prior to mass and nothing to the tables
        rest = np.delete(np.arange(cs["N"]), 5)
        sub = eng.expected_counts(rows=rest, nodes=cs["nodes"], span=cs["span"])
        prior = np.exp(want["logw"])
        d = _f8(got["mass"]) - _f8(sub["mass"])
        assert np.abs(d - prior).max() <= ROW_TOL
    if cs["name"] == cc.MISFIT_NAME:
        r = _f8(fit["rmsd"])
        assert int(r.argmax()) == cc.MISFIT_ITEM and r[cc.MISFIT_ITEM] > 3.0 * np.delete(r, cc.MISFIT_ITEM).max()


@pytest.mark.parametrize("case", cc.CDM_CASES, ids=[c[0] for c in cc.CDM_CASES])
def test_cdm_counts_vs_oracle(case):
    cs, want = _want(case)
    eng = _ccdm_engine(cs)
    got = eng.expected_counts()
    fit = eng.item_fit()
    torch.cuda.synchronize()
    assert tuple(got["patterns"].shape) == (1 << cs["K"], cs["K"])
    assert np.array_equal(_np(got["patterns"]), want["patterns"])
    _hold(cs["name"], got, fit, want, cs["y"])


def test_rows_subsets_single_persons_repeats_and_permutations():
    cs, want = _want(cc.COUNT_BIG)
    eng = _irt_engine(cs)
    rng = np.random.RandomState(4)
    idx = rng.choice(cs["N"], size=777, replace=False).astype(np.int64)          # three rounds and a ragged unit, one slab
    sub = eng.expected_counts(rows=torch.from_numpy(idx).to(_dev()))
    fit = eng.item_fit(rows=idx)
    torch.cuda.synchronize()
    _hold("rows: 777 of 2500", sub, fit, cc.irt_oracle(cs, rows=idx), cs["y"][idx])
    # one person: the tables are that person's posterior, on the rows of the items they answered
    for k in (0, 1234, 2499):
        one = eng.expected_counts(rows=[k])
        p = want["p"][k]
        yk = cs["y"][k]
        assert np.abs(_f8(one["mass"]) - p).max() <= ROW_TOL
        assert np.abs(_f8(one["n1"]) - np.outer(yk == 1, p)).max() <= ROW_TOL
        assert np.abs(_f8(one["n0"]) - np.outer(yk == 0, p)).max() <= ROW_TOL
        assert (_np(one["n1"])[yk != 1] == 0).all() and (_np(one["n0"])[yk != 0] == 0).all()
    # the same call twice: the same bits
    a, b = eng.expected_counts(), eng.expected_counts()
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass", "prob"):
        assert torch.equal(a[k], b[k]), k
    # a permutation of the rows changes the order of the sums: the row rule, not the bits
    perm = rng.permutation(cs["N"]).astype(np.int64)
    c = eng.expected_counts(rows=perm)
    torch.cuda.synchronize()
    for k in ("n1", "n0"):
        e, worst = _row_errors(_f8(c[k]), _f8(a[k]), floor=1.0)
        assert e <= ROW_TOL, (k, worst, e)
    e, _ = _row_errors(_f8(c["mass"])[None, :], _f8(a["mass"])[None, :], floor=1.0)
    assert e <= ROW_TOL
    with pytest.raises(IndexError):
        eng.expected_counts(rows=np.array([0, cs["N"]]))


def test_new_persons_on_a_padded_amortized_engine():
    """VaeIRT with hidden_dim 32 and 37 items runs on phantom items and dimensions; the tables of 50 respondents it has never
    seen have the real J rows and go by its param() values alone."""
    from vipsy_amd import vi
    rng = np.random.RandomState(32)
    J, D = 37, 2
    y = (rng.uniform(size=(120, J)) < 0.5).astype(np.uint8)
    vi.clear_param_store()
    m = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=D, hidden_dim=32, subsample_size=60, seed=4)
    eng = m.engine
    assert (eng.J, eng.D) == (40, 4) and (eng.J_items, eng.D_model) == (J, D)
    a = rng.uniform(0.4, 1.0, size=(D, J)).astype(np.float32) * vo.default_a_free(D, J)
    b = rng.normal(size=(1, J)).astype(np.float32)
    eng.unconstrained("a").copy_(torch.from_numpy(a.astype(np.float32)).to(_dev()))
    eng.unconstrained("b").copy_(torch.from_numpy(b).to(_dev()))
    new = (rng.uniform(size=(50, J)) < 0.5).astype(np.float32)
    new[rng.uniform(size=new.shape) < 0.2] = np.nan
    got = m.expected_counts(data=torch.from_numpy(new), nodes=21)
    fit = m.item_fit(data=torch.from_numpy(new), nodes=21)
    torch.cuda.synchronize()
    y_new = np.where(np.isnan(new), 255, new).astype(np.uint8)
    params = {"a": _np(vi.param("a")), "b": _np(vi.param("b"))}
    assert params["a"].shape == (D, J)
    cs = {"D": D, "nodes": 21, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "y": y_new, "params": params}
    assert tuple(got["n1"].shape) == (J, 21 * 21)
    _hold("new persons, padded engine", got, fit, cc.irt_oracle(cs), y_new)
    with pytest.raises(ValueError):
        m.expected_counts(data=torch.from_numpy(new[:, :36]))


def test_an_item_nobody_answered():
    """One column of case 1 set to 255: the item's rows of n1 / n0 are exactly zero, its md / rmsd NaN and its n_obs 0; the
    other items are held to the oracle as ever, and -- the item's table rows reach no person's likelihood -- moving its
    parameters changes no bit of any table or of any other item's statistics."""
    cs0 = sc.irt_case(sc.IRT_CASES[0])
    j = 11
    cs = dict(cs0)
    cs["y"] = cs0["y"].copy()
    cs["y"][:, j] = 255
    want = cc.irt_oracle(cs)
    assert np.isnan(want["md"][j]) and np.isnan(want["rmsd"][j]) and want["n_obs"][j] == 0
    eng = _irt_engine(cs)
    got, fit = eng.expected_counts(), eng.item_fit()
    torch.cuda.synchronize()
    _hold("case 1 without item %d" % j, got, fit, want, cs["y"])
    assert (_np(got["n1"])[j] == 0).all() and (_np(got["n0"])[j] == 0).all()
    assert np.isnan(_np(fit["md"])[j]) and np.isnan(_np(fit["rmsd"])[j]) and float(fit["n_obs"][j]) == 0.0
    assert np.isnan(_np(fit["observed"])[j]).all()
    others = np.delete(np.arange(cs["J"]), j)
    assert np.isfinite(_np(fit["md"])[others]).all() and np.isfinite(_np(fit["rmsd"])[others]).all()
    eng.unconstrained("a")[0, j] = 3.0
    eng.unconstrained("b")[0, j] = -2.0
    got2, fit2 = eng.expected_counts(), eng.item_fit()
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass"):
        assert torch.equal(got[k], got2[k]), k
    sel = torch.from_numpy(others).to(_dev())
    assert torch.equal(got["prob"][sel], got2["prob"][sel]) and not torch.equal(got["prob"][j], got2["prob"][j])
    for k in ("n_obs", "md", "rmsd", "observed"):
        assert torch.equal(fit[k][sel].nan_to_num(nan=-1.0), fit2[k][sel].nan_to_num(nan=-1.0)), k      # (observed has NaN cells)


def test_public_surface():
    from vipsy_amd import vi
    # VIRT.item_fit(): numpy, ready to print
    cs, want = _want(cc.COUNT_BIG)
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    fit = m.item_fit()
    J, G = cs["J"], 61
    assert set(fit) == {"n_obs", "md", "rmsd", "observed", "prob"}
    assert all(isinstance(v, np.ndarray) for v in fit.values())
    assert fit["n_obs"].shape == fit["md"].shape == fit["rmsd"].shape == (J,)
    assert fit["observed"].shape == fit["prob"].shape == (J, G)
    assert np.abs(fit["rmsd"] - want["rmsd"]).max() <= ROW_TOL and np.abs(fit["md"] - want["md"]).max() <= ROW_TOL
    # the misfit data through the same model: item 3 is named
    mis, mwant = _want(cc.MISFIT_NAME)
    data = mis["y"].astype(np.float32)
    data[mis["y"] == 255] = np.nan                                        # the reference's contract: float, NaN = missing
    r = m.item_fit(data=torch.from_numpy(data))["rmsd"]
    print("misfit through VIRT.item_fit: rmsd of item 3 %.4f, largest of the others %.4f" % (r[3], np.delete(r, 3).max()))
    assert int(np.argmax(r)) == cc.MISFIT_ITEM and r[cc.MISFIT_ITEM] > 3.0 * np.delete(r, cc.MISFIT_ITEM).max()
    assert np.abs(r - mwant["rmsd"]).max() <= ROW_TOL
    assert np.array_equal(m.item_fit(data=mis["y"])["rmsd"], r)           # uint8 with 255: the same bits
    with pytest.raises(ValueError):
        m.item_fit(data=mis["y"][:, :36])
    # VCCDM.expected_counts(): device tensors
    cd, cwant = _want(cc.CDM_CASES[0])
    vi.clear_param_store()
    c = vi.VCCDM(data=torch.from_numpy(cd["y"]).to(_dev()), q=torch.from_numpy(cd["q"]), model=cd["cdm"])
    for name, v in cd["params"].items():
        c.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    got = c.expected_counts()
    C = 1 << cd["K"]
    assert set(got) == {"n1", "n0", "mass", "prob", "patterns"} and all(torch.is_tensor(v) and v.is_cuda for v in got.values())
    assert tuple(got["n1"].shape) == (cd["J"], C) and tuple(got["mass"].shape) == (C,) and tuple(got["patterns"].shape) == (C, cd["K"])
    assert _row_errors(_f8(got["n1"]), cwant["n1"], floor=1.0)[0] <= ROW_TOL
    assert set(vi.VIRT.expected_counts(m)) == {"n1", "n0", "mass", "prob", "theta", "logw"}


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
            m.expected_counts()
        assert len(str(e.value)) > 20
        with pytest.raises(NotImplementedError):
            m.item_fit()


def test_counts_between_two_fits_change_nothing():
    """fit(8), expected_counts(), fit(8) leaves the parameter bits of sixteen uninterrupted iterations from the same seed."""
    from vipsy_amd import vi
    rng = np.random.RandomState(9)
    y = (rng.uniform(size=(300, 24)) < 0.6).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.1] = 255

    def run(interrupt):
        vi.clear_param_store()
        m = vi.VIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=1, seed=7)
        opt = vi.Adam({"lr": 1e-2})
        if interrupt:
            m.fit(optim=opt, max_iter=8, progress=False)
            c = m.expected_counts()
            assert torch.isfinite(c["n1"]).all() and abs(float(c["mass"].sum()) - 300.0) < 300.0 * ROW_TOL
            assert np.isfinite(m.item_fit()["rmsd"]).all()
            m.fit(optim=opt, max_iter=8, progress=False)
        else:
            m.fit(optim=opt, max_iter=16, progress=False)
        torch.cuda.synchronize()
        eng = m.engine
        return eng.P.clone(), (eng.PP.clone() if eng.per_person else None), eng.M.clone(), eng.V.clone()

    a, b = run(True), run(False)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


def test_oracle_comparisons_under_a_second_schedule():
    """Case 1 and the 2 500 persons (as simulated) again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "irt_counts_vs_oracle and (case1 or n2500) and not misfit"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "2 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
