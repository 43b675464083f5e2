"""fit_em on the GPU (vx_grid_mstep_irt / vx_grid_mstep_cdm behind IrtEngine / CcdmEngine.fit_em and the model classes' fit_em())
against the float64 oracle of tests/em_cases.py.

The rule is the project's ROW_TOL (3e-5, imported from tests/test_gpu_response_designs.py): IRT a and b absolutely, the CDM
parameters on the probability scale (an estimate of exactly 0 sits at the clamp, where unconstrained values are not comparable),
loglik[k] relatively.  It does not come from the kernel: the method said again in float32 numpy (tests/test_em_host.py) stays
below 1.2e-6 on these cases.  The errors found are printed.

Shapes: those of the score and count tests (ragged J and G, 1 to 32 node tiles = 1 to 12 nodes a lane, masked loadings in two and
three dimensions, 2 500 persons), a 1PL case of its own, J = 1 and G = 8."""
import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import em_cases as ec
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in ec.ALL_EM]


def _np(t):
    return t.detach().cpu().numpy()


def _t(v, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(v)).to(device=_dev(), dtype=dtype).contiguous()


def _model(case, cs=None, kind=None, cls=None, **kw):
    """A fresh model of the case at the case's start (em_cases.start_of): the engine's own initial values."""
    from vipsy_amd import vi
    if cs is None:
        cs, kind = ec.case_of(case)
    vi.clear_param_store()
    yd = torch.from_numpy(cs["y"]).to(_dev())
    if kind == "cdm":
        m = vi.VCCDM(data=yd, q=torch.from_numpy(cs["q"]), model=cs["cdm"], seed=3)
    else:
        if cs["D"] > 1:
            kw["a0"] = torch.full((cs["D"], cs["J"]), 0.5)
        m = (cls or vi.VIRT)(data=yd, model=cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=3, **kw)
    for name, v in ec.start_of(cs, kind).items():
        assert np.array_equal(_np(m.engine.unconstrained(name)), v), (cs["name"], name)
    return m, cs, kind


def _grid_kw(cs, kind):
    return {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}


def _param_errors(eng, kind, want, skip=()):
    """Largest |got - want| per parameter: IRT a, b as they are, CDM g, s on the probability scale."""
    errs = {}
    for name, w in want.items():
        g = _np(eng.unconstrained(name)).astype(np.float64)
        if kind == "cdm":
            g, w = vo.sigmoid(g), vo.sigmoid(w)
        d = np.abs(g - w)
        if len(skip):
            d = np.delete(d, list(skip), axis=1)
        errs[name] = float(d.max())
    return errs


def _monotone(tag, lks, after):
    for k in range(len(lks) - 1):
        assert lks[k + 1] >= lks[k] - 1e-6 * abs(lks[k]), (tag, k, lks)
    assert after >= lks[-1] - 1e-6 * abs(lks[-1]), (tag, after, lks)


# ---- 1. the M-step alone, through the ABI --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.IRT_EM, ids=[c[0] for c in ec.IRT_EM])
def test_irt_mstep_alone(case):
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    cs, kind = ec.case_of(case)
    theta, _ = ec.grid_of(cs)
    start, free = ec.start_of(cs, kind), ec.a_free_of(cs)
    n1, n0, _ = ec.irt_estep(cs, start)
    n1, n0 = n1.astype(np.float32), n0.astype(np.float32)                       # what the kernel is fed: the oracle is too
    a64, b64 = ec.newton_mstep(cs["model"], theta, cs["Dc"], n1, n0, start.get("a"), start["b"], free, 25)
    J, G, D = cs["J"], theta.shape[0], cs["D"]
    two = cs["model"] != "irt_1pl"
    a = _t(start["a"]) if two else None
    b = _t(start["b"].reshape(-1))
    fr = _t(free.astype(np.float32)) if (two and D > 1) else None              # one dimension: NULL = all free
    cfg = be.cfg(cs["model"], D, J, 0, cs["Dc"], 1.0, 0, 0, 0)
    be.grid_mstep_irt(cfg, _t(theta), G, _t(n1), _t(n0), fr, a, b, 25)
    torch.cuda.synchronize()
    errs = {"b": float(np.abs(_np(b).astype(np.float64) - b64[0]).max())}
    if two:
        got = _np(a)
        errs["a"] = float(np.abs(got.astype(np.float64) - a64).max())
        assert np.array_equal(got[~free].view(np.uint32), start["a"][~free].view(np.uint32))      # masked loadings keep their bits
    print("%s M-step alone: %s (rule %.1e)" % (cs["name"], "  ".join("%s %.2e" % kv for kv in sorted(errs.items())), ROW_TOL))
    for k, e in errs.items():
        assert e <= ROW_TOL, (cs["name"], k, e)


@pytest.mark.parametrize("case", ec.CDM_EM, ids=[c[0] for c in ec.CDM_EM])
def test_cdm_mstep_alone(case):
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    cs, kind = ec.case_of(case)
    start = ec.start_of(cs, kind)
    n1, n0, _ = ec.cdm_estep(cs, start)
    n1, n0 = n1.astype(np.float32), n0.astype(np.float32)
    g64, s64 = ec.cdm_mstep(cs["cdm"], cs["K"], cs["q"], n1.astype(np.float64), n0.astype(np.float64), start["g"], start["s"])
    cfg = be.hodina_cfg(cs["K"], cs["J"], 0, 1.0, 0, 0, 0)
    for J in (cs["J"], 1):                                                      # (J = 1: the first item alone)
        g, s = _t(start["g"].reshape(-1)[:J]), _t(start["s"].reshape(-1)[:J])
        cfg.J = J
        be.grid_mstep_cdm(cfg, cs["cdm"] == "dino", _t(cs["q"][:, :J]), _t(n1[:J]), _t(n0[:J]), g, s)
        torch.cuda.synchronize()
        eg = float(np.abs(vo.sigmoid(_np(g).astype(np.float64)) - vo.sigmoid(g64[0, :J])).max())
        es = float(np.abs(vo.sigmoid(_np(s).astype(np.float64)) - vo.sigmoid(s64[0, :J])).max())
        print("%s M-step alone, J = %d: g %.2e  s %.2e (rule %.1e)" % (cs["name"], J, eg, es, ROW_TOL))
        assert eg <= ROW_TOL and es <= ROW_TOL
        assert np.isfinite(_np(g)).all() and np.isfinite(_np(s)).all()
        if cs["cdm"] == "dino":
            single = (cs["q"][:, :J].sum(0) == 1)
            assert single.any()
            assert np.array_equal(_np(s)[single].view(np.uint32), start["s"].reshape(-1)[:J][single].view(np.uint32))


def test_irt_mstep_one_item_eight_nodes():
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    rng = np.random.RandomState(7)
    theta = np.linspace(-2.0, 2.0, 8).astype(np.float32)[:, None]
    n1 = (rng.uniform(1.0, 5.0, size=(1, 8)) * vo.sigmoid(1.3 * theta[:, 0] - 0.4)).astype(np.float32)
    n0 = (rng.uniform(1.0, 5.0, size=(1, 8)) * vo.sigmoid(-1.3 * theta[:, 0] + 0.4)).astype(np.float32)
    a0, b0 = np.ones((1, 1), np.float32), np.zeros((1, 1), np.float32)
    a64, b64 = ec.newton_mstep("irt_2pl", theta, 1.0, n1, n0, a0, b0, np.ones((1, 1), bool), 25)
    a, b = _t(a0), _t(b0.reshape(-1))
    be.grid_mstep_irt(be.cfg("irt_2pl", 1, 1, 0, 1.0, 1.0, 0, 0, 0), _t(theta), 8, _t(n1), _t(n0), None, a, b, 25)
    torch.cuda.synchronize()
    ea, eb = abs(float(a[0, 0]) - a64[0, 0]), abs(float(b[0]) - b64[0, 0])
    print("J = 1, G = 8: a %.2e  b %.2e" % (ea, eb))
    assert ea <= ROW_TOL and eb <= ROW_TOL


# ---- 2. one and four EM iterations against the oracle's trajectory -------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 4])
@pytest.mark.parametrize("case", ec.ALL_EM, ids=IDS)
def test_em_iterations_vs_oracle(case, iters):
    cs, kind, ps, lks, _ = ec.trajectory(case, iters)
    m, _, _ = _model(case, cs, kind)
    out = m.fit_em(max_iter=iters, tol=0, **_grid_kw(cs, kind))
    torch.cuda.synchronize()
    assert out["iterations"] == iters and len(out["loglik"]) == iters and all(isinstance(v, float) for v in out["loglik"])
    assert out["converged"] is False
    errs = _param_errors(m.engine, kind, ps[iters])
    errs["loglik"] = max(abs(g - w) / abs(w) for g, w in zip(out["loglik"], lks))
    print("%s after %d: %s (rule %.1e)" % (cs["name"], iters, "  ".join("%s %.2e" % kv for kv in sorted(errs.items())), ROW_TOL))
    for k, e in errs.items():
        assert e <= ROW_TOL, (cs["name"], iters, k, e)


# ---- 3. the marginal log-likelihood does not fall ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.ALL_EM, ids=IDS)
def test_loglik_is_monotone(case):
    m, cs, kind = _model(case)
    out = m.fit_em(max_iter=6, tol=0, **_grid_kw(cs, kind))
    after = m.marginal_loglik(**_grid_kw(cs, kind))
    print(cs["name"], ["%.6f" % v for v in out["loglik"]], "%.6f" % after)
    assert len(out["loglik"]) >= 2
    _monotone(cs["name"], out["loglik"], after)


# ---- 4. bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ec.IRT_EM[0], ec.IRT_EM[2], ec.ONEPL, ec.CDM_EM[2]], ids=lambda c: c[0])
def test_bits(case):
    runs = []
    for _ in range(2):
        m, cs, kind = _model(case)
        before = m.marginal_loglik(**_grid_kw(cs, kind))
        out = m.fit_em(max_iter=3, tol=0, **_grid_kw(cs, kind))
        assert out["loglik"][0] == before, (cs["name"], out["loglik"][0], before)
        runs.append((out["loglik"], {n: _np(m.engine.unconstrained(n)).copy() for n in ec.start_of(cs, kind)}))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert np.array_equal(runs[0][1][n].view(np.uint32), runs[1][1][n].view(np.uint32)), (cs["name"], n)


# ---- 5. designs: an item nobody answered, an item whose answers are all equal --------------------------------------------
def test_designs():
    cs = ec.design_case()
    m, _, kind = _model(None, cs, "irt")
    eng = m.engine
    ju, jc = ec.DESIGN_UNANSWERED, ec.DESIGN_CONSTANT
    a0, b0 = _np(eng.unconstrained("a")).copy(), _np(eng.unconstrained("b")).copy()
    p = {k: v.astype(np.float64) for k, v in ec.start_of(cs, kind).items()}
    want_lk = []
    for _ in range(4):
        p, lk = ec.em_iteration(cs, kind, p)
        want_lk.append(lk)
    out = m.fit_em(max_iter=4, tol=0, **_grid_kw(cs, kind))
    a1, b1 = _np(eng.unconstrained("a")), _np(eng.unconstrained("b"))
    assert a1[0, ju].view(np.uint32) == a0[0, ju].view(np.uint32) and b1[0, ju].view(np.uint32) == b0[0, ju].view(np.uint32)
    assert np.isfinite(a1).all() and np.isfinite(b1).all()
    errs = _param_errors(eng, kind, p, skip=(ju, jc))
    errs["loglik"] = max(abs(g - w) / abs(w) for g, w in zip(out["loglik"], want_lk))
    print("%s after 4: %s; the constant item ends at a %.4f b %.4f (oracle %.4f %.4f)"
          % (cs["name"], "  ".join("%s %.2e" % kv for kv in sorted(errs.items())), a1[0, jc], b1[0, jc], p["a"][0, jc], p["b"][0, jc]))
    for k, e in errs.items():
        assert e <= ROW_TOL, (k, e)
    m2, _, _ = _model(None, cs, "irt")
    out6 = m2.fit_em(max_iter=6, tol=0, **_grid_kw(cs, kind))
    assert np.isfinite(_np(m2.engine.unconstrained("a"))).all() and np.isfinite(_np(m2.engine.unconstrained("b"))).all()
    _monotone(cs["name"], out6["loglik"], m2.marginal_loglik(**_grid_kw(cs, kind)))


# ---- 6. nothing else moved -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amortized", [True, False], ids=["VaeIRT", "VIRT"])
def test_nothing_else_moved(amortized):
    from vipsy_amd import vi
    m, cs, kind = _model(ec.IRT_EM[0], cls=vi.VaeIRT if amortized else vi.VIRT)
    eng = m.engine
    if amortized:
        assert eng.J == 40 and eng.J_items == 37                               # the padded engine: three phantom items
    keep = torch.ones(eng.n_params, dtype=torch.bool, device=eng.dev)
    for name in ("a", "b"):
        o = eng.off[name]
        keep[o:o + eng.J_items] = False                                        # (D = 1: the own items lead each segment)
    state = {"P": eng.P.clone(), "M": eng.M.clone(), "V": eng.V.clone(), "G": eng.G.clone()}
    if eng.per_person:
        state.update({"PP": eng.PP.clone(), "MP": eng.MP.clone(), "VP": eng.VP.clone()})
    t0 = eng.t
    m.fit_em(max_iter=2, tol=0, **_grid_kw(cs, kind))
    torch.cuda.synchronize()
    assert eng.t == t0
    assert torch.equal(eng.P[keep], state["P"][keep]) and not torch.equal(eng.P[~keep], state["P"][~keep])
    for k in state:
        if k != "P":
            assert torch.equal(getattr(eng, k), state[k]), k


def test_fit_then_fit_em_then_step():
    from vipsy_amd import vi
    from vipsy_amd.engine import LrSpec
    m, cs, kind = _model(ec.IRT_EM[0])
    m.fit(max_iter=8, progress=False)
    out = m.fit_em(max_iter=2, **_grid_kw(cs, kind))
    assert len(out["loglik"]) == 2 and np.isfinite(out["loglik"]).all()
    m.fit(max_iter=2, progress=False)
    for cls in (vi.VIRT, vi.VaeIRT):
        # A refits; B, built from the same data and seed, is handed A's refit values: their next steps agree to the bit
        A, _, _ = _model(ec.IRT_EM[0], cls=cls)
        A.fit_em(max_iter=3, tol=0, **_grid_kw(cs, kind))
        vals = {n: A.engine.unconstrained(n).clone() for n in ("a", "b")}
        loss_a = float(A.engine.step(LrSpec(1e-2)))
        B, _, _ = _model(ec.IRT_EM[0], cls=cls)
        for n, v in vals.items():
            B.engine.unconstrained(n).copy_(v)
        loss_b = float(B.engine.step(LrSpec(1e-2)))
        assert loss_a == loss_b, (cls.__name__, loss_a, loss_b)
        assert torch.equal(A.engine.P, B.engine.P)


# ---- 7. the guide plays no part ------------------------------------------------------------------------------------------
def test_vaeirt_gives_the_bits_of_virt():
    from vipsy_amd import vi
    res = []
    for cls in (vi.VIRT, vi.VaeIRT):
        m, cs, kind = _model(ec.IRT_EM[0], cls=cls)
        out = m.fit_em(max_iter=2, tol=0, **_grid_kw(cs, kind))
        res.append((out["loglik"], _np(m.engine.unconstrained("a")).copy(), _np(m.engine.unconstrained("b")).copy()))
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))
    assert np.array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))

