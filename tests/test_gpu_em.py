"""fit_em on the GPU (vx_grid_mstep_irt / vx_grid_mstep_cdm behind IrtEngine / CcdmEngine.fit_em and the model classes' fit_em())
against the float64 oracle of tests/em_cases.py.

The rule is the project's ROW_TOL (3e-5, imported from tests/test_gpu_response_designs.py): IRT a and b absolutely, the CDM
parameters on the probability scale (an estimate of exactly 0 sits at the clamp, where unconstrained values are not comparable),
loglik[k] relatively.  It does not come from the kernel: the method said again in float32 numpy (tests/test_em_host.py) stays
below 1.2e-6 on these cases.  The errors found are printed.

Shapes: those of the score and count tests (ragged J and G, 1 to 32 node tiles = 1 to 12 nodes a lane, masked loadings in two and
three dimensions, 2 500 persons), a 1PL case of its own, J = 1 and G = 8; and for the step control of the M-step kernel the
synthetic launches of em_cases.STEP_CASES (sections 8 to 10): every Newton budget that tells a path apart, G = 64, 65, 961, 1 000
and 1 024 (1, 2 and 16 nodes a lane, ragged and full), tables times 2^10 and 2^20, the CDM closed form at K = 1 and K = 10 with
empty and one-sided classes, fit_em's stopping rule and `newton` other than 4.

Largest errors of the step-control launches on an MI355X, as parts of their rule, over all launches and budgets: items with a
finite maximiser 0.053 (1.6e-6 in a or b: step_2pl_easy_items, easy_steep, newton 2); constant 1PL items 0.007 of
ROW_TOL max(1, |b|) (step_1pl_dc1702, all_correct_cap3, newton 3).  Tables times 2^10 and 2^20 gave the bits of the unscaled
launches, so the same figures.  CDM closed form on synthetic tables: 6.5e-7 on the probability scale.  The figures launch by
launch are in docs/NOTEBOOK.md (the M-step's step control)."""
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



# ---- 8. the M-step's step control: cap, halving, clamp and stop paths (em_cases.STEP_CASES) ------------------------------
STEP_IDS = [c["name"] for c in ec.STEP_CASES]


def _step_launch(be, spec, newton, scale=1.0, start=None):
    """One launch of vx_grid_mstep_irt on all items of a STEP_CASES entry: (a [D][J] or None, b [1][J]) as float32 numpy."""
    c = ec.step_case(spec)
    two = spec["model"] != "irt_1pl"
    a0, b0 = (c["a0"], c["b0"]) if start is None else start
    a = _t(a0) if two else None
    b = _t(b0.reshape(-1))
    fr = _t(c["free"].astype(np.float32)) if two else None
    cfg = be.cfg(spec["model"], spec["D"], c["J"], 0, spec["Dc"], 1.0, 0, 0, 0)
    be.grid_mstep_irt(cfg, _t(c["theta"]), c["G"], _t(c["n1"] * np.float32(scale)), _t(c["n0"] * np.float32(scale)), fr, a, b, newton)
    torch.cuda.synchronize()
    return (_np(a).copy() if two else None), _np(b).reshape(1, -1).copy()


def _step_compare(spec, newton, a, b, tag):
    """The rule of the step-control comparisons (em_cases.step_errors at ROW_TOL) on one launch; masked loadings keep their bits."""
    c = ec.step_case(spec)
    a64, b64, _ = ec.step_run(spec, newton)
    assert np.isfinite(b).all() and (a is None or np.isfinite(a).all()), (tag, a, b)
    if a is not None:
        assert np.array_equal(a[~c["free"]].view(np.uint32), c["a0"][~c["free"]].view(np.uint32)), tag
    errs = ec.step_errors(spec, a, b, a64, b64, ROW_TOL)
    worst = {}
    for kind, e, name in zip(c["kinds"], errs, c["names"]):
        if e is not None:
            worst[kind] = max(worst.get(kind, (0.0, "")), (e, name))
    print("%s newton %d: %s" % (tag, newton, "  ".join("%s %.3f of the rule (%s)" % (k, v[0], v[1]) for k, v in sorted(worst.items()))))
    for e, name in zip(errs, c["names"]):
        assert e is None or e <= 1.0, (tag, newton, name, e)
    return worst


def _z32(spec, theta, a, b, j):
    """z of item j at every node in the kernel's float32 arithmetic (b, then the dimensions by fma; times Dc)."""
    sz = np.full(theta.shape[0], b[0, j], np.float32)
    for d in range(spec["D"]):
        sz = (theta[:, d].astype(np.float64) * np.float64(a[d, j]) + sz.astype(np.float64)).astype(np.float32)
    return np.float32(spec["Dc"]) * sz


@pytest.mark.parametrize("spec", ec.STEP_CASES, ids=STEP_IDS)
def test_step_control(spec):
    """Every launch of the entry, one a Newton budget (1 .. one past the last capped or halved step of the oracle, then 25, and
    64 where an item stops later), against the float64 oracle run with the same budget: ROW_TOL on a and b of an item with a
    finite maximiser, ROW_TOL max(1, |b|) on a constant 1PL item, which ends near +-23 or +-16 -- the rule and the margin of the
    method under it are those of tests/test_em_host.py::test_step_case_conditions, not the kernel's.  A constant 2PL item is
    held to the documented contract instead of values.

    Largest errors found on an MI355X, as parts of the rule: 0.053 (finite), 0.007 (constant 1PL); launch by launch in the
    table of docs/NOTEBOOK.md (the M-step's step control)."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    c = ec.step_case(spec)
    budgets = ec.step_budgets(spec)
    for newton in budgets:
        a, b = _step_launch(be, spec, newton)
        _step_compare(spec, newton, a, b, spec["name"])
    # the last launch again: the same bits
    a2, b2 = _step_launch(be, spec, budgets[-1])
    assert np.array_equal(b.view(np.uint32), b2.view(np.uint32)) and (a is None or np.array_equal(a.view(np.uint32), a2.view(np.uint32)))
    # the constant 2PL items: where the clamp holds at every node
    newton = budgets[-1]
    _, _, tr = ec.step_run(spec, newton)
    for j, kind in enumerate(c["kinds"]):
        if kind != "contract":
            continue
        assert tr[j]["stop"] == "pivot", (spec["name"], c["names"][j])            # (the oracle's item has stopped)
        z = _z32(spec, c["theta"], a, b, j)
        U = np.concatenate([np.ones((c["G"], 1)), c["theta"].astype(np.float64)], axis=1)
        n1, n0 = c["n1"][j].astype(np.float64), c["n0"][j].astype(np.float64)
        q0 = ec._item_eval(U, n1, n0, np.concatenate([c["b0"][:, j], c["a0"][:, j]]).astype(np.float64), spec["Dc"], ec.ZL)[0]
        q1 = ec._item_eval(U, n1, n0, np.concatenate([b[:, j], a[:, j]]).astype(np.float64), spec["Dc"], ec.ZL)[0]
        moved = max(abs(float(b[0, j]) - c["b0"][0, j]), float(np.abs(a[:, j] - c["a0"][:, j]).max()))
        print("%s %s: ends at a %s b %.4f (oracle a %s b %.4f), smallest |z| %.4f, Q %.3e -> %.3e, moved %.2f"
              % (spec["name"], c["names"][j], a[:, j], b[0, j], ec.step_run(spec, newton)[0][:, j], ec.step_run(spec, newton)[1][0, j],
                 np.abs(z).min(), q0, q1, moved))
        assert np.abs(z).min() >= np.float32(ec.ZL), (c["names"][j], np.abs(z).min())
        assert q1 >= q0 and moved <= ec.STEP_CAP * newton
    if "contract" in c["kinds"]:
        a3, b3 = _step_launch(be, spec, newton, start=(a, b))
        for j, kind in enumerate(c["kinds"]):
            if kind == "contract":
                assert b3[0, j].view(np.uint32) == b[0, j].view(np.uint32) and np.array_equal(a3[:, j].view(np.uint32), a[:, j].view(np.uint32))


@pytest.mark.parametrize("power", [10, 20])
@pytest.mark.parametrize("spec", ec.STEP_CASES, ids=STEP_IDS)
def test_step_control_scaled_tables(spec, power):
    """The same tables times 2^10 and 2^20 -- the sizes of a million persons and more: the oracle is scale-free, so the rule is
    the same; and with an even power of two every product, sum, pivot, square root and quotient of the kernel scales exactly
    and its acceptance rule is relative, so the bits are those of the unscaled launch."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    for newton in ec.step_budgets(spec):
        a1, b1 = _step_launch(be, spec, newton)
        a, b = _step_launch(be, spec, newton, scale=float(2 ** power))
        _step_compare(spec, newton, a, b, "%s x 2^%d" % (spec["name"], power))
        same = np.array_equal(b.view(np.uint32), b1.view(np.uint32)) and (a is None or np.array_equal(a.view(np.uint32), a1.view(np.uint32)))
        assert same, (spec["name"], power, newton, np.abs(b - b1).max(), None if a is None else np.abs(a - a1).max())


# ---- 9. the CDM closed form on synthetic tables --------------------------------------------------------------------------
def _cdm_synthetic(cdm, K, J, seed):
    """q, float32 tables and a start for J items: item 0 / 1 with R0 = 0 / W0 = 0, item 2 / 3 with W1 = 0 / R1 = 0 (where the
    item has an eta = 1 class), item 4 with no mass in its eta = 1 class, item 5 (where there is one) none in its eta = 0 class."""
    rng = np.random.RandomState(seed)
    q = np.zeros((K, J), np.float32)
    for j in range(J):                                                          # one, two, three attributes in turn
        q[[(j + d) % K for d in (0, 4, 7)[:1 + j % 3]], j] = 1
    eta, _ = (vo.dino_eta if cdm == "dino" else vo.dina_eta)(K, q.astype(np.float64))
    e1 = (eta > 0).T                                                            # [J][C]
    G = 1 << K
    n1 = (rng.uniform(0.5, 5.0, size=(J, G)) * 2000.0 / G).astype(np.float32)
    n0 = (rng.uniform(0.5, 5.0, size=(J, G)) * 2000.0 / G).astype(np.float32)
    n1[0, ~e1[0]] = 0
    n0[1, ~e1[1]] = 0
    n0[2, e1[2]] = 0
    n1[3, e1[3]] = 0
    n1[4, e1[4]] = 0
    n0[4, e1[4]] = 0
    if J > 5:
        n1[5, ~e1[5]] = 0
        n0[5, ~e1[5]] = 0
    g0 = (0.3 - 0.01 * np.arange(J)).astype(np.float32)
    s0 = (-0.2 + 0.01 * np.arange(J)).astype(np.float32)
    return q, e1, n1, n0, g0, s0


@pytest.mark.parametrize("power", [0, 20])
@pytest.mark.parametrize("cdm,K,J", [("dina", 1, 5), ("dino", 1, 5), ("dina", 10, 7), ("dino", 10, 7)],
                         ids=["dina_k1", "dino_k1", "dina_k10", "dino_k10"])
def test_cdm_closed_form_on_synthetic_tables(cdm, K, J, power):
    """K = 1 (two patterns) and K = 10 (1 024, 16 a lane); a class whose answers are all wrong or all correct ends on the bits of
    -+ZL, a class without mass keeps its bits; the rest at ROW_TOL on the probability scale, also with tables times 2^20."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    q, e1, n1, n0, g0, s0 = _cdm_synthetic(cdm, K, J, 5 + K)
    n1, n0 = n1 * np.float32(2 ** power), n0 * np.float32(2 ** power)
    g64, s64 = ec.cdm_mstep(cdm, K, q, n1.astype(np.float64), n0.astype(np.float64), g0, s0)
    g, s = _t(g0), _t(s0)
    cfg = be.hodina_cfg(K, J, 0, 1.0, 0, 0, 0)
    be.grid_mstep_cdm(cfg, cdm == "dino", _t(q), _t(n1), _t(n0), g, s)
    torch.cuda.synchronize()
    g, s = _np(g), _np(s)
    zl = np.float32(ec.ZL)
    seen = {"clamp": 0, "kept": 0}
    for name, got, want, start, cls in (("g", g, g64[0], g0, ~e1), ("s", s, s64[0], s0, e1)):
        mass = (n1 * cls).sum(1) + (n0 * cls).sum(1)
        for j in range(J):
            if not mass[j] > 0:
                assert got[j].view(np.uint32) == start[j].view(np.uint32), (name, j, got[j])
                seen["kept"] += 1
            elif abs(want[j]) == ec.ZL:
                assert got[j].view(np.uint32) == np.float32(np.sign(want[j]) * zl).view(np.uint32), (name, j, got[j], want[j])
                seen["clamp"] += 1
        err = float(np.abs(vo.sigmoid(got.astype(np.float64)) - vo.sigmoid(want)).max())
        print("%s K = %d x 2^%d: %s %.2e (rule %.1e)" % (cdm, K, power, name, err, ROW_TOL))
        assert err <= ROW_TOL, (name, err)
    assert seen["kept"] >= 1 and seen["clamp"] >= 2, seen
    if cdm == "dina":
        assert seen["clamp"] == 4 and seen["kept"] == (1 if J == 5 else 2), seen


# ---- 10. fit_em's loop: the stopping rule, and newton other than 4 -------------------------------------------------------
@pytest.mark.parametrize("case,tol", ec.CONVERGED, ids=[c[0][0] for c in ec.CONVERGED])
def test_converged(case, tol):
    cs, kind, ps, lks, _ = ec.trajectory(case, 8)
    n = ec.stop_iteration(lks, tol)
    m, _, _ = _model(case, cs, kind)
    out = m.fit_em(max_iter=20, tol=tol, **_grid_kw(cs, kind))
    assert out["converged"] is True and out["iterations"] == n and len(out["loglik"]) == n, (out, n)
    errs = _param_errors(m.engine, kind, ps[n])
    errs["loglik"] = max(abs(g - w) / abs(w) for g, w in zip(out["loglik"], lks))
    print("%s tol %.0e: stopped after %d; %s" % (cs["name"], tol, n, "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        assert e <= ROW_TOL, (cs["name"], k, e)
    m2, _, _ = _model(case, cs, kind)
    out2 = m2.fit_em(max_iter=20, tol=1e30, **_grid_kw(cs, kind))
    assert out2["converged"] is True and out2["iterations"] == 2 and len(out2["loglik"]) == 2
    assert max(_param_errors(m2.engine, kind, ps[2]).values()) <= ROW_TOL


@pytest.mark.parametrize("newton", [1, 8])
def test_newton_through_fit_em(newton):
    case = ec.IRT_EM[0]
    cs, kind, ps, lks, _ = ec.trajectory(case, 2, newton=newton)
    m, _, _ = _model(case, cs, kind)
    out = m.fit_em(max_iter=2, tol=0, newton=newton, **_grid_kw(cs, kind))
    assert out["iterations"] == 2 and out["converged"] is False
    errs = _param_errors(m.engine, kind, ps[2])
    errs["loglik"] = max(abs(g - w) / abs(w) for g, w in zip(out["loglik"], lks))
    print("%s newton %d: %s" % (cs["name"], newton, "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        assert e <= ROW_TOL, (cs["name"], newton, k, e)
