"""vx_grid_mstep_irt_map and fit_em(prior=) on the GPU against the float64 oracle of tests/map_cases.py.

Every rule is path-independent: none follows the kernel's accept / reject decisions.
  1. Maximum reached (one launch, newton = 64, from within 0.5 of the generating values): the float64 maximiser started AT the
     kernel's output gains at most C_Q 1e-6 |Q_j|, and every unknown is within sqrt(2 C_Q 1e-6 |Q_j| (H^-1)_kk) of its end point.
  2. One step (newton = 1, from a start where the float64 step is accepted by 100 tolerances -- tests/test_map_host.py): the
     output is the float64 one-step result to C_STEP eps32 |H^-1| S.
  3. Exact statements: the same bits twice, item j alone gives its bits of the full launch, what is fixed keeps its bits,
     lprior is the float64 log prior at the incoming parameters to float32 rounding, and precision 0 everywhere on the 2PL
     case agrees with vx_grid_mstep_irt -- in a and b to the bit, on the 1PL case and at D = 2 and 3 too.
  4. End to end: fit_em(prior=) on the 3PL and the 4PL case, on the 1PL case, and at x_feature = 2 (4PL) and 3 (2PL, its prior
     on a given entry by entry) with the engine's own triangular mask.
The step control from far starts and the exact promises of the kernel's header: tests/test_gpu_map_paths.py.
C_Q = 16 and C_STEP = 32 are reasoned in tests/map_cases.py; the method alone (float32 numpy) meets both at half.  Largest
ratios on an MI355X are printed by the tests and recorded in DESIGN.md section 6."""
import numpy as np
import pytest
import torch

from tests import map_cases as mc
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL

pytestmark = pytest.mark.gpu

NAMES = list(mc.CASES)


def _np(t):
    return t.detach().cpu().numpy()


def _t(v, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(v)).to(device=_dev(), dtype=dtype).contiguous()


def _launch(cs, L, p0, newton, prior=None, items=None, lprior=False, a_free="case"):
    """One launch on the items `items` (default all) of a case from p0 [6][J]: (p [6][J'] float32, lprior [J'] or None).
    a_free: the case's mask, or a [D][J] array, or None (the NULL pointer: every loading free)."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    sel = np.arange(cs["J"]) if items is None else np.asarray(items)
    m, D, J = mc.MODEL_NO[cs["model"]], cs["D"], len(sel)
    p0 = np.asarray(p0, np.float32)[:, sel]
    pr = np.ascontiguousarray(np.asarray(L["prior"] if prior is None else prior, np.float32)[:, :, sel])
    a = _t(p0[1:1 + D]) if m >= 2 else None
    mask = cs["a_free"] if isinstance(a_free, str) else a_free
    fr = _t(np.asarray(mask)[:, sel].astype(np.float32)) if m >= 2 and mask is not None else None
    b, c, d = _t(p0[0]), (_t(p0[4]) if m >= 3 else None), (_t(p0[5]) if m == 4 else None)
    lp = torch.full((J,), float("nan"), device=_dev()) if lprior else None
    cfg = be.cfg(cs["model"], D, J, 0, cs["Dc"], 1.0, 0, 0, 0)
    be.grid_mstep_irt_map(cfg, _t(cs["theta"]), cs["G"], _t(L["n1"][sel]), _t(L["n0"][sel]), fr, a, b, c, d, _t(pr), newton, lp)
    torch.cuda.synchronize()
    p = p0.copy()
    p[0] = _np(b)
    if m >= 2:
        p[1:1 + D] = _np(a)
    if m >= 3:
        p[4] = _np(c)
    if m == 4:
        p[5] = _np(d)
    return p, (None if lp is None else _np(lp))


_RUN = {}


def _full(name):
    """The case's launch of 64 steps from its start, run once and shared (never modified)."""
    if name not in _RUN:
        cs, L = mc.case(name), mc.launch(name)
        _RUN[name] = _launch(cs, L, L["p0"], 64, lprior=True)
    return _RUN[name]


# ---- 1. maximum reached --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_maximum_reached(name):
    cs, L = mc.case(name), mc.launch(name)
    p, _ = _full(name)
    assert np.isfinite(p).all()
    gain, dev, last = mc.rule1(cs, L, p)
    print("%s: the oracle gains at most %.3g of 1e-6 |Q_j| (C_Q = %g); parameters at most %.3g of their bound"
          % (name, gain.max(), mc.C_Q, dev.max()))
    assert last <= 1e-6
    assert gain.max() <= mc.C_Q, (name, gain)
    assert dev.max() <= 1.0, (name, dev)


# ---- 2. one step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_one_step(name):
    cs, L = mc.case(name), mc.launch(name)
    p, _ = _launch(cs, L, L["p0_near"], 1)
    ratio, p64, _ = mc.rule2(cs, L, p)
    print("%s: one step at most %.3g of eps32 |H^-1| S (C_STEP = %g)" % (name, ratio.max(), mc.C_STEP))
    assert ratio.max() <= mc.C_STEP, (name, ratio)


# ---- 3. exact statements -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bits(name):
    """The same call gives the same bits; an item alone (tables of one row) gives its bits of the full launch; the unanswered
    item, the masked loadings and the rows the model does not have keep their bits."""
    cs, L = mc.case(name), mc.launch(name)
    p, lp = _full(name)
    p2, lp2 = _launch(cs, L, L["p0"], 64, lprior=True)
    assert p.tobytes() == p2.tobytes() and lp.tobytes() == lp2.tobytes()
    for j in range(cs["J"]):
        pj, lpj = _launch(cs, L, L["p0"], 64, items=[j], lprior=True)
        assert pj[:, 0].tobytes() == p[:, j].tobytes() and lpj[0].tobytes() == lp[j].tobytes(), (name, j)
    assert p[:, mc.UNANSWERED].tobytes() == L["p0"][:, mc.UNANSWERED].tobytes()
    assert p[~L["free"]].tobytes() == L["p0"][~L["free"]].tobytes()
    moved = L["free"] & mc.answered(L)[None, :]
    assert (p[moved] != L["p0"][moved]).all()


@pytest.mark.parametrize("name", NAMES)
def test_lprior_is_the_log_prior_of_the_incoming_parameters(name):
    cs, L = mc.case(name), mc.launch(name)
    _, lp = _full(name)
    p0, pr = L["p0"].astype(np.float64), L["prior"].astype(np.float64)
    want = mc.log_prior(p0, L["free"], pr)
    tol = 8 * mc.EPS32 * np.abs(want) + 1e-30                         # at most six terms of three roundings each
    assert np.isfinite(lp).all() and lp.shape == (cs["J"],)
    assert (np.abs(lp.astype(np.float64) - want) <= tol).all(), (name, lp, want)
    assert want[-1] < 0 and (want[mc.UNANSWERED] < 0) == bool((pr[1, :, mc.UNANSWERED] * L["free"][:, mc.UNANSWERED]).any())
    if mc.MODEL_NO[cs["model"]] >= 3:
        assert want[mc.UNANSWERED] < 0                                  # the unanswered item reports its term too


def test_precision_zero_agrees_with_the_unpenalised_entry():
    """The 2PL case without its constant item (no prior: no finite maximum), every precision 0: both entries reach the maximum
    of the same Q_j under rule 1, so they are within twice its bound of each other."""
    from vipsy_amd.engine import HipBackend
    name = "map4_2pl_j8_g61"
    cs, L = mc.case(name), mc.launch(name)
    sel = np.arange(cs["J"] - 1)
    zero = np.zeros_like(L["prior"])
    p, _ = _launch(cs, L, L["p0"], 64, prior=zero, items=sel)
    be = HipBackend()
    a, b = _t(L["p0"][1:2, sel]), _t(L["p0"][0, sel])
    be.grid_mstep_irt(be.cfg(cs["model"], 1, len(sel), 0, cs["Dc"], 1.0, 0, 0, 0), _t(cs["theta"]), cs["G"], _t(L["n1"][sel]),
                      _t(L["n0"][sel]), None, a, b, 64)
    torch.cuda.synchronize()
    q = p.copy()
    q[0], q[1] = _np(b), _np(a)[0]
    sub = dict(cs, J=len(sel), a_free=cs["a_free"][:, sel])
    Ls = {"n1": L["n1"][sel], "n0": L["n0"][sel], "free": L["free"][:, sel], "prior": zero[:, :, sel]}
    for tag, out in (("vx_grid_mstep_irt_map", p), ("vx_grid_mstep_irt", q)):
        gain, dev, last = mc.rule1(sub, Ls, out)
        print("%s, precision 0: gain at most %.3g, parameters at most %.3g" % (tag, gain.max(), dev.max()))
        assert last <= 1e-6 and gain.max() <= mc.C_Q and dev.max() <= 1.0, (tag, gain, dev)
    assert p[:, mc.UNANSWERED].tobytes() == q[:, mc.UNANSWERED].tobytes()


# map_cases has no 2PL case at D = 2: the 3PL D = 2 case's tables, grid, mask and start, launched as a 2PL (c_un is not passed)
ZERO_PRECISION = [("map4_2pl_j8_g61", None), ("map7_1pl_j7_g61", None), ("map3_3pl_d2_j7_g441", "irt_2pl"),
                  ("map9_2pl_d3_j7_g343", None)]


@pytest.mark.parametrize("name,model", ZERO_PRECISION, ids=["2pl_d1", "1pl", "2pl_d2", "2pl_d3"])
def test_precision_zero_gives_the_bits_of_the_unpenalised_entry(name, model):
    """Every precision 0 with finite means (the case's own), the same start, the constant item left out: both entries are one
    kernel, and what a prior adds to it is then nothing -- the penalty and its gradient term are products with 0, adding +-0 to
    a float that is not zero changes no bit of it, and a step of zero leaves p where it was.  a and b come back the same bytes."""
    from vipsy_amd.engine import HipBackend
    cs, L = mc.case(name), mc.launch(name)
    if model is not None:
        cs = dict(cs, model=model)
    sel = np.arange(cs["J"] - 1)
    D, two = cs["D"], cs["model"] != "irt_1pl"
    pr = L["prior"].copy()
    pr[1] = 0
    assert np.isfinite(pr[0]).all()
    p, _ = _launch(cs, L, L["p0"], 64, prior=pr, items=sel)
    be = HipBackend()
    a, b = (_t(L["p0"][1:1 + D, sel]) if two else None), _t(L["p0"][0, sel])
    fr = _t(cs["a_free"][:, sel].astype(np.float32)) if two else None
    be.grid_mstep_irt(be.cfg(cs["model"], D, len(sel), 0, cs["Dc"], 1.0, 0, 0, 0), _t(cs["theta"]), cs["G"], _t(L["n1"][sel]),
                      _t(L["n0"][sel]), fr, a, b, 64)
    torch.cuda.synchronize()
    assert p[0].tobytes() == _np(b).tobytes()
    if two:
        assert p[1:1 + D].tobytes() == _np(a).tobytes()
    moved = L["free"][:1 + D, sel] & mc.answered(L)[None, sel]
    assert (p[:1 + D][moved] != L["p0"][:1 + D, sel][moved]).all()     # (both moved: the same bytes are not the start's)


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
def _model(name, cls=None, items=None):
    from vipsy_amd import vi
    cs = mc.case(name)
    vi.clear_param_store()
    y = cs["y"] if items is None else np.ascontiguousarray(cs["y"][:, :items])
    m = (cls or vi.VIRT)(data=torch.from_numpy(y).to(_dev()), model=cs["model"], x_feature=cs["D"], D=cs["Dc"], seed=3)
    if cs["a_free"] is not None and items is None:                       # (the engine's own mask is the case's)
        assert np.array_equal(_np(m.engine.unconstrained("a", m.engine.free)) != 0, cs["a_free"])
    for k, v in mc.em_start(cs).items():
        m.engine.unconstrained(k).copy_(_t(v[:, :y.shape[1]]))
    return m, cs


def _kw(cs):
    return dict(prior=mc.em_prior_of(cs), nodes=cs["nodes"], span=cs["span"])


_FIT = {}


def _fit25(name):
    if name not in _FIT:
        m, cs = _model(name)
        before = m.marginal_loglik(nodes=cs["nodes"], span=cs["span"])
        out = m.fit_em(max_iter=25, tol=-1.0, **_kw(cs))               # (never converged: late rises are below float32's ulp)
        torch.cuda.synchronize()
        _FIT[name] = (before, out, {k: _np(m.engine.unconstrained(k)).copy() for k in mc.em_start(cs)})
    return _FIT[name]


@pytest.mark.parametrize("name", mc.EM_CASES)
def test_fit_em_logpost(name):
    cs = mc.case(name)
    before, out, _ = _fit25(name)
    _, lks, lps, _ = mc.trajectory(name, 25)
    assert sorted(out) == ["converged", "iterations", "loglik", "logpost"] and out["iterations"] == 25 and not out["converged"]
    assert out["loglik"][0] == before                                   # bit for bit what marginal_loglik() gave
    lp = out["logpost"]
    for k in range(24):
        assert lp[k + 1] >= lp[k] - 1e-6 * abs(lp[k]), (name, k, lp)
    err = max(abs(g - w) / abs(w) for g, w in zip(lp, lps))
    errl = max(abs(g - w) / abs(w) for g, w in zip(out["loglik"], lks))
    print("%s: logpost %.4f -> %.4f; against the oracle logpost %.2e loglik %.2e (rule %.1e)" % (name, lp[0], lp[-1], err, errl, ROW_TOL))
    assert err <= ROW_TOL and errl <= ROW_TOL
    assert lp[-1] < out["loglik"][-1]                                   # (a log prior of normals, constants dropped, is <= 0)


@pytest.mark.parametrize("name", mc.EM_CASES)
def test_fit_em_three_iterations_vs_the_oracle(name):
    """Rule 1's bound an unknown, at the oracle's parameters, widened by ROW_TOL -- the absolute rule tests/test_gpu_em.py holds
    the trajectories of the unpenalised EM to (the E-step's tables and float32 leaves)."""
    m, cs = _model(name)
    out = m.fit_em(max_iter=3, tol=0, **_kw(cs))
    ps, _, _, _ = mc.trajectory(name, 3)
    sd, qs = mc.posterior_sd(cs, ps[3])
    worst = 0.0
    for k, w in ps[3].items():
        tol = np.sqrt(2 * mc.C_Q * mc.QTOL * qs[None, :]) * sd[k] + ROW_TOL
        r = np.abs(_np(m.engine.unconstrained(k)).astype(np.float64) - w) / tol
        worst = max(worst, float(np.nanmax(r)))
        assert not (r > 1).any(), (name, k, r)
    print("%s after 3 iterations: at most %.3g of the bound" % (name, worst))
    assert out["iterations"] == 3


@pytest.mark.parametrize("name", mc.EM_CASES)
def test_fit_em_ends_where_the_oracle_ends(name):
    """c, d and a (and b) after 25 iterations against the ORACLE's 25 iterations, not the truth: within a hundredth of the
    unknown's own posterior standard deviation sqrt((H^-1)_kk) -- the same fit to any reader of it (tests/test_map_host.py:
    rounding alone moves the end by 1e-4 of one at most)."""
    cs = mc.case(name)
    _, _, got = _fit25(name)
    ps, _, _, _ = mc.trajectory(name, 25)
    sd, _ = mc.posterior_sd(cs, ps[25])
    for k, w in ps[25].items():
        r = np.abs(got[k].astype(np.float64) - w) / sd[k]
        print("%s %s: at most %.2e posterior sd from the oracle's end" % (name, k, np.nanmax(r)))
        assert np.nanmax(r) <= 1e-2, (name, k, r)
        assert got[k][:, mc.UNANSWERED].tobytes() == mc.em_start(cs)[k][:, mc.UNANSWERED].tobytes()
    assert np.all(np.isfinite(np.concatenate([v.reshape(-1) for v in got.values()])))


def _model_2pl_d2():
    """Thirteen items of the 3PL case's responses under a VaeIRT 2PL with x_feature = 2: a padded engine, in whose `a` segment
    phantom items lie between the two rows of own loadings: the own items do NOT lead it."""
    from vipsy_amd import vi
    cs = mc.case("map1_3pl_j14_g41")
    vi.clear_param_store()
    y = np.ascontiguousarray(cs["y"][:, :13])
    m = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=2, D=cs["Dc"], seed=3)
    free = _np(m.engine.unconstrained("a", m.engine.free)) != 0
    assert free.shape == (2, 13) and not free.all()                     # (the triangular default: a masked loading)
    m.engine.unconstrained("a").copy_(_t(np.where(free, 1.0, 0.0)))
    m.engine.unconstrained("b").copy_(_t(np.zeros((1, 13))))
    return m, dict(cs, model="irt_2pl", prior={"a": (1.0, 0.5)}, nodes=15, span=5.0)


@pytest.mark.parametrize("kind", ["VaeIRT_padded_J13", "VIRT", "VaeIRT_2pl_d2_padded_J13"])
def test_nothing_else_moved(kind):
    """Thirteen items of the 4PL case: VaeIRT pads them to sixteen.  The guide, Adam's moments, the step count and the phantom
    items keep their bits; the four leaves of the own items move.  And thirteen items under a VaeIRT 2PL with x_feature = 2:
    the masked loadings keep their bits too, the own free loadings and b move."""
    from vipsy_amd import vi
    amortized, d2 = kind != "VIRT", kind == "VaeIRT_2pl_d2_padded_J13"
    m, cs = _model_2pl_d2() if d2 else _model("map2_4pl_j14_g41", cls=vi.VaeIRT if amortized else vi.VIRT, items=13)
    eng = m.engine
    leaves = ("a", "b") if d2 else ("a", "b", "c", "d")
    if amortized:
        assert eng.J > eng.J_items == 13                                # the padded engine: phantom items
    keep = torch.ones(eng.n_params, dtype=torch.bool, device=eng.dev)
    for name in leaves:
        eng.unconstrained(name, keep)[...] = False                     # (a view of `keep`: the own items, wherever they lie)
    if d2:
        o = eng.off["a"]
        J = eng.J                                                      # phantom items part the two rows of the own loadings
        assert not keep[o:o + 13].any() and keep[o + 13:o + J].all() and not keep[o + J:o + J + 13].any() and keep[o + J + 13:o + 2 * J].all()
        free = eng.unconstrained("a", eng.free) != 0
        eng.unconstrained("a", keep)[~free] = True                     # the masked loadings are to keep their bits as well
    state = {"P": eng.P.clone(), "M": eng.M.clone(), "V": eng.V.clone(), "G": eng.G.clone()}
    if eng.per_person:
        state.update({"PP": eng.PP.clone(), "MP": eng.MP.clone(), "VP": eng.VP.clone()})
    t0 = eng.t
    prior = dict(cs["prior"], b=(0.0, 3.0))                             # (the case's own b prior is shaped for fourteen items)
    out = m.fit_em(max_iter=2, tol=0, prior=prior, nodes=cs["nodes"], span=cs["span"])
    torch.cuda.synchronize()
    assert eng.t == t0 and len(out["logpost"]) == 2
    assert torch.equal(eng.P[keep], state["P"][keep])
    answered = torch.ones(eng.J_items, dtype=torch.bool, device=eng.dev)
    answered[mc.UNANSWERED] = False
    for name in leaves:
        now, was = eng.unconstrained(name), eng.unconstrained(name, state["P"])
        moves = answered[None, :] & (eng.unconstrained(name, eng.free) != 0)
        assert (now[moves] != was[moves]).all(), name
        assert torch.equal(now[~moves], was[~moves]), name
    for k in state:
        if k != "P":
            assert torch.equal(getattr(eng, k), state[k]), k
