"""Bifactor / testlet grid scores on the GPU (vx_grid_table_bifactor / vx_grid_bifactor / vx_grid_bifactor_specific behind
IrtEngine.score_bifactor and the model classes' score_bifactor()) against the float64 oracles of tests/bifactor_cases.py.

Item parameters are drawn and set on the engine through its views, not trained.  Every output -- loglik, eap_general,
psd_general, eap_specific, psd_specific -- is held to the oracle by the project's row rule, _row_errors(got, want, floor = 1) <=
row_tol(e_restated, tol_cap(loglik)) (tests/corner_cases.py; tests/test_bifactor_host.py asserts on the CPU that the restatement
itself meets a third of it), node by the node rule: equal to the oracle's wherever the oracle's best two general nodes differ by
more than max(ARGMAX_GAP, 4 d_f).  The errors found are printed.

Shapes: the smallest at which the kernels can go wrong -- see the table of bifactor_cases.CASES."""
import numpy as np
import pytest
import torch

from tests import bifactor_cases as bc
from tests import corner_cases as cn
from tests import score_cases as sc
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

SHARED = ("loglik", "eap_general", "psd_general", "node")


def _np(t):
    return t.detach().cpu().numpy()


def _engine(cs, D=None, params=None, own_mask=False):
    """own_mask: no a_free / a0 -- the engine's triangular default."""
    from vipsy_amd.engine import IrtEngine
    params = cs["params"] if params is None else params
    free = cs["free"]
    D = cs["D"] if D is None else D
    kw = {} if D == 1 or own_mask else {"a_free": torch.from_numpy(np.ascontiguousarray(free)), "a0": torch.from_numpy(np.ascontiguousarray(params["a"]))}
    eng = IrtEngine(torch.from_numpy(cs["y"]).to(_dev()), model=cs["model"], D=D, Dc=cs["Dc"], seed=3, **kw)
    for name, v in params.items():
        eng.unconstrained(name).copy_(torch.from_numpy(np.ascontiguousarray(v)).to(_dev()))
    return eng


_GOT = {}


def _got(case):
    """The engine of a case and its score_bifactor(specific=True), computed once and shared (never modified)."""
    if case[0] not in _GOT:
        cs = bc.case_of(case)
        eng = _engine(cs)
        got = eng.score_bifactor(nodes=cs["nodes"], span=cs["span"], general=cs["general"], specific=True)
        torch.cuda.synchronize()
        _GOT[case[0]] = (eng, got)
    return _GOT[case[0]]


def _hold(tag, got, want, tol, gap_thr, rows=None):
    """The row rule on every output that `got` has, the node rule on the node; prints what it finds."""
    pick = (lambda v: v) if rows is None else (lambda v: v[rows])
    errs = {}
    for k in bc.OUTPUTS:
        if k in got:
            errs[k] = cn._row_errors(_np(got[k]).astype(np.float64), pick(np.asarray(want[k], np.float64)), 1.0)
    sure = pick(want["gap"]) > gap_thr
    wrong = np.flatnonzero(sure & (_np(got["node"]).astype(np.int64) != pick(want["node"])))
    print("%s: %s; %.1f %% of the persons left out of the node rule (gap %.1e), %d wrong nodes"
          % (tag, "  ".join("%s %.2e (tol %.1e)" % (k, v, tol[k]) for k, v in errs.items()), 100 * float((~sure).mean()), gap_thr,
             len(wrong)))
    for k, e in errs.items():
        assert e <= tol[k], (tag, k, e, tol[k])
    assert float((~sure).mean()) <= sc.ARGMAX_LEFT_OUT, tag
    assert len(wrong) == 0, (tag, wrong[:10])


@pytest.mark.parametrize("case", bc.CASES, ids=bc.IDS)
def test_scores_vs_oracle(case):
    o = bc.oracle_of(case)
    cs, want = o["cs"], o["want"]
    eng, got = _got(case)
    N, S = cs["N"], len(cs["specific_dims"])
    for k in SHARED:
        assert got[k].shape == (N,), k
    assert got["node"].dtype == torch.int32
    assert got["eap_specific"].shape == (N, S) and got["psd_specific"].shape == (N, S)
    assert np.array_equal(np.asarray(got["specific_dims"]), cs["specific_dims"])
    st = eng.bifactor_structure(cs["general"])
    assert np.array_equal(st["testlet"], cs["testlet"]) and st["general"] == cs["general"]
    _hold(cs["name"], got, want, o["tol"], o["gap_thr"])
    if cs["name"] in bc.CONDITION_HELD:
        lo_g, lo_s, need_g, need_s = bc.condition(cs, want)
        assert lo_g >= need_g and lo_s >= need_s, (cs["name"], "oracle PSD below half the node spacing")
    # the specific dimension without items: the moments of the grid prior, for everybody
    col = bc.EMPTY_AT
    assert (cs["testlet"] != col).all()
    assert float(got["eap_specific"][:, col].abs().max()) <= cn.ROW_TOL
    assert float((got["psd_specific"][:, col] - float(want["psd_specific"][0, col])).abs().max()) <= cn.ROW_TOL
    # nobody's answers: the prior's moments, the centre node, the missing constant a cell; all correct: a high score
    assert (cs["y"][0] == 255).all() and (cs["y"][1] == 1).all()
    assert abs(float(got["eap_general"][0])) <= cn.ROW_TOL and int(got["node"][0]) == (cs["nodes"][0] - 1) // 2
    assert abs(float(got["loglik"][0]) - cs["J"] * cn.missing_constant()) <= cn.ROW_TOL
    assert float(got["eap_general"][1]) > 1.0


@pytest.mark.parametrize("name", ["s2_2pl", "s40", "gh1"])
def test_specific_off_gives_the_same_bits_and_so_does_a_second_call(name):
    case = bc.by_name(name)
    cs = bc.case_of(case)
    eng, got = _got(case)
    kw = dict(nodes=cs["nodes"], span=cs["span"], general=cs["general"])
    off = eng.score_bifactor(**kw)
    again = eng.score_bifactor(specific=True, **kw)
    torch.cuda.synchronize()
    assert sorted(off) == sorted(SHARED)
    for k in SHARED:
        assert torch.equal(off[k], got[k]), k
    for k in SHARED + ("eap_specific", "psd_specific"):
        assert torch.equal(again[k], got[k]), k


def test_rows_and_new_data_give_each_person_the_bits_of_the_full_call():
    case = bc.by_name("s40")
    cs = bc.case_of(case)
    eng, got = _got(case)
    kw = dict(nodes=cs["nodes"], span=cs["span"], general=cs["general"], specific=True)
    rows = np.random.RandomState(4).permutation(cs["N"])[:71]
    sub = eng.score_bifactor(rows=torch.from_numpy(rows), **kw)
    new = eng.score_bifactor(torch.from_numpy(cs["y"][rows]), **kw)
    torch.cuda.synchronize()
    at = torch.from_numpy(rows).to(_dev())
    for k in SHARED + ("eap_specific", "psd_specific"):
        assert sub[k].shape[0] == len(rows)
        assert torch.equal(sub[k], got[k][at]), k
        assert torch.equal(new[k], got[k][at]), k


@pytest.mark.parametrize("name", ["s2_2pl", "s5_3pl"])
def test_the_item_order_does_not_matter(name):
    """The same model and data with the items in another order: another testlet layout, the same scores within the row rule."""
    case = bc.by_name(name)
    o = bc.oracle_of(case)
    cs = o["cs"]
    _, got = _got(case)
    cs2, _ = bc.shuffled(cs)
    eng2 = _engine(cs2)
    got2 = eng2.score_bifactor(nodes=cs["nodes"], span=cs["span"], general=cs["general"], specific=True)
    torch.cuda.synchronize()
    for k in bc.OUTPUTS:
        e = cn._row_errors(_np(got2[k]).astype(np.float64), _np(got[k]).astype(np.float64), 1.0)
        print("%s shuffled: %s %.2e (tol %.1e)" % (name, k, e, o["tol"][k]))
        assert e <= o["tol"][k], (name, k, e)
    _hold(name + " shuffled", got2, o["want"], o["tol"], o["gap_thr"])


def _cross_case(D, J, N, seed):
    """A D-dimensional 2PL whose mask is a bifactor with general dimension 0: D = 2 -- the engine's triangular default; D = 3 --
    the items alternate between the two specific dimensions."""
    rng = np.random.RandomState(seed)
    free = np.zeros((D, J), np.float32)
    free[0] = 1
    if D == 2:
        free[1, :J - 1] = 1
    else:
        free[1 + np.arange(J) % 2, np.arange(J)] = 1
        free[:, J - 1] = (1, 0, 0)
    a = (rng.uniform(0.4, 1.0, size=(D, J)) * free).astype(np.float32)
    a[0] = rng.uniform(0.6, 1.4, size=J)
    b = rng.normal(size=J).astype(np.float32)
    z = rng.normal(size=(N, D)) @ a.astype(np.float64) + b[None, :]
    y = (rng.uniform(size=(N, J)) < 1.0 / (1.0 + np.exp(-z))).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.1] = 255
    return {"y": y, "model": "irt_2pl", "Dc": 1.0, "D": D, "J": J, "free": free, "params": {"a": a, "b": b}}


@pytest.mark.parametrize("D,n", [(2, 21), (3, 9)])
def test_against_score_on_the_same_quadrature(D, n):
    """score() of a D = 2 / D = 3 engine is the same quadrature on the tensor grid: loglik, the general and the specific EAP / PSD
    agree within twice the row rule (ROW_TOL: the persons answered 20 items)."""
    cs = _cross_case(D, 20, 100, 40 + D)
    eng = _engine(cs, own_mask=D == 2)
    if D == 2:                                                         # the engine's own default mask
        assert np.array_equal(_np(eng.unconstrained("a", eng.free)) != 0, cs["free"] != 0)
    full = eng.score(nodes=n, span=6.0)
    got = eng.score_bifactor(nodes=(n, n), span=(6.0, 6.0), specific=True)
    torch.cuda.synchronize()
    pairs = [("loglik", full["loglik"]), ("eap_general", full["eap"][:, 0]), ("psd_general", full["psd"][:, 0]),
             ("eap_specific", full["eap"][:, 1:]), ("psd_specific", full["psd"][:, 1:])]
    for k, want in pairs:
        e = cn._row_errors(_np(got[k]).astype(np.float64), _np(want).astype(np.float64), 1.0)
        print("D = %d, %d nodes a dimension: %s %.2e" % (D, n, k, e))
        assert e <= 2 * cn.ROW_TOL, (D, k, e)


def test_one_specific_node_is_the_unidimensional_model():
    """Gh = 1 (u = 0): loglik and the general moments are those of score() of a one-dimensional engine with the general loadings."""
    case = bc.by_name("gh1")
    cs = bc.case_of(case)
    _, got = _got(case)
    one = _engine(cs, D=1, params={"a": cs["params"]["a"][cs["general"]:cs["general"] + 1], "b": cs["params"]["b"]})
    full = one.score(nodes=cs["nodes"][0], span=cs["span"][0])
    torch.cuda.synchronize()
    for k, want in (("loglik", full["loglik"]), ("eap_general", full["eap"][:, 0]), ("psd_general", full["psd"][:, 0])):
        e = cn._row_errors(_np(got[k]).astype(np.float64), _np(want).astype(np.float64), 1.0)
        print("gh1 against the 1-D score(): %s %.2e" % (k, e))
        assert e <= 2 * cn.ROW_TOL, (k, e)
    assert torch.equal(got["node"], full["node"])


def test_a_waves_second_unit_starts_clean():
    """More persons than one launch has lanes for (2 blocks a CU, 4 waves a block, 64 persons a unit), in the manner of
    score_cases.second_unit_case: the head rows are coin flips with 70 % of the cells missing, the last 97 are drawn, eight of
    them with no answer.  The tail scored behind the others gives the bits it gives alone, and holds to its oracle: nothing of
    a unit reaches the next."""
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    case = ("second_unit", 97, (4, 3), 2, "irt_2pl", 1.0, (5, 3), 0.20, 18, 0)
    cs = dict(bc.case_of(case))
    y_tail = cs["y"].copy()
    y_tail[[3, 17, 31, 32, 47, 63, 64, 96]] = 255
    cs["y"] = y_tail
    want = bc.reduced(cs)
    r = bc.restated(cs)
    tol = {k: cn.row_tol(cn._row_errors(r[k], want[k], 1.0), cn.tol_cap(want["loglik"])) for k in bc.OUTPUTS}
    rng = np.random.RandomState(19)
    head = (rng.uniform(size=(2 * cus * 256, cs["J"])) < 0.5).astype(np.uint8)
    head[rng.uniform(size=head.shape) < 0.70] = 255
    both = dict(cs, y=np.concatenate([head, y_tail]))
    eng = _engine(both)
    kw = dict(nodes=cs["nodes"], span=cs["span"], specific=True)
    full = eng.score_bifactor(**kw)
    alone = eng.score_bifactor(torch.from_numpy(y_tail), **kw)
    torch.cuda.synchronize()
    behind = {k: full[k][len(head):] for k in SHARED + ("eap_specific", "psd_specific")}
    for k, v in behind.items():
        assert torch.equal(v, alone[k]), k
    # (five general nodes: the node rule's gap condition is about the quadrature, and is not asked -- as in score_cases)
    for k in bc.OUTPUTS:
        e = cn._row_errors(_np(behind[k]).astype(np.float64), want[k], 1.0)
        assert e <= tol[k], (k, e, tol[k])
    empty = np.flatnonzero((y_tail == 255).all(1))
    # (the eight, and row 0: every case's own person without answers)
    assert len(empty) == 9 and (np.abs(want["loglik"][empty]) < 1e-5).all() and (_np(behind["node"])[empty] == 2).all()


def test_the_a_free_route_end_to_end():
    """VIRT(x_feature = 1 + S, a_free = mask, a0 = mask) builds, takes a few fit() steps and is scored; score() still refuses
    x_feature > 3 as before."""
    from vipsy_amd import vi
    rng = np.random.RandomState(21)
    S, J, N = 4, 22, 200
    mask = np.zeros((1 + S, J), np.float32)
    mask[0] = 1
    mask[1 + rng.randint(0, S, size=J - 2), np.arange(J - 2)] = 1          # the last two items: general only
    y = (rng.uniform(size=(N, J)) < 0.55).astype(np.float32)
    y[rng.uniform(size=y.shape) < 0.1] = np.nan
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=1 + S, a_free=torch.from_numpy(mask),
                a0=torch.from_numpy(mask.copy()), seed=5)
    m.fit(optim=vi.Adam({"lr": 1e-2}), max_iter=3, progress=False)
    st = m.bifactor_structure()
    assert st["general"] == 0 and list(st["specific_dims"]) == [1, 2, 3, 4] and int(st["sizes"].sum()) == J - 2
    assert (st["testlet"][-2:] == -1).all()
    got = m.score_bifactor(specific=True)
    new = m.score_bifactor(data=torch.from_numpy(y[:50]).to(_dev()), specific=True)
    torch.cuda.synchronize()
    assert got["loglik"].shape == (N,) and got["eap_specific"].shape == (N, S)
    for k in SHARED + ("eap_specific", "psd_specific"):
        assert bool(torch.isfinite(got[k].float()).all()), k
        assert torch.equal(new[k], got[k][:50]), k
    assert float(got["psd_general"].min()) > 0 and float(got["psd_specific"].min()) > 0
    with pytest.raises(NotImplementedError, match="x_feature <= 3"):
        m.score()
    with pytest.raises(NotImplementedError):
        m.score_bifactor(covariates=torch.zeros(N, 1))
    with pytest.raises(NotImplementedError):
        m.score_bifactor(nodes=(np.linspace(-4, 4, 9), np.zeros(9)))


def test_the_limits_are_value_errors_and_the_other_classes_refuse():
    case = bc.by_name("s2_2pl")
    eng, _ = _got(case)
    for kw in (dict(nodes=(1, 5)), dict(nodes=(257, 5)), dict(nodes=(21, 0)), dict(nodes=(21, 33)), dict(nodes=21),
               dict(span=(6.0, -1.0)), dict(span=6.0), dict(general=4), dict(general=-1)):
        with pytest.raises(ValueError):
            eng.score_bifactor(**kw)
    from vipsy_amd.engine import CcdmEngine, IrtEngine
    y = torch.from_numpy(bc.case_of(case)["y"]).to(_dev())
    one = IrtEngine(y, model="irt_1pl", D=1, seed=3)
    for call in (one.bifactor_structure, one.score_bifactor):
        with pytest.raises(NotImplementedError):
            call()
    cdm = CcdmEngine(y, sc.cdm_q(3, int(y.shape[1]), np.random.RandomState(1)), cdm="dina")
    for call in (cdm.bifactor_structure, cdm.score_bifactor):
        with pytest.raises(NotImplementedError):
            call()
    three = IrtEngine(y, model="irt_2pl", D=3, seed=3)                 # the triangular default mask of x_feature = 3
    with pytest.raises(ValueError, match="item 0 is free on the specific dimensions"):
        three.score_bifactor()
