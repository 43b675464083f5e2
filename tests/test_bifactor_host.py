"""The host side of the bifactor / testlet scores, without a GPU: the structure reader, the two-axis grid, the testlet layout and
its limits (vipsy_amd/grid.py), the two float64 oracles against each other, the restated operand phase against them, the
conditions the cases of tests/bifactor_cases.py have to meet, and the new entries of the C ABI through ctypes."""
import ctypes

import numpy as np
import pytest

from oracle import vi_oracle as vo
from tests import bifactor_cases as bc
from tests import corner_cases as cn
from tests import score_cases as sc
from vipsy_amd import grid


def _mask(D, J, general, testlet):
    free = np.zeros((D, J))
    free[general] = 1
    spec = [d for d in range(D) if d != general]
    for j, s in enumerate(testlet):
        if s >= 0:
            free[spec[s], j] = 1
    return free


# ---- bifactor_structure --------------------------------------------------------------------------------------------------
def test_structure_of_good_masks():
    testlet = np.array([1, 0, -1, 1, 2, 0, -1, 2, 2])
    for general in (0, 2, 3):
        free = _mask(4, 9, general, testlet)
        st = grid.bifactor_structure(free, 0.7 * free, "irt_2pl", general)
        assert st["general"] == general
        assert list(st["specific_dims"]) == [d for d in range(4) if d != general]
        assert np.array_equal(st["testlet"], testlet) and list(st["sizes"]) == [2, 2, 3]
    # a specific dimension without items; an item that is not free on the general dimension either
    free = _mask(5, 9, 0, testlet)
    free[0, 4] = 0
    st = grid.bifactor_structure(free, free, "irt_3pl")
    assert list(st["sizes"]) == [2, 2, 3, 0] and np.array_equal(st["testlet"], testlet)


def test_every_two_dimensional_model_is_a_bifactor_and_the_default_mask_of_three_is_not():
    J = 12
    free = vo.default_a_free(2, J)
    for general in (0, 1):
        st = grid.bifactor_structure(free, free.astype(float), "irt_2pl", general)
        assert list(st["specific_dims"]) == [1 - general] and int(st["sizes"][0]) == (J - 1 if general == 0 else J)
    assert list(grid.bifactor_structure(free, free.astype(float), "irt_2pl")["testlet"]) == [0] * (J - 1) + [-1]
    free = vo.default_a_free(3, J)
    with pytest.raises(ValueError, match=r"item 0 is free on the specific dimensions \[1, 2\]"):
        grid.bifactor_structure(free, free.astype(float), "irt_2pl")


def test_bad_masks_are_refused_by_item():
    testlet = np.array([1, 0, -1, 1, 0, 0])
    free = _mask(3, 6, 0, testlet)
    twice = free.copy()
    twice[1, 3] = 1                                                 # item 3 on both specific dimensions
    with pytest.raises(ValueError, match="item 3 is free on the specific dimensions"):
        grid.bifactor_structure(twice, twice, "irt_2pl")
    a = 0.5 * free
    a[2, 1] = 0.25                                                  # a fixed loading that is not zero
    with pytest.raises(ValueError, match="item 1 has the fixed loading 0.25 on dimension 2"):
        grid.bifactor_structure(free, a, "irt_2pl")
    with pytest.raises(ValueError, match="item 0 has the fixed loading"):      # a_free without a0: the loadings start at 1
        grid.bifactor_structure(free, np.ones_like(free), "irt_2pl")
    for general in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="general must be"):
            grid.bifactor_structure(free, 0.5 * free, "irt_2pl", general)
    with pytest.raises(NotImplementedError, match="irt_1pl"):
        grid.bifactor_structure(np.ones((1, 6)), np.ones((1, 6)), "irt_1pl")
    with pytest.raises(NotImplementedError, match="x_feature = 1"):
        grid.bifactor_structure(np.ones((1, 6)), np.ones((1, 6)), "irt_2pl")


# ---- the two-axis grid ---------------------------------------------------------------------------------------------------
def test_two_axis_grid_and_its_weights():
    theta, logw, u, logv = grid.bifactor_grid((61, 21), (6.0, 4.0))
    assert theta.dtype == logw.dtype == u.dtype == logv.dtype == np.float32
    assert theta.shape == logw.shape == (61,) and u.shape == logv.shape == (21,)
    for p, lw, n, s in ((theta, logw, 61, 6.0), (u, logv, 21, 4.0)):
        want = np.linspace(-s, s, n)
        assert np.abs(p - want).max() < 1e-6 and p[0] == -s and p[-1] == s and p[n // 2] == 0
        w = np.exp(-0.5 * want ** 2)
        assert np.abs(lw - np.log(w / w.sum())).max() < 2e-6
        assert abs(np.exp(lw.astype(np.float64)).sum() - 1.0) < 1e-6
    # the general axis is the one-dimensional grid of score()
    t1, l1 = grid.score_grid(1, 61, 6.0)
    assert np.array_equal(t1[:, 0], theta) and np.array_equal(l1, logw)
    _, _, u1, v1 = grid.bifactor_grid((2, 1), (6.0, 4.0))
    assert u1.tolist() == [0.0] and v1.tolist() == [0.0]


def test_every_limit_of_the_grid_is_a_value_error():
    for nodes in ((1, 21), (257, 21), (61, 0), (61, 33), (61,), 61, (61.0, 21), (True, 21), (61, 21, 5)):
        with pytest.raises(ValueError):
            grid.bifactor_grid(nodes, (6.0, 4.0))
    for span in (6.0, (6.0,), (0.0, 4.0), (6.0, -4.0), (np.inf, 4.0), (6.0, np.nan), ("6", 4.0)):
        with pytest.raises(ValueError):
            grid.bifactor_grid((61, 21), span)
    for nodes in ((256, 32), (2, 1)):
        assert grid.bifactor_grid(nodes, (6.0, 4.0))[0].shape == (nodes[0],)
    with pytest.raises(NotImplementedError, match="explicit nodes"):
        grid.bifactor_grid((np.linspace(-6, 6, 5), np.zeros(5)), (6.0, 4.0))


# ---- the testlet layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.CASES, ids=bc.IDS)
def test_plan_against_a_restatement(case):
    cs = bc.case_of(case)
    Gg = cs["nodes"][0]
    plan = grid.bifactor_plan(cs["testlet"], cs["specific_dims"], Gg)
    # said again: testlets with items in the order of their columns, the general-only items last, each to whole chunks of 16
    groups = [np.flatnonzero(cs["testlet"] == s) for s in range(len(cs["specific_dims"]))] + [np.flatnonzero(cs["testlet"] == -1)]
    columns = list(range(len(cs["specific_dims"]))) + [-1]
    kept = [(c, g) for c, g in zip(columns, groups) if len(g)]
    chunks = [(len(g) + 15) // 16 for _, g in kept]
    assert plan["KC"] == sum(chunks) and list(plan["tl_start"]) == [0] + list(np.cumsum(chunks))
    assert list(plan["tl_column"]) == [c for c, _ in kept] and bc.EMPTY_AT not in plan["tl_column"]
    assert plan["image_bytes"] == Gg * plan["KC"] * 4096
    assert plan["col"].dtype == plan["sdim"].dtype == plan["tl_start"].dtype == np.int32
    assert plan["col"].shape == plan["sdim"].shape == (16 * plan["KC"],)
    for t, (c, g) in enumerate(kept):
        lo, hi = 16 * plan["tl_start"][t], 16 * plan["tl_start"][t + 1]
        assert list(plan["col"][lo:lo + len(g)]) == list(g) and (plan["col"][lo + len(g):hi] == -1).all()      # pad positions
        want_dim = cs["specific_dims"][c] if c >= 0 else -1
        assert (plan["sdim"][lo:lo + len(g)] == want_dim).all() and (plan["sdim"][lo + len(g):hi] == -1).all()
    assert sorted(plan["col"][plan["col"] >= 0]) == list(range(cs["J"]))                   # a permutation of the items
    # the responses in the layout, as score_bifactor permutes them: padding slots 254
    y = cs["y"]
    yp = np.concatenate([y, np.full((len(y), 1), 254, np.uint8)], 1)[:, np.where(plan["col"] >= 0, plan["col"], cs["J"])]
    assert ((yp == 254) == (plan["col"] < 0)[None, :]).all() and (yp == 255).sum() == (y == 255).sum()


def test_the_limits_of_the_plan():
    with pytest.raises(ValueError, match="1 .. 1024 items"):
        grid.bifactor_plan(np.zeros(1025, np.int64), [1], 61)
    with pytest.raises(ValueError, match="1 .. 1024 items"):
        grid.bifactor_plan(np.zeros(0, np.int64), [1], 61)
    # 1 024 testlets of one item: 1 024 chunks, 4 MB a general node
    one_each = np.arange(1024)
    assert grid.bifactor_plan(one_each, np.arange(1, 1025), 128)["image_bytes"] == 512 << 20
    with pytest.raises(ValueError, match="512 MB"):
        grid.bifactor_plan(one_each, np.arange(1, 1025), 129)
    assert grid.bifactor_slab_persons(1) == 262144 and grid.bifactor_slab_persons(100) == 167680
    assert grid.bifactor_slab_persons(1024) == 16384 and grid.bifactor_slab_persons(1024) % 256 == 0


# ---- the oracles, the restatement, the conditions ------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.BRUTE)
def test_brute_force_equals_the_reduction(name):
    o = bc.oracle_of(bc.by_name(name))
    brute, want = o["brute"], o["want"]
    for k in bc.OUTPUTS + ("F",):
        assert np.abs(brute[k] - want[k]).max() <= 1e-12, (name, k, np.abs(brute[k] - want[k]).max())
    assert np.array_equal(brute["node"], want["node"]) and np.abs(brute["gap"] - want["gap"]).max() <= 1e-12
    # the general marginal of the tensor grid is the tensor grid's own general posterior
    for k, j in (("loglik", "loglik_joint"), ("eap_general", "eap_general_joint"), ("psd_general", "psd_general_joint")):
        assert np.abs(brute[k] - brute[j]).max() <= 1e-12, (name, k)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.IDS)
def test_restatement_meets_a_third_of_the_row_rule(case):
    o = bc.oracle_of(case)
    print(case[0], {k: "%.1e" % v for k, v in o["e"].items()}, "cap %.1e" % o["cap"], "d_f %.1e" % o["d_f"])
    for k in bc.OUTPUTS:
        assert o["e"][k] <= o["tol"][k] / 3.0, (case[0], k, o["e"][k], o["tol"][k])
        assert cn.ROW_TOL <= o["tol"][k] <= max(cn.ROW_TOL, o["cap"])
    wrong = (o["r"]["node"] != o["want"]["node"]) & (o["want"]["gap"] > o["gap_thr"])
    assert not wrong.any(), (case[0], np.flatnonzero(wrong))
    if int((o["cs"]["y"] != 255).sum(1).max()) <= cn.SHORT:            # short rows: the rule is ROW_TOL itself
        assert all(o["tol"][k] == cn.ROW_TOL for k in bc.OUTPUTS)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.IDS)
def test_conditions_of_the_cases(case):
    o = bc.oracle_of(case)
    cs, want = o["cs"], o["want"]
    # the node rule leaves nobody out in the oracle alone: no person's best two general nodes within 1e-4, nor within the widened gap
    assert want["gap"].min() > sc.ARGMAX_GAP and o["left_out"] == 0.0 <= sc.ARGMAX_LEFT_OUT, (case[0], want["gap"].min(), o["gap_thr"])
    lo_g, lo_s, need_g, need_s = bc.condition(cs, want)
    if case[0] in bc.CONDITION_HELD:
        assert lo_g >= need_g and lo_s >= need_s, (case[0], lo_g, need_g, lo_s, need_s)
    # what every case carries: nobody's answers, an all-correct person, a specific dimension without items, shuffled items
    assert (cs["y"][0] == 255).all() and (cs["y"][1] == 1).all() and (cs["testlet"] != bc.EMPTY_AT).all()
    assert abs(want["eap_general"][0]) < 1e-9 and want["eap_general"][1] > 1.0
    st = grid.bifactor_structure(cs["free"], cs["params"]["a"], cs["model"], cs["general"])
    assert np.array_equal(st["testlet"], cs["testlet"]) and st["sizes"][bc.EMPTY_AT] == 0
    real = [s for s in range(len(st["sizes"])) if s != bc.EMPTY_AT]
    assert tuple(st["sizes"][real]) == tuple(cs["sizes"])
    for s in real:                                                   # no testlet of two or more items is contiguous
        items = np.flatnonzero(cs["testlet"] == s)
        assert len(items) == 1 or items[-1] - items[0] >= len(items), (case[0], s)
    assert any(bc.case_of(c)["general"] != 0 for c in bc.CASES)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW = ("vx_grid_bifactor_image_bytes", "vx_grid_bifactor_workspace_floats", "vx_grid_table_bifactor", "vx_grid_bifactor",
       "vx_grid_bifactor_specific")


def test_new_symbols_are_declared_bound_and_refuse_bad_arguments():
    import os
    import __graft_entry__ as g
    g.build()
    from vipsy_amd import _hip
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vipsy_amd.h")).read()
    L = _hip.lib()
    for name in NEW:
        assert name in _hip.SIGNATURES and (name + "(") in hdr and hasattr(L, name), name
    assert _hip.ABI_VERSION == 9 and L.vx_abi_version() == 9                     # entries were only added
    # the size queries: from scalars alone, no product overflows
    assert L.vx_grid_bifactor_image_bytes(61, 100) == 61 * 100 * 4096
    assert L.vx_grid_bifactor_image_bytes(128, 1024) == 512 << 20
    for Gg, KC in ((129, 1024), (1, 10), (257, 1), (61, 0), (61, 1025), (-1, 5)):
        assert L.vx_grid_bifactor_image_bytes(Gg, KC) == -1, (Gg, KC)
    assert L.vx_grid_bifactor_workspace_floats(100, 21) == 2 * 21 * 64
    assert L.vx_grid_bifactor_workspace_floats(1 << 48, 256) == (1 << 42) * 256 * 64
    for nb, Gg in ((0, 21), (-7, 21), ((1 << 48) + 1, 21), (100, 1), (100, 257)):
        assert L.vx_grid_bifactor_workspace_floats(nb, Gg) == -1, (nb, Gg)
    # the compute entries refuse before any HIP call (there is no GPU here): null pointers, shapes beyond the limits, and a
    # testlet table that is null or does not run strictly from 0 to KC
    host = (ctypes.c_float * 4096)()
    hp = ctypes.cast(host, ctypes.c_void_p)
    tl_ok = (ctypes.c_int32 * 3)(0, 1, 3)
    cfg = _hip.IrtCfg(2, 5, 23, 0, 1.0, 1.0, 0, 0, 0)
    table = lambda c, Gg, Gh, general, KC, p=hp: L.vx_grid_table_bifactor(ctypes.byref(c), p, Gg, p, Gh, general, p, p, KC,      # noqa: E731
                                                                          p, p, p, p, p, None)
    assert table(cfg, 21, 11, 0, 3, None) == -1
    for Gg, Gh, general, KC in ((1, 11, 0, 3), (257, 11, 0, 3), (21, 0, 0, 3), (21, 33, 0, 3), (21, 11, 5, 3), (21, 11, -1, 3),
                                (21, 11, 0, 0), (21, 11, 0, 1025), (129, 11, 0, 1024)):
        assert table(cfg, Gg, Gh, general, KC) == -1, (Gg, Gh, general, KC)
    for bad in (_hip.IrtCfg(1, 1, 23, 0, 1.0, 1.0, 0, 0, 0), _hip.IrtCfg(2, 1, 23, 0, 1.0, 1.0, 0, 0, 0),
                _hip.IrtCfg(2, 5, 1025, 0, 1.0, 1.0, 0, 0, 0), _hip.IrtCfg(2, 4097, 23, 0, 1.0, 1.0, 0, 0, 0)):
        assert table(bad, 21, 11, 0, 3) == -1

    def main(nb, KC, Gg, Gh, tl, n_tl, p=hp):
        return L.vx_grid_bifactor(p, nb, KC, Gg, Gh, tl, n_tl, p, p, p, p, p, p, p, p, p, p, None, None)

    def spec(nb, KC, Gg, Gh, tl, n_tl, p=hp):
        return L.vx_grid_bifactor_specific(p, nb, KC, Gg, Gh, tl, n_tl, p, p, p, p, p, p, p, p, None)

    for call in (main, spec):
        assert call(100, 3, 21, 11, tl_ok, 2, None) == -1                         # null pointers
        assert call(100, 3, 21, 11, None, 2) == -1                                # no testlet table
        for nb, KC, Gg, Gh, n_tl in ((0, 3, 21, 11, 2), (-7, 3, 21, 11, 2), (100, 0, 21, 11, 2), (100, 1025, 21, 11, 2),
                                     (100, 3, 1, 11, 2), (100, 3, 257, 11, 2), (100, 3, 21, 0, 2), (100, 3, 21, 33, 2),
                                     (100, 3, 21, 11, 0), (100, 3, 21, 11, 4), (100, 1024, 129, 11, 2)):
            assert call(nb, KC, Gg, Gh, tl_ok, n_tl) == -1, (call.__name__, nb, KC, Gg, Gh, n_tl)
        for tl in ((1, 2, 3), (0, 1, 2), (0, 0, 3), (0, 3, 3), (0, 2, 1)):     # not from 0, not to KC, an empty testlet, descending
            assert call(100, 3, 21, 11, (ctypes.c_int32 * 3)(*tl), 2) == -1, tl
