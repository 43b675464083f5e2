"""Expected counts and item fit, the parts that need no GPU: the float64 oracle the GPU tests hold the kernel to
(tests/count_cases.py) checked on identities that need no kernel, the misfit case, the declarations of the new entry points,
and the workspace query (host arithmetic of the library)."""
import os
import re

import numpy as np
import pytest

from tests import count_cases as cc
from tests import score_cases as sc
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ORACLE = {}


def _oracle(case):
    """Each case and its oracle once for the module (never modified)."""
    if case[0] not in _ORACLE:
        if case in cc.IRT_CASES:
            cs = sc.irt_case(case)
            _ORACLE[case[0]] = (cs, cc.irt_oracle(cs))
        else:
            cs = sc.cdm_case(case)
            _ORACLE[case[0]] = (cs, cc.cdm_oracle(cs))
    return _ORACLE[case[0]]


ALL = cc.IRT_CASES + cc.CDM_CASES


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_oracle_identities(case):
    cs, want = _oracle(case)
    y = cs["y"]
    N, J = y.shape
    assert want["n1"].shape == want["n0"].shape == want["prob"].shape == (J, want["mass"].shape[0])
    assert np.abs(want["n1"].sum(1) - (y == 1).sum(0)).max() < 1e-9 * N
    assert np.abs(want["n0"].sum(1) - (y == 0).sum(0)).max() < 1e-9 * N
    assert abs(want["mass"].sum() - N) < 1e-9 * N
    assert np.abs(want["n_obs"] - (y != 255).sum(0)).max() < 1e-9 * N
    assert ((want["prob"] > 0) & (want["prob"] < 1)).all()
    assert np.isfinite(want["md"]).all() and np.isfinite(want["rmsd"]).all()      # every item of every case has an answer
    assert (want["rmsd"] >= np.abs(want["md"]) - 1e-12).all()                     # Cauchy-Schwarz over the nodes


def test_a_person_without_a_response_adds_the_prior_to_mass():
    cs, want = _oracle(cc.IRT_CASES[0])
    assert (cs["y"][5] == 255).all()
    prior = np.exp(want["logw"])
    assert np.abs(want["p"][5] - prior / prior.sum()).max() < 1e-15
    rest = cc.irt_oracle(cs, rows=np.delete(np.arange(cs["N"]), 5))
    assert np.abs((want["mass"] - rest["mass"]) - prior / prior.sum()).max() < 1e-12
    assert np.abs(want["n1"] - rest["n1"]).max() < 1e-12 and np.abs(want["n0"] - rest["n0"]).max() < 1e-12


def test_prob_is_the_response_function_of_the_case():
    from oracle import vi_oracle as vo
    from vipsy_amd.engine import score_grid
    cs, want = _oracle(cc.IRT_CASES[0])                                           # 2PL, D = 1
    theta, _ = score_grid(1, cs["nodes"], cs["span"])
    a, b = cs["params"]["a"].astype(np.float64), cs["params"]["b"].astype(np.float64)
    p = vo.sigmoid(cs["Dc"] * (theta.astype(np.float64) @ a + b)).T
    assert np.abs(want["prob"] - np.clip(p, vo.EPS32, 1 - vo.EPS32)).max() < 1e-6


def test_the_misfit_item_stands_out():
    cs = cc.misfit_case()
    want = cc.irt_oracle(cs)
    r = want["rmsd"]
    others = np.delete(r, cc.MISFIT_ITEM)
    print("misfit: rmsd of item %d %.4f, largest of the others %.4f, median %.4f" % (cc.MISFIT_ITEM, r[cc.MISFIT_ITEM], others.max(),
                                                                                       np.median(r)))
    assert int(r.argmax()) == cc.MISFIT_ITEM
    assert r[cc.MISFIT_ITEM] > 3.0 * others.max()
    assert r[cc.MISFIT_ITEM] == pytest.approx(0.3245, abs=5e-4) and others.max() == pytest.approx(0.0311, abs=5e-4)
    fit = _oracle(cc.COUNT_BIG)[1]["rmsd"]
    assert fit.max() < 0.05                                                       # the same persons with the item as simulated


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_the_method_leaves_a_wide_margin_under_the_row_rule(case):
    """float32 + fp16-pair arithmetic, said again in numpy, against the float64 oracle: the method itself costs at most 3.4e-6 on the
    tables and 6.6e-7 on md / rmsd (printed), so the row rule of the GPU test (3e-5) has a ninefold margin that owes nothing to
    the kernel.  Asserted at an eighth of the rule."""
    cs, want = _oracle(case)
    if case in cc.IRT_CASES:
        from vipsy_amd.engine import score_grid
        theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
        ll = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y"])
    else:
        ll, logw, _ = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], cs["y"])
    got = cc.restated_f32(ll, logw, cs["y"])
    errs = {}
    for k in ("n1", "n0"):
        errs[k] = float((np.abs(got[k] - want[k]).max(1) / np.maximum(np.abs(want[k]).max(1), 1.0)).max())
    errs["mass"] = float(np.abs(got["mass"] - want["mass"]).max() / max(np.abs(want["mass"]).max(), 1.0))
    f32 = cc.fit_stats(got["n1"].astype(np.float64), got["n0"].astype(np.float64), want["prob"].astype(np.float32).astype(np.float64))
    errs["md"] = float(np.abs(f32["md"] - want["md"]).max())
    errs["rmsd"] = float(np.abs(f32["rmsd"] - want["rmsd"]).max())
    print(cs["name"], "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e <= ROW_TOL / 8, (cs["name"], k, e)


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"\bint64_t\s+vx_grid_counts_workspace_floats\s*\(\s*int64_t nb,\s*int32_t J,\s*int32_t G\s*\)\s*;", header)
    assert re.search(r"\bint\s+vx_grid_counts\s*\(\s*const uint8_t\*", header)
    assert len(_hip.SIGNATURES["vx_grid_counts_workspace_floats"][1]) == 3
    assert len(_hip.SIGNATURES["vx_grid_counts"][1]) == 13


def test_model_classes_have_the_methods():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, IrtEngine
    for name in ("expected_counts", "item_fit"):
        assert callable(getattr(vi.BasePsy, name))
        assert callable(getattr(IrtEngine, name)) and callable(getattr(CcdmEngine, name))
    assert "shard" in vi.BasePsy.expected_counts.__doc__


def test_item_fit_stats_match_the_oracle_formulas():
    import torch
    from vipsy_amd.engine import item_fit_stats
    _, want = _oracle(cc.IRT_CASES[0])
    n1, n0 = want["n1"].copy(), want["n0"].copy()
    n1[4] = 0.0
    n0[4] = 0.0                                                                   # an item nobody answered
    n1[6, :7] = 0.0
    n0[6, :7] = 0.0                                                               # nodes no person of the item reaches
    ref = cc.fit_stats(n1, n0, want["prob"])
    got = item_fit_stats(torch.from_numpy(n1), torch.from_numpy(n0), torch.from_numpy(want["prob"]))
    for k in ("n_obs", "md", "rmsd", "observed"):
        assert got[k].dtype == torch.float64
        np.testing.assert_allclose(got[k].numpy(), ref[k], rtol=1e-13, atol=1e-15, equal_nan=True)
    assert np.isnan(ref["md"][4]) and np.isnan(ref["rmsd"][4]) and ref["n_obs"][4] == 0
    assert np.isnan(ref["observed"][6, :7]).all() and np.isfinite(ref["md"][6])


# ---- the workspace query -----------------------------------------------------------------------------------------------------
def test_workspace_query_limits_and_growth():
    from vipsy_amd import _hip
    L = _hip.lib()
    q = L.vx_grid_counts_workspace_floats
    slab = 2 * 37 * 61 + 61
    assert q(64, 37, 61) == slab                                                  # one chunk of persons: one slab
    assert q(2500, 37, 61) > slab and q(2500, 37, 61) % slab == 0                 # COUNT_BIG really sums several
    assert q(1, 1, 1) == 3 and q(1, 1024, 1024) == 2 * 1024 * 1024 + 1024
    for nb, J, G in [(0, 37, 61), (-5, 37, 61), (64, 1025, 61), (64, 37, 1025), (64, 0, 61), (64, 37, 0), (64, -1, -1)]:
        assert q(nb, J, G) == -1, (nb, J, G)
    # a million persons: the slabs stay a small multiple of the tables, nowhere near persons x nodes
    assert q(1 << 20, 500, 61) <= 256 * (2 * 500 * 61 + 61)
    assert q(1 << 40, 1024, 1024) > 0                                             # int64 arithmetic
