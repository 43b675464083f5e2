"""fit_sums / person_fit / item_msq, the parts that need no GPU: the declarations, the workspace arithmetic, the formulas of lz
against an enumeration of every response vector, the host functions on hand-made sums, the condition under which the float64
oracle of tests/fit_cases.py is a fair yardstick, the sums said again in float32 against it, the planted case and the refusals."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fit_cases as fc
from tests import score_cases as sc
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("fit_sums", "person_fit", "item_msq")


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9 and _hip.lib().vx_abi_version() == 9
    for name, nargs in (("vx_grid_fit_workspace_floats", 2), ("vx_grid_fit_irt", 14), ("vx_grid_fit_cdm", 14)):
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")) == nargs, name
        assert len(_hip.SIGNATURES[name][1]) == nargs, name


def test_workspace_query_answers_without_a_gpu():
    """Host arithmetic: one partial [4][J] a workgroup, a workgroup a unit of 32 persons up to 1 024 workgroups, then contiguous
    chunks of units -- a function of nb and J alone.  Bad shapes answer -1."""
    from vipsy_amd import _hip
    L = _hip.lib()
    for J in (1, 33, 500, 1024):
        for nb, blocks in ((1, 1), (32, 1), (33, 2), (257, 9), (32768, 1024), (32769, 513), (32801, 513), (1000000, 1009)):
            assert L.vx_grid_fit_workspace_floats(nb, J) == blocks * 4 * J, (nb, J)
    for J in (0, -1, 1025, 1 << 20):
        assert L.vx_grid_fit_workspace_floats(100, J) == -1
    for nb in (0, -7, (1 << 48) + 1):
        assert L.vx_grid_fit_workspace_floats(nb, 37) == -1


def test_model_classes_have_the_methods():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, HipBackend, IrtEngine, _EngineBase
    for name in CALLS:
        assert callable(getattr(vi.BasePsy, name))
        assert getattr(IrtEngine, name) is not getattr(_EngineBase, name) and getattr(CcdmEngine, name) is not getattr(_EngineBase, name)
    for doc in (vi.BasePsy.person_fit.__doc__, IrtEngine.person_fit.__doc__):
        doc = " ".join(doc.split())
        assert "Snijders" in doc and "narrower than N(0, 1)" in doc
    for name in ("grid_fit_irt", "grid_fit_cdm", "grid_fit_workspace"):
        assert callable(getattr(HipBackend, name))
    assert callable(IrtEngine._fit_call) and callable(CcdmEngine._fit_call)


# ---- the formulas ------------------------------------------------------------------------------------------------------------
def test_e_and_v_are_the_mean_and_variance_of_l0():
    """Ten items: the oracle's e and v equal the mean and the variance of l0 over all 2^10 response vectors, weighted by their
    probability under the model, to 1e-10.  This checks the formula, not the arithmetic."""
    rng = np.random.RandomState(9)
    P = rng.uniform(0.05, 0.95, size=10)
    Y = np.array(list(itertools.product((0, 1), repeat=10)), np.uint8)
    o = fc.sums(Y, np.broadcast_to(P, Y.shape))
    l0 = o["person"]["l0"]
    prob = np.exp(l0)
    assert abs(prob.sum() - 1.0) <= 1e-12
    mean = (prob * l0).sum()
    var = (prob * (l0 - mean) ** 2).sum()
    assert np.abs(o["person"]["e"] - mean).max() <= 1e-10 and np.abs(o["person"]["v"] - var).max() <= 1e-10
    assert (o["person"]["n"] == 10).all()
    # under the model the squared standardised residual has mean 1: outfit of every item, weighted by the vectors' probability
    t, _ = fc.cell_terms(Y, np.broadcast_to(P, Y.shape))
    assert np.abs((prob[:, None] * t["sz2"]).sum(0) - 1.0).max() <= 1e-10
    assert np.abs((prob[:, None] * t["sr2"]).sum(0) - P * (1 - P)).max() <= 1e-10


def test_host_functions_on_hand_made_sums():
    from vipsy_amd.grid import item_msq_host, person_fit_host
    person = {"n": [4, 0, 3, 2], "l0": [-3.0, 0, -1.0, -2.0], "e": [-2.0, 0, -1.5, -1.0], "v": [4.0, 0, 0.0, 0.25],
              "sr2": [1.0, 0, 0.6, 0.3], "sw": [0.8, 0, 0.5, 0.0], "sz2": [6.0, 0, 2.4, 1.0]}
    out = person_fit_host(person)
    assert set(out) == {"lz", "infit", "outfit"} and all(v.dtype == np.float64 for v in out.values())
    assert out["lz"][0] == -0.5 and np.isnan(out["lz"][1]) and np.isnan(out["lz"][2]) and out["lz"][3] == -2.0
    assert out["infit"][0] == 1.25 and np.isnan(out["infit"][1]) and out["infit"][2] == 1.2 and np.isnan(out["infit"][3])
    assert out["outfit"][0] == 1.5 and np.isnan(out["outfit"][1]) and out["outfit"][2] == pytest.approx(0.8) and out["outfit"][3] == 0.5
    item = {k: person[k] for k in fc.ITEM}
    got = item_msq_host(item)
    assert set(got) == {"infit", "outfit"}
    assert np.array_equal(got["infit"], out["infit"], equal_nan=True) and np.array_equal(got["outfit"], out["outfit"], equal_nan=True)
    with pytest.raises(ValueError):
        person_fit_host(dict(person, v=[1.0]))
    with pytest.raises(KeyError):
        item_msq_host({"n": [1]})


@pytest.mark.parametrize("kind,case", fc.ALL, ids=fc.ALL_IDS)
def test_host_functions_agree_with_the_oracle(kind, case):
    from vipsy_amd.grid import item_msq_host, person_fit_host
    o = fc.oracle(kind, case)
    got = person_fit_host(o["person"])
    for k in ("lz", "infit", "outfit"):
        assert np.allclose(got[k], o[k], rtol=0, atol=1e-12, equal_nan=True), k
    it = item_msq_host(o["item"])
    assert np.allclose(it["infit"], o["item_infit"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.allclose(it["outfit"], o["item_outfit"], rtol=0, atol=1e-12, equal_nan=True)


# ---- the oracle as a yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", fc.ALL, ids=fc.ALL_IDS)
def test_comparison_condition_and_its_cap(kind, case):
    """The condition of the lz comparison (oracle n >= 5, v > 0.25) leaves out at most 5 % of a case's persons: 3 % of
    case1_2pl_n33_j37 (the person without answers) and nobody elsewhere."""
    o = fc.oracle(kind, case)
    left = 1.0 - o["keep"].mean()
    print("%s: %.3f of the persons left out; n min %d, v min %.3f" % (case[0], left, o["person"]["n"].min(), o["person"]["v"].min()))
    assert left <= fc.LEFT_OUT_CAP
    if case[0] == "case1_2pl_n33_j37":
        assert (~o["keep"]).sum() == 1 and o["person"]["n"][5] == 0 and np.isnan(o["lz"][5])
        assert all(o["person"][k][5] == 0 for k in fc.PERSON)
    else:
        assert left == 0.0
    assert np.isfinite(o["lz"][o["keep"]]).all()
    for k in fc.PERSON:
        assert np.isfinite(o["person"][k]).all() and np.isfinite(o["person_abs"][k]).all()


@pytest.mark.parametrize("kind,case", fc.ALL, ids=fc.ALL_IDS)
def test_float32_restatement_meets_the_rules(kind, case):
    """A plain float32 numpy restatement of the sums (fit_cases.restated_f32) against the float64 oracle by the rules of
    tests/fit_cases.py: n exact, every sum and lz within C = fit_cases.FIT_C of the rule's unit.  Measured: at most 4.92 (an
    item's sr2 in case3_1pl_j130) for a sum and 1.65 for lz.  Printed."""
    o, r = fc.oracle(kind, case), fc.restated_f32(kind, case)
    assert np.array_equal(r["person"]["n"].astype(np.float64), o["person"]["n"])
    assert np.array_equal(r["item"]["n"].astype(np.float64), o["item"]["n"])
    rp = fc.sum_ratios(r["person"], o["person"], o["person_abs"], fc.PERSON)
    ri = fc.sum_ratios(r["item"], o["item"], o["item_abs"], fc.ITEM)
    rl = fc.lz_ratio(r["lz"], o)
    print("%s: person sums %s; item sums %s; lz %.2f" % (case[0], " ".join("%s %.2f" % kv for kv in rp.items()),
                                                        " ".join("%s %.2f" % kv for kv in ri.items()), rl))
    assert max(rp.values()) <= fc.FIT_C and max(ri.values()) <= fc.FIT_C and rl <= fc.FIT_C


def test_planted_case_in_the_oracle():
    """pf_2pl_n5000_j70_aberrant in float64: of the 250 persons with the lowest lz at least 200 are planted ones, the planted
    persons' mean lz lies below -3 and that of the rest within 0.5 of zero.  Measured: 222 of the 250, mean lz -4.25 against
    +0.20, mean outfit 1.77 against 0.95.  The figures are printed."""
    o = fc.oracle("irt", fc.PLANTED)
    who = fc.planted_persons()
    assert len(who) == 250 and len(np.unique(who)) == 250
    lz = o["lz"]
    assert np.isfinite(lz).all()
    planted = np.zeros(len(lz), bool)
    planted[who] = True
    lowest = np.argsort(lz)[:250]
    hits = int(planted[lowest].sum())
    print("planted: %d of the 250 lowest lz are planted persons; mean lz planted %.2f, rest %.2f; outfit planted %.2f, rest %.2f"
          % (hits, lz[planted].mean(), lz[~planted].mean(), o["outfit"][planted].mean(), o["outfit"][~planted].mean()))
    assert hits >= 200
    assert lz[planted].mean() < -3.0 and abs(lz[~planted].mean()) < 0.5
    assert o["outfit"][planted].mean() > 1.3 and abs(o["outfit"][~planted].mean() - 1.0) < 0.15


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


def test_classes_without_grid_scores_refuse():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VCHoDina, vi.VaeCCDM, vi.VCDM):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        for name in CALLS:
            with pytest.raises(NotImplementedError) as e:
                getattr(m, name)()
            assert type(m.engine).__name__ in str(e.value)


def test_four_dimensions_refuse_with_the_wording_of_score():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", x_feature=4, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        m.engine.score()
    for name in CALLS:
        with pytest.raises(NotImplementedError) as e:
            getattr(m, name)()
        assert str(e.value) == str(want.value) and "x_feature" in str(e.value)


def test_bad_data_is_refused_before_anything_is_computed():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_3pl", backend=OracleBackend())
    with pytest.raises(ValueError):
        m.person_fit(data=_y(j=11))
    with pytest.raises(IndexError):
        m.engine.fit_sums(rows=[0, 24])
    with pytest.raises(ValueError):
        m.item_msq(nodes=1)


def test_item_msq_refuses_two_ranks_in_the_wording_of_item_fit(tmp_path):
    """A gloo group of two: item_msq refuses through the model class and on the engine, before anything is computed, in the
    wording of item_fit()."""
    worker = os.path.join(ROOT, "tests", "_fit_dist_worker.py")
    out = str(tmp_path / "fit_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29657", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29657", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            lines = f.read().splitlines()
        assert lines[0] == "NotImplementedError NotImplementedError NotImplementedError"
        assert lines[1] == "item_msq with a group of 2 ranks: fit_sums() gives the local shard's sums; the cross-rank sum is not built"
        assert lines[1].replace("item_msq", "item_fit").replace("fit_sums()", "expected_counts()") == lines[3]
        assert lines[2].startswith("item_msq over a process group: ") and lines[2].endswith("the cross-rank sum is not built")
