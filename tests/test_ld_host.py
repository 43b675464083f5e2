"""residual_sums / local_dependence, the parts that need no GPU: the declarations, the workspace arithmetic, the host formulas of
Q3 against an independent np.corrcoef oracle, the conditions and caps under which the float64 oracle of tests/ld_cases.py is a fair
yardstick (checked on the oracle alone), the kernels' arithmetic said again in float32 + fp16 pairs against it, and the refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ld_cases as ld
from tests import score_cases as sc
from tests.oracle_backend import OracleBackend
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = ("irt", ld.PLANTED)


# ---- declarations ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from vipsy_amd import _hip
    with open(os.path.join(ROOT, "include", "vipsy_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define VX_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9 and _hip.lib().vx_abi_version() == 9
    for name, nargs in (("vx_grid_pairs_workspace_floats", 2), ("vx_grid_pairs_workspace_min_floats", 1),
                        ("vx_grid_pairs_irt", 16), ("vx_grid_pairs_cdm", 16)):
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")) == nargs, name
        assert len(_hip.SIGNATURES[name][1]) == nargs, name
    assert "2^24" in header                                         # how far n is exact


def test_workspace_queries_answer_without_a_gpu():
    """Host arithmetic: the minimum holds the fragments of one slab of 256 persons (8 units x JT tiles x 2 k-steps x 5 operands x 64
    lanes x 16 B) and three sets of 6 tiles a tile pair (one chunk, its sum, the running sum); the preferred size is never below
    it and never above 512 MB where the minimum is below that; bad shapes answer -1."""
    from vipsy_amd import _hip
    L = _hip.lib()
    for J in (1, 32, 33, 37, 130, 500, 1024):
        JT = (J + 31) // 32
        lo = L.vx_grid_pairs_workspace_min_floats(J)
        assert lo == 8 * JT * 2 * 5 * 64 * 4 + 3 * (JT * (JT + 1) // 2) * 6 * 1024
        for nb in (1, 255, 256, 257, 5000, 1000000, 1 << 30):
            pref = L.vx_grid_pairs_workspace_floats(nb, J)
            assert lo <= pref <= max(lo, 128 << 20), (J, nb, lo, pref)
        assert L.vx_grid_pairs_workspace_floats(256, J) == lo
    for J in (0, -1, 1025, 1 << 20):
        assert L.vx_grid_pairs_workspace_min_floats(J) == -1 and L.vx_grid_pairs_workspace_floats(100, J) == -1
    for nb in (0, -7, (1 << 48) + 1):
        assert L.vx_grid_pairs_workspace_floats(nb, 37) == -1


def test_model_classes_have_the_methods():
    from vipsy_amd import vi
    from vipsy_amd.engine import CcdmEngine, HipBackend, IrtEngine, _EngineBase
    for name in ("residual_sums", "local_dependence"):
        assert callable(getattr(vi.BasePsy, name))
        assert getattr(IrtEngine, name) is not getattr(_EngineBase, name) and getattr(CcdmEngine, name) is not getattr(_EngineBase, name)
        for doc in (getattr(vi.BasePsy, name).__doc__, getattr(IrtEngine, name).__doc__):
            doc = " ".join(doc.split())
            assert "as they stand" in doc and "pairwise-complete" in doc and ("EAP" in doc and "MAP" in doc)
    assert "NaN in `q3` means" in " ".join(vi.BasePsy.local_dependence.__doc__.split())
    for name in ("grid_pairs_irt", "grid_pairs_cdm", "grid_pairs_workspace"):
        assert callable(getattr(HipBackend, name))
    assert callable(IrtEngine._pairs_call) and callable(CcdmEngine._pairs_call)


# ---- the host formulas -------------------------------------------------------------------------------------------------------
SMALL = [(k, c) for k, c in ld.ALL if c[2] <= ld.CORRCOEF_MAX_J]


@pytest.mark.parametrize("kind,case", SMALL, ids=[c[0] for _, c in SMALL])
def test_pair_q3_host_agrees_with_corrcoef(kind, case):
    """pair_q3_host over the oracle's tables against np.corrcoef over the persons who answered both items, pair by pair: the
    closed form IS the correlation.  Compared where the pair has its 8 persons and both variances are not rounding (v / n > 1e-9;
    a variance that is zero up to rounding is NaN in one and may be +-1e-17 in the other); below 8 persons both give NaN."""
    from vipsy_amd.grid import pair_q3_host
    o = ld.oracle(kind, case)
    got = pair_q3_host(o["n"], o["s"], o["ss"], o["sp"], min_pairs=8)
    want = ld.q3_corrcoef(o)
    assert got.dtype == np.float64 and got.shape == want.shape
    n, v = o["n"], o["v"]
    with np.errstate(divide="ignore", invalid="ignore"):
        clear = (n >= 8) & (np.where(n > 0, v / n, 0) > 1e-9) & (np.where(n > 0, v.T / n, 0) > 1e-9)
    assert np.isfinite(got[clear]).all() and np.isfinite(want[clear]).all()
    err = np.abs(got[clear] - want[clear]).max() if clear.any() else 0.0
    print("%s: %d of %d entries compared, |q3 - corrcoef| <= %.2e" % (case[0], clear.sum(), clear.size, err))
    assert err <= 1e-10
    assert np.isnan(got[n < 8]).all() and np.isnan(want[n < 8]).all()
    d = np.arange(len(n))
    assert (got[d, d][clear[d, d]] == 1.0).all()
    assert np.array_equal(got, got.T, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(o["q3"])) and np.allclose(got, o["q3"], rtol=0, atol=1e-12, equal_nan=True)


def test_pair_q3_host_nan_rules():
    """NaN below min_pairs, at zero variance and for an item nobody answered; min_pairs moves the line."""
    from vipsy_amd.grid import pair_q3_host, pair_q3_summary
    rng = np.random.RandomState(4)
    N, J = 40, 5
    y = (rng.uniform(size=(N, J)) < 0.5).astype(np.uint8)
    y[:, 3] = 255                                                   # nobody answered item 3
    y[:, 4] = 1                                                     # everybody answered item 4 alike: no spread at a constant P
    y[6:, 2] = 255                                                  # six persons answered item 2
    y[:6, 2] = [0, 1, 0, 1, 1, 0]
    t = ld.tables(y, np.full((N, J), 0.4))
    q8 = pair_q3_host(t["n"], t["s"], t["ss"], t["sp"], 8)
    q2 = pair_q3_host(t["n"], t["s"], t["ss"], t["sp"], 2)
    assert np.isnan(q8[3]).all() and np.isnan(q8[:, 3]).all() and np.isnan(q2[3]).all()
    assert np.isnan(q8[4]).all() and np.isnan(q8[:, 4]).all() and np.isnan(q2[4]).all()
    assert np.isnan(q8[2]).all() and np.isnan(q8[:, 2]).all()
    assert np.isfinite(q2[2, :3]).all() and q2[2, 2] == 1.0
    assert np.isfinite(q8[:2, :2]).all() and q8[0, 0] == 1.0 and q8[1, 1] == 1.0
    assert abs(q8[0, 1] - np.corrcoef(t["r"][:, 0], t["r"][:, 1])[0, 1]) <= 1e-12
    s = pair_q3_summary(q8, top=20)
    assert len(s["item_j"]) == 1 and (s["item_j"][0], s["item_k"][0]) == (0, 1) and s["value"][0] == q8[0, 1]
    assert s["mean"] == q8[0, 1] and s["max"] == 0.0
    e = pair_q3_summary(np.full((3, 3), np.nan))
    assert np.isnan(e["mean"]) and np.isnan(e["max"]) and len(e["item_j"]) == 0
    with pytest.raises(ValueError):
        pair_q3_host(t["n"], t["s"][:4], t["ss"], t["sp"], 8)


@pytest.mark.parametrize("bad", [1, 0, -3, 2.5, True, None, "8"])
def test_min_pairs_is_validated(bad):
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", backend=OracleBackend())
    with pytest.raises(ValueError) as e:
        m.local_dependence(min_pairs=bad)
    assert "min_pairs" in str(e.value)
    with pytest.raises(ValueError):
        m.engine.local_dependence(top=-1)


# ---- the oracle: the planted case, the conditions and their caps ---------------------------------------------------------
def test_planted_pair_in_the_oracle():
    """q3_2pl_n5000_j70_ld in float64: the planted pair stands at about 0.80 (measured 0.803), every other |q3| stays below 0.1
    (0.090) and the mean sits within 0.005 of Yen's -1 / (J - 1) (-0.0153 against -0.0145)."""
    o = ld.oracle(*PLANTED)
    q3 = o["q3"]
    J = len(q3)
    assert np.isfinite(q3).all()
    rest = np.abs(q3[~np.eye(J, dtype=bool)].copy().reshape(J, J - 1))
    other = np.abs(q3.copy())
    other[[0, 1], [1, 0]] = 0
    other[np.arange(J), np.arange(J)] = 0
    print("planted: q3[0][1] %.4f, largest other |q3| %.4f, mean %.5f (-1/69 = %.5f), n min %d, v/n min %.3f"
          % (q3[0, 1], other.max(), o["mean"], -1 / 69.0, o["n"].min(), (o["v"] / o["n"]).min()))
    assert abs(q3[0, 1] - 0.80) <= 0.01 and q3[0, 1] == q3[1, 0] and rest.max() == abs(q3[0, 1])
    assert other.max() < 0.1
    assert abs(o["mean"] - (-1 / 69.0)) <= 0.005
    assert abs(o["max"] - (q3[0, 1] - o["mean"])) <= 1e-15
    from vipsy_amd.grid import pair_q3_summary
    s = pair_q3_summary(q3, top=20)
    assert (s["item_j"][0], s["item_k"][0]) == (0, 1) and len(s["value"]) == 20 and (s["item_j"] < s["item_k"]).all()
    assert s["mean"] == pytest.approx(o["mean"], abs=1e-15) and s["max"] == pytest.approx(o["max"], abs=1e-15)
    assert (np.diff(np.abs(s["value"] - s["mean"])) <= 0).all()


@pytest.mark.parametrize("kind,case", ld.ALL, ids=ld.ALL_IDS)
def test_comparison_condition_and_its_cap(kind, case):
    """The condition of the q3 comparison (oracle n >= 8, both oracle v / n > 0.01) leaves out no more than the case's cap:
    nothing, except 40 % at most of case3_1pl_j130 (thresholds spread over [-4, 4]: items nearly everybody answers alike) and
    case4_3pl_j500_sparse, whose pairs share two persons on average: tables only."""
    o = ld.oracle(kind, case)
    J = len(o["n"])
    kept = o["keep"].sum() / float(J * (J - 1))
    cap = ld.LEFT_OUT_CAP.get(case[0], 0.0)
    print("%s: kept %.3f of the off-diagonal pairs (cap on left out: %s); n min %d" % (case[0], kept, cap, o["n"].min()))
    assert (o["n"] == o["n"].T).all() and (o["n"] == np.rint(o["n"])).all() and np.abs(o["sp"] - o["sp"].T).max() <= 1e-12
    if cap is None:
        assert kept < 0.01
    else:
        assert 1.0 - kept <= cap
        assert np.isfinite(o["q3"][o["keep"]]).all()
    if case[0] == ld.PLANTED[0]:
        assert o["n"].min() >= 3000 and (o["v"] / o["n"]).min() > 0.05


@pytest.mark.parametrize("kind,case", ld.ALL, ids=ld.ALL_IDS)
def test_the_method_leaves_a_wide_margin_under_the_row_rule(kind, case):
    """The kernels' arithmetic in float32 + fp16 pairs at scale 2^10 (ld_cases.restated_f32) against the float64 oracle: n exact,
    s, ss, sp within a third of the row rule, q3 under the comparison condition within a third of ROW_TOL.  Printed."""
    o, r = ld.oracle(kind, case), ld.restated_f32(kind, case)
    assert np.array_equal(r["n"].astype(np.float64), o["n"])
    e = {k: ld.row_error(r[k], o[k]) for k in ("s", "ss", "sp")}
    keep = o["keep"]
    tables_only = ld.LEFT_OUT_CAP.get(case[0], 0.0) is None
    e_q = 0.0 if tables_only or not keep.any() else float(np.abs(r["q3"][keep] - o["q3"][keep]).max())
    print("%s: s %.2e ss %.2e sp %.2e by the row rule, q3 %.2e on %d pairs%s"
          % (case[0], e["s"], e["ss"], e["sp"], e_q, keep.sum(), " (tables only)" if tables_only else ""))
    assert max(e.values()) <= ROW_TOL / 3
    assert e_q <= ROW_TOL / 3


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _y(n=24, j=12, seed=2):
    return torch.from_numpy((np.random.RandomState(seed).uniform(size=(n, j)) < 0.5).astype(np.uint8))


def test_classes_without_grid_scores_refuse():
    from vipsy_amd import vi
    vi.clear_param_store()
    q = torch.from_numpy(sc.cdm_q(3, 12, np.random.RandomState(2)))
    for cls in (vi.VCHoDina, vi.VaeCCDM, vi.VCDM):
        m = cls(data=_y(), q=q, backend=OracleBackend())
        for call in (m.residual_sums, m.local_dependence):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert type(m.engine).__name__ in str(e.value)


def test_four_dimensions_refuse_with_the_wording_of_score():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_2pl", x_feature=4, backend=OracleBackend())
    with pytest.raises(NotImplementedError) as want:
        m.engine.score()
    for call in (m.residual_sums, m.local_dependence):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == str(want.value) and "x_feature" in str(e.value)


def test_bad_data_is_refused_before_anything_is_computed():
    from vipsy_amd import vi
    vi.clear_param_store()
    m = vi.VIRT(data=_y(), model="irt_3pl", backend=OracleBackend())
    with pytest.raises(ValueError):
        m.local_dependence(data=_y(j=11))
    with pytest.raises(IndexError):
        m.engine.residual_sums(rows=[0, 24])
    with pytest.raises(ValueError):
        m.local_dependence(nodes=1)


def test_two_ranks_refuse(tmp_path):
    """A gloo group of two: the model class and the engine both refuse, before anything is computed."""
    worker = os.path.join(ROOT, "tests", "_ld_dist_worker.py")
    out = str(tmp_path / "ld_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29655", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29655", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            assert f.read().split() == ["NotImplementedError"] * 4
