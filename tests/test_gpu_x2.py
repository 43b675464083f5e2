"""Pairwise 2 x 2 tables and LD X2 on the GPU: vx_pair_tables at the ABI, IrtEngine / CcdmEngine.pair_tables and .ld_x2 and the
model classes' methods against the float64 oracle of tests/x2_cases.py.

Rules.  The tables are integers: every entry equals the int64 numpy product of the indicators, bit for bit, and the relations
between the tables hold as integers.  ld_x2(): on the pairs of the comparison condition (oracle N >= 8, all four oracle E >= 1;
x2_cases.condition, whose share tests/test_x2_host.py asserts on the CPU) every expected count is within REL_E of the oracle's,
relatively, and |x2 - oracle| <= REL_E * sum_ab (2 |O - E| + (O - E)^2 / E) -- the relative bound on E carried through d x2 / d E.
REL_E = 64 * 2^-24 comes from the precision of the operand image (x2_cases); the image said again in numpy stays below 3 units.
A case of x2_cases.TABLES_ONLY is compared on its tables only.  What is found is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import ld_cases as ld
from tests import x2_cases as xc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

TABLES = ("n11", "n10", "n01", "n00")
N_EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
N_TWO_CHUNKS = 200               # two stages of 128 persons: two person chunks a pair of item groups (asserted off the plan)


def _abi(y, rows=None, be=None):
    """vx_pair_tables on a HipBackend alone: no engine.  The tables start as garbage: every entry has to be written."""
    from vipsy_amd.engine import HipBackend
    be = be or HipBackend()
    dev = _dev()
    yd = y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    J = int(yd.shape[1])
    rd = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).to(dev)
    n = int(yd.shape[0]) if rd is None else int(rd.numel())
    out = {k: torch.full((J, J), -7, dtype=torch.int32, device=dev) for k in TABLES}
    assert be.pair_tables_workspace(n, J) == 0
    be.pair_tables(yd, rd, n, J, out["n11"], out["n10"], out["n01"], out["n00"], None, 0)
    torch.cuda.synchronize()
    return out


def _hold(tag, got, y):
    want = xc.tables(np.asarray(y))
    for k in TABLES:
        g = _np(got[k])
        assert g.dtype == np.int32 and g.shape == want[k].shape, (tag, k)
        bad = int((g.astype(np.int64) != want[k]).sum())
        assert bad == 0, "%s: %s differs in %d of %d entries" % (tag, k, bad, g.size)


def _mixed(n, J, seed):
    """0 / 1 answers with the bytes 2, 253, 254 and 255 mixed in."""
    rng = np.random.RandomState(seed)
    y = (rng.uniform(size=(n, J)) < 0.6).astype(np.uint8)
    hole = rng.uniform(size=(n, J))
    for lo, byte in ((0.00, 255), (0.10, 254), (0.14, 253), (0.18, 2)):
        y[(hole >= lo) & (hole < lo + 0.04 + 0.06 * (byte == 255))] = byte
    return y


# ---- the tables, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 31, 32, 33, 70, 129, 300])
def test_tables_bit_for_bit(J):
    """One tile, the tile edge, three tiles, two and three groups of 128 items (pairs of different groups add their transpose
    partners); one person to 65 and two person chunks a group pair.  J = 32 and 300 are read a dword a lane, the others by
    bytes."""
    from vipsy_amd.engine import HipBackend
    be = HipBackend()
    assert be.pair_tables_chunks(N_TWO_CHUNKS, J) == 2 and be.pair_tables_chunks(128, J) == 1
    for n in (N_EDGES if J <= 70 else (1, 33, 65)) + (N_TWO_CHUNKS,):
        y = _mixed(n, J, 100 + J + n)
        assert n * J < 400 or {0, 1, 2, 253, 254, 255} <= set(np.unique(y).tolist())
        _hold("J %d n %d" % (J, n), _abi(y, be=be), y)


def test_special_matrices():
    """An item nobody answered, a block of 64 consecutive persons without a response, all ones, all zeros, nothing observed."""
    y = _mixed(333, 70, 7)
    y[:, 11] = 255
    y[130:194] = 254
    got = _abi(y)
    _hold("holes", got, y)
    for k in TABLES:
        assert int(got[k][11].abs().sum()) == 0 and int(got[k][:, 11].abs().sum()) == 0, k
    for byte, full in ((1, "n11"), (0, "n00")):
        y = np.full((150, 33), byte, np.uint8)
        got = _abi(y)
        _hold("all %d" % byte, got, y)
        for k in TABLES:
            assert bool((got[k] == (150 if k == full else 0)).all()), (byte, k)
    y = np.full((150, 33), 255, np.uint8)
    _hold("nothing observed", _abi(y), y)


def test_relations_as_integers_and_the_count_of_residual_sums():
    kind, case = "irt", ld.PLANTED
    cs = xc.case_of(kind, case)
    eng = _irt_engine(cs)
    t = eng.pair_tables()
    torch.cuda.synchronize()
    assert set(t) == set(TABLES) and all(v.dtype == torch.int32 and v.is_cuda and tuple(v.shape) == (70, 70) for v in t.values())
    _hold("planted, engine", t, cs["y"])
    assert torch.equal(t["n11"], t["n11"].t()) and torch.equal(t["n00"], t["n00"].t()) and torch.equal(t["n10"], t["n01"].t())
    assert int(t["n10"].diagonal().abs().sum()) == 0 and int(t["n01"].diagonal().abs().sum()) == 0
    assert np.array_equal(_np(t["n11"].diagonal()), (cs["y"] == 1).sum(0)) and np.array_equal(_np(t["n00"].diagonal()), (cs["y"] == 0).sum(0))
    n = eng.residual_sums(nodes=cs["nodes"], span=cs["span"])["n"]
    total = t["n11"] + t["n10"] + t["n01"] + t["n00"]
    assert torch.equal(total.to(torch.float32), n) and torch.equal(total, n.to(torch.int32))


def test_rows_equal_the_same_rows_passed_as_data():
    """A shuffled subset with a repeated row against the same rows handed over as data, bit for bit; the same call twice."""
    cs = xc.case_of("irt", ld.PLANTED)
    eng = _irt_engine(cs)
    sub = np.random.RandomState(5).permutation(cs["N"])[:1301].astype(np.int64)
    sub[-1] = sub[0]
    a = eng.pair_tables(rows=torch.from_numpy(sub).to(_dev()))
    b = eng.pair_tables(y_u8=torch.from_numpy(np.ascontiguousarray(cs["y"][sub])))
    c = eng.pair_tables(rows=sub)
    torch.cuda.synchronize()
    for k in TABLES:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    _hold("rows", a, cs["y"][sub])
    # at the ABI, by bytes and by dwords
    for J in (33, 36):
        y = _mixed(500, J, 9)
        rows = np.random.RandomState(6).randint(0, 500, size=777)
        _hold("rows at the ABI, J %d" % J, _abi(y, rows), y[rows])


def test_counts_beyond_what_float32_holds():
    """2^24 + 3 persons, two items, all ones: every entry of n11 is 2^24 + 3 exactly."""
    n = 2 ** 24 + 3
    got = _abi(torch.ones(n, 2, dtype=torch.uint8, device=_dev()))
    assert bool((got["n11"] == n).all())
    for k in ("n10", "n01", "n00"):
        assert int(got[k].abs().sum()) == 0, k


# ---- classes and padding ---------------------------------------------------------------------------------------------------
def test_model_classes_and_padding():
    """VCCDM and a padded VaeIRT (37 items, 150 persons, hidden_dim 24: phantom items) count the model's own items and persons;
    VaeIRT with x_feature = 4 is served -- no grid is needed; fit(8), pair_tables(), fit(8) leaves the bits of fit(16)."""
    from tests import score_cases as sc
    from vipsy_amd import vi
    rng = np.random.RandomState(33)
    J = 37
    y = (rng.uniform(size=(150, J)) < 0.55).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.15] = 255

    def run(interrupt):
        vi.clear_param_store()
        m = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=1, hidden_dim=24, seed=5)
        opt = vi.Adam({"lr": 1e-2})
        mid = None
        if interrupt:
            m.fit(optim=opt, max_iter=8, progress=False)
            mid = m.pair_tables()
            m.fit(optim=opt, max_iter=8, progress=False)
        else:
            m.fit(optim=opt, max_iter=16, progress=False)
        torch.cuda.synchronize()
        eng = m.engine
        return (eng.P.clone(), eng.M.clone(), eng.V.clone()), mid, eng

    a, mid, eng = run(True)
    b, _, _ = run(False)
    assert eng.J_items == J and eng.J > J
    for x, z in zip(a, b):
        assert torch.equal(x, z)
    _hold("padded VaeIRT", mid, y)
    vi.clear_param_store()
    y30 = y[:, :30].copy()
    m = vi.VCCDM(data=torch.from_numpy(y30).to(_dev()), q=torch.from_numpy(sc.cdm_q(3, 30, rng)))
    _hold("VCCDM", m.pair_tables(), y30)
    out = m.ld_x2(top=3)
    assert out["x2"].shape == (30, 30) and len(out["value"]) == 3
    vi.clear_param_store()
    m4 = vi.VaeIRT(data=torch.from_numpy(y).to(_dev()), model="irt_2pl", x_feature=4)
    _hold("x_feature 4", m4.pair_tables(), y)
    data = y[:70].astype(np.float32)
    data[y[:70] == 255] = np.nan
    _hold("x_feature 4, float data with NaN", m4.pair_tables(data=torch.from_numpy(data)), y[:70])
    with pytest.raises(NotImplementedError):
        m4.ld_x2()
    for other in (vi.VCHoDina(data=torch.from_numpy(y30).to(_dev()), q=torch.from_numpy(sc.cdm_q(3, 30, rng))),):
        with pytest.raises(NotImplementedError):
            other.pair_tables()


# ---- ld_x2 end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", xc.ALL, ids=xc.ALL_IDS)
def test_ld_x2_against_the_oracle(kind, case):
    cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
    eng = _ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs)
    kw = {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}
    _hold(case[0], eng.pair_tables(), cs["y"])
    out = eng.ld_x2(**kw)
    J = cs["J"]
    assert set(out) == {"x2", "g2", "z", "p", "sign", "phi_obs", "phi_exp", "n_pairs", "expected", "item_j", "item_k", "value", "sign_top"}
    for k in ("x2", "g2", "z", "p", "sign", "phi_obs", "phi_exp"):
        assert out[k].shape == (J, J) and out[k].dtype == np.float64 and np.array_equal(out[k], out[k].T, equal_nan=True), k
    assert out["n_pairs"].dtype == np.int64 and np.array_equal(out["n_pairs"], o["N"].astype(np.int64))
    assert out["expected"].shape == (2, 2, J, J)
    assert np.isnan(np.diag(out["x2"])).all() and np.isnan(out["x2"][o["N"] < 8]).all()
    if case[0] in xc.TABLES_ONLY:
        return
    keep = o["keep"]
    rel_e, ratio = xc.ratios(o, out["x2"], out["expected"])
    print("%s: E %.2f, x2 ratio %.2f units of 2^-24 on %d of %d off-diagonal pairs (the constant: %.0f)"
          % (case[0], rel_e / xc.UNIT, ratio / xc.UNIT, keep.sum(), J * (J - 1), xc.REL_E / xc.UNIT))
    assert np.isfinite(out["x2"][keep & (o["E"].min((0, 1)) > 1.0 + 1e-4)]).all()
    fin = keep & np.isfinite(out["x2"])
    assert rel_e <= xc.REL_E, (case[0], rel_e)
    assert np.isfinite(ratio) and ratio <= xc.REL_E, (case[0], ratio)
    # g2 moves with E as x2 does, to first order by sum |O / E - 1| dE; the same constant on sum_ab |O - E| + the x2 rule
    d_g2 = np.abs(out["g2"][fin] - o["g2"][fin])
    rule = xc.REL_E * (2.0 * np.abs(o["O"] - o["E"])).sum((0, 1))[fin] + xc.X2_FLOOR
    assert (d_g2 <= rule).all(), (case[0], float((d_g2 / rule).max()))
    clear = np.isfinite(o["phi_obs"]) & (np.abs(o["phi_obs"] - o["phi_exp"]) > 1e-4) & fin
    assert np.array_equal(out["sign"][clear], o["sign"][clear])
    assert np.array_equal(out["value"], out["x2"][out["item_j"], out["item_k"]]) and (out["item_j"] < out["item_k"]).all()
    assert (np.diff(out["value"]) <= 0).all() and len(out["value"]) == min(20, int(np.isfinite(out["x2"]).sum()) // 2)


def test_the_planted_pair_comes_first_through_the_model_class():
    from vipsy_amd import vi
    kind, case = "irt", ld.PLANTED
    cs, o = xc.case_of(kind, case), xc.oracle(kind, case)
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1, seed=7)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    out = m.ld_x2()
    print("planted, VIRT.ld_x2(): x2[0][1] %.1f (oracle %.1f) sign %+d, next %.2f" % (out["value"][0], o["x2"][0, 1], out["sign_top"][0],
                                                                                    out["value"][1]))
    assert (out["item_j"][0], out["item_k"][0]) == (0, 1) and out["sign_top"][0] == 1 and out["sign"][0, 1] == 1
    assert abs(out["value"][0] - o["x2"][0, 1]) <= 1e-4 * o["x2"][0, 1] and out["value"][0] > 20 * out["value"][1]
    assert out["p"][0, 1] < 1e-100 and out["z"][0, 1] == (out["x2"][0, 1] - 1) / np.sqrt(2)
    # new respondents as float data with NaN, and top / min_pairs / min_expected reach the engine
    data = cs["y"][:700].astype(np.float32)
    data[cs["y"][:700] == 255] = np.nan
    new = m.ld_x2(data=torch.from_numpy(data), top=3, min_pairs=430, min_expected=2.0)
    assert len(new["value"]) == 3 and (new["item_j"][0], new["item_k"][0]) == (0, 1)
    off = ~np.eye(70, dtype=bool)
    assert np.array_equal(np.isnan(new["x2"])[off], ((new["n_pairs"] < 430) | (new["expected"].min((0, 1)) < 2.0))[off])
    assert np.isnan(new["x2"]).sum() > 70
    with pytest.raises(ValueError):
        m.ld_x2(data=cs["y"][:, :69])
