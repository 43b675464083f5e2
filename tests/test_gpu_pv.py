"""Plausible values on the GPU (vx_grid_draw behind IrtEngine.plausible_values, CcdmEngine.plausible_values and the model
classes' plausible_values()) against the float64 oracle draws of tests/pv_cases.py: the numpy restatement of the Philox / Gumbel
noise over f = logw + ll of tests/score_cases.py.  tests/test_pv_host.py checks on the CPU that those oracle draws sample the
posterior; here the kernel has to reproduce them draw for draw.

A drawn node must equal the oracle's wherever the oracle's best and second-best perturbed value differ by more than ARGMAX_GAP
(1e-4); at most ARGMAX_LEFT_OUT (2 %) of the (person, draw) pairs may be left out by that rule.  The engines, cases and shapes
are those of tests/test_gpu_score.py: one person tile + 1 row, ragged J and G (case 1), 32 item chunks (4), odd and even
numbers of node tiles (5: 14 and 23; 6: 1 and 32), a wave's second person tile partly empty."""
import numpy as np
import pytest
import torch

from tests import pv_cases as pv
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ALL_CASES = sc.IRT_CASES + sc.CDM_CASES


def _engine(case):
    cs = pv.posterior_f(case)[0]
    if case in sc.IRT_CASES:
        return cs, _irt_engine(cs), {"nodes": cs["nodes"], "span": cs["span"]}, ("theta", "node")
    return cs, _ccdm_engine(cs), {}, ("attr", "pattern")


def _hold_draws(tag, got_node, want_node, gap):
    sure = gap > sc.ARGMAX_GAP
    out = 1.0 - float(sure.mean())
    wrong = np.argwhere(sure & (got_node.astype(np.int64) != want_node))
    print("%s: %.3f %% of the (person, draw) pairs left out of the argmax rule, %d wrong draws of %d"
          % (tag, 100 * out, len(wrong), sure.size))
    assert out <= sc.ARGMAX_LEFT_OUT, (tag, out)
    assert len(wrong) == 0, (tag, wrong[:10], [(int(got_node[i, k]), int(want_node[i, k]), float(gap[i, k])) for i, k in wrong[:10]])


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_draws_vs_oracle(case):
    cs, eng, grid_kw, (coord_k, node_k) = _engine(case)
    _, _, coord, _ = pv.posterior_f(case)
    want_node, gap = pv.oracle_draws(case)
    got = eng.plausible_values(draws=pv.DRAWS, seed=pv.SEED, **grid_kw)
    torch.cuda.synchronize()
    node, val = _np(got[node_k]), _np(got[coord_k])
    assert node.dtype == np.int32 and node.shape == (cs["N"], pv.DRAWS)
    assert val.dtype == np.float32 and val.shape == (cs["N"], pv.DRAWS, coord.shape[1])
    assert node.min() >= 0 and node.max() < coord.shape[0]
    _hold_draws(cs["name"], node, want_node, gap)
    assert np.array_equal(val, coord.astype(np.float32)[node])              # the grid's own coordinates, bit for bit


def test_more_draws_extend_fewer_and_repeat():
    """37 draws cross the 16 of one launch and are no multiple of 4."""
    for case, k in ((sc.IRT_CASES[4], "node"), (sc.CDM_CASES[1], "pattern")):
        cs, eng, grid_kw, _ = _engine(case)
        a = eng.plausible_values(draws=37, seed=pv.SEED, **grid_kw)
        b = eng.plausible_values(draws=37, seed=pv.SEED, **grid_kw)
        c = eng.plausible_values(draws=5, seed=pv.SEED, **grid_kw)
        torch.cuda.synchronize()
        assert a[k].shape == (cs["N"], 37) and c[k].shape == (cs["N"], 5)
        for key in a:
            assert torch.equal(a[key], b[key]), key
            assert torch.equal(a[key][:, :5], c[key]), key


def test_rows_are_keyed_by_their_index_and_seeds_differ():
    case = sc.IRT_CASES[4]                                                    # case 5: D = 2, 441 nodes, 100 persons
    cs, eng, grid_kw, _ = _engine(case)
    idx = np.array([99, 3, 3, 64, 31, 32, 0, 98, 17, 5, 50, 63, 65, 3, 77, 12, 40, 41, 42, 96, 2, 1, 88, 70, 33, 34, 35,
                    36, 9, 8, 7, 66, 67, 68, 69, 20, 21], dtype=np.int64)
    assert len(np.unique(idx)) < len(idx) and (np.diff(idx) < 0).any()
    full = eng.plausible_values(draws=pv.DRAWS, seed=pv.SEED, **grid_kw)
    sub = eng.plausible_values(rows=torch.from_numpy(idx).to(_dev()), draws=pv.DRAWS, seed=pv.SEED, **grid_kw)
    other = eng.plausible_values(draws=pv.DRAWS, seed=pv.SEED + 1, **grid_kw)
    # the same responses handed in as new data: keyed by their index there, which is the same index
    again = eng.plausible_values(torch.from_numpy(cs["y"]), draws=pv.DRAWS, seed=pv.SEED, **grid_kw)
    torch.cuda.synchronize()
    for key in ("theta", "node"):
        assert torch.equal(sub[key], full[key][torch.from_numpy(idx).to(_dev())]), key
        assert torch.equal(again[key], full[key]), key
    changed = float((other["node"] != full["node"]).float().mean())
    print("case 5: another seed changes %.1f %% of the draws" % (100 * changed))
    assert changed >= 0.5


def test_a_waves_second_unit_starts_clean():
    """sc.second_unit_case: two waves take a second unit.  The draws of the last 97 rows behind the others are the bits of the
    call that takes those rows alone (`rows`: keyed by the same row index), and both are the oracle's draws."""
    from vipsy_amd.engine import score_grid
    cs, _ = sc.second_unit_case(torch.cuda.get_device_properties(_dev()).multi_processor_count)
    eng = _irt_engine(cs)
    kw = dict(draws=5, seed=pv.SEED, nodes=cs["nodes"], span=cs["span"])
    full = eng.plausible_values(**kw)
    tail = torch.from_numpy(cs["tail"]).to(_dev())
    alone = eng.plausible_values(rows=tail, **kw)
    torch.cuda.synchronize()
    assert full["node"].shape == (cs["N"], 5) and alone["node"].shape == (sc.SECOND_UNIT_TAIL, 5)
    for key in ("theta", "node"):
        assert torch.equal(full[key][tail], alone[key]), key
    theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
    f = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y_tail"]) + logw.astype(np.float64)[None, :]
    want_node, gap = pv.draw(f, pv.gumbel(pv.SEED, cs["tail"], len(logw), 5))
    _hold_draws(cs["name"], _np(alone["node"]), want_node, gap)
    assert np.array_equal(_np(alone["theta"])[:, :, 0], theta[:, 0][_np(alone["node"])])


def test_pure_noise_on_1024_equal_nodes():
    """65 rows without a response over 1 024 equally weighted nodes: f is one constant, every draw is the argmax of the noise
    alone -- the counter layout over all 32 node tiles and both tails of the noise."""
    from vipsy_amd.engine import IrtEngine
    G, N = 1024, 65
    y = np.full((N, 24), 255, dtype=np.uint8)
    eng = IrtEngine(torch.from_numpy(y).to(_dev()), model="irt_2pl", D=1, seed=3)
    theta = np.linspace(-4.0, 4.0, G).astype(np.float32)
    logw = np.full(G, -np.log(G), dtype=np.float32)
    got = eng.plausible_values(draws=pv.DRAWS, seed=pv.SEED, nodes=(theta, logw))
    torch.cuda.synchronize()
    noise = pv.gumbel(pv.SEED, np.arange(N), G, pv.DRAWS)
    want_node, gap = pv.draw(np.zeros((N, G)), noise)
    _hold_draws("pure noise", _np(got["node"]), want_node, gap)
    assert len(np.unique(want_node >> 5)) == 32                               # every node tile wins somewhere
    assert np.array_equal(_np(got["theta"])[:, :, 0], theta[_np(got["node"])])


def test_mean_of_the_draws_agrees_with_score():
    case = sc.IRT_CASES[0]
    cs, eng, grid_kw, _ = _engine(case)
    M = 1024
    got = eng.plausible_values(draws=M, seed=pv.SEED, **grid_kw)
    s = eng.score(**grid_kw)
    torch.cuda.synchronize()
    mean = _np(got["theta"]).astype(np.float64)[:, :, 0].mean(1)
    z = np.abs(mean - _np(s["eap"])[:, 0]) / (_np(s["psd"])[:, 0] / np.sqrt(M))
    print("case 1, %d draws: the mean drawn theta is at most %.2f standard errors from score()'s EAP" % (M, z.max()))
    assert (z <= 5.0).all(), (int(z.argmax()), float(z.max()))


def test_model_classes_follow_the_data_contract():
    from vipsy_amd import vi
    rng = np.random.RandomState(4)
    cs = pv.posterior_f(sc.IRT_CASES[0])[0]
    new = cs["y"].astype(np.float32)
    new[cs["y"] == 255] = np.nan
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(new).to(_dev()), model="irt_2pl", x_feature=1, seed=7)
    other = (rng.uniform(size=(50, cs["J"])) < 0.5).astype(np.float32)
    other[rng.uniform(size=other.shape) < 0.2] = np.nan
    got = m.plausible_values(data=torch.from_numpy(other), draws=7, seed=3)
    want = m.engine.plausible_values(torch.from_numpy(np.where(np.isnan(other), 255, other).astype(np.uint8)), draws=7, seed=3)
    own = m.plausible_values(draws=7, seed=3)
    torch.cuda.synchronize()
    assert got["theta"].shape == (50, 7, 1) and own["node"].shape == (cs["N"], 7)
    for key in ("theta", "node"):
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError):
        m.plausible_values(data=torch.from_numpy(other[:, :36]))

    cc = pv.posterior_f(sc.CDM_CASES[0])[0]
    data = cc["y"].astype(np.float32)
    data[cc["y"] == 255] = np.nan
    vi.clear_param_store()
    c = vi.VCCDM(data=torch.from_numpy(data).to(_dev()), q=torch.from_numpy(cc["q"]), model=cc["cdm"])
    got = c.plausible_values(data=torch.from_numpy(data[:37]), draws=6, seed=9)
    want = c.engine.plausible_values(torch.from_numpy(cc["y"][:37]), draws=6, seed=9)
    torch.cuda.synchronize()
    assert got["attr"].shape == (37, 6, cc["K"]) and got["pattern"].dtype == torch.int32
    for key in ("attr", "pattern"):
        assert torch.equal(got[key], want[key]), key


def test_refusals():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VIRT(data=yd, model="irt_2pl", x_feature=4)):
        with pytest.raises(NotImplementedError) as e:
            m.plausible_values()
        assert len(str(e.value)) > 20
    for m in (vi.VIRT(data=yd, model="irt_2pl", x_feature=1), vi.VCCDM(data=yd, q=torch.from_numpy(q))):
        for kw in ({"draws": 0}, {"draws": 1025}, {"seed": -1}, {"seed": 2 ** 64}, {"draws": 2.5}, {"draws": True}):
            with pytest.raises(ValueError):
                m.plausible_values(**kw)
        assert m.plausible_values(draws=1, seed=2 ** 64 - 1)[("node" if "VIRT" in type(m).__name__ else "pattern")].shape == (64, 1)
