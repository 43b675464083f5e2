"""Host-side logic of the engine that needs no GPU: the observed-cell lists of the D = 1 list kernel (their layout is an ABI
contract, include/vipsy_amd.h) and the O(B) subsample of small minibatches."""
import numpy as np
import torch

from tests.oracle_backend import OracleBackend
from vipsy_amd.engine import IrtEngine


def _decode_lists(sp, n, J):
    """Rebuild the response matrix from pidx / pent / glen exactly as k_irt1d_sp walks them."""
    pent = sp["pent"].cpu().numpy().view(np.uint16)            # [ng][Lq][64][4]
    pidx = sp["pidx"].cpu().numpy()
    glen = sp["glen"].cpu().numpy()
    ng, Lq = pent.shape[0], pent.shape[1]
    assert pent.shape == (ng, Lq, 64, 4) and pidx.shape == (ng * 64,) and glen.shape == (ng,)
    y = np.full((n, J), 255, dtype=np.uint8)
    seen = np.zeros(n, dtype=bool)
    for g in range(ng):
        for lane in range(64):
            i = pidx[g * 64 + lane]
            codes = pent[g, :, lane, :].reshape(-1)
            if i < 0:
                assert (codes == 0xFFFF).all()                  # an empty slot has an empty list
                continue
            assert not seen[i]
            seen[i] = True
            live = codes != 0xFFFF
            k = int(live.sum())
            assert live[:k].all() and k <= 4 * glen[g]          # the list is a prefix; the group's quad count covers it
            items = (codes[:k] & 0x7FFF).astype(int)
            assert (np.diff(items) > 0).all()                   # ascending items, each once
            y[i, items] = (codes[:k] >> 15).astype(np.uint8)
    assert seen.all()
    return y


def test_observed_cell_lists_encode_the_responses():
    rng = np.random.RandomState(0)
    for n, J, miss in ((300, 37, 0.9), (5000, 12, 0.6), (64, 500, 0.95), (65, 8, 0.999)):
        y = rng.randint(0, 2, size=(n, J)).astype(np.uint8)
        y[rng.rand(n, J) < miss] = 255
        eng = IrtEngine(torch.from_numpy(y), model="irt_2pl", D=1, backend=OracleBackend(), observed_lists=True)
        sp = eng._sparse_lists(None)
        assert sp is not None and sp["n_groups"] == (n + 63) // 64
        assert np.array_equal(_decode_lists(sp, n, J), y)
        # slots are sorted by list length inside windows of 4096: the 64 lists of a group end (almost) together
        cnt = (y != 255).sum(1)
        pidx = sp["pidx"].cpu().numpy()
        for w0 in range(0, len(pidx), 4096):
            c = np.array([cnt[i] if i >= 0 else -1 for i in pidx[w0:w0 + 4096]])
            assert (np.diff(c) <= 0).all()
    # structured designs (tests/response_designs.py): booklets of very different length in file order and shuffled, 64 empty
    # persons in a row, a complete case at J = 1024, the degenerate ends -- where the lists of a group do NOT end together
    from tests import design_cases as dc
    for name in ("sorted9000", "shuffled3000", "j1024_complete", "empty_block_small", "all_missing", "single_cell", "hetero_shards"):
        y, facts = dc.design(name)
        n, J = y.shape
        eng = IrtEngine(torch.from_numpy(y), model="irt_2pl", D=1, backend=OracleBackend(), observed_lists=True)
        sp = eng._sparse_lists(None)
        assert sp is not None and sp["n_groups"] == (n + 63) // 64 and sp["missing"] == facts["missing"], name
        assert np.array_equal(_decode_lists(sp, n, J), y), name
        cnt = (y != 255).sum(1)
        pidx, glen = sp["pidx"].cpu().numpy(), sp["glen"].cpu().numpy()
        c = np.where(pidx >= 0, cnt[np.maximum(pidx, 0)], -1)
        for w0 in range(0, len(pidx), 4096):
            assert (np.diff(c[w0:w0 + 4096]) <= 0).all(), name
            assert sorted(pidx[w0:w0 + 4096][pidx[w0:w0 + 4096] >= 0].tolist()) == list(range(w0, min(n, w0 + 4096))), name
        longest = np.maximum(c, 0).reshape(-1, 64).max(1)
        assert np.array_equal(glen, (longest + 3) // 4), name         # the quads of the longest list of each group
        assert np.array_equal(glen == 0, longest == 0), name          # ... none exactly for a group without an observed cell
        assert sp["Lq"] == max(1, (int(cnt.max()) + 3) // 4), name
        if "empty_block" in facts:
            assert int((glen == 0).sum()) >= 1, name                  # the 64 empty persons fill a whole group (with the lone one)
        if name == "j1024_complete":
            assert sp["Lq"] == 256 and glen[0] == 256 and int(np.median(glen)) <= 32      # one complete case sets Lq for all
        if name == "all_missing":
            assert sp["Lq"] == 1 and (glen == 0).all()
        if name == "single_cell":
            assert sp["Lq"] == 1 and glen.tolist() == [1] + [0] * (len(glen) - 1)
        if name in ("shuffled3000", "sorted9000"):
            # lists of one group do not end together: the group at a booklet boundary holds lists of two lengths
            spread = np.array([c[g * 64:(g + 1) * 64].max() - max(0, c[g * 64:(g + 1) * 64].min()) for g in range(len(glen))])
            assert spread.max() >= 30, name
    # mostly observed responses, or a minibatch: no lists
    y = rng.randint(0, 2, size=(100, 10)).astype(np.uint8)
    eng = IrtEngine(torch.from_numpy(y), model="irt_2pl", D=1, backend=OracleBackend(), observed_lists=True)
    assert eng._sparse_lists(None) is None
    assert eng._sparse_lists(torch.arange(10)) is None


def test_small_subsamples_are_distinct_rows_drawn_on_the_host():
    from vipsy_amd import vi
    y = torch.from_numpy(np.random.RandomState(1).randint(0, 2, size=(4000, 6)).astype(np.uint8))
    m = vi.VIRT(data=y, model="irt_2pl", subsample_size=100, backend=OracleBackend(), seed=5)
    draws = [m._subsample() for _ in range(50)]
    for idx, bg in draws:
        a = idx.cpu().numpy()
        assert bg == 100 and a.shape == (100,) and len(set(a.tolist())) == 100 and a.min() >= 0 and a.max() < 4000
    assert len({tuple(d[0].cpu().numpy().tolist()) for d in draws}) == 50            # fresh rows every step
    m2 = vi.VIRT(data=y, model="irt_2pl", subsample_size=100, backend=OracleBackend(), seed=5)
    assert np.array_equal(m2._subsample()[0].cpu().numpy(), draws[0][0].cpu().numpy())   # reproducible from the seed
    hits = np.bincount(np.concatenate([d[0].cpu().numpy() for d in draws]), minlength=4000)
    assert hits.max() <= 8                                     # 5000 draws over 4000 rows: no row is favoured


def test_captured_row_forms_are_bounded():
    """Every distinct (nb, b_global) subsample form would keep a captured graph for ever: beyond
    graph_max_row_forms the least recently used forms are dropped, the most recently used stay."""
    y = torch.from_numpy(np.random.RandomState(2).randint(0, 2, size=(64, 6)).astype(np.uint8))
    eng = IrtEngine(y, model="irt_2pl", D=1, backend=OracleBackend())
    eng._graphs, eng._graph = {}, None
    full = ("full", 64, 64)
    eng._graphs[full] = {"graph": object()}
    for nb in range(1, 21):
        eng._graphs[("rows", nb, 100)] = {"graph": object(), "rows": object()}
        eng._evict_graph_forms()
        if nb == 5:                                            # a form that is used again moves to the recent end
            eng._graphs[("rows", 1, 100)] = eng._graphs.pop(("rows", 1, 100))
    rows_forms = [m for m in eng._graphs if m[0] == "rows"]
    assert len(rows_forms) == eng.graph_max_row_forms == 8
    assert rows_forms == [("rows", nb, 100) for nb in range(13, 21)]
    assert full in eng._graphs                                 # the full-batch form is not a candidate


def test_loss_reaches_the_ring_without_an_optimiser_launch():
    """A step whose optimiser has nothing to launch still files its loss (the ring slot used to be written only
    as a side effect of the first Adam launch)."""
    from vipsy_amd.engine import LrSpec, LOSS_RING
    y = torch.from_numpy(np.random.RandomState(3).randint(0, 2, size=(32, 5)).astype(np.uint8))
    eng = IrtEngine(y, model="irt_2pl", D=1, backend=OracleBackend())
    eng.loss_and_grads(None, None, None, 0)
    want = float(eng.G[eng.n_params])
    eng.names = lambda: []                                     # no trainable replicated segment ...
    eng.per_person = False                                     # ... and no per-person one: apply_optim launches nothing
    eng.apply_optim(LrSpec(1e-2))
    assert float(eng.step_loss()) == want and float(eng.loss_ring[eng.t % LOSS_RING]) == want


def test_pad_batch_host_side():
    """IrtEngine._pad_batch without a device (a stub HipBackend that answers the two layout queries): a subsample that is no
    multiple of 4 grows by indices equal to n_local -- the phantom person behind the shard's own, every response missing in the
    extended copy -- with b_global made explicit, a list entry by entry; and everything it stands down on.  steps() tells
    loss_and_grads how many phantoms the rows carry, and only while it runs."""
    from vipsy_amd.engine import HipBackend, LrSpec

    class _Stub(HipBackend):
        layout, gd_offset, asked = 1, 0, None

        def __init__(self):
            pass

        def mvn_enc_bwd_layout(self, cfg, nb):
            self.asked = nb
            return self.layout

        def mvn_enc_bwd_gd_offset(self, cfg, nb):
            return self.gd_offset

    n, J = 64, 8
    y = torch.from_numpy(np.random.RandomState(6).randint(0, 2, size=(n, J)).astype(np.uint8))

    def mk(be=None, **kw):
        kw = dict({"D": 4, "amortized": True, "H": 64}, **kw)
        return IrtEngine(y, model="irt_2pl", backend=_Stub() if be is None else be, **kw)

    for B, pad in ((50, 2), (1, 3), (2, 2), (3, 1), (61, 3)):
        eng = mk()
        rows = torch.randperm(n)[:B]
        got, bg = eng._pad_batch(rows, None, None)
        assert eng.be.asked == B + pad                          # the layout is asked for the padded count, before anything is padded
        assert bg == B and got.dtype == rows.dtype and got.numel() == B + pad and (B + pad) % 4 == 0
        assert torch.equal(got[:B], rows) and bool((got[B:] == n).all())
        assert tuple(eng._y_ext.shape) == (n + 1, J) and torch.equal(eng._y_ext[:n], eng.y) and bool((eng._y_ext[n] == 255).all())
        assert eng._y_ext_lik is eng._y_ext                     # (no phantom items here: one copy serves the likelihood too)
        assert eng._pad_batch(rows, 1000, None)[1] == 1000      # the caller's b_global stands
    eng = mk()
    lst = [torch.randperm(n)[:10] for _ in range(3)]            # a list (the steps of steps()): entry by entry
    got, bg = eng._pad_batch(lst, None, None)
    assert bg == 10 and len(got) == 3
    for r, g in zip(lst, got):
        assert torch.equal(g[:10], r) and g.tolist()[10:] == [n, n]
    eng = IrtEngine(y[:, :7].contiguous(), model="irt_2pl", D=4, amortized=True, H=64, backend=_Stub())
    eng._pad_batch(torch.arange(10), None, None)                # phantom items: the likelihood's extended copy is its own
    assert eng._y_ext_lik is not eng._y_ext and tuple(eng._y_ext_lik.shape) == (n + 1, eng.J) and bool((eng._y_ext_lik[n] == 255).all())

    rows = torch.arange(10)

    def stands_down(eng, r=rows, eps=None):
        got, bg = eng._pad_batch(r, None, eps)
        return got is r and bg is None and eng._y_ext is None
    assert stands_down(mk(), torch.arange(12))                  # a multiple of 4
    assert stands_down(mk(), None)                              # the full batch
    assert stands_down(mk(), eps=torch.zeros(10, 4))            # the caller's draws
    assert stands_down(mk(be=OracleBackend()))                  # not the HIP backend
    assert stands_down(mk(estimator="score"))
    assert stands_down(mk(amortized=False))                     # the per-person guide
    assert stands_down(mk(D=1))
    assert stands_down(mk(), [torch.arange(10), torch.arange(9)])       # unequal sizes
    off = mk()
    off.pad_batch = False                                       # the seam (VX_PAD_BATCH=0)
    assert stands_down(off)
    for layout, gd in ((0, 0), (1, -1)):                        # the padded count would not run the dimension-major backward
        eng = mk()
        eng.be.layout, eng.be.gd_offset = layout, gd
        assert stands_down(eng)

    # steps(): the phantom count is set for loss_and_grads while the steps run, and cleared behind them -- also when they raise
    eng, seen = mk(), []
    eng.step = lambda lrs, rows=None, b_global=None: seen.append((eng._phantom_rows, int(rows.numel()), b_global))
    eng.use_graph = False
    eng.steps(LrSpec(0.0), [torch.arange(10), torch.arange(10, 20)])
    assert seen == [(2, 12, 10), (2, 12, 10)] and eng._phantom_rows == 0
    seen.clear()
    eng.steps(LrSpec(0.0), [torch.arange(12)], b_global=77)
    assert seen == [(0, 12, 77)] and eng._phantom_rows == 0

    def boom(lrs, rows=None, b_global=None):
        raise KeyError("stop")
    eng.step = boom
    try:
        eng.steps(LrSpec(0.0), [torch.arange(10)])
    except KeyError:
        pass
    assert eng._phantom_rows == 0

    # loss_and_grads refuses -- before its first launch -- rows that carry phantoms on a launch that could not take them out
    # behind the likelihood: a count the dimension-major backward does not run, or no extended copy of the responses
    for layout, gd, ext in ((0, 0, True), (1, -1, True), (1, 0, False)):
        eng = mk()
        if ext:
            eng._pad_batch(torch.arange(10), None, None)
        eng.be.layout, eng.be.gd_offset, eng._phantom_rows = layout, gd, 2
        try:
            eng.loss_and_grads(torch.cat([torch.arange(10), torch.full((2,), n)]), 10)
        except RuntimeError as e:
            assert "2 phantom rows" in str(e) and "12 rows" in str(e) and "D = 4" in str(e)
        else:
            raise AssertionError("phantom rows were launched on layout %d, gd offset %d" % (layout, gd))


def test_graph_replay_forms_per_engine():
    """Which steps of each engine replay from a captured HIP graph (_graph_mode), and which IrtEngine steps fuse the optimiser
    into the step kernel (_fused_tail_args).  A stub HipBackend: building an engine and asking for its form call no library."""
    from vipsy_amd.engine import (HipBackend, LrSpec, HoDinaEngine, CcdmEngine, VaeCcdmEngine, CdmSfEngine)

    class _Stub(HipBackend):
        def __init__(self):
            pass

    n, J, K, b = 64, 8, 3, 100
    rng = np.random.RandomState(4)
    y = torch.from_numpy(rng.randint(0, 2, size=(n, J)).astype(np.uint8))
    q = np.zeros((K, J), dtype=np.float32)
    q[np.arange(J) % K, np.arange(J)] = 1
    rows = torch.arange(10, dtype=torch.int64)
    nb = int(rows.numel())

    def irt(**kw):
        return IrtEngine(y, model="irt_2pl", backend=_Stub(), **kw)

    replays_all = {
        "irt_d1": irt(D=1),
        "irt_d1_amortized": irt(D=1, amortized=True, H=64),
        "irt_d4_amortized": irt(D=4, amortized=True, H=64),
        "irt_d3_bbvi": irt(D=3),
        "hodina_amortized": HoDinaEngine(y, q, amortized=True, H=64, backend=_Stub()),
        "ccdm": CcdmEngine(y, q, backend=_Stub()),
        "vaeccdm": VaeCcdmEngine(y, q, backend=_Stub()),
        "cdm_sf": CdmSfEngine(y, q, backend=_Stub()),
    }
    for tag, eng in replays_all.items():
        assert eng._graph_mode(None, None, None, 1) == ("full", n, n), tag
        assert eng._graph_mode(rows, b, None, 1) == ("rows", nb, b), tag
        assert eng._graph_mode([rows, rows], b, None, 2) == ("rows", nb, b, 2), tag
        assert eng._graph_mode(None, b, None, 1) is None, tag
        assert eng._graphable(), tag
        # a one-element list with S = 1, the caller's draws, phase events or graphs switched off: an eager step
        assert eng._graph_mode([rows], b, None, 1) is None, tag
        assert eng._graph_mode(None, None, torch.zeros(n), 1) is None, tag
        eng.events = []
        assert eng._graph_mode(None, None, None, 1) is None, tag
        eng.events, eng.use_graph = None, False
        assert eng._graph_mode(None, None, None, 1) is None, tag
        assert eng._graph_mode(rows, b, None, 1) is None, tag

    never = {
        "irt_score": irt(D=1, estimator="score"),
        "cdm_sf_loo": CdmSfEngine(y, q, baseline="loo", backend=_Stub()),
        "vaeccdm_group": VaeCcdmEngine(y, q, group=object(), backend=_Stub()),
    }
    for tag, eng in never.items():
        assert eng._graph_mode(None, None, None, 1) is None, tag
        assert eng._graph_mode(rows, b, None, 1) is None, tag
        assert eng._graph_mode([rows, rows], b, None, 2) is None, tag
        assert eng._graph_mode(None, b, None, 1) is None, tag

    hd = HoDinaEngine(y, q, backend=_Stub())                   # the per-person guide: full batches only
    assert hd._graph_mode(None, None, None, 1) == ("full", n, n)
    assert hd._graph_mode(rows, b, None, 1) is None
    assert hd._graph_mode([rows, rows], b, None, 2) is None
    assert hd._graph_mode(None, b, None, 1) is None

    big = irt(D=4, amortized=True, H=64)
    big.graph_max_persons = n - 1                              # a shard above the switch: its full batch runs eagerly
    assert big._graph_mode(None, None, None, 1) is None
    assert big._graph_mode(rows, b, None, 1) == ("rows", nb, b)

    assert irt(D=1)._fused_tail_args(LrSpec(1e-2), None, None, 1) is not None
    assert irt(D=1, amortized=True, H=64)._fused_tail_args(LrSpec(1e-2), None, None, 1) is None
    assert irt(D=1, estimator="score")._fused_tail_args(LrSpec(1e-2), None, None, 1) is None

    assert IrtEngine.step.__qualname__ == "IrtEngine.step"     # the step written in the class is the one that runs
