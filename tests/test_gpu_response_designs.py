"""Every engine on STRUCTURED response designs (tests/response_designs.py) instead of coin flips with independent holes:
booklets of very different length in file order and shuffled, persons without a response (one alone, and 64 in a row: a whole
list group of the observed-cell kernel with glen == 0), a complete case among 95 % missing, items nobody answered, constant
items and persons, a missing fraction set by count on either side of the list kernel's switch, the degenerate ends.

Each case builds its engine as the family's existing parity test does (tests/design_cases.py restates the parameter rules),
calls loss_and_grads once and compares with the float64 oracle at the same parameters and the same Philox draws:

* loss and replicated gradients at the figures of the family's own test (imported, not restated);
* the item parameters of an item nobody answered: gradient exactly 0.0;
* per-person rows ROW BY ROW: |got_i - oracle_i|_inf <= 3e-5 max(|oracle_i|_inf, N / B) -- N / B is what the prior and the
  entropy term alone put into every row.  Tighter than the whole-tensor rule for every short row (a 10-item person beside a
  150-item one), equal to it for the longest; the whole-tensor rule is kept beside it;
* a repeated call is bit-identical.

Nothing is left out of any comparison: tests/test_response_designs.py checks on the CPU, and every case here again on the
oracle's logits, that no observed cell sits on the Bernoulli clamp (design_cases.band)."""
import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import design_cases as dc
from tests.test_gpu_parity import GRAD_TOL, GRAD_TOL_LARGE, HODINA_TOL, _dev, _oracle_headline_chunked

pytestmark = pytest.mark.gpu

ROW_TOL = 3e-5


def _ids(cases):
    return [c[0] for c in cases]


def _rows_arg(idx, N):
    return None if (len(idx) == N and np.array_equal(idx, np.arange(N))) else torch.from_numpy(idx).to(_dev())


def _grads(eng, mask_free=False):
    """Every tensor's gradient as the parity tests read it: per-person tensors from GP, the rest from G."""
    out = {}
    for name in eng.all_names():
        pp = eng.per_person and name in eng.pp_off
        g = eng.unconstrained(name, eng.GP if pp else eng.G).cpu().numpy().copy()
        if mask_free and not pp:
            g = g * eng.unconstrained(name, eng.free).cpu().numpy()
        out[name] = g
    return out


def _call_twice(eng, idx, N, b_global=0):
    """loss_and_grads, and once more: the second call leaves the same bits (integer atomics, fixed-order reductions).
    b_global: the plate's batch (default: the rows of the call; None: a shard's full batch of the whole problem)."""
    rows = _rows_arg(idx, N)
    b_global = len(idx) if b_global == 0 else b_global
    eng.loss_and_grads(rows, b_global)
    torch.cuda.synchronize()
    first = _grads(eng)
    loss = eng.G[eng.n_params:eng.n_params + 1].cpu().numpy().copy()
    eng.loss_and_grads(rows, b_global)
    torch.cuda.synchronize()
    again = _grads(eng)
    assert np.array_equal(loss.view(np.uint32), eng.G[eng.n_params:eng.n_params + 1].cpu().numpy().view(np.uint32))
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), again[name].view(np.uint32)), "repeated call differs in " + name


def _device_draws(eng, idx, seed):
    """The step-0 Philox normals of the persons idx as the DEVICE evaluates them (vx_philox_normals: the function the step
    kernels draw with), checked against the oracle's statement of the rule at the figure of test_philox_normals_match_oracle.
    The oracle is then run on these draws, as the multivariate parity tests run it on the forward's own eps: the device's
    Box-Muller is a few float32 roundings off the float64 one (1.2e-6 at eps = 2.1), and a person's row multiplies a
    difference in x by the curvature of its likelihood (15 for a 40-item person) -- more than the row rule allows, and no
    error of the step."""
    out = torch.empty(len(idx), dtype=torch.float32, device=_dev())
    gids = torch.from_numpy(np.ascontiguousarray(eng.gid0 + idx, dtype=np.int64)).to(_dev())
    eng.be.philox_normals(out, gids, eng.gid0, len(idx), 1, seed, 0, 0)
    torch.cuda.synchronize()
    eps = out.cpu().numpy().reshape(-1, 1)
    np.testing.assert_allclose(eps, vo.philox_normals(seed, 0, 0, eng.gid0 + idx, 1), atol=2e-5, rtol=1e-5)
    return eps


def _row_errors(got, want, floor):
    """max_i |got_i - want_i|_inf / max(|want_i|_inf, floor) over the rows of a per-person quantity."""
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    assert got.shape == want.shape
    if got.size == 0:
        return 0.0, -1
    err = np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), floor)
    return float(err.max()), int(err.argmax())


def _compare(tag, eng, loss_o, g_o, facts, scale, loss_rel, tol, mask_free=False, scale_of=None, zero_items=True):
    """Loss, every tensor by the whole-tensor rule, the per-person tensors row by row, unanswered items exactly zero."""
    loss_h = float(eng.G[eng.n_params].item())
    loss_err = abs(loss_h - loss_o) / max(abs(loss_o), 1e-300)
    g_h = _grads(eng, mask_free)
    assert sorted(g_o) == sorted(g_h), (sorted(g_o), sorted(g_h))
    errs = {}
    for name, go in g_o.items():
        assert np.isfinite(go).all() and np.isfinite(g_h[name]).all(), name
        sc = max(1e-6, float(np.abs(go).max())) if scale_of is None else scale_of(name, g_o)
        errs[name] = float(np.abs(g_h[name].reshape(go.shape) - go).max() / sc)
    row_err = 0.0
    pp = [n for n in g_o if eng.per_person and n in eng.pp_off]
    if pp:
        n_loc = g_o[pp[0]].shape[0]
        got = np.concatenate([g_h[n].reshape(n_loc, -1) for n in pp], axis=1)
        want = np.concatenate([g_o[n].reshape(n_loc, -1) for n in pp], axis=1)
        row_err, worst = _row_errors(got, want, scale)
    print("DESIGNS %s: loss error %.2e (bound %.0e), largest whole-tensor gradient error %.2e in %s (bound %.0e), largest "
          "per-row error %.2e (bound %.0e)" % (tag, loss_err, loss_rel, max(errs.values()), max(errs, key=errs.get), tol,
                                               row_err, ROW_TOL))
    assert np.isfinite(loss_o) and loss_h == pytest.approx(loss_o, rel=loss_rel), (tag, loss_h, loss_o)
    assert max(errs.values()) < tol, (tag, errs)
    if pp:
        assert row_err <= ROW_TOL, (tag, "person", worst, row_err, got[worst], want[worst])
    for j in np.asarray(facts["unanswered_items"] if zero_items else [], dtype=np.int64):
        for name in ("a", "b", "c", "d", "g", "s"):
            if name in g_o:
                assert (g_o[name][..., j] == 0.0).all(), (tag, name, j)
                assert (g_h[name].reshape(g_o[name].shape)[..., j] == 0.0).all(), (tag, "unanswered item", j, name)
    return g_h


# ---- D = 1, per-person guide: the list kernel and the dense kernel ----------------------------------------------------------
def _irt1d_elbo_rows(spec, params, y, idx, eps):
    """The per-person ELBO terms the step kernels leave in `elbo`: ll_i - x_i^2 / 2 + eps_i^2 / 2 + raw_i."""
    x = dc.irt_latents(spec, params, y, idx, eps)
    if spec["amortized"]:
        W = {k: params["encoder$$$" + k] for k in vo.ENC_KEYS}
        raw = vo.enc_forward(W, vo.enc_input(y[idx], np.float64))[1]
    else:
        raw = params["x_scale"][idx]
    c = vo.sigmoid(params["c"]) if "c" in params else None
    d = vo.sigmoid(params["d"]) if "d" in params else None
    ll = vo.irt_loglik(spec["model"], x, params.get("a"), params["b"], c, d, spec["Dc"], y[idx])[0]
    return ll - 0.5 * x[:, 0] ** 2 + 0.5 * np.asarray(eps, np.float64).reshape(-1) ** 2 + raw[:, 0]


def _irt1d_check(tag, eng, y, idx, model, amortized, facts, want_lists):
    N = len(y)
    eps = _device_draws(eng, idx, dc.IRT1D_SEED)
    _call_twice(eng, idx, len(y))
    if want_lists is not None:
        assert isinstance(eng._sp, dict) if want_lists else not eng._sp, (tag, type(eng._sp))
    spec = dc.irt_spec(model, 1, eng.N, y.shape[1], amortized)
    params = dc.params_of(eng)
    on, below, above, n_obs, zmax = dc.band(spec, params, y, idx, eps)
    assert on == 0, (tag, on)                                   # no observed cell on the clamp: nothing is left out below
    loss_o, g_o = vo.loss_and_grads(spec, params, y, [idx], [eps])
    scale = eng.N / float(len(idx))
    g_h = _compare(tag, eng, loss_o, g_o, facts, scale, 3e-5, GRAD_TOL)
    el_err, worst = _row_errors(eng.last["elbo"][:len(idx)].cpu().numpy(), _irt1d_elbo_rows(spec, params, y, idx, eps), scale)
    print("DESIGNS %s: per-person ELBO rows %.2e (bound %.0e); %d observed cells, %d on the clamp, %d + %d beyond it, max |z| %.1f"
          % (tag, el_err, ROW_TOL, n_obs, on, below, above, zmax))
    assert el_err <= ROW_TOL, (tag, "elbo of batch row", worst, el_err)
    return g_h, (on, below, above, n_obs, zmax)


@pytest.mark.parametrize("case", dc.IRT1D_SPARSE, ids=_ids(dc.IRT1D_SPARSE))
def test_irt1d_list_kernel_on_designs(case):
    """>= 50 % missing, full batch: k_irt1d_sp<1..4>."""
    tag, dname, model, B, _, _, _ = case
    y, facts = dc.design(dname)
    assert facts["missing"] >= 0.5 and B is None
    eng, y, idx = dc.irt1d_engine(case, _dev())
    _, (on, below, above, n_obs, zmax) = _irt1d_check(tag, eng, y, idx, model, False, facts, True)
    sp = eng._sp
    cnt = (y != 255).sum(1)
    assert sp["Lq"] == max(1, (int(cnt.max()) + 3) // 4)
    if "empty_block" in facts:
        assert int((sp["glen"] == 0).sum().item()) >= 1         # a whole list group without an observed cell was walked
    if tag in dc.BEYOND_CLAMP:
        assert below + above >= 100 and (model != "irt_3pl" or below == 0), (tag, below, above)
    if tag in dc.NONE_BEYOND:
        assert below + above == 0, (tag, below, above)


@pytest.mark.parametrize("case", dc.IRT1D_DENSE, ids=_ids(dc.IRT1D_DENSE))
def test_irt1d_dense_kernel_on_designs(case):
    """< 50 % missing, or a row subsample of a sparse design (unsorted rows, as fit() draws them): k_irt1d<...>."""
    tag, dname, model, B, _, _, _ = case
    y, facts = dc.design(dname)
    assert facts["missing"] < 0.5 or B is not None
    eng, y, idx = dc.irt1d_engine(case, _dev())
    _, (on, below, above, n_obs, zmax) = _irt1d_check(tag, eng, y, idx, model, False, facts, None)
    assert not isinstance(eng._sp, dict) or B is not None
    if B is None:
        assert eng._sp is False
    if tag in dc.BEYOND_CLAMP:
        assert below + above >= 100 and (model != "irt_3pl" or below == 0), (tag, below, above)
    if tag in dc.NONE_BEYOND:
        assert below + above == 0, (tag, below, above)


@pytest.mark.parametrize("model", ["irt_2pl", "irt_3pl"])
def test_irt1d_either_side_of_the_list_switch(model):
    """The same persons, responses and parameters with the missing fraction one cell below, at, and one cell above 0.5: the
    dense kernel below (the rule is frac < 0.5), the lists from 0.5 on; each against the oracle."""
    from tests import response_designs as rd
    N, J = 200, 64
    half = N * J // 2
    got = {}
    for n_missing, lists in ((half - 1, False), (half, True), (half + 1, True)):
        y, facts = rd.near_switch(N, J, n_missing / float(N * J), seed=31)
        assert int((y == 255).sum()) == n_missing and facts["min_obs"] < 8 and facts["max_obs"] > 56
        case = ("near_switch-%s-%d" % (model[4:], n_missing), None, model, None, 161, 0, 0.0)
        eng, y, idx = dc.irt1d_engine(case, _dev(), y=y)
        _irt1d_check(case[0], eng, y, idx, model, False, facts, lists)
        assert (eng._sp is False) if not lists else isinstance(eng._sp, dict)
        got[n_missing] = _grads(eng)
    # one cell more or less: the two kernels agree on every person the cell does not belong to (each is within the row rule of
    # the oracle, so within twice that of the other)
    for a, b in ((half - 1, half), (half, half + 1)):
        ra = np.concatenate([got[a]["x_local"], got[a]["x_scale"]], axis=1)
        rb = np.concatenate([got[b]["x_local"], got[b]["x_scale"]], axis=1)
        differ = np.abs(ra - rb).max(1) > 2 * ROW_TOL * np.maximum(np.abs(rb).max(1), 1.0)
        assert differ.sum() <= 1, (a, b, np.flatnonzero(differ))


@pytest.mark.parametrize("model", ["irt_2pl", "irt_4pl"])
def test_irt1d_heterogeneous_shards(model):
    """A response file sorted by booklet, cut in two (n_global / gid0 as in test_cfg4_bbvi_missing90_sharding_additivity):
    shard 0 is 25 % missing and takes the dense kernel, shard 1 is 91 % missing and takes the lists, the unsharded engine (58 %)
    the lists.  Per-person rows of shard 1 equal the unsharded engine's bit for bit, those of shard 0 within the row rule; the
    summed replicated gradients and loss meet the unsharded engine at that test's bounds and the oracle at GRAD_TOL."""
    from vipsy_amd.engine import IrtEngine
    y, facts = dc.design("hetero_shards")
    N, J = y.shape
    pseed = 171
    yt = torch.from_numpy(y).to(_dev())
    full = IrtEngine(yt, model=model, D=1, n_global=N, gid0=0, seed=dc.IRT1D_SEED)
    dc.irt1d_params(full, y, model, pseed, 0, 0.0)
    idx = np.arange(N)
    g_full, _ = _irt1d_check("hetero-unsharded-" + model[4:], full, y, idx, model, False, facts, True)
    loss_full = float(full.G[full.n_params].item())
    spec = dc.irt_spec(model, 1, N, J, False)
    params = dc.params_of(full)
    loss_o, g_o = vo.loss_and_grads(spec, params, y, [idx], [_device_draws(full, idx, dc.IRT1D_SEED)])
    acc, loss_acc = {n: 0.0 for n in full.names()}, 0.0
    for s, (lo, hi, lists) in enumerate(((0, N // 2, False), (N // 2, N, True))):
        ys = y[lo:hi]
        frac = float((ys == 255).mean())
        assert (frac < 0.5) == (not lists) and abs(frac - 0.5) > 0.2
        sh = IrtEngine(yt[lo:hi].contiguous(), model=model, D=1, n_global=N, gid0=lo, seed=dc.IRT1D_SEED)
        dc.irt1d_params(sh, y, model, pseed, 0, 0.0, loc_rows=np.arange(lo, hi))
        assert torch.equal(sh.P, full.P)
        _call_twice(sh, np.arange(hi - lo), hi - lo, b_global=None)
        assert isinstance(sh._sp, dict) if lists else sh._sp is False
        g_s = _grads(sh)
        rows_s = np.concatenate([g_s["x_local"], g_s["x_scale"]], axis=1)
        rows_f = np.concatenate([g_full["x_local"][lo:hi], g_full["x_scale"][lo:hi]], axis=1)
        rows_o = np.concatenate([g_o["x_local"][lo:hi], g_o["x_scale"][lo:hi]], axis=1)
        if lists:
            assert np.array_equal(rows_s.view(np.uint32), rows_f.view(np.uint32))          # the same kernel: the same bits
        else:
            err, worst = _row_errors(rows_s, rows_f.astype(np.float64), 1.0)
            assert err <= ROW_TOL, ("shard 0 against the unsharded engine, person", lo + worst, err)
        err, worst = _row_errors(rows_s, rows_o, 1.0)
        assert err <= ROW_TOL, ("shard %d against the oracle, person" % s, lo + worst, err)
        for n in acc:
            acc[n] = acc[n] + g_s[n].astype(np.float64)
        loss_acc += float(sh.G[sh.n_params].item())
    errs_f, errs_o = {}, {}
    for n in acc:
        errs_f[n] = float(np.abs(acc[n] - g_full[n]).max() / np.abs(g_full[n]).max())
        errs_o[n] = float(np.abs(acc[n] - g_o[n]).max() / max(1e-6, np.abs(g_o[n]).max()))
    print("DESIGNS hetero-shards-%s: summed shards against the unsharded engine %s (bound 2e-4), against the oracle %s (bound %.0e), "
          "loss %.2e / %.2e" % (model[4:], errs_f, errs_o, GRAD_TOL, abs(loss_acc - loss_full) / abs(loss_full),
                                abs(loss_acc - loss_o) / abs(loss_o)))
    assert max(errs_f.values()) <= 2e-4 and loss_acc == pytest.approx(loss_full, rel=2e-5)
    assert max(errs_o.values()) < GRAD_TOL and loss_acc == pytest.approx(loss_o, rel=3e-5)
    for j in facts["unanswered_items"]:
        for n in acc:
            assert (acc[n][..., j] == 0.0).all(), (n, j)


# ---- D = 1, amortized guide -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.IRT1D_AMORT, ids=_ids(dc.IRT1D_AMORT))
def test_irt1d_amortized_on_designs(case):
    """k_norm_enc_fwd / bwd, k_fc1_bwd_c under the D = 1 step kernels: the encoder's input is -1 for a missing cell, so an empty
    person and an unanswered item send values through fc1 and its weight gradient that coin flips never did."""
    tag, dname, model, B, _ = case
    y, facts = dc.design(dname)
    eng, y, idx = dc.irt1d_amort_engine(case, _dev())
    _irt1d_check(tag, eng, y, idx, model, True, facts, (facts["missing"] >= 0.5) if B is None else None)


# ---- amortized multivariate guide -------------------------------------------------------------------------------------------
def _mvn_forward_rows(tag, eng, y, idx, D, H, params, eps, scale):
    """x, h and ent of every person of the batch, row by row, where the engine keeps them (ent only without phantom dimensions:
    with them the kernel's ent carries their eps^2 / 2, which its ll takes out again)."""
    nb, nbk = len(idx), eng.last["nb"]
    fw = eng.last["fw"]
    W = {k: params["encoder$$$" + k] for k in vo.ENC_KEYS}
    _, raw, cache = vo.enc_forward(W, vo.enc_input(y[idx], np.float64))
    x_o = dc.irt_latents({"D": D, "amortized": True}, params, y, idx, eps)
    r_, c_ = vo.tril_rows_cols(D)
    ent_o = 0.5 * (eps.astype(np.float64) ** 2).sum(1) + raw[:, np.flatnonzero(r_ == c_)].sum(1)
    x_h = fw["x"][:nbk * eng.D].reshape(nbk, eng.D)[:nb, :D].cpu().numpy()
    h_h = fw["h"][:nbk * eng.H].reshape(nbk, eng.H)[:nb, :H].cpu().numpy()
    out = {"x": _row_errors(x_h, x_o, scale), "h": _row_errors(h_h, cache[2], scale)}
    if eng.D == D:
        out["ent"] = _row_errors(fw["ent"][:nb].cpu().numpy(), ent_o, scale)
    print("DESIGNS %s: forward rows %s (bound %.0e)" % (tag, {k: "%.2e" % v[0] for k, v in out.items()}, ROW_TOL))
    for k, (err, worst) in out.items():
        assert err <= ROW_TOL, (tag, k, "batch row", worst, err)


def _mvn_amort_check(case, tol):
    tag, dname, D, H, model, B, slopes, _ = case
    y, facts = dc.design(dname)
    eng, y, idx = dc.mvn_amort_engine(case, _dev())
    N, J = y.shape
    _call_twice(eng, idx, N)
    nb = len(idx)
    nbk = eng.last["nb"]
    eps = eng.last["fw"]["eps"][:nbk * eng.D].reshape(nbk, eng.D)[:nb, :D].cpu().numpy()
    np.testing.assert_allclose(eps, vo.philox_normals(dc.MVN_SEED, 0, 0, idx, D), atol=2e-5)
    spec = dc.irt_spec(model, D, N, J, True)
    params = dc.params_of(eng)
    on, below, above, n_obs, zmax = dc.band(spec, params, y, idx, eps)
    assert on == 0 and (slopes != "small" or zmax < 15.0), (tag, on, zmax)
    return eng, y, idx, eps, spec, params, facts


@pytest.mark.parametrize("case", dc.MVN_AMORT, ids=_ids(dc.MVN_AMORT))
def test_mvn_amortized_on_designs(case):
    """The generic tier (H = 96), the packed one (H = 64, D % 4 == 0), phantom items and dimensions (J = 499, D = 99), the MFMA
    likelihood (D >= 96): full batches and 100 unsorted rows."""
    tag, dname, D, H, model, B, slopes, _ = case
    eng, y, idx, eps, spec, params, facts = _mvn_amort_check(case, GRAD_TOL)
    loss_o, g_o = vo.loss_and_grads(spec, params, y, [idx], [eps])
    scale = len(y) / float(len(idx))
    _compare(tag, eng, loss_o, g_o, facts, scale, 3e-5, GRAD_TOL, mask_free=True)
    _mvn_forward_rows(tag, eng, y, idx, D, H, params, eps, scale)


def test_mvn_amortized_large_batch_on_a_design():
    """The large-batch forms test_headline_large_batch_kernels_vs_oracle names (N = 33 024: k_mvn_enc_fwd_b2, k_irt_lik_h +
    k_lik_reduce_parts, k_mvn_enc_bwd_h_b2, k_mvn_enc_bwd_w_b, k_fc1_bwd_c) on the sorted booklet design, 'small' slopes."""
    case = dc.MVN_LARGE
    tag, dname, D, H, model, B, slopes, _ = case
    eng, y, idx, eps, spec, params, facts = _mvn_amort_check(case, GRAD_TOL_LARGE)
    loss_o, g_o, x_o, h_o, ent_o = _oracle_headline_chunked(eng, y, eps)
    _compare(tag, eng, loss_o, g_o, facts, 1.0, 3e-5, GRAD_TOL_LARGE, mask_free=True)
    _mvn_forward_rows(tag, eng, y, idx, D, H, params, eps, 1.0)


# ---- multivariate per-person guide ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.MVN_BBVI, ids=_ids(dc.MVN_BBVI))
def test_mvn_bbvi_on_designs(case):
    """VIRT with x_feature > 1 (k_mvn_bbvi), per-person and shared covariance."""
    tag, dname, D, share, B, _ = case
    y, facts = dc.design(dname)
    eng, y, idx = dc.mvn_bbvi_engine(case, _dev())
    N, J = y.shape
    _call_twice(eng, idx, N)
    eps = eng.last["fw"]["eps"][:len(idx) * D].reshape(len(idx), D).cpu().numpy()
    np.testing.assert_allclose(eps, vo.philox_normals(dc.BBVI_SEED, 0, 0, idx, D), atol=2e-5)
    spec = dc.irt_spec("irt_2pl", D, N, J, False, share)
    params = dc.params_of(eng)
    assert dc.band(spec, params, y, idx, eps)[0] == 0
    loss_o, g_o = vo.loss_and_grads(spec, params, y, [idx], [eps])
    _compare(tag, eng, loss_o, g_o, facts, N / float(len(idx)), 3e-5, GRAD_TOL, mask_free=True)


# ---- the CDMs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.HODINA, ids=_ids(dc.HODINA))
def test_hodina_on_designs(case):
    """k_hodina_m (5 <= K <= 8, J <= 32) and k_hodina, per-person and amortized guide."""
    tag, dname = case[0], case[1]
    facts = dc.design(dname)[1]
    eng, y, idx, spec = dc.hodina_engine(case, _dev())
    _call_twice(eng, idx, len(y))
    eps = _device_draws(eng, idx, dc.HODINA_SEED)
    loss_o, g_o = vo.loss_and_grads(spec, dc.params_of(eng), y, [idx], [eps])
    _compare(tag, eng, loss_o, g_o, facts, len(y) / float(len(idx)), 5e-5, HODINA_TOL)


@pytest.mark.parametrize("case", dc.CCDM, ids=_ids(dc.CCDM))
def test_ccdm_on_designs(case):
    """The enumerated DINA / DINO kernels with the empty guide; figures of test_ccdm_step_vs_oracle."""
    tag, dname = case[0], case[1]
    facts = dc.design(dname)[1]
    eng, y, idx, spec = dc.ccdm_engine(case, _dev())
    _call_twice(eng, idx, len(y))
    loss_o, g_o = vo.loss_and_grads(spec, dc.params_of(eng), y, [idx], [None])
    _compare(tag, eng, loss_o, g_o, facts, len(y) / float(len(idx)), 2e-5, GRAD_TOL)


@pytest.mark.parametrize("case", dc.VAECCDM, ids=_ids(dc.VAECCDM))
def test_vaeccdm_on_designs(case):
    """The enumerated kernels behind the SoftmaxEncoder; figures and gradient scales of test_vaeccdm_step_vs_oracle."""
    tag, dname = case[0], case[1]
    facts = dc.design(dname)[1]
    eng, y, idx, spec = dc.vaeccdm_engine(case, _dev())
    _call_twice(eng, idx, len(y))
    loss_o, g_o = vo.loss_and_grads(spec, dc.params_of(eng), y, [idx], [None])

    def scale_of(name, g):          # test_vaeccdm_step_vs_oracle: a floor of 1e-3 of the largest gradient of the step; fc2.bias is
        top = max(float(np.abs(v).max()) for v in g.values())       # exactly zero in exact arithmetic, measured on fc2.weight
        sc = max(1e-6, float(np.abs(g[name]).max()), 1e-3 * top)
        return max(sc, float(np.abs(g["encoder$$$fc2.weight"]).max())) if name == "encoder$$$fc2.bias" else sc
    # (no exact zeros here: VaeCCDM keeps the reference's -1 of a missing cell as an OBSERVATION, vi.py:882-891, so an item
    # nobody answered has a gradient, the oracle's)
    _compare(tag, eng, loss_o, g_o, facts, len(y) / float(len(idx)), 3e-5, 3e-4, scale_of=scale_of, zero_items=False)


@pytest.mark.parametrize("case", dc.CDM_SF, ids=_ids(dc.CDM_SF))
def test_cdm_sf_on_designs(case):
    """k_cdm_sf + k_cdm_sf_items reduce the item gradients to integer counts of the four (eta, y) combinations per item: a constant
    item leaves whole count rows at zero.  Complete responses (the engine refuses a missing cell); figures of
    test_cdm_sf_step_vs_oracle; no draw of these cases sits on its threshold, so nothing is left out."""
    tag, dname, K, cdm, B, amort, H, baseline, _ = case
    facts = dc.design(dname)[1]
    eng, y, idx, spec = dc.cdm_sf_engine(case, _dev())
    N = len(y)
    eng.t = dc.CDM_SF_T
    rows = _rows_arg(idx, N)
    eng.loss_and_grads(rows, len(idx), None, dc.CDM_SF_STREAM)
    torch.cuda.synchronize()
    params, attr, near = dc.cdm_sf_draws(eng, y, idx, K, amort)
    assert not near.any()
    loss_o, g_o, lr_o = vo.cdm_sf_particle(spec, params, y, idx, attr, baseline=np.zeros(len(idx)) if baseline == "avg" else None)
    lr_h = eng.last["log_r"][:len(idx)].cpu().numpy()
    np.testing.assert_allclose(lr_h, lr_o, rtol=3e-5, atol=3e-4)
    _compare(tag, eng, loss_o, g_o, facts, N / float(len(idx)), 3e-5, 2e-4)
    for j in (facts["all_one_item"], facts["all_zero_item"]):
        assert len(set(y[:, j].tolist())) == 1
    if baseline == "none":                                   # (the decaying average moves with every call)
        first = _grads(eng)
        eng.loss_and_grads(rows, len(idx), None, dc.CDM_SF_STREAM)
        torch.cuda.synchronize()
        again = _grads(eng)
        for name in first:
            assert np.array_equal(first[name].view(np.uint32), again[name].view(np.uint32)), name
    else:                                                    # test_baselines_on_hip_match_oracle: used before it is updated
        base = eng.base.cpu().numpy()
        want = np.zeros(N)
        want[idx] = (1.0 - eng.baseline_beta) * lr_o
        np.testing.assert_allclose(base[:N], want, rtol=1e-4, atol=1e-3)


# ---- replay and the class surface -------------------------------------------------------------------------------------------
def test_replayed_list_kernel_steps_equal_eager_steps_on_the_sorted_design():
    """eng.step replayed from its graph for five steps on the sorted booklet design (the lists and the item-major copies are
    built once and reused) equals five eager steps bit for bit: the pattern of test_captured_step_equals_eager_step."""
    from vipsy_amd.engine import LrSpec
    case = dc.IRT1D_SPARSE[1]
    out = []
    for graph in (True, False):
        eng, y, idx = dc.irt1d_engine(case, _dev())
        eng.use_graph = graph
        lrs = LrSpec(lambda m, p: {"lr": 1e-2 if p in ("a", "b") else 1e-3})
        losses = [eng.step(lrs) for _ in range(5)]
        torch.cuda.synchronize()
        assert eng.t == 5 and isinstance(eng._sp, dict)
        assert (getattr(eng, "_graph", None) or {}).get("graph") is not None if graph else getattr(eng, "_graph", None) is None
        out.append((torch.stack(losses).cpu().numpy(), eng.P.cpu().numpy().copy(), eng.PP.cpu().numpy().copy()))
    assert np.isfinite(out[0][0]).all() and len(set(out[0][0].tolist())) == 5
    for u, v in zip(out[0], out[1]):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_virt_fit_on_the_sorted_design_equals_the_engine_stepped_by_hand():
    """vi.VIRT(...).fit on the sorted booklet design, handed over as the reference's float tensor with NaN for missing, full
    batch (fit() draws no rows), six iterations: the parameters equal, bit for bit, those of an IrtEngine built with the same
    seed and stepped by hand as often."""
    from vipsy_amd import vi
    from vipsy_amd.engine import IrtEngine, LrSpec
    y, facts = dc.design("sorted9000")
    data = torch.from_numpy(y.astype(np.float32))
    data[torch.from_numpy(y == 255)] = float("nan")
    n_iter = 6
    vi.clear_param_store()
    m = vi.VIRT(data=data.to(_dev()), model="irt_2pl", seed=77)
    last = m.fit(optim=vi.Adam({"lr": 1e-2}), max_iter=n_iter, progress=False)
    torch.cuda.synchronize()
    assert np.isfinite(last) and m.engine.t == n_iter and isinstance(m.engine._sp, dict)
    assert torch.equal(m.engine.y.cpu(), torch.from_numpy(y))
    eng = IrtEngine(torch.from_numpy(y).to(_dev()), model="irt_2pl", D=1, seed=77)
    lrs = LrSpec({"lr": 1e-2})
    losses = [eng.step(lrs) for _ in range(n_iter)]
    torch.cuda.synchronize()
    assert float(losses[-1]) == last
    assert torch.equal(m.engine.P, eng.P) and torch.equal(m.engine.PP, eng.PP)
    vi.clear_param_store()
