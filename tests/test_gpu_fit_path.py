"""The path fit() takes: IrtEngine.steps() -- K-step replay, the pinned row ring, Philox step and Adam's t from the device
counter, the plate scale N / B from an explicit b_global, and a subsample that is no multiple of 4 drawn 1-3 phantom rows longer
(IrtEngine._pad_batch: the dimension-major backward kernels over an extended copy of the responses, the phantoms taken out
behind the likelihood) -- against the float64 oracle, step by step at frozen parameters and over a short trained trajectory."""
import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests.test_gpu_parity import GRAD_TOL, HODINA_TOL, _dev, _oracle_latents_chunked, _random_problem

pytestmark = pytest.mark.gpu

T_FIRST, T_SECOND = 19, 8      # 19: more than the ring's 16 slots, and 1 eager + 1 captured + 4 x 4 replayed + 1 single step;
#                                8 more: two whole replays, so the gradients left behind are those of a replay's fourth step
SEED = 11


def _draws(rng, N, B, T, always=None):
    """T unsorted draws of B distinct rows, as the fit loop makes them; `always`: a person every draw contains (at a position
    that moves with the step)."""
    out = []
    for t in range(T):
        if always is None:
            r = rng.choice(N, size=B, replace=False)
        else:
            others = np.delete(np.arange(N), always)
            r = np.insert(rng.choice(others, size=B - 1, replace=False), t % B, always)
        out.append(r.astype(np.int64))
    return out


def _grad_errors(eng, g_o):
    errs = {}
    for name, go in g_o.items():
        per_person = eng.per_person and name in eng.pp_off
        gh = eng.unconstrained(name, eng.GP if per_person else eng.G).cpu().numpy()
        if not per_person:
            gh = gh * eng.unconstrained(name, eng.free).cpu().numpy()
        errs[name] = float(np.abs(gh - go).max() / max(1e-6, float(np.abs(go).max())))
    return errs


def _frozen_steps_vs_oracle(eng, y, spec, rows_of, B, replay, tag, nb_want=None, loss_rel=3e-5, grad_tol=GRAD_TOL, z_of=None):
    """steps() at a learning rate of 0 for every tensor: the parameters stay at their initial bits, so step t of the call is
    the oracle's loss_and_grads at those parameters with that step's rows and philox_normals(seed, t, 0, gid0 + rows_t, D).
    Every loss of every step, and every gradient the last step of each of two calls leaves in G, against the oracle; returns
    the losses."""
    from vipsy_amd.engine import LrSpec
    eng.use_graph = replay
    lrs = LrSpec(0.0)
    P0 = eng.P.clone()
    PP0 = eng.PP.clone() if eng.per_person else None
    params = {n: eng.unconstrained(n).cpu().numpy().astype(np.float64) for n in eng.all_names()}
    D = spec.get("D", 1)
    all_losses, worst_loss, worst_grad, t0 = [], 0.0, {}, 0
    for T in (T_FIRST, T_SECOND):
        rows_all = [rows_of(t0 + j) for j in range(T)]
        losses = eng.steps(lrs, [torch.from_numpy(r) for r in rows_all], b_global=B)     # host indices, as the fit loop's
        torch.cuda.synchronize()
        losses = torch.stack(losses).cpu().numpy().astype(np.float64)
        assert eng.t == t0 + T and len(losses) == T
        assert torch.equal(eng.P, P0) and (PP0 is None or torch.equal(eng.PP, PP0))      # lr 0: Adam moved nothing, bit for bit
        if nb_want is not None:
            assert eng.last["nb"] == nb_want and eng.last["n_valid"] == B, (tag, eng.last["nb"], eng.last["n_valid"])
        st = getattr(eng, "_graph", None) or {}
        assert (st.get("graph") is not None) == replay
        if replay and nb_want is not None:
            # the form (rows launched, plate's batch), its single-step graph, the K-step graph and the pinned ring were all used
            assert eng._graphs.get(("rows", nb_want, B)) is st
            assert st.get("multi") is not None and eng.graph_steps == 4
            assert st.get("ring") is not None and st["ring"].is_pinned() and eng.rows_ring_slots < T_FIRST
        g_o = None
        for j, r in enumerate(rows_all):
            eps = vo.philox_normals(eng.seed, t0 + j, 0, eng.gid0 + r, D)
            if z_of is not None:
                assert z_of(params, r, eps) < 15.0                                   # no cell near the Bernoulli clamp
            loss_o, g_o = vo.loss_and_grads(spec, params, y, [r], [eps])
            worst_loss = max(worst_loss, abs(losses[j] - loss_o) / abs(loss_o))
            assert losses[j] == pytest.approx(loss_o, rel=loss_rel), (tag, t0 + j)
        assert sorted(g_o) == sorted(eng.all_names())                                # every tensor of the engine is compared
        errs = _grad_errors(eng, g_o)                                                # (g_o: the call's last step)
        worst_grad = {k: max(v, worst_grad.get(k, 0.0)) for k, v in errs.items()}
        assert max(errs.values()) < grad_tol, (tag, t0 + T - 1, errs)
        all_losses.append(losses)
        t0 += T
    print("steps() vs oracle, %s: nb %s, largest loss error %.2e, largest gradient error %.2e (%s)"
          % (tag, eng.last.get("nb"), worst_loss, max(worst_grad.values()), max(worst_grad, key=worst_grad.get)))
    return np.concatenate(all_losses)


def _step_bits(eng):
    """What a step leaves behind, for bit comparisons: every tensor's gradient, the loss slot, Adam's moments.  (Not G as a
    whole: its c / d segments exist for every link, and for a 1PL / 2PL model -- no such tensor, no optimiser segment, nothing
    reads them -- they hold minus the sum of the item slabs' c / d columns, which no kernel writes and the likelihood call's
    hipMemsetAsync clears.  Replayed from a captured graph that memset has been seen to leave a repeated 16-byte pattern of
    stale words there instead of zeros, once the host had copied something off the device between capture and replay.)"""
    out = {"g:" + n: eng.unconstrained(n, eng.G).cpu().numpy().copy() for n in eng.names()}
    out.update(loss=eng.G[eng.n_params:].cpu().numpy().copy(), M=eng.M.cpu().numpy().copy(), V=eng.V.cpu().numpy().copy())
    return out


def _mvn_engine(N, J, D, H, model, miss, seed, **kw):
    """The amortized multivariate engine with the 'small' inputs of test_headline_large_batch_kernels_vs_oracle: the default
    encoder, slopes of 0.05 (1 +- 0.3), b = 0.5 randn."""
    from vipsy_amd.engine import IrtEngine
    y, _, rng = _random_problem(N, J, D, H, model, miss, seed)
    eng = IrtEngine(torch.from_numpy(y).to(_dev()), model=model, D=D, amortized=True, H=H, seed=SEED, **kw)
    a0 = eng.unconstrained("a") * torch.from_numpy(0.05 * (1 + 0.3 * rng.randn(D, J))).float().to(_dev())
    eng.unconstrained("a").copy_(a0 * eng.unconstrained("a", eng.free))
    eng.unconstrained("b").copy_(torch.from_numpy(0.5 * rng.randn(1, J)).float())
    if model in ("irt_3pl", "irt_4pl"):
        eng.unconstrained("c").add_(torch.from_numpy(0.3 * rng.randn(1, J)).float().to(_dev()))
    if model == "irt_4pl":
        eng.unconstrained("d").add_(torch.from_numpy(0.3 * rng.randn(1, J)).float().to(_dev()))
    return eng, y


def _mvn_case(N, J, D, H, model, miss, B, replay, tag, padded, always=None, shard=False, pad_batch=True):
    kw = {"n_global": N + 8192, "gid0": 4096} if shard else {}
    eng, y = _mvn_engine(N, J, D, H, model, miss, seed=N + J + D + B, **kw)
    if not pad_batch:
        eng.pad_batch = False                # (the class attribute is read from VX_PAD_BATCH at import: the instance is the seam)
    nb_want = B + (-B) % 4 if padded else B
    if padded:
        # the shape pads only where the dimension-major backward takes the padded count (a host query): a vacuous case fails here
        cfg = eng.be.cfg(eng.model, eng.D, eng.J, eng.H, eng.Dc, 1.0, eng.seed, 0, 0)
        assert B % 4 != 0 and eng.be.mvn_enc_bwd_layout(cfg, nb_want) == 1 and eng.be.mvn_enc_bwd_gd_offset(cfg, nb_want) >= 0
    spec = {"family": "irt", "model": model, "D": D, "Dc": 1.0, "N": eng.N, "amortized": True, "share_cov": False,
            "a_free": vo.default_a_free(D, J)}
    draws = _draws(np.random.RandomState(5 + B), N, B, T_FIRST + T_SECOND, always=always)
    if always is not None:
        assert all(always in r for r in draws)

    def z_of(params, r, eps):
        x = _oracle_latents_chunked(params, y[r], eps, D)
        return float(np.abs(x @ params["a"] + params["b"]).max())
    return eng, y, draws, _frozen_steps_vs_oracle(eng, y, spec, lambda t: draws[t], B, replay, tag, nb_want=nb_want, z_of=z_of)


PADDED = [
    # model, N, J, D, H, miss, B, replay, extra
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, False, {}),     # _pad_batch's own example, launched kernel by kernel
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, True, {}),      # ... and replayed
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 101, True, {}),     # three phantom rows
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 1, False, {}),      # nb = 4, the smallest batch those kernels accept: one real person
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 2, False, {}),
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 3, False, {}),
    ("irt_4pl", 5000, 500, 100, 64, 0.1, 50, True, {}),      # the bf16x3 likelihood behind the same mask
    ("irt_3pl", 5000, 500, 64, 64, 0.3, 30, True, {}),       # 30 % missing
    ("irt_2pl", 5000, 500, 8, 64, 0.1, 50, True, {}),        # small D on the same layout
    ("irt_2pl", 3001, 37, 3, 32, 0.1, 50, True, {}),         # phantom items + a phantom dimension + phantom hidden units + rows
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, True, {"always": 4999}),    # the shard's last person, next to the phantom, in every draw
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, True, {"always": 0}),       # ... and its first
    # a shard: the phantom's index n_local is then a real global id of the next shard; plate scale from n_global
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, False, {"shard": True}),
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, True, {"shard": True}),
]


def _case_id(c):
    return "%s-J%d-D%d-B%d-%s%s" % (c[0][4:], c[2], c[3], c[6], "replay" if c[7] else "eager",
                                    "".join("-%s%s" % (k, "" if v is True else v) for k, v in sorted(c[8].items())))


@pytest.mark.parametrize("model,N,J,D,H,miss,B,replay,extra", PADDED, ids=[_case_id(c) for c in PADDED])
def test_padded_steps_vs_oracle_at_frozen_parameters(model, N, J, D, H, miss, B, replay, extra):
    """Subsamples that are no multiple of 4 through steps(), the way fit() hands them over: launched over B + 1..3 rows
    (eng.last: nb, n_valid), every step's loss and the last step's gradients as if the phantom person were not there.  With the
    mask behind the likelihood switched off every case here misses its first loss (the phantom's entropy and prior): by 2.4e-4
    of it at D = 8 and D = 3, 1.4e-2 to 2.6e-2 at D = 64 and 100 with B >= 30, 0.19 to 1.2 with B <= 3."""
    _mvn_case(N, J, D, H, model, miss, B, replay, _case_id((model, N, J, D, H, miss, B, replay, extra)), padded=True, **extra)


CONTROLS = [
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 100, True, {}),                      # a multiple of 4: nothing to pad
    ("irt_2pl", 5000, 500, 112, 64, 0.1, 50, True, {}),                       # person-major backward at 52 rows too: _pad_batch stands down
    ("irt_2pl", 5000, 500, 100, 64, 0.1, 50, True, {"pad_batch": False}),     # the seam (VX_PAD_BATCH=0)
]


@pytest.mark.parametrize("model,N,J,D,H,miss,B,replay,extra", CONTROLS, ids=[_case_id(c) for c in CONTROLS])
def test_unpadded_steps_vs_oracle_and_bit_equal_to_step_in_a_loop(model, N, J, D, H, miss, B, replay, extra):
    """Where steps() does not pad, the same oracle comparison -- and the promise of _EngineBase.steps: the same bits as step()
    called in a loop, in every loss, in the last gradients and in Adam's moments (which every step's gradients went into)."""
    from vipsy_amd.engine import LrSpec
    tag = _case_id((model, N, J, D, H, miss, B, replay, extra))
    eng, y, draws, losses = _mvn_case(N, J, D, H, model, miss, B, replay, tag, padded=False, **extra)
    ref, _ = _mvn_engine(N, J, D, H, model, miss, seed=N + J + D + B)
    ref.pad_batch = eng.pad_batch
    lrs = LrSpec(0.0)
    want = torch.stack([ref.step(lrs, rows=torch.from_numpy(r), b_global=B).clone() for r in draws])
    torch.cuda.synchronize()
    assert ref.t == eng.t == len(draws) and ref.last["nb"] == B
    assert np.array_equal(want.cpu().numpy().astype(np.float64), losses)
    got, ref_bits = _step_bits(eng), _step_bits(ref)
    assert sorted(got) == sorted(ref_bits) and len(got) == len(eng.names()) + 3
    for k in got:
        assert np.array_equal(got[k], ref_bits[k]), k


@pytest.mark.parametrize("kind", ["irt1d_per_person", "irt1d_amortized", "hodina_amortized", "hodina_per_person"])
def test_other_engines_steps_vs_oracle_at_frozen_parameters(kind):
    """steps() of the engines that do not pad, with the specs of their *_step_vs_oracle tests and 50 host-drawn rows a step:
    every step's loss (Philox steps 0 .. 26) and the last gradients against the oracle."""
    from vipsy_amd.engine import IrtEngine, HoDinaEngine
    B, loss_rel, grad_tol = 50, 3e-5, GRAD_TOL
    if kind.startswith("irt1d"):
        amort = kind == "irt1d_amortized"
        N, J, model, miss = (700, 500, "irt_2pl", 0.59) if amort else (5000, 100, "irt_4pl", 0.0)
        rng = np.random.RandomState(N + J)
        y = rng.randint(0, 2, size=(N, J)).astype(np.uint8)
        y[rng.rand(N, J) < miss] = 255
        eng = IrtEngine(torch.from_numpy(y).to(_dev()), model=model, D=1, amortized=amort, H=64, seed=5)
        eng.unconstrained("b").copy_(torch.from_numpy(0.7 * rng.randn(1, J)).float())
        eng.unconstrained("a").copy_(torch.from_numpy(0.5 + 2 * rng.rand(1, J)).float())
        if model == "irt_4pl":
            eng.unconstrained("c").add_(torch.from_numpy(0.3 * rng.randn(1, J)).float().to(_dev()))
        if not amort:
            eng.PP.copy_(torch.from_numpy(np.concatenate([rng.randn(N), 0.3 * rng.randn(N)])).float())
        spec = {"family": "irt", "model": model, "D": 1, "Dc": 1.0, "N": N, "amortized": amort, "share_cov": False, "a_free": None}
    else:
        amort = kind == "hodina_amortized"
        N, J, K, miss = (150, 40, 10, 0.0) if amort else (333, 100, 5, 0.2)
        rng = np.random.RandomState(N + J + K)
        q = (rng.rand(K, J) < 0.4).astype(np.float32)
        q[rng.randint(0, K, size=J), np.arange(J)] = 1.0
        y = rng.randint(0, 2, size=(N, J)).astype(np.uint8)
        y[rng.rand(N, J) < miss] = 255
        eng = HoDinaEngine(torch.from_numpy(y).to(_dev()), q, amortized=amort, H=64, seed=9)
        eng.unconstrained("lam0").copy_(torch.from_numpy(0.5 * rng.randn(1, K)).float())
        eng.unconstrained("lam1").copy_(torch.from_numpy(0.4 * rng.randn(1, K)).float())
        eng.unconstrained("g").add_(torch.from_numpy(0.5 * rng.randn(1, J)).float().to(_dev()))
        eng.unconstrained("s").add_(torch.from_numpy(0.5 * rng.randn(1, J)).float().to(_dev()))
        if not amort:
            eng.PP.copy_(torch.from_numpy(np.concatenate([rng.randn(N), 0.3 * rng.randn(N)])).float())
        spec = {"family": "hodina", "K": K, "N": N, "amortized": amort, "q": q}
        loss_rel, grad_tol = 5e-5, HODINA_TOL                  # (the figures of test_hodina_step_vs_oracle)
    draws = _draws(np.random.RandomState(7), N, B, T_FIRST + T_SECOND)
    replay = eng._graph_mode(torch.from_numpy(draws[0]), B, None, 1) is not None     # (HO-DINA's per-person guide: eager)
    assert replay == (kind != "hodina_per_person")
    _frozen_steps_vs_oracle(eng, y, spec, lambda t: draws[t], B, replay, kind, loss_rel=loss_rel, grad_tol=grad_tol)
    assert eng.last.get("nb", B) == B


def test_trained_trajectory_through_padded_steps_within_1e3_of_cpu_reference():
    """Learning rates on: 24 Adam steps over subsamples of 50 through steps() (52 rows a launch, four steps a replay, a
    scheduler milestone at step 13) and through step() in a loop (50 rows), each against vo.Adam + vo.loss_and_grads (float64)
    fed the same rows and philox_normals(seed, t, 0, rows_t, D): RMSE of a and of b below 1e-3 of the slopes' level, the figure
    and form of test_trained_item_parameters_within_1e3_of_cpu_reference.  Adam's t, its moments and the scheduler stay
    aligned across replays -- the two GPU paths are each held to the oracle, not to one another."""
    from vipsy_amd.engine import IrtEngine, LrSpec, ENC_KEYS
    N, J, D, H, B, n_steps, a_level, seed = 5000, 500, 100, 64, 50, 24, 0.05, 17
    rng = np.random.RandomState(99 + D)
    x = rng.randn(N, D)
    af = vo.default_a_free(D, J)
    a_true = a_level * rng.uniform(0.5, 2.0, size=(D, J)) * (1.0 if af is None else af)
    b_true = rng.randn(1, J)
    y = (rng.rand(N, J) < 1 / (1 + np.exp(-(x @ a_true + b_true)))).astype(np.uint8)
    y[rng.rand(N, J) < 0.1] = 255
    draws = _draws(np.random.RandomState(3), N, B, n_steps)

    def lr_fn(module, name):
        return {"lr": 2e-3 if name in ("a", "b", "c", "d") else 1e-3}

    def make():
        e = IrtEngine(torch.from_numpy(y).to(_dev()), model="irt_2pl", D=D, amortized=True, H=H, seed=seed)
        e.unconstrained("a").mul_(a_level)
        return e, LrSpec(lr_fn, milestones=(13,), gamma=0.5)

    spec = {"family": "irt", "model": "irt_2pl", "D": D, "Dc": 1.0, "N": N, "amortized": True, "share_cov": False, "a_free": af}
    eng, lrs = make()
    enc0 = {k: eng.unconstrained("encoder$$$" + k).cpu().numpy().astype(np.float64) for k in ENC_KEYS}
    params = vo.init_irt_params(spec, J, np.float64, encoder=enc0)
    params["a"] = params["a"] * a_level
    adam = vo.Adam(lr_fn, milestones=(13,), gamma=0.5)
    for t in range(n_steps):
        _, g = vo.loss_and_grads(spec, params, y, [draws[t]], [vo.philox_normals(seed, t, 0, draws[t], D)])
        adam.step(params, g)
        adam.scheduler_step()

    eng.steps(lrs, [torch.from_numpy(r) for r in draws], b_global=B, scheduler=True)
    torch.cuda.synchronize()
    assert eng.t == n_steps and lrs.epoch == n_steps and eng.last["nb"] == 52 and eng.last["n_valid"] == B
    assert (eng._graph or {}).get("multi") is not None
    loop, lrs2 = make()
    for r in draws:
        loop.step(lrs2, rows=torch.from_numpy(r), b_global=B)
        lrs2.scheduler_step()
    torch.cuda.synchronize()
    assert loop.t == n_steps and loop.last["nb"] == B
    rmse = {}
    for path, e in (("steps", eng), ("step", loop)):
        for name in ("a", "b"):
            po = vo.constrained(name, params[name])
            rmse[path, name] = float(np.sqrt(np.mean((e.param(name).double().cpu().numpy() - po) ** 2)))
            assert float(np.abs(po - (a_level if name == "a" else 0.0)).max()) > 0.05 * a_level     # the parameters did move
    print("trained trajectory, RMSE against the oracle: %s (bound %.1e)" % (rmse, 1e-3 * a_level))
    assert max(rmse.values()) < 1e-3 * a_level, rmse
