"""item_se(): time, memory and accuracy at three shapes, beside what a user would write today from torch operations.

Shapes: 1M persons x 500 items x 61 nodes (2PL, P = 1 000 parameters), 1M x 40 items x 9^3 = 729 nodes (3-D 2PL, P = 160),
1M x 30 items x K = 8 (DINA through CcdmEngine, 256 patterns, P = 60).  For each:
  * engine.item_se() end to end (tables, posterior kernel, derivative tables, vx_grid_info, the copy to the host and the float64
    inverse there) and vx_grid_info alone (on tables and loglik made once): device events around 10 back-to-back calls behind 2
    warm-up calls; k_grid_pscores and k_grid_xprod alone: their device times inside one vx_grid_info call, by torch.profiler;
  * the torch composition on the same GPU, in person slabs of 65 536: fp32 indicator matmuls for ll, softmax over the nodes (p
    [slab][G] in memory), p @ W1 and p @ W0, S [slab][P] in memory, S.T @ S in fp32 added over the slabs;
  * the peak device memory of both above what the responses and the engine hold;
  * 4 096 sampled persons (through `rows`) against the float64 oracle of tests/se_cases.py by the rule of tests/test_gpu_se.py;
  * the useful rate of the two kernels against the fp16-pair roofline (three MFMA products a useful one: a third of the dense
    fp16 peak): useful FLOP = 2 n (2 J G + 2 P G) for k_grid_pscores, 2 n P (P + 1) / 2 for k_grid_xprod.
The times are reported, not asserted.

--model irt_3pl | irt_4pl: item_se(prior=) instead, at 1M persons x 500 items x 61 nodes (P = 1 500 / 2 000) under the priors
c_un ~ N(-1.4, 1), d_un ~ N(2.2, 1), behind the 2PL shape of the same size for comparison: the table entry
(vx_grid_wtable_irt_map: the maximum pass, the trailer, the fill pass; device events around 200 back-to-back calls, and each
kernel's device time by torch.profiler), vx_grid_info at K = 3 / 4, item_se(prior=) end to end, and 4 096 sampled persons
against the float64 oracle of tests/se_map_cases.py.

usage (GPU box):  python tools/se_probe.py [out.txt] [--model irt_3pl]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import score_cases as sc                                              # noqa: E402
from tests import se_cases as se                                                 # noqa: E402  (the float64 oracle)
from vipsy_amd.engine import CcdmEngine, IrtEngine                               # noqa: E402

PEAK_F16_MFMA = 2.5e15       # FLOP/s, dense fp16 MFMA (spec)
ROW_TOL = 3e-5               # the row rule of tests/test_gpu_se.py
SLAB = 65536                 # persons a slab of the torch composition
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_of(fn):
    """(peak device memory of one call above what was allocated before it, in MB)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def torch_info(y, T1, T0, logw, W1, W0, K):
    """What a user would write today: p and S of a slab of persons in memory, S.T @ S in fp32."""
    P = W1.shape[1]
    info = torch.zeros(P, P, dtype=torch.float32, device=dev)
    grad = torch.zeros(P, dtype=torch.float32, device=dev)
    for i0 in range(0, y.shape[0], SLAB):
        ys = y[i0:i0 + SLAB]
        i1, i0_ = (ys == 1).to(torch.float32), (ys == 0).to(torch.float32)
        f = i1 @ T1 + i0_ @ T0 + ((ys == 255).sum(1).to(torch.float32) * -1.1920928244535389e-07)[:, None] + logw[None, :]
        p = torch.softmax(f, 1)
        S = i1.repeat_interleave(K, dim=1) * (p @ W1) - i0_.repeat_interleave(K, dim=1) * (p @ W0)
        info += S.t() @ S
        grad += S.sum(0)
    return info, grad


def kernel_times(fn, names=("k_grid_pscores", "k_grid_xprod")):
    """Device microseconds of the kernels whose names contain one of `names` inside one call of fn, or None where the profiler
    has no device activity to offer."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            for k in names:
                if k in ev.key:
                    out[k] = out.get(k, 0.0) + float(t)
        return out if len(out) == len(names) else None
    except Exception as e:  # noqa: BLE001
        say("    (no kernel times: %s)" % e)
        return None


def probe(tag, eng, kw, cs, kind, T1, T0):
    y, be = eng.y, eng.be
    N, J = int(y.shape[0]), cs["J"]
    t_e2e = timed(lambda: eng.item_se(**kw))
    call, K, fill_wtable, _ = eng._info_call(None, None, **kw)
    post = eng._grid_posterior(call)
    P, G = J * K, call.G
    f32 = dict(dtype=torch.float32, device=dev)
    wimg = torch.empty(be.grid_wimage_bytes(P, G), dtype=torch.uint8, device=dev)
    fill_wtable(wimg)
    ws_floats = be.grid_info_workspace(N, P, G)
    info, grad, ws = torch.empty(P, P, **f32), torch.empty(P, **f32), torch.empty(ws_floats, **f32)

    def run():
        be.grid_info(call.y, None, N, J, G, K, post["img"], wimg, call.logw, post["loglik"], info, grad, ws, ws_floats)

    t_info = timed(run)
    kt = kernel_times(run)
    t_table = timed(lambda: fill_wtable(wimg), warm=5, reps=200)
    W1n, W0n, _ = se.tables(cs, kind, cs["params"])
    W1, W0 = torch.from_numpy(W1n.astype(np.float32)).to(dev), torch.from_numpy(W0n.astype(np.float32)).to(dev)
    t_torch = timed(lambda: torch_info(y, T1, T0, call.logw, W1, W0, K), warm=1, reps=3)
    tq = torch_info(y, T1, T0, call.logw, W1, W0, K)
    run()
    torch.cuda.synchronize()
    top = float(info.diagonal().max())
    d_all = float((info - tq[0]).abs().max()) / top
    del tq, ws
    m_ours = peak_of(lambda: eng.item_information(**kw))
    m_torch = peak_of(lambda: torch_info(y, T1, T0, call.logw, W1, W0, K))
    say("%s: N = %d  J = %d  G = %d  P = %d" % (tag, N, J, G, P))
    say("    item_se() end to end           %9.3f ms   (workspace %.1f MB)" % (t_e2e, ws_floats * 4 / 1e6))
    say("    vx_grid_info alone             %9.3f ms" % t_info)
    say("    the table entry alone          %9.3f ms   (one pass; 200 back-to-back calls)" % t_table)
    if kt:
        roof = PEAK_F16_MFMA / 3
        f_ps, f_xp = 2.0 * N * (2 * J * G + 2 * P * G), 2.0 * N * P * (P + 1) / 2
        for k, fl in (("k_grid_pscores", f_ps), ("k_grid_xprod", f_xp)):
            ms = kt[k] / 1e3
            say("    %-30s %9.3f ms   useful %.1f TFLOP/s = %.1f %% of the fp16-pair roofline" % (k + " alone", ms, fl / ms / 1e9, 100 * fl / (ms * 1e-3) / roof))
    say("    torch composition (fp32)       %9.3f ms   slabs of %d persons" % (t_torch, SLAB))
    say("    item_se() / torch              %9.2f x faster (end to end against the composition); all persons, info against torch "
        "fp32: %.2e of the largest diagonal" % (t_torch / t_e2e, d_all))
    say("    peak device memory             %9.1f MB   item_information();  %.1f MB the torch composition" % (m_ours, m_torch))
    rng = np.random.RandomState(77)
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    sub = eng.item_information(rows=torch.from_numpy(idx).to(dev), **kw)
    torch.cuda.synchronize()
    want = se.oracle(cs, kind, cs["params"], y=y[torch.from_numpy(idx).to(dev)].cpu().numpy())
    topw = float(np.diag(want["info"]).max())
    e_i = float(np.abs(sub["info"].cpu().numpy().astype(np.float64) - want["info"]).max()) / topw
    e_g = float(np.abs(sub["gradient"].cpu().numpy().astype(np.float64) - want["gradient"]).max()) / np.sqrt(topw * len(idx))
    say("    %d sampled persons against float64 (row rule %.0e): info %.2e  gradient %.2e" % (len(idx), ROW_TOL, e_i, e_g))
    ok = max(e_i, e_g) <= ROW_TOL
    say("    within the row rule: %s" % ("yes" if ok else "NO"))
    return ok


def irt_shape(tag, N, J, D, nodes, slopes, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    a = rng.uniform(slopes[0], slopes[1], size=(D, J)).astype(np.float32)
    if D > 1:
        a = a * sc.vo.default_a_free(D, J)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    x = torch.randn(N, D, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    del x
    eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1)        # (amortized: no per-person rows to allocate)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt)
    cs = {"name": tag, "N": N, "J": J, "D": D, "nodes": nodes, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "params": {"a": a, "b": b}}
    theta = torch.from_numpy(se.ec.grid_of(cs)[0]).to(dev)
    eps = torch.finfo(torch.float32).eps
    Pm = torch.sigmoid(theta @ at + bt).clamp(eps, 1 - eps)                       # [G][J]
    ok = probe(tag, eng, {"nodes": nodes}, cs, "irt", torch.log(Pm).t().contiguous(), torch.log1p(-Pm).t().contiguous())
    del eng, y
    torch.cuda.empty_cache()
    return ok


def dina_shape(tag, N, J, K, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    q = sc.cdm_q(K, J, rng)
    gs = {"g": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32),
          "s": sc._logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)}
    C = 1 << K
    eta = torch.from_numpy(sc.vo.dina_eta(K, q.astype(np.float64))[0].astype(np.float32)).to(dev)       # [C][J]
    gt, st = torch.sigmoid(torch.from_numpy(gs["g"]).to(dev)), torch.sigmoid(torch.from_numpy(gs["s"]).to(dev))
    pat = torch.randint(0, C, (N,), device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.where(eta[pat] > 0, 1 - st, gt)).to(torch.uint8)
    eng = CcdmEngine(y, q, cdm="dina")
    for k in ("g", "s"):
        eng.unconstrained(k).copy_(torch.from_numpy(gs[k]).to(dev))
    Pt = torch.where(eta > 0, 1 - st, gt)                                                             # [C][J]
    cs = {"name": tag, "N": N, "J": J, "cdm": "dina", "K": K, "q": q, "params": gs}
    ok = probe(tag, eng, {}, cs, "cdm", torch.log(Pt).t().contiguous(), torch.log1p(-Pt).t().contiguous())
    del eng, y
    torch.cuda.empty_cache()
    return ok


def asym_shape(tag, N, J, nodes, model, seed):
    """item_se(prior=) of a 3PL / 4PL engine in one dimension, at the generating values."""
    from tests import se_map_cases as sm
    from vipsy_amd.grid import score_grid
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    four = model == "irt_4pl"
    a = rng.uniform(0.4, 1.0, size=(1, J)).astype(np.float32)
    b = rng.normal(size=(1, J)).astype(np.float32)
    c = sc._logit(rng.uniform(0.1, 0.3, size=(1, J))).astype(np.float32)
    d = sc._logit(rng.uniform(0.85, 0.97, size=(1, J))).astype(np.float32)
    params = {"a": a, "b": b, "c": c}
    prior = {"c": (-1.4, 1.0)}
    if four:
        params["d"] = d
        prior["d"] = (2.2, 1.0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    lo, hi = torch.sigmoid(t["c"]), (torch.sigmoid(t["d"]) if four else 1.0)
    x = torch.randn(N, 1, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < lo + (hi - lo) * torch.sigmoid(x @ t["a"] + t["b"])).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    del x
    eng = IrtEngine(y, model=model, D=1, amortized=True, H=64, seed=1)
    for k, v in t.items():
        eng.unconstrained(k).copy_(v)
    be, kw = eng.be, {"nodes": nodes, "prior": prior}
    t_e2e = timed(lambda: eng.item_se(**kw))
    call, K, fill_wtable, _ = eng._info_call(None, None, **kw)
    post = eng._grid_posterior(call)
    P, G = J * K, call.G
    f32 = dict(dtype=torch.float32, device=dev)
    wimg = torch.empty(be.grid_wimage_bytes(P, G), dtype=torch.uint8, device=dev)
    ws_floats = be.grid_info_workspace(N, P, G)
    info, grad, ws = torch.empty(P, P, **f32), torch.empty(P, **f32), torch.empty(ws_floats, **f32)
    t_table = timed(lambda: fill_wtable(wimg), warm=5, reps=200)

    def run():
        be.grid_info(call.y, None, N, J, G, K, post["img"], wimg, call.logw, post["loglik"], info, grad, ws, ws_floats)

    t_info = timed(run)
    kt = kernel_times(run)
    ktab = kernel_times(lambda: fill_wtable(wimg), ("k_grid_wtable_irt_asym", "k_grid_wscale"))
    say("%s: N = %d  J = %d  G = %d  K = %d  P = %d" % (tag, N, J, G, K, P))
    say("    item_se(prior=) end to end     %9.3f ms   (workspace %.1f MB)" % (t_e2e, ws_floats * 4 / 1e6))
    say("    vx_grid_info alone             %9.3f ms" % t_info)
    say("    the table entry alone          %9.3f ms   (trailer reset, maximum pass, trailer, fill pass; 200 back-to-back calls)" % t_table)
    if ktab:
        say("    k_grid_wtable_irt_asym, both passes %6.1f us   k_grid_wscale %.1f us   (device time inside one call; %d x %d cells)"
            % (ktab["k_grid_wtable_irt_asym"], ktab["k_grid_wscale"], ((G + 31) // 32) * 32, ((P + 32) // 32) * 32))
    if kt:
        roof = PEAK_F16_MFMA / 3
        f_ps, f_xp = 2.0 * N * (2 * J * G + 2 * P * G), 2.0 * N * P * (P + 1) / 2
        for k, fl in (("k_grid_pscores", f_ps), ("k_grid_xprod", f_xp)):
            ms = kt[k] / 1e3
            say("    %-30s %9.3f ms   useful %.1f TFLOP/s = %.1f %% of the fp16-pair roofline" % (k + " alone", ms, fl / ms / 1e9, 100 * fl / (ms * 1e-3) / roof))
    rng = np.random.RandomState(77)
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    rows = torch.from_numpy(idx).to(dev)
    sub = eng.item_information(rows=rows, **kw)
    torch.cuda.synchronize()
    theta, logw = score_grid(1, nodes, 6.0)
    cs = {"name": tag, "model": model, "D": 1, "J": J, "Dc": 1.0, "theta": theta, "logw": logw, "params": params,
          "a_free": np.ones((1, J), bool), "prior": prior, "y": y[rows].cpu().numpy()}
    want = sm.oracle(cs)
    e_i, _, e_g = sm.info_errors(sub["info"].cpu().numpy(), sub["gradient"].cpu().numpy(), want["info"], want["gradient"], len(idx))
    say("    %d sampled persons against float64 (row rule %.0e): info %.2e  gradient %.2e; condition of info + precision %.1f"
        % (len(idx), ROW_TOL, e_i, e_g, want["condition"]))
    ok = max(e_i, e_g) <= ROW_TOL
    say("    within the row rule: %s" % ("yes" if ok else "NO"))
    del eng, y
    torch.cuda.empty_cache()
    return ok


def main():
    args = [a for a in sys.argv[1:]]
    model = None
    if "--model" in args:
        i = args.index("--model")
        model = args[i + 1]
        del args[i:i + 2]
        if model not in ("irt_2pl", "irt_3pl", "irt_4pl"):
            raise SystemExit("--model takes irt_2pl, irt_3pl or irt_4pl")
    out = args[0] if args else None
    say("se_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n = max(4096, int(1000000 * SCALE))
    ok = irt_shape("2PL, 61 nodes", n, 500, 1, 61, (0.4, 1.0), 1)
    if model in ("irt_3pl", "irt_4pl"):
        ok = asym_shape("%s under item priors, 61 nodes" % model[4:].upper(), n, 500, 61, model, 4) and ok
    elif model is None:
        ok = irt_shape("3-D 2PL, 9^3 nodes", n, 40, 3, 9, (0.4, 1.0), 3) and ok
        ok = dina_shape("DINA, K = 8", n, 30, 8, 2) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
