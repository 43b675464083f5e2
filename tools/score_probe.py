"""score(): time and accuracy at sizes a user would run, beside what a user would write today from torch operations.

Shapes: 1M persons x 500 items x 61 nodes (2PL), 1M x 30 items x K = 8 (DINA, 256 patterns), 200 k x 100 items x 31^2 nodes
(2-D 2PL).  For each:
  * engine.score() end to end (tables + posterior kernel + output allocation), and the posterior kernel alone (vx_grid_posterior
    on tables built once): device events around 200 back-to-back calls behind 5 warm-up calls (the torch composition: 20 behind 3);
  * the torch composition on the same GPU: fp32 indicator matmuls [y == 1] @ T1 + [y == 0] @ T0, + logw, logsumexp, softmax
    moments, argmax -- with the indicators made INSIDE the timed region from the same uint8 responses (that is what a call on
    new data costs) and, separately, with the float indicators already in memory;
  * 4 096 sampled persons of the kernel's output against the float64 oracle (tests/score_cases.py) by the row rule of the
    tests, |got - want|_inf <= 3e-5 max(|want|_inf, 1);
  * the share of the rooflines: useful FLOP = 2 * persons * 2 J * G (the two indicator products; the kernel issues twice that,
    head and low term, on tiles padded to 16 items x 32 nodes), bytes = the responses read + the outputs written.

usage (GPU box):  python tools/score_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import score_cases as sc                                              # noqa: E402  (the float64 oracle)
from vipsy_amd.engine import CcdmEngine, IrtEngine, score_grid                   # noqa: E402

PEAK_F16_MFMA = 2.5e15       # FLOP/s, dense fp16 MFMA (spec)
PEAK_HBM = 8.0e12            # B/s (spec; 6.3e12 is what a copy reaches)
ROW_TOL = 3e-5               # the row rule of tests/test_gpu_score.py
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm=5, reps=200):
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


def row_err(got, want):
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    return float((np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), 1.0)).max())


def torch_tables_irt(theta, a, b, Dc):
    z = Dc * (theta @ a + b)                                                     # [G][J]
    eps = torch.finfo(torch.float32).eps
    P = torch.sigmoid(z).clamp(eps, 1 - eps)
    return torch.log(P).t().contiguous(), torch.log1p(-P).t().contiguous()      # T1, T0 [J][G]


def torch_posterior(y, T1, T0, logw, coord, ind=None):
    """What a user would write today: fp32 indicator matmuls, logsumexp, softmax moments."""
    if ind is None:
        ind = ((y == 1).to(torch.float32), (y == 0).to(torch.float32), (y == 255).sum(1).to(torch.float32))
    f = ind[0] @ T1 + ind[1] @ T0 + (ind[2] * -1.1920928244535389e-07)[:, None] + logw[None, :]
    loglik = torch.logsumexp(f, 1)
    p = torch.softmax(f, 1)
    mean = p @ coord
    sd = (p @ (coord * coord) - mean * mean).clamp_min(0).sqrt()
    return loglik, mean, sd, f.argmax(1)


def probe(tag, eng, score_kw, N, J, G, D, tables, logw, coord, oracle):
    y = eng.y
    flop = 2.0 * N * 2 * J * G
    byts = N * J + N * (4 + 4 + 8 * D)
    t_score = timed(lambda: eng.score(**score_kw))
    # the posterior kernel alone, on tables built once
    img = torch.empty(eng.be.grid_image_bytes(J, G), dtype=torch.uint8, device=dev)
    tables(img)
    f32 = dict(dtype=torch.float32, device=dev)
    o = (torch.empty(N, **f32), torch.empty(N, D, **f32), torch.empty(N, D, **f32), torch.empty(N, dtype=torch.int32, device=dev))
    t_tab = timed(lambda: tables(img))
    t_ker = timed(lambda: eng.be.grid_posterior(y, None, N, J, G, D, img, logw, coord, *o))
    T1, T0 = oracle["tables"]
    t_torch = timed(lambda: torch_posterior(y, T1, T0, logw, coord), warm=3, reps=20)
    ind = ((y == 1).to(torch.float32), (y == 0).to(torch.float32), (y == 255).sum(1).to(torch.float32))
    t_torch_pre = timed(lambda: torch_posterior(y, T1, T0, logw, coord, ind), warm=3, reps=20)
    bound = max(flop / PEAK_F16_MFMA, byts / PEAK_HBM)
    say("%s: N = %d  J = %d  G = %d  D = %d" % (tag, N, J, G, D))
    say("    score() end to end          %9.3f ms   (tables alone %.3f ms)" % (t_score, t_tab))
    say("    k_grid_post alone           %9.3f ms   useful %.1f TFLOP/s = %.2f %% of the fp16 MFMA peak (issued: x2 + padding); "
        "%.1f GB/s = %.2f %% of the HBM peak; roofline bound %.4f ms (%s) -> %.1f %% of it"
        % (t_ker, flop / t_ker / 1e9, 100 * flop / (t_ker * 1e-3) / PEAK_F16_MFMA, byts / t_ker / 1e6,
           100 * byts / (t_ker * 1e-3) / PEAK_HBM, 1e3 * bound, "MFMA" if flop / PEAK_F16_MFMA > byts / PEAK_HBM else "HBM",
           100 * bound * 1e3 / t_ker))
    say("    torch composition (fp32)    %9.3f ms   from the uint8 responses;  %.3f ms with the float indicators already made"
        % (t_torch, t_torch_pre))
    say("    score() / torch             %9.2f x faster (end to end against from-uint8)" % (t_torch / t_score))
    del ind
    # accuracy: 4 096 sampled persons against float64
    rng = np.random.RandomState(77)
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    got = eng.score(**score_kw)
    torch.cuda.synchronize()
    it = torch.from_numpy(idx).to(dev)
    want = oracle["fn"](y[it].cpu().numpy())
    names = [k for k in got if k not in ("node", "pattern", "loglik")]
    e_ll = row_err(got["loglik"][it].cpu().numpy().astype(np.float64), want["loglik"])
    e_mean = row_err(got[names[0]][it].cpu().numpy().astype(np.float64), want["mean"])
    e_sd = row_err(got["psd"][it].cpu().numpy().astype(np.float64), want["sd"]) if "psd" in got else float("nan")
    nk = "node" if "node" in got else "pattern"
    sure = want["gap"] > sc.ARGMAX_GAP
    wrong = int((sure & (got[nk][it].cpu().numpy().astype(np.int64) != want["node"])).sum())
    tq = torch_posterior(y[it], T1, T0, logw, coord)
    say("    %d sampled persons against float64 (row rule %.0e): loglik %.2e  %s %.2e  psd %.2e; %d wrong nodes, %.2f %% left out "
        "as tied; the torch composition's own errors: loglik %.2e  mean %.2e  sd %.2e"
        % (len(idx), ROW_TOL, e_ll, names[0], e_mean, e_sd, wrong, 100 * (1 - sure.mean()),
           row_err(tq[0].cpu().numpy().astype(np.float64), want["loglik"]), row_err(tq[1].cpu().numpy().astype(np.float64), want["mean"]),
           row_err(tq[2].cpu().numpy().astype(np.float64), want["sd"])))
    ok = e_ll <= ROW_TOL and e_mean <= ROW_TOL and not (e_sd > ROW_TOL) and wrong == 0
    say("    within the row rule: %s" % ("yes" if ok else "NO"))
    return ok


def irt_shape(tag, N, J, D, nodes, slopes, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    a = rng.uniform(slopes[0], slopes[1], size=(D, J)).astype(np.float32)
    if D > 1:
        for i in range(D):
            a[i, J - i:] = 0
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    x = torch.randn(N, D, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    del x
    eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1)        # (amortized: no per-person rows to allocate)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt)
    theta_np, logw_np = score_grid(D, nodes, 6.0)
    theta, logw = torch.from_numpy(theta_np).to(dev), torch.from_numpy(logw_np).to(dev)
    cfg = eng.be.cfg("irt_2pl", D, J, 0, 1.0, 1.0, 0, 0, 0)
    aa, bb = eng.unconstrained("a").contiguous(), eng.unconstrained("b").reshape(-1).contiguous()
    G = int(theta.shape[0])

    def oracle(ys):
        ll = sc.irt_grid_loglik("irt_2pl", theta_np, {"a": a, "b": b}, 1.0, ys)
        return sc.grid_posterior(ll, logw_np, theta_np)
    ok = probe(tag, eng, {"nodes": nodes}, N, J, G, D, lambda img: eng.be.grid_table_irt(cfg, theta, G, aa, bb, None, None, img),
               logw, theta, {"tables": torch_tables_irt(theta, at, bt, 1.0), "fn": oracle})
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
    P = torch.where(eta[pat] > 0, 1 - st, gt)
    y = (torch.rand(N, J, device=dev, generator=g) < P).to(torch.uint8)
    del P
    eng = CcdmEngine(y, q, cdm="dina")
    for k in ("g", "s"):
        eng.unconstrained(k).copy_(torch.from_numpy(gs[k]).to(dev))
    coord = ((torch.arange(C, device=dev)[:, None] >> torch.arange(K, device=dev)[None, :]) & 1).to(torch.float32).contiguous()
    logw = torch.full((C,), float(np.log(1.0 / C)), dtype=torch.float32, device=dev)
    cfg = eng.be.hodina_cfg(K, J, 0, 1.0, 0, 0, 0)
    Pt = torch.where(eta > 0, 1 - st, gt)                                                             # [C][J]
    tabs = (torch.log(Pt).t().contiguous(), torch.log1p(-Pt).t().contiguous())

    def oracle(ys):
        ll, lw, attrs = sc.cdm_grid_loglik("dina", K, q, gs, ys)
        return sc.grid_posterior(ll, lw, attrs)
    ok = probe(tag, eng, {}, N, J, C, K, lambda img: eng.be.grid_table_cdm(cfg, False, eng.q, eng.view("g"), eng.view("s"), img),
               logw, coord, {"tables": tabs, "fn": oracle})
    del eng, y
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("score_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n1, n3 = max(4096, int(1000000 * SCALE)), max(4096, int(200000 * SCALE))
    ok = irt_shape("2PL, 61 nodes", n1, 500, 1, 61, (0.4, 1.0), 1)
    ok = dina_shape("DINA, K = 8", n1, 30, 8, 2) and ok
    ok = irt_shape("2-D 2PL, 31^2 nodes", n3, 100, 2, 31, (0.4, 1.0), 3) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
