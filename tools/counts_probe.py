"""expected_counts(): time and accuracy at the three shapes of tools/score_probe.py, beside what a user would write today from
torch operations.

Shapes: 1M persons x 500 items x 61 nodes (2PL), 1M x 30 items x K = 8 (DINA, 256 patterns), 200 k x 100 items x 31^2 nodes
(2-D 2PL).  For each:
  * engine.expected_counts() end to end (tables + posterior kernel + counts kernel + slab sums + prob + allocations), and
    vx_grid_counts alone (the counts kernel and its three slab sums, on tables and loglik made once): device events around 50
    back-to-back calls behind 3 warm-up calls (the torch composition: 10 behind 2);
  * the torch composition on the same GPU: fp32 indicator matmuls for ll, softmax over the nodes ([n][G] in memory), then the
    two fp32 indicator matmuls [y == 1]^T @ p and [y == 0]^T @ p and a column sum -- from the uint8 responses, and with the
    float indicators already made;
  * 4 096 sampled persons (through `rows`) against the float64 oracle of tests/count_cases.py by the row rule of the tests,
    one row = one item; the whole sample's mass as one row;
  * the share of the fp16 MFMA peak: useful FLOP = 2 * persons * 2 J * G for each of the two chained products.
The times are reported, not asserted.

usage (GPU box):  python tools/counts_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import count_cases as cc                                              # noqa: E402  (the float64 oracle)
from tests import score_cases as sc                                              # noqa: E402
from vipsy_amd.engine import CcdmEngine, IrtEngine, score_grid                   # noqa: E402

PEAK_F16_MFMA = 2.5e15       # FLOP/s, dense fp16 MFMA (spec)
ROW_TOL = 3e-5               # the row rule of tests/test_gpu_counts.py
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm=3, reps=50):
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


def torch_counts(y, T1, T0, logw, ind=None):
    """What a user would write today: the posterior of every person in memory, two fp32 indicator matmuls behind it."""
    if ind is None:
        ind = ((y == 1).to(torch.float32), (y == 0).to(torch.float32), (y == 255).sum(1).to(torch.float32))
    f = ind[0] @ T1 + ind[1] @ T0 + (ind[2] * -1.1920928244535389e-07)[:, None] + logw[None, :]
    p = torch.softmax(f, 1)
    return ind[0].t() @ p, ind[1].t() @ p, p.sum(0)


def probe(tag, eng, kw, N, J, G, tables, logw, coord, T1, T0, oracle):
    y, be = eng.y, eng.be
    D = int(coord.shape[1])
    flop = 2 * (2.0 * N * 2 * J * G)
    t_e2e = timed(lambda: eng.expected_counts(**kw))
    t_score = timed(lambda: eng.score(**kw))
    img = torch.empty(be.grid_image_bytes(J, G), dtype=torch.uint8, device=dev)
    tables(img)
    f32 = dict(dtype=torch.float32, device=dev)
    loglik = torch.empty(N, **f32)
    be.grid_posterior(y, None, N, J, G, D, img, logw, coord, loglik, torch.empty(N, D, **f32), torch.empty(N, D, **f32),
                      torch.empty(N, dtype=torch.int32, device=dev))
    n1, n0, mass = torch.empty(J, G, **f32), torch.empty(J, G, **f32), torch.empty(G, **f32)
    ws = torch.empty(be.grid_counts_workspace(N, J, G), **f32)
    t_ker = timed(lambda: be.grid_counts(y, None, N, J, G, img, logw, loglik, n1, n0, mass, ws))
    t_torch = timed(lambda: torch_counts(y, T1, T0, logw), warm=2, reps=10)
    ind = ((y == 1).to(torch.float32), (y == 0).to(torch.float32), (y == 255).sum(1).to(torch.float32))
    t_torch_pre = timed(lambda: torch_counts(y, T1, T0, logw, ind), warm=2, reps=10)
    tq = torch_counts(y, T1, T0, logw, ind)
    got = eng.expected_counts(**kw)
    torch.cuda.synchronize()
    # the two routes against each other on ALL persons (float32 both; the sampled float64 comparison follows)
    d_all = max(row_err(got["n1"].cpu().numpy().astype(np.float64), tq[0].cpu().numpy().astype(np.float64)),
                row_err(got["n0"].cpu().numpy().astype(np.float64), tq[1].cpu().numpy().astype(np.float64)))
    del ind, tq
    say("%s: N = %d  J = %d  G = %d" % (tag, N, J, G))
    say("    expected_counts() end to end   %9.3f ms   (score() on the same data: %.3f ms; workspace %.1f MB)"
        % (t_e2e, t_score, ws.numel() * 4 / 1e6))
    say("    vx_grid_counts alone           %9.3f ms   useful %.1f TFLOP/s = %.2f %% of the fp16 MFMA peak (both products; issued: "
        "x2 + padding)" % (t_ker, flop / t_ker / 1e9, 100 * flop / (t_ker * 1e-3) / PEAK_F16_MFMA))
    say("    torch composition (fp32)       %9.3f ms   from the uint8 responses;  %.3f ms with the float indicators already made; "
        "[n][G] posterior in memory: %.0f MB" % (t_torch, t_torch_pre, N * G * 4 / 1e6))
    say("    expected_counts() / torch      %9.2f x faster (end to end against from-uint8); all persons, kernel against torch "
        "fp32, row rule: %.2e" % (t_torch / t_e2e, d_all))
    rng = np.random.RandomState(77)
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    sub = eng.expected_counts(rows=torch.from_numpy(idx).to(dev), **kw)
    torch.cuda.synchronize()
    want = oracle(y[torch.from_numpy(idx).to(dev)].cpu().numpy())
    e1 = row_err(sub["n1"].cpu().numpy().astype(np.float64), want["n1"])
    e0 = row_err(sub["n0"].cpu().numpy().astype(np.float64), want["n0"])
    em = row_err(sub["mass"].cpu().numpy().astype(np.float64)[None, :], want["mass"][None, :])
    ep = float(np.abs(sub["prob"].cpu().numpy().astype(np.float64) - want["prob"]).max())
    fit = {k: v.cpu().numpy() for k, v in eng.item_fit(rows=idx, **kw).items()}
    emd, ermsd = float(np.abs(fit["md"] - want["md"]).max()), float(np.abs(fit["rmsd"] - want["rmsd"]).max())
    say("    %d sampled persons against float64 (row rule %.0e): n1 %.2e  n0 %.2e  mass %.2e  prob %.2e  md %.2e  rmsd %.2e"
        % (len(idx), ROW_TOL, e1, e0, em, ep, emd, ermsd))
    ok = max(e1, e0, em, ep, emd, ermsd) <= ROW_TOL
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
    eps = torch.finfo(torch.float32).eps
    P = torch.sigmoid(theta @ at + bt).clamp(eps, 1 - eps)                        # [G][J]
    T1, T0 = torch.log(P).t().contiguous(), torch.log1p(-P).t().contiguous()
    cs = {"D": D, "nodes": nodes, "span": 6.0, "model": "irt_2pl", "Dc": 1.0, "params": {"a": a, "b": b}}
    ok = probe(tag, eng, {"nodes": nodes}, N, J, G, lambda img: eng.be.grid_table_irt(cfg, theta, G, aa, bb, None, None, img),
               logw, theta, T1, T0, lambda ys: cc.irt_oracle(dict(cs, y=ys)))
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
    cs = {"cdm": "dina", "K": K, "q": q, "params": gs}
    ok = probe(tag, eng, {}, N, J, C, lambda img: eng.be.grid_table_cdm(cfg, False, eng.q, eng.view("g"), eng.view("s"), img),
               logw, coord, torch.log(Pt).t().contiguous(), torch.log1p(-Pt).t().contiguous(),
               lambda ys: cc.cdm_oracle(dict(cs, y=ys)))
    del eng, y
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("counts_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
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
