"""fit_population(): what the per-person prior costs beside the shared one, and what an EM iteration of the latent regression takes.

Shape: 1M persons x 500 items x 61 nodes (2PL), p = 8 design columns (intercept, two dummies, five normal covariates), the latent
simulated as Gamma^T x + N(0, 0.8^2).  In the same run, on tables built once and the SAME inputs:
  * vx_grid_posterior_cond beside vx_grid_posterior, and vx_grid_draw_cond beside vx_grid_draw (16 draws: one launch each),
    alternating window by window: device events around REPS = 200 back-to-back calls (0.14 .. 0.37 s a window) behind 3 warm-up
    calls, three windows each, the median and the spread reported;
  * one EM iteration of fit_population (logw and tilt, the kernel, the log-likelihood sum, the M-step's sums, the fetch and the
    p x p solve on the host): wall time of fits of 40 and of 8 iterations (tol = -1: no stop before max_iter), three of each
    alternating behind one warm-up fit; the difference over 32 is an iteration, the rest of the short fit its fixed cost (the
    float64 design, X^T X, the tables);
  * what the fit finds: Gamma against the simulated one, Sigma against 0.64.

usage (GPU box):  python tools/pop_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipsy_amd.engine import IrtEngine, score_grid                               # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
REPS = 200
EM_LONG, EM_SHORT = 40, 8
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed_together(fns, windows=3):
    """Median and (min, max) of `windows` windows of each function, the functions alternating window by window."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            t[k].append(window(fn))
    return [(float(np.median(v)), min(v), max(v)) for v in t]


def fmt(t):
    return "%9.3f ms  (%.3f .. %.3f)" % t


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("pop_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    N, J, D, nodes, p = max(4096, int(1000000 * SCALE)), 500, 1, 61, 8
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rng = np.random.RandomState(1)
    a = rng.uniform(0.4, 1.0, size=(D, J)).astype(np.float32)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    cov = torch.cat([(torch.rand(N, 2, device=dev, generator=g) < 0.5).float(), torch.randn(N, p - 3, device=dev, generator=g)], 1)
    gamma_true = np.array([0.1, 0.5, -0.3, 0.2, -0.15, 0.1, 0.0, 0.1])             # (max |mu| + 4 sd stays inside span = 6 at 1M persons)
    mu = torch.cat([torch.ones(N, 1, device=dev), cov], 1) @ torch.from_numpy(gamma_true).float().to(dev)[:, None]
    x = mu + 0.8 * torch.randn(N, D, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    del x, mu
    eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1)        # (amortized: no per-person rows to allocate)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt)
    theta_np, logw_np = score_grid(D, nodes, 6.0)
    theta, logw = torch.from_numpy(theta_np).to(dev), torch.from_numpy(logw_np).to(dev)
    G = int(theta.shape[0])
    be = eng.be
    cfg = be.cfg("irt_2pl", D, J, 0, 1.0, 1.0, 0, 0, 0)
    img = torch.empty(be.grid_image_bytes(J, G), dtype=torch.uint8, device=dev)
    be.grid_table_irt(cfg, theta, G, eng.unconstrained("a").contiguous(), eng.unconstrained("b").reshape(-1).contiguous(), None, None, img)
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    o = (torch.empty(N, **f32), torch.empty(N, D, **f32), torch.empty(N, D, **f32), torch.empty(N, **i32))
    oc = (torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, D, **f32), torch.empty(N, D * (D + 1) // 2, **f32), torch.empty(N, **i32))
    tilt = (0.5 * torch.randn(N, D, device=dev, generator=g)).contiguous()
    node_a, node_b = torch.empty(N, 16, **i32), torch.empty(N, 16, **i32)

    k_post, k_cond, k_draw, k_dcond = timed_together([
        lambda: be.grid_posterior(y, None, N, J, G, D, img, logw, theta, *o),
        lambda: be.grid_posterior_cond(y, None, N, J, G, D, img, logw, theta, tilt, *oc),
        lambda: be.grid_draw(y, None, N, J, G, img, logw, 1, 0, 0, 16, 16, node_a),
        lambda: be.grid_draw_cond(y, None, N, J, G, D, img, logw, theta, tilt, 1, 0, 0, 16, 16, node_b)])
    flop = 2.0 * N * 2 * J * G
    say("2PL, 61 nodes, p = %d: N = %d  J = %d  G = %d  D = %d   (%d calls a window, 3 windows: median (min .. max))" % (p, N, J, G, D, REPS))
    say("    vx_grid_posterior                      %s   %.1f useful TFLOP/s" % (fmt(k_post), flop / k_post[0] / 1e9))
    say("    vx_grid_posterior_cond                 %s   %.1f useful TFLOP/s; cond / unconditioned = %.3f"
        % (fmt(k_cond), flop / k_cond[0] / 1e9, k_cond[0] / k_post[0]))
    say("    vx_grid_draw, 16 draws                 %s" % fmt(k_draw))
    say("    vx_grid_draw_cond, 16 draws            %s   cond / unconditioned = %.3f" % (fmt(k_dcond), k_dcond[0] / k_draw[0]))

    eng.fit_population(cov, max_iter=2, tol=-1.0)                                 # warm-up: allocator, the float64 products
    torch.cuda.synchronize()
    wall = {EM_LONG: [], EM_SHORT: []}
    for _ in range(3):
        for iters in (EM_LONG, EM_SHORT):
            t0 = time.perf_counter()
            fit = eng.fit_population(cov, max_iter=iters, tol=-1.0)
            torch.cuda.synchronize()
            wall[iters].append(1e3 * (time.perf_counter() - t0))
            assert fit["iterations"] == iters
    per = [(a - b) / (EM_LONG - EM_SHORT) for a, b in zip(wall[EM_LONG], wall[EM_SHORT])]
    it = float(np.median(per))
    say("    one EM iteration of fit_population     %9.3f ms  (%.3f .. %.3f)   (fit of %d - fit of %d iterations) / %d; %.2f x "
        "vx_grid_posterior_cond" % (it, min(per), max(per), EM_LONG, EM_SHORT, EM_LONG - EM_SHORT, it / k_cond[0]))
    say("    fixed cost of a fit                    %9.3f ms   fit of %d iterations (%.3f ms) less %d iterations: the float64 design, "
        "X^T X, the tables" % (float(np.median(wall[EM_SHORT])) - EM_SHORT * it, EM_SHORT, float(np.median(wall[EM_SHORT])), EM_SHORT))
    fit = eng.fit_population(cov, max_iter=200)
    err = float(np.abs(fit["gamma"][:, 0] - gamma_true).max())
    say("    fit_population: %d iterations, converged %s; max |gamma - simulated| = %.4f, sigma = %.4f (simulated 0.64)"
        % (fit["iterations"], fit["converged"], err, fit["sigma"][0, 0]))
    ok = fit["converged"] and err < 0.05 and abs(fit["sigma"][0, 0] - 0.64) < 0.05
    say("    the regression is recovered: %s" % ("yes" if ok else "NO"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
