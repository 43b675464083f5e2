"""fit_em(): time of an EM iteration at the three shapes of tools/counts_probe.py, the M-step's share of it, and what a user could
write today: expected_counts() followed by the same M-step in torch operations on the same GPU.

Shapes: 1M persons x 500 items x 61 nodes (2PL), 1M x 30 items x K = 8 (DINA, 256 patterns), 200 k x 100 items x 31^2 nodes
(2-D 2PL, triangular mask).  For each:
  * engine.fit_em(max_iter = 20, tol = -1: never converged) behind one warm-up call of 3 iterations: device events around the
    whole call, divided by 20 -- tables, posterior kernel, loglik sum, counts kernel, M-step, write-back and the host's one
    float an iteration, buffers made once a call;
  * the M-step launch alone (vx_grid_mstep_irt with newton = 4 / vx_grid_mstep_cdm, on tables made once): device events around
    50 back-to-back launches behind 3 (the launches update their copies in place, so all but the first start at the maximiser:
    the Newton steps are still taken, the halvings of a bad start are not in this number);
  * the composition: engine.expected_counts() and a batched torch M-step over all items -- for IRT 4 plain Newton steps (no step
    control: less work than the kernel does) on the [J][G] tables, for DINA the closed form through an eta matrix -- 10 runs
    behind 2.
The times are reported, not asserted.

usage (GPU box):  python tools/em_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import score_cases as sc                                              # noqa: E402
from vipsy_amd.engine import CcdmEngine, IrtEngine, score_grid                   # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
ZL = 15.942384719848633
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


def torch_newton(theta, n1, n0, a, b, free, steps=4):
    """Plain Newton on every item at once: U [G][P], p [J][P] = (b, a); masked loadings as unit rows."""
    G, D = theta.shape
    U = torch.cat([torch.ones(G, 1, device=dev), theta], 1)
    p = torch.cat([b.reshape(1, -1), a], 0).t().contiguous()                      # [J][P]
    fr = torch.cat([torch.ones(1, a.shape[1], device=dev), free], 0).t().contiguous()
    eye = torch.eye(D + 1, device=dev)[None]
    n = n1 + n0
    for _ in range(steps):
        z = p @ U.t()
        zc = z.clamp(-ZL, ZL)
        inside = (zc == z).to(torch.float32)
        sg = torch.sigmoid(zc)
        r = (n1 - n * sg) * inside
        w = n * sg * (1 - sg) * inside
        g = (r @ U) * fr
        H = torch.einsum("jg,gp,gq->jpq", w, U, U)
        m = fr[:, :, None] * fr[:, None, :]
        H = H * m + eye * (1 - m)
        p = p + torch.linalg.solve(H, g[:, :, None])[:, :, 0]
    return p[:, 1:].t().contiguous(), p[:, 0].contiguous()


def torch_cdm(eta, n1, n0):
    R1, W1 = (n1 * eta).sum(1), (n0 * eta).sum(1)
    R0, W0 = (n1 * (1 - eta)).sum(1), (n0 * (1 - eta)).sum(1)
    return (R0.log() - W0.log()).clamp(-ZL, ZL), (W1.log() - R1.log()).clamp(-ZL, ZL)


def report(tag, N, J, G, t_iter, t_m, t_comp, t_counts):
    say("%s: N = %d  J = %d  G = %d" % (tag, N, J, G))
    say("    fit_em, one iteration (of 20)           %9.3f ms" % t_iter)
    say("    M-step launch alone                     %9.3f ms   = %.1f %% of the iteration (it reads 2 J G floats = %.2f MB)"
        % (t_m, 100 * t_m / t_iter, 2 * J * G * 4 / 1e6))
    say("    expected_counts() + torch M-step        %9.3f ms   (expected_counts() alone: %.3f ms)   %.2f x the fit_em iteration"
        % (t_comp, t_counts, t_comp / t_iter))


def em_time(eng, kw):
    eng.fit_em(max_iter=3, tol=-1.0, **kw)
    return timed(lambda: eng.fit_em(max_iter=20, tol=-1.0, **kw), warm=0, reps=1) / 20


def irt_shape(tag, N, J, D, nodes, slopes, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    a = rng.uniform(slopes[0], slopes[1], size=(D, J)).astype(np.float32)
    for i in range(D if D > 1 else 0):
        a[i, J - i:] = 0
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(rng.normal(size=(1, J)).astype(np.float32)).to(dev)
    x = torch.randn(N, D, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    del x
    eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1, a0=torch.full((D, J), 0.5 if D > 1 else 1.0))
    kw = {"nodes": nodes}
    theta = torch.from_numpy(score_grid(D, nodes, 6.0)[0]).to(dev)
    G = int(theta.shape[0])
    free = eng.unconstrained("a", eng.free).contiguous().clone()
    c = eng.expected_counts(**kw)
    a0, b0 = eng.unconstrained("a").contiguous().clone(), eng.unconstrained("b").reshape(-1).contiguous().clone()
    aa, bb = a0.clone(), b0.clone()
    cfg = eng.be.cfg("irt_2pl", D, J, 0, 1.0, 1.0, 0, 0, 0)
    t_m = timed(lambda: eng.be.grid_mstep_irt(cfg, theta, G, c["n1"], c["n0"], free, aa, bb, 4))
    t_counts = timed(lambda: eng.expected_counts(**kw), warm=2, reps=10)

    def comp():
        cc_ = eng.expected_counts(**kw)
        return torch_newton(theta, cc_["n1"], cc_["n0"], a0, b0, free)

    k1a, k1b = a0.clone(), b0.clone()
    eng.be.grid_mstep_irt(cfg, theta, G, c["n1"], c["n0"], free, k1a, k1b, 4)
    torch.cuda.synchronize()
    try:
        t_comp = timed(comp, warm=2, reps=10)
        ta, tb = torch_newton(theta, c["n1"], c["n0"], a0, b0, free)
        diff = "a %.2e  b %.2e" % (float((k1a - ta).abs().max()), float((k1b - tb).abs().max()))
    except Exception as e:                                                        # noqa: BLE001  (reported, not hidden)
        t_comp, diff = float("nan"), "the torch composition failed: %s" % str(e).splitlines()[0]
    t_iter = em_time(eng, kw)
    report(tag, N, J, G, t_iter, t_m, t_comp, t_counts)
    say("    kernel against torch after 4 Newton steps from the same start: %s" % diff)
    del eng, y
    torch.cuda.empty_cache()


def dina_shape(tag, N, J, K, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    q = sc.cdm_q(K, J, rng)
    C = 1 << K
    eta = torch.from_numpy(sc.vo.dina_eta(K, q.astype(np.float64))[0].astype(np.float32)).to(dev)       # [C][J]
    gt = torch.from_numpy(rng.uniform(0.05, 0.25, size=(1, J)).astype(np.float32)).to(dev)
    st = torch.from_numpy(rng.uniform(0.05, 0.25, size=(1, J)).astype(np.float32)).to(dev)
    pat = torch.randint(0, C, (N,), device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.where(eta[pat] > 0, 1 - st, gt)).to(torch.uint8)
    eng = CcdmEngine(y, q, cdm="dina")
    c = eng.expected_counts()
    gg, ss = eng.view("g").clone(), eng.view("s").clone()
    cfg = eng.be.hodina_cfg(K, J, 0, 1.0, 0, 0, 0)
    t_m = timed(lambda: eng.be.grid_mstep_cdm(cfg, False, eng.q, c["n1"], c["n0"], gg, ss))
    t_counts = timed(lambda: eng.expected_counts(), warm=2, reps=10)
    etaT = eta.t().contiguous()

    def comp():
        cc_ = eng.expected_counts()
        return torch_cdm(etaT, cc_["n1"], cc_["n0"])

    t_comp = timed(comp, warm=2, reps=10)
    tg, ts = comp()
    torch.cuda.synchronize()
    t_iter = em_time(eng, {})
    report(tag, N, J, C, t_iter, t_m, t_comp, t_counts)
    say("    kernel against torch, probability scale: g %.2e  s %.2e"
        % (float((torch.sigmoid(gg) - torch.sigmoid(tg)).abs().max()), float((torch.sigmoid(ss) - torch.sigmoid(ts)).abs().max())))
    del eng, y
    torch.cuda.empty_cache()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("em_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n1, n3 = max(4096, int(1000000 * SCALE)), max(4096, int(200000 * SCALE))
    irt_shape("2PL, 61 nodes", n1, 500, 1, 61, (0.4, 1.0), 1)
    dina_shape("DINA, K = 8", n1, 30, 8, 2)
    irt_shape("2-D 2PL, 31^2 nodes", n3, 100, 2, 31, (0.4, 1.0), 3)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
