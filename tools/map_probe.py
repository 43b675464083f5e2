"""fit_em(prior=): device time of the penalised M-step launch beside the unpenalised one, and its share of an EM iteration.

Shape: 1M persons x 500 items x 61 nodes, the 2PL shape of tools/em_probe.py, with responses drawn from a 4PL so that every
model has something to fit.  Measured:
  * vx_grid_mstep_irt_map with newton = 4 for 2PL / 3PL / 4PL, on that model's own tables (made once, at the start values):
    device events around 50 back-to-back launches behind 3 -- the launches update their copies in place, so all but the first
    start near the maximiser: the Newton steps are still taken, the halvings of a bad start are not in this number;
  * vx_grid_mstep_irt, the parent's entry, on the same 2PL tables, the same way: the comparison;
  * one fit_em(prior=) iteration for each model: device events around a call of 20 iterations (tol = -1: never converged)
    behind a warm-up call of 3, divided by 20.
The times are reported, not asserted; no target is set -- the M-step reads 2 J G floats and is a small share of an iteration.

usage (GPU box):  python tools/map_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipsy_amd.engine import IrtEngine, score_grid                               # noqa: E402
from vipsy_amd.grid import em_prior                                              # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
PRIORS = {"irt_2pl": {"a": (1.0, 0.5)}, "irt_3pl": {"c": (-1.4, 1.0)}, "irt_4pl": {"c": (-1.4, 1.0), "d": (2.2, 1.0)}}
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


def responses(N, J, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    f = lambda lo, hi: torch.from_numpy(rng.uniform(lo, hi, size=(1, J)).astype(np.float32)).to(dev)   # noqa: E731
    a, b, c, d = f(0.7, 1.8), f(-1.5, 1.5), f(0.1, 0.3), f(0.85, 0.98)
    x = torch.randn(N, 1, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < c + (d - c) * torch.sigmoid(1.702 * (x * a + b))).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.10] = 255
    return y


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("map_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    N, J, nodes = max(4096, int(1000000 * SCALE)), 500, 61
    theta = torch.from_numpy(score_grid(1, nodes, 6.0)[0]).to(dev)
    G = int(theta.shape[0])
    y = responses(N, J, 1)
    say("N = %d  J = %d  G = %d  (the M-step reads 2 J G floats = %.2f MB)" % (N, J, G, 2 * J * G * 4 / 1e6))
    for model in ("irt_2pl", "irt_3pl", "irt_4pl"):
        eng = IrtEngine(y, model=model, D=1, Dc=1.702, amortized=True, H=64, seed=1)
        for name, v in (("c", -1.4), ("d", 2.2)):
            if name in eng.names():
                eng.unconstrained(name).fill_(v)
        kw = {"nodes": nodes}
        c = eng.expected_counts(**kw)
        cfg = eng.be.cfg(model, 1, J, 0, 1.702, 1.0, 0, 0, 0)
        flat = lambda n: eng.unconstrained(n).reshape(-1).contiguous().clone() if n in eng.names() else None    # noqa: E731
        a, b, cu, du = eng.unconstrained("a").contiguous().clone(), flat("b"), flat("c"), flat("d")
        pr = torch.from_numpy(em_prior(PRIORS[model], model, 1, J)).to(dev)
        lp = torch.empty(J, device=dev)
        t_map = timed(lambda: eng.be.grid_mstep_irt_map(cfg, theta, G, c["n1"], c["n0"], None, a, b, cu, du, pr, 4, lp))
        say("%s" % model)
        say("    vx_grid_mstep_irt_map, newton = 4        %9.3f ms" % t_map)
        if model == "irt_2pl":
            a2, b2 = eng.unconstrained("a").contiguous().clone(), flat("b")
            t_ml = timed(lambda: eng.be.grid_mstep_irt(cfg, theta, G, c["n1"], c["n0"], None, a2, b2, 4))
            say("    vx_grid_mstep_irt, the same tables       %9.3f ms   (the penalised launch: %.2f x)" % (t_ml, t_map / t_ml))
        eng.fit_em(max_iter=3, tol=-1.0, prior=PRIORS[model], **kw)
        t_iter = timed(lambda: eng.fit_em(max_iter=20, tol=-1.0, prior=PRIORS[model], **kw), warm=0, reps=1) / 20
        say("    fit_em(prior=), one iteration (of 20)    %9.3f ms   the M-step launch is %.1f %% of it" % (t_iter, 100 * t_map / t_iter))
        del eng
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
