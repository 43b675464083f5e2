"""plausible_values(): time beside score() at sizes a user would run, and what the draws give back.

Shapes: 1M persons x 500 items x 61 nodes (2PL), 1M x 40 items x 21^2 nodes (2-D 2PL).  For each, in the same run:
  * engine.plausible_values(draws=5) and engine.score() end to end (tables + kernel + output allocation; for the draws the
    gather of theta by node too), alternating, and the two kernels alone (vx_grid_draw with 5 and with 16 draws, one launch each,
    vx_grid_posterior) on tables built once: device events around REPS back-to-back calls behind 3 warm-up calls, three
    windows each, the median and the spread reported;
  * the noise's own cost: useful work of the operand phase is that of k_grid_post (2 * persons * 2 J * G FLOP), the rest is
    one Philox call a (person, node, four draws) and two logarithms a (person, node, draw);
  * what the draws give: the mean over persons of the variance of the drawn theta against the mean squared PSD of score()
    (the same quantity), and the variance over persons of one draw against that of the EAPs: the population variance the EAPs
    understate by the posterior variance.

usage (GPU box):  python tools/pv_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipsy_amd.engine import IrtEngine, score_grid                               # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
REPS = 20
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


def shape(tag, N, J, D, nodes, slopes, seed):
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
    G = int(theta.shape[0])
    be = eng.be
    cfg = be.cfg("irt_2pl", D, J, 0, 1.0, 1.0, 0, 0, 0)
    img = torch.empty(be.grid_image_bytes(J, G), dtype=torch.uint8, device=dev)
    be.grid_table_irt(cfg, theta, G, eng.unconstrained("a").contiguous(), eng.unconstrained("b").reshape(-1).contiguous(), None, None, img)
    f32 = dict(dtype=torch.float32, device=dev)
    o = (torch.empty(N, **f32), torch.empty(N, D, **f32), torch.empty(N, D, **f32), torch.empty(N, dtype=torch.int32, device=dev))
    node5 = torch.empty(N, 5, dtype=torch.int32, device=dev)
    node16 = torch.empty(N, 16, dtype=torch.int32, device=dev)

    t_pv, t_score = timed_together([lambda: eng.plausible_values(draws=5, seed=1, nodes=nodes), lambda: eng.score(nodes=nodes)])
    k_d5, k_d16, k_post = timed_together([lambda: be.grid_draw(y, None, N, J, G, img, logw, 1, 0, 0, 5, 5, node5),
                                          lambda: be.grid_draw(y, None, N, J, G, img, logw, 1, 0, 0, 16, 16, node16),
                                          lambda: be.grid_posterior(y, None, N, J, G, D, img, logw, theta, *o)])
    flop = 2.0 * N * 2 * J * G
    cells = float(N) * (32 * ((G + 31) // 32))
    say("%s: N = %d  J = %d  G = %d  D = %d   (%d calls a window, 3 windows: median (min .. max))" % (tag, N, J, G, D, REPS))
    say("    plausible_values(draws=5) end to end   %s" % fmt(t_pv))
    say("    score() end to end                     %s   plausible_values / score = %.2f" % (fmt(t_score), t_pv[0] / t_score[0]))
    say("    k_grid_draw alone,  5 draws            %s   %.1f ps a (person, node): 2 Philox calls + 10 logarithms" % (fmt(k_d5), 1e9 * k_d5[0] / cells))
    say("    k_grid_draw alone, 16 draws            %s   %.1f ps a (person, node): 4 Philox calls + 32 logarithms; %.3f ms a draw"
        % (fmt(k_d16), 1e9 * k_d16[0] / cells, k_d16[0] / 16))
    say("    k_grid_post alone                      %s   the operand phase both share: %.1f useful TFLOP/s" % (fmt(k_post), flop / k_post[0] / 1e9))
    got = eng.plausible_values(draws=5, seed=1, nodes=nodes)
    s = eng.score(nodes=nodes)
    torch.cuda.synchronize()
    th = got["theta"].double()
    within = float(th.var(dim=1, unbiased=True).mean())
    psd2 = float((s["psd"].double() ** 2).mean())
    say("    5 draws: mean within-person variance of the draws %.4f against mean PSD^2 of score() %.4f (ratio %.3f); variance over "
        "persons of one draw %.4f against that of the EAP %.4f (EAP variance + mean PSD^2: %.4f)"
        % (within, psd2, within / psd2, float(th[:, 0].var(dim=0).mean()), float(s["eap"].double().var(dim=0).mean()),
           float(s["eap"].double().var(dim=0).mean()) + psd2))
    ok = abs(within / psd2 - 1.0) < 0.05 and int(got["node"].min()) >= 0 and int(got["node"].max()) < G
    say("    the draws carry the posterior variance to within 5 %%: %s" % ("yes" if ok else "NO"))
    del eng, y
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("pv_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n = max(4096, int(1000000 * SCALE))
    ok = shape("2PL, 61 nodes", n, 500, 1, 61, (0.4, 1.0), 1)
    ok = shape("2-D 2PL, 21^2 nodes", n, 40, 2, 21, (0.4, 1.0), 3) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
