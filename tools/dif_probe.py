"""dif(): what the grouped tables cost at 1M persons x 500 items x 61 nodes (2PL), H = 1, 8 and 80 groups of equal size.

Three ways to the same tables, on the operand image and the normalisers made once, the persons reached through `rows` sorted by
group (as dif() hands them over):
  * vx_grid_counts_cond: ONE launch over all groups (the table writer, the segment kernel and its three slab sums), under a
    tilt a group;
  * vx_grid_counts once over all persons: the floor -- the same products with one table set and no tilt;
  * vx_grid_counts called H times through `rows`, one group a call: what there was before the segment kernel (N(0, I) only).
Device events around 20 back-to-back calls behind 3 warm-up calls; the three are timed in turn, three rounds, and the lowest and
highest round are reported beside the median.  Then dif() end to end (impact=False and impact=True) at H = 8, and the segment
launch against the float64 oracle on sampled persons of one group.  The times are reported, not asserted.

usage (GPU box):  python tools/dif_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import dif_cases as dc                                                # noqa: E402  (the float64 oracle)
from tests import score_cases as sc                                              # noqa: E402
from vipsy_amd.engine import IrtEngine, score_grid                               # noqa: E402
from vipsy_amd.grid import population_logw                                       # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
SIGMA = 0.64
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm=3, reps=20):
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


def rounds(fns, n=3):
    """Every function timed in turn, n rounds: {name: (median, lowest, highest)} in ms."""
    t = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("dif_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    N, J, D, nodes = max(8192, int(1000000 * SCALE)), 500, 1, 61
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rng = np.random.RandomState(1)
    a = rng.uniform(0.4, 1.0, size=(D, J)).astype(np.float32)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    for H in (1, 8, 80):
        label = torch.randint(0, H, (N,), device=dev, generator=g)
        label[:H] = torch.arange(H, device=dev)
        mean = torch.linspace(-0.75, 0.75, H, device=dev) if H > 1 else torch.zeros(1, device=dev)
        x = mean[label][:, None] + 0.8 * torch.randn(N, D, device=dev, generator=g)
        y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
        y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
        del x
        eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1)    # (amortized: no per-person rows to allocate)
        eng.unconstrained("a").copy_(at)
        eng.unconstrained("b").copy_(bt)
        be = eng.be
        order = torch.argsort(label, stable=True)
        counts = torch.bincount(label, minlength=H).cpu().numpy()
        seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        theta_np, logw0_np = score_grid(D, nodes, 6.0)
        G = int(theta_np.shape[0])
        call = eng._grid_call(None, order, nodes, 6.0)
        lw = torch.from_numpy(population_logw(theta_np, SIGMA * np.eye(D))).to(dev)
        tilt = (mean[label[order]][:, None] / SIGMA).to(torch.float32).contiguous()
        cond = eng._grid_posterior_cond(call._replace(logw=lw), tilt)
        post = eng._grid_posterior(call)
        img, logjoint, loglik = post["img"], cond["logjoint"], post["loglik"]
        n1, n0, mass = torch.empty(H, J, G, **f32), torch.empty(H, J, G, **f32), torch.empty(H, G, **f32)
        ws = torch.empty(be.grid_counts_cond_workspace(N, H, J, G), **f32)
        ws0 = torch.empty(be.grid_counts_workspace(N, J, G), **f32)
        ws1 = [torch.empty(be.grid_counts_workspace(int(c), J, G), **f32) for c in counts]
        parts = [(order[seg[h]:seg[h + 1]].contiguous(), loglik[seg[h]:seg[h + 1]].contiguous()) for h in range(H)]

        def seg_launch():
            be.grid_counts_cond(y, order, N, J, G, D, img, lw, call.theta, tilt, logjoint, seg, n1, n0, mass, ws)

        def once():
            be.grid_counts(y, order, N, J, G, img, call.logw, loglik, n1[0], n0[0], mass[0], ws0)

        def h_times():
            for h in range(H):
                be.grid_counts(y, parts[h][0], int(counts[h]), J, G, img, call.logw, parts[h][1], n1[h], n0[h], mass[h], ws1[h])

        t = rounds({"seg": seg_launch, "once": once, "h": h_times})
        say("H = %d: N = %d  J = %d  G = %d, groups of %d .. %d persons; workspace %.1f MB (vx_grid_counts: %.1f MB)"
            % (H, N, J, G, counts.min(), counts.max(), ws.numel() * 4 / 1e6, ws0.numel() * 4 / 1e6))
        for k, name in (("seg", "vx_grid_counts_cond, one launch over the groups"), ("once", "vx_grid_counts once over all persons"),
                        ("h", "vx_grid_counts H times through rows")):
            say("    %-52s %9.3f ms   (%.3f .. %.3f)" % (name, t[k][0], t[k][1], t[k][2]))
        say("    H calls / one segment launch: %.2f;  segment launch / one unconditioned call: %.2f" % (t["h"][0] / t["seg"][0],
                                                                                                      t["seg"][0] / t["once"][0]))
        if H == 8:
            groups = label.cpu().numpy()
            t_flat = timed(lambda: eng.dif(groups, impact=False), warm=1, reps=3)
            t0 = time.time()
            r = eng.dif(groups)
            torch.cuda.synchronize()
            say("    dif(impact=False) end to end                         %9.3f ms;  dif(impact=True), its private population fit "
                "included: %.0f ms (group means %.3f .. %.3f, sigma %.3f)" % (t_flat, 1e3 * (time.time() - t0), r["group_mean"].min(),
                                                                            r["group_mean"].max(), r["sigma"][0, 0]))
            # the segment launch against float64 on 2 048 sampled persons of group 3 and 2 048 of group 5, two segments
            seg_launch()
            torch.cuda.synchronize()
            k = int(min(2048, counts.min()))
            pick = np.concatenate([np.sort(rng.choice(np.arange(seg[h], seg[h + 1]), size=k, replace=False)) for h in (3, 5)])
            rows_s = order[torch.from_numpy(pick).to(dev)].contiguous()
            seg_s = np.array([0, k, 2 * k], np.int64)
            sub = {k_: torch.empty(2, J, G, **f32) for k_ in ("n1", "n0")}
            sub["mass"] = torch.empty(2, G, **f32)
            tl = tilt[torch.from_numpy(pick).to(dev)].contiguous()
            be.grid_counts_cond(y, rows_s, 2 * k, J, G, D, img, lw, call.theta, tl, logjoint[torch.from_numpy(pick).to(dev)].contiguous(),
                                seg_s, sub["n1"], sub["n0"], sub["mass"], torch.empty(be.grid_counts_cond_workspace(2 * k, 2, J, G), **f32))
            torch.cuda.synchronize()
            ys = y[rows_s].cpu().numpy()
            cs = {"model": "irt_2pl", "Dc": 1.0, "params": {"a": a, "b": b}, "J": J}
            ll = sc.irt_grid_loglik("irt_2pl", theta_np, cs["params"], 1.0, ys)
            want = dc.segment_counts(ll, theta_np, lw.cpu().numpy().astype(np.float64), tl.cpu().numpy().astype(np.float64), ys, seg_s)
            errs = dc.table_errors({k: v.cpu().numpy() for k, v in sub.items()}, want)
            say("    %d sampled persons of two groups against float64, row metric: n1 %.2e  n0 %.2e  mass %.2e"
                % (2 * k, errs["n1"][0], errs["n0"][0], errs["mass"][0]))
        del eng, y, ws, ws0, ws1, parts, n1, n0, mass, cond, post
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
