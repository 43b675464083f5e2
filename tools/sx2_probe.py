"""sx2(): the times of the three summed-score kernels beside score(), at the headline shape and on a 70-item test.

Shapes: 1M persons x 500 items x 61 nodes and 1M persons x 70 items x 61 nodes (2PL, complete data: S-X2 counts complete persons).
Reported for each:
  * vx_sumscore_model (with and without dist), vx_sumscore_persons and vx_sumscore_observed alone, on buffers made once, and
    engine.score() on the same data as the yardstick: device events around back-to-back calls behind a warm-up call;
  * engine.sumscore_tables() and engine.sx2() end to end (tables, the three kernels, the sort on the device, the host layer);
  * the device time of the kernels inside one vx_sumscore_model call, by torch.profiler, and the workspace;
  * the recursion's multiply-adds, Js (Js - 1) (Js + 1) G, and the rate they were done at;
  * the model tables against the float64 recursion of tests/sx2_cases.py in units of its rule (70 items only: the float64
    recursion at 500 items takes minutes on the host).
The times are reported, not asserted.

usage (GPU box):  python tools/sx2_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import sx2_cases as xc                                                # noqa: E402  (the float64 recursion, the rule)
from vipsy_amd.engine import IrtEngine                                           # noqa: E402
from vipsy_amd.grid import grid_image_probs                                      # noqa: E402

SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
KERNELS = ("k_sumscore", "k_reduce")
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm=1, reps=3):
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


def kernel_times(fn):
    """Device microseconds and launches of the kernels of one call of fn, by name prefix, or None without device activity."""
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
            for k in KERNELS:
                if k in ev.key:
                    us, cnt = out.get(k, (0.0, 0))
                    out[k] = (us + float(t), cnt + int(ev.count))
        return out or None
    except Exception as e:  # noqa: BLE001
        say("    (no kernel times: %s)" % e)
        return None


def probe(tag, N, J, seed, check):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.4, 1.0, size=(1, J)).astype(np.float32)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    x = torch.randn(N, 1, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    del x
    eng = IrtEngine(y, model="irt_2pl", D=1, amortized=True, H=64, seed=1)        # (amortized: no per-person rows to allocate)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt)
    be = eng.be
    call = eng._grid_call(None, None)
    G = call.G
    p1, p0 = grid_image_probs(eng._grid_image(call), J, G)
    f32 = dict(dtype=torch.float32, device=dev)
    e1, e0, dist = torch.empty(J, J + 1, **f32), torch.empty(J, J + 1, **f32), torch.empty(G, J + 1, **f32)
    ws_floats = be.sumscore_model_workspace(J, G)
    ws = torch.empty(ws_floats, **f32)
    t_model = timed(lambda: be.sumscore_model(p1, p0, call.logw, J, G, e1, e0, None, ws, ws_floats))
    t_dist = timed(lambda: be.sumscore_model(p1, p0, call.logw, J, G, e1, e0, dist, ws, ws_floats))
    kt = kernel_times(lambda: be.sumscore_model(p1, p0, call.logw, J, G, e1, e0, dist, ws, ws_floats))
    score = torch.empty(N, dtype=torch.int32, device=dev)
    t_persons = timed(lambda: be.sumscore_persons(y, None, N, J, None, J, score))
    sc, order = torch.sort(score, stable=True)
    rows = order.contiguous()
    o1 = torch.empty(J, J + 1, dtype=torch.int32, device=dev)
    t_obs = timed(lambda: be.sumscore_observed(y, rows, N, J, None, J, sc, o1))
    t_score = timed(lambda: eng.score())
    t_tables = timed(lambda: eng.sumscore_tables())
    t_sx2 = timed(lambda: eng.sx2(), reps=1)
    fma = float(J) * (J - 1) * (J + 1) * G
    say("%s: N = %d  Js = %d  G = %d" % (tag, N, J, G))
    say("    score() alone                     %9.3f ms" % t_score)
    say("    vx_sumscore_model, no dist        %9.3f ms   %.2e multiply-adds of the recursion, %.2f T a second; workspace %.1f MB"
        % (t_model, fma, fma / t_model / 1e9, ws_floats * 4 / 1e6))
    say("    vx_sumscore_model with dist       %9.3f ms" % t_dist)
    if kt:
        for k in KERNELS:
            if k in kt:
                say("    %-33s %9.3f ms   in %d launches" % (k + "*", kt[k][0] / 1e3, kt[k][1]))
    say("    vx_sumscore_persons               %9.3f ms   (N Js bytes of y: %.3f ms at 4.9 TB/s)" % (t_persons, N * J / 4.9e12 * 1e3))
    say("    vx_sumscore_observed              %9.3f ms   (persons sorted by score)" % t_obs)
    say("    sumscore_tables() end to end      %9.3f ms   (tables, the three kernels, the sort)" % t_tables)
    say("    sx2() with the host layer         %9.3f ms" % t_sx2)
    ok = True
    if check:
        want = xc.lord_wingersky(p1.cpu().numpy(), p0.cpu().numpy(), call.logw.cpu().numpy())
        r = {k: xc.table_ratio(t.cpu().numpy(), want[k], J, G) for k, t in (("e1", e1), ("e0", e0), ("dist", dist))}
        ok = max(r.values()) <= xc.SX2_C
        say("    against float64, in units of the rule (C = %g): %s   within the rule: %s"
            % (xc.SX2_C, "  ".join("%s %.3f" % kv for kv in r.items()), "yes" if ok else "NO"))
    res = eng.sx2()
    say("    S-X2 under the generating parameters: median p %.3f, %d of %d items below 0.01; %d complete persons, %d cells an item (median)"
        % (np.nanmedian(res["p"]), int((res["p"] < 0.01).sum()), J, res["n_persons"], int(np.median(res["n_cells"]))))
    del eng, y, ws
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("sx2_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    N = max(4096, int(1000000 * SCALE))
    ok = probe("2PL, 500 items, 61 nodes", N, 500, 1, False)
    ok = probe("2PL, 70 items, 61 nodes", N, 70, 2, True) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
