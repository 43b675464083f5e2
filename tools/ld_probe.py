"""local_dependence(): time, memory and accuracy beside score(), at the headline shape and at a sparse one.

Shapes: 1M persons x 500 items x 61 nodes (2PL), 5 % of the cells missing, and the same with 90 % missing.  For each:
  * engine.local_dependence() end to end (tables, posterior kernel, vx_grid_pairs_irt, the copy of the four tables to the host and
    the float64 formulas there), engine.score() alone and vx_grid_pairs_irt alone (on a theta_hat made once): device events around
    back-to-back calls behind warm-up calls;
  * the device time of every kernel inside one vx_grid_pairs_irt call, by torch.profiler, and the workspace;
  * the MFMA share of k_pair_xprod: its 2 nb 12 (tile pairs) 32 32 FLOP (twelve MFMAs a tile pair and k-step, diagonal pairs counted
    as twelve too) against the dense fp16 MFMA peak, and the fragment bytes its waves load a second (from L2, or behind it);
  * 4 096 sampled persons (through `rows`) against the float64 formulas of tests/ld_cases.py at the theta_hat returned, by the
    rule of tests/test_gpu_ld.py.
The times are reported, not asserted.

usage (GPU box):  python tools/ld_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ld_cases as ld                                                 # noqa: E402  (the float64 formulas)
from vipsy_amd.engine import IrtEngine                                           # noqa: E402

PEAK_F16_MFMA = 2.5e15       # FLOP/s, dense fp16 MFMA (spec)
ROW_TOL = 3e-5               # the row rule of tests/test_gpu_ld.py
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
KERNELS = ("k_pair_frag", "k_pair_xprod", "k_reduce", "k_info_add", "k_pair_finish")
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


def probe(tag, N, J, missing, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.4, 1.0, size=(1, J)).astype(np.float32)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    x = torch.randn(N, 1, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < missing] = 255
    del x
    eng = IrtEngine(y, model="irt_2pl", D=1, amortized=True, H=64, seed=1)        # (amortized: no per-person rows to allocate)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt)
    be = eng.be
    t_score = timed(lambda: eng.score())
    t_e2e = timed(lambda: eng.local_dependence())
    call, name, key, run = eng._pairs_call(None, None)
    est = eng._grid_posterior(call)[key]
    f32 = dict(dtype=torch.float32, device=dev)
    ws_floats = be.grid_pairs_workspace(N, J)
    out = {k: torch.empty(J, J, **f32) for k in ("n", "s", "ss", "sp")}
    ws = torch.empty(ws_floats, **f32)
    t_pairs = timed(lambda: run(est, out, ws, ws_floats))
    kt = kernel_times(lambda: run(est, out, ws, ws_floats))
    JT = (J + 31) // 32
    pairs = JT * (JT + 1) // 2
    say("%s: N = %d  J = %d  missing %.0f %%  (%d item tiles, %d tile pairs)" % (tag, N, J, 100 * missing, JT, pairs))
    say("    score() alone                  %9.3f ms" % t_score)
    say("    local_dependence() end to end  %9.3f ms   (workspace %.1f MB, one call's own)" % (t_e2e, ws_floats * 4 / 1e6))
    say("    vx_grid_pairs_irt alone        %9.3f ms" % t_pairs)
    if kt:
        for k in KERNELS:
            if k in kt:
                say("    %-30s %9.3f ms   in %d launches" % (k + "*", kt[k][0] / 1e3, kt[k][1]))
        if "k_pair_xprod" in kt:
            s = kt["k_pair_xprod"][0] * 1e-6
            flop = 2.0 * N * 12 * pairs * 32 * 32
            # a wave holds one tile pair: per k-step it reads the row tile's five fragments and the column tile's five (r^2 of the
            # column tile is not read on a diagonal pair), 1 KB each
            frag_bytes = (N / 16.0) * 1024 * (10 * pairs - 2 * JT)
            say("    k_pair_xprod: %.1f TFLOP/s = %.1f %% of the dense fp16 MFMA peak; its waves load %.2f TB/s of fragments"
                % (flop / s / 1e12, 100 * flop / s / PEAK_F16_MFMA, frag_bytes / s / 1e12))
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    rows = torch.from_numpy(idx).to(dev)
    sub = eng.residual_sums(rows=rows)
    torch.cuda.synchronize()
    cs = {"model": "irt_2pl", "Dc": 1.0, "params": {"a": a, "b": b}}
    ys = y[rows].cpu().numpy()
    want = ld.tables(ys, ld.irt_prob(cs, sub["theta_hat"].cpu().numpy()))
    exact = np.array_equal(sub["n"].cpu().numpy().astype(np.float64), want["n"])
    e = {k: ld.row_error(sub[k].cpu().numpy(), want[k]) for k in ("s", "ss", "sp")}
    say("    %d sampled persons against float64 (row rule %.0e): n exact: %s  s %.2e  ss %.2e  sp %.2e"
        % (len(idx), ROW_TOL, "yes" if exact else "NO", e["s"], e["ss"], e["sp"]))
    res = eng.local_dependence()
    say("    all persons: mean q3 %.5f (-1 / (J - 1) = %.5f), largest q3 - mean %.4f, smallest n_pairs %d, NaN pairs %d"
        % (res["mean"], -1.0 / (J - 1), res["max"], res["n_pairs"].min(), int(np.isnan(res["q3"]).sum())))
    ok = exact and max(e.values()) <= ROW_TOL
    say("    within the row rule: %s" % ("yes" if ok else "NO"))
    del eng, y, ws
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("ld_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n = max(4096, int(1000000 * SCALE))
    ok = probe("2PL, 61 nodes", n, 500, 0.05, 1)
    ok = probe("2PL, 61 nodes, sparse", n, 500, 0.90, 2) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
