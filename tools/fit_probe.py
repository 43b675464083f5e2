"""person_fit(): time and accuracy beside score(), at the headline shape.

Shape: 1M persons x 500 items x 61 nodes (2PL), 20 % of the cells missing.  Reported:
  * engine.fit_sums() end to end (tables, posterior kernel, vx_grid_fit_irt), engine.person_fit() with the copies to the host and
    the float64 formulas there, engine.score() alone and vx_grid_fit_irt alone (on a theta_hat made once): device events around
    back-to-back calls behind warm-up calls;
  * the device time of the kernels inside one vx_grid_fit_irt call, by torch.profiler, and the workspace;
  * two yardsticks: score() on the same data, and the floor of reading nb J bytes of y once at the 4.9 TB/s an HBM-bound
    reduction reaches here (docs/HARDWARE.md rule 41);
  * 4 096 sampled persons (through `rows`) against the float64 formulas of tests/fit_cases.py at the theta_hat returned, by the
    rules of tests/test_gpu_fit.py.
The times are reported, not asserted.

usage (GPU box):  python tools/fit_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fit_cases as fc                                                # noqa: E402  (the float64 formulas, the rules)
from vipsy_amd.engine import IrtEngine                                           # noqa: E402

HBM_RATE = 4.9e12            # B/s, an HBM-bound reduction on this chip (docs/HARDWARE.md rule 41)
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
KERNELS = ("k_fit_irt", "k_fit_items")
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
    t_sums = timed(lambda: eng.fit_sums())
    t_e2e = timed(lambda: eng.person_fit())
    call, name, key, run = eng._fit_call(None, None)
    est = eng._grid_posterior(call)[key]
    f32 = dict(dtype=torch.float32, device=dev)
    ws_floats = be.grid_fit_workspace(N, J)
    person, item, ws = torch.empty(7, N, **f32), torch.empty(4, J, **f32), torch.empty(ws_floats, **f32)
    t_fit = timed(lambda: run(est, person, item, ws, ws_floats))
    kt = kernel_times(lambda: run(est, person, item, ws, ws_floats))
    floor = N * J / HBM_RATE * 1e3
    say("%s: N = %d  J = %d  missing %.0f %%" % (tag, N, J, 100 * missing))
    say("    score() alone                     %9.3f ms" % t_score)
    say("    fit_sums() end to end             %9.3f ms   (score()'s kernels + vx_grid_fit_irt; workspace %.1f MB)"
        % (t_sums, ws_floats * 4 / 1e6))
    say("    person_fit() with the host layer  %9.3f ms   (seven copies of N floats, float64 numpy)" % t_e2e)
    say("    vx_grid_fit_irt alone             %9.3f ms   = %.1f x the floor of reading N J bytes of y once at %.1f TB/s (%.3f ms)"
        % (t_fit, t_fit / floor, HBM_RATE / 1e12, floor))
    if kt:
        for k in KERNELS:
            if k in kt:
                say("    %-33s %9.3f ms   in %d launches" % (k + "*", kt[k][0] / 1e3, kt[k][1]))
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    rows = torch.from_numpy(idx).to(dev)
    sub = eng.fit_sums(rows=rows)
    torch.cuda.synchronize()
    cs = {"model": "irt_2pl", "Dc": 1.0, "params": {"a": a, "b": b}}
    ys = y[rows].cpu().numpy()
    want = fc.sums(ys, fc.prob_at("irt", cs, sub["theta_hat"].cpu().numpy().astype(np.float64)))
    gp = {k: v.cpu().numpy().astype(np.float64) for k, v in sub["person"].items()}
    gi = {k: v.cpu().numpy().astype(np.float64) for k, v in sub["item"].items()}
    exact = np.array_equal(gp["n"], want["person"]["n"]) and np.array_equal(gi["n"], want["item"]["n"])
    rp = fc.sum_ratios(gp, want["person"], want["person_abs"], fc.PERSON)
    ri = fc.sum_ratios(gi, want["item"], want["item_abs"], fc.ITEM)
    rl = fc.lz_ratio(fc.stats(gp)["lz"], want)
    say("    %d sampled persons against float64, in units of the rules (C = %g): n exact: %s  person sums %.2f  item sums %.2f  lz %.2f"
        % (len(idx), fc.FIT_C, "yes" if exact else "NO", max(rp.values()), max(ri.values()), rl))
    res = eng.person_fit()
    lz = res["lz"][np.isfinite(res["lz"])]
    say("    all persons: mean lz %.3f, sd %.3f, %.2f %% below -1.645; mean outfit %.3f, mean infit %.3f; persons without answers %d"
        % (lz.mean(), lz.std(), 100 * (lz < -1.645).mean(), np.nanmean(res["outfit"]), np.nanmean(res["infit"]),
           int((res["n_obs"] == 0).sum())))
    ok = exact and max(max(rp.values()), max(ri.values()), rl) <= fc.FIT_C
    say("    within the rules: %s" % ("yes" if ok else "NO"))
    del eng, y, ws, person
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("fit_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    ok = probe("2PL, 61 nodes", max(4096, int(1000000 * SCALE)), 500, 0.20, 1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
