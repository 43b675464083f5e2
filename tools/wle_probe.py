"""point_estimates(): time, iteration counts and accuracy beside score() and fit_sums(), at the headline shape.

Shapes: 1M persons x 500 items, 2PL and 3PL, and 1M x 70 items 2PL; 61 nodes, 20 % of the cells missing.  Reported a shape:
  * the device time of vx_grid_point_irt alone for the three methods (from the EAP made once): device events around back-to-back
    calls behind a warm-up call, and the time over the floor of reading N J bytes of y once at the 4.9 TB/s an HBM-bound
    reduction reaches here (docs/HARDWARE.md rule 41);
  * the evaluations a person took (`iters`): mean, the share of each count, the status counts -- the time over (mean evaluations
    x the floor) is what one evaluation costs in passes over y, were y read again for each;
  * engine.point_estimates() end to end (tables, posterior kernel, vx_grid_point_irt, copies, the float64 host layer) beside
    engine.score() and engine.fit_sums() on the same data;
  * 4 096 sampled persons (through `rows`) against the float64 formulas of tests/point_cases.py by its rules.
The times are reported, not asserted.

usage (GPU box):  python tools/wle_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person count (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import point_cases as pc                                              # noqa: E402  (the float64 formulas, the rules)
from vipsy_amd.engine import IrtEngine                                           # noqa: E402
from vipsy_amd.grid import POINT_STATUS, tri_to_full                             # noqa: E402

HBM_RATE = 4.9e12            # B/s, an HBM-bound reduction on this chip (docs/HARDWARE.md rule 41)
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
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


def probe(tag, model, N, J, missing, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    p = {"a": rng.uniform(0.4, 1.0, size=(1, J)).astype(np.float32), "b": rng.normal(size=(1, J)).astype(np.float32)}
    if model == "irt_3pl":
        p["c"] = rng.normal(-1.5, 0.3, size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(p["a"]).to(dev), torch.from_numpy(p["b"]).to(dev)
    lo = torch.sigmoid(torch.from_numpy(p["c"]).to(dev)) if "c" in p else 0.0
    x = torch.randn(N, 1, device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < lo + (1.0 - lo) * torch.sigmoid(x @ at + bt)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < missing] = 255
    del x
    eng = IrtEngine(y, model=model, D=1, amortized=True, H=64, seed=1)            # (amortized: no per-person rows to allocate)
    for k, v in p.items():
        eng.unconstrained(k).copy_(torch.from_numpy(v).to(dev))
    t_score = timed(lambda: eng.score())
    t_sums = timed(lambda: eng.fit_sums())
    call = eng._grid_call(None, None)
    eap = eng._grid_posterior(call)["mean"]
    floor = N * J / HBM_RATE * 1e3
    say("%s: N = %d  J = %d  missing %.0f %%   (floor: N J bytes of y once at %.1f TB/s = %.3f ms)"
        % (tag, N, J, 100 * missing, HBM_RATE / 1e12, floor))
    say("    score() alone                          %9.3f ms" % t_score)
    say("    fit_sums() end to end                  %9.3f ms" % t_sums)
    ok = True
    for method in ("ml", "map", "wle"):
        t_k = timed(lambda: eng._point_run(call, eap, method))
        t_e2e = timed(lambda: eng.point_estimates(method=method))
        pt = eng._point_run(call, eap, method)
        torch.cuda.synchronize()
        it = pt["iters"].cpu().numpy()
        st = pt["status"].cpu().numpy()
        mean_it = it[it > 0].mean()
        hist = np.bincount(it, minlength=2)
        shares = "  ".join("%d: %.1f %%" % (k, 100.0 * hist[k] / len(it)) for k in np.flatnonzero(hist) if hist[k] / len(it) >= 0.001)
        say("    vx_grid_point_irt alone, %-3s           %9.3f ms   = %.1f x the floor; %.2f evaluations a person on average, the wave's "
            "slowest sets its count: %.2f x the floor an evaluation" % (method, t_k, t_k / floor, mean_it, t_k / floor / mean_it))
        say("        evaluations (share of the persons)  %s; at most %d" % (shares, it.max()))
        say("        status  %s" % "  ".join("%s %d" % (POINT_STATUS[k], (st == k).sum()) for k in range(5)))
        say("    point_estimates(%s) end to end          %9.3f ms   (score()'s kernels, the kernel, four copies, float64 numpy)"
            % (method, t_e2e))
        idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
        rows = torch.from_numpy(idx).to(dev)
        sub_call = eng._grid_call(None, rows)
        sub = eng._point_run(sub_call, eap[rows].contiguous(), method)
        torch.cuda.synchronize()
        cs = {"model": model, "Dc": 1.0, "D": 1, "J": J, "params": p, "y": y[rows].cpu().numpy()}
        got = {"theta_hat": sub["theta_hat"].cpu().numpy(), "info": tri_to_full(sub["info"].cpu().numpy().T.astype(np.float64), 1),
               "status": sub["status"].cpu().numpy(), "iterations": sub["iters"].cpu().numpy()}
        root = pc.fisher64(cs, method, eap[rows].cpu().numpy().astype(np.float64)) if pc.concave(cs) else None
        r = pc.ratios(cs, method, got, root=root, tag=tag)
        same = all(np.array_equal(got[k], pt[q][rows].cpu().numpy(), equal_nan=True) for k, q in (("theta_hat", "theta_hat"), ("status", "status")))
        say("        %d sampled persons against float64, in units of the rules (C = %g): s %.2f  root %.2f  info %.2f; the bits of the "
            "full call: %s" % (len(idx), pc.POINT_C, r["s"], r["root"], r["info"], "yes" if same else "NO"))
        ok = ok and same and max(r.values()) <= pc.POINT_C
    say("    within the rules: %s" % ("yes" if ok else "NO"))
    del eng, y
    torch.cuda.empty_cache()
    return ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("wle_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    N = max(4096, int(1000000 * SCALE))
    ok = probe("2PL, 500 items", "irt_2pl", N, 500, 0.20, 1)
    ok = probe("3PL, 500 items", "irt_3pl", N, 500, 0.20, 2) and ok
    ok = probe("2PL, 70 items", "irt_2pl", N, 70, 0.20, 3) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
