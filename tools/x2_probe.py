"""ld_x2(): time, traffic and exactness beside local_dependence()'s pair kernel, at the headline shape, a sparse one and a short test.

Shapes: 1M persons x 500 items x 61 nodes (2PL) with 5 % and with 90 % of the cells missing, and 1M x 70 with 5 %.  For each:
  * vx_pair_tables alone, engine.ld_x2() end to end (tables of the model, the operand image read back, vx_pair_tables, the copy of
    the four tables to the host and the float64 formulas there) and vx_grid_pairs_irt alone on the same data (on a theta_hat made
    once): device events around back-to-back calls behind warm-up calls;
  * the int8 MFMA rate of k_pair_tables: 4 MFMAs of 2 x 32 x 32 x 32 operations a tile pair and k-step, 16 tile pairs a pair of
    item groups (the diagonal pairs of groups compute both triangles), over the staged persons, against the dense int8 peak, and
    the bytes of y its workgroups read (every pair of item groups reads its one or two panels of every person);
  * 4 096 sampled persons (through `rows`) against the int64 numpy products: bit for bit;
  * the mean of x2 over the pairs at the generating item parameters and after fit_em(): about 3 and about 1 -- chi-square(1)
    is the reference after estimation.
The times are reported, not asserted.

usage (GPU box):  python tools/x2_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipsy_amd.engine import IrtEngine                                           # noqa: E402

PEAK_I8_MFMA = 5.0e15        # op/s, dense int8 MFMA (spec: twice the bf16 rate)
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
EM_ITERS = int(os.environ.get("VX_PROBE_EM_ITERS", "100"))
TABLES = ("n11", "n10", "n01", "n00")
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


def probe(tag, N, J, missing, seed, refit):
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
    Jm = eng.J_items
    yy = eng.y if eng.y.shape[1] == Jm else eng.y[:, :Jm].contiguous()
    out = {k: torch.empty(Jm, Jm, dtype=torch.int32, device=dev) for k in TABLES}
    t_tab = timed(lambda: be.pair_tables(yy, None, N, Jm, out["n11"], out["n10"], out["n01"], out["n00"], None, 0), warm=2, reps=5)
    t_e2e = timed(lambda: eng.ld_x2())
    call, name, key, run = eng._pairs_call(None, None)
    est = eng._grid_posterior(call)[key]
    f32 = dict(dtype=torch.float32, device=dev)
    ws_floats = be.grid_pairs_workspace(N, Jm)
    q = {k: torch.empty(Jm, Jm, **f32) for k in ("n", "s", "ss", "sp")}
    ws = torch.empty(ws_floats, **f32)
    t_pairs = timed(lambda: run(est, q, ws, ws_floats))
    del ws
    groups = (Jm + 127) // 128
    n_bp = groups * (groups + 1) // 2
    stages = (N + 127) // 128
    chunks = be.pair_tables_chunks(N, Jm)
    ops = stages * 4.0 * n_bp * 64 * 2 * 32 * 32 * 32
    width = [min(128, Jm - 128 * gi) for gi in range(groups)]
    y_bytes = float(N) * sum(width[ga] + (width[gb] if gb != ga else 0) for ga in range(groups) for gb in range(ga, groups))
    say("%s: N = %d  J = %d  missing %.0f %%  (%d item groups, %d group pairs, %d person chunks: %d workgroups)"
        % (tag, N, Jm, 100 * missing, groups, n_bp, chunks, n_bp * chunks))
    say("    vx_pair_tables alone           %9.3f ms   (no workspace)" % t_tab)
    say("    ld_x2() end to end             %9.3f ms" % t_e2e)
    say("    vx_grid_pairs_irt alone        %9.3f ms   (workspace %.1f MB) on the same data" % (t_pairs, ws_floats * 4 / 1e6))
    say("    k_pair_tables: %.1f Top/s = %.1f %% of the dense int8 MFMA peak; its workgroups read %.2f GB of y (%.2f x y) at %.2f TB/s"
        % (ops / (t_tab * 1e-3) / 1e12, 100 * ops / (t_tab * 1e-3) / PEAK_I8_MFMA, y_bytes / 1e9, y_bytes / (float(N) * Jm),
           y_bytes / (t_tab * 1e-3) / 1e12))
    idx = np.sort(rng.choice(N, size=min(4096, N), replace=False))
    sub = eng.pair_tables(rows=torch.from_numpy(idx).to(dev))
    torch.cuda.synchronize()
    ys = yy[torch.from_numpy(idx).to(dev)].cpu().numpy()
    u, z = (ys == 1).astype(np.int64), (ys == 0).astype(np.int64)
    want = {"n11": u.T @ u, "n10": u.T @ z, "n01": z.T @ u, "n00": z.T @ z}
    exact = all(np.array_equal(sub[k].cpu().numpy().astype(np.int64), want[k]) for k in TABLES)
    full = eng.pair_tables()
    ones = (yy == 1).sum(0).to(torch.int32)
    exact = exact and torch.equal(full["n11"].diagonal(), ones) and torch.equal(full["n10"], full["n01"].t())
    say("    %d sampled persons against int64 numpy, all persons' diagonal and transposes: %s" % (len(idx), "exact" if exact else "NOT EXACT"))
    res = eng.ld_x2()
    off = np.triu(np.ones((Jm, Jm), bool), 1)
    say("    x2 at the generating parameters: mean %.3f over %d pairs (a fully specified table: up to 3 df), largest %.1f, "
        "smallest n_pairs %d" % (np.nanmean(res["x2"][off]), int(np.isfinite(res["x2"][off]).sum()), np.nanmax(res["x2"][off]),
                                res["n_pairs"].min()))
    if refit:
        em = eng.fit_em(max_iter=EM_ITERS)
        res = eng.ld_x2()
        say("    x2 after fit_em() (%d iterations from the generating values): mean %.3f (chi-square(1): 1), share with p < 0.05: %.3f"
            % (int(em.get("iterations", EM_ITERS)), np.nanmean(res["x2"][off]),
               float(np.nanmean((res["p"][off] < 0.05).astype(np.float64)))))
    del eng, y, yy
    torch.cuda.empty_cache()
    return exact


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("x2_probe: %s, torch %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d")))
    n = max(4096, int(1000000 * SCALE))
    ok = probe("2PL, 61 nodes", n, 500, 0.05, 1, True)
    ok = probe("2PL, 61 nodes, sparse", n, 500, 0.90, 2, False) and ok
    ok = probe("2PL, 61 nodes, short test", n, 70, 0.05, 3, True) and ok
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
