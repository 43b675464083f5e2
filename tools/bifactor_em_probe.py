"""fit_em_bifactor(): time of the expected-count kernel and of one EM iteration at the documented bifactor workload, beside the
scores that existed before it.

Steps, each a child process of its own under its own time limit (a step that fails, or runs out of time, ends the probe: nothing
more is started on the GPU behind it):
  counts   1M persons x 500 items, 100 testlets of 5 items (x_feature = 101, items shuffled), 2PL, nodes = (41, 21):
           vx_grid_bifactor_counts alone on the first slab of persons (F and loglik made once, in front), then
           expected_counts_bifactor() end to end (tables, the permutation of the responses a slab at a time, vx_grid_bifactor with
           fws, the counts); the MFMA counts of its two products; 4 096 persons through `rows` against new data, bit for bit;
  em       one iteration of fit_em_bifactor(max_iter=1) end to end on the same data;
  score    score_bifactor() and score_bifactor(specific=True) of THIS commit on the same data and nodes: the E-step without its
           tables.  (The method's kernels and bits are the parent commit's; its host path now goes through IrtEngine._bifactor_call.
           For the parent's own time run tools/bifactor_probe.py there.)
Device events around three calls behind a warm-up.  The times are reported, not asserted.

usage (GPU box):  python tools/bifactor_em_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bifactor_probe import J, N, S, SCALE, SIZE, _data, say, timed      # noqa: E402  (the workload and the clock of bifactor_probe.py)

STEPS = (("counts", 420), ("em", 300), ("score", 240))                  # name, time limit in seconds
NODES = (41, 21)


def _engine():
    import numpy as np
    import torch
    from vipsy_amd.engine import IrtEngine
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    testlet = np.repeat(np.arange(S), SIZE)[rng.permutation(J)]
    mask = np.zeros((1 + S, J), np.float32)
    mask[0] = 1
    mask[1 + testlet, np.arange(J)] = 1
    a = (rng.uniform(0.4, 1.0, size=mask.shape) * mask).astype(np.float32)
    a[0] = rng.uniform(0.6, 1.4, size=J)
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    y = _data(dev, at, bt, 1)
    eng = IrtEngine(y, model="irt_2pl", D=1 + S, amortized=True, H=64, a_free=torch.from_numpy(mask), a0=torch.from_numpy(a), seed=1)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt.reshape(-1))
    return eng, rng


def step_counts():
    import numpy as np
    import torch
    eng, rng = _engine()
    dev = eng.dev
    Gg, Gh = NODES
    bf = eng._bifactor_call(None, None, NODES, (6.0, 4.0), 0)
    bf.fill()
    buf = eng._bifactor_buffers(bf)
    n_tl = len(bf.plan["tl_column"])
    s0, s1, yp = next(bf.slabs())
    nb = s1 - s0
    say("counts: N = %d  J = %d  %d testlets of %d  x_feature = %d  nodes (%d, %d)  %d chunks  image %.1f MB  first slab %d persons, "
        "count workspace %.1f MB" % (N, J, S, SIZE, 1 + S, Gg, Gh, bf.KC, Gg * bf.KC * 4096 / 1e6, nb,
                                    eng.be.grid_bifactor_counts_workspace(nb, bf.KC, Gg, n_tl) * 4 / 1e6))
    fws = buf["fws"][:eng.be.grid_bifactor_workspace(nb, Gg)]
    ll = buf["loglik"][s0:s1]
    post = lambda: eng.be.grid_bifactor(yp, nb, bf.KC, bf.plan["tl_start"], bf.tl_dev, bf.img, bf.logw, bf.theta, bf.logv, bf.u, ll,      # noqa: E731
                                        buf["mean"][s0:s1], buf["sd"][s0:s1], buf["node"][s0:s1], fws)
    ws = buf["ws"][:eng.be.grid_bifactor_counts_workspace(nb, bf.KC, Gg, n_tl)]
    cnt = lambda: eng.be.grid_bifactor_counts(yp, nb, bf.KC, Gg, bf.plan["tl_start"], bf.tl_dev, bf.col, bf.J, bf.img, bf.logv, ll, fws,   # noqa: E731
                                              False, buf["n1"], buf["n0"], buf["mass"], buf["mass_s"], ws)
    t_post = timed(post)
    t_cnt = timed(cnt)
    t_all = timed(lambda: eng.expected_counts_bifactor(nodes=NODES))
    m1 = (nb + 31) // 32 * Gg * bf.KC * 4.0
    m2 = (nb + 15) // 16 * Gg * bf.KC * 2.0
    say("    vx_grid_bifactor with fws, first slab          %9.3f ms" % t_post)
    say("    vx_grid_bifactor_counts, first slab            %9.3f ms   (%.3g MFMAs of product 1, %.3g of product 2)" % (t_cnt, m1, m2))
    say("    expected_counts_bifactor() end to end, N = %d  %9.3f ms" % (N, t_all))
    idx = torch.from_numpy(np.sort(rng.choice(N, size=min(4096, N), replace=False))).to(dev)
    sub, new = eng.expected_counts_bifactor(rows=idx, nodes=NODES), eng.expected_counts_bifactor(eng.y[idx][:, :J].contiguous(), nodes=NODES)
    full = eng.expected_counts_bifactor(nodes=NODES)
    torch.cuda.synchronize()
    same = all(torch.equal(sub[k], new[k]) for k in ("n1", "n0", "mass", "mass_specific", "loglik"))
    say("    %d persons through rows against the same persons as new data: %s" % (idx.numel(), "the same bits" if same else "NOT THE SAME BITS"))
    say("    sum of mass %.3f of N = %d; sum of n1 + n0 %.1f of %d answers"
        % (float(full["mass"].double().sum()), N, float((full["n1"].double() + full["n0"].double()).sum()), int((eng.y[:, :J] != 255).sum())))
    return 0 if same else 1


def step_em():
    eng, _ = _engine()
    before = eng.score_bifactor(nodes=NODES)["loglik"].double().sum().item()
    t = timed(lambda: eng.fit_em_bifactor(max_iter=1, nodes=NODES))
    after = eng.score_bifactor(nodes=NODES)["loglik"].double().sum().item()
    say("em: one iteration of fit_em_bifactor(max_iter=1), N = %d, nodes %s   %9.3f ms   (loglik %.1f -> %.1f after the four timed and "
        "warm-up iterations)" % (N, NODES, t, before, after))
    return 0


def step_score():
    eng, _ = _engine()
    t_off = timed(lambda: eng.score_bifactor(nodes=NODES))
    t_on = timed(lambda: eng.score_bifactor(nodes=NODES, specific=True))
    say("score: score_bifactor(nodes=%s), N = %d   %9.3f ms;  specific=True   %9.3f ms" % (NODES, N, t_off, t_on))
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        return {"counts": step_counts, "em": step_em, "score": step_score}[sys.argv[2]]()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def keep(new):
        say("\n".join(new))
        lines.extend(new)

    keep(["bifactor_em_probe: %s, scale %g" % (time.strftime("%Y-%m-%d"), SCALE)])
    rc = 0
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            keep(["%s: no result within %d s; the probe stops here" % (name, limit)])
            rc = 1
            break
        keep(r.stdout.rstrip().split("\n"))
        if r.returncode != 0:
            keep(["%s: exit status %d; the probe stops here" % (name, r.returncode)] + r.stderr.rstrip().split("\n")[-15:])
            rc = 1
            break
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
