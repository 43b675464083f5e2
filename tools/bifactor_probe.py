"""score_bifactor(): time at the shape the benchmark is named after, beside the grid scores that existed before it.

Steps, each a child process of its own under its own time limit (a step that fails, or runs out of time, ends the probe: nothing
more is started on the GPU behind it):
  bifactor   1M persons x 500 items, 100 testlets of 5 items (x_feature = 101, items shuffled), 2PL, nodes = (61, 21):
             score_bifactor() with specific off and on, end to end (tables, the permutation of the responses into the testlet
             layout a slab at a time, the kernels); the MFMA count (persons / 32 x Gg x chunks x 4) and its rate against the
             dense fp16 peak; 4 096 persons through `rows` against the full call, bit for bit;
  score_d2   score() of a two-dimensional 2PL on the same item count with 31 x 31 nodes (31 node tiles x 32 chunks x 4 MFMAs a
             person tile: a comparable MFMA count);
  score_d1   score() of a one-dimensional 2PL at 61 nodes.
The times are reported, not asserted.

usage (GPU box):  python tools/bifactor_probe.py [out.txt]        VX_PROBE_SCALE=0.01 shrinks the person counts (rehearsal)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F16_MFMA = 2.5e15       # op/s, dense fp16 MFMA (spec)
SCALE = float(os.environ.get("VX_PROBE_SCALE", "1"))
STEPS = (("bifactor", 360), ("score_d2", 200), ("score_d1", 200))        # name, time limit in seconds
N = max(4096, int(1000000 * SCALE))
J, S, SIZE = 500, 100, 5


def say(s):
    print(s, flush=True)


def timed(fn, warm=1, reps=3):
    import torch
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


def _data(dev, a, b, seed):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn(N, a.shape[0], device=dev, generator=g)
    y = (torch.rand(N, J, device=dev, generator=g) < torch.sigmoid(x @ a + b)).to(torch.uint8)
    y[torch.rand(N, J, device=dev, generator=g) < 0.05] = 255
    return y


def step_bifactor():
    import numpy as np
    import torch
    from vipsy_amd.engine import IrtEngine
    from vipsy_amd.grid import bifactor_slab_persons
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
    Gg, Gh, KC = 61, 21, S * ((SIZE + 15) // 16)
    slab = bifactor_slab_persons(KC)
    say("bifactor: N = %d  J = %d  %d testlets of %d  x_feature = %d  nodes (%d, %d)  %d chunks  image %.1f MB  slabs of %d persons"
        % (N, J, S, SIZE, 1 + S, Gg, Gh, KC, Gg * KC * 4096 / 1e6, slab))
    t_off = timed(lambda: eng.score_bifactor())
    t_on = timed(lambda: eng.score_bifactor(specific=True))
    mfma = (N + 31) // 32 * Gg * KC * 4.0
    say("    score_bifactor() end to end            %9.3f ms" % t_off)
    say("    score_bifactor(specific=True)          %9.3f ms   (the second kernel recomputes the tiles)" % t_on)
    say("    %.3g MFMAs (32x32x16 f16) a pass, %.0f %% of their rows and %.0f %% of their columns padding (Gh = %d of 32, %d items "
        "of 16): %.1f Top/s = %.1f %% of the dense fp16 peak end to end, specific off"
        % (mfma, 100 * (1 - Gh / 32.0), 100 * (1 - SIZE / 16.0), Gh, SIZE, mfma * 2 * 32 * 32 * 16 / (t_off * 1e-3) / 1e12,
           100 * mfma * 2 * 32 * 32 * 16 / (t_off * 1e-3) / PEAK_F16_MFMA))
    idx = torch.from_numpy(np.sort(rng.choice(N, size=min(4096, N), replace=False))).to(dev)
    full, sub = eng.score_bifactor(specific=True), eng.score_bifactor(rows=idx, specific=True)
    torch.cuda.synchronize()
    same = all(torch.equal(sub[k], full[k][idx]) for k in ("loglik", "eap_general", "psd_general", "node", "eap_specific", "psd_specific"))
    say("    %d persons through rows against the full call: %s" % (idx.numel(), "the same bits" if same else "NOT THE SAME BITS"))
    say("    general EAP against the generating theta: correlation %.3f; mean general PSD %.3f, mean specific PSD %.3f"
        % (0.0 if N < 2 else float(torch.corrcoef(torch.stack([full["eap_general"], _theta0(dev, 1 + S)]))[0, 1]),
           float(full["psd_general"].mean()), float(full["psd_specific"].mean())))
    return 0 if same else 1


def _theta0(dev, D):
    """The general coordinate of the generating draw of _data(seed 1)."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    return torch.randn(N, D, device=dev, generator=g)[:, 0].contiguous()


def step_score(D, nodes):
    import numpy as np
    import torch
    from vipsy_amd.engine import IrtEngine
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(2)
    a = rng.uniform(0.4, 1.0, size=(D, J)).astype(np.float32)
    if D == 2:
        a[1, J - 1:] = 0                                           # the triangular default mask
    b = rng.normal(size=(1, J)).astype(np.float32)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    y = _data(dev, at, bt, 2)
    eng = IrtEngine(y, model="irt_2pl", D=D, amortized=True, H=64, seed=1)
    eng.unconstrained("a").copy_(at)
    eng.unconstrained("b").copy_(bt.reshape(-1))
    t = timed(lambda: eng.score(nodes=nodes))
    G = nodes ** D
    mfma = (N + 31) // 32 * ((G + 31) // 32) * ((J + 15) // 16) * 4.0
    say("score(), x_feature = %d, %d nodes a dimension (%d nodes): N = %d  J = %d    %9.3f ms   (%.3g MFMAs)" % (D, nodes, G, N, J, t, mfma))
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        return {"bifactor": step_bifactor, "score_d2": lambda: step_score(2, 31), "score_d1": lambda: step_score(1, 61)}[sys.argv[2]]()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def keep(new):
        say("\n".join(new))
        lines.extend(new)

    keep(["bifactor_probe: %s, scale %g" % (time.strftime("%Y-%m-%d"), SCALE)])
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
