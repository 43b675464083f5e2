"""vx_grid_mstep_irt_map on the GPU where tests/test_gpu_map.py does not take it: the step control of the penalised kernel from far
starts, and the sentences of the kernel's header (vipsy_amd/csrc/k_grid_mstep.hip) that are exact promises.

  A. Far starts (tests/map_cases.py: FAR -- p0 + free U(-amp, amp), amp 1.5, 3 and 5, on the 3PL, 1PL, 4PL D = 2, 2PL D = 3 and
     4PL D = 3 cases, and three launches under priors 64 and 256 times as precise, where the penalty decides trials).
       One step (newton = 1): rule 3 of tests/map_cases.py -- the output is the float64 step t delta, capped and halved as the
       float64 method caps and halves it, unknown by unknown to C_STEP eps32 (t (|H^-1| S)_k + [capped] |t delta_k| (|H^-1| S)_m /
       |delta_m| + |p_k|) -- on every item-start whose float64 decisions are all clear by 100 tolerances.  tests/test_map_host.py
       holds the float32 restatement to half of it and shows that a halving factor of 0.25, a cap of 2, a cap that clips each
       component and acceptance on the unpenalised Q_j each break it.
       To the end (newton = 64): rule 1 as it stands, the float64 maximiser started at the kernel's output.
  B. The header's promises, bit for bit: prior rows the call must not read may hold NaN; with precision 0 the mean is irrelevant;
     a_free = NULL is an all-ones mask; n1, n0 and the precisions times 4 give the same parameters and 4 times the log prior; an
     item whose every node is clamped and whose prior is on b alone stops on its zero pivot with all its bits while its
     neighbours move; a steep start (nodes that are not `inside`) and a falling curve (d < c) end finite, at the maximum.
  C. A and B again in a child process on the library built under the other instruction schedule.
Largest ratios on an MI355X are printed by the tests and recorded in DESIGN.md section 6."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import map_cases as mc
from tests.test_gpu_map import _full, _launch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")
FAR_IDS = [mc.far_id(f) for f in mc.FAR]
FAR_END = [f for f in mc.FAR if f not in mc.FAR_NOT_TO_THE_END]
D3, D2, PL1 = "map9_2pl_d3_j7_g343", "map8_4pl_d2_j6_g225", "map7_1pl_j7_g61"


# ---- A. far starts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("far", mc.FAR, ids=FAR_IDS)
def test_far_one_step(far):
    cs, L = mc.case(far[0]), mc.far_launch(far)
    p, _ = _launch(cs, L, L["p0"], 1)
    ratio = mc.rule3(far, p)
    _, tr = mc.far_step(far)
    paths = sorted({n for j in ratio for n in mc.path_of(tr[j][0])})
    print("%s: one far step at most %.3g of rule 3's scale (C_STEP = %g) over %d item-starts; paths %s"
          % (mc.far_id(far), max(ratio.values()), mc.C_STEP, len(ratio), paths))
    assert np.isfinite(p).all() and len(ratio) >= 4
    assert max(ratio.values()) <= mc.C_STEP, (far, ratio)
    assert p[~L["free"]].tobytes() == L["p0"][~L["free"]].tobytes()
    assert p[:, mc.UNANSWERED].tobytes() == L["p0"][:, mc.UNANSWERED].tobytes()


@pytest.mark.parametrize("far", FAR_END, ids=[mc.far_id(f) for f in FAR_END])
def test_far_to_the_end(far):
    cs, L = mc.case(far[0]), mc.far_launch(far)
    p, _ = _launch(cs, L, L["p0"], 64)
    assert np.isfinite(p).all()
    gain, dev, last = mc.rule1(cs, L, p)
    print("%s: from the far start the oracle gains at most %.3g of 1e-6 |Q_j| (C_Q = %g); parameters at most %.3g of their bound"
          % (mc.far_id(far), gain.max(), mc.C_Q, dev.max()))
    assert last <= 1e-6
    assert gain.max() <= mc.C_Q, (far, gain)
    assert dev.max() <= 1.0, (far, dev)
    assert p[~L["free"]].tobytes() == L["p0"][~L["free"]].tobytes()


# ---- B. the header's promises ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [D3, D2, PL1])
def test_promise_unread_prior_rows_may_hold_nan(name):
    """"Rows the model or D does not have are not read", a fixed loading's "prior row is not read": NaN in the means and the
    precisions of the masked loadings, of the a rows at or beyond D (all three for 1PL) and of the c / d rows the model lacks --
    the same parameter bits and the same lprior as without."""
    cs, L = mc.case(name), mc.launch(name)
    p, lp = _full(name)
    pr = mc.unread_nan(cs, L)
    assert np.isnan(pr).sum() >= 2 * (7 if name == D2 else 17)
    q, lq = _launch(cs, L, L["p0"], 64, prior=pr, lprior=True)
    assert q.tobytes() == p.tobytes() and lq.tobytes() == lp.tobytes()
    assert np.isfinite(q).all() and np.isfinite(lq).all()


@pytest.mark.parametrize("name", [D3, D2])
def test_promise_precision_zero_makes_the_mean_irrelevant(name):
    """"Precision 0: no prior on that unknown (the mean must still be finite)": the precisions of b (all but the constant item's
    are 0 already) and of two free loadings an item set to 0; a mean of 1e6 there gives the bits of a mean of 0."""
    cs, L = mc.case(name), mc.launch(name)
    pr0 = L["prior"].copy()
    pr0[1, 1, :-1:2] = 0                                                # (not the constant item's: its a has no maximum without)
    pr0[1, 2, 1:-1:2] = 0
    off = (pr0[1] == 0) & L["free"]
    assert off[0, :-1].all() and off[1].any() and off[2].any() and not off[1].all() and not off.all()
    pr0[0][off] = 0
    pr1 = pr0.copy()
    pr1[0][off] = 1e6
    p0, l0 = _launch(cs, L, L["p0"], 64, prior=pr0, lprior=True)
    p1, l1 = _launch(cs, L, L["p0"], 64, prior=pr1, lprior=True)
    assert p0.tobytes() == p1.tobytes() and l0.tobytes() == l1.tobytes() and np.isfinite(p0).all()
    assert p0.tobytes() != _full(name)[0].tobytes()                     # (the priors taken away did weigh)


@pytest.mark.parametrize("name", [D3, D2])
def test_promise_a_free_null_is_an_all_ones_mask(name):
    cs, L = mc.case(name), mc.launch(name)
    ones = np.ones_like(cs["a_free"])
    p0 = L["p0"].copy()
    p0[1:1 + cs["D"]][~cs["a_free"]] = 0.8                              # (the loadings the case masks: free now, and not at 0)
    a, la = _launch(cs, L, p0, 64, lprior=True, a_free=None)
    b, lb = _launch(cs, L, p0, 64, lprior=True, a_free=ones)
    assert a.tobytes() == b.tobytes() and la.tobytes() == lb.tobytes() and np.isfinite(a).all()
    assert (a[1:1 + cs["D"]][~cs["a_free"]] != np.float32(0.8)).all()


@pytest.mark.parametrize("name", [D3, D2, PL1])
@pytest.mark.parametrize("newton", [1, 64])
def test_promise_scaling_by_four(name, newton):
    """n1, n0 and every precision times 4 give the same parameter bits, and lprior exactly 4 times the original.  Every number the
    kernel forms from them -- the cell weights c1 Q - c0 P and c1 + c0, the lane sums and the wave sums of Q_j, of the gradient and
    of the curvature, the penalty and its derivatives -- is a sum of products with exactly one factor that carries the 4, so each
    is exactly 4 times what it was (a power of two commutes with every rounding, fused or not, and nothing is near the ends of
    the exponent range); the Cholesky factor is exactly twice (sqrt(4 v) = 2 sqrt(v)), the forward solve gives 2 y, the backward
    solve the same delta; and both sides of the acceptance test, tr.q >= cur.q - 1e-6 |cur.q|, are 4 times theirs.  The float32
    restatement holds the same in tests/test_map_host.py."""
    cs, L = mc.case(name), mc.launch(name)
    L4 = mc.scaled4(L)
    p, lp = _full(name) if newton == 64 else _launch(cs, L, L["p0"], newton, lprior=True)
    p4, lp4 = _launch(cs, L4, L4["p0"], newton, lprior=True)
    assert p4.tobytes() == p.tobytes()
    assert (lp4 == np.float32(4) * lp).all() and lp[-1] < 0


def test_promise_pivot_stop_keeps_every_bit():
    """"On a pivot that is not positive the item stops where it is": the 2PL item of tests/map_cases.py's pivot_launch (every node
    clamped, a prior on b alone: the matrix is diag(prec_b, 0, 0, 0)) keeps ALL its bits, b included, whose own pivot is
    positive; the other three waves of its workgroup, and every other answered item, move; and its lprior is reported."""
    cs, L = mc.case(mc.PIVOT_CASE), mc.pivot_launch()
    j = mc.PIVOT_ITEM
    for newton in (1, 64):
        p, lp = _launch(cs, L, L["p0"], newton, lprior=True)
        assert p[:, j].tobytes() == L["p0"][:, j].tobytes(), (newton, p[:, j], L["p0"][:, j])
        others = [k for k in np.flatnonzero(mc.answered(L)) if k != j]
        assert 2 in others and 3 in others                              # (items 1 .. 3 share its workgroup; 1 is the unanswered one)
        assert (p[:, others][L["free"][:, others]] != L["p0"][:, others][L["free"][:, others]]).all()
        assert lp[j] == np.float32(-0.5 * 0.25 * 20.0 ** 2)
    gain, dev, last = mc.rule1(dict(cs, J=cs["J"] - 1, a_free=cs["a_free"][:, 1:]),
                               {k: (v[1:] if k in ("n1", "n0") else v[..., 1:]) for k, v in L.items()}, p[:, 1:])
    print("pivot launch, the items that are not stopped: gain at most %.3g, parameters at most %.3g" % (gain.max(), dev.max()))
    assert last <= 1e-6 and gain.max() <= mc.C_Q and dev.max() <= 1.0


@pytest.mark.parametrize("which", ["steep_3pl", "falling_4pl"])
def test_promise_steep_and_falling_starts_end_at_the_maximum(which):
    """"A node that is not `inside` adds its clamped log term to Q_j and nothing to the gradient or the curvature" (every loading
    of the 3PL case at 4.5 on span 6: Q < eps32 at the upper nodes) and "with d < c the curve falls ... and nothing here breaks"
    (a 4PL item started at c_un = 0.5, d_un = -0.5): the output is finite, rule 1 holds at the end, lprior is the log prior of
    the start."""
    cs, L = (mc.case(mc.STEEP_CASE), mc.steep_launch()) if which == "steep_3pl" else (mc.case(mc.FALLING_CASE), mc.falling_launch())
    p, lp = _launch(cs, L, L["p0"], 64, lprior=True)
    assert np.isfinite(p).all() and np.isfinite(lp).all()
    gain, dev, last = mc.rule1(cs, L, p)
    print("%s: the oracle gains at most %.3g of 1e-6 |Q_j| (C_Q = %g); parameters at most %.3g of their bound"
          % (which, gain.max(), mc.C_Q, dev.max()))
    assert last <= 1e-6 and gain.max() <= mc.C_Q and dev.max() <= 1.0
    want = mc.log_prior(L["p0"].astype(np.float64), L["free"], L["prior"].astype(np.float64))
    assert (np.abs(lp.astype(np.float64) - want) <= 8 * mc.EPS32 * np.abs(want) + 1e-30).all(), (lp, want)
    if which == "falling_4pl":
        j = mc.FALLING_ITEM
        assert want[j] < -0.5 * (1.9 ** 2 + 2.7 ** 2) + 0.01 and p[5, j] > p[4, j]      # (the prior and the data turn the curve round)


# ---- C. the other instruction schedule ---------------------------------------------------------------------------------------------
def test_paths_and_promises_under_a_second_schedule():
    """Every other test of this file, and the rules of tests/test_gpu_map.py on the four cases at D > 1, 1PL and Dc = 1, again in
    a fresh child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    here = os.path.abspath(__file__)
    cmd = [sys.executable, "-m", "pytest", here, os.path.join(ROOT, "tests", "test_gpu_map.py"), "-x", "-q", "-s", "-m", "gpu", "-k",
           "(far or promise or ((maximum_reached or one_step or bits or lprior) and (map7 or map8 or map9 or map10))) and not second",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    print("\n".join(line for line in r.stdout.splitlines() if "C_STEP = " in line or "C_Q = " in line))
    n = len(mc.FAR) + len(FAR_END) + 3 + 2 + 2 + 6 + 1 + 2 + 4 * 4
    assert "%d passed" % n in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
