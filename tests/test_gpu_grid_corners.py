"""The grid family on the GPU at its shape limits and on long dense tests (score(), expected_counts() / item_fit(),
plausible_values() and item_information() of IrtEngine and CcdmEngine) against the float64 oracle of tests/corner_cases.py.

Engines are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views, nothing trained.  One
test a case builds one engine and runs the four calls in turn.  Rules (tests/corner_cases.py; tests/test_grid_corners_host.py
checks their conditions on the CPU): every table and moment by the row rule with tol = max(ROW_TOL, 3 e_restated), never above
four float32 spacings of the case's largest |loglik| -- e_restated is the error of the numpy restatement of the operand phase
against the oracle, computed here on the CPU, never from what the GPU returned; nodes and draws equal to the oracle's wherever
its best two values differ by more than max(ARGMAX_GAP, 4 d_f); the count identities, the symmetry of info, its dead
parameters and the bits of a second call as they are everywhere.  The errors found are printed beside tol.

Shapes: J = 1, 16, 17 and 1 024 (KC 64; NIT 32 = 4 GC_WAVES in k_grid_counts<4, 1>), G = 1 (explicit), 2, 4, 32, 33, 512 (NT 16: the
largest one-phase k_grid_pscores), 529 (NT 17: the first two-phase launch), 1 000 and 1 024, K = 1, 2, 5 .. 10 (k_grid_post<1>
.. <10> with padded coordinate columns at 5, 7, 9), P = 2 .. 4 096 (PT 129, nbb 33, 561 workgroup blocks, one chunk), and
vx_grid_info between its smallest and its preferred workspace (several slabs of several chunks, the last slab's last chunks empty).

Measured on an MI355X (docs/NOTEBOOK.md has the table per case and output: GPU error, e_restated, tol).  No kernel failed at a
shape corner.  Up to 60 answered items every output sits at 1e-9 .. 5e-6 (restatement alike) and tol is ROW_TOL.  At 946 .. 1 024
answered items the IRT cases give EAP 3.2e-5 .. 2.3e-4 (e_restated 2.4e-5 .. 1.2e-4, tol 7.2e-5 .. 3.0e-4), PSD 2.1e-5 .. 9.1e-5,
n1 / n0 1.0e-4 .. 2.4e-4 (e_restated 7e-5 .. 1.3e-4, tol 2.0e-4 .. 3.1e-4), mass 2.6e-5 .. 6.7e-5, info 1.8e-5 .. 4.5e-5 (tol 4.8e-5 ..
8.9e-5), loglik 2 .. 5e-7; the DINA / DINO cases at J = 1 024 stay below 1e-5 everywhere.  Where 3 e_restated passes the cap (n1 / n0
of long_j1024_d1: 3.9e-4 and 3.5e-4 against 3.1e-4; n1 of long_j1024_4pl; EAP of long_j1024_g512_d3: 3.7e-4 against 3.0e-4) the
cap is the tolerance, and the GPU is below it (2.3e-4, 1.2e-4, 2.3e-4).  d_f 3.6e-4 .. 4.2e-4 on the long IRT cases (gap 1.4e-3 ..
1.7e-3): no wrong node, no wrong draw of 37 248; at most 1.6 % of the persons and 0.25 % of the draws left out.  The count
identities: 2.1 .. 2.4e-5 on the long IRT cases (loglik_i is a float32 at 650), 1e-7 .. 5e-7 elsewhere.  The in-between workspace of
vx_grid_info: 1.5e-7 of the one-slab matrix.  The file: 11 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import corner_cases as co
from tests import score_cases as sc
from tests import se_cases as se
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np
from tests.test_gpu_se import _case, _engine, _info_errors, _raw_info

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _finite(tag, out, keys):
    for k in keys:
        assert bool(torch.isfinite(out[k]).all()), (tag, k)


def _report(tag, what, errs, tols):
    print("%s %s: %s" % (tag, what, "  ".join("%s %.2e (tol %.1e)" % (k, errs[k], tols[k]) for k in errs)))
    for k in errs:
        assert errs[k] <= tols[k], (tag, what, k, errs[k], tols[k])


def _hold_score(tag, got, o):
    """The row rule on loglik and the moments, the node rule on the node."""
    N, D = o["f"].shape[0], o["coord"].shape[1]
    mean_k, node_k = ("eap", "node") if o["kind"] == "irt" else ("attr_prob", "pattern")
    assert tuple(got[mean_k].shape) == (N, D) and tuple(got["loglik"].shape) == (N,) and tuple(got[node_k].shape) == (N,)
    assert got[mean_k].dtype == torch.float32 and got["loglik"].dtype == torch.float32 and got[node_k].dtype == torch.int32
    names = [("loglik", "loglik"), (mean_k, "mean")] + ([("psd", "sd")] if o["kind"] == "irt" else [])
    if o["kind"] == "irt":
        assert tuple(got["psd"].shape) == (N, D) and got["psd"].dtype == torch.float32
    _finite(tag, got, [g for g, _ in names])
    want = o["post"]
    errs = {g: _row_errors(_f8(got[g]), np.asarray(want[w], np.float64), floor=1.0)[0] for g, w in names}
    _report(tag, "score", errs, {g: o["tol"][w] for g, w in names})
    node = _np(got[node_k]).astype(np.int64)
    assert node.min() >= 0 and node.max() < o["f"].shape[1]
    sure = want["gap"] > o["gap_thr"]
    wrong = np.flatnonzero(sure & (node != want["node"]))
    print("%s score: %.1f %% of the persons left out below the gap %.2e, %d wrong nodes" % (tag, 100 * (1 - sure.mean()), o["gap_thr"], len(wrong)))
    assert 1 - sure.mean() <= sc.ARGMAX_LEFT_OUT, tag
    assert len(wrong) == 0, (tag, wrong[:10], node[wrong[:10]], want["node"][wrong[:10]], want["gap"][wrong[:10]])


def _hold_counts(tag, got, fit, o):
    """The row rule on the tables, the absolute rule on the proportions, the count identities of test_gpu_counts._hold."""
    want, y = o["counts"], o["cs"]["y"]
    J, G = want["n1"].shape
    for k in ("n1", "n0", "prob"):
        assert tuple(got[k].shape) == (J, G) and got[k].dtype == torch.float32, (tag, k)
    assert tuple(got["mass"].shape) == (G,) and got["mass"].dtype == torch.float32
    assert set(fit) == {"n_obs", "md", "rmsd", "observed", "prob"} and fit["md"].dtype == torch.float64
    _finite(tag, got, ("n1", "n0", "mass", "prob"))
    errs, tols = {}, {}
    for k in ("n1", "n0"):
        errs[k], tols[k] = _row_errors(_f8(got[k]), want[k], floor=1.0)[0], o["tol"][k]
    errs["mass"], tols["mass"] = _row_errors(_f8(got["mass"])[None, :], want["mass"][None, :], floor=1.0)[0], o["tol"]["mass"]
    errs["prob"], tols["prob"] = float(np.abs(_f8(got["prob"]) - want["prob"]).max()), ROW_TOL       # (out of the table, not of f)
    for k in ("md", "rmsd"):
        g, w = _f8(fit[k]), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, k)
        errs[k], tols[k] = (float(np.nanmax(np.abs(g - w))) if np.isfinite(w).any() else 0.0), o["tol"][k]
    n_got = _f8(got["n1"]) + _f8(got["n0"])
    obs = _f8(fit["observed"])
    assert obs.shape == (J, G) and np.array_equal(np.isnan(obs), n_got == 0), tag
    assert ((obs[n_got > 0] >= 0) & (obs[n_got > 0] <= 1)).all(), tag
    for k, v in (("n1", 1), ("n0", 0)):
        cnt = (y == v).sum(0).astype(np.float64)
        errs["sum " + k] = float((np.abs(_f8(got[k]).sum(1) - cnt) / np.maximum(cnt, 1.0)).max())
    cnt = (y != 255).sum(0).astype(np.float64)
    errs["n_obs"] = float((np.abs(_f8(fit["n_obs"]) - cnt) / np.maximum(cnt, 1.0)).max())
    errs["sum mass"] = abs(float(_f8(got["mass"]).sum()) - len(y)) / len(y)
    for k in ("sum n1", "sum n0", "n_obs", "sum mass"):
        tols[k] = ROW_TOL
    _report(tag, "counts", errs, tols)
    # a cell nobody could fill is exactly zero
    assert (_np(got["n1"])[(y == 1).sum(0) == 0] == 0).all() and (_np(got["n0"])[(y == 0).sum(0) == 0] == 0).all(), tag


def _hold_draws(tag, got, o):
    coord_k, node_k = ("theta", "node") if o["kind"] == "irt" else ("attr", "pattern")
    N, (G, D) = o["f"].shape[0], o["coord"].shape
    node, val = _np(got[node_k]), _np(got[coord_k])
    assert node.dtype == np.int32 and node.shape == (N, co.DRAWS)
    assert val.dtype == np.float32 and val.shape == (N, co.DRAWS, D)
    assert node.min() >= 0 and node.max() < G
    want_node, gap = o["draws"]
    sure = gap > o["gap_thr"]
    wrong = np.argwhere(sure & (node.astype(np.int64) != want_node))
    print("%s draws: %.3f %% of the (person, draw) pairs left out below the gap %.2e, %d wrong draws of %d"
          % (tag, 100 * (1 - sure.mean()), o["gap_thr"], len(wrong), sure.size))
    assert 1 - sure.mean() <= sc.ARGMAX_LEFT_OUT, tag
    assert len(wrong) == 0, (tag, wrong[:10], [(int(node[i, k]), int(want_node[i, k]), float(gap[i, k])) for i, k in wrong[:10]])
    assert np.array_equal(val, o["coord"].astype(np.float32)[node])              # the grid's own coordinates, bit for bit


def _hold_info(tag, got, i):
    """The row rule on info and gradient (floors as test_gpu_se._info_errors has them), symmetry and dead parameters exactly."""
    P = len(i["free"])
    info, grad = got["info"], got["gradient"]
    assert tuple(info.shape) == (P, P) and tuple(grad.shape) == (P,) and info.dtype == torch.float32 and info.is_cuda
    _finite(tag, got, ("info", "gradient"))
    e_i, row, e_g = _info_errors(info, grad, i["info"], i["gradient"], i["n"])
    _report(tag, "info (P %d, worst row %d)" % (P, row), {"info": e_i, "gradient": e_g}, i["tol"])
    assert torch.equal(info, info.t()), tag                                     # symmetric bit for bit
    assert got["n"] == i["n"] and np.array_equal(_np(got["free"]), i["free"])
    d = np.diag(i["info"])
    dead = np.flatnonzero(d == 0)
    gi = _np(info)
    assert (gi[dead] == 0).all() and (gi[:, dead] == 0).all() and (_np(grad)[dead] == 0).all(), tag
    assert (np.diag(gi)[d > 1e-6 * d.max()] > 0).all(), tag                     # (far below that a float32 p may round to 0)


def _same_bits(tag, a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), (tag, k, "a second call gave other bits")


@pytest.mark.parametrize("case", co.ALL_CASES, ids=co.ALL_IDS)
def test_corner_case(case):
    o = co.oracle_of(case)
    cs, kind = o["cs"], o["kind"]
    tag = cs["name"]
    eng = _ccdm_engine(cs) if kind == "cdm" else _irt_engine(cs)
    kw = {} if kind == "cdm" else {"nodes": cs["nodes"], "span": cs["span"]}
    got = eng.score(**kw)
    torch.cuda.synchronize()
    _hold_score(tag, got, o)
    _same_bits(tag, got, eng.score(**kw), list(got))
    cnt, fit = eng.expected_counts(**kw), eng.item_fit(**kw)
    torch.cuda.synchronize()
    _hold_counts(tag, cnt, fit, o)
    _same_bits(tag, cnt, eng.expected_counts(**kw), ("n1", "n0", "mass", "prob"))
    pvs = eng.plausible_values(draws=co.DRAWS, seed=co.SEED, **kw)
    torch.cuda.synchronize()
    _hold_draws(tag, pvs, o)
    _same_bits(tag, pvs, eng.plausible_values(draws=co.DRAWS, seed=co.SEED, **kw), list(pvs))
    if co.has_info(case):
        i = co.info_oracle(case)
        inf = eng.item_information(**kw)
        torch.cuda.synchronize()
        if tag == "long_j1024_g512_d3":
            assert tuple(inf["info"].shape) == (4096, 4096)
        _hold_info(tag, inf, i)
        _same_bits(tag, inf, eng.item_information(**kw), ("info", "gradient"))


def test_one_node():
    """Explicit nodes (theta = [0.3], logw = [0.0]) on corner_j16_g33: the posterior is that node.  EAP is float32(0.3) and PSD 0
    exactly, every node and every draw is 0, mass[0] is the number of persons and loglik the oracle's ll at the node, both by
    the row rule; the tables are the response counts."""
    o = co.oracle_of(co.by_name("corner_j16_g33"))
    cs = o["cs"]
    theta, logw = np.array([0.3], np.float32), np.array([0.0], np.float32)
    T1, T0 = co.item_tables(cs, "irt", theta.astype(np.float64)[:, None])
    ll = co.loglik_from_tables(T1, T0, cs["y"])[:, 0]
    eng = _irt_engine(cs)
    got = eng.score(nodes=(theta, logw))
    pvs = eng.plausible_values(draws=co.DRAWS, seed=co.SEED, nodes=(theta, logw))
    cnt = eng.expected_counts(nodes=(theta, logw))
    torch.cuda.synchronize()
    N = cs["N"]
    assert tuple(got["eap"].shape) == (N, 1) and tuple(pvs["node"].shape) == (N, co.DRAWS) and tuple(cnt["n1"].shape) == (cs["J"], 1)
    assert (_np(got["eap"]) == theta[0]).all() and (_np(got["psd"]) == 0).all() and (_np(got["node"]) == 0).all()
    assert (_np(pvs["node"]) == 0).all() and (_np(pvs["theta"]) == theta[0]).all()
    e_ll = _row_errors(_f8(got["loglik"]), ll, floor=1.0)[0]
    e_mass = abs(float(cnt["mass"][0]) - N) / N
    e_n = max(float(np.abs(_f8(cnt[k])[:, 0] - (cs["y"] == v).sum(0)).max()) / N for k, v in (("n1", 1), ("n0", 0)))
    print("one node: loglik %.2e, mass %.2e, tables %.2e (rule: %.1e)" % (e_ll, e_mass, e_n, ROW_TOL))
    assert e_ll <= ROW_TOL and e_mass <= ROW_TOL and e_n <= ROW_TOL


@pytest.mark.parametrize("idx", [0, 5], ids=[se.SE_IDS[0], se.SE_IDS[5]])
def test_info_workspace_between_the_smallest_and_the_preferred(idx):
    """vx_grid_info with the workspace that is the preferred one of 1 024 persons.  By gi_slab_plan (grid_plan.h) a slab then holds
    1 024 persons = 32 units of 32 in four chunks of eight units: the 2 500 persons (P 74, PT 3, one workgroup block) go as
    slabs of 1 024, 1 024 and 452, the 1 500 of se_dina_k3 (P 40, PT 2) as 1 024 and 476.  The last slab has 16 units (eight of 64
    persons from k_grid_pscores), so its chunks 2 and 3 run k_grid_xprod over an empty unit range and must leave exact zero tiles
    for vx_reduce_slabs.  The result against the oracle and against the one-slab result by the row rule; symmetric bit for bit;
    the same bits on a second call."""
    cs, kind, o = _case("se", se.SE_CASES[idx])
    eng = _engine(cs, kind)
    one, g_one, (P, G, n) = _raw_info(eng, cs, kind, None)
    be = eng.be
    ws = be.grid_info_workspace(1024, P, G)
    PT = (P + 32) // 32
    pairs = PT * (PT + 1) // 2
    assert ws == (32 * PT + (4 + 2) * pairs) * 1024                             # 32 units of S, four chunk partials, two sums
    assert be.grid_info_workspace_min(P, G) < ws < be.grid_info_workspace(n, P, G)
    assert 2048 < n < 3072 if idx == 0 else 1024 < n < 2048
    assert -(-(n % 1024) // 64) * 2 == 16                                       # the last slab's units: chunks 2 and 3 are empty
    mid, g_mid, _ = _raw_info(eng, cs, kind, ws)
    e_i, row, e_g = _info_errors(mid, g_mid, _f8(one), _f8(g_one), n)
    a_i, _, a_g = _info_errors(mid, g_mid, o["info"], o["gradient"], n)
    print("%s: slabs of 1 024 in four chunks against one slab: info %.2e gradient %.2e; against the oracle: info %.2e gradient "
          "%.2e (rule: %.1e)" % (cs["name"], e_i, e_g, a_i, a_g, ROW_TOL))
    assert e_i <= ROW_TOL and e_g <= ROW_TOL and a_i <= ROW_TOL and a_g <= ROW_TOL
    assert bool(torch.isfinite(mid).all()) and torch.equal(mid, mid.t())
    again, g_again, _ = _raw_info(eng, cs, kind, ws)
    assert torch.equal(mid, again) and torch.equal(g_mid, g_again)


def test_oracle_comparisons_under_a_second_schedule():
    """long_j1024_d1 and the DINA K = 9 case again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "test_corner_case and (long_j1024_d1 or corner_dina_k9)"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "2 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
