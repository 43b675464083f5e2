"""item_information(prior=) / item_se(prior=) on the GPU: the information of the 3PL / 4PL item parameters at the Bayes-modal fit
(vx_grid_wtable_irt_map: k_grid_wtable_irt_asym, then vx_grid_info at K up to 6) against the float64 oracle of
tests/se_map_cases.py.

Engines are set up as tests/test_gpu_se.py does it: parameters copied into the engine's views, nothing trained -- but in the fit
test.  Rules, as there: info by the project's row rule, _row_errors(got, want, floor = max diagonal) <= ROW_TOL (3e-5); the
gradient as one row with floor = (max diagonal x n)^0.5; standard errors: relative error <= ROW_TOL x the oracle's condition
number of the block that is inverted.  The bounds do not come from the kernels: the same arithmetic said again in numpy
(tests/test_se_map_host.py) stays below a third of each on exactly these cases.  The errors found are printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import score_cases as sc
from tests import se_map_cases as sm
from tests.test_gpu_parity import _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors
from tests.test_gpu_score import _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")


def _kw(cs):
    return {"nodes": cs["nodes"], "span": cs["span"]}


def _f8(t):
    return (_np(t) if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _hold_info(tag, got, o):
    """The row rule on info and gradient, the exact structure, free, index and K, the prior's share; prints what it finds."""
    P, K = len(o["free"]), o["K"]
    info, grad = got["info"], got["gradient"]
    assert tuple(info.shape) == (P, P) and tuple(grad.shape) == (P,) and info.dtype == torch.float32 and info.is_cuda
    e_i, row, e_g = sm.info_errors(_f8(info), _f8(grad), o["info"], o["gradient"], o["n"])
    print("%s: P %d, K %d, info %.2e (row %d), gradient %.2e (rule: %.1e)" % (tag, P, K, e_i, row, e_g, ROW_TOL))
    assert e_i <= ROW_TOL and e_g <= ROW_TOL, (tag, e_i, row, e_g)
    assert torch.equal(info, info.t()), tag                                     # symmetric bit for bit
    assert got["n"] == o["n"] and isinstance(got["n"], int)
    assert np.array_equal(_np(got["free"]), o["free"]) and got["free"].dtype == torch.bool
    assert np.array_equal(got["index"]["item"], np.arange(P) // K) and np.array_equal(got["index"]["k"], np.arange(P) % K)
    # the item nobody answered: its rows, its columns and its gradient are exact zeros, and nothing else is
    dead = np.flatnonzero(np.diag(o["info"]) == 0)
    assert np.array_equal(dead, sm.UNANSWERED * K + np.arange(K))
    gi = _np(info)
    assert (gi[dead] == 0).all() and (gi[:, dead] == 0).all() and (_np(grad)[dead] == 0).all(), tag
    assert (np.diag(gi)[np.diag(o["info"]) > 0] > 0).all(), tag
    for k in ("prior_precision", "prior_gradient"):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == np.float64 and got[k].shape == (P,), k
        assert np.allclose(got[k], o[k], rtol=1e-12, atol=0), k
    assert (got["prior_precision"][~o["free"]] == 0).all() and (got["prior_gradient"][~o["free"]] == 0).all()


@pytest.mark.parametrize("name", sm.IDS)
def test_info_vs_oracle(name):
    """Cases 1 and 2 of the issue at 300 persons: one slab of 256 and a ragged one."""
    cs, o = sm.oracle_of(name, sm.N_INFO)
    eng = _irt_engine(cs)
    got = eng.item_information(prior=cs["prior"], **_kw(cs))
    torch.cuda.synchronize()
    assert set(got) == {"info", "gradient", "n", "free", "index", "prior_precision", "prior_gradient"}
    _hold_info(name, got, o)
    # two independent kernels against each other: the gradient the penalised M-step would form from expected_counts() of this engine
    c = eng.expected_counts(**_kw(cs))
    want = sm.mstep_gradient(cs, _f8(c["n1"]), _f8(c["n0"]))
    top = float(np.abs(np.diag(o["info"])).max())
    e, _ = _row_errors((_f8(got["gradient"]) + got["prior_gradient"])[None, :], want[None, :], floor=np.sqrt(top * o["n"]))
    print("%s: gradient + prior_gradient against the penalised M-step's from expected_counts(): %.2e" % (name, e))
    assert e <= ROW_TOL, (name, e)
    # the same call twice: the same bits
    again = eng.item_information(prior=cs["prior"], **_kw(cs))
    torch.cuda.synchronize()
    assert torch.equal(got["info"], again["info"]) and torch.equal(got["gradient"], again["gradient"])


@pytest.mark.parametrize("name", sm.IDS)
def test_item_se_vs_oracle(name):
    cs, o = sm.oracle_of(name, sm.N_SE)
    eng = _irt_engine(cs)
    got = eng.item_se(prior=cs["prior"], **_kw(cs))
    J, D, K = cs["J"], cs["D"], o["K"]
    dense = o["se"].reshape(J, K)
    want = {"b": dense[:, 0].reshape(1, J), "a": dense[:, 1:1 + D].T, "c_un": dense[:, D + 1].reshape(1, J)}
    un = {"c": cs["params"]["c"].astype(np.float64)}
    if cs["model"] == "irt_4pl":
        want["d_un"] = dense[:, D + 2].reshape(1, J)
        un["d"] = cs["params"]["d"].astype(np.float64)
    for k, u in un.items():                                                     # the delta method: se x (1 - x)
        x = 1.0 / (1.0 + np.exp(-u))
        want[k] = want[k + "_un"] * x * (1.0 - x)
    assert set(got) == set(want) | {"cov", "kept", "gradient_max", "condition"}
    assert np.array_equal(got["kept"], o["kept"])
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape == ((D, J) if k == "a" else (1, J)) and g.dtype == np.float64, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, k)
        worst = max(worst, float(np.nanmax(np.abs(g / w - 1))))
    assert np.isnan(got["b"]).sum() == 1 and np.isnan(got["c"]).sum() == 1 and np.isnan(got["b"][0, sm.UNANSWERED])
    assert np.isnan(got["a"]).sum() == D + D * (D - 1) // 2                     # the unanswered item and the masked loadings
    e_cov = np.abs(got["cov"] - o["cov"]).max() / np.abs(o["cov"]).max()
    gmax = float(np.abs((o["gradient"] + o["prior_gradient"])[o["kept"]]).max())
    print("%s: se %.2e relative, cov %.2e of its largest entry (bound: %.1e x condition %.1f = %.2e); condition %.1f, largest "
          "|gradient of the log posterior| %.4f (oracle %.4f)" % (name, worst, e_cov, ROW_TOL, o["condition"], ROW_TOL * o["condition"],
                                                                 got["condition"], got["gradient_max"], gmax))
    assert o["condition"] <= 1e3                                                # se_cases.CONDITION_MAX
    assert worst <= ROW_TOL * o["condition"], (name, worst)
    assert e_cov <= ROW_TOL * o["condition"], (name, e_cov)
    assert abs(got["condition"] / o["condition"] - 1) <= ROW_TOL * o["condition"]
    assert got["cov"].shape == (len(o["kept"]),) * 2 and got["cov"].dtype == np.float64
    top = float(np.abs(np.diag(o["info"])).max())
    assert abs(got["gradient_max"] - gmax) <= ROW_TOL * np.sqrt(top * o["n"])


def _raw_info(eng, cs, ws_floats):
    """vx_grid_info itself over all rows, on the tables of the prior path, with a workspace of ws_floats floats (None: the
    preferred size)."""
    be = eng.be
    call, K, fill_wtable, _ = eng._info_call(None, None, prior=cs["prior"], **_kw(cs))
    post = eng._grid_posterior(call)
    P, G, n = call.J * K, call.G, call.n
    f32 = dict(dtype=torch.float32, device=_dev())
    wimg = torch.empty(be.grid_wimage_bytes(P, G), dtype=torch.uint8, device=_dev())
    fill_wtable(wimg)
    if ws_floats is None:
        ws_floats = be.grid_info_workspace(n, P, G)
    info, grad, ws = torch.full((P, P), float("nan"), **f32), torch.full((P,), float("nan"), **f32), torch.empty(ws_floats, **f32)
    be.grid_info(call.y, call.rows, n, call.J, G, K, post["img"], wimg, call.logw, post["loglik"], info, grad, ws, ws_floats)
    torch.cuda.synchronize()
    return info, grad, (P, G, n)


@pytest.mark.parametrize("name", sm.IDS)
def test_slabs_of_the_smallest_workspace(name):
    """300 persons with the smallest workspace vx_grid_info accepts (a slab of 256 and a ragged one of 44) against the
    preferred one: the row rule; each against the oracle."""
    cs, o = sm.oracle_of(name, sm.N_INFO)
    eng = _irt_engine(cs)
    one, g_one, (P, G, n) = _raw_info(eng, cs, None)
    lo = eng.be.grid_info_workspace_min(P, G)
    assert eng.be.grid_info_workspace(n, P, G) > lo and n == 300
    two, g_two, _ = _raw_info(eng, cs, lo)
    e_i, row, e_g = sm.info_errors(_f8(two), _f8(g_two), _f8(one), _f8(g_one), n)
    print("%s: two slabs against one: info %.2e gradient %.2e" % (name, e_i, e_g))
    assert e_i <= ROW_TOL and e_g <= ROW_TOL
    assert torch.equal(two, two.t())
    for inf, gr in ((one, g_one), (two, g_two)):
        a, _, b = sm.info_errors(_f8(inf), _f8(gr), o["info"], o["gradient"], n)
        assert a <= ROW_TOL and b <= ROW_TOL


@pytest.mark.parametrize("entry", sm.BIT_CASES, ids=sm.BIT_IDS)
def test_1pl_and_2pl_keep_their_bits(entry):
    """Models 1 and 2: the image of vx_grid_wtable_irt_map is vx_grid_wtable_irt's byte for byte; info and gradient of
    item_information(prior=) have the bits of the call without it; item_se(prior=) is item_se_host on those with the precision."""
    from vipsy_amd.grid import item_se_host
    case, prior = entry
    cs = sc.irt_case(case)
    eng = _irt_engine(cs)
    kw = _kw(cs)
    plain_call, K, fill_plain, free = eng._info_call(None, None, **kw)
    _, K2, fill_map, free2 = eng._info_call(None, None, prior=prior, **kw)
    assert K == K2 and torch.equal(free, free2)
    nbytes = eng.be.grid_wimage_bytes(plain_call.J * K, plain_call.G)
    img_a = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=_dev())
    img_b = torch.full((nbytes,), 0x5C, dtype=torch.uint8, device=_dev())
    fill_plain(img_a)
    fill_map(img_b)
    torch.cuda.synchronize()
    assert torch.equal(img_a, img_b)
    plain = eng.item_information(**kw)
    got = eng.item_information(prior=prior, **kw)
    torch.cuda.synchronize()
    assert set(plain) == {"info", "gradient", "n", "free", "index"}
    assert torch.equal(plain["info"], got["info"]) and torch.equal(plain["gradient"], got["gradient"])
    prec, pgrad = got["prior_precision"], got["prior_gradient"]
    assert (prec[_np(free)] > 0).any() and (prec[~_np(free)] == 0).all()
    se = eng.item_se(prior=prior, **kw)
    want = item_se_host(_np(plain["info"]), _f8(plain["gradient"]) + pgrad, _np(free), precision=prec)
    leaves = eng._se_leaves(want["se"].copy())
    assert set(se) == set(leaves) | {"cov", "kept", "gradient_max", "condition"} and set(leaves) == set(cs["params"])
    for k, w in leaves.items():
        assert np.array_equal(se[k], w, equal_nan=True), k
    assert np.array_equal(se["cov"], want["cov"]) and se["gradient_max"] == want["gradient_max"]
    # the prior narrows: every standard error is below the likelihood's alone
    alone = eng.item_se(**kw)
    assert all((se[k][np.isfinite(se[k])] <= alone[k][np.isfinite(se[k])]).all() for k in leaves)


def test_gradient_max_falls_over_a_fit():
    """500 persons x 8 items, 3PL, from the engine's own start: the largest entry of the gradient of the log posterior after
    fit_em(prior=) is below its value before -- a monotone claim.  Measured on an MI355X: 47.51 before, 0.1003 after the 13
    iterations to convergence at tol 1e-6."""
    from vipsy_amd.engine import IrtEngine
    cs = sm.case("sm1_3pl_d1_j11")
    y = np.ascontiguousarray(cs["y"][:500, :8])
    eng = IrtEngine(torch.from_numpy(y).to(_dev()), model="irt_3pl", D=1, Dc=cs["Dc"], seed=3)
    before = eng.item_se(prior=cs["prior"], **_kw(cs))
    fit = eng.fit_em(max_iter=40, prior=cs["prior"], **_kw(cs))
    after = eng.item_se(prior=cs["prior"], **_kw(cs))
    print("fit_em(prior=) over %d iterations: gradient_max %.4f before, %.4f after" % (fit["iterations"], before["gradient_max"],
                                                                                     after["gradient_max"]))
    assert np.array_equal(before["kept"], after["kept"])
    assert after["gradient_max"] < before["gradient_max"]


def test_oracle_comparisons_under_a_second_schedule():
    """One 3PL and one 4PL case (the K = 6 one) again in a child process on the library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "(info_vs_oracle or item_se_vs_oracle) and (%s)" % " or ".join(sm.SCHED2_IDS)
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
