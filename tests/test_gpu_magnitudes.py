"""The fp16-pair ("f16x2") kernels of the amortized multivariate guide on operands far from unit scale (tests/magnitude_cases.py):
heads 2^-20, a hidden layer spanning 2^8, rows and elements spread over 2^12, one entry far above its tensor at the first, the
last and a middle position of each of the six encoder tensors, head biases that are zero, tiny (2^-30) or dominant, item chunks
of k_irt_lik_h whose largest magnitude is 0 or sits 2^13 above their slopes, Dc = 1.702.  The power of two that brings every
operand to the top of the fp16 range (sc[0..10]) is computed from maxima taken by several kernels; none
of that was reached by inputs whose entries all lie near 1.

Every case builds its engine as test_mvn_amortized_step_vs_oracle does, calls loss_and_grads once and is held to the float64
oracle (oracle/vi_oracle.py::loss_and_grads in person chunks) at the same parameters and the forward's own draws:

* the route: the measurement slots name the kernels the call took; a case that fell to another generation fails;
* everything finite (a maximum that misses an element overflows fp16), then the loss at rel 3e-5;
* every gradient by the whole-tensor rule (GRAD_TOL) AND row by row (_row_errors <= ROW_TOL): x (floor 1) and h (floor 2^-12
  max |h|) per person, ent as one row, the gradients of fc21.weight / fc22.weight / fc1.weight per output row and of a and b
  as one column [G_a; G_b] per item (magnitude_cases.item_columns says why not b's entry alone), floor 2^-12 of the tensor's
  largest oracle entry -- the whole-tensor rule alone accepts anything in the small rows;
* the scale words: sc[8..10] equal the float32 maxima bit for bit, sc[2], sc[3], sc[5], sc[6] are powers of two, the scaled
  maxima stay under 2^15, the weights sit in the top binade unless the bias dominates, sc[6] is an fp16 normal, sc[7] bounds h.

tests/test_magnitude_host.py shows on the CPU that the inputs keep |z| < 15, |x| < 100 and |M_kk| < 5 and that the method alone
(numpy restatement) meets both rules at a third of the tolerance on every case; the conditions are asserted here again.

Measured on one MI355X (the largest figure over all cases of a shape; the unit case in brackets):
    shape A  512 x 500 x 100     loss 9.5e-08 (7.9e-08)   whole-tensor 8.7e-07 (1.8e-07)   rows 3.9e-06 (1.5e-06)
    shape B  33 024 x 40 x 8     loss 9.8e-08 (3.1e-08)   whole-tensor 8.6e-07 (5.4e-07)   rows 1.7e-06 (7.2e-07)
    shape C  36 x 40 x 8         loss 1.1e-07 (6.9e-08)   whole-tensor 4.6e-07 (1.4e-07)   rows 3.0e-06 (6.4e-07)
    score operands: 4.8e-07 of the tensor's max and 1.2e-06 by rows against float64, 6.3e-07 against the scalar kernel
The worst rows are a gradient row of fc21.weight under the element spread (A) and of fc22.weight beside an outlier (B, C).
Zero head biases, run once on the library as it was before enc_scales_from_max learnt that an all-zero bias is no bias term:
sc[2] = 2^3 on shapes B, C, S1 and S2 where 2^16 (S1: 2^15) fits, sc[8] sc[2] = 3.1 to 4.6 -- the scale-word rule failed on all
of them; with the fix sc[2] = 2^16 / 2^15 and the figures above.  An item's entry of the gradient of b held to its OWN magnitude
(not what this file asserts: see magnitude_cases.item_columns) came to 1.4e-04 on the unit case of shape A, 6.8e-05 for a
float32 sum of the float64 terms on the CPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vi_oracle as vo
from tests import magnitude_cases as mc
from tests.test_gpu_parity import GRAD_TOL, _dev
from tests.test_gpu_response_designs import ROW_TOL, _row_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED2 = os.path.join(ROOT, "vipsy_amd", "_lib", "libvipsy_hip_sched2.so")

PAIR_H, PAIR_W = "k_mvn_enc_bwd_h_b2 beside k_mvn_enc_bwd_w_b", "k_mvn_enc_bwd_w_b beside k_mvn_enc_bwd_h_b2"
FC1 = "k_fc1_bwd_c"
# the measurement slots a call has to fill (the f16x2 hidden gradient and head weight gradient run side by side at all three)
ROUTES = {
    "A": {"k_mvn_enc_fwd_b", PAIR_H, PAIR_W, "k_irt_lik_h", FC1},
    "B": {"k_mvn_enc_fwd_b2", PAIR_H, PAIR_W, FC1},
    "C": {"k_mvn_enc_fwd_b", PAIR_H, PAIR_W, FC1},
}


def _id(r):
    return "%s__%s" % r


def _engine(p, **kw):
    from vipsy_amd.engine import IrtEngine
    N, J, D, H, _ = mc.SHAPES[p["shape"]]
    eng = IrtEngine(torch.from_numpy(p["y"]).to(_dev()), model="irt_2pl", D=D, Dc=p["Dc"], amortized=True, H=H, seed=mc.SEED,
                    encoder_init={k: v.astype(np.float32) for k, v in p["enc"].items()}, **kw)
    eng.unconstrained("a").copy_(torch.from_numpy(p["a"]).float())
    eng.unconstrained("b").copy_(torch.from_numpy(p["b"]).float())
    params = {n: eng.unconstrained(n).cpu().numpy().astype(np.float64) for n in eng.names()}
    want = mc.params_of(p)
    assert sorted(params) == sorted(want)
    for n in want:                                  # the engine holds the case's float32 parameters, bit for bit
        assert np.array_equal(params[n].reshape(want[n].shape), want[n]), n
    return eng, params


def _routed_call(eng):
    """loss_and_grads with the measurement slots on: the names of the kernels the call took (tests/helpers/gpu_routes.py)."""
    lib = eng.be.L
    torch.cuda.synchronize()
    assert lib.vx_prof_enable(1) == 0
    try:
        eng.loss_and_grads()
        torch.cuda.synchronize()
        names = set()
        for slot in range(lib.vx_prof_count()):
            nm, ms, cnt = ctypes.create_string_buffer(64), ctypes.c_float(0), ctypes.c_int(0)
            assert lib.vx_prof_read(slot, nm, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            names.add(nm.value.decode())
    finally:
        assert lib.vx_prof_enable(0) == 0
    return names


def _scale_words(eng, p, h_max):
    """sc[0..10] behind the call, held to what DESIGN.md section 3 says of them; returns them."""
    N, J, D, H, _ = mc.SHAPES[p["shape"]]
    cfg = eng.be.cfg(eng.model, D, J, H, p["Dc"], 1.0, mc.SEED, 0, 0)
    om = eng.be.mvn_pack_opmax_offset(cfg, eng.last["nb"])
    assert om >= 11, om
    sc = eng.last["fw"]["packws"][om - 11:om].cpu().numpy()
    a32 = lambda k: np.abs(p["enc"][k].astype(np.float32)).max()
    want = np.array([max(a32("fc21.weight"), a32("fc22.weight")), max(a32("fc21.bias"), a32("fc22.bias")), a32("fc1.weight")], np.float32)
    print("%s on %s: scale words %s" % (p["case"], p["shape"], " ".join("%.6g" % v for v in sc)))
    assert np.array_equal(sc[8:11].view(np.uint32), want.view(np.uint32)), (sc[8:11], want)
    for i in (0, 2, 3, 5, 6):
        assert np.isfinite(sc[i]) and sc[i] > 0 and np.frexp(sc[i])[0] == 0.5, (i, sc[i])
    assert float(sc[9]) * float(sc[5]) < 2.0 ** 15
    top = float(sc[8]) * float(sc[2])
    assert top < 2.0 ** 15 and (p["bias_dominates"] or top >= 2.0 ** 14), (top, np.log2(top))
    assert 2.0 ** -14 <= sc[6] <= 2.0 ** 15, sc[6]
    assert sc[7] >= h_max and float(sc[7]) * float(sc[3]) < 2.0 ** 15, (sc[7], h_max)
    assert 2.0 ** 14 <= float(sc[10]) * float(sc[0]) < 2.0 ** 15 and sc[1] * sc[0] == 1.0
    return sc


@pytest.mark.parametrize("case,shape", mc.runs(), ids=[_id(r) for r in mc.runs()])
def test_magnitude_case_vs_oracle(case, shape):
    p = mc.problem(case, shape)
    N, J, D, H, _ = mc.SHAPES[shape]
    eng, params = _engine(p)
    names = _routed_call(eng)
    print("%s on %s: route %s" % (case, shape, sorted(names)))
    fw = eng.last["fw"]
    eps = fw["eps"][:N * D].reshape(N, D).cpu().numpy()
    np.testing.assert_allclose(eps, vo.philox_normals(mc.SEED, 0, 0, np.arange(N), D), atol=2e-5)
    got = {"x": fw["x"][:N * D].reshape(N, D).cpu().numpy(), "h": fw["h"][:N * H].reshape(N, H).cpu().numpy(),
           "ent": fw["ent"][:N].cpu().numpy()}
    loss_h = float(eng.G[eng.n_params].item())
    g_h = {n: eng.unconstrained(n, eng.G).cpu().numpy() * eng.unconstrained(n, eng.free).cpu().numpy() for n in eng.names()}
    assert ROUTES[shape] <= names, (case, shape, sorted(ROUTES[shape] - names), sorted(names))
    # a maximum that missed an element has overflowed fp16 by now
    assert np.isfinite(loss_h) and all(np.isfinite(v).all() for v in got.values()) and all(np.isfinite(v).all() for v in g_h.values())

    loss_o, g_o, x_o, h_o, ent_o = mc.oracle_chunked(params, p["y"], eps, Dc=p["Dc"])
    z_o = p["Dc"] * (x_o @ params["a"] + params["b"])
    assert np.abs(z_o).max() < 15.0 and np.abs(x_o).max() < 100.0            # no cell near the clamp; k_irt_lik_h does the step
    sc = _scale_words(eng, p, h_o.max())

    rows = {"x": _row_errors(got["x"], x_o, 1.0), "h": _row_errors(got["h"], h_o, 2.0 ** -12 * np.abs(h_o).max()),
            "ent": _row_errors(got["ent"][None, :], ent_o[None, :], 1.0)}
    tens = {}
    assert sorted(g_o) == sorted(g_h)
    for name, go in g_o.items():
        gh = g_h[name].reshape(go.shape)
        top = float(np.abs(go).max())
        tens[name] = float(np.abs(gh - go).max() / max(1e-6, top))
        if name.endswith("weight"):
            rows["G " + name] = _row_errors(gh, go, 2.0 ** -12 * top)
    ab_o = mc.item_columns(g_o["a"], g_o["b"])                                    # one column [G_a; G_b] per item
    rows["G a|b"] = _row_errors(mc.item_columns(g_h["a"].reshape(g_o["a"].shape), g_h["b"]), ab_o, 2.0 ** -12 * np.abs(ab_o).max())
    loss_err = abs(loss_h - loss_o) / abs(loss_o)
    print("MAGNITUDES %s on %s: loss %.2e (rel 3e-5); whole-tensor %s (bound %.0e); rows %s (bound %.0e)"
          % (case, shape, loss_err, "  ".join("%s %.2e" % (k.replace("encoder$$$", ""), v) for k, v in tens.items()), GRAD_TOL,
             "  ".join("%s %.2e" % (k.replace("encoder$$$", ""), v[0]) for k, v in rows.items()), ROW_TOL))
    assert loss_h == pytest.approx(loss_o, rel=3e-5)
    assert max(tens.values()) < GRAD_TOL, (case, shape, tens)
    for k, (e, worst) in rows.items():
        assert e <= ROW_TOL, (case, shape, k, "row", worst, e)


@pytest.mark.parametrize("case,shape", mc.SCORE_RUNS, ids=[_id(r) for r in mc.SCORE_RUNS])
def test_score_operands_on_spread_head_rows(case, shape):
    """k_mvn_score_b reads sc[2], sc[5], sc[6] for its column-order image of the head rows: the row-spread cases through
    estimator = 'score', the operands gxT / gdT against the scalar kernel (same engine state) and against float64 (L rebuilt
    from the heads, u by a triangular solve) for a sample of the persons, whole tensor and person by person."""
    p = mc.problem(case, shape)
    N, J, D, H, _ = mc.SHAPES[shape]
    eng, params = _engine(p, estimator="score", baseline="avg", baseline_beta=0.8)
    gd_off = eng.be.mvn_enc_bwd_gd_offset(eng.be.cfg(eng.model, D, J, H, 1.0, 1.0, mc.SEED, 0, 0), N)
    assert gd_off >= 0
    out = {}
    for mfma in (True, False):
        eng.score_mfma = mfma
        eng.base.zero_()
        names = _routed_call(eng)
        assert ("k_mvn_score_b" in names) == mfma, sorted(names)
        out[mfma] = (eng.last["gxT"][:N * D].reshape(D, N).cpu().numpy().copy(),
                     eng._ws["encb_ws"][gd_off:gd_off + N * D].reshape(D, N).cpu().numpy().copy(), eng.last_log_r.cpu().numpy().copy())
    fw = eng.last["fw"]
    rng = np.random.RandomState(5)
    idx = np.unique(np.concatenate([np.arange(40), np.arange(N - 40, N), rng.choice(N, 200, replace=False)]))
    eps = fw["eps"][:N * D].reshape(N, D).cpu().numpy()[idx].astype(np.float64)
    f = mc.forward64(params, p["y"][idx], eps)
    _scale_words(eng, p, f["h"].max())
    r_, c_ = vo.tril_rows_cols(D)
    w = out[True][2][idx].astype(np.float64)                  # log_r - baseline (the baseline starts at zero)
    gx_o, gd_o = np.empty((len(idx), D)), np.empty((len(idx), D))
    for n in range(len(idx)):
        M = np.zeros((D, D))
        M[r_, c_] = f["raw"][n]
        L = np.tril(M, -1) + np.diag(np.exp(np.diag(M)))
        u = np.linalg.solve(L.T, eps[n])
        gx_o[n] = w[n] * u
        gd_o[n] = w[n] * (u * eps[n] * np.diag(L) - 1.0)
    errs = {}
    for q, name, want in ((0, "gxT", gx_o), (1, "gdT", gd_o)):
        assert np.isfinite(out[True][q]).all(), name
        errs[name + " MFMA / scalar"] = np.abs(out[True][q] - out[False][q]).max() / np.abs(out[False][q]).max()
        g = out[True][q][:, idx].T
        errs[name + " / float64"] = np.abs(g - want).max() / np.abs(want).max()
        errs[name + " / float64, rows"] = _row_errors(g, want, 2.0 ** -12 * np.abs(want).max())[0]
    print("MAGNITUDES score operands, %s on %s: %s" % (case, shape, "  ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= (ROW_TOL if "rows" in k else GRAD_TOL), (case, shape, k, e)


def test_magnitude_cases_under_a_second_schedule():
    """The unit case, the row spread and the outlier at the last element of W22 (shape A) again, in a child process on the
    library built under the other instruction schedule."""
    assert os.path.exists(SCHED2), "build it: make -C vipsy_amd/csrc sched2 (or __graft_entry__.build())"
    env = dict(os.environ)
    env["VX_LIB"] = SCHED2
    sel = "case_vs_oracle and (unit__A or row_spread__A or outlier_22W_last__A)"
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert "3 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1], tail
    probe = subprocess.run([sys.executable, "-c", "from vipsy_amd import _hip; print(_hip.LIB_PATH); _hip.lib()"], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert probe.returncode == 0 and probe.stdout.strip().endswith("libvipsy_hip_sched2.so"), probe.stdout + probe.stderr
