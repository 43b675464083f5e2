"""The magnitude cases of tests/magnitude_cases.py, the parts that need no GPU: every case's conditions in the float64 oracle
(no logit near the Bernoulli clamp, the latent inside the fp16 image of k_irt_lik_h, a moderate Cholesky diagonal), and the
METHOD alone -- scale words, float32 scaling, fp16 head and remainder, three float32 products, restated in numpy -- against
float64 on the head GEMM and the head weight gradient, under the whole-tensor rule and the row rule at a THIRD of the
project's tolerances (the rest is room for the float32 work around the GEMMs: softplus, exp, the likelihood).  A GPU failure
of tests/test_gpu_magnitudes.py is then the code's, not the inputs' and not the method's."""
import numpy as np
import pytest

from oracle import vi_oracle as vo
from tests import magnitude_cases as mc
from tests.test_gpu_parity import GRAD_TOL
from tests.test_gpu_response_designs import ROW_TOL, _row_errors

RUNS = mc.runs() + mc.SCORE_RUNS


def _id(r):
    return "%s__%s" % r


@pytest.mark.parametrize("case,shape", RUNS, ids=[_id(r) for r in RUNS])
def test_conditions_and_method_bound(case, shape):
    p = mc.problem(case, shape)
    N, J, D, H, _ = mc.SHAPES[shape]
    eps = vo.philox_normals(mc.SEED, 0, 0, np.arange(N), D)
    f = mc.forward64(mc.params_of(p), p["y"], eps, p["Dc"], operands=True)
    dsel = np.flatnonzero(np.equal(*vo.tril_rows_cols(D)))
    zmax, xmax, dmax = np.abs(f["z"]).max(), np.abs(f["x"]).max(), np.abs(f["raw"][:, dsel]).max()
    assert zmax < 15.0 and xmax < 100.0 and dmax < 5.0, (zmax, xmax, dmax)

    # ---- the head GEMM: [loc | raw], and what the tests see of it: x of every person, ent
    s = mc.scale_words(p["enc"])
    M = np.concatenate([f["loc"], f["raw"]], axis=1)
    Mr = mc.restated_heads(p["enc"], f["h"], s)
    assert np.isfinite(Mr).all()
    x_r, col0 = Mr[:, :D].copy(), D
    for k in range(D):
        x_r[:, k] += (Mr[:, col0:col0 + k] * eps[:, :k]).sum(1) + np.exp(Mr[:, col0 + k]) * eps[:, k]
        col0 += k + 1
    ent_r = 0.5 * (eps.astype(np.float64) ** 2).sum(1) + Mr[:, D:][:, dsel].sum(1)
    errs = {"M tensor": np.abs(Mr - M).max() / np.abs(M).max(),
            "x tensor": np.abs(x_r - f["x"]).max() / np.abs(f["x"]).max(),
            "x rows": _row_errors(x_r, f["x"], 1.0)[0],
            "ent row": _row_errors(ent_r[None, :], f["ent"][None, :], 1.0)[0]}

    # ---- the head weight gradients
    gxm = np.abs(f["gx"]).max()
    vmax = max(gxm * np.abs(eps).max(), np.abs(f["V22"][:, dsel]).max(), gxm)
    for name, V in (("fc22.weight", f["V22"]), ("fc21.weight", f["V21"])):
        G = V.T @ f["h"]
        Gr = mc.restated_head_grads(V, f["h"], s["sh"], vmax)
        errs["G_%s tensor" % name] = np.abs(Gr - G).max() / np.abs(G).max()
        errs["G_%s rows" % name] = _row_errors(Gr, G, 2.0 ** -12 * np.abs(G).max())[0]
    # ---- the item gradients, one column [G_a; G_b] per item: float32 operands and float32 sums, nothing else
    free = vo.default_a_free(D, J)
    R, x = f["R"], f["x"]
    want = mc.item_columns(-(x.T @ R) * free, -R.sum(0))
    R32, x32 = R.astype(np.float32), x.astype(np.float32)
    gb32 = -R32.sum(0, dtype=np.float32).astype(np.float64)
    got = mc.item_columns(-(x32.T @ R32).astype(np.float64) * free, gb32)
    errs["G_ab columns (float32)"] = _row_errors(got, want, 2.0 ** -12 * np.abs(want).max())[0]
    alone = _row_errors(gb32[:, None], want[:, -1:], 2.0 ** -12 * np.abs(want[:, -1]).max())[0]
    print("%s on %s: an item's entry of G_b held to its own magnitude, float32 sum of float64 terms: %.1e" % (case, shape, alone))
    print("%s on %s: |z| %.2f |x| %.2f |diag| %.2f; sw %d sh %d sb %d eb %d; method alone: %s"
          % (case, shape, zmax, xmax, dmax, s["sw"], s["sh"], s["sb"], s["eb"], "  ".join("%s %.1e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= (ROW_TOL if "row" in k else GRAD_TOL) / 3, (case, shape, k, e)


@pytest.mark.parametrize("case,shape", RUNS, ids=[_id(r) for r in RUNS])
def test_restated_scale_words(case, shape):
    """What the GPU file asserts of sc[], on the restated rule: every scaled maximum under 2^15, the weights at the top of the
    range unless the bias dominates, the bias constant an fp16 normal; and the branch each bias case is there for."""
    p = mc.problem(case, shape)
    s = mc.scale_words(p["enc"])
    assert s["mw"] * 2.0 ** s["sw"] < 2.0 ** 15 and s["mb"] * 2.0 ** s["sb"] < 2.0 ** 15 and s["m1"] * 2.0 ** s["sw1"] < 2.0 ** 15
    assert s["hbound"] * 2.0 ** s["sh"] < 2.0 ** 15 and s["m1"] * 2.0 ** s["sw1"] >= 2.0 ** 14
    assert -14 <= s["eb"] <= 15 and s["eb"] == s["sw"] + s["sh"] - s["sb"]
    top = s["mw"] * 2.0 ** s["sw"] >= 2.0 ** 14
    assert top != p["bias_dominates"], (case, s)
    if case == "tiny_biases":
        assert s["eb"] == -14 and s["sb"] == s["sw"] + s["sh"] + 14 and s["mb"] * 2.0 ** s["sb"] < 2.0 ** 14
    if case == "dominant_biases":
        assert s["eb"] == 15 and mc.f16_scale_exp(s["mw"]) - s["sw"] == 5          # five bits given up, by design
    if case == "zero_head_biases":
        assert s["mb"] == 0.0 and s["sw"] == mc.f16_scale_exp(s["mw"])              # no bias term: nothing given up
        assert s["sw"] + s["sh"] > 15                                                # ... where sb = 0 would have cost sw + sh - 15 bits


def test_the_cases_are_what_they_say():
    jc = mc.lik_chunk()
    J = mc.SHAPES["A"][1]
    n_ch = (J + jc - 1) // jc
    assert jc == 128 and n_ch == 4 and J % jc != 0             # four item chunks of k_irt_lik_h on shape A, the last ragged
    u, it = mc.problem("unit", "A"), mc.problem("items", "A")
    assert it["Dc"] == 1.702 and np.abs(it["b"]).max() == 5.0 and np.abs(it["b"]).max() > 2 * np.abs(u["b"]).max()
    last = (n_ch - 1) * jc
    assert not it["a"][:, last:].any() and not it["b"][:, last:].any()
    assert np.array_equal(it["a"][:, jc:last], u["a"][:, jc:last] * 0.5)
    free = vo.default_a_free(*u["a"].shape)
    assert np.array_equal(it["a"][:, :jc], u["a"][:, :jc] * 2.0 ** -11) and np.array_equal(u["a"] != 0, free)
    for key in mc.OUTLIER_TENSORS:
        short = key.replace("fc", "").replace(".weight", "W").replace(".bias", "b")
        for shape in ("A", "B", "C"):
            seen = set()
            for where in ("first", "last", "middle"):
                t = np.abs(mc.problem("outlier_%s_%s" % (short, where), shape)["enc"][key]).reshape(-1)
                i = int(t.argmax())
                seen.add(i)
                rest = np.delete(t, i).max()
                assert t[i] >= (64.0 if key in mc.HEADS else 16.0) * rest, (key, shape, where)
                assert (where != "first" or i == 0) and (where != "last" or i == t.size - 1)
            assert len(seen) == 3, (key, shape, seen)
    z = mc.problem("zero_head_biases", "A")["enc"]
    r = mc.problem("row_spread", "A")["enc"]
    assert not z["fc21.bias"].any() and not z["fc22.bias"].any() and np.array_equal(z["fc22.weight"], r["fc22.weight"])
    assert np.array_equal(r["fc22.weight"][1::2], u["enc"]["fc22.weight"][1::2] * 2.0 ** -12)
    assert np.array_equal(r["fc22.bias"][1::2], u["enc"]["fc22.bias"][1::2] * 2.0 ** -12)
    assert np.array_equal(r["fc22.weight"][0::2], u["enc"]["fc22.weight"][0::2])
    starred = {c for c, sh in mc.runs() if sh == "B"}
    assert starred == {c for c, sh in mc.runs() if sh == "C"} and "items" not in starred and len(starred) == 4 + 18


def test_split_is_exact_to_the_stated_bound():
    """|v 2^s - hi - lo| <= max(2^-22 |v 2^s|, 2^-25), fp16 subnormals included."""
    rng = np.random.RandomState(3)
    v = (rng.randn(4096) * 2.0 ** rng.randint(-40, 1, size=4096)).astype(np.float32)
    s = mc.f16_scale_exp(np.abs(v).max())
    hi, lo = mc.split2h(v, s)
    t = v.astype(np.float64) * 2.0 ** s
    assert np.abs(t).max() < 2.0 ** 15
    assert (np.abs(t - hi - lo.astype(np.float64)) <= np.maximum(2.0 ** -22 * np.abs(t), 2.0 ** -25)).all()
    assert mc.f16_scale_exp(0.0) == 0 and mc.f16_scale_exp(1.0) == 14 and mc.f16_scale_exp(0.75) == 15
