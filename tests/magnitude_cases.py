"""Operands far from unit scale for the fp16-pair ("f16x2", vx_common.h) kernels of the amortized multivariate guide: the cases
(tests/test_magnitude_host.py on the CPU, tests/test_gpu_magnitudes.py on the GPU), the float64 forward they are judged by, and
a numpy restatement of the METHOD -- the scale words of DESIGN.md section 3, a float32 scaling, an fp16 head and an fp16
remainder with round to nearest, three products accumulated in float32 -- in the manner of count_cases.restated_f32 and
tools/sim16.py.  The restatement bounds what the method alone costs on these inputs, so that a GPU failure points at the code.

Every case is a transform of the encoder of test_gpu_parity._random_problem and of "small" slopes (0.05 (1 +- 0.3) at D >= 64).
The transforms are powers of two (and one cap on b), so the float32 parameters of a case are exact images of the unit case's."""
import os
import re

import numpy as np

from oracle import vi_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, J, D, H, missing fraction; all 2PL, full batch
SHAPES = {
    # the recorded route's small shape (tests/golden/gpu_routes.json): k_mvn_enc_fwd_b, bwd_h_b2 beside bwd_w_b, k_irt_lik_h
    # (four item chunks, the last ragged), k_fc1_bwd_c.  (At 512 x 132 x 108 the hidden gradient is none of the f16x2 kernels: not that route.)
    "A": (512, 500, 100, 64, 0.1),
    "B": (33024, 40, 8, 64, 0.1),       # k_mvn_enc_fwd_b2: 64 persons a wave
    "C": (36, 40, 8, 64, 0.1),          # one ragged person tile in every dimension-major kernel
    # estimator = 'score' (k_mvn_score_b reads the same scale words): two shapes of
    # test_mvn_score_operands_mfma_kernel_vs_scalar_kernel_and_oracle
    "S1": (1000, 40, 100, 64, 0.1),     # a large dimension, a ragged last wave
    "S2": (4104, 36, 8, 64, 0.1),       # the smallest dimension the kernel takes
}
SCORE_RUNS = [(c, s) for s in ("S1", "S2") for c in ("row_spread", "zero_head_biases")]
SEED = 11                               # the engines' Philox seed
HEADS = ("fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias")


def lik_chunk():
    """Items a workgroup of k_irt_lik_h owns (it scales a and b by the largest magnitude among them): LB_JC of the kernel."""
    src = open(os.path.join(ROOT, "vipsy_amd", "csrc", "k_irt_lik_b.hip")).read()
    return int(re.search(r"^#define\s+LB_JC\s+(\d+)", src, re.M).group(1))


# ---------------------------------------------------------------------------------------------------------------------
# the unit problem and its transforms
# ---------------------------------------------------------------------------------------------------------------------
_UNIT = {}


def unit_problem(shape):
    """y, the _random_problem encoder, small slopes on the default zero pattern, b = 0.5 randn; float32 values in float64 arrays."""
    if shape not in _UNIT:
        from tests.test_gpu_parity import _random_problem
        N, J, D, H, miss = SHAPES[shape]
        y, enc, rng = _random_problem(N, J, D, H, "irt_2pl", miss, seed=N + J + D)
        slope = 0.05 if D >= 64 else 0.3
        a = slope * (1 + 0.3 * rng.randn(D, J)) * vo.default_a_free(D, J)
        b = 0.5 * rng.randn(1, J)
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
        _UNIT[shape] = {"y": y, "enc": {k: f32(v) for k, v in enc.items()}, "a": f32(a), "b": f32(b), "Dc": 1.0}
    u = _UNIT[shape]
    return {"y": u["y"], "enc": {k: v.copy() for k, v in u["enc"].items()}, "a": u["a"].copy(), "b": u["b"].copy(), "Dc": 1.0}


def _scale(p, keys, e):
    for k in keys:
        p["enc"][k] *= 2.0 ** e


def _row_spread(p, e):
    """Every other row of W22 and of W21 (the odd ones, in the tensors' own order -- which interleaves them inside every
    32-row tile of the packed order, pk_decode), with its bias entry, times 2^e."""
    for w, b in (("fc22.weight", "fc22.bias"), ("fc21.weight", "fc21.bias")):
        p["enc"][w][1::2] *= 2.0 ** e
        p["enc"][b][1::2] *= 2.0 ** e


def _unit(p):
    pass


def _heads_small(p):
    _scale(p, HEADS, -20)


def _wide_h(p):
    _scale(p, ("fc1.weight", "fc1.bias"), 4)
    _scale(p, HEADS, -8)


def _flat_h(p):
    # narrowed from 2^-16.  With every h at log 2 a row of the head weight gradient is log 2 times a sum over the persons of
    # zero-mean terms; the sum cancels, and the float32 CHAIN itself then misses the row rule on the rows that cancel most
    # (shape A: 4.0e-4 at 2^-16, 5.7e-5 at 2^-6, 2.0e-5 at 2^-4, 7.5e-6 at 2^-2; the fp16 pairs the same within 30 %).
    # 2^-2 is the widest spread that keeps a third of ROW_TOL; the power of two of a tiny W1 (sc[0]) is still exercised
    # by element_spread and the fc1 outliers.
    _scale(p, ("fc1.weight", "fc1.bias"), -2)


def _rows(p):
    _row_spread(p, -12)


def _elements(p):
    rng = np.random.RandomState(77)
    for k in ("fc21.weight", "fc22.weight", "fc1.weight"):
        p["enc"][k] *= 2.0 ** rng.randint(-12, 1, size=p["enc"][k].shape)


def _zero_bias(p):
    _row_spread(p, -12)
    p["enc"]["fc21.bias"][:] = 0.0
    p["enc"]["fc22.bias"][:] = 0.0


def _tiny_bias(p):
    _scale(p, ("fc21.bias", "fc22.bias"), -30)


def _dominant_bias(p):
    # the trade-off DESIGN.md section 4 states: the weights give up headroom (five bits here) to a bias 2^10 above them
    _scale(p, ("fc21.weight", "fc22.weight"), -10)
    p["enc"]["fc21.weight"][1::2] *= 2.0 ** -6
    p["enc"]["fc22.weight"][1::2] *= 2.0 ** -6


def _items(p):
    J, jc = p["a"].shape[1], lik_chunk()
    n_chunks = (J + jc - 1) // jc
    assert n_chunks >= 2, "the item case needs two chunks of k_irt_lik_h"
    b = p["b"]
    sel = np.arange(J) % 7 == 0
    # a few large intercepts among the chunks' small slopes.  |z| = Dc |x.a + b| has to stay under 15 with Dc = 1.702 and
    # |x.a| up to 5.4 in the unit case: every slope is halved and the cap is 5, inside the |b| <= 8 asked for
    p["a"] *= 0.5
    b[0, sel] = np.clip(b[0, sel] * 8.0, -5.0, 5.0)
    p["a"][:, :jc] *= 2.0 ** -10                                    # chunk 0: every slope far below the chunk's largest |b|
    p["a"][:, (n_chunks - 1) * jc:] = 0.0                           # the last chunk: a = b = 0, its maximum is 0
    b[0, (n_chunks - 1) * jc:] = 0.0
    p["Dc"] = 1.702


def _outlier(key, where):
    """One entry far above everything else in its tensor: set to 2^6 (heads) or 2^4 (fc1) times the tensor's largest magnitude,
    its own sign kept, so that a maximum that misses it leaves a scaled value of 2^18 or more -- an fp16 overflow.
    Heads: the four head tensors (a bias entry: the two biases, or it would dominate |W||h| and cost the weights a bit) are
    first brought down by 2^-6, which puts the entry at the unit case's largest magnitude -- 64 times a unit-scale diagonal row of W22 puts exp(M_kk) beyond 300 at D = 8 and the latent outside the conditions.
    fc1: narrowed to 2^4.  64 max |W1| = 22 to 35 sends |z| past 15 on all three shapes (up to 41), and bringing fc1 down
    first flattens h: the rows of the head weight gradient, sums over the persons, then cancel and the float32 chain itself
    leaves a third of ROW_TOL (1.7e-5 at 2^-2 on 512 x 132 x 108); 2^4 with fc1 as it is keeps every condition and the method's bound."""
    def f(p):
        heads = key in HEADS
        if heads:
            _scale(p, HEADS if key.endswith("weight") else ("fc21.bias", "fc22.bias"), -6)
        flat = p["enc"][key].reshape(-1)
        i = {"first": 0, "last": flat.size - 1, "middle": flat.size // 2 + (3 if flat.size > 16 else 0)}[where]
        big = (64.0 if heads else 16.0) * np.abs(flat).max()
        flat[i] = big if flat[i] >= 0 else -big
    return f


# name -> (transform, runs on shapes B and C too, the bias dominates |W||h| (the weights give up headroom by design))
CASES = {
    "unit": (_unit, True, False),
    "heads_small": (_heads_small, False, False),
    "wide_h": (_wide_h, True, False),
    "flat_h": (_flat_h, False, False),
    "row_spread": (_rows, True, False),
    "element_spread": (_elements, False, False),
    "zero_head_biases": (_zero_bias, True, False),
    "tiny_biases": (_tiny_bias, False, False),
    "dominant_biases": (_dominant_bias, False, True),
    "items": (_items, False, False),
}
OUTLIER_TENSORS = ("fc22.weight", "fc22.bias", "fc21.weight", "fc21.bias", "fc1.weight", "fc1.bias")
for _k in OUTLIER_TENSORS:
    for _w in ("first", "last", "middle"):
        CASES["outlier_%s_%s" % (_k.replace("fc", "").replace(".weight", "W").replace(".bias", "b"), _w)] = (_outlier(_k, _w), True, False)


def runs():
    """(case, shape) pairs of the GPU file: every case on A, the starred ones on B and C as well; 'items' needs two chunks: A."""
    out = [(c, "A") for c in CASES]
    out += [(c, s) for s in ("B", "C") for c, (_, star, _) in CASES.items() if star]
    return out


def problem(case, shape):
    p = unit_problem(shape)
    CASES[case][0](p)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    p["enc"] = {k: f32(v) for k, v in p["enc"].items()}
    p["a"], p["b"] = f32(p["a"]), f32(p["b"])
    p["case"], p["shape"], p["bias_dominates"] = case, shape, CASES[case][2]
    return p


def params_of(p):
    out = {"a": p["a"], "b": p["b"]}
    out.update({"encoder$$$" + k: v for k, v in p["enc"].items()})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64: the oracle in person chunks, the forward values and the operands of the head weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def forward64(params, y, eps, Dc=1.0, operands=False):
    """x, h, ent = 0.5 |eps|^2 + sum_k M_kk, the head outputs loc / raw and the logits z of the amortized guide (vi.py:448-455,
    692-693) for every person; with operands also gx = d ELBO / d x and the rows V of the head weight gradient
    G = V^T h (oracle/vi_oracle.py::irt_particle, pathwise, plate scale 1): V[(k, c)] = gx_k eps_c, V[(k, k)] = gx_k eps_k
    exp(M_kk) + 1, V[loc k] = gx_k -- the gradients of the LOSS are their negatives."""
    W = {k: params["encoder$$$" + k] for k in vo.ENC_KEYS}
    D = W["fc21.weight"].shape[0]
    loc, raw, cache = vo.enc_forward(W, vo.enc_input(y, np.float64))
    ec = eps.astype(np.float64)
    r_, c_ = vo.tril_rows_cols(D)
    dsel = np.flatnonzero(r_ == c_)
    x, col0 = loc.copy(), 0
    for k in range(D):                                   # row k of L: raw[(k, 0..k-1)] off the diagonal, exp on it (vi.py:452-454)
        x[:, k] += (raw[:, col0:col0 + k] * ec[:, :k]).sum(1) + np.exp(raw[:, col0 + k]) * ec[:, k]
        col0 += k + 1
    out = {"x": x, "h": cache[2], "ent": 0.5 * (ec ** 2).sum(1) + raw[:, dsel].sum(1), "loc": loc, "raw": raw,
           "z": Dc * (x @ params["a"] + params["b"])}
    if operands:
        _, g = vo.irt_loglik("irt_2pl", x, params["a"], params["b"], None, None, Dc, y)
        gx = g["x"] - x
        V = gx[:, r_] * ec[:, c_]
        V[:, dsel] = V[:, dsel] * np.exp(raw[:, dsel]) + 1.0
        # R = Dc dlogp/dz [n][J]: the item gradients of the loss are -x^T R (a, on its free pattern) and -sum_p R (b)
        out.update(gx=gx, V22=V, V21=gx, R=_lik_R(x, params["a"], params["b"], Dc, y))
    return out


def _lik_R(x, a, b, Dc, y):
    """Dc dlogp/dz of the 2PL link for every cell (0 where the response is missing), |z| away from the clamp."""
    z = Dc * (x @ a + b)
    return Dc * np.where(y == 255, 0.0, np.where(y == 1, 1.0, 0.0) - vo.sigmoid(z))


def item_columns(ga, gb):
    """The gradients of a [D][J] and b [1][J] as ONE column per item, [J][D + 1]: the likelihood kernels compute them as one
    product x_aug^T R (b's row is the one of the constant 1 appended to x).  The row rule is applied to these columns.  An
    item's entry of b ALONE is a single sum over the persons of terms of either sign; held to its own magnitude it measures
    how far that sum happens to cancel -- the float32 sum of the float64 terms already misses ROW_TOL that way on the unit
    case (tests/test_magnitude_host.py prints it) -- and not the kernel."""
    return np.concatenate([ga, gb.reshape(1, -1)], axis=0).T


def oracle_chunked(params, y, eps, model="irt_2pl", Dc=1.0, chunk=2048):
    """oracle/vi_oracle.py::loss_and_grads on a full batch too large for one call ((B, D, D) temporaries): a full-batch loss and
    every gradient are sums over the persons (plate scale N / B = 1), so person chunks are evaluated with spec N = chunk size
    and added.  Also returns the per-person forward values x, h and ent of the guide."""
    N, J = y.shape
    D = params["encoder$$$fc21.weight"].shape[0]
    H = params["encoder$$$fc1.weight"].shape[0]
    loss, grads = 0.0, None
    x_o, h_o, ent_o = np.empty((N, D)), np.empty((N, H)), np.empty(N)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        yc, ec = y[lo:hi], eps[lo:hi].astype(np.float64)
        spec = {"family": "irt", "model": model, "D": D, "Dc": Dc, "N": hi - lo, "amortized": True, "share_cov": False,
                "a_free": vo.default_a_free(D, J)}
        l, g = vo.loss_and_grads(spec, params, yc, [np.arange(hi - lo)], [ec])
        loss += l
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
        f = forward64(params, yc, ec)
        x_o[lo:hi], h_o[lo:hi], ent_o[lo:hi] = f["x"], f["h"], f["ent"]
    return loss, grads, x_o, h_o, ent_o


def row_errors(got, want, floor):
    """tests/test_gpu_response_designs.py::_row_errors (restated: this module imports no GPU test file at import time)."""
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    assert got.shape == want.shape
    err = np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), floor)
    return float(err.max()), int(err.argmax())


# ---------------------------------------------------------------------------------------------------------------------
# the method, restated in numpy
# ---------------------------------------------------------------------------------------------------------------------
def f16_scale_exp(vmax):
    """vx_common.h: the exponent s with |v| 2^s < 2^15 for |v| <= vmax; 0 for vmax = 0 or not finite."""
    vmax = float(np.float32(vmax))
    if not (vmax > 0.0) or not (vmax < 3.0e38):
        return 0
    return 15 - int(np.frexp(vmax)[1])


def scale_words(enc):
    """every operand brought under 2^15 by the power of two of its tensor's largest magnitude (h: of the
    bound softplus(max_u |W1[u, :]|_1 + |b1[u]|)); the bias enters the accumulator as (b 2^sb) x 2^eb with eb = sw + sh - sb
    kept an fp16 normal, -14 <= eb <= 15: a bias far above |W||h| costs the weights headroom, one far below sits lower in the
    fp16 range -- and an all-zero bias is NO bias term: the weights keep their power of two, sb is whatever puts eb in range."""
    a32 = lambda k: np.abs(np.asarray(enc[k], np.float32))
    mw = max(a32("fc21.weight").max(), a32("fc22.weight").max())
    mb = max(a32("fc21.bias").max(), a32("fc22.bias").max())
    m1 = a32("fc1.weight").max()
    l1 = float((a32("fc1.weight").astype(np.float64).sum(1) + a32("fc1.bias")).max())
    hbound = 1.001 * (max(l1, 0.0) + np.log1p(np.exp(-abs(l1)))) + 1e-30
    sw1, sh, sw = f16_scale_exp(m1), f16_scale_exp(hbound), f16_scale_exp(mw)
    if mb > 0:
        sb = f16_scale_exp(mb)
        eb = sw + sh - sb
        if eb > 15:
            sw, eb = sw - (eb - 15), 15
        if eb < -14:
            sb, eb = sw + sh + 14, -14
    else:
        eb = min(max(sw + sh, -14), 15)
        sb = sw + sh - eb
    return {"sw1": sw1, "sw": sw, "sh": sh, "sb": sb, "eb": eb, "hbound": hbound, "mw": mw, "mb": mb, "m1": m1}


def split2h(v, s):
    """v 2^s in float32 -> fp16 head and fp16 remainder (round to nearest at both stages), as float32 arrays."""
    t = (np.asarray(v, np.float32) * np.float32(2.0) ** s).astype(np.float32)
    with np.errstate(over="ignore"):
        hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def three_products(ah, al, bh, bl):
    """lo hi + hi lo + hi hi, each a float32 matmul, added in float32 in the kernels' order."""
    return ((al @ bh).astype(np.float32) + (ah @ bl).astype(np.float32)) + (ah @ bh).astype(np.float32)


def restated_heads(enc, h, sw_words=None):
    """The head GEMM as the forward kernels run it: [loc | raw] [n][D + T] in float64 from float32 arithmetic."""
    s = scale_words(enc) if sw_words is None else sw_words
    W = np.concatenate([enc["fc21.weight"], enc["fc22.weight"]])
    b = np.concatenate([enc["fc21.bias"], enc["fc22.bias"]])
    wh, wl = split2h(W, s["sw"])
    hh, hl = split2h(h, s["sh"])
    bh, bl = split2h(b, s["sb"])
    c = np.float32(2.0) ** s["eb"]
    acc = (bl * c + bh * c).astype(np.float32)[None, :] + three_products(hh, hl, wh.T, wl.T)
    return acc.astype(np.float64) * 2.0 ** -(s["sw"] + s["sh"])


def restated_head_grads(V, h, sh, vmax):
    """The head weight gradient G[r] = sum_p V[p][r] h[p] as k_mvn_enc_bwd_w_b runs it: V in float32 times ONE power of two for
    the launch -- of vmax = max(|gx|max |eps|max, |gd|max, |gx|max), the bound the kernel takes from the step's operand maxima --
    h 2^sh, two fp16 terms each, three products."""
    V32 = np.asarray(V, np.float32)
    sv = f16_scale_exp(vmax)
    vh, vl = split2h(V32, sv)
    hh, hl = split2h(h, sh)
    return three_products(vh.T, vl.T, hh, hl).astype(np.float64) * 2.0 ** -(sv + sh)
