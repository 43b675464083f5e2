"""The float64 oracle and the cases of the grid-score tests (tests/test_score_host.py on the CPU, tests/test_gpu_score.py on the
GPU).  The oracle is a few lines over the public pieces of oracle/vi_oracle.py: irt_loglik evaluated at x = node for every node,
dina_eta / dino_eta, bernoulli_logprob_probs, the clamped uniform Categorical of ccdm_particle, a max-shifted log-sum-exp and
the moments.  Item parameters are DRAWN (seeded), not trained; every case is the same on every machine.

Condition on the IRT inputs (checked by irt_condition, on the CPU): every person's oracle PSD is at least half the node spacing
in every dimension -- below that the quadrature itself means nothing.  The slopes of each case are drawn so that it holds (1PL
has no slopes to draw: its thresholds are spread over [-4, 4] instead, so that few items inform any one person)."""
import numpy as np

from oracle import vi_oracle as vo

ARGMAX_GAP = 1e-4            # node / pattern must equal the oracle's where its best and second-best logw + ll differ by more
ARGMAX_LEFT_OUT = 0.02       # ... and at most this share of the persons may be left out by that rule

# name, N, J, model, D, Dc, nodes per dimension, missing rate, slope range, seed
IRT_CASES = [
    ("case1_2pl_n33_j37", 33, 37, "irt_2pl", 1, 1.0, 61, 0.30, (0.5, 1.5), 11),
    ("case2_4pl_j130", 100, 130, "irt_4pl", 1, 1.702, 41, 0.10, (0.3, 0.8), 12),
    ("case3_1pl_j130", 100, 130, "irt_1pl", 1, 1.702, 41, 0.10, None, 13),
    ("case4_3pl_j500_sparse", 200, 500, "irt_3pl", 1, 1.0, 61, 0.90, (0.4, 1.0), 14),
    ("case5_2pl_d2_441", 100, 40, "irt_2pl", 2, 1.0, 21, 0.0, (0.4, 1.0), 15),
    ("case5_2pl_d3_729", 100, 40, "irt_2pl", 3, 1.0, 9, 0.0, (0.1, 0.3), 16),
]
# name, N, J, cdm, K, missing rate, seed
CDM_CASES = [
    ("case6_dina_k3", 100, 30, "dina", 3, 0.10, 21),
    ("case6_dina_k10", 100, 30, "dina", 10, 0.10, 22),
    ("case7_dino_k4", 100, 30, "dino", 4, 0.0, 23),
]
SPAN = 6.0


def _logit(p):
    return np.log(p) - np.log1p(-p)


def irt_case(case):
    """Drawn item parameters (float32, the engine's unconstrained leaves) and responses simulated from them."""
    name, N, J, model, D, Dc, nodes, missing, slopes, seed = case
    rng = np.random.RandomState(seed)
    p = {}
    if model == "irt_1pl":
        p["b"] = rng.uniform(-4.0, 4.0, size=(1, J)).astype(np.float32)
        a = np.ones((1, J))
    else:
        a = rng.uniform(slopes[0], slopes[1], size=(D, J))
        if D > 1:
            a = a * vo.default_a_free(D, J)                         # the engine's default a_free (vi.py:570-572)
        p["a"] = a.astype(np.float32)
        p["b"] = rng.normal(0.0, 1.0, size=(1, J)).astype(np.float32)
    if model in ("irt_3pl", "irt_4pl"):
        p["c"] = _logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)
    if model == "irt_4pl":
        p["d"] = _logit(rng.uniform(0.85, 0.98, size=(1, J))).astype(np.float32)
    x = rng.normal(size=(N, D))
    z = Dc * ((x + p["b"]) if model == "irt_1pl" else (x @ a + p["b"]))
    lo = vo.sigmoid(p["c"].astype(np.float64)) if "c" in p else 0.0
    hi = vo.sigmoid(p["d"].astype(np.float64)) if "d" in p else 1.0
    y = (rng.uniform(size=(N, J)) < lo + (hi - lo) * vo.sigmoid(z)).astype(np.uint8)
    if missing > 0:
        y[rng.uniform(size=(N, J)) < missing] = 255
    if name.startswith("case1"):
        y[5] = 255                                                  # nobody's answers: the prior comes back
        y[7] = 1                                                    # all correct, nothing missing
    return {"name": name, "N": N, "J": J, "model": model, "D": D, "Dc": Dc, "nodes": nodes, "span": SPAN, "y": y, "params": p}


def cdm_q(K, J, rng):
    """A binary Q-matrix [K][J] that identifies every attribute: K single-attribute items, every pair of attributes once (as
    far as the items last), the rest two or three attributes drawn."""
    q = np.zeros((K, J), np.float32)
    cols = [[k] for k in range(K)] + [[k, l] for k in range(K) for l in range(k + 1, K)]
    for j in range(J):
        ks = cols[j] if j < len(cols) else rng.choice(K, size=min(K, rng.randint(2, 4)), replace=False)
        q[np.asarray(ks), j] = 1
    return q


def cdm_case(case):
    name, N, J, cdm, K, missing, seed = case
    rng = np.random.RandomState(seed)
    q = cdm_q(K, J, rng)
    p = {"g": _logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32),
         "s": _logit(rng.uniform(0.05, 0.25, size=(1, J))).astype(np.float32)}
    eta_all, attrs = (vo.dino_eta if cdm == "dino" else vo.dina_eta)(K, q.astype(np.float64))
    if cdm == "dino":
        # the reference's dino() gives single-attribute items eta = 0 for everybody, so patterns of three and more attributes
        # meet every remaining item and cannot be told apart (an exact tie, which the argmax rule leaves out): the simulated
        # examinees hold at most two attributes
        pool = np.flatnonzero(attrs.sum(1) <= 2)
    else:
        pool = np.arange(2 ** K)
    pat = pool[rng.randint(0, len(pool), size=N)]
    eta = eta_all[pat]
    g, s = vo.sigmoid(p["g"].astype(np.float64)), vo.sigmoid(p["s"].astype(np.float64))
    y = (rng.uniform(size=(N, J)) < np.where(eta > 0, 1 - s, g)).astype(np.uint8)
    if missing > 0:
        # the holes fall on the items behind the K single-attribute ones, at the rate that leaves `missing` of all cells empty:
        # a person who lacks the one item that identifies an attribute has two patterns EXACTLY tied, which the argmax rule
        # would leave out (9 of 100 persons with holes everywhere)
        y[:, K:][rng.uniform(size=(N, J - K)) < missing * J / (J - K)] = 255
    return {"name": name, "N": N, "J": J, "cdm": cdm, "K": K, "q": q, "y": y, "params": p}


SECOND_UNIT_TAIL = 97
_SECOND = {}


def second_unit_case(cus):
    """The case in which a wave of the person-on-lane kernels takes a SECOND unit (k_grid_post, k_grid_draw: a launch stops at
    2 blocks a CU, 4 waves a block, 64 persons a unit): 2 * cus * 256 + 97 persons, 9 items (rows start at every byte alignment;
    one item chunk), 2PL, 5 nodes (one node tile).  The first 2 * cus * 256 rows -- every wave's first unit -- are coin flips with
    about 70 % of the cells missing; the last 97, the second units of two waves, are drawn as irt_case draws them, except
    eight of them with no answer at all, whose loglik is of the order of 1e-6: one missing cell carried over from the first
    unit changes its bits.  What a unit leaves behind must not reach the next; the oracle is that of the last 97 rows alone.
    (irt_condition does not hold on five nodes and is not asked: it is about what the quadrature means, not what the kernel
    computes.)  Computed once for a device; callers must not modify it."""
    if cus not in _SECOND:
        T = SECOND_UNIT_TAIL
        cs = irt_case(("second_unit_2pl_j9", T, 9, "irt_2pl", 1, 1.0, 5, 0.20, (0.5, 1.5), 17))
        y_tail = cs["y"]
        y_tail[[3, 17, 31, 32, 47, 63, 64, 96]] = 255               # both person tiles of the first unit, and the second unit
        rng = np.random.RandomState(18)
        head = (rng.uniform(size=(2 * cus * 256, cs["J"])) < 0.5).astype(np.uint8)
        head[rng.uniform(size=head.shape) < 0.70] = 255
        cs.update(N=len(head) + T, y=np.concatenate([head, y_tail]), y_tail=y_tail, tail=np.arange(len(head), len(head) + T))
        _SECOND[cus] = (cs, irt_oracle(cs, y=y_tail))
    return _SECOND[cus]


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def irt_grid_loglik(model, theta, params, Dc, y):
    """ll[i][g] = log p(y_i | x = theta_g): vo.irt_loglik at every node.  params: unconstrained leaves (any float dtype)."""
    f8 = lambda v: np.asarray(v, np.float64)                        # noqa: E731
    J = y.shape[1]
    a = f8(params["a"]) if "a" in params else None
    b = f8(params["b"]).reshape(1, J)
    c = vo.sigmoid(f8(params["c"])).reshape(1, J) if model in ("irt_3pl", "irt_4pl") else None
    d = vo.sigmoid(f8(params["d"])).reshape(1, J) if model == "irt_4pl" else None
    theta = f8(theta)
    ll = np.empty((y.shape[0], theta.shape[0]))
    for g in range(theta.shape[0]):
        x = np.broadcast_to(theta[g][None, :], (y.shape[0], theta.shape[1]))
        ll[:, g] = vo.irt_loglik(model, x, a, b, c, d, Dc, y)[0]
    return ll


def cdm_grid_loglik(cdm, K, q, params, y):
    """ll[i][c] over the 2^K patterns, and (logw, coord): the clamped uniform Categorical of vo.ccdm_particle, the attribute bits."""
    q = np.asarray(q, np.float64)
    eta, attrs = (vo.dino_eta if cdm == "dino" else vo.dina_eta)(K, q)
    C = eta.shape[0]
    g_ = vo.sigmoid(np.asarray(params["g"], np.float64)).reshape(1, -1)
    s_ = vo.sigmoid(np.asarray(params["s"], np.float64)).reshape(1, -1)
    lp0, _ = vo.bernoulli_logprob_probs(np.broadcast_to(g_, y.shape).copy(), y)
    lp1, _ = vo.bernoulli_logprob_probs(np.broadcast_to(1 - s_, y.shape).copy(), y)
    ll = lp0.sum(1, keepdims=True) + (lp1 - lp0) @ eta.T
    pr = np.full(C, 1.0 / C)
    logw = np.log(np.clip(pr / pr.sum(), vo.EPS32, 1 - vo.EPS32))
    return ll, logw, attrs


def grid_posterior(ll, logw, coord):
    """loglik, mean, sd, argmax node and the gap between the best and the second-best logw + ll, per person."""
    coord = np.asarray(coord, np.float64)
    f = ll + np.asarray(logw, np.float64)[None, :]
    m = f.max(1)
    w = np.exp(f - m[:, None])
    s0 = w.sum(1)
    p = w / s0[:, None]
    mean = p @ coord
    var = (p[:, :, None] * (coord[None, :, :] - mean[:, None, :]) ** 2).sum(1)
    top = np.sort(f, axis=1)
    gap = top[:, -1] - top[:, -2] if f.shape[1] > 1 else np.full(len(f), np.inf)
    return {"loglik": m + np.log(s0), "mean": mean, "sd": np.sqrt(var), "node": f.argmax(1), "gap": gap}


def irt_oracle(cs, params=None, y=None, nodes=None):
    from vipsy_amd.engine import score_grid
    theta, logw = score_grid(cs["D"], cs["nodes"] if nodes is None else nodes, cs["span"])
    ll = irt_grid_loglik(cs["model"], theta, cs["params"] if params is None else params, cs["Dc"], cs["y"] if y is None else y)
    return grid_posterior(ll, logw, theta)


def cdm_oracle(cs, params=None, y=None):
    ll, logw, attrs = cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"] if params is None else params,
                                      cs["y"] if y is None else y)
    return grid_posterior(ll, logw, attrs)


def irt_condition(cs, want):
    """(smallest oracle PSD over persons and dimensions, half the node spacing)."""
    return float(want["sd"].min()), 0.5 * (2.0 * cs["span"] / (cs["nodes"] - 1))


def left_out(want):
    """Share of the persons whose best and second-best node are closer than ARGMAX_GAP in the float64 oracle."""
    return float((want["gap"] <= ARGMAX_GAP).mean())
