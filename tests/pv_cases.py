"""The numpy restatement of the plausible-value noise (vipsy_amd/csrc/k_grid_draw.hip, include/vipsy_amd.h: vx_grid_draw) and the
float64 oracle draws of tests/test_pv_host.py (CPU) and tests/test_gpu_pv.py (GPU).

Noise, for the person with global row r, node g and absolute draw index m:
    w = philox4x32_10(lo32(r), hi32(r), g, (PV_STREAM << 16) | (m >> 2); key lo32(seed), hi32(seed)),   x = word m & 3 of w,
    u = ((x >> 9) + 0.5) 2^-23,   noise = -log(-log(u)),
and a draw is argmax_g (f_g + noise_g) with f = logw + ll of tests/score_cases.py (ties: the lowest node, numpy's argmax).
Every oracle here is computed once and shared; callers must not modify what they get."""
import numpy as np

from oracle import vi_oracle as vo
from tests import score_cases as sc

DRAWS, SEED = 16, 7              # the oracle comparisons of both test files


def pv_stream():
    from vipsy_amd.engine import PV_STREAM
    return PV_STREAM


def lattice_u(x, dtype=np.float64):
    """uint32 words -> u on the 23-bit lattice, computed in `dtype`."""
    x = np.asarray(x, dtype=np.uint32)
    return ((x >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def words(seed, r, G, draws, draw0=0):
    """The Philox words x[i][g][k] of draw m = draw0 + k for rows r (global indices, int64) -- uint32 [len(r), G, draws]."""
    r = np.asarray(r, dtype=np.int64).astype(np.uint64)
    m = np.arange(draw0, draw0 + draws)
    q0, q1 = draw0 >> 2, (draw0 + draws - 1) >> 2
    quads = np.arange(q0, q1 + 1, dtype=np.uint32)
    c0 = (r & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    c1 = (r >> np.uint64(32)).astype(np.uint32)[:, None, None]
    c2 = np.arange(G, dtype=np.uint32)[None, :, None]
    c3 = ((np.uint32(pv_stream()) << np.uint32(16)) | quads)[None, None, :]
    w = vo.philox4x32_10(c0, c1, c2, c3, np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    allw = np.stack(w, axis=-1).reshape(len(r), G, 4 * len(quads))          # [.., 4 (quad - q0) + word]
    return allw[:, :, m - 4 * q0]


def gumbel(seed, r, G, draws, draw0=0):
    """noise[i][g][k] in float64."""
    return -np.log(-np.log(lattice_u(words(seed, r, G, draws, draw0))))


def draw(f, noise):
    """node [n, draws] = argmax_g (f + noise) and the gap between the best and the second-best perturbed value."""
    v = np.asarray(f, np.float64)[:, :, None] + noise
    node = v.argmax(1)
    if v.shape[1] > 1:
        top = np.partition(v, v.shape[1] - 2, axis=1)
        gap = top[:, -1, :] - top[:, -2, :]
    else:
        gap = np.full(node.shape, np.inf)
    return node, gap


_F = {}


def posterior_f(case):
    """(case dict, f = logw + ll float64 [N, G], coord float64 [G, D], the oracle posterior of score_cases) of an IRT or CDM
    score case, computed once."""
    if case[0] not in _F:
        if case in sc.IRT_CASES:
            from vipsy_amd.engine import score_grid
            cs = sc.irt_case(case)
            theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
            ll = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y"])
            coord = theta.astype(np.float64)
        else:
            cs = sc.cdm_case(case)
            ll, logw, coord = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], cs["y"])
        f = ll + np.asarray(logw, np.float64)[None, :]
        _F[case[0]] = (cs, f, np.asarray(coord, np.float64), sc.grid_posterior(ll, logw, coord))
    return _F[case[0]]


_D = {}


def oracle_draws(case, draws=DRAWS, seed=SEED):
    """(node [N, draws], gap [N, draws]) of a score case; rows are keyed by their index (row_offset 0).  Computed once."""
    key = (case[0], draws, seed)
    if key not in _D:
        cs, f, _, _ = posterior_f(case)
        _D[key] = draw(f, gumbel(seed, np.arange(f.shape[0]), f.shape[1], draws))
    return _D[key]


def left_out(gap):
    """Share of the (person, draw) pairs whose best two perturbed values are closer than ARGMAX_GAP in the float64 oracle."""
    return float((gap <= sc.ARGMAX_GAP).mean())
