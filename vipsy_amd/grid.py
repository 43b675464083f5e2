"""The grid family: what needs a person's posterior over a fixed set of latent nodes and no guide.  On IrtEngine (x_feature <= 3)
and CcdmEngine: score(), expected_counts() / item_fit(), fit_em(), plausible_values(), item_information() / item_se(),
residual_sums() / local_dependence(), fit_sums() / person_fit() / item_msq(), group_counts() / dif(), sumscore_tables() /
sx2() / score_table() and marginal_loglik().  On
IrtEngine alone: fit_population(), the latent regression, and the score() / plausible_values() / expected_counts() conditioned on
it (covariates=), and score_bifactor(), the exact scores of a bifactor / testlet model with any x_feature >= 2 (its structure
reader, two-axis grid and testlet layout are the bifactor_* functions below; the method itself is in engine.py).  All of it runs
on the vx_grid_* entries of the C ABI (k_grid_*.hip; no reference counterpart) and works in buffers of its own: nothing a step
reads is touched."""
from collections import namedtuple

import numpy as np
import torch

SCORE_MAX_NODES = 1024           # GP_MAXG (vipsy_amd/csrc/k_grid_post.hip)
SCORE_MAX_DIMS = 3               # IRT: the tensor-product grid stops being a method beyond three dimensions
EM_MAX_NEWTON = 64               # GM_MAX_NEWTON (vipsy_amd/csrc/k_grid_mstep.hip)
PV_MAX_DRAWS = 1024              # PV_MAXDRAWS (vipsy_amd/csrc/k_grid_draw.hip)
INFO_MAX_PARAMS = 4096           # GI_MAXP (vipsy_amd/csrc/k_grid_info.hip): columns of the information matrix
PV_STREAM = 0xC7                 # PV_STREAM (vipsy_amd/csrc/vx_common.h): the Philox stream tag of the plausible-value draws


def score_grid(D, nodes=61, span=6.0):
    """The quadrature grid of IrtEngine.score: `nodes` equally spaced points on [-span, span] in each of the D dimensions
    (tensor product, dimension 0 slowest: node g = (i_0 * nodes + i_1) * nodes + i_2 sits at (p[i_0], p[i_1], p[i_2])), weights
    proportional to exp(-|theta|^2 / 2) -- the N(0, I) prior of the model (vi.py:590) -- normalised to sum 1.
    Returns (theta float32 [G, D], logw float32 [G]); `nodes` may also be an explicit pair (theta [G, D], logw [G])."""
    D = int(D)
    if not 1 <= D <= SCORE_MAX_DIMS:
        raise ValueError("grid scores need 1 <= x_feature <= %d (got %d): a tensor-product grid of n nodes a dimension has "
                         "n**D points, and the kernel takes at most %d" % (SCORE_MAX_DIMS, D, SCORE_MAX_NODES))
    if isinstance(nodes, (tuple, list)):
        if len(nodes) != 2:
            raise ValueError("explicit nodes are a pair (theta [G, D], logw [G])")
        theta = np.asarray(nodes[0], dtype=np.float64)
        logw = np.asarray(nodes[1], dtype=np.float64).reshape(-1)
        if theta.ndim == 1 and D == 1:
            theta = theta[:, None]
        if theta.ndim != 2 or theta.shape[1] != D or theta.shape[0] != logw.shape[0]:
            raise ValueError("explicit nodes: theta must be [G, %d] and logw [G]" % D)
        if not 1 <= theta.shape[0] <= SCORE_MAX_NODES:
            raise ValueError("explicit nodes: 1 <= G <= %d" % SCORE_MAX_NODES)
        if not (np.isfinite(theta).all() and np.isfinite(logw).all()):
            raise ValueError("explicit nodes: theta and logw must be finite")
        return np.ascontiguousarray(theta, dtype=np.float32), np.ascontiguousarray(logw, dtype=np.float32)
    if isinstance(nodes, bool) or not isinstance(nodes, (int, np.integer)) or nodes < 2:
        raise ValueError("nodes must be an integer >= 2 (points per dimension) or a pair (theta, logw)")
    if not (isinstance(span, (int, float, np.floating, np.integer)) and np.isfinite(span) and span > 0):
        raise ValueError("span must be a positive finite number")
    n = int(nodes)
    if n ** D > SCORE_MAX_NODES:
        raise ValueError("%d nodes in each of %d dimensions are %d grid points; the kernel takes at most %d" %
                         (n, D, n ** D, SCORE_MAX_NODES))
    p = np.linspace(-float(span), float(span), n)
    theta = np.stack([m.reshape(-1) for m in np.meshgrid(*([p] * D), indexing="ij")], axis=1)
    lw = -0.5 * (theta ** 2).sum(axis=1)
    lw = lw - (lw.max() + np.log(np.exp(lw - lw.max()).sum()))
    return np.ascontiguousarray(theta, dtype=np.float32), np.ascontiguousarray(lw, dtype=np.float32)


BIFACTOR_MAX_GENERAL = 256       # GB_MAXGG (vipsy_amd/csrc/grid_plan.h): general nodes
BIFACTOR_MAX_SPECIFIC = 32       # GB_MAXGH: specific nodes, the rows of one tile
BIFACTOR_MAX_ITEMS = 1024        # GP_MAXJ
BIFACTOR_MAX_IMAGE = 512 << 20   # GB_MAX_IMAGE: bytes of the operand image
BIFACTOR_SLAB_BYTES = 256 << 20  # the permuted responses of one slab of persons at the most ...
BIFACTOR_SLAB_PERSONS = 262144   # ... and its persons at the most (a multiple of 256)


def bifactor_structure(free, a, model, general=0):
    """The bifactor / testlet structure of an IRT model, read from its free mask on the host: `free` and `a` [D][J] (the mask of
    the loadings and their values as they stand), `general` the index of the dimension every item may load on.  Every other
    dimension is a SPECIFIC one, and an item may be free on one of them at the most.  Returns {"general", "specific_dims" int64
    [S = D - 1] (ascending), "testlet" int64 [J] (the column of specific_dims the item loads on; -1: the general dimension alone)
    and "sizes" int64 [S] (items a specific dimension; 0 where none)}.
    NotImplementedError: irt_1pl or x_feature = 1 (no loadings to read a structure from).  ValueError: `general` out of range; an
    item that is free on two specific dimensions (the first such item is named: the model is not a bifactor -- the triangular
    default mask of x_feature >= 3 is refused here); a loading that is not free and not zero (a fixed non-zero loading on a
    second specific dimension would break the factorisation silently; pass a0 = a_free, as the reference's CFA example does)."""
    free = np.asarray(free) != 0
    a = np.asarray(a, np.float64)
    if model == "irt_1pl" or free.ndim != 2 or free.shape[0] < 2:
        raise NotImplementedError("a bifactor structure needs irt_2pl / irt_3pl / irt_4pl with x_feature >= 2 (got %s with "
                                  "x_feature = %d): there are no loadings to read it from"
                                  % (model, free.shape[0] if free.ndim == 2 else 1))
    D, J = free.shape
    if a.shape != (D, J):
        raise ValueError("free and a must both be [x_feature][items]")
    if isinstance(general, bool) or not isinstance(general, (int, np.integer)) or not 0 <= general < D:
        raise ValueError("general must be the index of a dimension, 0 .. %d" % (D - 1))
    general = int(general)
    specific = np.array([d for d in range(D) if d != general], np.int64)
    fs = free[specific]                                                          # [S][J]
    twice = np.flatnonzero(fs.sum(0) > 1)
    if twice.size:
        j = int(twice[0])
        raise ValueError("item %d is free on the specific dimensions %s: not a bifactor / testlet model with general dimension %d "
                         "(an item loads on the general dimension and on ONE specific dimension at the most; %d items do not)"
                         % (j, [int(d) for d in specific[fs[:, j]]], general, twice.size))
    fixed = np.argwhere(~free & (a != 0))
    if fixed.size:
        d, j = int(fixed[0, 0]), int(fixed[0, 1])
        raise ValueError("item %d has the fixed loading %g on dimension %d: a loading that is not free must be 0 in a bifactor "
                         "model (pass a0 = a_free); %d loadings are not" % (j, a[d, j], d, len(fixed)))
    testlet = np.where(fs.any(0), fs.argmax(0), -1).astype(np.int64)
    return {"general": general, "specific_dims": specific, "testlet": testlet,
            "sizes": np.bincount(testlet[testlet >= 0], minlength=len(specific)).astype(np.int64)}


def bifactor_grid(nodes=(61, 21), span=(6.0, 4.0)):
    """The two axes of score_bifactor: nodes = (Gg, Gh) equally spaced points on [-span[0], span[0]] for the general dimension
    and on [-span[1], span[1]] for every specific one, weights proportional to exp(-x^2 / 2) normalised to sum 1 an axis -- the
    N(0, I) prior of the model.  Gh = 1: the single point u = 0 with weight 1.  Returns float32 (theta [Gg], logw [Gg], u [Gh],
    logv [Gh]).  ValueError beyond 2 <= Gg <= 256, 1 <= Gh <= 32 or for a span that is not positive and finite;
    NotImplementedError for explicit nodes (arrays in place of the counts)."""
    if not isinstance(nodes, (tuple, list)) or len(nodes) != 2:
        raise ValueError("nodes must be a pair (general nodes, specific nodes)")
    if any(isinstance(v, (np.ndarray, torch.Tensor, list, tuple)) for v in nodes):
        raise NotImplementedError("score_bifactor with explicit nodes is not built: nodes = (Gg, Gh) points on [-span, span]")
    for name, v, lo, hi in (("general", nodes[0], 2, BIFACTOR_MAX_GENERAL), ("specific", nodes[1], 1, BIFACTOR_MAX_SPECIFIC)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("the %s nodes must be an integer in %d .. %d (got %r)" % (name, lo, hi, v))
    if not isinstance(span, (tuple, list)) or len(span) != 2 or not all(
            isinstance(s, (int, float, np.floating, np.integer)) and not isinstance(s, bool) and np.isfinite(s) and s > 0 for s in span):
        raise ValueError("span must be a pair of positive finite numbers (general, specific)")
    out = []
    for n, s in zip(nodes, span):
        p = np.linspace(-float(s), float(s), int(n)) if n > 1 else np.zeros(1)
        lw = -0.5 * p * p
        lw = lw - (lw.max() + np.log(np.exp(lw - lw.max()).sum()))
        out += [np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(lw, dtype=np.float32)]
    return tuple(out)


def bifactor_plan(testlet, specific_dims, Gg):
    """The testlet layout of the items and the operand image over it (vipsy_amd/csrc/k_grid_bifactor.hip): the testlets in the
    order of specific_dims, those without items left out, then the items that load on the general dimension alone as one
    pseudo-testlet; inside a testlet the items in their own order; every testlet padded to whole chunks of 16.  Returns `col`
    int32 [16 KC] (the item in a slot; -1: padding), `sdim` int32 [16 KC] (its specific DIMENSION of the model; -1: none),
    `tl_start` int32 [n_tl + 1] (chunk starts), `tl_column` int64 [n_tl] (the column of specific_dims behind a testlet; -1: the
    pseudo-testlet), `KC` and `image_bytes` = Gg KC 4096.  The public API puts no constraint on the order of the items: score_bifactor
    permutes the responses into this layout.  ValueError: more than 1 024 items, an image beyond 512 MB."""
    testlet = np.asarray(testlet, np.int64).reshape(-1)
    specific_dims = np.asarray(specific_dims, np.int64).reshape(-1)
    J = int(testlet.shape[0])
    if not 1 <= J <= BIFACTOR_MAX_ITEMS:
        raise ValueError("score_bifactor takes 1 .. %d items (got %d)" % (BIFACTOR_MAX_ITEMS, J))
    col, sdim, tl_start, tl_column = [], [], [0], []
    for s in list(range(len(specific_dims))) + [-1]:
        items = np.flatnonzero(testlet == s)
        if items.size == 0:
            continue
        pad = -items.size % 16
        col += items.tolist() + [-1] * pad
        sdim += [int(specific_dims[s]) if s >= 0 else -1] * items.size + [-1] * pad
        tl_start.append(len(col) // 16)
        tl_column.append(s)
    KC = len(col) // 16
    image_bytes = int(Gg) * KC * 4 * 64 * 16
    if image_bytes > BIFACTOR_MAX_IMAGE:
        raise ValueError("the operand image of %d general nodes x %d item chunks is %d MB; score_bifactor takes 512 MB at the most "
                         "(fewer general nodes)" % (Gg, KC, image_bytes >> 20))
    return {"col": np.array(col, np.int32), "sdim": np.array(sdim, np.int32), "tl_start": np.array(tl_start, np.int32),
            "tl_column": np.array(tl_column, np.int64), "KC": KC, "image_bytes": image_bytes}


def bifactor_slab_persons(KC):
    """Persons whose permuted responses ([persons][16 KC] bytes) score_bifactor holds at a time: 256 MB of them, 262 144 persons
    at the most, a multiple of 256 and at least 256.  A person's result does not depend on the slab it falls into."""
    return int(max(256, min(BIFACTOR_SLAB_PERSONS, BIFACTOR_SLAB_BYTES // (16 * int(KC)) // 256 * 256)))


class BifactorCall(namedtuple("BifactorCall", "st plan n J KC Gg Gh theta logw u logv u_np logv_np col tl_dev img fill slabs")):
    """What one call of the bifactor family works on (IrtEngine._bifactor_call): the structure `st`, the layout `plan`, n, J, KC,
    Gg, Gh, the axes on the device (theta, logw, u, logv) and on the host (u_np, logv_np), col and tl_dev (plan["col"] /
    plan["tl_start"] on the device), the operand image `img`, fill() (tabulate the parameters into it) and slabs() (yields s0, s1
    and the responses of the persons s0 .. s1 - 1 in the testlet layout)."""
    __slots__ = ()


BIFACTOR_EM_NODES = 1024         # GP_MAXG: nodes of the M-step (vipsy_amd/csrc/k_grid_mstep.hip), Gg Gh here


def bifactor_em_index(st):
    """The rows of the two-dimensional M-step of fit_em_bifactor, from bifactor_structure(): (`sd` int64 [J], the model dimension
    of the item's specific loading -- the general dimension, as a placeholder, for an item that has none; `has` bool [J], whether
    it has one)."""
    testlet = np.asarray(st["testlet"], np.int64)
    has = testlet >= 0
    sd = np.where(has, np.asarray(st["specific_dims"], np.int64)[np.where(has, testlet, 0)], int(st["general"]))
    return sd.astype(np.int64), has


def bifactor_gather(a, general, sd, has):
    """[D][J] (loadings, their free mask) -> [2][J]: row 0 the general dimension's, row 1 the item's own specific dimension's, 0
    where it has none.  torch, on a's device; sd int64 [J] and has bool [J] (bifactor_em_index) on it as well."""
    j = torch.arange(a.shape[1], device=a.device)
    return torch.stack([a[general], torch.where(has, a[sd, j], torch.zeros_like(a[general]))]).contiguous()


def bifactor_scatter(a, a2, general, sd, has):
    """bifactor_gather undone, in place: a2 [2][J] back into the two rows of a [D][J] it came from; nothing else of a is written
    (the specific rows of the other testlets stay as they are: 0)."""
    j = torch.arange(a.shape[1], device=a.device)
    a[general] = a2[0]
    a[sd[has], j[has]] = a2[1][has]
    return a


def bifactor_em_prior(prior, model, D, J, general, sd, has):
    """fit_em_bifactor's `prior` as the two-dimensional M-step takes it (em_prior with D = 2, whose rules and error texts hold): a
    prior on "a" -- (mean, sd), each a scalar or shaped like the leaf, [D][J] -- is gathered like the loadings, row 1 of
    em_prior's layout from the general dimension and row 2 from the item's own specific dimension (no prior, sd = inf, where it
    has none)."""
    if isinstance(prior, dict) and "a" in prior and isinstance(prior["a"], (tuple, list)) and len(prior["a"]) == 2:
        pair = []
        for what, v, none in (("mean", prior["a"][0], 0.0), ("sd", prior["a"][1], np.inf)):
            try:
                v = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise ValueError("prior['a']: %s must be a number or an array shaped like the leaf" % what)
            if v.shape not in ((), (D, J)):
                raise ValueError("prior['a']: %s must be a scalar or shaped like the leaf, %s (got %s)" % (what, (D, J), v.shape))
            if v.shape == (D, J):
                v = np.stack([v[general], np.where(has, v[sd, np.arange(J)], none)])
            pair.append(v)
        prior = dict(prior, a=tuple(pair))
    return em_prior(prior, model, 2, J)


EM_PRIOR_ROWS = 6                # GM_ROWS (vipsy_amd/csrc/k_grid_mstep.hip): b, a_0 .. a_2, c_un, d_un
EM_PRIOR_KEYS = {"irt_1pl": ("b",), "irt_2pl": ("a", "b"), "irt_3pl": ("a", "b", "c"), "irt_4pl": ("a", "b", "c", "d")}


def em_prior(prior, model, D, J):
    """fit_em's `prior` as vx_grid_mstep_irt_map takes it: float32 numpy [2][6][J], [0][k] the means and [1][k] the precisions
    1 / sd^2 of unknown k (0: b, 1 + d: a_d, 4: c_un, 5: d_un), zero where there is no prior.  The one place the argument is
    checked -- the C entry cannot look into device memory, so negative or non-finite precisions are refused HERE.
    prior: a dict over "a", "b", "c", "d", each (mean, sd) on the unconstrained scale of the leaves (c_un = logit c, d_un =
    logit d); mean and sd are scalars or arrays shaped like the leaf ([D][J] for a, [1][J] for the others); sd > 0, inf or an
    absent key meaning no prior.  ValueError: not a dict, an unknown key, a key the model does not have, a value that is no
    (mean, sd) pair, a wrong shape, a non-finite mean, an sd that is not > 0 -- and a 3PL without a finite sd on every item's c,
    or a 4PL without one on c and d: the likelihood alone does not identify an asymptote (the M-step is not concave in it and
    walks its logit to the clamp), so the prior is what the fit rests on."""
    keys = EM_PRIOR_KEYS[model]
    if not isinstance(prior, dict):
        raise ValueError('prior must be a dict over "a", "b", "c", "d" of (mean, sd) pairs')
    out = np.zeros((2, EM_PRIOR_ROWS, J), np.float64)
    finite = {}
    for key, value in prior.items():
        if key not in ("a", "b", "c", "d"):
            raise ValueError('prior has the unknown key %r: the keys are "a", "b", "c", "d"' % (key,))
        if key not in keys:
            raise ValueError("prior[%r]: %s has no such parameter" % (key, model))
        if not isinstance(value, (tuple, list)) or len(value) != 2:
            raise ValueError("prior[%r] must be a pair (mean, sd)" % key)
        shape = (D, J) if key == "a" else (1, J)
        pair = []
        for what, v in zip(("mean", "sd"), value):
            try:
                v = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise ValueError("prior[%r]: %s must be a number or an array shaped like the leaf" % (key, what))
            if v.shape not in ((), shape):
                raise ValueError("prior[%r]: %s must be a scalar or shaped like the leaf, %s (got %s)" % (key, what, shape, v.shape))
            pair.append(np.broadcast_to(v, shape))
        mean, sd = pair
        if not np.isfinite(mean).all():
            raise ValueError("prior[%r]: the mean must be finite" % key)
        if not (sd > 0).all():                                         # (NaN fails it too)
            raise ValueError("prior[%r]: sd must be > 0 (inf: no prior)" % key)
        with np.errstate(over="ignore", divide="ignore"):
            prec = np.where(np.isinf(sd), 0.0, 1.0 / (sd * sd)).astype(np.float32)      # (as the kernel reads it)
        if not np.isfinite(prec).all():
            raise ValueError("prior[%r]: 1 / sd^2 is not a finite float32" % key)
        lo = 1 if key == "a" else {"b": 0, "c": 4, "d": 5}[key]
        out[0, lo:lo + shape[0]] = np.where(prec > 0, mean, 0.0)
        out[1, lo:lo + shape[0]] = prec
        finite[key] = bool((prec > 0).all())
    for key, name in (("c", "guessing"), ("d", "slipping")):
        if key in keys and not finite.get(key, False):
            raise ValueError("%s needs a prior with a finite sd on %r for every item: the likelihood alone does not pin the %s "
                             "asymptote -- without a prior its logit walks to the clamp" % (model, key, name))
    return np.ascontiguousarray(out, dtype=np.float32)


def population_logw(theta, sigma):
    """The shared log-weights of the nodes under a population N(mu_i, sigma): -1/2 theta_g^T sigma^-1 theta_g, shifted so that the
    largest is 0 (the per-person normaliser is the kernel's lognorm), computed in float64, returned as float32 [G]."""
    theta = np.asarray(theta, np.float64)
    sigma = np.asarray(sigma, np.float64)
    if theta.ndim != 2 or sigma.shape != (theta.shape[1], theta.shape[1]):
        raise ValueError("theta must be [G, D] and sigma [D, D]")
    lw = -0.5 * np.einsum("gd,de,ge->g", theta, np.linalg.inv(sigma), theta)
    return np.ascontiguousarray(lw - lw.max(), dtype=np.float32)


def tri_to_full(tri, D):
    """[..., D (D + 1) / 2] upper triangle row by row (00, 01, 02, 11, 12, 22) -> the symmetric [..., D, D]."""
    iu = np.triu_indices(D)
    if isinstance(tri, torch.Tensor):
        full = tri.new_empty(tri.shape[:-1] + (D, D))
        r, c = torch.as_tensor(iu[0], device=tri.device), torch.as_tensor(iu[1], device=tri.device)
    else:
        tri = np.asarray(tri)
        full = np.empty(tri.shape[:-1] + (D, D), tri.dtype)
        r, c = iu
    full[..., r, c] = tri
    full[..., c, r] = tri
    return full


def _population_sums(X, mean, cov):
    """What the M-step needs of the persons, in float64 torch where X lives, as one flat tensor: X^T m [p][D], m^T m [D][D] and
    the sum of the persons' covariance triangles [D (D + 1) / 2]."""
    m = mean.to(torch.float64)
    # elementwise products and a column reduction, not a GEMM: see _population_em
    xtm = torch.stack([(X * m[:, d:d + 1]).sum(0) for d in range(m.shape[1])], 1)
    mtm = (m[:, :, None] * m[:, None, :]).sum(0)
    return torch.cat([xtm.reshape(-1), mtm.reshape(-1), cov.to(torch.float64).sum(0).reshape(-1)])


def _population_solve(sums, XtX_chol, n, p, D):
    """Gamma' and Sigma' from _population_sums on the host.  With X^T X Gamma' = X^T m the residual cross products are
    sum_i (m_i - Gamma'^T x_i)(m_i - Gamma'^T x_i)^T = m^T m - Gamma'^T (X^T m)."""
    sums = np.asarray(sums, np.float64)
    xtm, mtm = sums[:p * D].reshape(p, D), sums[p * D:p * D + D * D].reshape(D, D)
    csum = tri_to_full(sums[p * D + D * D:], D)
    L = np.asarray(XtX_chol, np.float64)
    gamma = np.linalg.solve(L.T, np.linalg.solve(L, xtm))
    rss = mtm - gamma.T @ xtm
    sigma = (csum + 0.5 * (rss + rss.T)) / float(n)
    return gamma, sigma


def population_mstep(X, XtX_chol, mean, cov):
    """The M-step of the latent regression theta_i ~ N(Gamma^T x_i, Sigma) from the persons' posterior means m_i and covariances
    C_i, in float64: Gamma' = (X^T X)^-1 X^T m and Sigma' = (1 / n) sum_i [C_i + (m_i - Gamma'^T x_i)(m_i - Gamma'^T x_i)^T].
    X [n][p] float64 torch (on any device: the n x p products run there), XtX_chol the lower Cholesky factor of X^T X (numpy
    [p][p]: the solve runs on the host), mean [n][D], cov [n][D (D + 1) / 2] (upper triangle row by row) torch, any float dtype.
    Returns (Gamma' [p][D], Sigma' [D][D]) as float64 numpy."""
    n, p = int(X.shape[0]), int(X.shape[1])
    D = int(mean.shape[1])
    if X.dtype != torch.float64 or mean.shape[0] != n or tuple(cov.shape) != (n, D * (D + 1) // 2):
        raise ValueError("X must be float64 [n][p], mean [n][D] and cov [n][D (D + 1) / 2]")
    return _population_solve(_population_sums(X, mean, cov).cpu().numpy(), XtX_chol, n, p, D)


def design_cholesky(X):
    """The lower Cholesky factor of X^T X (float64 numpy [p][p]) of a design X float64 torch [n][p]; ValueError naming the
    column of the failing pivot if X^T X is not positive definite (a constant column beside the intercept, collinear columns)."""
    A = torch.stack([(X * X[:, j:j + 1]).sum(0) for j in range(X.shape[1])]).cpu().numpy()      # (X^T X as _population_sums forms X^T m)
    A = 0.5 * (A + A.T)
    W = A.copy()
    for i in range(A.shape[0]):                     # the pivots: one below 1e-10 of its diagonal entry is rounding, not information
        if not W[i, i] > 1e-10 * A[i, i]:
            raise ValueError("X^T X of the %d design columns is not positive definite: pivot %.3e at column %d (the intercept, "
                             "where there is one, is column 0) -- a constant or collinear covariate" % (A.shape[0], W[i, i], i))
        W[i + 1:, i + 1:] -= np.outer(W[i + 1:, i], W[i, i + 1:]) / W[i, i]
    return np.linalg.cholesky(A)


def grid_image_prob(img, J, G):
    """P(y_j = 1 | node g), float32 [J][G], read back from the operand image of vx_grid_table_* (k_grid_post.hip: [node tile][item
    chunk][T1 head, T1 low, T0 head, T0 low][64 lanes][8 fp16], lane = node % 32 + 32 * (item % 16 // 8), values T * 2^10): the
    exponential of the very T1 the kernels multiply with, not a second evaluation of the response function."""
    KC, NT = (J + 15) // 16, (G + 31) // 32
    t = img.view(torch.float16).view(NT, KC, 4, 2, 32, 8)[:, :, 0:2].to(torch.float64)
    t1 = (t[:, :, 0] + t[:, :, 1]) / 1024.0                                   # [node tile][item chunk][item half][node][item]
    t1 = t1.permute(1, 2, 4, 0, 3).reshape(KC * 16, NT * 32)[:J, :G]
    return torch.exp(t1).to(torch.float32).contiguous()


def item_fit_stats(n1, n0, prob):
    """Per-item fit from the expected counts, in float64 on the tables' device.  With n = n1 + n0, N_j = sum_g n[j][g] and every
    sum over the nodes with n[j][g] > 0: n_obs = N_j (the persons who answered j), md = sum (n1 - n prob) / N_j, rmsd =
    sqrt(sum (n1 - n prob)^2 / n / N_j), observed = n1 / n (NaN where n = 0).  An item nobody answered: NaN, NaN, n_obs 0."""
    n1, n0, prob = n1.to(torch.float64), n0.to(torch.float64), prob.to(torch.float64)
    n = n1 + n0
    pos = n > 0
    zero = torch.zeros_like(n)
    n_obs = torch.where(pos, n, zero).sum(-1)
    safe = torch.where(pos, n, torch.ones_like(n))
    resid = torch.where(pos, n1 - n * prob, zero)
    md = resid.sum(-1) / n_obs                                                # 0 / 0 = NaN: nobody answered
    rmsd = torch.sqrt((resid * resid / safe).sum(-1) / n_obs)
    observed = torch.where(pos, n1 / safe, torch.full_like(n, float("nan")))
    return {"n_obs": n_obs, "md": md, "rmsd": rmsd, "observed": observed}


SUMSCORE_MAX_ITEMS = 1023        # SS_MAXJ (vipsy_amd/csrc/k_sumscore.hip): a score vector of Js + 1 <= 1024 entries


def grid_image_probs(img, J, G):
    """(p1, p0) = P(y_j = 1 | node g) and P(y_j = 0 | node g), float32 [J][G] each, read back from the operand image as
    grid_image_prob reads T1: the exponentials of the very T1 and T0 the kernels multiply with.  p0 comes from T0, never as
    1 - p1."""
    KC, NT = (J + 15) // 16, (G + 31) // 32
    t = img.view(torch.float16).view(NT, KC, 4, 2, 32, 8).to(torch.float64)
    out = []
    for h in (0, 2):                                                          # [T1 head, T1 low, T0 head, T0 low]
        tt = (t[:, :, h] + t[:, :, h + 1]) / 1024.0                           # [node tile][item chunk][item half][node][item]
        tt = tt.permute(1, 2, 4, 0, 3).reshape(KC * 16, NT * 32)[:J, :G]
        out.append(torch.exp(tt).to(torch.float32).contiguous())
    return out[0], out[1]


def chi2_sf(x, df):
    """The upper tail of the chi-square distribution with an integer df >= 1 at x >= 0, in closed form: for even df = 2 m
    exp(-x / 2) sum_{k < m} (x / 2)^k / k!, for odd df = 2 m + 1 erfc(sqrt(x / 2)) + sqrt(2 x / pi) exp(-x / 2) sum_{k < m} x^k /
    (1 * 3 * .. * (2 k + 1)).  The finite sum is carried with a scale of its own (rescaled whenever a term passes 1e250) and meets
    exp(-x / 2) in the exponent, so that a large statistic on many cells gives its tail -- 0 once that leaves float64 -- and never
    inf * 0.  NaN for df <= 0 or an x that is negative or not finite."""
    import math
    x, df = float(x), int(df)
    if df <= 0 or not math.isfinite(x) or x < 0:
        return float("nan")
    h = 0.5 * x
    even = df % 2 == 0
    term, total, scale = 1.0, (1.0 if even else 0.0), 0.0                       # sum = total * exp(scale)
    big, log_big = 1e250, math.log(1e250)
    for k in (range(1, df // 2) if even else range(df // 2)):
        if even:
            term *= h / k
        elif k:
            term *= x / (2 * k + 1)
        total += term
        if term > big:
            term, total, scale = term / big, total / big, scale + log_big
    if even:
        return min(1.0, math.exp(math.log(total) + scale - h))
    tail = math.erfc(math.sqrt(h))
    if total > 0 and x > 0:
        tail += math.exp(0.5 * math.log(2.0 * x / math.pi) + math.log(total) + scale - h)
    return min(1.0, tail)


def sx2_host(e1, e0, o1, n, n_params, min_expected=1.0):
    """The host layer of sx2(): Orlando & Thissen's S-X2 of every listed item from the summed-score tables, in float64 numpy.
    e1, e0 [Js][Js + 1] (the model's joint probabilities of score s with y_j = 1 / 0), o1 [Js][Js + 1] and n [Js + 1] (the
    observed counts), n_params [Js] (the free parameters of each item).  For item j the score groups s = 1 .. Js - 1, with E_s =
    e1 / (e1 + e0), are collapsed by ONE left-to-right sweep -- this project's own rule; other packages merge neighbours in other
    orders, which gives the same statistic over other cells: a cell takes groups in until both its expected counts, sum n[s] E_s and sum
    n[s] (1 - E_s) (the latter from e0, not by subtraction), reach min_expected, then closes; what remains at the right end joins
    the last closed cell, or forms the only cell.  `sx2` = sum over the cells of (O - E)^2 / E + (O - E)^2 / (N - E), `n_cells`,
    `df` = n_cells - n_params, `p` = chi2_sf(sx2, df) (NaN for df <= 0), beside `observed` = o1 / n and `expected` = E_s
    [Js][Js + 1], NaN where n[s] = 0.  A cell whose expected count is 0 adds 0 where its observed count agrees and inf where not."""
    e1, e0 = np.asarray(e1, np.float64), np.asarray(e0, np.float64)
    o1, n = np.asarray(o1, np.float64), np.asarray(n, np.float64).reshape(-1)
    n_params = np.asarray(n_params, np.int64).reshape(-1)
    Js = e1.shape[0]
    if e1.shape != (Js, Js + 1) or e0.shape != e1.shape or o1.shape != e1.shape or n.shape != (Js + 1,) or n_params.shape != (Js,):
        raise ValueError("e1, e0 and o1 must be [Js][Js + 1], n [Js + 1] and n_params [Js]")
    if isinstance(min_expected, bool) or not (isinstance(min_expected, (int, float, np.floating, np.integer))
                                              and np.isfinite(min_expected) and min_expected > 0):
        raise ValueError("min_expected must be a positive finite number")
    tot = e1 + e0
    safe = np.where(tot > 0, tot, 1.0)
    E1, E0 = e1 / safe, e0 / safe                                             # (a score the model gives no mass: 0 and 0)

    def term(O, E, F):
        with np.errstate(divide="ignore", invalid="ignore"):
            d2 = (O - E) ** 2
            return np.where(d2 > 0, d2 / E + d2 / F, 0.0)

    z = np.zeros(Js)
    run_O, run_E, run_F = z.copy(), z.copy(), z.copy()
    last_O, last_E, last_F = z.copy(), z.copy(), z.copy()
    have = np.zeros(Js, bool)
    stat, cells = z.copy(), np.zeros(Js, np.int64)
    for s in range(1, Js):
        run_O += o1[:, s]
        run_E += n[s] * E1[:, s]
        run_F += n[s] * E0[:, s]
        close = (run_E >= min_expected) & (run_F >= min_expected)
        stat += np.where(close & have, term(last_O, last_E, last_F), 0.0)
        last_O, last_E, last_F = (np.where(close, r, l) for r, l in ((run_O, last_O), (run_E, last_E), (run_F, last_F)))
        have |= close
        cells += close
        run_O, run_E, run_F = (np.where(close, 0.0, r) for r in (run_O, run_E, run_F))
    if Js >= 2:
        last_O, last_E, last_F = last_O + run_O, last_E + run_E, last_F + run_F      # (never closed: last is 0, the only cell)
        cells = np.where(have, cells, 1)
        stat += term(last_O, last_E, last_F)
    df = cells - n_params
    p = np.array([chi2_sf(x, d) for x, d in zip(stat, df)], np.float64).reshape(Js)
    nan = np.full((Js, Js + 1), np.nan)
    pos = np.broadcast_to(n > 0, (Js, Js + 1))
    observed = np.where(pos, o1 / np.where(n > 0, n, 1.0), nan)
    expected = np.where(pos, E1, nan)
    return {"sx2": stat, "df": df, "p": p, "n_cells": cells, "observed": observed, "expected": expected}


def score_table_host(dist, logw, theta):
    """The host layer of score_table(): the summed-score -> latent conversion table in float64 numpy from dist [G][Js + 1] = S(s |
    node g), logw [G] and the nodes theta [G][D].  With w_g = exp(logw[g]): `prob` [Js + 1] = sum_g w_g S(s | g), the posterior of
    the nodes given the score post = w S / prob, `eap` [Js + 1][D] = sum_g post theta_g and `psd` = the square root of sum_g post
    (theta_g - eap)^2; NaN for a score the model gives no mass."""
    dist, logw, theta = np.asarray(dist, np.float64), np.asarray(logw, np.float64).reshape(-1), np.asarray(theta, np.float64)
    if dist.ndim != 2 or theta.ndim != 2 or dist.shape[0] != logw.shape[0] or theta.shape[0] != logw.shape[0]:
        raise ValueError("dist must be [G][Js + 1], logw [G] and theta [G][D]")
    joint = np.exp(logw)[:, None] * dist
    prob = joint.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        post = joint / prob[None, :]
    eap = np.einsum("gs,gd->sd", post, theta)
    dev = theta[:, None, :] - eap[None, :, :]
    psd = np.sqrt(np.einsum("gs,gsd->sd", post, dev * dev))
    return {"score": np.arange(dist.shape[1], dtype=np.int64), "prob": prob, "eap": eap, "psd": psd}


DIF_MAX_GROUPS = 4096            # GCC_MAXSEG (vipsy_amd/csrc/k_grid_counts_cond.hip): segments of a vx_grid_counts_cond call


def group_labels(groups, n):
    """The groups of dif(): `groups`, one integer label a person ([n]; numpy, torch, or a list), -> (labels [H] as np.unique sorts
    them, order int64 [n]: the persons sorted by label, stably, and seg_start int64 [H + 1]: group h holds the batch positions
    seg_start[h] .. seg_start[h + 1] of that order).  ValueError for labels that are not integers, a wrong length, fewer than two
    groups or more than DIF_MAX_GROUPS."""
    g = groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
    if g.dtype.kind not in "iu":
        raise ValueError("groups must be integer labels, one a person (got dtype %s)" % g.dtype)
    g = g.reshape(-1)
    if g.shape[0] != n:
        raise ValueError("groups has %d labels, the scored rows are %d" % (g.shape[0], n))
    labels, inv = np.unique(g, return_inverse=True)
    H = int(labels.shape[0])
    if not 2 <= H <= DIF_MAX_GROUPS:
        raise ValueError("dif needs 2 .. %d groups (got %d)" % (DIF_MAX_GROUPS, H))
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable").astype(np.int64)
    seg_start = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.bincount(inv, minlength=H)).astype(np.int64)])
    return labels, order, seg_start


def group_fit_stats(n1, n0, prob, min_obs=8):
    """item_fit_stats a group: n1, n0 [H][J][G] against the pooled prob [J][G] -> `n_obs`, `md`, `rmsd` [H][J] and `observed`
    [H][J][G], float64 on the tables' device; md and rmsd NaN where fewer than min_obs persons of the group answered the item."""
    s = item_fit_stats(n1, n0, prob)
    few = torch.round(s["n_obs"]) < min_obs
    nan = torch.full_like(s["md"], float("nan"))
    s["md"], s["rmsd"] = torch.where(few, nan, s["md"]), torch.where(few, nan, s["rmsd"])
    return s


def group_fit_top(rmsd, top=20):
    """The `top` finite cells of rmsd [H][J] by descending value (ties: the lower cell first), as `group` (the index into labels),
    `item` (int64) and `value`."""
    rmsd = np.asarray(rmsd, np.float64)
    flat = rmsd.reshape(-1)
    fin = np.flatnonzero(np.isfinite(flat))
    sel = fin[np.argsort(-flat[fin], kind="stable")[:top]]
    return {"group": (sel // rmsd.shape[1]).astype(np.int64), "item": (sel % rmsd.shape[1]).astype(np.int64), "value": flat[sel]}


def item_se_host(info, gradient, free, names=None, precision=None):
    """The host layer of item_se(): standard errors from an information matrix, in float64 numpy.  info [P][P], gradient [P],
    free bool [P].  Kept are the free columns whose diagonal is not exactly 0 (a column of exact zeros belongs to an item nobody
    answered or to a class no pattern reaches); the kept block is inverted through its Cholesky factor -- no pseudo-inverse: a
    block that is not positive definite raises ValueError naming the parameter of the smallest pivot (names: a function of the
    dense column, by default the column number).  Returns `se` [P] (NaN where fixed or dropped), `cov` [kept][kept], `kept`,
    `gradient_max` = max |gradient| over the kept columns and `condition`, the 2-norm condition number of the kept block.
    precision [P] (item_se(prior=): the precisions of the normal priors, >= 0): the block that is inverted is then
    info[kept, kept] + diag(precision[kept]) -- the likelihood's information plus the prior's curvature -- and `gradient` is taken
    as handed over (the caller adds the prior's share).  `kept` is still decided on the diagonal of `info` alone: about an item
    nobody answered the data say nothing, and it stays NaN under any prior.  precision None: every bit as without the argument."""
    info = np.asarray(info, np.float64)
    gradient = np.asarray(gradient, np.float64).reshape(-1)
    free = np.asarray(free, bool).reshape(-1)
    P = info.shape[0]
    if info.shape != (P, P) or gradient.shape != (P,) or free.shape != (P,):
        raise ValueError("info must be [P][P], gradient and free [P]")
    kept = np.flatnonzero(free & (np.diag(info) != 0))
    A = info[np.ix_(kept, kept)]
    A = 0.5 * (A + A.T)
    if precision is not None:
        precision = np.asarray(precision, np.float64).reshape(-1)
        if precision.shape != (P,) or not (np.isfinite(precision).all() and (precision >= 0).all()):
            raise ValueError("precision must be [P], finite and >= 0")
        A = A + np.diag(precision[kept])
    se = np.full(P, np.nan)
    if kept.size == 0:
        return {"se": se, "cov": np.zeros((0, 0)), "kept": kept, "gradient_max": 0.0, "condition": float("nan")}
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        W, piv = A.copy(), np.full(kept.size, np.inf)
        for i in range(kept.size):                                              # the pivots up to the first that is not positive
            piv[i] = W[i, i]
            if not piv[i] > 0:
                break
            W[i + 1:, i + 1:] -= np.outer(W[i + 1:, i], W[i, i + 1:]) / piv[i]
        worst = int(np.argmin(piv))
        col = int(kept[worst])
        raise ValueError("the information matrix of the %d estimated parameters is not positive definite: pivot %.3e at %s -- "
                         "too few persons for the parameters, or parameters the data cannot tell apart; no standard errors"
                         % (kept.size, piv[worst], names(col) if names else "column %d" % col))
    Li = np.linalg.solve(L, np.eye(kept.size))
    cov = Li.T @ Li
    se[kept] = np.sqrt(np.diag(cov))
    w = np.linalg.eigvalsh(A)
    return {"se": se, "cov": cov, "kept": kept, "gradient_max": float(np.abs(gradient[kept]).max()),
            "condition": float(w[-1] / w[0])}


def pair_q3_host(n, s, ss, sp, min_pairs=8):
    """The host layer of local_dependence(): Yen's Q3 from the four pairwise-complete tables [J][J] (n[j][k] the persons who answered
    both, s / ss the sums of the ROW item's residuals and their squares over them, sp the sum of the products), in float64 numpy:
    cov = sp - s s^T / n, v = ss - s^2 / n, q3 = cov / sqrt(v v^T) -- the correlation of the two items' residuals over the persons
    who answered both.  NaN where n < min_pairs or where either v <= 0 (an item nobody answered, or residuals without spread);
    the diagonal is exactly 1 where defined."""
    n, s, ss, sp = (np.asarray(t, np.float64) for t in (n, s, ss, sp))
    J = n.shape[0]
    if n.ndim != 2 or any(t.shape != (J, J) for t in (n, s, ss, sp)):
        raise ValueError("n, s, ss and sp must be [J][J]")
    safe = np.where(n > 0, n, 1.0)
    cov = sp - s * s.T / safe
    v = ss - s * s / safe
    ok = (n >= min_pairs) & (v > 0) & (v.T > 0)
    q3 = np.full((J, J), np.nan)
    q3[ok] = cov[ok] / np.sqrt((v * v.T)[ok])
    d = np.arange(J)
    q3[d, d] = np.where(ok[d, d], 1.0, np.nan)
    return q3


def pair_q3_summary(q3, top=20):
    """`mean` of the finite off-diagonal entries of q3, `max` of the off-diagonal q3 - mean, and the `top` pairs j < k by
    descending |q3 - mean| (ties: the lower pair first) as `item_j`, `item_k` (int64) and `value` = their q3.  No finite pair:
    mean and max NaN, no pairs."""
    J = q3.shape[0]
    jj, kk = np.triu_indices(J, 1)
    val = q3[jj, kk]
    fin = np.isfinite(val)
    jj, kk, val = jj[fin], kk[fin], val[fin]
    if val.size == 0:
        e = np.zeros(0, np.int64)
        return {"mean": float("nan"), "max": float("nan"), "item_j": e, "item_k": e.copy(), "value": np.zeros(0)}
    mean = float(val.mean())
    order = np.argsort(-np.abs(val - mean), kind="stable")[:top]
    return {"mean": mean, "max": float((val - mean).max()), "item_j": jj[order].astype(np.int64),
            "item_k": kk[order].astype(np.int64), "value": val[order]}


PAIR_TABLES = ("n11", "n10", "n01", "n00")                       # the tables of vx_pair_tables, in its argument order


def _phi_2x2(t11, t10, t01, t00):
    """phi of a 2 x 2 table, (t11 t00 - t10 t01) / sqrt(the product of the two row and the two column margins); NaN where a
    margin is not positive."""
    den = ((t11 + t10) * (t11 + t01)) * ((t01 + t00) * (t10 + t00))         # (an order a transposition leaves as it is)
    ok = den > 0
    return np.where(ok, (t11 * t00 - t10 * t01) / np.sqrt(np.where(ok, den, 1.0)), np.nan)


def pair_x2_host(n11, n10, n01, n00, p1, p0, logw, min_pairs=8, min_expected=1.0):
    """The host layer of ld_x2(): Chen & Thissen's (1997) LD X2 and G2 of every item pair, in float64 numpy, from the observed
    2 x 2 tables n_ab [J][J] (vx_pair_tables: the persons who answered both items, a to the row item and b to the column item)
    and the model's p1, p0 [J][G] = P(y_j = 1 | node g), P(y_j = 0 | node g) with the log-weights logw [G] of the nodes.
    Expected: w = softmax(logw), e_ab[j][k] = sum_g w_g p_a[j][g] p_b[k][g], the four divided by their sum (p0 is given, not
    1 - p1), E_ab = N_jk e_ab with N_jk = the sum of the four observed cells.  e10 is computed and e01 is its transpose; e11 and
    e00 are made symmetric, so every statistic is symmetric bit for bit.
    `x2` = sum_ab (O - E)^2 / E, `g2` = 2 sum_ab O ln(O / E) (0 ln 0 = 0), `z` = (x2 - 1) / sqrt 2, `p` = chi2_sf(x2, 1) = erfc(sqrt(x2 / 2)): NaN
    where j = k, where N_jk < min_pairs and where any E_ab < min_expected.  `phi_obs`, `phi_exp` = phi of the observed and of the
    expected table (NaN where a margin is 0), `sign` = sign(phi_obs - phi_exp): +1 the pair agrees more than the model says, -1
    less; 0 where either phi is undefined and wherever x2 is NaN.  `n_pairs` = N int64 [J][J], `expected` = E [2][2][J][J],
    indexed [a][b]."""
    O = {ab: np.asarray(t, np.float64) for ab, t in (((1, 1), n11), ((1, 0), n10), ((0, 1), n01), ((0, 0), n00))}
    p1, p0 = np.asarray(p1, np.float64), np.asarray(p0, np.float64)
    J = O[1, 1].shape[0]
    if O[1, 1].ndim != 2 or any(t.shape != (J, J) for t in O.values()):
        raise ValueError("n11, n10, n01 and n00 must be [J][J]")
    if p1.ndim != 2 or p1.shape[0] != J or p0.shape != p1.shape:
        raise ValueError("p1 and p0 must be [J][G]")
    lw = np.asarray(logw, np.float64).reshape(-1)
    if lw.shape[0] != p1.shape[1]:
        raise ValueError("logw must be [G]")
    for name, v in (("min_pairs", min_pairs), ("min_expected", min_expected)):
        if isinstance(v, bool) or not (isinstance(v, (int, float, np.floating, np.integer)) and np.isfinite(v) and v > 0):
            raise ValueError("%s must be a positive finite number" % name)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    e11, e00, e10 = (p1 * w) @ p1.T, (p0 * w) @ p0.T, (p1 * w) @ p0.T
    e = {(1, 1): 0.5 * (e11 + e11.T), (0, 0): 0.5 * (e00 + e00.T), (1, 0): e10, (0, 1): e10.T}
    tot = (e[1, 1] + e[0, 0]) + (e[1, 0] + e[0, 1])
    N = (O[1, 1] + O[0, 0]) + (O[1, 0] + O[0, 1])
    E = {ab: N * (e[ab] / tot) for ab in e}

    def x2_term(ab):
        with np.errstate(divide="ignore", invalid="ignore"):
            d2 = (O[ab] - E[ab]) ** 2
            return np.where(d2 > 0, d2 / E[ab], 0.0)

    def g2_term(ab):
        with np.errstate(divide="ignore", invalid="ignore"):
            pos = O[ab] > 0
            return np.where(pos, O[ab] * np.log(np.where(pos, O[ab], 1.0) / E[ab]), 0.0)

    # (11 + 00) + (10 + 01): the order that a transposition leaves as it is
    x2 = (x2_term((1, 1)) + x2_term((0, 0))) + (x2_term((1, 0)) + x2_term((0, 1)))
    g2 = 2.0 * ((g2_term((1, 1)) + g2_term((0, 0))) + (g2_term((1, 0)) + g2_term((0, 1))))
    bad = np.eye(J, dtype=bool) | (N < min_pairs)
    for ab in E:
        bad |= ~(E[ab] >= min_expected)
    x2, g2 = np.where(bad, np.nan, x2), np.where(bad, np.nan, g2)
    # chi2_sf(x, 1) = erfc(sqrt(x / 2)), for all pairs at once
    p = np.where(bad, np.nan, torch.erfc(torch.from_numpy(np.sqrt(0.5 * np.where(bad, 0.0, x2)))).numpy())
    phi_obs = _phi_2x2(O[1, 1], O[1, 0], O[0, 1], O[0, 0])
    phi_exp = _phi_2x2(e[1, 1], e[1, 0], e[0, 1], e[0, 0])
    with np.errstate(invalid="ignore"):
        sign = np.where(bad | ~np.isfinite(phi_obs) | ~np.isfinite(phi_exp), 0.0, np.sign(phi_obs - phi_exp))
    return {"x2": x2, "g2": g2, "z": (x2 - 1.0) / np.sqrt(2.0), "p": p, "sign": sign, "phi_obs": phi_obs, "phi_exp": phi_exp,
            "n_pairs": np.rint(N).astype(np.int64), "expected": np.stack([np.stack([E[0, 0], E[0, 1]]), np.stack([E[1, 0], E[1, 1]])])}


def pair_x2_top(x2, sign, top=20):
    """The `top` pairs j < k by descending x2 (ties: the lower pair first) as `item_j`, `item_k` (int64), `value` = their x2 and
    `sign`; pairs without a statistic (NaN) are not listed."""
    J = x2.shape[0]
    jj, kk = np.triu_indices(J, 1)
    val = x2[jj, kk]
    fin = np.isfinite(val)
    jj, kk, val = jj[fin], kk[fin], val[fin]
    order = np.argsort(-val, kind="stable")[:top]
    return {"item_j": jj[order].astype(np.int64), "item_k": kk[order].astype(np.int64), "value": val[order],
            "sign": np.asarray(sign)[jj[order], kk[order]]}


PERSON_SUMS = ("n", "l0", "e", "v", "sr2", "sw", "sz2")          # the rows of vx_grid_fit_*'s `person` ...
ITEM_SUMS = ("n", "sr2", "sw", "sz2")                            # ... and of its `item`


def _msq(n, sr2, sw, sz2):
    """outfit = sz2 / n and infit = sr2 / sw in float64, NaN where n = 0 or sw <= 0."""
    n, sr2, sw, sz2 = (np.asarray(t, np.float64) for t in (n, sr2, sw, sz2))
    outfit, infit = np.full(n.shape, np.nan), np.full(n.shape, np.nan)
    ok = n > 0
    outfit[ok] = sz2[ok] / n[ok]
    ok = ok & (sw > 0)
    infit[ok] = sr2[ok] / sw[ok]
    return infit, outfit


def person_fit_host(person):
    """The host layer of person_fit(): from the seven sums of a person's answered items ({n, l0, e, v, sr2, sw, sz2}, each
    [persons]), in float64 numpy: `lz` = (l0 - e) / sqrt(v), the standardised log-likelihood of Drasgow, Levine and Williams
    (e and v are the mean and the variance of l0 under the model at the estimate), `outfit` = sz2 / n, the mean squared
    standardised residual, and `infit` = sr2 / sw, the information-weighted one.  NaN where the person answered nothing
    (n = 0) or where v <= 0 (lz) / sw <= 0 (infit)."""
    s = {k: np.asarray(person[k], np.float64) for k in PERSON_SUMS}
    if any(v.ndim != 1 or v.shape != s["n"].shape for v in s.values()):
        raise ValueError("the person sums must be vectors of one length")
    lz = np.full(s["n"].shape, np.nan)
    ok = (s["n"] > 0) & (s["v"] > 0)
    lz[ok] = (s["l0"][ok] - s["e"][ok]) / np.sqrt(s["v"][ok])
    infit, outfit = _msq(s["n"], s["sr2"], s["sw"], s["sz2"])
    return {"lz": lz, "infit": infit, "outfit": outfit}


def item_msq_host(item):
    """The host layer of item_msq(): `infit` = sr2 / sw and `outfit` = sz2 / n from the four sums over the persons who answered
    an item ({n, sr2, sw, sz2}, each [items]), float64 numpy; NaN for an item nobody answered (n = 0) or with sw <= 0."""
    s = {k: np.asarray(item[k], np.float64) for k in ITEM_SUMS}
    if any(v.ndim != 1 or v.shape != s["n"].shape for v in s.values()):
        raise ValueError("the item sums must be vectors of one length")
    infit, outfit = _msq(s["n"], s["sr2"], s["sw"], s["sz2"])
    return {"infit": infit, "outfit": outfit}


POINT_METHODS = {"ml": 0, "map": 1, "wle": 2}                    # VX_POINT_ML / _MAP / _WLE (include/vipsy_amd.h)
POINT_STATUS = ("converged", "at_bound", "max_iter", "singular", "empty")        # the names of vx_grid_point_irt's status codes
POINT_CONVERGED, POINT_AT_BOUND, POINT_MAX_ITER, POINT_SINGULAR, POINT_EMPTY = range(5)
POINT_MAX_ITERS = 255            # GPT_MAX_ITERS (vipsy_amd/csrc/k_grid_point.hip)
POINT_STEP_CAP = 1.0             # the largest component of a Fisher-scoring step
POINT_AT = ("eap",) + tuple(POINT_METHODS)                       # what the diagnostics take as at=


def point_estimates_host(theta_hat, info_tri, status, iterations, method):
    """The host layer of point_estimates(): from vx_grid_point_irt's theta_hat (n, D) float32, info_tri [D (D + 1) / 2][n] (the
    upper triangle of the likelihood's information at theta_hat), status and iterations (n,), in float64 numpy: `info` (n, D, D),
    `cov` = M^-1 with M = info (+ the unit matrix for method "map", the N(0, I) prior), `se` = the square roots of its diagonal,
    `n_converged` and the person separation `reliability` (D,) = 1 - mean(se^2) / var(theta_hat) over the persons with status
    `converged` (var with n - 1; NaN with fewer than two of them).  cov and se are NaN where status is `empty` or `singular`, or
    where M is not positive definite."""
    th = np.asarray(theta_hat)
    n, D = th.shape
    status = np.asarray(status).astype(np.int32)
    info = tri_to_full(np.asarray(info_tri, np.float64).T, D)
    M = info + (np.eye(D) if method == "map" else 0.0)
    cov = np.full((n, D, D), np.nan)
    ok = (status != POINT_EMPTY) & (status != POINT_SINGULAR) & np.isfinite(M).all((1, 2))
    if D == 1:                                                                  # (a million persons: no batched LAPACK for 1 x 1)
        ok &= M[:, 0, 0] > 0
        cov[ok, 0, 0] = 1.0 / M[ok, 0, 0]
    else:
        for d in range(D):                                                      # positive definite: every leading minor
            ok &= np.linalg.det(np.where(ok[:, None, None], M, np.eye(D))[:, :d + 1, :d + 1]) > 0
        if ok.any():
            cov[ok] = np.linalg.inv(M[ok])
    se = np.sqrt(np.diagonal(cov, axis1=1, axis2=2)).copy()
    conv = status == POINT_CONVERGED
    rel = np.full(D, np.nan)
    if conv.sum() >= 2:
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = 1.0 - (se[conv] ** 2).mean(0) / th[conv].astype(np.float64).var(0, ddof=1)
    return {"theta_hat": th, "se": se, "cov": cov, "info": info, "status": status,
            "iterations": np.asarray(iterations).astype(np.int32), "n_converged": int(conv.sum()), "reliability": rel}


class GridCall(namedtuple("GridCall", "y rows J theta logw fill_tables cfg")):
    """What an engine's `_grid_call` hands to the grid kernels: the responses y ([n][J] u8 on the device) and the rows of them to
    score (int64 on the device, or None: all), the nodes theta [G][D] with their log-weights logw [G], fill_tables(img), which
    tabulates the item parameters into an operand image, and the cfg those tables are built from, which the M-step of the same
    engine takes: a vx_irt_cfg from IrtEngine, a vx_hodina_cfg from CcdmEngine."""
    n = property(lambda c: int(c.y.shape[0]) if c.rows is None else int(c.rows.numel()))
    G = property(lambda c: int(c.theta.shape[0]))
    D = property(lambda c: int(c.theta.shape[1]))


class GridMixin(object):
    """The grid methods of an engine class that brings `_grid_call(y_u8, rows, ..., params=None)` -> GridCall: its nodes and how
    its item parameters become tables (IrtEngine, CcdmEngine)."""

    @staticmethod
    def _int_in(name, value, lo, hi=None, says=None):
        """value as an int, refused unless it is an integer (no bool) in lo .. hi (hi None: no upper end); says: the range in words."""
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
            raise ValueError("%s must be an integer %s" % (name, says or (">= %d" % lo if hi is None else "in %d .. %d" % (lo, hi))))
        return int(value)

    def _one_rank_only(self, message):
        if self.group is not None and torch.distributed.get_world_size(self.group) > 1:
            raise NotImplementedError(message)

    def _em_refusals(self, max_iter, newton):
        """What every fit_em refuses before it looks at the model."""
        self._one_rank_only("fit_em over a process group: the expected counts are the local shard's sums and the cross-rank sum "
                            "is not built (one rank refits; the other ranks copy its item parameters)")
        self._int_in("max_iter", max_iter, 1)
        self._int_in("newton", newton, 1, EM_MAX_NEWTON,
                     "in 1 .. %d (Newton steps of an item inside one M-step launch)" % EM_MAX_NEWTON)

    def _score_inputs(self, y_u8, rows, J):
        """The responses a score call reads ([n][J] u8 on the device, the training responses by default) and its rows."""
        if y_u8 is None:
            y = self.y if self.y.shape[1] == J else self.y[:, :J].contiguous()      # (without the phantom items)
        else:
            y = torch.as_tensor(y_u8)
            if y.dtype != torch.uint8 or y.dim() != 2:
                raise ValueError("responses must be a uint8 matrix (0 / 1 / 255 = missing)")
            if y.shape[1] != J:
                raise ValueError("responses have %d items, the model has %d" % (y.shape[1], J))
            y = y.to(self.dev).contiguous()
        if y.shape[0] < 1:
            raise ValueError("no persons to score")
        if rows is not None:
            rows = torch.as_tensor(rows).to(device=self.dev, dtype=torch.int64).reshape(-1).contiguous()
            if rows.numel() < 1:
                raise ValueError("no persons to score")
            if int(rows.min()) < 0 or int(rows.max()) >= y.shape[0]:
                raise IndexError("rows must index the %d response rows" % y.shape[0])
        return y, rows

    def _grid_image(self, call):
        """The operand image of a call, with its tables in it."""
        img = torch.empty(self.be.grid_image_bytes(call.J, call.G), dtype=torch.uint8, device=self.dev)
        call.fill_tables(img)
        return img

    def _grid_posterior(self, call):
        """Tables and the posterior kernel: loglik [n], mean, sd [n][D], node [n], and the image they came from."""
        n, D = call.n, call.D
        img = self._grid_image(call)
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {"loglik": torch.empty(n, **f32), "mean": torch.empty(n, D, **f32), "sd": torch.empty(n, D, **f32),
               "node": torch.empty(n, dtype=torch.int32, device=self.dev)}
        self.be.grid_posterior(call.y, call.rows, n, call.J, call.G, D, img, call.logw, call.theta, out["loglik"], out["mean"],
                               out["sd"], out["node"])
        out["img"] = img
        return out

    def _draw_args(self, draws, seed):
        """What every plausible_values refuses before it looks at the data."""
        return self._int_in("draws", draws, 1, PV_MAX_DRAWS), self._int_in("seed", seed, 0, 2 ** 64 - 1, "in 0 .. 2**64 - 1")

    def _grid_draws(self, call, draws, seed, row_offset):
        """Tables and the draw kernel (vx_grid_draw: Gumbel-max over the nodes, Philox noise keyed by (seed, row_offset + row,
        node, draw)).  Returns (node int32 [n, draws], coord float32 [n, draws, D] = theta[node], gathered on the device)."""
        img = self._grid_image(call)
        node = torch.empty(call.n, draws, dtype=torch.int32, device=self.dev)
        self.be.grid_draw(call.y, call.rows, call.n, call.J, call.G, img, call.logw, seed, row_offset, 0, draws, draws, node)
        return node, call.theta[node.long()]

    def _grid_posterior_cond(self, call, tilt, img=None, out=None):
        """Tables (unless img holds them) and the conditioned posterior kernel under call.logw and a tilt a person ([n][D] float32,
        by batch position): logjoint, lognorm [n], mean [n][D], cov [n][D (D + 1) / 2], node [n], and the image."""
        n, D = call.n, call.D
        if img is None:
            img = self._grid_image(call)
        if out is None:
            f32 = dict(dtype=torch.float32, device=self.dev)
            out = {"logjoint": torch.empty(n, **f32), "lognorm": torch.empty(n, **f32), "mean": torch.empty(n, D, **f32),
                   "cov": torch.empty(n, D * (D + 1) // 2, **f32), "node": torch.empty(n, dtype=torch.int32, device=self.dev)}
        self.be.grid_posterior_cond(call.y, call.rows, n, call.J, call.G, D, img, call.logw, call.theta, tilt, out["logjoint"],
                                    out["lognorm"], out["mean"], out["cov"], out["node"])
        out["img"] = img
        return out

    def _grid_draws_cond(self, call, tilt, draws, seed, row_offset):
        """_grid_draws under call.logw and a tilt a person (vx_grid_draw_cond): the noise goes by the row, the tilt by the batch
        position."""
        img = self._grid_image(call)
        node = torch.empty(call.n, draws, dtype=torch.int32, device=self.dev)
        self.be.grid_draw_cond(call.y, call.rows, call.n, call.J, call.G, call.D, img, call.logw, call.theta, tilt, seed, row_offset,
                               0, draws, draws, node)
        return node, call.theta[node.long()]

    def _design(self, covariates, n_rows, intercept, p=None):
        """covariates [n_rows][p'] -> the design X float64 [n_rows][p] on the device, a column of ones in front where intercept."""
        X = torch.as_tensor(covariates)
        if X.dim() == 1:
            X = X[:, None]
        if X.dim() != 2 or not (X.dtype.is_floating_point or X.dtype in (torch.int32, torch.int64, torch.uint8, torch.bool)):
            raise ValueError("covariates must be a numeric matrix [persons][p]")
        X = X.to(device=self.dev, dtype=torch.float64)
        if int(X.shape[0]) != n_rows:
            raise ValueError("covariates have %d rows, the responses %d" % (X.shape[0], n_rows))
        if intercept:
            X = torch.cat([torch.ones(n_rows, 1, dtype=torch.float64, device=self.dev), X], 1)
        if p is not None and int(X.shape[1]) != p:
            raise ValueError("the population was fitted on %d design columns (intercept %s), these covariates give %d"
                             % (p, "included" if intercept else "not used", X.shape[1]))
        if not bool(torch.isfinite(X).all()):
            raise ValueError("covariates must be finite")
        return X.contiguous()

    @staticmethod
    def _population_check(sigma, spacing):
        """The refusal of a Sigma the grid cannot resolve, before anything is computed from it: a diagonal entry below (half the
        node spacing)^2, or -- for D > 1, where the diagonal can stay healthy while a correlation runs to +-1 -- a smallest
        eigenvalue at or below 1e-6 of the largest: Lambda = Sigma^-1 then has entries a million times the scale of the problem,
        and the float32 log-weights and tilts built from it carry nothing."""
        lim = (0.5 * spacing) ** 2
        ev = np.linalg.eigvalsh(0.5 * (sigma + sigma.T)) if np.isfinite(sigma).all() else np.full(1, np.nan)
        if not np.isfinite(sigma).all() or (np.diag(sigma) < lim).any() or not ev[0] > 1e-6 * ev[-1]:
            raise ValueError("the population covariance collapses: diag(Sigma) = %s fell below (half the node spacing)^2 = %.3e, or "
                             "Sigma is singular (eigenvalues %s) -- the grid cannot resolve such a population (more nodes, or a "
                             "test that measures every dimension)" % (np.diag(sigma), lim, ev))

    @staticmethod
    def _population_reach(mu_max, sigma, span):
        """The refusal of a population that leaves the grid."""
        reach = np.asarray(mu_max, np.float64) + 4.0 * np.sqrt(np.diag(sigma))
        if (reach > span).any():
            raise ValueError("the population leaves the grid: max_i |mu_id| + 4 sqrt(Sigma_dd) = %s exceeds span = %g -- raise span "
                             "(and nodes with it)" % (reach, span))

    def _population_em(self, call, X, chol, spacing, span, max_iter, tol, progress):
        """The EM iterations of fit_population over a call whose tables stay fixed: logw and tilt = X Gamma Lambda of the
        parameters as they stand, vx_grid_posterior_cond, the sum of logjoint - lognorm (as marginal_loglik sums), and the
        sums of the M-step on the device; the p x p solve runs on the host.  Every buffer, on the device and pinned on the host,
        is made once, before the loop, and an iteration writes into them (out=): it allocates nothing on the device.  The
        parameters of an iteration (logw, Gamma, Lambda) go up in ONE asynchronous copy out of a pinned staging buffer, and its
        results (the log-likelihood, max |mu|, X^T m, m^T m, the sum of the covariance triangles) come back in ONE copy into a
        pinned buffer, behind which the host waits: the one host sync of an iteration."""
        be, dev, n, D, p, G = self.be, self.dev, call.n, call.D, int(X.shape[1]), call.G
        T = D * (D + 1) // 2
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        img = self._grid_image(call)                                             # (the item parameters are fixed: filled once)
        out = {"logjoint": torch.empty(n, **f32), "lognorm": torch.empty(n, **f32), "mean": torch.empty(n, D, **f32),
               "cov": torch.empty(n, T, **f32), "node": torch.empty(n, dtype=torch.int32, device=dev)}
        diff, tilt, logw = torch.empty(n, **f32), torch.empty(n, D, **f32), torch.empty(G, **f32)
        total, sum_ws = torch.empty(1, **f32), torch.empty(1024, **f32)          # vx_sum_workspace_floats(); not the step's
        # up: [logw G | Gamma p D | Lambda D D]; down: [loglik 1 | max |mu| D | (X^T m)^T D p | m^T m D D | sum C T]
        up_h = torch.empty(G + p * D + D * D, dtype=torch.float64).pin_memory()
        up = torch.empty(G + p * D + D * D, **f64)
        down_h = torch.empty(1 + D + D * p + D * D + T, dtype=torch.float64).pin_memory()
        down = torch.empty(1 + D + D * p + D * D + T, **f64)
        up_np, down_np = up_h.numpy(), down_h.numpy()
        gam_d, lam_d = up[G:G + p * D].view(p, D), up[G + p * D:].view(D, D)
        mumax_d, xtm_d = down[1:1 + D], down[1 + D:1 + D + D * p].view(D, p)
        mtm_d, csum_d = down[1 + D + D * p:1 + D + D * p + D * D].view(D, D), down[1 + D + D * p + D * D:]
        mu, work, m64, c64 = torch.empty(n, D, **f64), torch.empty(n, D, **f64), torch.empty(n, D, **f64), torch.empty(n, T, **f64)
        xw = torch.empty(n, p, **f64)
        theta64 = call.theta.cpu().numpy().astype(np.float64)
        cond = call._replace(logw=logw)
        stream = torch.cuda.current_stream(dev)

        def mu_into():
            """mu = X Gamma and max_i |mu_id| (into the results buffer) of the Gamma that has gone up."""
            torch.matmul(X, gam_d, out=mu)
            torch.abs(mu, out=work)
            torch.amax(work, 0, out=mumax_d)

        gamma, sigma = np.zeros((p, D)), np.eye(D)
        bar = None
        if progress:
            try:
                from tqdm import trange
                bar = trange(max_iter)
            except Exception:  # pragma: no cover
                bar = None
        hist, converged = [], False
        for _ in range(max_iter):
            self._population_check(sigma, spacing)                               # (before Sigma is inverted)
            lam = np.linalg.inv(sigma)
            lw = -0.5 * np.einsum("gd,de,ge->g", theta64, lam, theta64)
            up_np[:G], up_np[G:G + p * D], up_np[G + p * D:] = lw - lw.max(), gamma.reshape(-1), lam.reshape(-1)
            up.copy_(up_h, non_blocking=True)
            logw.copy_(up[:G])                                                   # (float64 -> float32: population_logw's rounding)
            mu_into()
            torch.matmul(mu, lam_d, out=work)
            tilt.copy_(work)
            self._grid_posterior_cond(cond, tilt, img, out)
            torch.sub(out["logjoint"], out["lognorm"], out=diff)
            be.sum_into(diff, n, 1.0, total, sum_ws)
            down[0:1].copy_(total)
            # the M-step's sums as elementwise products and column reductions: a float64 GEMM whose inner dimension is the
            # persons and whose outer ones are 1 .. 8 takes 20 ms at a million persons where these take 0.04
            m64.copy_(out["mean"])
            c64.copy_(out["cov"])
            for d in range(D):
                torch.mul(X, m64[:, d:d + 1], out=xw)
                torch.sum(xw, 0, out=xtm_d[d])
                torch.mul(m64, m64[:, d:d + 1], out=work)
                torch.sum(work, 0, out=mtm_d[d])
            torch.sum(c64, 0, out=csum_d)
            down_h.copy_(down, non_blocking=True)
            stream.synchronize()                                                 # the iteration's one host sync
            self._population_reach(down_np[1:1 + D], sigma, span)                # (of the parameters this iteration started from)
            sums = np.concatenate([down_np[1 + D:1 + D + D * p].reshape(D, p).T.reshape(-1), down_np[1 + D + D * p:]])
            hist.append(float(down_np[0]))
            gamma, sigma = _population_solve(sums, chol, n, p, D)
            if bar is not None:
                bar.update(1)
                bar.set_postfix(loglik="{0:1.4f}".format(hist[-1]))
            if len(hist) > 1 and abs(hist[-1] - hist[-2]) <= tol * abs(hist[-2]):
                converged = True
                break
        if bar is not None:
            bar.close()
        self._population_check(sigma, spacing)                                   # what is returned is held to the same two rules
        up_np[G:G + p * D] = gamma.reshape(-1)
        up.copy_(up_h, non_blocking=True)
        mu_into()
        down_h.copy_(down, non_blocking=True)
        stream.synchronize()
        self._population_reach(down_np[1:1 + D], sigma, span)
        return {"gamma": gamma, "sigma": sigma, "loglik": hist, "iterations": len(hist), "converged": converged}

    def fit_population(self, covariates, **kw):
        raise NotImplementedError("%s has no latent regression: fit_population models a continuous latent, theta_i ~ N(Gamma^T x_i, "
                                  "Sigma); attribute patterns have no such population (IrtEngine with x_feature <= 3 has it)"
                                  % type(self).__name__)

    def _grid_counts(self, call):
        """The posterior kernel for loglik, then the counts kernel over the same image: n1, n0 [J][G], mass [G] and prob [J][G] =
        P(y_j = 1 | node g) out of the image."""
        be, J, G = self.be, call.J, call.G
        post = self._grid_posterior(call)
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {"n1": torch.empty(J, G, **f32), "n0": torch.empty(J, G, **f32), "mass": torch.empty(G, **f32)}
        ws = torch.empty(be.grid_counts_workspace(call.n, J, G), **f32)
        be.grid_counts(call.y, call.rows, call.n, J, G, post["img"], call.logw, post["loglik"], out["n1"], out["n0"], out["mass"], ws)
        out["prob"] = grid_image_prob(post["img"], J, G)
        return out

    def _grid_counts_cond(self, call, tilt, seg_start):
        """The counts of `call` under call.logw and a tilt a person ([n][D] float32 by batch position), a table set a segment of
        the batch positions (seg_start: int64 numpy [S + 1] on the host): the conditioned posterior kernel for logjoint, then
        vx_grid_counts_cond over the same image -- n1, n0 [S][J][G], mass [S][G] and prob [J][G].  tilt None: the zero tilt, with
        the unconditioned posterior kernel's loglik as the normaliser (the same bits) and one zero coordinate a node, which
        also serves nodes of more than three dimensions (the patterns of CcdmEngine)."""
        be, J, G, n = self.be, call.J, call.G, call.n
        S = int(len(seg_start)) - 1
        f32 = dict(dtype=torch.float32, device=self.dev)
        if tilt is None:
            post = self._grid_posterior(call)
            D, coord, tilt, logjoint = 1, torch.zeros(G, 1, **f32), torch.zeros(n, 1, **f32), post["loglik"]
        else:
            post = self._grid_posterior_cond(call, tilt)
            D, coord, logjoint = call.D, call.theta, post["logjoint"]
        out = {"n1": torch.empty(S, J, G, **f32), "n0": torch.empty(S, J, G, **f32), "mass": torch.empty(S, G, **f32)}
        ws = torch.empty(be.grid_counts_cond_workspace(n, S, J, G), **f32)
        be.grid_counts_cond(call.y, call.rows, n, J, G, D, post["img"], call.logw, coord, tilt, logjoint, seg_start, out["n1"],
                            out["n0"], out["mass"], ws)
        out["prob"] = grid_image_prob(post["img"], J, G)
        return out

    def _group_counts(self, groups, y_u8, covariates, impact, **grid_kw):
        """What group_counts() and dif() share: the persons sorted by label, the prior each is scored under (_group_prior, the
        engine's own) and the grouped tables of ONE vx_grid_counts_cond launch.  Returns (tables, call, labels, seg_start)."""
        self._one_rank_only("dif / group_counts over a process group: the tables are the sums over the local shard's persons and "
                            "the cross-rank sum is not built")
        self._group_refusals(covariates, impact)
        call = self._grid_call(y_u8, None, **grid_kw)
        labels, order, seg_start = group_labels(groups, call.n)
        call = call._replace(rows=torch.from_numpy(order).to(self.dev))
        call, tilt, group_mean, sigma = self._group_prior(call, seg_start, covariates, impact, **grid_kw)
        out = self._grid_counts_cond(call, tilt, seg_start)
        if group_mean is not None:
            out["group_mean"], out["sigma"] = group_mean, sigma
        return out, call, labels, seg_start

    def group_counts(self, groups, y_u8=None, covariates=None, impact=None, **grid_kw):
        """The tables behind dif(), as device tensors: `n1`, `n0` [H][J][G] and `mass` [H][G], the expected counts of every group
        of persons (`groups`: one integer label a person; H = the distinct labels, `labels`, sorted) under the prior dif()
        describes for `impact` / `covariates`, beside `prob` [J][G], `n_group` (int64 [H], the persons of each group) and, for
        IrtEngine, `group_mean` [H][D] and `sigma` [D][D] (numpy).  One launch over all groups.  Deterministic: the same call
        gives the same bits, and a group's tables do not depend on the other groups' persons (under impact=True the prior does:
        Sigma is shared).  Refusals as dif()."""
        out, _, labels, seg_start = self._group_counts(groups, y_u8, covariates, impact, **grid_kw)
        out["labels"], out["n_group"] = labels, np.diff(seg_start)
        return out

    def dif(self, groups, y_u8=None, covariates=None, impact=None, min_obs=8, top=20, refit=False, newton=8, **grid_kw):
        """Differential item functioning as the item-by-group fit of the large-scale assessments: for every group of persons
        (`groups`: one integer label a person of the scored rows; `labels` = np.unique of them, H = 2 .. 4096 groups) the RMSD
        and MD of the group's observed item characteristic curve -- from the group's own expected counts -- against the POOLED
        fitted curve `prob` under the item parameters as they stand.  Nothing of the engine changes.
        The prior a person is scored under decides what the statistic means:
          impact=True (IrtEngine's default) fits a private latent regression on group dummies first (reference: the first
            label; one shared Sigma; the EM of fit_population with its refusals, 200 iterations at most, not kept in
            engine.population), so that a group whose ability differs is scored around its own mean;
          covariates=x scores under engine.population as it stands (fit_population()); impact must then be None or False;
          impact=False scores everybody under N(0, I) (CcdmEngine: the uniform pattern prior, its only setting).  A group
            whose mean is off centre is then shrunk towards 0 and its observed curve is bent on EVERY item: this setting reads
            impact as DIF.
        Returns numpy: `labels` [H], `n_group` [H], `rmsd`, `md` float64 [H][J] (item_fit_stats a group; NaN where fewer than
        min_obs persons of the group answered the item), `n_obs` int64 [H][J], `observed` [H][J][G], `prob` [J][G], `mass`
        [H][G], `group_mean` [H][D] and `sigma` [D][D] (IrtEngine; zeros and I for impact=False), and `group` (index into
        labels), `item`, `value`: the `top` cells by descending rmsd.
        refit=True (irt_1pl / irt_2pl): every group's items refitted to that group's tables from the pooled values -- `newton`
        steps of fit_em's M-step (vx_grid_mstep_irt), one call a group, under the engine's free mask -- as `b_group` [H][J],
        `a_group` [H][D][J] and `delta_b` = b_group - b.  No test statistic is attached: expected counts are not data, and a
        standard error computed from them as if they were would be too small.
        Inputs and grid as score(); one rank only."""
        min_obs = self._int_in("min_obs", min_obs, 1)
        top = self._int_in("top", top, 0)
        if refit:
            self._int_in("newton", newton, 1, EM_MAX_NEWTON,
                         "in 1 .. %d (Newton steps of an item inside one M-step launch)" % EM_MAX_NEWTON)
            self._group_refit_check()
        c, call, labels, seg_start = self._group_counts(groups, y_u8, covariates, impact, **grid_kw)
        s = group_fit_stats(c["n1"], c["n0"], c["prob"], min_obs)
        out = {"labels": labels, "n_group": np.diff(seg_start), "rmsd": s["rmsd"].cpu().numpy(), "md": s["md"].cpu().numpy(),
               "n_obs": np.rint(s["n_obs"].cpu().numpy()).astype(np.int64), "observed": s["observed"].cpu().numpy(),
               "prob": c["prob"].cpu().numpy(), "mass": c["mass"].cpu().numpy()}
        if "group_mean" in c:
            out["group_mean"], out["sigma"] = c["group_mean"], c["sigma"]
        out.update(group_fit_top(out["rmsd"], top))
        if refit:
            out.update(self._group_refit(call, c["n1"], c["n0"], newton))
        return out

    def _em_loop(self, call, mstep, leaves, max_iter, tol, progress, lprior=None):
        """The EM iterations of IrtEngine.fit_em and CcdmEngine.fit_em over a call on the caller's compact parameter copies:
        tables, vx_grid_posterior, the sum of its loglik (as marginal_loglik sums it), vx_grid_counts, the M-step (mstep(n1, n0),
        on those copies) and the write-back of the copies into the leaves ({name: copy}).  Every buffer is made once, before the
        loop.  The float of an iteration is fetched after its M-step is queued: one host sync an iteration, behind which the
        device is never idle for long.
        lprior (fit_em(prior=)): the [J] tensor into which mstep writes every item's log prior at the parameters it started
        from.  Its sum (on the device) added to the iteration's loglik is `logpost`, the quantity a penalised EM raises:
        the history that is returned beside loglik and on which convergence is then judged."""
        be = self.be
        y, J, theta, logw, G, D, n = call.y, call.J, call.theta, call.logw, call.G, call.D, call.n
        f32 = dict(dtype=torch.float32, device=self.dev)
        img = torch.empty(be.grid_image_bytes(J, G), dtype=torch.uint8, device=self.dev)     # (filled anew every iteration)
        loglik, mean, sd = torch.empty(n, **f32), torch.empty(n, D, **f32), torch.empty(n, D, **f32)
        node = torch.empty(n, dtype=torch.int32, device=self.dev)
        n1, n0, mass = torch.empty(J, G, **f32), torch.empty(J, G, **f32), torch.empty(G, **f32)
        ws = torch.empty(be.grid_counts_workspace(n, J, G), **f32)
        total, sum_ws = torch.zeros(2, **f32), torch.empty(1024, **f32)      # vx_sum_workspace_floats(); not the step's

        def iteration():
            call.fill_tables(img)
            be.grid_posterior(y, None, n, J, G, D, img, logw, theta, loglik, mean, sd, node)
            be.sum_into(loglik, n, 1.0, total[:1], sum_ws)
            be.grid_counts(y, None, n, J, G, img, logw, loglik, n1, n0, mass, ws)
            mstep(n1, n0)

        return self._em_history(iteration, total, sum_ws, leaves, max_iter, tol, progress, lprior)

    def _em_history(self, iteration, total, sum_ws, leaves, max_iter, tol, progress, lprior=None):
        """What every EM of the family does around its own E- and M-step: iteration() queues one of them on the caller's compact
        copies and leaves the float32 sum of loglik in total[0]; here the log prior's sum into total[1] (lprior), the write-back
        of the copies into the leaves ({name: copy}), the one host sync an iteration, the histories and the stopping rule."""
        be = self.be
        bar = None
        if progress:
            try:
                from tqdm import trange
                bar = trange(max_iter)
            except Exception:  # pragma: no cover
                bar = None
        liks, hist, converged = [], [], False
        for _ in range(max_iter):
            iteration()
            if lprior is not None:
                be.sum_into(lprior, int(lprior.numel()), 1.0, total[1:], sum_ws)
            for name, t in leaves.items():
                leaf = self.unconstrained(name)
                leaf.copy_(t.reshape(leaf.shape))
            lik, lp = total.tolist()
            liks.append(lik)
            hist.append(lik + lp if lprior is not None else lik)
            if bar is not None:
                bar.update(1)
                bar.set_postfix(loglik="{0:1.4f}".format(hist[-1]))
            if len(hist) > 1 and hist[-1] - hist[-2] <= tol * abs(hist[-2]):
                converged = True
                break
        if bar is not None:
            bar.close()
        out = {"loglik": liks, "iterations": len(hist), "converged": converged}
        if lprior is not None:
            out["logpost"] = hist
        return out

    def item_information(self, y_u8=None, rows=None, prior=None, **kw):
        """The cross-product (BHHH, empirical) information of the item parameters over the scored rows, AT THE PARAMETERS
        AS THEY STAND: with s_i the marginal score of person i (Fisher's identity over the grid posterior of score()), `info` =
        sum_i s_i s_i^T, float32 [P][P] on the device, symmetric bit for bit, and `gradient` = sum_i s_i [P], the gradient of
        marginal_loglik() -- what fit_em's M-step forms from the expected counts.  Dense layout: column c = j K + k; IrtEngine:
        K = x_feature + 1 (k = 0: b, k = 1 + d: a_d; 1PL: K = 1), CcdmEngine: K = 2 (g_un, s_un); P = J K <= 4096.  Also `n`
        (the persons), `free` bool [P] (the engine's free mask over a; b, g and s are always free) and `index`, the numpy arrays
        `item` and `k` [P].  Its inverse is a covariance only at the marginal maximum, i.e. after fit_em() has converged;
        `gradient` says how far from it the parameters are.  Inputs, grid and limits as score(); one rank only.
        Works in buffers of its own.  Deterministic: the same call gives the same bits.
        prior (IrtEngine; fit_em's argument, checked by grid.em_prior with its rules and ValueErrors): the matrix at the
        Bayes-modal fit of fit_em(prior=), which opens irt_3pl and irt_4pl -- their columns go on with k = x_feature + 1: c_un and,
        for 4PL, k = x_feature + 2: d_un (K = x_feature + 2 / + 3; 4PL at three dimensions allows 682 items), the tables of
        vx_grid_wtable_irt_map.  `info` and `gradient` remain the LIKELIHOOD's (for 1PL / 2PL with the bits of the call without
        `prior`); the prior's share comes beside them as float64 numpy [P] over the dense layout: `prior_precision` (1 / sd^2)
        and `prior_gradient` = -precision (p - mean), both zero where the unknown is not free or has no prior.  info +
        diag(prior_precision) approximates the negative Hessian of the log posterior, and gradient + prior_gradient is the
        gradient of the log posterior: what vanishes where fit_em(prior=) converged.  Without `prior` nothing changes: 1PL / 2PL
        and CcdmEngine as before, irt_3pl / irt_4pl refuse (the likelihood alone does not pin an asymptote: there is no fit to
        stand at); CcdmEngine refuses a prior with ValueError, as its fit_em does."""
        self._one_rank_only("item_information / item_se over a process group: the matrix is the sum over the local shard's "
                            "persons and the cross-rank sum is not built")
        if prior is None:
            call, K, fill_wtable, free = self._info_call(y_u8, rows, **kw)
        else:
            call, K, fill_wtable, free = self._info_call(y_u8, rows, prior=prior, **kw)
        be, J, G, n = self.be, call.J, call.G, call.n
        P = J * K
        if P > INFO_MAX_PARAMS:
            raise NotImplementedError("item_information takes at most %d item parameters (this model has %d x %d; irt_4pl at three "
                                      "dimensions, 6 an item, allows 682 items)" % (INFO_MAX_PARAMS, J, K))
        post = self._grid_posterior(call)
        f32 = dict(dtype=torch.float32, device=self.dev)
        wimg = torch.empty(be.grid_wimage_bytes(P, G), dtype=torch.uint8, device=self.dev)
        fill_wtable(wimg)
        info, gradient = torch.empty(P, P, **f32), torch.empty(P, **f32)
        ws_floats = be.grid_info_workspace(n, P, G)
        ws = torch.empty(ws_floats, **f32)
        be.grid_info(call.y, call.rows, n, J, G, K, post["img"], wimg, call.logw, post["loglik"], info, gradient, ws, ws_floats)
        out = {"info": info, "gradient": gradient, "n": n, "free": free,
               "index": {"item": np.repeat(np.arange(J), K), "k": np.tile(np.arange(K), J)}}
        if prior is not None:
            out["prior_precision"], out["prior_gradient"] = self._info_prior(prior, free.cpu().numpy())
        return out

    def item_se(self, y_u8=None, rows=None, prior=None, **kw):
        """Standard errors of the item parameters from item_information(), as float64 numpy arrays shaped like the leaves
        (IrtEngine: `b` and, for 2PL, `a`; CcdmEngine: `g_un`, `s_un` and, by the delta method, `g`, `s` on the probability
        scale), NaN for a parameter that is fixed (a_free = 0) or was dropped because its column of the matrix is exactly zero
        (an item nobody answered; the s of a DINO single-attribute item).  Also `cov` (float64, kept x kept), `kept` (the dense
        columns of its rows), `gradient_max` and `condition` (item_se_host).  The matrix is the cross-product information AT THE
        PARAMETERS AS THEY STAND: these are standard errors only at the marginal maximum, after fit_em() has converged --
        `gradient_max` shows how far from it the parameters are.  A kept block that is not positive definite raises ValueError.
        prior (item_information's; IrtEngine, all four models): the matrix that is inverted is the cross-product information of
        the likelihood PLUS the prior's precision on its diagonal, at the parameters as they stand -- an approximation to the
        posterior covariance at the posterior mode, where fit_em(prior=) ends.  `gradient_max` is then the largest entry of
        the gradient of the log POSTERIOR (gradient + prior_gradient), the quantity that vanishes there.  irt_3pl / irt_4pl
        also return `c_un` (and `d_un`) shaped like the leaves and, by the delta method, `c` (`d`) on the probability scale:
        se x (1 - x), x the asymptote as the tables cap it.  An item nobody answered stays NaN under any prior."""
        inf = self.item_information(y_u8, rows, prior=prior, **kw)
        item, k = inf["index"]["item"], inf["index"]["k"]
        gradient = inf["gradient"].cpu().numpy()
        if prior is not None:
            gradient = gradient.astype(np.float64) + inf["prior_gradient"]
        out = item_se_host(inf["info"].cpu().numpy(), gradient, inf["free"].cpu().numpy(),
                           names=lambda c: "item %d, parameter %d of its %d" % (item[c], k[c], int(k.max()) + 1),
                           precision=inf.get("prior_precision"))
        out.update(self._se_leaves(out.pop("se")))
        return out

    def _point_refusals(self, method):
        """What a class without point_estimates() says to at= other than "eap" (IrtEngine has its own)."""
        raise ValueError("at=%r on %s: its point estimate is the MAP pattern of score(); only at='eap' is served"
                         % (method, type(self).__name__))

    def _at_check(self, at):
        """The refusals of at=, before anything is computed."""
        if not isinstance(at, str) or at not in POINT_AT:
            raise ValueError("at must be one of %s (got %r)" % (", ".join(repr(k) for k in POINT_AT), at))
        if at != "eap":
            self._point_refusals(at)

    def _estimate_at(self, call, post, key, at):
        """The point estimates a diagnostic takes its residuals at: at="eap", the posterior kernel's own (`post[key]`, today's
        path and bits); "wle" | "ml" | "map", the theta_hat of point_estimates() with its defaults (_point_run), the EAP in its
        place for a person whose status is `empty` or `singular` -- returns (estimates, that mask or None)."""
        if at == "eap":
            return post[key], None
        pt = self._point_run(call, post["mean"], at)
        bad = (pt["status"] == POINT_EMPTY) | (pt["status"] == POINT_SINGULAR)
        return torch.where(bad[:, None], post["mean"], pt["theta_hat"]).contiguous(), bad

    def residual_sums(self, y_u8=None, rows=None, at="eap", **grid_kw):
        """The pairwise-complete residual sums of the scored rows (vx_grid_pairs_*): with r_ij = y_ij - P_ij the residual of an
        observed cell AT THE PERSON'S POINT ESTIMATE -- the grid EAP of score() for IrtEngine (all four models), the MAP pattern
        for CcdmEngine -- under the item parameters as they stand, and I_jk the persons who answered both j and k: float32
        device tensors [J][J] `n` = |I_jk|, `s` = sum of r_ij, `ss` = sum of r_ij^2 (the ROW item's, over I_jk: not symmetric) and
        `sp` = sum of r_ij r_ik (symmetric bit for bit, as is n), beside `theta_hat` (n, D) or `pattern` (n,), the estimates the
        residuals were taken at.  Inputs, grid and refusals as score(); one rank only.  Works in buffers of its own.
        Deterministic: the same call gives the same bits.  n is exact up to 2**24 scored persons.
        at (IrtEngine): "eap" (the default: the path and the bits above), or "wle" | "ml" | "map": the residuals at the theta_hat
        of point_estimates(method=at) with its defaults.  A person whose estimate has status `empty` or `singular` is passed
        with its EAP instead (an empty person adds nothing to any pair); CcdmEngine raises ValueError for anything but "eap"."""
        self._one_rank_only("residual_sums / local_dependence over a process group: the tables are the sums over the local shard's "
                            "persons and the cross-rank sum is not built")
        self._at_check(at)
        call, name, key, run = self._pairs_call(y_u8, rows, **grid_kw)
        post = self._grid_posterior(call)
        est, _ = self._estimate_at(call, post, key, at)
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {k: torch.empty(call.J, call.J, **f32) for k in ("n", "s", "ss", "sp")}
        ws_floats = self.be.grid_pairs_workspace(call.n, call.J)
        ws = torch.empty(ws_floats, **f32)
        run(est, out, ws, ws_floats)
        out[name] = est
        return out

    def local_dependence(self, y_u8=None, rows=None, min_pairs=8, top=20, at="eap", **grid_kw):
        """Yen's Q3 of every item pair (pair_q3_host over residual_sums): the correlation, over the persons who answered both
        items, of the residuals y - P taken at the EAP (IrtEngine) or the MAP pattern (CcdmEngine) under the item parameters as
        they stand.  Pairs are pairwise-complete: a 255 cell takes its person out of the pairs of that item only.  Returns numpy:
        `q3` float64 [J][J] (NaN where fewer than min_pairs persons answered both items or where an item's residuals have no
        spread over them; the diagonal is 1 where defined), `n_pairs` int64 [J][J], `mean` = the mean of the finite off-diagonal
        entries (about -1 / (J - 1) under local independence, which is why it is reported), `max` = the largest off-diagonal
        q3 - mean, and `item_j`, `item_k`, `value`: the `top` pairs j < k by descending |q3 - mean| with their q3.
        min_pairs: an integer >= 2; below the default 8 the statistic's own cancellation magnifies float32 rounding.
        at: "eap" (default) or "wle" | "ml" | "map" (IrtEngine): where the residuals are taken, as residual_sums() has it."""
        min_pairs = self._int_in("min_pairs", min_pairs, 2)
        top = self._int_in("top", top, 0)
        t = self.residual_sums(y_u8, rows, at=at, **grid_kw)
        n = t["n"].cpu().numpy()
        q3 = pair_q3_host(n, t["s"].cpu().numpy(), t["ss"].cpu().numpy(), t["sp"].cpu().numpy(), min_pairs)
        out = pair_q3_summary(q3, top)
        out["q3"], out["n_pairs"] = q3, np.rint(n).astype(np.int64)
        return out

    def pair_tables(self, y_u8=None, rows=None):
        """The observed 2 x 2 table of every item pair over the scored rows (vx_pair_tables, the int8 MFMA): int32 device tensors
        [J][J] `n11`, `n10`, `n01`, `n00` -- n_ab[j][k] = the persons who answered both items, a to item j and b to item k.  A
        cell that is neither 0 nor 1 (255 = missing) takes its person out of that item's pairs only.  n11 and n00 are symmetric,
        n10[j][k] = n01[k][j]; the diagonal of n11 / n00 holds the item's counts of 1s / 0s, that of n10 and n01 zeros; their sum
        is residual_sums()["n"].  Inputs and `rows` as score(); the model's own items and persons only (no phantoms of a padded
        engine).  Needs no grid and no item parameter: every model and every x_feature.  Exact integers up to 2**31 - 1
        persons, the same bits on every call.  One rank only."""
        self._one_rank_only("pair_tables / ld_x2 over a process group: the tables are the sums over the local shard's persons and "
                            "the cross-rank sum is not built")
        J = int(getattr(self, "J_items", self.J))
        y, rows = self._score_inputs(y_u8, rows, J)
        n = int(y.shape[0]) if rows is None else int(rows.numel())
        out = {k: torch.empty(J, J, dtype=torch.int32, device=self.dev) for k in PAIR_TABLES}
        ws_ints = self.be.pair_tables_workspace(n, J)
        ws = torch.empty(ws_ints, dtype=torch.int32, device=self.dev) if ws_ints else None
        self.be.pair_tables(y, rows, n, J, out["n11"], out["n10"], out["n01"], out["n00"], ws, ws_ints)
        return out

    def ld_x2(self, y_u8=None, rows=None, min_pairs=8, min_expected=1.0, top=20, **grid_kw):
        """Chen & Thissen's (1997) LD X2 (and G2) of every item pair (pair_x2_host over pair_tables): the observed 2 x 2 table
        of the persons who answered both items against the table the model predicts, E_ab = N_jk sum_g w_g p_a[j][g] p_b[k][g]
        over the nodes and the prior of score(), with p1 and p0 read back from the operand image the kernels multiply with.
        **The statistic is taken at the item parameters as they stand.  chi-square(1) is the reference Chen & Thissen propose
        after the item parameters were ESTIMATED from these data -- estimation fits the margins.  At parameters that were not
        fitted to these data (generating values, another sample's estimates) a fully specified 2 x 2 table has up to 3 degrees
        of freedom and the statistic runs higher.  The reference is approximate in any case; the authors say so.**  With cells
        missing completely at random (booklet designs) the persons who answered both items have the prior of score(); under
        other missingness mechanisms they have not, and E is off by that much.
        Returns numpy: `x2`, `g2`, `z` = (x2 - 1) / sqrt 2, `p` = chi2_sf(x2, 1), `sign` (+1: the pair agrees more than the model
        says, -1: less), `phi_obs`, `phi_exp`, float64 [J][J], all symmetric; NaN in x2, g2, z, p on the diagonal, where fewer
        than min_pairs persons answered both items and where an expected count is below min_expected (sign 0 there);
        `n_pairs` int64 [J][J]; `expected` [2][2][J][J]; and `item_j`, `item_k`, `value`, `sign_top`: the `top` pairs j < k by
        descending x2 with their signs.  Inputs, grid and refusals as score(); one rank only.  Not built: polytomous tables,
        covariates= / at=, M2, more than one rank."""
        min_pairs = self._int_in("min_pairs", min_pairs, 1)
        top = self._int_in("top", top, 0)
        if isinstance(min_expected, bool) or not (isinstance(min_expected, (int, float, np.floating, np.integer))
                                                  and np.isfinite(min_expected) and min_expected > 0):
            raise ValueError("min_expected must be a positive finite number")
        for k in ("covariates", "at"):
            if k in grid_kw:
                raise NotImplementedError("ld_x2 with %s=: the expected tables are built under the prior of score() and need no "
                                          "point estimate; the latent regression's prior is not built" % k)
        self._one_rank_only("pair_tables / ld_x2 over a process group: the tables are the sums over the local shard's persons and "
                            "the cross-rank sum is not built")
        call = self._grid_call(y_u8, rows, **grid_kw)
        p1, p0 = grid_image_probs(self._grid_image(call), call.J, call.G)
        t = self.pair_tables(call.y, call.rows)
        out = pair_x2_host(*(t[k].cpu().numpy() for k in PAIR_TABLES), p1.cpu().numpy(), p0.cpu().numpy(), call.logw.cpu().numpy(),
                           min_pairs, min_expected)
        tp = pair_x2_top(out["x2"], out["sign"], top)
        out.update({"item_j": tp["item_j"], "item_k": tp["item_k"], "value": tp["value"], "sign_top": tp["sign"]})
        return out

    def fit_sums(self, y_u8=None, rows=None, at="eap", **grid_kw):
        """The sums behind person_fit() and item_msq() (vx_grid_fit_*), over the observed cells of the scored rows.  With P the
        model probability AT THE PERSON'S POINT ESTIMATE -- the grid EAP of score() for IrtEngine (all four models), the MAP
        pattern for CcdmEngine -- under the item parameters as they stand, Q = 1 - P and lambda = log(P / Q): float32 device
        tensors `person` = {n, l0 = sum(y ? log P : log Q), e = sum(P log P + Q log Q), v = sum(P Q lambda^2), sr2 = sum(y ? Q^2
        : P^2), sw = sum(P Q), sz2 = sum(y ? Q / P : P / Q)}, each (n,), over the items a person answered, and `item` = {n, sr2,
        sw, sz2}, each (J,), over the persons who answered an item, beside `theta_hat` (n, D) or `pattern` (n,), the estimates
        they were taken at.  A person or item without answers has exact zeros.  Inputs, grid and refusals as score(); with a
        process group the sums are this rank's shard's (the person sums are complete, the item sums are not).  Works in buffers
        of its own.  Deterministic: the same call gives the same bits.  The counts are exact up to 2**24 scored persons.
        at (IrtEngine): "eap" (the default: the path and the bits above), or "wle" | "ml" | "map": the sums at the theta_hat of
        point_estimates(method=at) with its defaults; then also `no_estimate` (bool (n,)): the persons whose estimate has
        status `empty` or `singular` -- their sums are taken at the EAP, and person_fit() reports NaN for them.  CcdmEngine
        raises ValueError for anything but "eap"."""
        self._at_check(at)
        call, name, key, run = self._fit_call(y_u8, rows, **grid_kw)
        post = self._grid_posterior(call)
        est, bad = self._estimate_at(call, post, key, at)
        f32 = dict(dtype=torch.float32, device=self.dev)
        person, item = torch.empty(len(PERSON_SUMS), call.n, **f32), torch.empty(len(ITEM_SUMS), call.J, **f32)
        ws_floats = self.be.grid_fit_workspace(call.n, call.J)
        ws = torch.empty(ws_floats, **f32)
        run(est, person, item, ws, ws_floats)
        out = {"person": dict(zip(PERSON_SUMS, person.unbind(0))), "item": dict(zip(ITEM_SUMS, item.unbind(0))), name: est}
        if bad is not None:
            out["no_estimate"] = bad
        return out

    def person_fit(self, y_u8=None, rows=None, at="eap", **grid_kw):
        """Person fit of the scored rows (person_fit_host over fit_sums), numpy: `lz`, `infit`, `outfit` float64 (n,), `n_obs`
        int64, `loglik0`, `expected`, `variance` (the l0, e, v of lz) and `theta_hat` or `pattern`.  lz is taken at the estimate
        without Snijders' correction: on short tests its null distribution is somewhat narrower than N(0, 1).  NaN where a
        person answered nothing.  With a process group: this rank's shard, as score().
        at: "eap" (default) or "wle" | "ml" | "map" (IrtEngine): the statistics at the theta_hat of point_estimates(method=at) --
        the estimate lz and the mean squares are defined at; a person whose estimate has status `empty` or `singular` gets NaN
        in lz, infit, outfit and theta_hat."""
        t = self.fit_sums(y_u8, rows, at=at, **grid_kw)
        s = {k: v.cpu().numpy() for k, v in t["person"].items()}
        out = person_fit_host(s)
        out["n_obs"] = np.rint(s["n"]).astype(np.int64)
        out["loglik0"], out["expected"], out["variance"] = (s[k].astype(np.float64) for k in ("l0", "e", "v"))
        name = "theta_hat" if "theta_hat" in t else "pattern"
        out[name] = t[name].cpu().numpy()
        if "no_estimate" in t:
            bad = t["no_estimate"].cpu().numpy()
            for k in ("lz", "infit", "outfit", "theta_hat"):
                out[k][bad] = np.nan
        return out

    def item_msq(self, y_u8=None, rows=None, at="eap", **grid_kw):
        """The residual mean squares of every item over the scored rows (item_msq_host over fit_sums), numpy: `infit`, `outfit`
        float64 (J,) and `n_obs` int64; NaN for an item nobody answered.  One rank only.  at: as fit_sums() has it."""
        self._one_rank_only("item_msq over a process group: fit_sums() gives the local shard's sums; the cross-rank sum is not "
                            "built")
        s = {k: v.cpu().numpy() for k, v in self.fit_sums(y_u8, rows, at=at, **grid_kw)["item"].items()}
        out = item_msq_host(s)
        out["n_obs"] = np.rint(s["n"]).astype(np.int64)
        return out

    def item_fit(self, y_u8=None, rows=None, **kw):
        """Per-item fit statistics of the scored rows (item_fit_stats over expected_counts): `n_obs`, `md`, `rmsd` [J] and
        `observed` [J][G] as float64 device tensors, beside the `prob` [J][G] they are measured against.  One rank only."""
        self._one_rank_only("item_fit over a process group: expected_counts() gives the local shard's sums; the cross-rank sum "
                            "is not built")
        c = self.expected_counts(y_u8, rows, **kw)
        out = item_fit_stats(c["n1"], c["n0"], c["prob"])
        out["prob"] = c["prob"]
        return out

    def _sumscore_items(self, items, J):
        """`items` -> the sorted distinct item indices as int64 numpy [Js] (None: all J), refused as sx2() describes."""
        if items is None:
            it = np.arange(J, dtype=np.int64)
        else:
            it = items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
            if it.dtype.kind not in "iu" or it.ndim != 1 or it.size < 1:
                raise ValueError("items must be a list of integer item indices, sorted and distinct")
            it = it.astype(np.int64)
            if it.min() < 0 or it.max() >= J or (np.diff(it) <= 0).any():
                raise ValueError("items must be sorted, distinct and in 0 .. %d" % (J - 1))
        if it.size > SUMSCORE_MAX_ITEMS:
            raise NotImplementedError("summed-score tables take at most %d items (got %d): name a booklet with items="
                                      % (SUMSCORE_MAX_ITEMS, it.size))
        return it

    def _sumscore_refusals(self, what, covariates, grid_kw):
        if "rows" in grid_kw:
            raise NotImplementedError("%s with rows=: a row subset is not built -- pass those persons' responses as data (the "
                                      "complete persons among them are found by the call itself)" % what)
        self._one_rank_only("%s over a process group: the tables are the sums over the local shard's persons and the cross-rank "
                            "sum is not built" % what)
        if covariates is not None:
            raise NotImplementedError("%s with covariates=: the summed-score tables are built under the prior score() uses "
                                      "without covariates; the latent regression's is not built" % what)

    def _sumscore_model(self, call, it, want_dist=True):
        """The model side: p1, p0 of the listed items out of the operand image and vx_sumscore_model."""
        be, G, Js = self.be, call.G, int(it.size)
        p1, p0 = grid_image_probs(self._grid_image(call), call.J, G)
        if Js != call.J:
            sel = torch.from_numpy(it).to(self.dev)
            p1, p0 = p1[sel].contiguous(), p0[sel].contiguous()
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {"e1": torch.empty(Js, Js + 1, **f32), "e0": torch.empty(Js, Js + 1, **f32),
               "dist": torch.empty(G, Js + 1, **f32) if want_dist else None}
        ws_floats = be.sumscore_model_workspace(Js, G)
        ws = torch.empty(ws_floats, **f32)
        be.sumscore_model(p1, p0, call.logw, Js, G, out["e1"], out["e0"], out["dist"], ws, ws_floats)
        return out

    def sumscore_tables(self, y_u8=None, items=None, covariates=None, **grid_kw):
        """The summed-score tables behind sx2() and score_table(), as device tensors, over `items` (a sorted list of Js distinct
        item indices; default all, Js <= 1023) and the nodes of score().  The model side, by the Lord-Wingersky recursion over
        p1 = P(y_j = 1 | node) and p0 = P(y_j = 0 | node) as the operand image holds them (vx_sumscore_model): `e1`, `e0` float32
        [Js][Js + 1], the joint probability of summed score s with y_j = 1 / 0 (e1 + e0 = P(score = s) for every j), and `dist`
        [G][Js + 1] = P(score = s | node g).  The observed side, over the COMPLETE persons of the scored rows -- every listed
        cell 0 or 1; a 255 or 254 among the listed items takes the person out -- (vx_sumscore_persons, vx_sumscore_observed):
        `score` int32 [n] (-1: not complete), `o1` int32 [Js][Js + 1] = the complete persons of score s with y_j = 1, `n` int64
        [Js + 1] = the complete persons of score s.  Also `items` (int64), `theta` [G][D] and `logw` [G].  Inputs, grid and
        refusals as score(); covariates= and rows= are not built; one rank only.  Deterministic: the same call gives the same
        bits."""
        self._sumscore_refusals("sumscore_tables / sx2", covariates, grid_kw)
        call = self._grid_call(y_u8, None, **grid_kw)
        it = self._sumscore_items(items, call.J)
        be, Js, n = self.be, int(it.size), call.n
        out = self._sumscore_model(call, it)
        items_dev = torch.from_numpy(it.astype(np.int32)).to(self.dev) if Js != call.J else None
        score = torch.empty(n, dtype=torch.int32, device=self.dev)
        be.sumscore_persons(call.y, None, n, call.J, items_dev, Js, score)
        rows = torch.nonzero(score >= 0).reshape(-1)
        sc, order = torch.sort(score[rows], stable=True)                         # (plumbing: the kernel wants the persons by score)
        rows, sc = rows[order].contiguous(), sc.contiguous()
        o1 = torch.empty(Js, Js + 1, dtype=torch.int32, device=self.dev)
        be.sumscore_observed(call.y, rows, int(rows.numel()), call.J, items_dev, Js, sc, o1)
        out.update({"o1": o1, "n": torch.bincount(sc.long(), minlength=Js + 1), "score": score,
                    "items": torch.from_numpy(it).to(self.dev), "theta": call.theta, "logw": call.logw})
        return out

    def sx2(self, y_u8=None, items=None, min_expected=1.0, covariates=None, **grid_kw):
        """Orlando & Thissen's S-X2 item-fit test of every listed item (sx2_host over sumscore_tables): within each summed-score
        group, the observed proportion correct against the proportion the model predicts for that group under the item
        parameters as they stand.  The cells are observable, so a chi-square reference applies.  Returns numpy: `sx2`, `df`, `p`,
        `n_cells` [Js]; `observed`, `expected` [Js][Js + 1], the proportions correct per score group (NaN where n[s] = 0);
        `n_persons` (the complete persons), `n_dropped` and `items`.  df = cells - the item's free parameters (1PL: 1; 2PL: 1 +
        its free loadings; 3PL / 4PL: + 1 / + 2; DINA / DINO: 2); p is NaN where df <= 0.  The score groups are collapsed by one
        left-to-right sweep until both expected counts of a cell reach min_expected (sx2_host): this project's own rule.
        Only COMPLETE persons count: with a design that leaves cells missing, name one booklet's items with items=.
        ValueError when no person is complete.  Not built: sampling weights, covariates=, more than one rank, polytomous
        items."""
        if not (isinstance(min_expected, (int, float, np.floating, np.integer)) and not isinstance(min_expected, bool)
                and np.isfinite(min_expected) and min_expected > 0):
            raise ValueError("min_expected must be a positive finite number")
        t = self.sumscore_tables(y_u8, items, covariates, **grid_kw)
        n = t["n"].cpu().numpy()
        n_persons = int(n.sum())
        total = int(t["score"].numel())
        if n_persons == 0:
            raise ValueError("no person of the %d scored rows is complete on the %d listed items: S-X2 counts complete response "
                             "vectors only -- pass items= to score one booklet of a missing-by-design test"
                             % (total, int(t["items"].numel())))
        it = t["items"].cpu().numpy()
        out = sx2_host(t["e1"].cpu().numpy(), t["e0"].cpu().numpy(), t["o1"].cpu().numpy(), n, self._sx2_params(it), min_expected)
        out.update({"n_persons": n_persons, "n_dropped": total - n_persons, "items": it})
        return out

    def score_table(self, items=None, covariates=None, **grid_kw):
        """The summed-score -> latent conversion table of the listed items (score_table_host over vx_sumscore_model's `dist`),
        under the item parameters as they stand and the prior of score(); takes no data.  Returns numpy, float64: `score`
        [Js + 1], `prob` = the model's P(score = s), and what score() reports of a person, given the summed score alone: `eap`,
        `psd` [Js + 1][D] (IrtEngine) or `attr_prob` [Js + 1][K] (CcdmEngine).  Refusals as sumscore_tables()."""
        self._sumscore_refusals("score_table", covariates, grid_kw)
        call = self._grid_call(None, None, **grid_kw)
        it = self._sumscore_items(items, call.J)
        m = self._sumscore_model(call, it)
        out = score_table_host(m["dist"].cpu().numpy(), call.logw.cpu().numpy(), call.theta.cpu().numpy())
        out["items"] = it
        return self._score_table_leaves(out)

    def marginal_loglik(self, y_u8=None, rows=None, **kw):
        """sum_i log p(y_i) under the item parameters as they stand, summed on the device in a fixed order."""
        self._one_rank_only("marginal_loglik over a process group: score() gives the local shard's rows; the cross-rank sum is "
                            "not built")
        ll = self.score(y_u8, rows, **kw)["loglik"]
        out = torch.empty(1, dtype=torch.float32, device=self.dev)
        ws = torch.empty(1024, dtype=torch.float32, device=self.dev)            # vx_sum_workspace_floats(); not the step's
        self.be.sum_into(ll, int(ll.numel()), 1.0, out, ws)
        return float(out.item())
