"""Host-side mirror of the reference's model-class surface (/root/reference/vi.py) for the path that is
accelerated: same class names, constructor kwargs, `.fit(optim, loss, max_iter, random_instance)`
signature and result access (`param(name)` / `clear_param_store()` standing in for pyro.param /
pyro.clear_param_store, test.py:66,73-87), so the reference's demos read the same:

    from vipsy_amd.vi import VaeIRT, Adam, MultiStepLR, Trace_ELBO, param
    model = VaeIRT(data=y, model='irt_2pl', subsample_size=100, x_feature=100)     # test.py:343
    model.fit(optim=MultiStepLR({...}), max_iter=20000, random_instance=ri, loss=Trace_ELBO(num_particles=1))
    a_hat = param('a')

What runs underneath is NOT pyro: every iteration is one vipsy_amd.engine step, i.e. the HIP kernels behind
include/vipsy_amd.h (no CPU fallback).  Every model class of the reference is built: VIRT, VaeIRT, VCDM, VaeCDM, VCCDM,
VaeCCDM, VCHoDina, VaeCHoDina.
"""
import numpy as np
import torch

from .engine import CcdmEngine, CdmSfEngine, IrtEngine, HoDinaEngine, LrSpec, VaeCcdmEngine
from .random_data import (RandomPsyData, RandomIrt1PL, RandomIrt2PL, RandomIrt3PL, RandomIrt4PL, RandomMilIrt2PL,    # noqa: F401
                          RandomMilIrt3PL, RandomMilIrt4PL, RandomDina, RandomDino, RandomHoDina)  # vi.py:120-412 live in vi too

_STORE = {}          # name -> engine that owns the parameter (the process-global store of the reference)


def clear_param_store():
    _STORE.clear()


def param(name):
    """Constrained value of a parameter, like pyro.param(name) (vi.py:644-654; test.py:73-87)."""
    if name not in _STORE:
        raise KeyError(name)
    return _STORE[name].param(name)


# ---- optimiser / loss descriptors (pyro.optim.Adam, pyro.optim.MultiStepLR, pyro.infer.*_ELBO) ------------
class Adam(object):
    """pyro.optim.Adam(optim_args): optim_args is a dict or a callable(module_name, param_name) -> dict
    (test.py:321-327, 345-350).  One Adam state per tensor, betas/eps as torch defaults."""

    def __init__(self, optim_args):
        self.optim_args = optim_args

    def spec(self):
        return LrSpec(self.optim_args)                  # lr / betas / eps per tensor, dict or callable alike


class PyroLRScheduler(object):
    pass


class MultiStepLR(PyroLRScheduler):
    """pyro.optim.MultiStepLR({'optimizer': torch.optim.Adam, 'optim_args': dict|callable, 'milestones': [...],
    'gamma': g}) (test.py:352-359).  The scheduler advances once per iteration (vi.py:639-640)."""

    def __init__(self, args):
        if args.get("optimizer") not in (None, torch.optim.Adam):
            raise NotImplementedError("only torch.optim.Adam is on the HIP path")
        self.args = args

    def spec(self):
        return LrSpec(self.args["optim_args"], milestones=tuple(self.args.get("milestones", ())),
                      gamma=float(self.args.get("gamma", 0.1)))


class Trace_ELBO(object):
    def __init__(self, num_particles=1):
        self.num_particles = int(num_particles)


class TraceEnum_ELBO(Trace_ELBO):
    pass


# ---- data ----------------------------------------------------------------------------------------------
def to_u8(data, device):
    """Reference data contract (float tensor, NaN = missing; vi.py:621) -> uint8 0/1/255 on the device."""
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(data)
    if data.dtype == torch.uint8:
        return data.to(device).contiguous()
    d = data.to(device)
    miss = torch.isnan(d)
    vals = torch.where(miss, torch.zeros_like(d), d)
    if not bool(((vals == 0) | (vals == 1)).all()):
        raise ValueError("responses must be 0/1 (NaN = missing)")
    out = vals.to(torch.uint8)
    out[miss] = 255
    return out.contiguous()


class BasePsy(object):
    """vi.py:521-533.  Multi-GPU is explicit: pass `group` (a torch.distributed process group, e.g.
    torch.distributed.group.WORLD) and `data` is THIS rank's shard of persons, placed in the global plate by
    `sample_size_global` / `gid0`.  Without `group` the object owns its whole problem even when a process group is up
    (independent replications on different ranks, vipsy_amd/harness.py)."""

    def __init__(self, data, subsample_size=None, sample_size_global=None, gid0=0, seed=1234, device=None, group=None,
                 **kwargs):
        if device is None:
            if torch.is_tensor(data) and (data.device.type != "cpu" or kwargs.get("backend") is not None):
                device = data.device
            else:
                device = torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(device)
        self.data = to_u8(data, dev)
        self.sample_size_local = int(self.data.shape[0])
        self.sample_size = int(sample_size_global) if sample_size_global is not None else self.sample_size_local
        self.item_size = int(self.data.shape[1])
        self.subsample_size = int(subsample_size) if subsample_size is not None else self.sample_size
        self.gid0, self.seed, self.device = int(gid0), int(seed), dev
        self.kwargs = kwargs
        self.group = group
        self.world = torch.distributed.get_world_size(group) if group is not None else 1
        if self.world == 1 and self.sample_size != self.sample_size_local:
            raise ValueError("sample_size_global differs from the rows of `data` but no `group` shares the problem")
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(self.seed * 7919 + self.gid0)
        self._np_gen = np.random.Generator(np.random.PCG64([self.seed, self.gid0, 7919]))
        # engine keyword arguments shared by every model class (`backend` is the test seam of tests/oracle_backend.py)
        self._eng_kw = {"n_global": self.sample_size, "gid0": self.gid0, "seed": self.seed, "group": group}
        if kwargs.get("backend") is not None:
            self._eng_kw["backend"] = kwargs["backend"]

    def _register(self):
        for n in self.engine.all_names():
            _STORE[n] = self.engine

    def _subsample(self):
        """plate("data", N, subsample_size=B): randperm(N)[:B].  Multi-rank: every
        rank draws B / world of its own shard (stratified, unbiased)."""
        B = self.subsample_size
        if B >= self.sample_size:
            return None, self.sample_size
        b_local = B // self.world if self.world > 1 else B
        b_local = max(1, min(b_local, self.sample_size_local))
        n = self.sample_size_local
        if 16 * b_local <= n:
            # a small subset of many rows: a full permutation on the device is a radix sort of n keys (0.25 ms at 1M, a
            # third of a B = 100 step).  numpy's Generator.choice draws b distinct rows in O(b); same distribution over
            # subsets, ordered like the first b of a random permutation (shuffle=True)
            # (left on the host: the engine copies the indices into the fixed buffer its captured step reads, or moves them itself)
            idx = torch.from_numpy(self._np_gen.choice(n, size=b_local, replace=False, shuffle=True).astype(np.int64))
        else:
            idx = torch.randperm(n, generator=self._gen, device=self.device)[:b_local].contiguous()
        return idx, b_local * self.world

    def _loop(self, optim, loss, max_iter, progress):
        lrs = optim.spec()
        S = getattr(loss, "num_particles", 1)
        it = range(max_iter)
        bar = None
        if progress:
            try:
                from tqdm import trange
                bar = trange(max_iter)
                it = bar
            except Exception:  # pragma: no cover
                bar = None
        last = None
        sched = isinstance(optim, PyroLRScheduler)
        K = getattr(self.engine, "graph_steps", 1) if S == 1 and hasattr(self.engine, "steps") else 1
        if K > 1:
            # one particle: the iterations go to the engine K at a time (IrtEngine.steps: several steps of the loop replayed from
            # one graph where the step's form allows; the draws are made in the same order.  The results are the bits of step()
            # in a loop, except for a subsample_size that is no multiple of 4 on the shapes IrtEngine.steps pads: there both
            # are within the parity tolerance of the oracle, tests/test_gpu_fit_path.py)
            i = 0
            while i < max_iter:
                n = min(K, max_iter - i)
                draws = [self._subsample() for _ in range(n)]
                last = self.engine.steps(lrs, [d[0] for d in draws], b_global=draws[0][1], scheduler=sched)[-1]
                i += n
                if bar is not None:
                    bar.update(n)
                    if (i - n) // 50 != i // 50 or i >= max_iter:
                        bar.set_postfix(loss="{0:1.2f}".format(float(last.item())), **self._postfix())
            if bar is not None:
                bar.close()
            return None if last is None else float(last.item())
        for i in it:
            if S == 1:
                rows, bg = self._subsample()
            else:
                draws = [self._subsample() for _ in range(S)]
                rows, bg = [d[0] for d in draws], draws[0][1]
            last = self.engine.step(lrs, rows=rows, b_global=bg, num_particles=S)
            if sched:
                lrs.scheduler_step()                                   # vi.py:639-640
            if bar is not None and (i % 50 == 0 or i == max_iter - 1):
                bar.set_postfix(loss="{0:1.2f}".format(float(last.item())), **self._postfix())
        return None if last is None else float(last.item())

    def _postfix(self):
        return {}

    # -- after the fit: person scores and the marginal log-likelihood (no reference counterpart) -------------------------
    def _score_data(self, data):
        """`data` under the reference's contract (float with NaN = missing, or uint8), with the model's item count."""
        if data is None:
            return None
        y = to_u8(data, self.device)
        if y.dim() != 2 or int(y.shape[1]) != self.item_size:
            raise ValueError("data must be [persons, %d items], got %s" % (self.item_size, tuple(y.shape)))
        return y

    def score(self, data=None, **kw):
        """Exact grid posteriors of the persons in `data` (None: the training data; with a `group` this rank's shard) under
        the item parameters as they stand -- VIRT / VaeIRT with x_feature <= 3: eap, psd, loglik, node (IrtEngine.score);
        VCCDM: attr_prob, pattern, loglik (CcdmEngine.score).  The other classes refuse."""
        return self.engine.score(self._score_data(data), **kw)

    def score_bifactor(self, data=None, **kw):
        """Exact grid scores of a bifactor / testlet model -- VIRT / VaeIRT, irt_2pl / irt_3pl / irt_4pl, any x_feature >= 2, with
        a free mask (a_free, and a0 = a_free so that the loadings that are not free are zero) in which every item loads on the
        `general` dimension and on one specific dimension at the most: loglik, eap_general, psd_general, node (persons,), and
        with specific=True eap_specific, psd_specific (persons, x_feature - 1) and specific_dims (IrtEngine.score_bifactor:
        rows, nodes=(61, 21), span=(6.0, 4.0), general=0, specific=False).  `data` None: the training data; with a `group` this
        rank's shard, as score().  The work is that of one two-dimensional grid whatever x_feature is -- score() itself stops
        at x_feature = 3.  The other classes refuse; covariates= is not built."""
        return self.engine.score_bifactor(self._score_data(data), **kw)

    def expected_counts_bifactor(self, data=None, **kw):
        """The expected-count tables of a bifactor / testlet model over the grid of score_bifactor() -- models and structure as
        there: device tensors n1, n0, prob [items][Gg][Gh] (every item on the grid of the general dimension and ITS OWN specific
        dimension), mass [Gg], mass_specific [x_feature - 1][Gg][Gh], loglik (the sum) and the axes theta, logw, u, logv
        (IrtEngine.expected_counts_bifactor: rows, nodes=(41, 21), span=(6.0, 4.0), general=0).  `data` None: the training
        data.  One rank only; the other classes refuse."""
        if self.world > 1:
            raise NotImplementedError("expected_counts_bifactor with a group of %d ranks: the tables are the sums over the local "
                                      "shard's persons; the cross-rank sum is not built" % self.world)
        return self.engine.expected_counts_bifactor(self._score_data(data), **kw)

    def fit_em_bifactor(self, max_iter=100, tol=1e-6, newton=4, nodes=(41, 21), span=(6.0, 4.0), general=0, prior=None,
                        progress=False):
        """Refit the items of a bifactor / testlet model by marginal maximum likelihood: Bock-Aitkin EM on the training data
        over the grid of score_bifactor(), any x_feature >= 2 -- fit_em() itself stops at x_feature = 3.  Every iteration takes
        each item's expected counts on the Gg x Gh grid of its own testlet and refits its intercept, general loading and specific
        loading by fit_em's M-step in two dimensions (nodes[0] * nodes[1] <= 1024).  irt_2pl; irt_3pl / irt_4pl with `prior`
        (fit_em's argument and rules).  A testlet of one item needs a prior with a finite sd on "a".  Return, stopping rule and
        what is left alone as fit_em(): {"loglik", "iterations", "converged"} and, with `prior`, "logpost"
        (IrtEngine.fit_em_bifactor).  One rank only; the other classes refuse."""
        if self.world > 1:
            raise NotImplementedError("fit_em_bifactor with a group of %d ranks: the expected counts are the local shard's sums; "
                                      "the cross-rank sum is not built" % self.world)
        return self.engine.fit_em_bifactor(max_iter=max_iter, tol=tol, newton=newton, nodes=nodes, span=span, general=general,
                                           prior=prior, progress=progress)

    def bifactor_structure(self, general=0):
        """{"general", "specific_dims", "testlet" (per item: the column of specific_dims it loads on, -1: general only),
        "sizes"} as read from the model's free mask on the host (IrtEngine.bifactor_structure); ValueError naming the first
        item that is free on two specific dimensions, or whose fixed loading is not zero."""
        return self.engine.bifactor_structure(general)

    def point_estimates(self, data=None, **kw):
        """Likelihood-based person scores of the persons in `data` (None: the training data; with a `group` this rank's shard, as
        score()), ready to print: Warm's weighted likelihood estimate (method="wle", the default: what PISA, TIMSS, ConQuest and
        TAM report), the maximum-likelihood ("ml") or the MAP ("map") estimate, by Fisher scoring from the EAP of score() under
        the item parameters as they stand.  A dict of numpy arrays: theta_hat, se [persons, x_feature], cov, info [persons,
        x_feature, x_feature], status (0 converged, 1 at_bound, 2 max_iter, 3 singular, 4 empty: vipsy_amd.grid.POINT_STATUS),
        iterations, n_converged and reliability [x_feature], the person separation reliability 1 - mean(se^2) / var(theta_hat)
        (IrtEngine.point_estimates: method, max_iter=32, tol=1e-6, bound=None (= span), nodes=61, span=6.0).  An all-correct or
        all-wrong row has no finite ML estimate: it ends at_bound, on +-bound; the WLE and the MAP of such a row are finite.
        VIRT / VaeIRT, every IRT model: x_feature <= 3 for "ml" and "map", x_feature = 1 for "wle"; covariates= is not built.
        VCCDM refuses: its point estimate is the MAP pattern of score().  The other classes refuse as for score()."""
        return self.engine.point_estimates(self._score_data(data), **kw)

    def plausible_values(self, data=None, **kw):
        """Plausible values: draws of each person's latent from the exact grid posterior of score() (`data` None: the training
        data; with a `group` this rank's shard, keyed by global person id) -- VIRT / VaeIRT with x_feature <= 3: theta
        [persons, draws, x_feature] and node [persons, draws] (IrtEngine.plausible_values: draws=5, seed=0, nodes=61,
        span=6.0); VCCDM: attr [persons, draws, K] and pattern [persons, draws] (CcdmEngine.plausible_values: draws=5, seed=0).
        The draws sit on grid nodes, so their resolution is the node spacing: use more nodes for finer draws.  They are taken
        under the item parameters as they stand, without item-parameter uncertainty.  The other classes refuse."""
        return self.engine.plausible_values(self._score_data(data), **kw)

    def fit_population(self, covariates, **kw):
        """The latent regression of the training data on `covariates` ([persons][p], float, finite): theta_i ~ N(Gamma^T x_i,
        Sigma), fitted by EM over the grid of score() with the item parameters fixed as they stand (IrtEngine.fit_population:
        rows, max_iter=200, tol=1e-7, intercept=True, nodes=61, span=6.0).  Returns {"gamma" [p][x_feature], "sigma", "loglik",
        "iterations", "converged"} and keeps the population on the engine: score(covariates=...), plausible_values(covariates=...)
        and marginal_loglik(covariates=...) then work under each person's own prior -- the conditioning model a secondary
        analysis of plausible values needs.  VIRT / VaeIRT with x_feature <= 3, every IRT model; the classes score() refuses and
        VCCDM refuse.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("fit_population with a group of %d ranks: the M-step's sums are the local shard's; the "
                                      "cross-rank sum is not built" % self.world)
        return self.engine.fit_population(covariates, **kw)

    def expected_counts(self, data=None, **kw):
        """The expected-count tables of the persons in `data` (None: the training data) over the grid of score(): device
        tensors n1, n0 [items][nodes], mass [nodes], prob [items][nodes], and theta / logw (IRT) or patterns (VCCDM); see
        IrtEngine.expected_counts / CcdmEngine.expected_counts.  With a `group` of more than one rank these are the sums over
        THIS rank's shard only: add them across ranks yourself.  The classes without score() refuse.
        covariates=x (VIRT / VaeIRT, as score() takes them): the tables under each person's own prior of the population
        fit_population() estimated, instead of N(0, I); item_fit() takes it too."""
        return self.engine.expected_counts(self._score_data(data), **kw)

    def item_fit(self, data=None, **kw):
        """Per-item fit of `data` (None: the training data) against the model as it stands, ready to print: a dict of numpy
        arrays n_obs, md, rmsd [items] (the mean and root-mean-square deviation of the observed from the fitted item
        characteristic curve, weighted by the posterior population), observed, prob [items][nodes].  One rank only."""
        if self.world > 1:
            raise NotImplementedError("item_fit with a group of %d ranks: expected_counts() gives the local shard's sums; the "
                                      "cross-rank sum is not built" % self.world)
        return {k: v.detach().cpu().numpy() for k, v in self.engine.item_fit(self._score_data(data), **kw).items()}

    def group_counts(self, groups, data=None, **kw):
        """The grouped expected-count tables behind dif(), as device tensors: n1, n0 [groups][items][nodes] and mass
        [groups][nodes], one launch over all groups, beside prob, labels, n_group and (IRT) group_mean, sigma
        (GridMixin.group_counts; kw: covariates, impact, nodes, span).  One rank only."""
        if self.world > 1:
            raise NotImplementedError("group_counts with a group of %d ranks: the tables are the sums over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        return self.engine.group_counts(groups, self._score_data(data), **kw)

    def dif(self, groups, data=None, covariates=None, impact=None, min_obs=8, top=20, refit=False, newton=8, **grid_kw):
        """Differential item functioning, ready to print: does an item work the same way in every group (country, language,
        booklet)?  `groups`: one integer label a person of `data` (None: the training data).  For every (group, item) cell the
        RMSD and MD of the group's observed item characteristic curve against the pooled fitted curve under the item parameters
        as they stand -- the item-by-group fit of PISA and PIAAC -- from ONE launch over all groups.  A dict of numpy arrays:
        labels, n_group [groups], rmsd, md, n_obs [groups][items] (NaN where fewer than min_obs persons of a group answered an
        item), observed [groups][items][nodes], prob [items][nodes], mass [groups][nodes], group_mean, sigma, and group, item,
        value: the `top` cells by rmsd (GridMixin.dif).
        Each person is scored under a prior: impact=True (the default of VIRT / VaeIRT) first fits every group's mean and a
        shared Sigma by a private latent regression on group dummies, so that a difference in ABILITY between the groups
        (impact) is not read as DIF; covariates=x uses the population fit_population() left on the engine instead; impact=False
        keeps N(0, I) for everybody, which bends the observed curve of every item of a group whose mean is off centre.  VCCDM
        has the uniform pattern prior only: impact=True, covariates= and refit=True are refused there.
        refit=True (irt_1pl / irt_2pl): also b_group, a_group and delta_b, every group's items refitted to its own tables by
        `newton` steps of fit_em's M-step; no test statistic is attached, since expected counts are not data.
        VIRT / VaeIRT with x_feature <= 3 (grid_kw: nodes, span), VCCDM; the other classes refuse.  Nothing of the model
        changes.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("dif with a group of %d ranks: the tables are the sums over the local shard's persons; the "
                                      "cross-rank sum is not built" % self.world)
        return self.engine.dif(groups, self._score_data(data), covariates=covariates, impact=impact, min_obs=min_obs, top=top,
                               refit=refit, newton=newton, **grid_kw)

    def marginal_loglik(self, data=None, **kw):
        """The marginal log-likelihood of `data` (None: the training data), a Python float.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("marginal_loglik with a group of %d ranks: score() gives the local shard's rows; the "
                                      "cross-rank sum is not built" % self.world)
        return self.engine.marginal_loglik(self._score_data(data), **kw)

    def fit_em(self, max_iter=100, tol=1e-6, newton=4, progress=False, prior=None, **grid_kw):
        """Refit the item parameters by marginal maximum likelihood: Bock-Aitkin EM on the training data (this object's
        `data`) over the grid of score() (grid_kw: nodes, span), until the marginal log-likelihood rises by no more than
        tol times its size between two iterations or max_iter is reached.  VIRT / VaeIRT with irt_1pl / irt_2pl and
        x_feature <= 3 (IrtEngine.fit_em: `newton` Newton steps an item and iteration), VCCDM (CcdmEngine.fit_em: closed form);
        the other classes refuse.  Returns {"loglik": [floats], "iterations": int, "converged": bool}, loglik[k] being the
        marginal log-likelihood under the parameters at the START of iteration k: loglik[0] is marginal_loglik() before the
        call, marginal_loglik() after it gives the value of the final parameters.  The guide, the optimiser's state and the
        step count are left alone: a later fit() continues from the refitted items.  One rank only.
        prior: normal priors on the item parameters (Bayes-modal EM), which opens irt_3pl and irt_4pl -- a dict over "a", "b",
        "c", "d" of (mean, sd) on the unconstrained scale of the leaves (c, d as logits), scalars or arrays shaped like the
        leaf, e.g. prior={"c": (-1.4, 1.0), "d": (2.2, 1.0)}; irt_3pl needs a finite sd on "c", irt_4pl on "c" and "d".  The
        return then has "logpost" (loglik + the log prior, what the iterations raise and convergence is judged on) as well;
        VCCDM refuses it (IrtEngine.fit_em)."""
        if self.world > 1:
            raise NotImplementedError("fit_em with a group of %d ranks: the expected counts are the local shard's sums; the "
                                      "cross-rank sum is not built" % self.world)
        if prior is not None:
            grid_kw["prior"] = prior
        return self.engine.fit_em(max_iter=max_iter, tol=tol, newton=newton, progress=progress, **grid_kw)

    def item_information(self, data=None, prior=None, **grid_kw):
        """The cross-product (BHHH) information matrix of the item parameters over the persons in `data` (None: the training
        data) AT THE PARAMETERS AS THEY STAND, and the gradient of the marginal log-likelihood: device tensors `info` [P][P] and
        `gradient` [P] over the dense layout, with `n`, `free` and `index` (IrtEngine / CcdmEngine.item_information).  The
        inverse of the matrix is a covariance only at the marginal maximum, that is after fit_em() has converged.  VIRT / VaeIRT
        with irt_1pl / irt_2pl and x_feature <= 3, VCCDM; the other classes and models refuse.  One rank only.
        prior (fit_em's item priors, e.g. {"c": (-1.4, 1.0), "d": (2.2, 1.0)}; VIRT / VaeIRT): the matrix at the Bayes-modal
        fit of fit_em(prior=), which opens irt_3pl and irt_4pl (columns c_un, d_un after the loadings).  `info` and `gradient`
        stay the likelihood's; `prior_precision` and `prior_gradient` (float64 numpy [P]) carry the prior's curvature and the
        gradient of the log prior.  irt_3pl needs a finite sd on "c", irt_4pl on "c" and "d"; VCCDM refuses a prior."""
        if self.world > 1:
            raise NotImplementedError("item_information with a group of %d ranks: the matrix is the sum over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        if prior is not None:
            grid_kw["prior"] = prior
        return self.engine.item_information(self._score_data(data), **grid_kw)

    def item_se(self, data=None, prior=None, **grid_kw):
        """Standard errors of the item parameters, ready to print: numpy arrays shaped like the leaves (`a`, `b`; VCCDM: `g_un`,
        `s_un` and `g`, `s` on the probability scale), NaN where a parameter is fixed or has no information, with `cov`, `kept`,
        `gradient_max` and `condition` (GridMixin.item_se).  They come from the inverse of the cross-product information AT THE
        PARAMETERS AS THEY STAND: standard errors only at the marginal maximum, that is after fit_em() has converged;
        `gradient_max` shows how far from it the parameters are.  Models and refusals as item_information().  One rank only.
        prior (fit_em's; all four IRT models): the standard errors at the Bayes-modal fit, the ones a calibration report of
        irt_3pl / irt_4pl items prints.  The matrix that is inverted is the cross-product information of the likelihood plus
        the prior's precision, at the parameters as they stand: an approximation to the posterior covariance at the posterior
        mode.  `gradient_max` is then the largest entry of the gradient of the log posterior, which vanishes where
        fit_em(prior=) converged.  irt_3pl / irt_4pl also give `c_un` (`d_un`) and, by the delta method, `c` (`d`)."""
        if self.world > 1:
            raise NotImplementedError("item_se with a group of %d ranks: the information matrix is the sum over the local "
                                      "shard's persons; the cross-rank sum is not built" % self.world)
        if prior is not None:
            grid_kw["prior"] = prior
        return self.engine.item_se(self._score_data(data), **grid_kw)

    def residual_sums(self, data=None, **kw):
        """The pairwise-complete residual sums behind local_dependence(), as device tensors [items][items]: `n` (the persons who
        answered both items of a pair), `s`, `ss` (the sums of the row item's residuals and of their squares over those persons)
        and `sp` (the sum of the products of the two items' residuals), beside `theta_hat` or `pattern`.  The residuals y - P are
        taken at each person's point estimate -- the EAP of score() for VIRT / VaeIRT (every model, x_feature <= 3), the MAP
        pattern for VCCDM -- under the item parameters as they stand; pairs are pairwise-complete: a missing cell takes its person
        out of that item's pairs only.  `data`: None = the training data.  The other classes refuse.  One rank only.
        at="wle" | "ml" | "map" (VIRT / VaeIRT): the residuals at that point_estimates() score instead of the EAP."""
        if self.world > 1:
            raise NotImplementedError("residual_sums with a group of %d ranks: the tables are the sums over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        return self.engine.residual_sums(self._score_data(data), **kw)

    def local_dependence(self, data=None, **kw):
        """Yen's Q3 for every item pair, ready to print: the correlation, over the persons who answered both items, of the
        residuals y - P taken at each person's point estimate -- the EAP of score() for VIRT / VaeIRT (every model, x_feature
        <= 3), the MAP pattern for VCCDM -- under the item parameters as they stand; nothing is refitted.  Pairs are
        pairwise-complete: a missing cell takes its person out of that item's pairs only.  A dict of numpy values: `q3`
        [items][items], `n_pairs`, `mean` (about -1 / (items - 1) under local independence), `max` (the largest q3 - mean off
        the diagonal) and `item_j`, `item_k`, `value`, the `top` (20) pairs by |q3 - mean| (GridMixin.local_dependence).  NaN in
        `q3` means no statistic: fewer than `min_pairs` (8) persons answered both items, or one item's residuals have no spread
        over them (an item nobody answered among them).  `data`: None = the training data.  The other classes refuse.  One
        rank only.  at="wle" | "ml" | "map" (VIRT / VaeIRT): Q3 at that point_estimates() score instead of the EAP (the default,
        at="eap"); a person without such an estimate (status empty or singular) enters with its EAP."""
        if self.world > 1:
            raise NotImplementedError("local_dependence with a group of %d ranks: the tables are the sums over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        return self.engine.local_dependence(self._score_data(data), **kw)

    def pair_tables(self, data=None, **kw):
        """The observed 2 x 2 table of every item pair, as int32 device tensors [items][items]: `n11`, `n10`, `n01`, `n00`, the
        persons who answered both items with a to the row item and b to the column item (GridMixin.pair_tables: exact integer
        cross products on the int8 matrix cores).  A missing cell takes its person out of that item's pairs only.  `data`: None
        = the training data; rows= as score().  VIRT / VaeIRT with any model and any x_feature -- no grid is needed -- and
        VCCDM; the other classes refuse.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("pair_tables with a group of %d ranks: the tables are the sums over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        return self.engine.pair_tables(self._score_data(data), **kw)

    def ld_x2(self, data=None, min_pairs=8, min_expected=1.0, top=20, **grid_kw):
        """Chen & Thissen's LD X2 for every item pair, ready to print beside local_dependence(): the observed 2 x 2 table of the
        persons who answered both items against the table the model predicts under the prior of score(), as a test with a
        reference distribution where Q3 is a size without one.  A dict of numpy values: `x2`, `g2`, `z` = (x2 - 1) / sqrt 2, `p`
        (the chi-square(1) tail of x2), `sign` (+1: the pair agrees more than the model says), `phi_obs`, `phi_exp`
        [items][items], `n_pairs`, `expected` [2][2][items][items] and `item_j`, `item_k`, `value`, `sign_top`, the `top` (20)
        pairs by x2 (GridMixin.ld_x2).  NaN means no statistic: the diagonal, fewer than `min_pairs` (8) persons answered both
        items, or an expected count below `min_expected` (1).
        **The statistic is taken at the item parameters as they stand.  chi-square(1) is the reference Chen & Thissen propose
        after the item parameters were ESTIMATED from these data (estimation fits the margins); at parameters that were not
        fitted to them, generating values for instance, a fully specified 2 x 2 table has up to 3 degrees of freedom and the
        statistic runs higher.  The reference is approximate in any case, as the authors say.**  The expected table assumes
        the persons who answered both items have the prior of score(): true for cells missing completely at random (booklet
        designs), not for other missingness mechanisms.  `data`: None = the training data.  VIRT / VaeIRT with x_feature <= 3,
        every IRT model (grid_kw: nodes, span), VCCDM; the other classes refuse.  Not built: polytomous tables, covariates= /
        at=, M2, more than one rank."""
        if self.world > 1:
            raise NotImplementedError("ld_x2 with a group of %d ranks: the tables are the sums over the local shard's persons; "
                                      "the cross-rank sum is not built" % self.world)
        return self.engine.ld_x2(self._score_data(data), min_pairs=min_pairs, min_expected=min_expected, top=top, **grid_kw)

    def fit_sums(self, data=None, **grid_kw):
        """The sums behind person_fit() and item_msq(), as device tensors: `person` {n, l0, e, v, sr2, sw, sz2}, each [persons],
        `item` {n, sr2, sw, sz2}, each [items], and `theta_hat` or `pattern` (GridMixin.fit_sums).  `data`: None = the training
        data; with a `group` this rank's shard.  The classes score() refuses refuse."""
        return self.engine.fit_sums(self._score_data(data), **grid_kw)

    def person_fit(self, data=None, **grid_kw):
        """Person fit, ready to print: which response vectors the model cannot explain (guessing, copying, carelessness, a
        booklet keyed with the wrong form).  For every person in `data` (None: the training data; with a `group` this rank's
        shard, as score()), over the items the person answered and at the person's point estimate -- the EAP of score() for VIRT
        / VaeIRT (every model, x_feature <= 3), the MAP pattern for VCCDM -- under the item parameters as they stand, numpy
        arrays [persons]: `lz` (the standardised log-likelihood of Drasgow, Levine and Williams: large negative values are
        misfit), `infit` and `outfit` (the information-weighted and the plain mean square of the standardised residuals: about
        1 under the model), `n_obs` (int64, the answered items), `loglik0`, `expected`, `variance` (the log-likelihood at the
        estimate, its mean and its variance under the model: lz = (loglik0 - expected) / sqrt(variance)) and `theta_hat` or
        `pattern`.  lz is taken at the estimate WITHOUT Snijders' correction: its null distribution is somewhat narrower than
        N(0, 1) on short tests.  NaN for a person who answered nothing.  The other classes refuse.
        at="wle" | "ml" | "map" (VIRT / VaeIRT): the statistics at that point_estimates() score -- the likelihood-based estimate
        lz and the mean squares are defined at -- instead of the EAP (the default, at="eap", whose shrinkage biases the residuals
        of extreme persons); NaN then also for a person without such an estimate (status empty or singular)."""
        return self.engine.person_fit(self._score_data(data), **grid_kw)

    def item_msq(self, data=None, **grid_kw):
        """The residual mean squares of every item over the persons in `data` (None: the training data), numpy arrays [items]:
        `infit`, `outfit` (about 1 under the model; residuals and point estimates as person_fit()) and `n_obs` (int64, the
        persons who answered the item); NaN for an item nobody answered.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("item_msq with a group of %d ranks: fit_sums() gives the local shard's sums; the "
                                      "cross-rank sum is not built" % self.world)
        return self.engine.item_msq(self._score_data(data), **grid_kw)

    def sumscore_tables(self, data=None, items=None, **grid_kw):
        """The summed-score tables behind sx2() and score_table(), as device tensors: the model's `e1`, `e0` [items][items + 1]
        and `dist` [nodes][items + 1] by the Lord-Wingersky recursion, the observed `o1`, `n` and `score` over the complete
        persons of `data` (None: the training data), and `items`, `theta`, `logw` (GridMixin.sumscore_tables).  `items`: a sorted
        list of distinct item indices, at most 1023 (default: all).  VIRT / VaeIRT with x_feature <= 3 (grid_kw: nodes, span),
        VCCDM; the other classes refuse.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("sumscore_tables with a group of %d ranks: the tables are the sums over the local shard's "
                                      "persons; the cross-rank sum is not built" % self.world)
        return self.engine.sumscore_tables(self._score_data(data), items, **grid_kw)

    def sx2(self, data=None, items=None, min_expected=1.0, **grid_kw):
        """Orlando & Thissen's S-X2 item-fit test, ready to print beside the item parameters: for every listed item the
        statistic `sx2`, its `df`, the chi-square tail probability `p` and `n_cells`, with `observed` and `expected`
        [items][items + 1], the proportions correct per summed-score group, `n_persons`, `n_dropped` and `items`
        (GridMixin.sx2).  Within each summed-score group the observed proportion correct is compared with the one the model
        predicts for that group (Lord-Wingersky); the cells are observable, so the statistic has a chi-square reference, which
        the RMSD of item_fit() has not.  Score groups are collapsed by one left-to-right sweep until both expected counts of a
        cell reach min_expected -- this project's own rule; other packages merge in other orders.  Only persons who answered
        every listed item count: for a test with cells missing by design pass one booklet's items as items=; ValueError when no
        person is complete.  `data`: None = the training data.  VIRT / VaeIRT with x_feature <= 3, every IRT model (grid_kw:
        nodes, span), VCCDM; the other classes refuse.  covariates= is not built.  One rank only."""
        if self.world > 1:
            raise NotImplementedError("sx2 with a group of %d ranks: the tables are the sums over the local shard's persons; the "
                                      "cross-rank sum is not built" % self.world)
        return self.engine.sx2(self._score_data(data), items, min_expected, **grid_kw)

    def score_table(self, items=None, **grid_kw):
        """The summed-score -> latent conversion table a testing programme publishes, numpy float64: `score` [items + 1], `prob`
        = the model's P(score = s), and for VIRT / VaeIRT `eap`, `psd` [items + 1][x_feature], for VCCDM `attr_prob`
        [items + 1][K]: what score() would say of a person of whom only the summed score over `items` is known
        (GridMixin.score_table).  Takes no data.  Classes and refusals as sx2().  One rank only."""
        if self.world > 1:
            raise NotImplementedError("score_table with a group of %d ranks is not built: every rank holds the item parameters; "
                                      "ask one" % self.world)
        return self.engine.score_table(items, **grid_kw)


class BaseIRT(BasePsy):
    """vi.py:536-656 (constructor kwargs identical: model, x_feature, share_cov, D, a_free, a0, b0)."""

    amortized = False

    def __init__(self, model="irt_2pl", x_feature=1, share_cov=False, D=1, hidden_dim=64, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._model, self.x_feature, self.share_cov, self.D = model, int(x_feature), share_cov, D
        self.engine = IrtEngine(self.data, model=model, D=self.x_feature, Dc=float(D), amortized=self.amortized,
                                H=hidden_dim, share_cov=share_cov, a_free=self.kwargs.get("a_free"),
                                a0=self.kwargs.get("a0"), b0=self.kwargs.get("b0"),
                                encoder_init=self.kwargs.get("encoder_init"),
                                observed_lists=self.kwargs.get("observed_lists", True),
                                estimator=self.kwargs.get("estimator", "pathwise"),      # 'score': north_star's REINFORCE mode
                                baseline=self.kwargs.get("baseline", "none"),
                                baseline_beta=self.kwargs.get("baseline_beta", 0.9), **self._eng_kw)
        self._register()
        self._ri = None
        self._S, self._loo_left = 1, 0

    def fit(self, optim=None, loss=None, max_iter=5000, random_instance=None, progress=True):
        """vi.py:627-656 (defaults Adam lr 5e-2, Trace_ELBO(1), 5000 iterations).  Returns the last loss."""
        optim = optim if optim is not None else Adam({"lr": 5e-2})
        loss = loss if loss is not None else Trace_ELBO(num_particles=1)
        self._ri = random_instance
        self._S, self._loo_left = max(1, getattr(loss, "num_particles", 1)), 0
        return self._loop(optim, loss, max_iter, progress)

    def _subsample(self):
        if self.engine.estimator == "score" and self.engine.baseline == "loo":   # the particles of a step share one subsample
            if self._loo_left == 0:
                self._loo_cache, self._loo_left = super()._subsample(), self._S
            self._loo_left -= 1
            return self._loo_cache
        return super()._subsample()

    def _postfix(self):
        ri, out = self._ri, {}
        if ri is None:
            return out
        dev = self.device
        out["threshold_error"] = "{0:.4f}".format(float((param("b") - ri.b.to(dev)).abs().mean()))      # vi.py:645
        if self._model != "irt_1pl":
            d = self.x_feature
            den = d * self.item_size - d * (d - 1) / 2
            out["slop_error"] = "{0:.4f}".format(float((param("a") - ri.a.to(dev)).abs().sum() / den))  # vi.py:648
        if self._model in ("irt_3pl", "irt_4pl"):
            out["guess_error"] = "{0:.4f}".format(float((param("c") - ri.c.to(dev)).abs().mean()))
        if self._model == "irt_4pl":
            out["slip_error"] = "{0:.4f}".format(float((param("d") - ri.d.to(dev)).abs().mean()))
        return out


class VIRT(BaseIRT):
    """Black-box VI with per-person variational rows (vi.py:696-723)."""
    amortized = False


class VaeIRT(BaseIRT):
    """Amortized VI with the NormEncoder / MvnEncoder guide (vi.py:659-693)."""
    amortized = True


class _HoDinaBase(BasePsy):
    amortized = False

    def __init__(self, q, hidden_dim=64, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.q = q
        self.attr_size = int(q.shape[0])
        self.engine = HoDinaEngine(self.data, q, amortized=self.amortized, H=hidden_dim,
                                   encoder_init=self.kwargs.get("encoder_init"), **self._eng_kw)
        self._register()
        self._ri = None

    def fit(self, optim=None, loss=None, max_iter=50000, random_instance=None, progress=True):
        """vi.py:936-958 (defaults Adam lr 5e-3, TraceEnum_ELBO(1), 50000 iterations).  The reference runs
        a second evaluate_loss per iteration only to display it (vi.py:942); the step's own loss is shown."""
        optim = optim if optim is not None else Adam({"lr": 5e-3})
        loss = loss if loss is not None else TraceEnum_ELBO(num_particles=1)
        self._ri = random_instance
        return self._loop(optim, loss, max_iter, progress)

    def _postfix(self):
        ri, out = self._ri, {}
        if ri is None:
            return out
        for n in ("g", "s", "lam0", "lam1"):
            out[n] = "{0:.4f}".format(float((param(n) - getattr(ri, n).to(self.device)).abs().mean()))   # vi.py:953-956
        return out


class VCHoDina(_HoDinaBase):
    """vi.py:894-958."""
    amortized = False


class VaeCHoDina(_HoDinaBase):
    """vi.py:961-981."""
    amortized = True


class _CdmSfBase(BasePsy):
    """BaseCDM (vi.py:726-782) with a Bernoulli guide: the score-function (REINFORCE) estimator of pyro's Trace_ELBO.
    Extra keyword arguments of this build: attr_prior (None = the reference's Bernoulli(1.5) prior, vi.py:753; a float
    p = Bernoulli(p)), baseline ('none' = pyro; 'avg' = per-person decaying average; 'loo' = leave-one-out over the
    particles), baseline_beta."""

    amortized = False

    def __init__(self, q=None, model="dina", hidden_dim=64, *args, **kwargs):
        if q is None or kwargs.get("data") is None:
            raise NotImplementedError("%s needs q and data (vi.py:733-743)" % type(self).__name__)
        super().__init__(*args, **kwargs)
        self.q, self._model = q, model
        self.attr_size = int(q.shape[0])
        self.engine = CdmSfEngine(self.data, q, cdm=model, amortized=self.amortized, H=hidden_dim,
                                  encoder_init=self.kwargs.get("encoder_init"), attr_prior=self.kwargs.get("attr_prior"),
                                  baseline=self.kwargs.get("baseline", "none"),
                                  baseline_beta=self.kwargs.get("baseline_beta", 0.9), **self._eng_kw)
        self._register()
        self._ri = None

    def fit(self, optim=None, loss=None, max_iter=5000, random_instance=None, progress=True):
        """vi.py:758-782 (defaults Adam lr 1e-3, Trace_ELBO(1), 5000 iterations).  The reference evaluates the loss a
        second time per iteration only to display it (vi.py:770); the step's own loss is shown."""
        optim = optim if optim is not None else Adam({"lr": 1e-3})
        loss = loss if loss is not None else Trace_ELBO(num_particles=1)
        self._ri = random_instance
        self._S, self._loo_left = max(1, getattr(loss, "num_particles", 1)), 0
        return self._loop(optim, loss, max_iter, progress)

    def _subsample(self):
        if self.engine.baseline == "loo":                 # the particles of a step share one subsample
            if self._loo_left == 0:
                self._loo_cache, self._loo_left = super()._subsample(), self._S
            self._loo_left -= 1
            return self._loo_cache
        return super()._subsample()

    def _postfix(self):
        ri, out = self._ri, {}
        if ri is None:
            return out
        for n in ("g", "s"):
            out[n] = "{0:.4f}".format(float((param(n) - getattr(ri, n).to(self.device)).abs().mean()))   # vi.py:775-779
        return out


class VCDM(_CdmSfBase):
    """Black-box VI for DINA / DINO with per-person Bernoulli guide rows `attr_p` (vi.py:807-816)."""
    amortized = False


class VaeCDM(_CdmSfBase):
    """Amortized VI for DINA / DINO with the BinEncoder guide (vi.py:785-804, 458-470).  Positional order as in the
    reference: (hidden_dim, q, model) (vi.py:785-793)."""
    amortized = True

    def __init__(self, hidden_dim=64, q=None, model="dina", *args, **kwargs):
        super().__init__(q, model, hidden_dim, *args, **kwargs)


class VCCDM(BasePsy):
    """Pattern-enumerated DINA / DINO with the uniform pattern prior (vi.py:819-865; BaseCDM ctor vi.py:733-743:
    q, model='dina'|'dino'; fit defaults vi.py:758, 863-864: Adam lr 1e-3, TraceEnum_ELBO(1), 5000 iterations)."""

    def __init__(self, q=None, model="dina", *args, **kwargs):
        if q is None or kwargs.get("data") is None:
            raise NotImplementedError("VCCDM needs q and data (vi.py:733-743)")
        super().__init__(*args, **kwargs)
        self.q, self._model = q, model
        self.attr_size = int(q.shape[0])
        self.engine = CcdmEngine(self.data, q, cdm=model, **self._eng_kw)
        self._register()
        self._ri = None

    def fit(self, optim=None, loss=None, max_iter=5000, random_instance=None, progress=True):
        optim = optim if optim is not None else Adam({"lr": 1e-3})
        loss = loss if loss is not None else TraceEnum_ELBO(num_particles=1)
        self._ri = random_instance
        return self._loop(optim, loss, max_iter, progress)

    def _postfix(self):
        ri, out = self._ri, {}
        if ri is None:
            return out
        for n in ("g", "s"):
            out[n] = "{0:.4f}".format(float((param(n) - getattr(ri, n).to(self.device)).abs().mean()))   # vi.py:775-779
        return out


class VaeCCDM(VCCDM):
    """Pattern-enumerated DINA / DINO with the SoftmaxEncoder prior inside the model (vi.py:866-891, 473-485); as in the
    reference the encoder's softmax normalises over the persons of the batch and missing responses enter the likelihood as -1."""

    def __init__(self, hidden_dim=64, q=None, model="dina", *args, **kwargs):
        if q is None or kwargs.get("data") is None:
            raise NotImplementedError("VaeCCDM needs q and data (vi.py:733-743)")
        BasePsy.__init__(self, *args, **kwargs)
        self.q, self._model = q, model
        self.attr_size = int(q.shape[0])
        self.engine = VaeCcdmEngine(self.data, q, cdm=model, H=hidden_dim, encoder_init=self.kwargs.get("encoder_init"),
                                    **self._eng_kw)
        self._register()
        self._ri = None


def rmse_(item_size, model_name, r, x_feature):
    """The reference's error metric (test.py:70-91) -- a mean ABSOLUTE error despite the name."""
    out = {}
    if model_name in ("irt_2pl", "irt_3pl", "irt_4pl"):
        a = param("a")
        out["a"] = float((a - r.a.to(a.device)).abs().sum() / (x_feature * item_size - x_feature * (x_feature - 1) / 2))
    b = param("b")
    out["b"] = float((b - r.b.to(b.device)).abs().mean())
    if model_name in ("irt_3pl", "irt_4pl"):
        c = param("c")
        out["c"] = float((c - r.c.to(c.device)).abs().mean())
    if model_name == "irt_4pl":
        d = param("d")
        out["d"] = float((d - r.d.to(d.device)).abs().mean())
    return out


# north_star spelling of the same surface (name map)
def Irt2PL(amortized=False, **kw):
    return (VaeIRT if amortized else VIRT)(model="irt_2pl", **kw)


def Irt4PL(amortized=False, **kw):
    return (VaeIRT if amortized else VIRT)(model="irt_4pl", **kw)


def IrtMultiDim(x_feature, model="irt_2pl", **kw):
    return VaeIRT(model=model, x_feature=x_feature, **kw)


def Dina(amortized=False, enumerate=True, model="dina", **kw):
    """The DINA / DINO surface: pattern-enumerated (`VCCDM` / `VaeCCDM`, what the reference's PaDina tests run,
    test.py:558-566) or the Bernoulli-guide score-function classes (`VCDM` / `VaeCDM`, test.py:520-550)."""
    if enumerate:
        return (VaeCCDM if amortized else VCCDM)(model=model, **kw)
    return (VaeCDM if amortized else VCDM)(model=model, **kw)


def HoDina(amortized=False, **kw):
    return (VaeCHoDina if amortized else VCHoDina)(**kw)

