"""Differential item functioning on the GPU: vx_grid_counts_cond (k_grid_counts_cond.hip) directly, behind
expected_counts(covariates=) / item_fit(covariates=), and behind group_counts() / dif() of IrtEngine, CcdmEngine and the model
classes, against the float64 oracle of tests/dif_cases.py.

Every table is held to the oracle by the rule of its case (dif_cases.rule_of: C_RULE = 8 times what the float32 + fp16-pair
method costs on that case when said again in numpy, tests/test_dif_host.py), one row = one item of one segment, mass one row a
segment; rmsd and md absolutely, observed as the rule reaches a ratio.  The errors found are printed beside the rule.  Engines
are set up as tests/test_gpu_score.py does it: drawn parameters copied into the engine's views, nothing trained."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dif_cases as dc
from tests import pop_cases as pc
from tests import score_cases as sc
from tests.test_gpu_parity import _dev
from tests.test_gpu_score import _ccdm_engine, _irt_engine, _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(_dev())


def _kernel(eng, cs, tilt=None, rows=None, seg_start=None):
    """vx_grid_posterior_cond for logjoint and vx_grid_counts_cond over a kernel case (or a variant of its tilt / rows / segments)."""
    rows = cs["rows"] if rows is None else rows
    call = eng._grid_call(None, _t(rows), cs["nodes"], cs["span"])._replace(logw=_t(cs["lw"]))
    out = eng._grid_counts_cond(call, _t(cs["tilt"] if tilt is None else tilt), cs["seg_start"] if seg_start is None else seg_start)
    torch.cuda.synchronize()
    return out


def _hold(tag, got, want, rule):
    errs = dc.table_errors({k: _np(got[k]) for k in ("n1", "n0", "mass")}, want)
    errs["prob"] = (float(np.abs(_np(got["prob"]).astype(np.float64) - want["prob"]).max()), -1)
    print("%s: %s (rule %.2e; the largest is %.2f of it)" % (tag, "  ".join("%s %.2e" % (k, v[0]) for k, v in errs.items()), rule,
                                                             max(v[0] for v in errs.values()) / rule))
    for k, (e, worst) in errs.items():
        assert e <= rule, (tag, k, "row", worst, e, rule)
    return max(v[0] for v in errs.values()) / rule


@pytest.mark.parametrize("key", list(dc.KCASES))
def test_tables_of_every_segment_vs_oracle(key):
    cs, want, rule = dc.kcase(key), dc.koracle(key), dc.krule(key)
    S, J, G = len(cs["seg_start"]) - 1, cs["J"], cs["theta"].shape[0]
    got = _kernel(_irt_engine(cs), cs)
    assert tuple(got["n1"].shape) == (S, J, G) and tuple(got["n0"].shape) == (S, J, G) and tuple(got["mass"].shape) == (S, G)
    assert all(got[k].dtype == torch.float32 for k in ("n1", "n0", "mass"))
    _hold(cs["name"], got, want, rule)
    n = np.diff(cs["seg_start"]).astype(np.float64)
    mass = _np(got["mass"]).astype(np.float64).sum(1)
    print("    sum of a segment's mass against its persons: %.2e" % (np.abs(mass - n) / np.maximum(n, 1.0)).max())
    assert (np.abs(mass - n) / np.maximum(n, 1.0)).max() <= rule
    for s in np.flatnonzero(n == 0):                                          # an empty segment: exact zeros
        assert (_np(got["n1"])[s] == 0).all() and (_np(got["n0"])[s] == 0).all() and (_np(got["mass"])[s] == 0).all()
    y = cs["y"][cs["rows"]]
    for s in range(S):                                                        # a cell nobody of the segment filled is exactly zero
        ys = y[cs["seg_start"][s]:cs["seg_start"][s + 1]]
        assert (_np(got["n1"])[s][(ys == 1).sum(0) == 0] == 0).all() and (_np(got["n0"])[s][(ys == 0).sum(0) == 0] == 0).all()


@pytest.mark.parametrize("key", dc.BITWISE)
def test_one_segment_and_a_zero_tilt_are_the_unconditioned_bits(key):
    """The same y, rows, img and logw, logjoint = vx_grid_posterior's loglik: the three tables of vx_grid_counts bit for bit, on one
    case for each template instance (IT = 1, 2, 4)."""
    cs = dc.kcase(key)
    eng = _irt_engine(cs)
    be, n, J, G, D = eng.be, cs["N"], cs["J"], cs["theta"].shape[0], cs["D"]
    call = eng._grid_call(None, _t(cs["rows"]), cs["nodes"], cs["span"])._replace(logw=_t(cs["lw"]))
    post = eng._grid_posterior(call)
    f32 = dict(dtype=torch.float32, device=_dev())
    a = {"n1": torch.empty(J, G, **f32), "n0": torch.empty(J, G, **f32), "mass": torch.empty(G, **f32)}
    be.grid_counts(call.y, call.rows, n, J, G, post["img"], call.logw, post["loglik"], a["n1"], a["n0"], a["mass"],
                   torch.empty(be.grid_counts_workspace(n, J, G), **f32))
    b = {"n1": torch.full((1, J, G), -1.0, **f32), "n0": torch.full((1, J, G), -1.0, **f32), "mass": torch.full((1, G), -1.0, **f32)}
    be.grid_counts_cond(call.y, call.rows, n, J, G, D, post["img"], call.logw, call.theta, torch.zeros(n, D, **f32), post["loglik"],
                        np.array([0, n], np.int64), b["n1"], b["n0"], b["mass"],
                        torch.empty(be.grid_counts_cond_workspace(n, 1, J, G), **f32))
    torch.cuda.synchronize()
    assert float(a["mass"].sum()) > 0.99 * n
    for k in ("n1", "n0", "mass"):
        assert torch.equal(a[k], b[k][0]), (key, k, float((a[k] - b[k][0]).abs().max()))
    # ... and through the host layer, whose zero tilt (tilt None) takes one zero coordinate a node
    c = eng._grid_counts_cond(call, None, np.array([0, n], np.int64))
    torch.cuda.synchronize()
    for k in ("n1", "n0", "mass"):
        assert torch.equal(a[k], c[k][0]), (key, k)


def test_same_bits_twice_and_segments_do_not_see_each_other():
    cs = dc.kcase("K1")
    eng = _irt_engine(cs)
    a, b = _kernel(eng, cs), _kernel(eng, cs)
    for k in ("n1", "n0", "mass"):
        assert torch.equal(a[k], b[k]), k
    # the rows of the last two segments (600 and 1 100 persons) reordered within their segments, their tilts with them: every
    # other segment keeps its bits; the reordered ones change the order of their sums and are held to the rule
    seg = cs["seg_start"]
    perm = np.arange(cs["N"])
    rng = np.random.RandomState(5)
    for s in (6, 7):
        perm[seg[s]:seg[s + 1]] = seg[s] + rng.permutation(seg[s + 1] - seg[s])
    c = _kernel(eng, cs, tilt=cs["tilt"][perm], rows=cs["rows"][perm])
    for k in ("n1", "n0", "mass"):
        assert torch.equal(a[k][:6], c[k][:6]), k
        assert not torch.equal(a[k][6:], c[k][6:]), k
    _hold("K1, two segments reordered", c, dc.koracle("K1"), dc.krule("K1"))
    # the segments of a call alone: every segment as a call of its own (one segment) gives the bits it has in the joint call
    # (the two plans cut these segments alike: 1 100 persons are chunks of three and two rounds either way)
    for s in (1, 3, 7):
        lo, hi = int(seg[s]), int(seg[s + 1])
        one = _kernel(eng, cs, tilt=cs["tilt"][lo:hi], rows=cs["rows"][lo:hi], seg_start=np.array([0, hi - lo], np.int64))
        for k in ("n1", "n0", "mass"):
            assert torch.equal(one[k][0], a[k][s]), (s, k)


@pytest.mark.parametrize("key", ["P1", "P2"])
def test_expected_counts_under_the_fitted_population(key):
    """expected_counts(covariates=) / item_fit(covariates=) under pop_cases' population (the oracle's own EM fit, eight iterations)."""
    from tests import count_cases as cc
    cs = pc.case(key)
    theta, ll = pc.grid_ll(key)
    fit = pc.em_oracle(key, 8)
    e = pc.estep(ll, theta, cs["X"], fit["gamma"], fit["sigma"])
    lw, tilt, _ = pc.population_prior(theta, cs["X"], fit["gamma"], fit["sigma"])
    seg = np.array([0, cs["N"]], np.int64)
    want = dc.segment_counts(ll, theta, lw, tilt, cs["y"], seg)
    want["prob"] = dc.prob_of(cs, theta)
    assert np.allclose(want["logjoint"], e["logjoint"])
    rule = dc.rule_of(dc.restated_error(want, theta, lw, tilt, cs["y"], seg))
    eng = _irt_engine(cs)
    base = eng.expected_counts(nodes=cs["nodes"], span=cs["span"])
    with pytest.raises(ValueError):
        eng.expected_counts(nodes=cs["nodes"], span=cs["span"], covariates=cs["cov"])          # no population yet
    eng.population = {"gamma": fit["gamma"], "sigma": fit["sigma"], "intercept": True}
    got = eng.expected_counts(nodes=cs["nodes"], span=cs["span"], covariates=cs["cov"])
    fitg = eng.item_fit(nodes=cs["nodes"], span=cs["span"], covariates=cs["cov"])
    torch.cuda.synchronize()
    J, G = cs["J"], theta.shape[0]
    assert set(got) == {"n1", "n0", "mass", "prob", "theta", "logw"} and tuple(got["n1"].shape) == (J, G) and tuple(got["mass"].shape) == (G,)
    _hold(cs["name"] + " expected_counts(covariates=)", {k: (got[k][None] if k != "prob" else got[k]) for k in ("n1", "n0", "mass", "prob")},
          want, rule)
    ws = cc.fit_stats(want["n1"][0], want["n0"][0], want["prob"])
    for k in ("md", "rmsd"):
        err = float(np.nanmax(np.abs(_np(fitg[k]) - ws[k])))
        print("    %s %.2e" % (k, err))
        assert err <= rule
    # a population that is not N(0, I) moves the tables; without covariates nothing has changed, bits included
    assert float((got["n1"] - base["n1"]).abs().max()) > 100 * rule
    again = eng.expected_counts(nodes=cs["nodes"], span=cs["span"])
    for k in ("n1", "n0", "mass", "prob", "logw"):
        assert torch.equal(base[k], again[k]), k
    # rows pick the covariates with the responses
    idx = np.random.RandomState(3).choice(cs["N"], size=41, replace=False).astype(np.int64)
    sub = eng.expected_counts(rows=idx, nodes=cs["nodes"], span=cs["span"], covariates=cs["cov"])
    wsub = dc.segment_counts(ll[idx], theta, lw, tilt[idx], cs["y"][idx], np.array([0, 41], np.int64))
    wsub["prob"] = want["prob"]
    _hold(cs["name"] + " rows", {k: (sub[k][None] if k != "prob" else sub[k]) for k in ("n1", "n0", "mass", "prob")}, wsub, rule)


# ---- dif() end to end on the planted case --------------------------------------------------------------------------------
def _planted_model():
    from vipsy_amd import vi
    cs = dc.planted()
    vi.clear_param_store()
    m = vi.VIRT(data=torch.from_numpy(cs["y"]).to(_dev()), model="irt_2pl", x_feature=1)
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    return cs, m


def _hold_dif(tag, got, want, rule):
    H, J, G = want["n1"].shape
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["n_group"], np.diff(want["seg_start"]))
    assert got["n_obs"].dtype == np.int64 and np.array_equal(got["n_obs"], want["n_obs"])
    assert got["rmsd"].shape == got["md"].shape == (H, J) and got["observed"].shape == (H, J, G) and got["prob"].shape == (J, G)
    assert got["mass"].shape == (H, G) and all(isinstance(v, np.ndarray) for v in got.values())
    errs = {}
    for k in ("rmsd", "md"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (tag, k)
        errs[k] = float(np.nanmax(np.abs(got[k] - want[k])))
    errs["prob"] = float(np.abs(got["prob"] - want["prob"]).max())
    errs["mass"] = dc._row_errors(got["mass"].astype(np.float64), want["mass"], floor=1.0)[0]
    n = want["n1"] + want["n0"]
    rowmax = np.maximum(np.abs(want["n1"]).max(-1), np.abs(want["n0"]).max(-1))
    errs["observed"] = dc.ratio_errors(got["observed"], want["observed"], n, rowmax)
    print("%s: %s (rule %.2e)" % (tag, "  ".join("%s %.2e" % kv for kv in errs.items()), rule))
    for k, e in errs.items():
        assert e <= rule, (tag, k, e, rule)


def test_dif_on_the_planted_case():
    cs, m = _planted_model()
    flat_w = dc.planted_oracle(False)
    rule_flat = dc.rule_of(dc.restated_error(flat_w, flat_w["theta"], flat_w["lw"], flat_w["tilt"], flat_w["y"], flat_w["seg_start"]))
    flat = m.dif(cs["groups"], impact=False)
    _hold_dif("planted, impact=False", flat, flat_w, rule_flat)
    assert np.array_equal(flat["group_mean"], np.zeros((2, 1))) and np.array_equal(flat["sigma"], np.eye(1))
    # impact=True (the default): the fitted population against the oracle's, the tables under the population dif() reports
    own = m.dif(cs["groups"])
    ref = dc.planted_oracle(True)
    print("group means %s (oracle %s), sigma %.4f (oracle %.4f)" % (own["group_mean"].ravel(), ref["group_mean"].ravel(),
                                                                    own["sigma"][0, 0], ref["sigma"][0, 0]))
    assert np.abs(own["group_mean"] - ref["group_mean"]).max() <= dc.POP_TOL and np.abs(own["sigma"] - ref["sigma"]).max() <= dc.POP_TOL
    own_w = dc.planted_oracle(True, prior=(own["group_mean"], own["sigma"]))
    rule_own = dc.rule_of(dc.restated_error(own_w, own_w["theta"], own_w["lw"], own_w["tilt"], own_w["y"], own_w["seg_start"]))
    _hold_dif("planted, impact=True", own, own_w, rule_own)
    assert m.engine.population is None                                        # the private fit is not kept
    # the top cells, where the oracle's gaps exceed twice the rule
    for got, want, rule in ((flat, flat_w, rule_flat), (own, own_w, rule_own)):
        keep = dc.top_cells(want["rmsd"], 20, 2.0 * rule)
        assert len(got["group"]) == 16 and len(keep) >= 4
        assert list(zip(got["group"].tolist(), got["item"].tolist()))[:len(keep)] == keep
        assert np.array_equal(got["value"], got["rmsd"][got["group"], got["item"]]) and (np.diff(got["value"]) <= 0).all()
    assert (own["group"][0], own["item"][0]) == (dc.PLANT_GROUP, dc.PLANT_ITEM)
    # the statistical claim on what the GPU returned
    c = dc.clean_cells()
    print("clean max / planted with the groups' own priors: %.4f / %.4f; under N(0, I): %.4f / %.4f; t = %.3f" % (
        own["rmsd"][c].max(), own["rmsd"][dc.PLANT_GROUP, dc.PLANT_ITEM], flat["rmsd"][c].max(), flat["rmsd"][dc.PLANT_GROUP, dc.PLANT_ITEM],
        dc.PLANT_T))
    assert dc.claim(own["rmsd"], flat["rmsd"]) == (True, True, True)
    # NaN below min_obs, top = 3, and group_counts(): the device tensors behind the same statistics
    few = m.dif(cs["groups"], impact=False, min_obs=dc.PLANT_MIN_OBS, top=3)
    _hold_dif("planted, min_obs=%d" % dc.PLANT_MIN_OBS, few, dc.planted_oracle(False, min_obs=dc.PLANT_MIN_OBS), rule_flat)
    assert np.isnan(few["rmsd"]).any() and np.isfinite(few["rmsd"]).any() and len(few["value"]) == 3 and np.isfinite(few["value"]).all()
    gc = m.group_counts(cs["groups"], impact=False)
    assert all(torch.is_tensor(gc[k]) and gc[k].is_cuda for k in ("n1", "n0", "mass", "prob"))
    assert tuple(gc["n1"].shape) == (2, cs["J"], dc.PLANT_NODES) and np.array_equal(gc["labels"], dc.PLANT_LABELS)
    assert np.array_equal(_np(gc["mass"]), flat["mass"])
    _hold("planted, group_counts", gc, flat_w, rule_flat)
    # labels are labels: other integers, another order of the persons, the same groups
    perm = np.random.RandomState(8).permutation(cs["N"])
    other = m.dif(np.where(cs["groups"][perm] == dc.PLANT_LABELS[0], -7, 40), data=cs["y"][perm], impact=False)
    assert other["labels"].tolist() == [-7, 40] and np.array_equal(other["n_obs"], flat["n_obs"])
    assert np.abs(other["rmsd"] - flat["rmsd"]).max() <= 2 * rule_flat


def test_dif_under_engine_population():
    """covariates=: the population on the engine as it stands (here the oracle's group fit as a regression on the group dummy)."""
    cs, m = _planted_model()
    ref = dc.planted_oracle(True)
    gamma = np.array([ref["group_mean"][0], ref["group_mean"][1] - ref["group_mean"][0]])
    m.engine.population = {"gamma": gamma, "sigma": ref["sigma"], "intercept": True}
    got = m.dif(cs["groups"], covariates=cs["group"].astype(np.float64)[:, None])
    rule = dc.rule_of(dc.restated_error(ref, ref["theta"], ref["lw"], ref["tilt"], ref["y"], ref["seg_start"]))
    _hold_dif("planted, covariates=", got, ref, rule)
    assert np.abs(got["group_mean"] - ref["group_mean"]).max() < 1e-6 and np.array_equal(got["sigma"], ref["sigma"])


@pytest.mark.parametrize("newton", [1, 8])
def test_refit_vs_the_oracle_mstep(newton):
    """Every group's items by `newton` steps from the pooled values on that group's tables, against em_cases.newton_mstep on the
    oracle's tables under the population dif() reports: ROW_TOL on a and b, the rule of fit_em's iteration (tests/test_gpu_em.py)
    -- the float32 chain said again in numpy stays below 6e-7 (tests/test_dif_host.py)."""
    cs, m = _planted_model()
    got = m.dif(cs["groups"], refit=True, newton=newton)
    want = dc.planted_oracle(True, newton=newton, prior=(got["group_mean"], got["sigma"]))
    assert got["b_group"].shape == (2, cs["J"]) and got["a_group"].shape == (2, 1, cs["J"]) and got["delta_b"].shape == (2, cs["J"])
    eb, ea = np.abs(got["b_group"] - want["b_group"]).max(), np.abs(got["a_group"] - want["a_group"]).max()
    print("refit, newton %d: b %.2e  a %.2e (rule %.1e); delta_b of the planted cell %.3f" % (newton, eb, ea, dc.ROW_TOL,
                                                                                             got["delta_b"][dc.PLANT_GROUP, dc.PLANT_ITEM]))
    assert eb <= dc.ROW_TOL and ea <= dc.ROW_TOL
    assert np.abs(got["delta_b"] - (got["b_group"] - cs["params"]["b"].astype(np.float64))).max() == 0
    assert got["delta_b"][dc.PLANT_GROUP, dc.PLANT_ITEM] > 0.3
    # nothing of the engine changed
    assert np.array_equal(_np(m.engine.unconstrained("b")), cs["params"]["b"]) and np.array_equal(_np(m.engine.unconstrained("a")), cs["params"]["a"])


def test_vccdm_dif():
    from vipsy_amd import vi
    cs, want = dc.cdm_oracle(sc.CDM_CASES[0])
    y = cs["y"][np.argsort(np.unique(want["groups"], return_inverse=True)[1], kind="stable")]
    C = 1 << cs["K"]
    rule = dc.rule_of(dc.restated_error(want, np.zeros((C, 1)), np.full(C, np.log(1.0 / C)), np.zeros((len(y), 1)), y, want["seg_start"]))
    vi.clear_param_store()
    m = vi.VCCDM(data=torch.from_numpy(cs["y"]).to(_dev()), q=torch.from_numpy(cs["q"]), model=cs["cdm"])
    for name, v in cs["params"].items():
        m.engine.unconstrained(name).copy_(torch.from_numpy(v).to(_dev()))
    got = m.dif(want["groups"])
    assert "group_mean" not in got and "sigma" not in got
    _hold_dif("%s dif" % cs["name"], got, want, rule)
    assert np.array_equal(m.dif(want["groups"], impact=False)["rmsd"], got["rmsd"], equal_nan=True)
    gc = m.engine.group_counts(want["groups"])
    _hold("%s group_counts" % cs["name"], gc, want, rule)
    for kw in ({"impact": True}, {"covariates": np.zeros((cs["N"], 1))}, {"refit": True}):
        with pytest.raises(NotImplementedError):
            m.dif(want["groups"], **kw)


def test_classes_out_of_scope_refuse():
    from vipsy_amd import vi
    rng = np.random.RandomState(2)
    y = (rng.uniform(size=(64, 12)) < 0.5).astype(np.uint8)
    q = sc.cdm_q(3, 12, rng)
    g = np.arange(64) % 2
    vi.clear_param_store()
    yd = torch.from_numpy(y).to(_dev())
    for m in (vi.VCHoDina(data=yd, q=torch.from_numpy(q)), vi.VaeCCDM(data=yd, q=torch.from_numpy(q)),
              vi.VCDM(data=yd, q=torch.from_numpy(q)), vi.VaeIRT(data=yd, model="irt_2pl", x_feature=4)):
        with pytest.raises(NotImplementedError) as want:
            m.score()
        for call in (m.dif, m.group_counts):
            with pytest.raises(NotImplementedError) as e:
                call(g)
            assert str(e.value) == str(want.value)


def test_two_ranks_refuse(tmp_path):
    """A gloo group of two: the model class and the engine both refuse, before anything is computed."""
    worker = os.path.join(ROOT, "tests", "_dif_dist_worker.py")
    out = str(tmp_path / "dif_refusal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29667", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29667", worker, out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for r in range(2):
        with open(out + ".%d" % r) as f:
            assert f.read().split() == ["NotImplementedError"] * 4
