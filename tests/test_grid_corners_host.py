"""The corner cases of the grid family (tests/corner_cases.py), the parts that need no GPU: the conditions under which the float64
oracle is a fair yardstick there and the rules of tests/test_gpu_grid_corners.py are sound -- checked on the oracle and on the
numpy restatement of the operand phase alone, never on what a kernel returned.  For every case: the node rule leaves out at
most ARGMAX_LEFT_OUT of the persons and of the (person, draw) pairs at the case's gap threshold; irt_condition holds where it is
asked; the row rule max(ROW_TOL, 3 e_restated) stays below four float32 spacings of the accumulated log-likelihood and is
ROW_TOL itself wherever nobody answered more than 130 items.  e_restated, tol, d_f and the gap threshold are printed per case."""
import numpy as np
import pytest

from tests import corner_cases as co
from tests import score_cases as sc
from tests.test_gpu_response_designs import ROW_TOL            # 3e-5, the project's row rule


def test_the_row_rule_is_the_projects():
    assert co.ROW_TOL == ROW_TOL and (co.DRAWS, co.SEED) == (16, 7)


@pytest.mark.parametrize("case", co.ALL_CASES, ids=co.ALL_IDS)
def test_conditions_of_the_rules(case):
    o = co.oracle_of(case)
    cs = o["cs"]
    G = o["f"].shape[1]
    persons, draws = co.left_out(o)
    plain = (sc.left_out(o["post"]), float((o["draws"][1] <= sc.ARGMAX_GAP).mean()))
    print("%s: N %d J %d G %d, answered <= %d, max |loglik| %.1f, cap %.2e" % (cs["name"], cs["N"], cs["J"], G, o["answered"],
                                                                               np.abs(o["post"]["loglik"]).max(), o["cap"]))
    print("    d_f %.2e, gap threshold %.2e: left out %.2f %% of the persons, %.3f %% of the draws (at %.0e: %.2f %%, %.3f %%)"
          % (o["d_f"], o["gap_thr"], 100 * persons, 100 * draws, sc.ARGMAX_GAP, 100 * plain[0], 100 * plain[1]))
    print("    " + "  ".join("%s e %.2e tol %.1e" % (k, o["e"][k], o["tol"][k]) for k in o["e"]))
    assert persons <= sc.ARGMAX_LEFT_OUT and draws <= sc.ARGMAX_LEFT_OUT, (cs["name"], persons, draws)
    if o["kind"] == "irt" and cs["name"] not in co.CONDITION_WAIVED:
        lo, need = sc.irt_condition(cs, o["post"])
        assert lo >= need, (cs["name"], "oracle PSD below half the node spacing", lo, need)
    tols = dict(o["tol"])
    if co.has_info(case):
        i = co.info_oracle(case)
        print("    P %d: " % len(i["free"]) + "  ".join("%s e %.2e tol %.1e" % (k, i["e"][k], i["tol"][k]) for k in i["e"]))
        tols.update(i["tol"])
        assert np.abs(i["info"] - i["info"].T).max() <= 1e-12 * np.abs(i["info"]).max()
    errs = dict(o["e"], **(i["e"] if co.has_info(case) else {}))
    for k, t in tols.items():
        # (a person without a long log-likelihood cannot widen anything: the cap never falls below the rule it caps)
        assert t <= max(o["cap"], ROW_TOL), (cs["name"], k, t, o["cap"])
        if 3.0 * errs[k] > t:
            print("    %s: 3 e_restated = %.2e is above the cap, the tolerance is the cap %.2e" % (k, 3.0 * errs[k], t))
        assert errs[k] < t, (cs["name"], k, "the method alone misses the tolerance", errs[k], t)
        if o["answered"] <= co.SHORT:
            assert t == ROW_TOL, (cs["name"], k, t)


def test_restated_f_agrees_with_the_oracle_on_a_short_case():
    """On 16 and on 30 items the restated f is the oracle's logw + ll of sc.irt_grid_loglik / sc.cdm_grid_loglik to float32
    accuracy: every rounding is at most 2^-24 of the running sum, whose size is at most |f| (every term has one sign): four a
    chunk, the fma, the log-weight, and the tables' own rounding to float32, which adds up to 2^-24 of |f| once more."""
    for name in ("corner_j16_g33", "corner_dina_k5"):
        o = co.oracle_of(co.by_name(name))
        cs = o["cs"]
        if o["kind"] == "irt":
            from vipsy_amd.engine import score_grid
            theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
            ll = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y"])
        else:
            ll, logw, _ = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], cs["y"])
        f = ll + np.asarray(logw, np.float64)[None, :]
        err = np.abs(o["f_r"].astype(np.float64) - f) / np.maximum(np.abs(f), 1.0)
        bound = (4 * ((cs["J"] + 15) // 16) + 3) * 2.0 ** -24
        print("%s: restated f against the oracle: %.2e of |f| (|f| <= %.1f; bound %.2e)" % (name, err.max(), np.abs(f).max(), bound))
        assert err.max() <= bound


@pytest.mark.parametrize("name", ["corner_j16_g33", "corner_j17_g32_1pl", "corner_dina_k5", "corner_dino_k5"])
def test_the_table_shortcut_is_the_grid_loglik(name):
    """ll by indicator matmuls over the per-item tables reproduces sc.irt_grid_loglik / sc.cdm_grid_loglik to 1e-12 relative."""
    o = co.oracle_of(co.by_name(name))
    cs = o["cs"]
    got = co.loglik_from_tables(o["T1"], o["T0"], cs["y"])
    if o["kind"] == "irt":
        from vipsy_amd.engine import score_grid
        theta, logw = score_grid(cs["D"], cs["nodes"], cs["span"])
        want = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], cs["y"])
        assert np.array_equal(theta.astype(np.float64), o["coord"])
    else:
        want, logw, attrs = sc.cdm_grid_loglik(cs["cdm"], cs["K"], cs["q"], cs["params"], cs["y"])
        assert np.array_equal(attrs, o["coord"])
    assert np.array_equal(np.asarray(logw, np.float32), o["logw"])
    err = np.abs(got - want).max() / np.abs(want).max()
    print("%s: %.2e" % (name, err))
    assert err <= 1e-12


def test_the_4pl_tables_too():
    """The 4PL tables (asymptotes through vo.sigmoid of the unconstrained leaves) on 40 rows of the long case."""
    o = co.oracle_of(co.by_name("long_j1024_4pl"))
    cs = o["cs"]
    from vipsy_amd.engine import score_grid
    theta, _ = score_grid(cs["D"], cs["nodes"], cs["span"])
    y = cs["y"][:40]
    want = sc.irt_grid_loglik(cs["model"], theta, cs["params"], cs["Dc"], y)
    assert np.abs(co.loglik_from_tables(o["T1"], o["T0"], y) - want).max() <= 1e-12 * np.abs(want).max()
