"""The plausible-value sampler restated in numpy (tests/pv_cases.py), on the CPU: the lattice of the uniforms, how often the
float64 oracle itself cannot tell the best two perturbed nodes apart, and that Gumbel-max over that noise samples the grid
posterior of tests/score_cases.py.  What the GPU test (tests/test_gpu_pv.py) compares the kernel with is checked here."""
import numpy as np
import pytest

from tests import pv_cases as pv
from tests import score_cases as sc

ALL_CASES = sc.IRT_CASES + sc.CDM_CASES
CASE1 = sc.IRT_CASES[0]


def test_lattice_is_exact_in_float32_and_inside_the_unit_interval():
    rng = np.random.RandomState(1)
    x = np.concatenate([np.array([0, 1, 2 ** 32 - 1, 2 ** 32 - 2, 511, 512, 2 ** 31], dtype=np.uint32),
                        rng.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)])
    u32, u64 = pv.lattice_u(x, np.float32), pv.lattice_u(x, np.float64)
    assert u32.dtype == np.float32
    assert np.array_equal(u32.astype(np.float64), u64)                       # no rounding anywhere in float32
    assert np.array_equal(u64 * 2.0 ** 24, 2.0 * (x >> np.uint32(9)) + 1.0)   # the odd 24-bit numerators
    assert (u32 > 0).all() and (u32 < 1).all()
    assert u32.min() == np.float32(2.0 ** -24) and u32.max() == np.float32(1.0 - 2.0 ** -24)
    noise = -np.log(-np.log(u64))
    assert np.isfinite(noise).all() and noise.min() > -2.83 and noise.max() < 16.7
    # the rule the step kernels use rounds its top word to 1.0 -- an infinite Gumbel
    from oracle import vi_oracle as vo
    assert vo._u01(np.uint32(0xFFFFFFFF)) == 1.0


def test_words_do_not_depend_on_the_chunk_of_draws():
    r = np.array([0, 5, 2 ** 33 + 7], dtype=np.int64)
    full = pv.words(9, r, 70, 37)
    assert full.shape == (3, 70, 37)
    assert np.array_equal(pv.words(9, r, 70, 5), full[:, :, :5])
    assert np.array_equal(pv.words(9, r, 70, 11, draw0=18), full[:, :, 18:29])
    assert np.array_equal(pv.words(9, r[1:2], 70, 37), full[1:2])
    assert not np.array_equal(pv.words(10, r, 70, 37), full)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_oracle_gaps_stay_inside_the_cap(case):
    node, gap = pv.oracle_draws(case)
    cs, f, _, _ = pv.posterior_f(case)
    assert node.shape == gap.shape == (cs["N"], pv.DRAWS)
    out = pv.left_out(gap)
    print("%s: %.3f %% of the (person, draw) pairs within %.0e" % (case[0], 100 * out, sc.ARGMAX_GAP))
    assert out <= sc.ARGMAX_LEFT_OUT, (case[0], out)


def test_restated_sampler_samples_the_posterior():
    """Case 1, 4096 draws a person against the oracle posterior of every person: cells with an expected count below 5 are pooled
    into one, the chi-square over its degrees of freedom stays below 3 and the total variation below 0.06 (of 4096 draws from
    at most 61 cells it is about sqrt(cells / (2 pi 4096)) <= 0.05)."""
    M = 4096
    cs, f, coord, post = pv.posterior_f(CASE1)
    N, G = f.shape
    node, _ = pv.draw(f, pv.gumbel(pv.SEED, np.arange(N), G, M))
    p = np.exp(f - f.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    worst_chi, worst_tv = 0.0, 0.0
    for i in range(N):
        cnt = np.bincount(node[i], minlength=G).astype(np.float64)
        tv = 0.5 * np.abs(cnt / M - p[i]).sum()
        exp = M * p[i]
        big = exp >= 5
        o, e = list(cnt[big]), list(exp[big])
        if (~big).any():
            o.append(cnt[~big].sum())
            e.append(exp[~big].sum())
        o, e = np.array(o), np.array(e)
        keep = e > 0
        dof = int(keep.sum()) - 1
        assert dof >= 1, i
        chi = float((((o - e) ** 2)[keep] / e[keep]).sum()) / dof
        worst_chi, worst_tv = max(worst_chi, chi), max(worst_tv, tv)
        assert chi < 3.0, (i, chi, dof)
        assert tv < 0.06, (i, tv)
    print("case 1, %d draws: worst chi-square / dof %.2f, worst total variation %.3f" % (M, worst_chi, worst_tv))
    # nobody's answers (row 5): the prior comes back
    from vipsy_amd.engine import score_grid
    prior = np.exp(score_grid(1, cs["nodes"], cs["span"])[1].astype(np.float64))
    assert (cs["y"][5] == 255).all()
    assert 0.5 * np.abs(np.bincount(node[5], minlength=G) / M - prior).sum() < 0.06


def test_mean_of_the_draws_is_the_eap():
    M = 1024
    cs, f, coord, post = pv.posterior_f(CASE1)
    node, _ = pv.draw(f, pv.gumbel(pv.SEED, np.arange(f.shape[0]), f.shape[1], M))
    mean = coord[node, 0].mean(1)
    z = np.abs(mean - post["mean"][:, 0]) / (post["sd"][:, 0] / np.sqrt(M))
    print("case 1, %d draws: the mean drawn theta is at most %.2f standard errors from the oracle EAP" % (M, z.max()))
    assert (z <= 5.0).all(), (int(z.argmax()), float(z.max()))
