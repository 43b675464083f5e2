"""The (engine family, response design) pairs of tests/test_gpu_response_designs.py, and how each builds its engine.

Kept apart from the GPU module so that the CPU suite (tests/test_response_designs.py) can build the SAME engines on the
numpy backend, read the same parameters off them and check, without a GPU, what the GPU comparison relies on: the oracle's
loss and gradients are finite, and no observed cell sits on the Bernoulli clamp (band() below).

Parameter rules are those of the family's existing parity test (tests/test_gpu_parity.py, tests/test_gpu_cdm_sf.py), drawn
from the case's own seed; the seeds committed here were chosen on the CPU so that the clamp band is empty."""
import functools

import numpy as np
import torch

from oracle import vi_oracle as vo
from tests import response_designs as rd

Z_CLAMP = float(np.log((1.0 - vo.EPS32) / vo.EPS32))      # 15.9424: logit(1 - eps32)
BAND = 1e-3                                                # the band of test_headline_large_batch_kernels_vs_oracle


# ---- designs, by name ---------------------------------------------------------------------------------------------------
def _edges(y, f, **kw):
    return rd.with_edges(y, f, seed=7, **kw)


@functools.lru_cache(maxsize=None)
def design(name):
    """(y, facts) of a named design.  Cached: the arrays are shared, nobody writes to them."""
    if name == "sorted9000":        # the issue's design: booklets of 10 / 40 / 150 of 500 items, rows in file order, three sort
        y, f = rd.booklets(9000, 500, (150, 40, 10), True, seed=1)        # windows of the lists, 50 + 250 items in no booklet
        return _edges(y, f, empty_block=4096 + 640)
    if name == "shuffled3000":      # the same booklets shuffled: every 64-person group and the window mix all three lengths
        y, f = rd.booklets(3000, 500, (10, 40, 150, 250), False, seed=2)
        return _edges(y, f, empty_block=1280)
    if name == "j1024_complete":    # J at the list kernel's limit, one complete case among 95 % missing: Lq = 256
        y, f = rd.booklets(640, 1024, (16, 48, 128), False, seed=3)
        return _edges(y, f, complete_case=True, unanswered_item=False)
    if name == "all_missing":
        return rd.all_missing(200, 37)
    if name == "single_cell":
        return rd.single_cell(200, 37)
    if name == "empty_block_small":  # three list groups, the last of them made of 64 empty persons and nothing else
        y, f = rd.booklets(192, 40, (3, 8, 17), True, seed=4)
        return _edges(y, f, empty_block=64)
    if name == "dense3000":         # overlapping booklets of 480 / 300 / 100 of 500 items: 38 % missing, the dense kernel
        y, f = rd.booklets(3000, 500, (480, 300, 100), False, seed=5, counts=(1350, 600, 1050))
        return _edges(y, f)
    if name == "hetero_shards":     # a file sorted by booklet, cut in two: rows 0-1023 are 25 % missing, rows 1024-2047 91 %,
        y, f = rd.booklets(2048, 400, (300, 60, 12), True, seed=22, counts=(1024, 512, 512))      # the whole 58 %
        return _edges(y, f, empty_block=1536)
    if name == "amort640":          # the amortized D = 1 guide, J = 500
        y, f = rd.booklets(640, 500, (10, 40, 150), False, seed=6)
        return _edges(y, f, empty_block=128)
    if name == "amort_oddj":        # ... an odd item count (a phantom item beside the missing code)
        y, f = rd.booklets(333, 37, (4, 9, 20), True, seed=7)
        return _edges(y, f)
    if name == "amort4608":         # ... from 4 096 persons on: the fp16-pair forward, observed-cell lists, two windows
        y, f = rd.booklets(4608, 500, (10, 40, 150), True, seed=8)
        return _edges(y, f, empty_block=4200)
    if name == "mvn257":            # the generic tier (H = 96 > 64)
        y, f = rd.booklets(257, 130, (10, 30, 80), False, seed=9)
        return _edges(y, f)
    if name == "mvn256":            # the packed tier (H = 64, D % 4 == 0)
        y, f = rd.booklets(256, 72, (6, 20, 40), False, seed=10)
        return _edges(y, f)
    if name == "mvn320":            # J = 500, D = 100: the MFMA likelihood, item-major responses
        y, f = rd.booklets(320, 500, (10, 40, 150), False, seed=11)
        return _edges(y, f)
    if name == "mvn320_j499":       # ... with a phantom item and a phantom dimension (J = 499, D = 99)
        y, f = rd.booklets(320, 499, (10, 40, 150), True, seed=12)
        return _edges(y, f)
    if name == "mvn33024":          # the large-batch forms
        y, f = rd.booklets(33024, 500, (150, 40, 10), True, seed=13)
        return _edges(y, f, empty_block=20000)
    if name == "bbvi300":
        y, f = rd.booklets(300, 64, (4, 12, 40), False, seed=14)
        return _edges(y, f)
    if name == "bbvi200":
        y, f = rd.booklets(200, 33, (3, 8, 20), True, seed=15)
        return _edges(y, f)
    if name == "cdm400_j30":        # the reference's HO-DINA item count
        y, f = rd.booklets(400, 30, (3, 8, 17), False, seed=16)
        return _edges(y, f)
    if name == "cdm333_j70":
        y, f = rd.booklets(333, 70, (5, 15, 40), True, seed=17)
        return _edges(y, f)
    if name == "cdm260_j17":
        y, f = rd.booklets(260, 17, (2, 5, 10), False, seed=18)
        return _edges(y, f)
    if name == "cdm300_j40":
        y, f = rd.booklets(300, 40, (4, 10, 24), False, seed=19)
        return _edges(y, f)
    if name == "complete400_j30":   # the score-function CDMs take complete responses only (CdmSfEngine refuses a missing cell):
        y, f = rd.booklets(400, 30, (30,), False, seed=20)                # their edges are the constant items and persons
        return _edges(y, f, empty_person=False, unanswered_item=False, constant_persons=False)
    if name == "complete333_j100":
        y, f = rd.booklets(333, 100, (100,), False, seed=21)
        return _edges(y, f, empty_person=False, unanswered_item=False, constant_persons=False)
    raise KeyError(name)


def subsample_rows(N, B, seed):
    """B distinct rows in the order fit() draws them: unsorted."""
    return np.random.RandomState(seed).permutation(N)[:B].astype(np.int64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


# ---- D = 1, per-person guide --------------------------------------------------------------------------------------------
IRT1D_SEED = 5

# (id, design, model, B, parameter seed, far persons, their |x_local|)
# far persons: every `far`-th person is moved to |x_local| = far_x -- cells far beyond the clamp (1PL: z = x + b needs
# |x| = 21; 2PL / 3PL: 11 as in test_irt1d_step_vs_oracle, slopes above 1.45 take the cell over)
IRT1D_SPARSE = [
    ("sorted9000-1pl", "sorted9000", "irt_1pl", None, 101, 500, 21.0),
    ("sorted9000-2pl", "sorted9000", "irt_2pl", None, 3102, 500, 11.0),
    ("sorted9000-3pl", "sorted9000", "irt_3pl", None, 3103, 500, 11.0),
    ("sorted9000-4pl", "sorted9000", "irt_4pl", None, 104, 500, 11.0),
    ("shuffled3000-1pl", "shuffled3000", "irt_1pl", None, 111, 0, 0.0),
    ("shuffled3000-2pl", "shuffled3000", "irt_2pl", None, 112, 0, 0.0),
    ("shuffled3000-3pl", "shuffled3000", "irt_3pl", None, 113, 0, 0.0),
    ("shuffled3000-4pl", "shuffled3000", "irt_4pl", None, 114, 0, 0.0),
    ("j1024_complete-2pl", "j1024_complete", "irt_2pl", None, 121, 0, 0.0),
    ("j1024_complete-3pl", "j1024_complete", "irt_3pl", None, 122, 0, 0.0),
    ("j1024_complete-4pl", "j1024_complete", "irt_4pl", None, 123, 0, 0.0),
    ("all_missing-1pl", "all_missing", "irt_1pl", None, 131, 0, 0.0),
    ("all_missing-4pl", "all_missing", "irt_4pl", None, 132, 0, 0.0),
    ("single_cell-2pl", "single_cell", "irt_2pl", None, 141, 0, 0.0),
    ("single_cell-3pl", "single_cell", "irt_3pl", None, 142, 0, 0.0),
    ("empty_block_small-1pl", "empty_block_small", "irt_1pl", None, 151, 0, 0.0),
    ("empty_block_small-4pl", "empty_block_small", "irt_4pl", None, 152, 0, 0.0),
]
IRT1D_DENSE = [
    ("dense3000-1pl", "dense3000", "irt_1pl", None, 201, 600, 21.0),
    ("dense3000-2pl", "dense3000", "irt_2pl", None, 3202, 600, 11.0),
    ("dense3000-3pl", "dense3000", "irt_3pl", None, 5203, 600, 11.0),
    ("dense3000-4pl", "dense3000", "irt_4pl", None, 204, 600, 11.0),
    ("sorted9000-2pl-rows1000", "sorted9000", "irt_2pl", 1000, 211, 500, 11.0),
    ("sorted9000-3pl-rows100", "sorted9000", "irt_3pl", 100, 212, 0, 0.0),
    ("shuffled3000-4pl-rows100", "shuffled3000", "irt_4pl", 100, 213, 0, 0.0),
    ("j1024_complete-1pl-rows100", "j1024_complete", "irt_1pl", 100, 214, 0, 0.0),
    ("single_cell-2pl-rows100", "single_cell", "irt_2pl", 100, 217, 0, 0.0),
]
# the designs that must hold at least 100 observed cells BEYOND the clamp (1PL, 2PL, 3PL of each row of the table; 3PL on
# the upper side only), and the 4PL ones that must hold none
BEYOND_CLAMP = ("sorted9000-1pl", "sorted9000-2pl", "sorted9000-3pl", "dense3000-1pl", "dense3000-2pl", "dense3000-3pl")
NONE_BEYOND = ("sorted9000-4pl", "dense3000-4pl")


def irt1d_params(eng, y, model, pseed, far, far_x, loc_rows=None):
    """The parameter rule of test_irt1d_step_vs_oracle; loc_rows: global ids of the engine's persons (a shard takes its rows of
    the draws made for the whole problem)."""
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    eng.unconstrained("b").copy_(_t(0.7 * rng.randn(1, J)))
    if model != "irt_1pl":
        eng.unconstrained("a").copy_(_t(0.5 + 2 * rng.rand(1, J)))
    if model in ("irt_3pl", "irt_4pl"):
        eng.unconstrained("c").add_(_t(0.3 * rng.randn(1, J)).to(eng.dev))
    loc0 = rng.randn(N)
    if far:
        loc0[::far] = far_x * np.sign(loc0[::far])
    raw0 = 0.3 * rng.randn(N)
    if loc_rows is not None:
        loc0, raw0 = loc0[loc_rows], raw0[loc_rows]
    eng.PP.copy_(_t(np.concatenate([loc0, raw0])))


def irt1d_engine(case, dev, backend=None, y=None, **kw):
    from vipsy_amd.engine import IrtEngine
    _, dname, model, B, pseed, far, far_x = case
    if y is None:
        y = design(dname)[0]
    eng = IrtEngine(torch.from_numpy(y).to(dev), model=model, D=1, seed=IRT1D_SEED, backend=backend, **kw)
    irt1d_params(eng, y, model, pseed, far, far_x)
    idx = np.arange(len(y)) if B is None else subsample_rows(len(y), B, pseed)
    return eng, y, idx


def irt_spec(model, D, N, J, amortized, share_cov=False):
    return {"family": "irt", "model": model, "D": D, "Dc": 1.0, "N": N, "amortized": amortized, "share_cov": share_cov,
            "a_free": vo.default_a_free(D, J) if D > 1 else None}


# ---- D = 1, amortized guide ---------------------------------------------------------------------------------------------
# (id, design, model, B, parameter seed)
IRT1D_AMORT = [
    ("amort640-2pl", "amort640", "irt_2pl", None, 301),
    ("amort640-4pl-rows100", "amort640", "irt_4pl", 100, 302),
    ("amort_oddj-3pl", "amort_oddj", "irt_3pl", None, 303),
    ("amort_oddj-1pl-rows100", "amort_oddj", "irt_1pl", 100, 304),
    ("amort4608-2pl", "amort4608", "irt_2pl", None, 305),
    ("amort4608-4pl-rows100", "amort4608", "irt_4pl", 100, 306),
]


def irt1d_amort_engine(case, dev, backend=None):
    """The parameter rule of test_irt1d_amortized_step_vs_oracle (the default encoder of the engine's seed)."""
    from vipsy_amd.engine import IrtEngine
    _, dname, model, B, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    eng = IrtEngine(torch.from_numpy(y).to(dev), model=model, D=1, amortized=True, H=64, seed=IRT1D_SEED, backend=backend)
    eng.unconstrained("b").copy_(_t(0.7 * rng.randn(1, J)))
    if model != "irt_1pl":
        eng.unconstrained("a").copy_(_t(0.5 + 2 * rng.rand(1, J)))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    return eng, y, idx


# ---- amortized multivariate guide ---------------------------------------------------------------------------------------
MVN_SEED = 11
# (id, design, D, H, model, B, slopes, parameter seed); slopes 'unit': the rule of test_mvn_amortized_step_vs_oracle,
# 'small': 0.05 (1 +- 0.3) as in the large-batch tests (D >= 64: |z| stays under 15)
MVN_AMORT = [
    ("mvn257-d33-h96-2pl", "mvn257", 33, 96, "irt_2pl", None, "small", 401),
    ("mvn257-d7-h96-4pl-rows100", "mvn257", 7, 96, "irt_4pl", 100, "unit", 402),
    ("mvn256-d8-h64-3pl", "mvn256", 8, 64, "irt_3pl", None, "unit", 403),
    ("mvn256-d8-h64-2pl-rows100", "mvn256", 8, 64, "irt_2pl", 100, "unit", 404),
    ("mvn320-d100-h64-2pl", "mvn320", 100, 64, "irt_2pl", None, "small", 405),
    ("mvn320-d100-h64-4pl", "mvn320", 100, 64, "irt_4pl", None, "small", 406),
    ("mvn320_j499-d99-h64-2pl", "mvn320_j499", 99, 64, "irt_2pl", None, "small", 407),
    ("mvn320_j499-d99-h64-2pl-rows100", "mvn320_j499", 99, 64, "irt_2pl", 100, "small", 408),
]
MVN_LARGE = ("mvn33024-d100-h64-2pl", "mvn33024", 100, 64, "irt_2pl", None, "small", 409)


def mvn_amort_engine(case, dev, backend=None):
    from vipsy_amd.engine import IrtEngine
    _, dname, D, H, model, B, slopes, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    if slopes == "unit":            # the hand-made encoder of _random_problem
        enc = {"fc1.weight": rng.randn(H, J) / np.sqrt(J), "fc1.bias": 0.1 * rng.randn(H),
               "fc21.weight": rng.randn(D, H) / np.sqrt(H), "fc21.bias": 0.1 * rng.randn(D),
               "fc22.weight": 0.3 * rng.randn(D * (D + 1) // 2, H) / np.sqrt(H), "fc22.bias": 0.05 * rng.randn(D * (D + 1) // 2)}
        eng = IrtEngine(torch.from_numpy(y).to(dev), model=model, D=D, amortized=True, H=H,
                        encoder_init={k: v.astype(np.float32) for k, v in enc.items()}, seed=MVN_SEED, backend=backend)
        mult = 1 + 0.3 * rng.randn(D, J)
    else:                           # the default encoder, as in the judged run
        eng = IrtEngine(torch.from_numpy(y).to(dev), model=model, D=D, amortized=True, H=H, seed=MVN_SEED, backend=backend)
        mult = 0.05 * (1 + 0.3 * rng.randn(D, J))
    a0 = eng.unconstrained("a") * _t(mult).to(dev)
    eng.unconstrained("a").copy_(a0 * eng.unconstrained("a", eng.free))
    eng.unconstrained("b").copy_(_t(0.5 * rng.randn(1, J)))
    if model in ("irt_3pl", "irt_4pl"):
        eng.unconstrained("c").add_(_t(0.3 * rng.randn(1, J)).to(dev))
    if model == "irt_4pl":
        eng.unconstrained("d").add_(_t(0.3 * rng.randn(1, J)).to(dev))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    return eng, y, idx


# ---- multivariate per-person guide --------------------------------------------------------------------------------------
BBVI_SEED = 13
# (id, design, D, share_cov, B, parameter seed)
MVN_BBVI = [
    ("bbvi300-d20", "bbvi300", 20, False, None, 501),
    ("bbvi300-d20-rows100", "bbvi300", 20, False, 100, 502),
    ("bbvi200-d9-shared", "bbvi200", 9, True, None, 503),
    ("bbvi200-d9-shared-rows100", "bbvi200", 9, True, 100, 504),
]


def mvn_bbvi_engine(case, dev, backend=None):
    """The parameter rule of test_mvn_bbvi_step_vs_oracle."""
    from vipsy_amd.engine import IrtEngine
    _, dname, D, share, B, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    eng = IrtEngine(torch.from_numpy(y).to(dev), model="irt_2pl", D=D, share_cov=share, seed=BBVI_SEED, backend=backend)
    eng.unconstrained("b").copy_(_t(0.5 * rng.randn(1, J)))
    eng.unconstrained("x_local").copy_(_t(0.5 * rng.randn(N, D)))
    eng.unconstrained("x_scale").copy_(_t(0.2 * rng.randn(*eng.unconstrained("x_scale").shape)))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    return eng, y, idx


# ---- the CDMs -----------------------------------------------------------------------------------------------------------
def q_matrix(rng, K, J):
    """The Q-matrix rule of the CDM parity tests: 40 % ones, every item needs at least one attribute."""
    q = (rng.rand(K, J) < 0.4).astype(np.float32)
    q[rng.randint(0, K, size=J), np.arange(J)] = 1.0
    return q


HODINA_SEED = 9
# (id, design, K, amortized, B, parameter seed)
HODINA = [
    ("hodina-k5-j30", "cdm400_j30", 5, False, None, 601),            # 5 <= K <= 8, J <= 32: k_hodina_m
    ("hodina-k5-j30-rows100", "cdm400_j30", 5, False, 100, 602),
    ("hodina-k3-j70", "cdm333_j70", 3, False, None, 603),            # k_hodina
    ("hodina-k9-j70-rows100", "cdm333_j70", 9, False, 100, 604),
    ("vaehodina-k6-j17", "cdm260_j17", 6, True, None, 605),          # k_hodina_m, amortized guide
    ("vaehodina-k10-j40-rows100", "cdm300_j40", 10, True, 100, 606),  # k_hodina, 1024 patterns
]


def hodina_engine(case, dev, backend=None):
    """The parameter rule of test_hodina_step_vs_oracle."""
    from vipsy_amd.engine import HoDinaEngine
    _, dname, K, amort, B, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    q = q_matrix(rng, K, J)
    eng = HoDinaEngine(torch.from_numpy(y).to(dev), q, amortized=amort, H=64, seed=HODINA_SEED, backend=backend)
    eng.unconstrained("lam0").copy_(_t(0.5 * rng.randn(1, K)))
    eng.unconstrained("lam1").copy_(_t(0.4 * rng.randn(1, K)))
    eng.unconstrained("g").add_(_t(0.5 * rng.randn(1, J)).to(dev))
    eng.unconstrained("s").add_(_t(0.5 * rng.randn(1, J)).to(dev))
    if not amort:
        eng.PP.copy_(_t(np.concatenate([rng.randn(N), 0.3 * rng.randn(N)])))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    spec = {"family": "hodina", "K": K, "N": N, "amortized": amort, "q": q}
    return eng, y, idx, spec


# (id, design, K, cdm, B, parameter seed)
CCDM = [
    ("ccdm-dina-k8-j30", "cdm400_j30", 8, "dina", None, 701),
    ("ccdm-dino-k5-j70-rows100", "cdm333_j70", 5, "dino", 100, 702),
]


def ccdm_engine(case, dev, backend=None):
    """The parameter rule of test_ccdm_step_vs_oracle."""
    from vipsy_amd.engine import CcdmEngine
    _, dname, K, cdm, B, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    q = q_matrix(rng, K, J)
    eng = CcdmEngine(torch.from_numpy(y).to(dev), q, cdm=cdm, seed=3, backend=backend)
    eng.unconstrained("g").add_(_t(0.5 * rng.randn(1, J)).to(dev))
    eng.unconstrained("s").add_(_t(0.5 * rng.randn(1, J)).to(dev))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    spec = {"family": "ccdm", "cdm": cdm, "K": K, "N": N, "amortized": False, "q": q}
    return eng, y, idx, spec


# (id, design, K, cdm, B, H, parameter seed)
VAECCDM = [
    ("vaeccdm-dina-k8-j30", "cdm400_j30", 8, "dina", None, 64, 801),
    ("vaeccdm-dino-k5-j70-rows100", "cdm333_j70", 5, "dino", 100, 24, 802),
]


def vaeccdm_engine(case, dev, backend=None):
    """The parameter rule of test_vaeccdm_step_vs_oracle."""
    from vipsy_amd.engine import VaeCcdmEngine
    _, dname, K, cdm, B, H, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    q = q_matrix(rng, K, J)
    eng = VaeCcdmEngine(torch.from_numpy(y).to(dev), q, cdm=cdm, H=H, seed=4, backend=backend)
    eng.unconstrained("g").copy_(_t(vo.logit(0.05 + 0.3 * rng.rand(1, J))))
    eng.unconstrained("s").copy_(_t(vo.logit(0.05 + 0.3 * rng.rand(1, J))))
    eng.unconstrained("encoder$$$fc2.weight").mul_(3.0)
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    spec = {"family": "vaeccdm", "cdm": cdm, "K": K, "N": N, "amortized": True, "q": q.astype(np.float64)}
    return eng, y, idx, spec


CDM_SF_SEED, CDM_SF_T, CDM_SF_STREAM, CDM_SF_GID0 = 9, 3, 2, 1 << 33
# (id, design, K, cdm, B, amortized, H, baseline, parameter seed)
CDM_SF = [
    ("cdmsf-dina-k8-j30", "complete400_j30", 8, "dina", None, False, 0, "none", 901),
    ("cdmsf-dina-k8-j30-avg-rows100", "complete400_j30", 8, "dina", 100, False, 0, "avg", 902),
    ("cdmsf-dino-k5-j100-rows100", "complete333_j100", 5, "dino", 100, False, 0, "none", 903),
    ("vaecdmsf-dina-k5-j100", "complete333_j100", 5, "dina", None, True, 64, "none", 904),
    ("vaecdmsf-dino-k8-j30-avg-rows100", "complete400_j30", 8, "dino", 100, True, 24, "avg", 905),
]


def cdm_sf_engine(case, dev, backend=None):
    """The parameter rule of test_cdm_sf_step_vs_oracle."""
    from vipsy_amd.engine import CdmSfEngine
    _, dname, K, cdm, B, amort, H, baseline, pseed = case
    y = design(dname)[0]
    N, J = y.shape
    rng = np.random.RandomState(pseed)
    q = q_matrix(rng, K, J)
    eng = CdmSfEngine(torch.from_numpy(y).to(dev), q, cdm=cdm, amortized=amort, H=H, seed=CDM_SF_SEED, gid0=CDM_SF_GID0,
                      n_global=N, attr_prior=0.4, baseline=baseline, backend=backend)
    eng.unconstrained("g").copy_(_t(vo.logit(0.05 + 0.3 * rng.rand(1, J))))
    eng.unconstrained("s").copy_(_t(vo.logit(0.05 + 0.3 * rng.rand(1, J))))
    if not amort:
        eng.unconstrained("attr_p").copy_(_t(rng.randn(N, K)))
    idx = np.arange(N) if B is None else subsample_rows(N, B, pseed)
    spec = {"family": "cdm_sf", "cdm": cdm, "K": K, "N": N, "amortized": amort, "q": q.astype(np.float64), "attr_prior": 0.4}
    return eng, y, idx, spec


def cdm_sf_draws(eng, y, idx, K, amort):
    """The kernel's draw rule restated (test_cdm_sf_step_vs_oracle): u_ik < p_ik with p in float32.  Returns the draws and the
    persons with a draw within 1e-6 of its threshold (either rounding is right there)."""
    from vipsy_amd.engine import BIN_ENC_KEYS
    params = {n: eng.unconstrained(n).cpu().numpy().astype(np.float64) for n in eng.all_names()}
    if amort:
        W = {k: params["encoder$$$" + k] for k in BIN_ENC_KEYS}
        u, _ = vo.bin_enc_forward(W, y[idx].astype(np.float64))
        p = vo.sigmoid(u)
    else:
        p = np.clip(vo.sigmoid(params["attr_p"][idx]), vo.TINY32, 1 - vo.EPS32)
    uni = vo.philox_uniforms(CDM_SF_SEED, CDM_SF_T, CDM_SF_STREAM, CDM_SF_GID0 + idx, K)
    attr = (uni < p.astype(np.float32)).astype(np.float64)
    near = (np.abs(uni - p) < 1e-6).any(axis=1)
    return params, attr, near


# ---- the oracle's view of a case ----------------------------------------------------------------------------------------
def params_of(eng):
    return {n: eng.unconstrained(n).cpu().numpy().astype(np.float64) for n in eng.all_names()}


def irt_latents(spec, params, y, idx, eps):
    """x of the persons idx under the oracle's guide (irt_particle), float64."""
    D = spec["D"]
    eps = np.asarray(eps, np.float64).reshape(len(idx), D)
    if spec["amortized"]:
        if D == 1:
            W = {k: params["encoder$$$" + k] for k in vo.ENC_KEYS}
            loc, raw, _ = vo.enc_forward(W, vo.enc_input(y[idx], np.float64))
            return loc + np.exp(raw) * eps
        from tests.test_gpu_parity import _oracle_latents_chunked
        return _oracle_latents_chunked(params, y[idx], eps, D)
    loc = params["x_local"][idx]
    if D == 1:
        return loc + np.exp(params["x_scale"][idx]) * eps
    M = np.broadcast_to(params["x_scale"], (len(idx), D, D)) if spec["share_cov"] else params["x_scale"][idx]
    L = np.tril(M, -1) + np.einsum("bi,ij->bij", np.exp(np.einsum("bii->bi", M)), np.eye(D))
    return loc + np.einsum("bij,bj->bi", L, eps)


def band(spec, params, y, idx, eps):
    """The observed cells of the batch against the Bernoulli clamp, from the oracle's own response probability P: with
    l = logit(P) (l = z for 1PL / 2PL), a cell is ON the clamp where | |l| - zc | < 1e-3 |l| and BEYOND it where P lies outside
    [eps32, 1 - eps32].  Returns (cells on the clamp, cells beyond below, cells beyond above, observed cells, max |z|)."""
    model = spec["model"]
    x = irt_latents(spec, params, y, idx, eps)
    z = spec["Dc"] * ((x + params["b"]) if model == "irt_1pl" else (x @ params["a"] + params["b"]))
    obs = y[idx] != 255
    lo = vo.sigmoid(params["c"]) if model in ("irt_3pl", "irt_4pl") else 0.0
    hi = vo.sigmoid(params["d"]) if model == "irt_4pl" else 1.0
    sg, sgc = vo.sigmoid(z), vo.sigmoid(-z)
    P, Q = lo + (hi - lo) * sg, (1.0 - hi) + (hi - lo) * sgc          # P and 1 - P, each without cancellation
    with np.errstate(divide="ignore"):
        l = np.log(P) - np.log(Q)
    al = np.abs(l)
    on = obs & (np.abs(al - Z_CLAMP) < BAND * al)
    below, above = obs & (P < vo.EPS32), obs & (Q < vo.EPS32)
    return int(on.sum()), int(below.sum()), int(above.sum()), int(obs.sum()), float(np.abs(z[obs]).max()) if obs.any() else 0.0
