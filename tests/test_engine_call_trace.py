"""The calls a step makes, pinned without a GPU.  A recording backend that computes nothing answers every size / offset /
layout query from a table and files every compute call: its name, nb, the configuration it carries and, argument by argument,
what was handed over (absent or present, how long, where in its buffer, which copy of the responses).  The traces of
tests/golden/engine_call_trace.json were recorded with this file before IrtEngine.loss_and_grads was split into one pass per
guide; they are compared exactly.  Record again (on purpose only): python -m tests.test_engine_call_trace --record

What the stub's few side effects pin: its likelihood fills gxT / gdT / ll / ent (its 1-D step kernels gloc / graw) with ones,
and its encoder backward calls file how many entries are still non-zero -- the phantoms taken out in between -- and fill the
encoder's gradient with ones, so that the zeroed gradients of phantom head rows / columns show in the case's `after`."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from vipsy_amd.engine import CdmSfEngine, HipBackend, HoDinaEngine, IrtEngine, LrSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_call_trace.json")

QUERIES = {"mvn_pack_floats": 1 << 16, "lik_ximg_bytes": 1 << 10, "lik_workspace": 1 << 16, "mvn_pack_opmax_offset": 8,
           "mvn_enc_bwd_workspace": 1 << 16, "mvn_enc_bwd_layout": 1, "mvn_enc_bwd_gd_offset": 64,
           "mvn_enc_bwd_hs_offset": 1 << 15, "irt1d_workspace": 1 << 16, "irt1d_sparse_workspace": 1 << 16,
           "mvn_bbvi_bwd_workspace": 1 << 16, "norm_enc_pack_floats": 1 << 10, "norm_enc_bwd_workspace": 1 << 16,
           "hodina_workspace": 1 << 16, "cdm_sf_workspace": 1 << 16, "mvn_score_heads_workspace": 1 << 10,
           "bin_enc_bwd_workspace": 1 << 16}
COMPUTE = ("mvn_enc_forward", "lik_grad", "mvn_enc_backward", "irt1d_grad", "irt1d_sparse_grad", "mvn_bbvi_forward",
           "mvn_bbvi_backward", "norm_enc_forward", "norm_enc_backward", "hodina_grad", "cdm_sf_grad", "irt1d_score_grad",
           "mvn_score_operands", "mvn_score_heads", "mvn_score_diag", "loo_baseline", "bin_enc_forward", "bin_enc_backward",
           "sum_into", "sum2_into", "adam", "adam2", "philox_normals")


def _describe(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, ctypes.Structure):
        return {k: getattr(v, k) for k in ("model", "K", "D", "J", "H", "scale", "step", "stream") if hasattr(v, k)}
    if torch.is_tensor(v):
        if v.dtype == torch.uint8 and v.dim() == 2:            # a copy of the responses: which one
            return {"u8": list(v.shape), "n254": int((v == 254).sum()), "n255": int((v == 255).sum())}
        if v.dtype == torch.int64:                             # row indices
            return {"rows": v.reshape(-1).tolist()}
        return {"n": int(v.numel()), "at": int(v.storage_offset())}
    if isinstance(v, dict):
        return {str(k): _describe(v[k]) for k in sorted(v)}
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    raise TypeError("argument of a kind the trace does not know: %r" % (v,))


def _nz(t, n):
    return None if t is None else int((t.reshape(-1)[:n] != 0).sum())


class _Recorder(object):
    """Queries answered from a table (QUERIES; keyword arguments override an entry), compute calls filed."""

    def __init__(self, **table):
        self.table, self.calls, self.kept = dict(QUERIES, **table), [], {}

    cfg, hodina_cfg = staticmethod(HipBackend.cfg), staticmethod(HipBackend.hodina_cfg)

    def _file(self, name, args):
        rec = {"call": name}
        for k, v in args.items():
            rec[k] = _describe(v)
        self.calls.append(rec)
        getattr(self, "_after_" + name, lambda a, r: None)(args, rec)

    # what the stub does beyond filing -------------------------------------------------------------
    def _after_mvn_enc_forward(self, a, rec):
        self.kept["ent"] = a["out"]["ent"]

    def _after_mvn_bbvi_forward(self, a, rec):
        self.kept["ent"] = a["ent"]

    def _after_lik_grad(self, a, rec):
        for k in ("gx", "gxT", "gdT", "ll"):
            if a[k] is not None:
                a[k].fill_(1.0)
        self.kept["ent"].fill_(1.0)
        self.kept["gdT"] = a["gdT"]

    def _after_mvn_enc_backward(self, a, rec):
        nb, D = a["nb"], a["cfg"].D
        ll, ent = (a["loss"][0], a["loss"][1]) if a["loss"] is not None else (None, self.kept["ent"])
        rec["nonzero"] = {"gx": _nz(a["gx"], nb * D), "gxT": _nz(a["gxT"], nb * D), "gdT": _nz(self.kept["gdT"], nb * D),
                          "ll": _nz(ll, nb), "ent": _nz(ent, nb)}
        a["genc"].fill_(1.0)

    def _ones_gloc_graw(self, a, rec):
        a["gloc"].fill_(1.0)
        a["graw"].fill_(1.0)

    _after_irt1d_grad = _after_irt1d_sparse_grad = _after_hodina_grad = _ones_gloc_graw

    def _after_norm_enc_backward(self, a, rec):
        rec["nonzero"] = {"gloc": _nz(a["gloc"], a["nb"]), "graw": _nz(a["graw"], a["nb"])}
        a["genc"].fill_(1.0)


def _make_query(name):
    def query(self, *args):
        return self.table[name]
    return query


def _make_compute(name):
    sig = inspect.signature(getattr(HipBackend, name))

    def compute(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)
        bound.apply_defaults()
        a = dict(bound.arguments)
        a.pop("self")
        self._file(name, a)
    return compute


for _n in QUERIES:
    setattr(_Recorder, _n, _make_query(_n))
for _n in COMPUTE:
    setattr(_Recorder, _n, _make_compute(_n))


class RecHip(_Recorder, HipBackend):
    """The recording backend as the HIP one (no library: HipBackend.__init__ is skipped)."""


class RecPlain(_Recorder):
    """... and as a backend that is not: what the CPU rehearsal backends of tests/ look like to the engine."""
    name = "plain"


N, J, K = 61, 7, 3


def _y(n=N, j=J):
    return torch.from_numpy(np.random.RandomState(n + j).randint(0, 2, size=(n, j)).astype(np.uint8))


def _q(j):
    q = np.zeros((K, j), dtype=np.float32)
    q[np.arange(j) % K, np.arange(j)] = 1
    return q


ROWS = (torch.arange(10, dtype=torch.int64) * 5 + 2)
ROWS2 = (torch.arange(10, dtype=torch.int64) * 6 + 1)
GUIDES = {"virt": dict(D=4), "vae": dict(D=4, amortized=True, H=64), "d1": dict(D=1), "d1_vae": dict(D=1, amortized=True, H=64)}


def _irt(be=None, cls=IrtEngine, model="irt_2pl", **kw):
    return cls(_y(), model=model, backend=RecHip() if be is None else be, **kw)


def _seam_off(name):
    return type("IrtEngineSeamOff", (IrtEngine,), {name: False})


def _pass(eng, rows=None, b_global=None, **kw):
    eng.loss_and_grads(rows, b_global, **kw)
    return eng


def _steps(eng, seq=(ROWS, ROWS2)):
    eng.use_graph = False
    eng.steps(LrSpec(1e-2), list(seq))
    return eng


def _step(eng, **kw):
    eng.use_graph = False
    eng.step(LrSpec(1e-2), **kw)
    return eng


def _off(eng, name):
    setattr(eng, name, False)                                  # (a seam read per call: the instance is the switch)
    return eng


CASES = {}
for _g, _kw in GUIDES.items():
    CASES[_g + "_full"] = lambda kw=_kw: _pass(_irt(**kw))
    CASES[_g + "_sub10"] = lambda kw=_kw: _pass(_irt(**kw), ROWS, 10)
    for _b in ("none", "avg"):
        CASES[_g + "_score_" + _b] = lambda kw=_kw, b=_b: _pass(_irt(estimator="score", baseline=b, **kw))
    CASES[_g + "_score_avg_sub10"] = lambda kw=_kw: _pass(_irt(estimator="score", baseline="avg", **kw), ROWS, 10)
    for _m in ("irt_1pl", "irt_4pl"):
        CASES[_g + "_" + _m] = lambda kw=_kw, m=_m: _pass(_irt(model=m, **kw))
CASES.update({
    "virt_share_cov": lambda: _pass(_irt(D=4, share_cov=True)),
    "virt_share_cov_score": lambda: _pass(_irt(D=4, share_cov=True, estimator="score")),
    "vae_score_scalar_kernel": lambda: _pass(_irt(be=RecHip(mvn_score_heads_workspace=-1), estimator="score", **GUIDES["vae"])),
    "vae_score_mfma_seam_off": lambda: _pass(_off(_irt(estimator="score", **GUIDES["vae"]), "score_mfma")),
    "vae_loo_2_particles": lambda: _step(_irt(estimator="score", baseline="loo", **GUIDES["vae"]), num_particles=2),
    "d1_vae_loo_2_particles_sub10": lambda: _step(_irt(estimator="score", baseline="loo", **GUIDES["d1_vae"]), rows=ROWS,
                                                  b_global=10, num_particles=2),
    "vae_2_particles": lambda: _step(_irt(**GUIDES["vae"]), num_particles=2),
    "vae_d3_h32_full": lambda: _pass(_irt(D=3, amortized=True, H=32)),
    "vae_d3_h32_sub10": lambda: _pass(_irt(D=3, amortized=True, H=32), ROWS, 10),
    "d1_vae_h32_full": lambda: _pass(_irt(D=1, amortized=True, H=32)),
    "vae_steps_two_draws_of_10": lambda: _steps(_irt(**GUIDES["vae"])),
    "vae_d3_h32_steps_two_draws_of_10": lambda: _steps(_irt(D=3, amortized=True, H=32)),
    "vae_steps_two_draws_of_12": lambda: _steps(_irt(**GUIDES["vae"]), (torch.arange(12), torch.arange(12) + 20)),
    "vae_sub10_after_padded_steps": lambda: _pass(_steps(_irt(**GUIDES["vae"])), ROWS, 10),
    "vae_step_full": lambda: _step(_irt(**GUIDES["vae"])),
    "d1_step_full_fused_tail": lambda: _step(_irt(D=1)),
    "d1_step_sub10": lambda: _step(_irt(D=1), rows=ROWS, b_global=10),
    "vae_eps": lambda: _pass(_irt(**GUIDES["vae"]), eps=torch.zeros(N, 4)),
    "vae_d3_h32_eps": lambda: _pass(_irt(D=3, amortized=True, H=32), eps=torch.zeros(N, 3)),
    "d1_vae_eps": lambda: _pass(_irt(**GUIDES["d1_vae"]), eps=torch.zeros(N)),
    "d1_score_eps": lambda: _pass(_irt(D=1, estimator="score"), eps=torch.zeros(N)),
    "vae_pad_items_off": lambda: _pass(_irt(cls=_seam_off("pad_items"), **GUIDES["vae"])),
    "vae_d3_h32_pad_hidden_off": lambda: _pass(_irt(cls=_seam_off("pad_hidden"), D=3, amortized=True, H=32)),
    "vae_d3_h32_pad_dims_off": lambda: _pass(_irt(cls=_seam_off("pad_dims"), D=3, amortized=True, H=32)),
    "vae_pad_persons_off": lambda: _pass(_off(_irt(**GUIDES["vae"]), "pad_persons")),
    "d1_vae_pad_persons_off": lambda: _pass(_off(_irt(**GUIDES["d1_vae"]), "pad_persons")),
    "vae_pad_batch_off_steps": lambda: _steps(_off(_irt(**GUIDES["vae"]), "pad_batch")),
    "vae_layout0": lambda: _pass(_irt(be=RecHip(mvn_enc_bwd_layout=0), **GUIDES["vae"])),
    "vae_layout0_sub10": lambda: _pass(_irt(be=RecHip(mvn_enc_bwd_layout=0), **GUIDES["vae"]), ROWS, 10),
    "vae_gd_offset_none": lambda: _pass(_irt(be=RecHip(mvn_enc_bwd_gd_offset=-1), **GUIDES["vae"])),
    "vae_layout0_gd_offset_none_steps": lambda: _steps(_irt(be=RecHip(mvn_enc_bwd_layout=0, mvn_enc_bwd_gd_offset=-1),
                                                            **GUIDES["vae"])),
    "vae_no_hs_no_opmax_no_ximg": lambda: _pass(_irt(be=RecHip(mvn_enc_bwd_hs_offset=-1, mvn_pack_opmax_offset=-1,
                                                               lik_ximg_bytes=0, norm_enc_pack_floats=0), **GUIDES["vae"])),
    "d1_vae_no_pack": lambda: _pass(_irt(be=RecHip(norm_enc_pack_floats=0), **GUIDES["d1_vae"])),
    "vae_64_persons": lambda: _pass(IrtEngine(_y(64, 8), backend=RecHip(), **GUIDES["vae"])),
    "vae_7_persons": lambda: _pass(IrtEngine(_y(7, 8), backend=RecHip(), **GUIDES["vae"])),
    "plain_vae_full": lambda: _pass(_irt(be=RecPlain(mvn_enc_bwd_layout=0, mvn_enc_bwd_gd_offset=-1, mvn_enc_bwd_hs_offset=-1),
                                         **GUIDES["vae"])),
    "plain_vae_steps": lambda: _steps(_irt(be=RecPlain(mvn_enc_bwd_layout=0, mvn_enc_bwd_gd_offset=-1, mvn_enc_bwd_hs_offset=-1),
                                           **GUIDES["vae"])),
    "plain_vae_dim_major": lambda: _pass(_irt(be=RecPlain(), **GUIDES["vae"])),
    "plain_d1_step": lambda: _step(_irt(be=RecPlain(), D=1)),
    "plain_d1_vae_full": lambda: _pass(_irt(be=RecPlain(), **GUIDES["d1_vae"])),
    "plain_vae_score": lambda: _pass(_irt(be=RecPlain(), estimator="score", **GUIDES["vae"])),
    "hodina_vae_j30_h32": lambda: _pass(HoDinaEngine(_y(N, 30), _q(30), amortized=True, H=32, backend=RecHip())),
    "hodina_vae_j30_h32_sub10": lambda: _pass(HoDinaEngine(_y(N, 30), _q(30), amortized=True, H=32, backend=RecHip()), ROWS, 10),
    "hodina_vae_plain": lambda: _pass(HoDinaEngine(_y(N, 30), _q(30), amortized=True, H=32, backend=RecPlain())),
    "hodina_per_person": lambda: _pass(HoDinaEngine(_y(N, 30), _q(30), backend=RecHip())),
    "hodina_per_person_step": lambda: _step(HoDinaEngine(_y(N, 30), _q(30), backend=RecHip())),
    "cdm_sf": lambda: _pass(CdmSfEngine(_y(), _q(J), backend=RecHip())),
    "cdm_sf_vae_avg_sub10": lambda: _pass(CdmSfEngine(_y(), _q(J), amortized=True, H=64, baseline="avg", backend=RecHip()),
                                          ROWS, 10),
    "cdm_sf_loo_2_particles": lambda: _step(CdmSfEngine(_y(), _q(J), baseline="loo", backend=RecHip()), num_particles=2),
})


def _after(eng):
    """What the pass left behind that tests and tools read."""
    out = {"last": sorted(eng.last), "nb": eng.last.get("nb"), "n_valid": eng.last.get("n_valid"), "n_pad": eng._n_pad,
           "t": eng.t, "shapes": [getattr(eng, k, None) for k in ("J", "D", "H")],
           "last_fw": sorted(eng.last["fw"]) if "fw" in eng.last else None,
           "last_log_r": _describe(getattr(eng, "last_log_r", None)), "buffers": sorted(eng._ws),
           "phantom_rows": getattr(eng, "_phantom_rows", None),
           "y_copies": [_describe(getattr(eng, k, None)) for k in ("y", "y_lik", "_y_ext", "_y_ext_lik", "_y_pad", "_y_pad_lik",
                                                                    "_yT", "y_enc", "_yT_enc")]}
    if getattr(eng, "n_enc", 0):
        out["genc_nonzero"] = {k: _nz(eng.view("encoder$$$" + k, eng.G), 1 << 30) for k in eng.enc_shapes}
    return out


def trace(case):
    torch.manual_seed(0)
    eng = CASES[case]()
    return json.loads(json.dumps({"calls": eng.be.calls, "after": _after(eng)}))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_trace(case, golden):
    got, want = trace(case), golden[case]
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w, "%s: %s" % (case, g["call"])
    assert got["after"] == want["after"]


def test_the_shape_the_issue_names():
    """61 persons x 7 items, D = 4, amortized: launched over 64 persons and 8 items, and the backward sees the 61 x 4 entries
    of gxT / gdT and the 61 of ll / ent that belong to persons -- the three phantoms are gone."""
    t = trace("vae_full")
    bw = [c for c in t["calls"] if c["call"] == "mvn_enc_backward"][0]
    assert bw["nb"] == 64 and bw["cfg"]["J"] == 8
    assert bw["nonzero"] == {"gx": None, "gxT": 244, "gdT": 244, "ll": 61, "ent": 61}
    t = trace("vae_steps_two_draws_of_10")                     # phantom rows: 12 launched, 10 kept
    for bw in [c for c in t["calls"] if c["call"] == "mvn_enc_backward"]:
        assert bw["nb"] == 12 and bw["nonzero"] == {"gx": None, "gxT": 40, "gdT": 40, "ll": 10, "ent": 10}


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python -m tests.test_engine_call_trace --record")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join('%s: %s' % (json.dumps(c), json.dumps(trace(c), sort_keys=True, separators=(",", ":")))
                                  for c in sorted(CASES)) + "\n}\n")
    print("recorded %d cases, %d bytes" % (len(CASES), os.path.getsize(GOLDEN)))
