"""The kernels a step of the amortized multivariate guide launches, pinned: which generation of the forward, the likelihood,
the hidden gradient, the head weight gradient and the fc1 gradient a call takes is decided by the host dispatch of
vx_abi.hip, and a slower generation computes the same numbers -- the oracle comparisons cannot see a silent downgrade.

tests/golden/gpu_routes.json holds what tests/helpers/gpu_routes.py printed on an MI355X (256 CUs) for the library before
the backward's route moved into a resolver (BwdRoute): per switch setting and batch size, every measurement slot's name, its
launches and its `units` (the persons of a launch that is not the whole batch).  Times are not compared.  2PL, D = 100,
J = 500, H = 64; 512 persons: the small-batch forms; 33 024: the large-batch forms, whole workgroups only; 70 016: a short
last chip round beside the whole rounds (65 536 persons) in the forward and the hidden gradient."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "gpu_routes.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gpu_routes.json")
SEAMS = {"default": {}, "mfma16_0": {"VX_MFMA16": "0"}, "generic": {"VX_FORCE_GENERIC": "1"}}
PAIR = "k_mvn_enc_bwd_h_b2 | k_mvn_enc_bwd_w_b side by side"          # bench.py's name for the backward pair


@pytest.mark.gpu
@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_a_step_takes_the_recorded_route(seam):
    want = json.load(open(GOLDEN))[seam]
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    env.update(SEAMS[seam], PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, HELPER], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == sorted(want) == ["33024", "512", "70016"]
    for N in want:
        assert got[N] == want[N], (seam, N, [s for s in got[N] if s not in want[N]], [s for s in want[N] if s not in got[N]])
    if seam == "default":               # the table against a reading of the dispatch: the headline route at 70 016 persons
        big = {name: (launches, units) for name, launches, units in got["70016"]}
        assert big["k_mvn_enc_fwd_b2"] == (1, 65536)
        assert big[PAIR] == (1, 0)
        assert "k_mvn_enc_fwd_b" not in big                              # its last round ran beside the whole rounds: not filed
        small = {name for name, _, _ in got["512"]}
        assert "k_mvn_enc_fwd_b" in small and "k_mvn_enc_fwd_b2" not in small
