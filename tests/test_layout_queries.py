"""The workspace and pack-buffer layout of the amortized multivariate guide and the likelihood, as the size and offset queries
report it, pinned on the CPU (no GPU: the library plans for 256 CUs).  engine.py cuts gdT, hs and the operand maxima out of
the caller's buffers at these offsets, so a refactor of the dispatch in vx_abi.hip must leave every value where it was.

tests/golden/layout_queries.json holds what tests/helpers/layout_queries.py printed for the library before the guide's kernel
and layout choices moved into one plan per path: a list of the eight queries per shape of layout_queries.cases(), for the
default kernels and for each VX_* switch setting that changes a choice.  Each setting runs in a child process of its own
(the library reads the switches once)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "layout_queries.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_queries.json")
SEAMS = {"default": {}, "mfma16_0": {"VX_MFMA16": "0"}, "mfma16_w": {"VX_MFMA16": "w"}, "mfma16_h": {"VX_MFMA16": "h"},
         "mfma16_g": {"VX_MFMA16": "g"}, "generic": {"VX_FORCE_GENERIC": "1"}}

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import layout_queries as lq  # noqa: E402


def _query(seam):
    import __graft_entry__ as g
    g.build()
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    env.update(SEAMS[seam], PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, HELPER], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_layout_queries_match_the_recorded_layout(seam):
    want = json.load(open(GOLDEN))[seam]
    got = _query(seam)
    cases = lq.cases()
    assert len(want) == len(cases) == len(got)
    diff = [(c, dict(zip(lq.QUERIES, w)), dict(zip(lq.QUERIES, g))) for c, w, g in zip(cases, want, got) if w != g]
    assert not diff, "%d of %d shapes moved; first: %s" % (len(diff), len(cases), diff[:3])
    if seam == "default":               # the headline shape: D 100, J 500, H 64, 1M persons
        row = dict(zip(lq.QUERIES, got[cases.index((2, 100, 500, 64, 1000000))]))
        assert row["vx_mvn_enc_bwd_workspace_floats"] == 246838540
        assert row["vx_mvn_enc_bwd_gd_offset"] == 82458624
        assert row["vx_mvn_enc_bwd_hs_offset"] == 182458628


@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_layout_regions_lie_inside_their_buffers(seam):
    for (model, D, J, H, nb), row in zip(lq.cases(), _query(seam)):
        q = dict(zip(lq.QUERIES, row))
        pack, total = q["vx_mvn_pack_floats"], q["vx_mvn_enc_bwd_workspace_floats"]
        gd, hs, opmax = q["vx_mvn_enc_bwd_gd_offset"], q["vx_mvn_enc_bwd_hs_offset"], q["vx_mvn_pack_opmax_offset"]
        where = (seam, model, D, J, H, nb, q)
        assert pack > 0 and total > 0 and q["vx_irt_lik_workspace_floats"] > 0 and q["vx_irt_lik_ximg_bytes"] >= 0, where
        assert q["vx_mvn_enc_bwd_layout"] in (0, 1), where
        if q["vx_mvn_enc_bwd_layout"] == 1:
            assert gd >= 0 or nb * D % 4 != 0, where        # the dimension-major backward reads gdT from the workspace
        if gd >= 0:
            assert gd % 4 == 0 and gd + nb * D + 4 <= total, where
        if hs >= 0:
            assert gd >= 0 and hs % 4 == 0 and hs >= gd + nb * D + 4 and hs + nb * 64 <= total, where
        if opmax >= 0:
            assert hs >= 0 and 0 <= opmax and opmax + 4 <= pack, where
