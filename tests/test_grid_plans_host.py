"""The host half of the grid family (vx_grid_*, vx_sumscore_*), pinned on the CPU.

The plans of vipsy_amd/csrc/grid_plan.h decide the order of every sum these entries promise to repeat bit for bit, and they are
otherwise reachable only through a GPU call.  Three checks, none of which needs a device:

  plans     tests/helpers/grid_plans.cpp includes the header alone and prints every field of every plan over a sweep of shapes and
            workspace sizes; it is compiled with the host compiler under AddressSanitizer + UBSan (a stand-alone program: nothing
            is preloaded) and its output compared with tests/golden/grid_plans.json;
  queries   the ten size queries of the built library over the same shapes, against tests/golden/grid_queries.json;
  gates     every compute entry with one argument wrong at a time: VX_EINVAL before the HIP runtime is touched.

Both fixtures were recorded BEFORE the plans moved into grid_plan.h: the same driver compiled host-only against GiPlan / gi_plan,
PpPlan / pp_plan, gc_plan, gcc_*, gf_plan and ss_plan as they stood in the k_grid_*.hip files (a thin adapter gave them the names
of the header), and the same helper against the library of that commit.  A refactor of the plans or of the dispatch in vx_abi.hip
must leave every value where it was."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")
GOLDEN = os.path.join(ROOT, "tests", "golden")

sys.path.insert(0, HELPERS)


def _first_difference(want, got, path=""):
    if type(want) is not type(got):
        return "%s: %r != %r" % (path, want, got)
    if isinstance(want, dict):
        if sorted(want) != sorted(got):
            return "%s: keys %s != %s" % (path, sorted(want), sorted(got))
        for k in want:
            d = _first_difference(want[k], got[k], "%s.%s" % (path, k))
            if d:
                return d
    elif isinstance(want, list):
        if len(want) != len(got):
            return "%s: %d entries != %d" % (path, len(want), len(got))
        for i, (w, g) in enumerate(zip(want, got)):
            d = _first_difference(w, g, "%s[%d]" % (path, i))
            if d:
                return d
    elif want != got:
        return "%s: %r != %r" % (path, want, got)
    return None


def test_plans_match_the_recorded_plans_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler"
    exe = str(tmp_path / "grid_plans")
    # the sanitizers' runtimes linked INTO the program (clang's default; g++ has to be told)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "vipsy_amd", "csrc"), "-o", exe,
                           os.path.join(HELPERS, "grid_plans.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    got = json.loads(r.stdout)
    with open(os.path.join(GOLDEN, "grid_plans.json")) as f:
        want = json.load(f)
    assert _first_difference(want, got) is None
    # the sweep is the one the fixture was recorded over, and no part of it is empty
    s = got["sweep"]
    assert len(got["slab_info"]) == len(s["info_P"]) and len(got["slab_pairs"]) == len(s["pairs_J"])
    assert all(len(shape[-1]) == 6 * len(s["nb"]) for shape in got["slab_info"] + got["slab_pairs"])
    assert len(got["gc"]) == len(s["gc_J"]) * len(s["gc_G"]) * len(s["nb"])
    assert len(got["gf"]) == len(s["gf_nb"]) and len(got["ss"]) == len(s["ss_Js"]) * len(s["ss_G"])


def _helper(mode):
    import __graft_entry__ as g
    g.build()
    env = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(HELPERS, "grid_queries.py"), mode], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_size_queries_match_the_recorded_sizes():
    got = _helper("queries")
    with open(os.path.join(GOLDEN, "grid_queries.json")) as f:
        want = json.load(f)
    assert len(want) == 10
    assert _first_difference(want, got) is None
    assert all(v > 0 for row in got.values() for v in row)                 # every shape of the sweep is inside the limits
    # the preferred workspace of the headline shapes of item_se() and local_dependence(): one slab, by hand from SlabPlan
    import grid_queries as gq
    L_info = dict(zip([(P, nb) for P in gq.INFO_P for nb in gq.NBS], got["vx_grid_info_workspace_floats"]))
    assert L_info[(74, 549)] == (3 * 8 * 3 + (3 + 2) * 6) * 1024           # 3 granules x 8 units x 3 tiles; 3 chunks + 2 of 6 pairs
    L_pairs = dict(zip([(J, nb) for J in gq.PAIRS_J for nb in gq.NBS], got["vx_grid_pairs_workspace_floats"]))
    assert L_pairs[(37, 549)] == 3 * 8 * 2 * 2 * 5 * 256 + (3 + 2) * 3 * 6 * 1024


def test_every_gate_refuses_one_wrong_argument_before_the_runtime():
    import grid_queries as gq
    got = _helper("gates")
    want = [(name, label) for name in gq.ENTRIES for label, _ in gq.rows_of(name)]
    assert [(n, l) for n, l, _ in got] == want
    passed = [(n, l, rc) for n, l, rc in got if rc != -1]
    assert not passed, passed
    # the table covers what it says: all eighteen compute entries, each model gate, each person limit, both draw ranges
    labels = {}
    for n, l in want:
        labels.setdefault(n, []).append(l)
    assert len(labels) == 18 and all(n in _SIGNATURES() for n in labels)
    irt = [n for n in labels if n.endswith("_irt")]
    cdm = [n for n in labels if n.endswith("_cdm")]
    assert len(irt) == 6 and len(cdm) == 5
    for n in irt:
        assert {"D over the limit", "model 0", "model 5", "1PL with D 2", "2PL without a"} <= set(labels[n])
        assert ("model 3" in labels[n]) == (n in gq.TWO_PL_ONLY)
        assert ("4PL without d_un" in labels[n]) == (n not in gq.TWO_PL_ONLY)
    for n in cdm:
        assert {"dino 2", "K 11", "J 1025"} <= set(labels[n])
    with_persons = [n for n in labels if "nb 0" in labels[n]]
    assert len(with_persons) == 12 and all({"nb 2^48 + 1", "J 1025"} <= set(labels[n]) for n in with_persons)
    assert sorted(n for n in labels if "draw0 -1" in labels[n]) == ["vx_grid_draw", "vx_grid_draw_cond"]
    assert sum("off by 4 bytes" in l for n, l in want) == 8 and sum(l == "G 1025" for n, l in want) == 7


def _SIGNATURES():
    from vipsy_amd import _hip
    return _hip.SIGNATURES
