"""The item-wise M-step kernel, bit for bit: one sha256 a launch over the launches the GPU suite holds it to.

A change that is not meant to move the arithmetic of k_grid_mstep_irt (vipsy_amd/csrc/k_grid_mstep.hip) is shown not to by running
this on both commits, for the same build, and comparing the two files byte for byte: every sum of the kernel runs in a fixed order,
so the same build on the same tables gives the same bits.  Only the Python entry points are used, so the file runs on any commit
that has them.  The launches:
  * vx_grid_mstep_irt (HipBackend.grid_mstep_irt): every entry of tests/em_cases.STEP_CASES -- the cap, halving, clamp and stop
    paths and the grids either side of the 64-lane boundaries, D = 1 .. 3, 1PL and 2PL -- at newton = 1, 4 and 64;
  * vx_grid_mstep_irt_map (HipBackend.grid_mstep_irt_map, with lprior): every launch of tests/map_cases -- the cases from their
    start and their near start, the far starts, the pivot / steep / falling launches -- at newton = 1 and 64.
A line is `<entry> <launch> newton=<n> <sha256 of the bytes of a, b, c_un, d_un, lprior as far as the launch has them>`.

usage (GPU box):  python tools/mstep_bits.py [out.txt]        VX_LIB=<library> selects another build (vipsy_amd/_hip.py)"""
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import em_cases as ec                                                 # noqa: E402
from tests import map_cases as mc                                                # noqa: E402
from vipsy_amd import _hip                                                       # noqa: E402
from vipsy_amd.engine import HipBackend                                          # noqa: E402

dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev).contiguous()


def digest(outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        if o is not None:
            h.update(o.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def plain(be, spec, newton):
    c = ec.step_case(spec)
    two = spec["model"] != "irt_1pl"
    a, b = (_t(c["a0"]) if two else None), _t(c["b0"].reshape(-1))
    fr = _t(c["free"]) if two else None
    cfg = be.cfg(spec["model"], spec["D"], c["J"], 0, spec["Dc"], 1.0, 0, 0, 0)
    be.grid_mstep_irt(cfg, _t(c["theta"]), c["G"], _t(c["n1"]), _t(c["n0"]), fr, a, b, newton)
    return digest((a, b))


def penalised(be, cs, L, p0, newton):
    m, D = mc.MODEL_NO[cs["model"]], cs["D"]
    a = _t(p0[1:1 + D]) if m >= 2 else None
    fr = _t(cs["a_free"]) if m >= 2 and cs["a_free"] is not None else None
    b, c, d = _t(p0[0]), (_t(p0[4]) if m >= 3 else None), (_t(p0[5]) if m == 4 else None)
    lp = torch.full((cs["J"],), float("nan"), device=dev)
    cfg = be.cfg(cs["model"], D, cs["J"], 0, cs["Dc"], 1.0, 0, 0, 0)
    be.grid_mstep_irt_map(cfg, _t(cs["theta"]), cs["G"], _t(L["n1"]), _t(L["n0"]), fr, a, b, c, d, _t(L["prior"]), newton, lp)
    return digest((a, b, c, d, lp))


def map_launches():
    for name in mc.CASES:
        yield name, mc.case(name), mc.launch(name), "p0"
        yield name + "_near", mc.case(name), mc.launch(name), "p0_near"
    for far in mc.FAR:
        yield "far_" + mc.far_id(far), mc.case(far[0]), mc.far_launch(far), "p0"
    for tag, name, L in (("pivot", mc.PIVOT_CASE, mc.pivot_launch()), ("steep", mc.STEEP_CASE, mc.steep_launch()),
                         ("falling", mc.FALLING_CASE, mc.falling_launch())):
        yield tag, mc.case(name), L, "p0"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("mstep_bits: %s, torch %s, %s, %s" % (torch.cuda.get_device_name(0), torch.__version__, os.path.basename(_hip.LIB_PATH),
                                                time.strftime("%Y-%m-%d")))
    be = HipBackend()
    for spec in ec.STEP_CASES:
        for newton in (1, 4, 64):
            say("vx_grid_mstep_irt %s newton=%d %s" % (spec["name"], newton, plain(be, spec, newton)))
    for tag, cs, L, start in map_launches():
        for newton in (1, 64):
            say("vx_grid_mstep_irt_map %s newton=%d %s" % (tag, newton, penalised(be, cs, L, L[start], newton)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines[1:]) + "\n")                  # (without the line that names the day and the build)
    return 0


if __name__ == "__main__":
    sys.exit(main())
