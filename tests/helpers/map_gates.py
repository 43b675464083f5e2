"""The gate of vx_grid_mstep_irt_map through the built library, without a GPU (tests/test_map_host.py runs this in a child
process and reads one JSON line): the entry with ONE argument wrong at a time, everything else a call that would be launched --
each must come back with VX_EINVAL (-1) before the HIP runtime is touched.  Every pointer is a 16-byte-aligned HOST buffer that
nothing may be read through: that is also why the gate cannot look at the precisions inside `prior` (vipsy_amd/grid.py does)."""
import ctypes
import json

from vipsy_amd import _hip

_RAW = (ctypes.c_uint8 * (1 << 12))()
BUF = ctypes.c_void_p((ctypes.addressof(_RAW) + 15) & ~15)
ARGS = "cfg theta G n1 n0 a_free a b c_un d_un prior newton lprior hs".split()
BASE = dict(model=4, D=1, J=37, G=61, newton=4)                    # a 4PL call that passes the gate

ROWS = [
    ("model 0", dict(model=0)), ("model 5", dict(model=5)), ("D 0", dict(D=0)), ("D 4", dict(D=4)), ("1PL with D 2", dict(model=1, D=2)),
    ("J 0", dict(J=0)), ("J 1025", dict(J=1025)), ("G 0", dict(G=0)), ("G 1025", dict(G=1025)),
    ("newton 0", dict(newton=0)), ("newton 65", dict(newton=65)),
    ("no cfg", dict(cfg=None)), ("no theta", dict(theta=None)), ("no n1", dict(n1=None)), ("no n0", dict(n0=None)), ("no b", dict(b=None)),
    ("2PL without a", dict(model=2, a=None)), ("3PL without c_un", dict(model=3, c_un=None)), ("4PL without c_un", dict(c_un=None)),
    ("4PL without d_un", dict(d_un=None)), ("no prior", dict(prior=None)), ("2PL without prior", dict(model=2, prior=None)),
]


def arguments(change, keep):
    v = dict(BASE, **change)
    call = []
    for k in ARGS:
        if k == "cfg":
            keep.append(_hip.IrtCfg(v["model"], v["D"], v["J"], 0, 1.702, 1.0, 0, 0, 0))
            call.append(None if "cfg" in change else ctypes.byref(keep[-1]))
        elif k == "hs":
            call.append(None)
        else:
            call.append(v[k] if k in v else BUF)                    # (a_free and lprior may be NULL: BUF here)
    return call


def gates():
    L = _hip.lib()
    out = []
    for label, change in ROWS:
        keep = []
        out.append([label, int(L.vx_grid_mstep_irt_map(*arguments(change, keep)))])
    return out


if __name__ == "__main__":
    print(json.dumps(gates(), separators=(",", ":")))
