"""The gates of vx_grid_wtable_irt_map and of vx_grid_info at the new K limit through the built library, without a GPU
(tests/test_se_map_host.py runs this in a child process and reads one JSON line): each entry with ONE argument wrong at a time,
everything else a call that would be launched -- each must come back with VX_EINVAL (-1) before the HIP runtime is touched.
Every pointer is a 16-byte-aligned HOST buffer that nothing may be read through."""
import ctypes
import json

from vipsy_amd import _hip

_RAW = (ctypes.c_uint8 * (1 << 12))()
ADDR = (ctypes.addressof(_RAW) + 15) & ~15
BUF = ctypes.c_void_p(ADDR)
OFF4 = ctypes.c_void_p(ADDR + 4)

TABLE_ARGS = "cfg theta G a b c_un d_un wimg hs".split()
TABLE_BASE = dict(model=4, D=1, J=37, G=61)                        # a 4PL call that passes the gate
TABLE_ROWS = [
    ("model 0", dict(model=0)), ("model 5", dict(model=5)), ("D 4", dict(D=4)), ("1PL with D 2", dict(model=1, D=2)),
    ("2PL without a", dict(model=2, a=None)), ("3PL without c_un", dict(model=3, c_un=None)), ("4PL without d_un", dict(d_un=None)),
    ("J 1025", dict(J=1025)), ("G 1025", dict(G=1025)), ("wimg off by 4 bytes", dict(wimg=OFF4)), ("no theta", dict(theta=None)),
    ("no wimg", dict(wimg=None)), ("no b", dict(b=None)), ("no cfg", dict(cfg=None)), ("4PL D 3 with J 683", dict(D=3, J=683)),
]

INFO_ARGS = "y rows nb J G K img wimg logw loglik info gradient workspace ws_floats hs".split()
INFO_BASE = dict(nb=300, J=37, G=61, K=4, ws_floats=1 << 28)        # a call that passes the gate
INFO_ROWS = [("vx_grid_info with K 7", dict(K=7)), ("vx_grid_info with K 6, J 683", dict(K=6, J=683)), ("vx_grid_info with K 0", dict(K=0))]


def table_arguments(change, keep):
    v = dict(TABLE_BASE, **change)
    call = []
    for k in TABLE_ARGS:
        if k == "cfg":
            keep.append(_hip.IrtCfg(v["model"], v["D"], v["J"], 0, 1.702, 1.0, 0, 0, 0))
            call.append(None if "cfg" in change else ctypes.byref(keep[-1]))
        elif k == "hs":
            call.append(None)
        else:
            call.append(v[k] if k in v else BUF)
    return call


def info_arguments(change):
    v = dict(INFO_BASE, **change)
    return [None if k in ("hs", "rows") else (v[k] if k in v else BUF) for k in INFO_ARGS]


def gates():
    L = _hip.lib()
    out = []
    for label, change in TABLE_ROWS:
        keep = []
        out.append([label, int(L.vx_grid_wtable_irt_map(*table_arguments(change, keep)))])
    for label, change in INFO_ROWS:
        out.append([label, int(L.vx_grid_info(*info_arguments(change)))])
    return out


if __name__ == "__main__":
    print(json.dumps(gates(), separators=(",", ":")))
