"""The host side of the grid family (vx_grid_*, vx_sumscore_*) through the built library, without a GPU
(tests/test_grid_plans_host.py runs this in a child process and reads one JSON line):

  queries   what the ten size queries return over the shapes of tests/helpers/grid_plans.cpp -- without a device the library
            plans for 256 CUs, and none of these plans looks at the device anyway;
  gates     every compute entry with ONE argument wrong at a time, everything else a call that would be launched: each must come
            back with VX_EINVAL (-1) before the HIP runtime is touched.  Every pointer is a 16-byte-aligned HOST buffer that
            nothing may be read through (vx_grid_counts_cond's seg_start, which IS host memory, holds a valid cut)."""
import ctypes
import json
import sys

from vipsy_amd import _hip

NBS = (1, 255, 256, 257, 549, 4096, 33024, 1000000, 1 << 24)
INFO_P = (1, 31, 32, 74, 1000, 4096)
PAIRS_J = (1, 32, 33, 37, 500, 1024)
GC_J = (1, 37, 256, 257, 512, 513, 1024)
GC_G = (1, 32, 61, 512, 1024)
GC_SEG = (1, 2, 7, 4096)
GF_NBS = NBS + (32 * 1024, 32 * 1024 + 1)
SS_JS = (1, 2, 37, 1023)
SS_G = (1, 61, 1024)


def queries():
    L = _hip.lib()
    return {
        "vx_grid_image_bytes": [L.vx_grid_image_bytes(J, G) for J in GC_J for G in GC_G],
        "vx_grid_wimage_bytes": [L.vx_grid_wimage_bytes(P, G) for P in INFO_P for G in GC_G],
        "vx_grid_counts_workspace_floats": [L.vx_grid_counts_workspace_floats(nb, J, G) for J in GC_J for G in GC_G for nb in NBS],
        "vx_grid_counts_cond_workspace_floats": [L.vx_grid_counts_cond_workspace_floats(nb, n_seg, J, G)
                                                 for J in GC_J for G in GC_G for nb in NBS for n_seg in GC_SEG],
        "vx_grid_info_workspace_floats": [L.vx_grid_info_workspace_floats(nb, P, 61) for P in INFO_P for nb in NBS],
        "vx_grid_info_workspace_min_floats": [L.vx_grid_info_workspace_min_floats(P, 61) for P in INFO_P],
        "vx_grid_pairs_workspace_floats": [L.vx_grid_pairs_workspace_floats(nb, J) for J in PAIRS_J for nb in NBS],
        "vx_grid_pairs_workspace_min_floats": [L.vx_grid_pairs_workspace_min_floats(J) for J in PAIRS_J],
        "vx_grid_fit_workspace_floats": [L.vx_grid_fit_workspace_floats(nb, J) for J in PAIRS_J for nb in GF_NBS],
        "vx_sumscore_model_workspace_floats": [L.vx_sumscore_model_workspace_floats(Js, G) for Js in SS_JS for G in SS_G],
    }


# ---- gates -------------------------------------------------------------------------------------------------------------------
_RAW = (ctypes.c_uint8 * (1 << 16))()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15
BUF = ctypes.c_void_p(_BASE)                          # 16-byte aligned
OFF4 = ctypes.c_void_p(_BASE + 4)                     # the same buffer, off by 4 bytes
NB, J, G, K_CDM = 549, 37, 61, 3
TOO_MANY = (1 << 48) + 1

IRT = ("cfg", "model", "D", "J")                      # the fields of vx_irt_cfg a row may set
CDM = ("cfg", "K", "J")

# entry -> (its arguments in order, the values of a call that passes the gate).  "cfg" is built from the model / D / J or K / J
# keys; every argument not listed is BUF (hs: the null stream).
ENTRIES = {
    "vx_grid_table_irt": ("cfg theta G a b c_un d_un img hs", dict(model=2, D=1, J=J, G=G)),
    "vx_grid_table_cdm": ("cfg dino q g_un s_un img hs", dict(K=K_CDM, J=J, dino=0)),
    "vx_grid_posterior": ("y rows nb J G D img logw coord loglik mean sd argmax hs", dict(nb=NB, J=J, G=G, D=1)),
    "vx_grid_draw": ("y rows nb J G img logw seed row_offset draw0 ndraws stride node hs",
                     dict(nb=NB, J=J, G=G, seed=1, row_offset=0, draw0=0, ndraws=5, stride=5)),
    "vx_grid_posterior_cond": ("y rows nb J G D img logw coord tilt logjoint lognorm mean cov argmax hs", dict(nb=NB, J=J, G=G, D=1)),
    "vx_grid_draw_cond": ("y rows nb J G D img logw coord tilt seed row_offset draw0 ndraws stride node hs",
                          dict(nb=NB, J=J, G=G, D=1, seed=1, row_offset=0, draw0=0, ndraws=5, stride=5)),
    "vx_grid_counts": ("y rows nb J G img logw loglik n1 n0 mass workspace hs", dict(nb=NB, J=J, G=G)),
    "vx_grid_counts_cond": ("y rows nb J G D img logw coord tilt logjoint seg_start n_seg n1 n0 mass workspace hs",
                            dict(nb=NB, J=J, G=G, D=1, n_seg=1)),
    "vx_grid_mstep_irt": ("cfg theta G n1 n0 a_free a b newton hs", dict(model=2, D=1, J=J, G=G, newton=4)),
    "vx_grid_mstep_cdm": ("cfg dino q n1 n0 g_un s_un hs", dict(K=K_CDM, J=J, dino=0)),
    "vx_grid_wtable_irt": ("cfg theta G a b wimg hs", dict(model=2, D=1, J=J, G=G)),
    "vx_grid_wtable_cdm": ("cfg dino q g_un s_un wimg hs", dict(K=K_CDM, J=J, dino=0)),
    "vx_grid_info": ("y rows nb J G K img wimg logw loglik info gradient workspace ws_floats hs", dict(nb=NB, J=J, G=G, K=2)),
    "vx_grid_pairs_irt": ("cfg y rows nb theta_hat a b c_un d_un n s ss sp workspace ws_floats hs", dict(model=2, D=1, J=J, nb=NB)),
    "vx_grid_pairs_cdm": ("cfg dino q y rows nb pattern g_un s_un n s ss sp workspace ws_floats hs", dict(K=K_CDM, J=J, dino=0, nb=NB)),
    "vx_grid_fit_irt": ("cfg y rows nb theta_hat a b c_un d_un person item workspace ws_floats hs", dict(model=2, D=1, J=J, nb=NB)),
    "vx_grid_fit_cdm": ("cfg dino q y rows nb pattern g_un s_un person item workspace ws_floats hs", dict(K=K_CDM, J=J, dino=0, nb=NB)),
    "vx_grid_point_irt": ("cfg y rows nb theta0 a b c_un d_un method max_iter tol bound step_cap theta_hat info status iters hs",
                          dict(model=2, D=1, J=J, nb=NB, method=0, max_iter=32, tol=1e-6, bound=6.0, step_cap=1.0)),
}
D_LIMIT = {"vx_grid_table_irt": 10}                   # GP_MAXD; every other *_irt entry: 3
TWO_PL_ONLY = ("vx_grid_mstep_irt", "vx_grid_wtable_irt")


def rows_of(name):
    """(label, the arguments that differ from the entry's passing call) -- one thing wrong a row."""
    names, base = ENTRIES[name]
    names = names.split()
    out = []
    if name.endswith("_irt"):
        out += [("D over the limit", dict(D=D_LIMIT.get(name, 3) + 1)), ("model 0", dict(model=0)), ("model 5", dict(model=5)),
                ("1PL with D 2", dict(model=1, D=2)), ("2PL without a", dict(a=None))]
        if name in TWO_PL_ONLY:
            out += [("model 3", dict(model=3))]
        else:
            out += [("3PL without c_un", dict(model=3, c_un=None)), ("4PL without d_un", dict(model=4, d_un=None))]
    if name.endswith("_cdm"):
        out += [("dino 2", dict(dino=2)), ("K 11", dict(K=11)), ("J 1025", dict(J=1025))]
    if "nb" in names:
        out += [("nb 0", dict(nb=0)), ("nb 2^48 + 1", dict(nb=TOO_MANY))]
        if not name.endswith("_cdm"):
            out += [("J 1025", dict(J=1025))]
        if "G" in names:
            out += [("G 1025", dict(G=1025))]
        out += [("%s off by 4 bytes" % k, {k: OFF4}) for k in ("img", "wimg") if k in names]
    if "draw0" in names:
        out += [("draw0 -1", dict(draw0=-1)), ("ndraws 0", dict(ndraws=0)), ("draws beyond 1024", dict(draw0=1, ndraws=1024, stride=1025)),
                ("stride below the draws", dict(stride=4))]
    if name == "vx_grid_point_irt":
        out += [("method 3", dict(method=3)), ("max_iter 0", dict(max_iter=0)), ("max_iter 256", dict(max_iter=256)),
                ("tol 0", dict(tol=0.0)), ("tol inf", dict(tol=float("inf"))), ("WLE with D 2", dict(method=2, D=2))]
    return out


def arguments(name, change, keep):
    names, base = ENTRIES[name]
    v = dict(base, **change)
    L = _hip.lib()
    call = []
    for k in names.split():
        if k == "cfg" and "model" in v:
            keep.append(_hip.IrtCfg(v["model"], v["D"], v["J"], 0, 1.0, 1.0, 0, 0, 0))
            call.append(ctypes.byref(keep[-1]))
        elif k == "cfg":
            keep.append(_hip.HoDinaCfg())
            keep[-1].K, keep[-1].J, keep[-1].scale = v["K"], v["J"], 1.0
            call.append(ctypes.byref(keep[-1]))
        elif k == "hs":
            call.append(None)
        elif k == "seg_start":                        # host memory by contract: one segment of the BASE call's persons
            keep.append((ctypes.c_int64 * 2)(0, base["nb"]))
            call.append(ctypes.cast(keep[-1], ctypes.c_void_p))
        elif k == "ws_floats":                        # what the BASE shape needs, so that only the changed argument is wrong
            if name == "vx_grid_info":
                call.append(L.vx_grid_info_workspace_min_floats(base["J"] * base["K"], base["G"]))
            elif "pairs" in name:
                call.append(L.vx_grid_pairs_workspace_min_floats(base["J"]))
            else:
                call.append(L.vx_grid_fit_workspace_floats(base["nb"], base["J"]))
            assert call[-1] > 0
        else:
            call.append(v[k] if k in v else BUF)
    return call


def gates():
    L = _hip.lib()
    out = []
    for name in ENTRIES:
        for label, change in rows_of(name):
            keep = []
            out.append([name, label, int(getattr(L, name)(*arguments(name, change, keep)))])
    return out


if __name__ == "__main__":
    print(json.dumps({"queries": queries, "gates": gates}[sys.argv[1]](), separators=(",", ":")))
