"""Prints, as one JSON line, what the size and offset queries of the amortized multivariate guide and the likelihood return
over a fixed set of shapes (tests/test_layout_queries.py).  The queries need no GPU: without one the library plans for the
MI355X's 256 CUs.  The library caches its VX_* switches in statics, so each switch setting runs in a process of its own."""
import ctypes
import json

from vipsy_amd import _hip

QUERIES = ("vx_mvn_pack_floats", "vx_mvn_pack_opmax_offset", "vx_mvn_enc_bwd_workspace_floats", "vx_mvn_enc_bwd_layout",
           "vx_mvn_enc_bwd_gd_offset", "vx_mvn_enc_bwd_hs_offset", "vx_irt_lik_workspace_floats", "vx_irt_lik_ximg_bytes")

NBS = (0, 4, 100, 33024, 70016, 1000000, 1 << 23)


def shapes():
    """(model, D, J, H): every D kind of the dispatch, item counts below, at and beyond the packed layout's LDS budget,
    the padded hidden widths and the links that change the likelihood's kernels."""
    out = []
    for D in (2, 4, 8, 31, 64, 92, 96, 100, 112, 124, 127):
        for J in (30, 500, 2000):
            out.append((2, D, J, 64))
    for D in (8, 64, 100):
        for H in (32, 100):
            out.append((2, D, 500, H))
    for D in (64, 100, 112, 124):
        for model in (3, 4):
            out.append((model, D, 500, 64))
    out.append((2, 100, 1024, 64))
    out.append((2, 100, 501, 64))
    return out


def cases():
    return [(m, D, J, H, nb) for (m, D, J, H) in shapes() for nb in NBS]


def main():
    lib = _hip.lib()
    rows = []
    for (m, D, J, H, nb) in cases():
        cfg = _hip.IrtCfg(m, D, J, H, 1.0, 1.0, 1234, 0, 0)
        row = []
        for q in QUERIES:
            f = getattr(lib, q)
            row.append(int(f(ctypes.byref(cfg))) if q == "vx_mvn_pack_floats" else int(f(ctypes.byref(cfg), nb)))
        rows.append(row)
    print(json.dumps(rows, separators=(",", ":")))


if __name__ == "__main__":
    main()
