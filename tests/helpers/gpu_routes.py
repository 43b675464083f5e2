"""Prints, as one JSON line, the measurement slots (vx_prof_*) that one IrtEngine.loss_and_grads() of the amortized
multivariate guide fills at each batch size of NS: {N: [[name, launches, units], ...]}, sorted by name.  The slots name the
kernels the guide's and the likelihood's dispatch took and the persons of a launch that is not the whole batch, so they pin
the route of a call without timing it (tests/test_gpu_routes.py).  The library reads its VX_* switches once: each switch
setting runs in a process of its own."""
import ctypes
import json

import numpy as np
import torch

from vipsy_amd import _hip
from vipsy_amd.engine import IrtEngine

NS = (512, 33024, 70016)
J, D, H = 500, 100, 64


def slots(N):
    lib = _hip.lib()
    rng = np.random.RandomState(5)
    y = rng.randint(0, 2, size=(N, J)).astype(np.uint8)
    y[rng.rand(N, J) < 0.2] = 255
    eng = IrtEngine(torch.from_numpy(y).cuda(), model="irt_2pl", D=D, amortized=True, H=H, seed=21)
    torch.cuda.synchronize()
    assert lib.vx_prof_enable(1) == 0
    eng.loss_and_grads()
    torch.cuda.synchronize()
    out = []
    for slot in range(lib.vx_prof_count()):
        nm, ms, cnt, un = ctypes.create_string_buffer(64), ctypes.c_float(0), ctypes.c_int(0), ctypes.c_int64(0)
        assert lib.vx_prof_read(slot, nm, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0
        assert lib.vx_prof_units(slot, ctypes.byref(un)) == 0
        out.append([nm.value.decode(), cnt.value, un.value])
    assert lib.vx_prof_enable(0) == 0
    return sorted(out)


if __name__ == "__main__":
    print(json.dumps({str(N): slots(N) for N in NS}, separators=(",", ":")))
