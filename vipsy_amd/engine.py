"""The training-step engine: what `svi.step(data)` does in the reference (vi.py:503-516), driven
through the C ABI (include/vipsy_amd.h).  One process per GPU; persons are sharded by contiguous
ranges, item / encoder parameters are replicated, and the only exchange per step is one all-reduce
(RCCL via torch.distributed) of the flat gradient buffer [item grads | encoder grads | loss].

torch here is plumbing: it owns device buffers and the process group.  All arithmetic of the step
is in the HIP kernels behind vipsy_amd/_hip.py.
"""
import ctypes
import os
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip
from .grid import (EM_MAX_NEWTON, PV_MAX_DRAWS, PV_STREAM, SCORE_MAX_DIMS, SCORE_MAX_NODES, GridCall, GridMixin,  # noqa: F401
                   design_cholesky, em_prior, grid_image_prob, item_fit_stats, population_logw, score_grid, tri_to_full)     # (re-exported: the grid family lives in grid.py)
from .grid import (POINT_AT_BOUND, POINT_CONVERGED, POINT_EMPTY, POINT_MAX_ITER, POINT_MAX_ITERS, POINT_METHODS,  # noqa: F401
                   POINT_SINGULAR, POINT_STATUS, POINT_STEP_CAP, point_estimates_host)
from .grid import bifactor_grid, bifactor_plan, bifactor_slab_persons, bifactor_structure  # noqa: F401
from .grid import (BIFACTOR_EM_NODES, BifactorCall, bifactor_em_index, bifactor_em_prior, bifactor_gather,  # noqa: F401
                   bifactor_scatter)

MODEL_CODE = {"irt_1pl": 1, "irt_2pl": 2, "irt_3pl": 3, "irt_4pl": 4}       # vi.py:538-543
LOSS_RING = 64                                                               # VX_LOSS_RING (include/vipsy_amd.h)
ENC_KEYS = ("fc1.weight", "fc1.bias", "fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias")


def _logit(p):
    return math.log(p) - math.log1p(-p)


class HipBackend(object):
    """Thin call layer over the C ABI.  tests/ substitute an oracle-backed object with the same
    methods to exercise the sharding / all-reduce host logic on CPU (gloo)."""

    name = "hip"

    def __init__(self):
        _hip.require_gpu()
        self.L = _hip.lib()

    # -- helpers -----------------------------------------------------------------------------
    @staticmethod
    def cfg(model, D, J, H, Dc, scale, seed, step, stream, step_dev=None, rows_ring=None):
        """step_dev: the device step counter of a captured step (vx_irt_cfg.step_dev) or None; rows_ring: the pinned
        [slots][stride] int64 host tensor a captured subsampled step takes its row indices from (vx_irt_cfg.rows_ring)."""
        c = _hip.IrtCfg(MODEL_CODE[model], D, J, H, Dc, scale, seed, step, stream,
                        None if step_dev is None else step_dev.data_ptr())
        if rows_ring is not None:
            c.rows_ring, c.rows_ring_stride, c.rows_ring_slots = rows_ring.data_ptr(), rows_ring.shape[1], rows_ring.shape[0]
        return c

    def _size(self, fn, *args):
        """The answer of a size query of the C ABI; a negative one: the configuration is not supported."""
        n = getattr(self.L, fn)(*args)
        if n < 0:
            raise _hip.VxError("%s: unsupported configuration (code %d)" % (fn, n))
        return n

    def mvn_enc_forward(self, cfg, y, rows, nb, gid0, enc, eps_in, out):
        rc = self.L.vx_mvn_enc_forward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, gid0,
                                       _hip.ptr(enc["fc1.weight"]), _hip.ptr(enc["fc1.bias"]),
                                       _hip.ptr(enc["fc21.weight"]), _hip.ptr(enc["fc21.bias"]),
                                       _hip.ptr(enc["fc22.weight"]), _hip.ptr(enc["fc22.bias"]),
                                       _hip.ptr(eps_in), _hip.ptr(out["h"]), _hip.ptr(out["x"]),
                                       _hip.ptr(out["eps"]), _hip.ptr(out["ldT"]), _hip.ptr(out["ent"]),
                                       _hip.ptr(out.get("hT")), _hip.ptr(out.get("epsT")),
                                       _hip.ptr(out.get("packws")), _hip.ptr(out.get("ximg")), _hip.ptr(out.get("hs")),
                                       _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_enc_forward")

    def mvn_pack_floats(self, cfg):
        return self._size("vx_mvn_pack_floats", ctypes.byref(cfg))

    def lik_ximg_bytes(self, cfg, nb):
        return self._size("vx_irt_lik_ximg_bytes", ctypes.byref(cfg), nb)

    def lik_workspace(self, cfg, nb):
        return self._size("vx_irt_lik_workspace_floats", ctypes.byref(cfg), nb)

    def mvn_pack_opmax_offset(self, cfg, nb):
        return int(self.L.vx_mvn_pack_opmax_offset(ctypes.byref(cfg), nb))

    def lik_grad(self, cfg, y, rows, nb, x, a, b, c_un, d_un, gx, ll, gitem, ws, gxT=None, yT=None, ximg=None,
                 epsT=None, ldT=None, gdT=None, opmax=None):
        rc = self.L.vx_irt_lik_grad(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(x), _hip.ptr(a),
                                    _hip.ptr(b), _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(gx), _hip.ptr(gxT),
                                    _hip.ptr(ll), _hip.ptr(gitem), _hip.ptr(ws), _hip.ptr(yT),
                                    int(yT.shape[1]) if yT is not None else 0, _hip.ptr(ximg), _hip.ptr(epsT),
                                    _hip.ptr(ldT), _hip.ptr(gdT), _hip.ptr(opmax), _hip.stream_ptr())
        _hip.check(rc, "vx_irt_lik_grad")

    def mvn_enc_bwd_workspace(self, cfg, nb):
        return self._size("vx_mvn_enc_bwd_workspace_floats", ctypes.byref(cfg), nb)

    def mvn_enc_bwd_layout(self, cfg, nb):
        return int(self.L.vx_mvn_enc_bwd_layout(ctypes.byref(cfg), nb))

    def mvn_enc_bwd_gd_offset(self, cfg, nb):
        return int(self.L.vx_mvn_enc_bwd_gd_offset(ctypes.byref(cfg), nb))

    def mvn_enc_bwd_hs_offset(self, cfg, nb):
        return int(self.L.vx_mvn_enc_bwd_hs_offset(ctypes.byref(cfg), nb))

    def mvn_enc_backward(self, cfg, y, rows, nb, enc, fw, gx, genc, ws, gxT=None, gd_ready=False, opmax_ready=False, loss=None):
        """loss = (ll, ent, alpha, slot, sum_ws): the step's loss from the call's last launch (vx_mvn_enc_backward_loss)."""
        args = [ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb,
                _hip.ptr(enc["fc21.weight"]), _hip.ptr(enc["fc22.weight"]),
                _hip.ptr(fw["h"]), _hip.ptr(fw["eps"]), _hip.ptr(fw["ldT"]), _hip.ptr(gx),
                _hip.ptr(fw.get("hT")), _hip.ptr(fw.get("epsT")), _hip.ptr(gxT),
                _hip.ptr(fw.get("yT")), int(fw["yT"].shape[1]) if fw.get("yT") is not None else 0,
                _hip.ptr(genc), _hip.ptr(ws), _hip.ptr(fw.get("packws")),
                int(bool(gd_ready)) | (2 if fw.get("hs") is not None else 0) | (4 if opmax_ready else 0)]
        if loss is None:
            rc = self.L.vx_mvn_enc_backward(*args, _hip.stream_ptr())
            _hip.check(rc, "vx_mvn_enc_backward")
            return
        ll, ent, alpha, slot, sum_ws = loss
        rc = self.L.vx_mvn_enc_backward_loss(*args, _hip.ptr(ll), _hip.ptr(ent), alpha, _hip.ptr(slot), _hip.ptr(sum_ws),
                                             _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_enc_backward_loss")

    def irt1d_workspace(self, cfg, nb):
        return self._size("vx_irt1d_workspace_floats", ctypes.byref(cfg), nb)

    @staticmethod
    def _adam_tail(adam):
        """struct vx_adam_tail from the engine's description of its optimiser step (IrtEngine._fused_tail_args); the
        segment arrays ride along so that they outlive the call."""
        (pA, mA, vA, freeA, nA, segsA), B = adam["A"], adam.get("B")
        arrA = (_hip.AdamSeg * len(segsA))(*[_hip.AdamSeg(b, e, lr, 0.0) for (b, e, lr) in segsA])
        t = _hip.AdamTail()
        t.pA, t.mA, t.vA, t.freeA, t.nA, t.segsA, t.n_segsA = _hip.ptr(pA), _hip.ptr(mA), _hip.ptr(vA), _hip.ptr(freeA), nA, arrA, len(segsA)
        keep = [arrA]
        if B is not None:
            pB, gB, mB, vB, nB, segsB = B
            arrB = (_hip.AdamSeg * len(segsB))(*[_hip.AdamSeg(b, e, lr, 0.0) for (b, e, lr) in segsB])
            t.pB, t.gB, t.mB, t.vB, t.nB, t.segsB, t.n_segsB = _hip.ptr(pB), _hip.ptr(gB), _hip.ptr(mB), _hip.ptr(vB), nB, arrB, len(segsB)
            keep.append(arrB)
        t.t, (t.beta1, t.beta2), t.eps = adam["t"], adam["betas"], adam["eps"]
        t.loss_ring = _hip.ptr(adam.get("loss_ring"))
        return t, keep

    def irt1d_grad(self, cfg, y, rows, nb, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo, gitem, ws,
                   loss=None, step_dev=None, adam=None):
        args = [ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, gid0, _hip.ptr(loc),
                _hip.ptr(raw), _hip.ptr(eps_in), _hip.ptr(a), _hip.ptr(b), _hip.ptr(c_un),
                _hip.ptr(d_un), _hip.ptr(gloc), _hip.ptr(graw), _hip.ptr(elbo), _hip.ptr(gitem),
                _hip.ptr(loss), _hip.ptr(step_dev), _hip.ptr(ws)]
        if adam is not None:                                 # the optimiser in the step's last launch (vx_irt1d_grad_adam)
            tail, _keep = self._adam_tail(adam)
            rc = self.L.vx_irt1d_grad_adam(*args, ctypes.byref(tail), _hip.stream_ptr())
            _hip.check(rc, "vx_irt1d_grad_adam")
            return
        rc = self.L.vx_irt1d_grad(*args, _hip.stream_ptr())
        _hip.check(rc, "vx_irt1d_grad")

    def irt1d_sparse_workspace(self, cfg, n_groups):
        return self._size("vx_irt1d_sparse_workspace_floats", ctypes.byref(cfg), n_groups)

    def irt1d_sparse_grad(self, cfg, lists, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo, gitem, ws,
                          loss=None, step_dev=None, adam=None):
        args = [ctypes.byref(cfg), _hip.ptr(lists["pent"]), _hip.ptr(lists["glen"]),
                int(lists["Lq"]), _hip.ptr(lists["pidx"]), int(lists["n_groups"]), gid0,
                _hip.ptr(loc), _hip.ptr(raw), _hip.ptr(eps_in), _hip.ptr(a), _hip.ptr(b),
                _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(gloc), _hip.ptr(graw), _hip.ptr(elbo),
                _hip.ptr(gitem), _hip.ptr(loss), _hip.ptr(step_dev), _hip.ptr(ws)]
        if adam is not None:
            tail, _keep = self._adam_tail(adam)
            rc = self.L.vx_irt1d_sparse_grad_adam(*args, ctypes.byref(tail), _hip.stream_ptr())
            _hip.check(rc, "vx_irt1d_sparse_grad_adam")
            return
        rc = self.L.vx_irt1d_sparse_grad(*args, _hip.stream_ptr())
        _hip.check(rc, "vx_irt1d_sparse_grad")

    def mvn_bbvi_forward(self, cfg, nb, rows, gid0, loc, M, shared, eps_in, x, eps, ent):
        rc = self.L.vx_mvn_bbvi_forward(ctypes.byref(cfg), nb, _hip.ptr(rows), gid0, _hip.ptr(loc), _hip.ptr(M),
                                        int(shared), _hip.ptr(eps_in), _hip.ptr(x), _hip.ptr(eps), _hip.ptr(ent),
                                        _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_bbvi_forward")

    def mvn_bbvi_bwd_workspace(self, cfg, nb, shared):
        return max(1, int(self.L.vx_mvn_bbvi_bwd_workspace_floats(ctypes.byref(cfg), nb, int(shared))))

    def mvn_bbvi_backward(self, cfg, nb, rows, M, shared, gx, eps, gloc, gM, ws=None):
        rc = self.L.vx_mvn_bbvi_backward(ctypes.byref(cfg), nb, _hip.ptr(rows), _hip.ptr(M), int(shared), _hip.ptr(gx),
                                         _hip.ptr(eps), _hip.ptr(gloc), _hip.ptr(gM), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_bbvi_backward")

    def norm_enc_forward(self, cfg, y, rows, nb, enc, out):
        rc = self.L.vx_norm_enc_forward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb,
                                        _hip.ptr(enc["fc1.weight"]), _hip.ptr(enc["fc1.bias"]),
                                        _hip.ptr(enc["fc21.weight"]), _hip.ptr(enc["fc21.bias"]),
                                        _hip.ptr(enc["fc22.weight"]), _hip.ptr(enc["fc22.bias"]),
                                        _hip.ptr(out["h"]), _hip.ptr(out["loc"]), _hip.ptr(out["raw"]),
                                        _hip.ptr(out.get("packws")), _hip.stream_ptr())
        _hip.check(rc, "vx_norm_enc_forward")

    def norm_enc_pack_floats(self, cfg):
        return self._size("vx_norm_enc_pack_floats", ctypes.byref(cfg))

    def norm_enc_bwd_workspace(self, cfg, nb):
        return self._size("vx_norm_enc_bwd_workspace_floats", ctypes.byref(cfg), nb)

    def norm_enc_backward(self, cfg, y, rows, nb, enc, h, gloc, graw, genc, ws, yT=None):
        rc = self.L.vx_norm_enc_backward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb,
                                         _hip.ptr(enc["fc21.weight"]), _hip.ptr(enc["fc22.weight"]), _hip.ptr(h),
                                         _hip.ptr(gloc), _hip.ptr(graw), _hip.ptr(yT),
                                         int(yT.shape[1]) if yT is not None else 0, _hip.ptr(genc), _hip.ptr(ws),
                                         _hip.stream_ptr())
        _hip.check(rc, "vx_norm_enc_backward")

    @staticmethod
    def hodina_cfg(K, J, H, scale, seed, step, stream, step_dev=None):
        return _hip.HoDinaCfg(K, J, H, 0, scale, 0.0, seed, step, stream, None if step_dev is None else step_dev.data_ptr())

    def hodina_workspace(self, cfg, nb):
        return self._size("vx_hodina_workspace_floats", ctypes.byref(cfg), nb)

    def hodina_grad(self, cfg, y, rows, nb, gid0, loc, raw, eps_in, q, lam0, lam1, g, s_, gloc, graw, elbo, gitem, ws):
        rc = self.L.vx_hodina_grad(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, gid0, _hip.ptr(loc),
                                   _hip.ptr(raw), _hip.ptr(eps_in), _hip.ptr(q), _hip.ptr(lam0), _hip.ptr(lam1),
                                   _hip.ptr(g), _hip.ptr(s_), _hip.ptr(gloc), _hip.ptr(graw), _hip.ptr(elbo),
                                   _hip.ptr(gitem), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_hodina_grad")

    def ccdm_workspace(self, cfg, nb):
        return self._size("vx_ccdm_workspace_floats", ctypes.byref(cfg), nb)

    def ccdm_grad(self, cfg, dino, y, rows, nb, q, g, s_, elbo, gitem, ws):
        rc = self.L.vx_ccdm_grad(ctypes.byref(cfg), int(dino), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(q), _hip.ptr(g),
                                 _hip.ptr(s_), _hip.ptr(elbo), _hip.ptr(gitem), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_ccdm_grad")

    def grid_image_bytes(self, J, G):
        return self._size("vx_grid_image_bytes", J, G)

    def grid_table_irt(self, cfg, theta, G, a, b, c_un, d_un, img):
        rc = self.L.vx_grid_table_irt(ctypes.byref(cfg), _hip.ptr(theta), G, _hip.ptr(a), _hip.ptr(b), _hip.ptr(c_un),
                                      _hip.ptr(d_un), _hip.ptr(img), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_table_irt")

    def grid_table_cdm(self, cfg, dino, q, g, s_, img):
        rc = self.L.vx_grid_table_cdm(ctypes.byref(cfg), int(dino), _hip.ptr(q), _hip.ptr(g), _hip.ptr(s_), _hip.ptr(img),
                                      _hip.stream_ptr())
        _hip.check(rc, "vx_grid_table_cdm")

    def grid_counts_workspace(self, nb, J, G):
        return self._size("vx_grid_counts_workspace_floats", nb, J, G)

    def grid_counts(self, y, rows, nb, J, G, img, logw, loglik, n1, n0, mass, ws):
        rc = self.L.vx_grid_counts(_hip.ptr(y), _hip.ptr(rows), nb, J, G, _hip.ptr(img), _hip.ptr(logw), _hip.ptr(loglik),
                                   _hip.ptr(n1), _hip.ptr(n0), _hip.ptr(mass), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_counts")

    def grid_counts_cond_workspace(self, nb, n_seg, J, G):
        return self._size("vx_grid_counts_cond_workspace_floats", nb, n_seg, J, G)

    def grid_counts_cond(self, y, rows, nb, J, G, D, img, logw, coord, tilt, logjoint, seg_start, n1, n0, mass, ws):
        """seg_start: int64 numpy [n_seg + 1] on the HOST (the entry checks it and plans the launch from it)."""
        seg = np.ascontiguousarray(seg_start, dtype=np.int64)
        rc = self.L.vx_grid_counts_cond(_hip.ptr(y), _hip.ptr(rows), nb, J, G, D, _hip.ptr(img), _hip.ptr(logw), _hip.ptr(coord),
                                        _hip.ptr(tilt), _hip.ptr(logjoint), seg.ctypes.data_as(ctypes.c_void_p), int(seg.size) - 1,
                                        _hip.ptr(n1), _hip.ptr(n0), _hip.ptr(mass), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_counts_cond")

    def grid_mstep_irt(self, cfg, theta, G, n1, n0, a_free, a, b, newton):
        rc = self.L.vx_grid_mstep_irt(ctypes.byref(cfg), _hip.ptr(theta), G, _hip.ptr(n1), _hip.ptr(n0), _hip.ptr(a_free),
                                      _hip.ptr(a), _hip.ptr(b), int(newton), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_mstep_irt")

    def grid_mstep_irt_map(self, cfg, theta, G, n1, n0, a_free, a, b, c_un, d_un, prior, newton, lprior=None):
        rc = self.L.vx_grid_mstep_irt_map(ctypes.byref(cfg), _hip.ptr(theta), G, _hip.ptr(n1), _hip.ptr(n0), _hip.ptr(a_free),
                                          _hip.ptr(a), _hip.ptr(b), _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(prior), newton,
                                          _hip.ptr(lprior), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_mstep_irt_map")

    def grid_mstep_cdm(self, cfg, dino, q, n1, n0, g, s_):
        rc = self.L.vx_grid_mstep_cdm(ctypes.byref(cfg), int(dino), _hip.ptr(q), _hip.ptr(n1), _hip.ptr(n0), _hip.ptr(g),
                                      _hip.ptr(s_), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_mstep_cdm")

    def grid_posterior(self, y, rows, nb, J, G, D, img, logw, coord, loglik, mean, sd, argmax):
        rc = self.L.vx_grid_posterior(_hip.ptr(y), _hip.ptr(rows), nb, J, G, D, _hip.ptr(img), _hip.ptr(logw), _hip.ptr(coord),
                                      _hip.ptr(loglik), _hip.ptr(mean), _hip.ptr(sd), _hip.ptr(argmax), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_posterior")

    def grid_bifactor_image_bytes(self, Gg, KC):
        return self._size("vx_grid_bifactor_image_bytes", Gg, KC)

    def grid_bifactor_workspace(self, nb, Gg):
        return self._size("vx_grid_bifactor_workspace_floats", nb, Gg)

    def grid_table_bifactor(self, cfg, theta, u, general, col, sdim, KC, a, b, c_un, d_un, img):
        rc = self.L.vx_grid_table_bifactor(ctypes.byref(cfg), _hip.ptr(theta), int(theta.numel()), _hip.ptr(u), int(u.numel()),
                                           int(general), _hip.ptr(col), _hip.ptr(sdim), int(KC), _hip.ptr(a), _hip.ptr(b),
                                           _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(img), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_table_bifactor")

    @staticmethod
    def _tl_start(tl_start):
        """tl_start as the entries read it on the HOST: contiguous int32 numpy, and the pointer to it."""
        tl = np.ascontiguousarray(tl_start, dtype=np.int32)
        return tl, tl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def grid_bifactor(self, y, nb, KC, tl_start, tl_start_dev, img, logw, coord, logv, u, loglik, mean, sd, argmax, fws):
        """tl_start: int32 numpy [n_tl + 1] on the HOST (the entry checks it); tl_start_dev: the same on the device."""
        tl, tlp = self._tl_start(tl_start)
        rc = self.L.vx_grid_bifactor(_hip.ptr(y), nb, int(KC), int(logw.numel()), int(logv.numel()), tlp, int(tl.size) - 1,
                                     _hip.ptr(tl_start_dev), _hip.ptr(img), _hip.ptr(logw), _hip.ptr(coord), _hip.ptr(logv),
                                     _hip.ptr(u), _hip.ptr(loglik), _hip.ptr(mean), _hip.ptr(sd), _hip.ptr(argmax), _hip.ptr(fws),
                                     _hip.stream_ptr())
        _hip.check(rc, "vx_grid_bifactor")

    def grid_bifactor_specific(self, y, nb, KC, Gg, tl_start, tl_start_dev, img, logv, u, loglik, fws, mean_s, sd_s):
        tl, tlp = self._tl_start(tl_start)
        rc = self.L.vx_grid_bifactor_specific(_hip.ptr(y), nb, int(KC), int(Gg), int(logv.numel()), tlp, int(tl.size) - 1,
                                              _hip.ptr(tl_start_dev), _hip.ptr(img), _hip.ptr(logv), _hip.ptr(u), _hip.ptr(loglik),
                                              _hip.ptr(fws), _hip.ptr(mean_s), _hip.ptr(sd_s), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_bifactor_specific")

    def grid_bifactor_counts_workspace(self, nb, KC, Gg, n_tl):
        return self._size("vx_grid_bifactor_counts_workspace_floats", nb, KC, Gg, n_tl)

    def grid_bifactor_counts(self, y, nb, KC, Gg, tl_start, tl_start_dev, col, J, img, logv, loglik, fws, accumulate, n1, n0, mass,
                             mass_s, ws):
        """n1, n0 [J][Gg Gh], mass [Gg], mass_s [n_tl][Gg Gh] or None; accumulate: add to what the tables hold."""
        tl, tlp = self._tl_start(tl_start)
        rc = self.L.vx_grid_bifactor_counts(_hip.ptr(y), nb, int(KC), int(Gg), int(logv.numel()), tlp, int(tl.size) - 1,
                                            _hip.ptr(tl_start_dev), _hip.ptr(col), int(J), _hip.ptr(img), _hip.ptr(logv),
                                            _hip.ptr(loglik), _hip.ptr(fws), 1 if accumulate else 0, _hip.ptr(n1), _hip.ptr(n0),
                                            _hip.ptr(mass), _hip.ptr(mass_s), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_bifactor_counts")

    def grid_draw(self, y, rows, nb, J, G, img, logw, seed, row_offset, draw0, ndraws, stride, node):
        rc = self.L.vx_grid_draw(_hip.ptr(y), _hip.ptr(rows), nb, J, G, _hip.ptr(img), _hip.ptr(logw), int(seed), int(row_offset),
                                 int(draw0), int(ndraws), int(stride), _hip.ptr(node), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_draw")

    def grid_posterior_cond(self, y, rows, nb, J, G, D, img, logw, coord, tilt, logjoint, lognorm, mean, cov, argmax):
        rc = self.L.vx_grid_posterior_cond(_hip.ptr(y), _hip.ptr(rows), nb, J, G, D, _hip.ptr(img), _hip.ptr(logw), _hip.ptr(coord),
                                           _hip.ptr(tilt), _hip.ptr(logjoint), _hip.ptr(lognorm), _hip.ptr(mean), _hip.ptr(cov),
                                           _hip.ptr(argmax), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_posterior_cond")

    def grid_draw_cond(self, y, rows, nb, J, G, D, img, logw, coord, tilt, seed, row_offset, draw0, ndraws, stride, node):
        rc = self.L.vx_grid_draw_cond(_hip.ptr(y), _hip.ptr(rows), nb, J, G, D, _hip.ptr(img), _hip.ptr(logw), _hip.ptr(coord),
                                      _hip.ptr(tilt), int(seed), int(row_offset), int(draw0), int(ndraws), int(stride),
                                      _hip.ptr(node), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_draw_cond")

    def grid_wimage_bytes(self, P, G):
        return self._size("vx_grid_wimage_bytes", P, G)

    def grid_wtable_irt(self, cfg, theta, G, a, b, wimg):
        rc = self.L.vx_grid_wtable_irt(ctypes.byref(cfg), _hip.ptr(theta), G, _hip.ptr(a), _hip.ptr(b), _hip.ptr(wimg),
                                       _hip.stream_ptr())
        _hip.check(rc, "vx_grid_wtable_irt")

    def grid_wtable_irt_map(self, cfg, theta, G, a, b, c_un, d_un, wimg):
        rc = self.L.vx_grid_wtable_irt_map(ctypes.byref(cfg), _hip.ptr(theta), G, _hip.ptr(a), _hip.ptr(b), _hip.ptr(c_un),
                                           _hip.ptr(d_un), _hip.ptr(wimg), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_wtable_irt_map")

    def grid_wtable_cdm(self, cfg, dino, q, g, s_, wimg):
        rc = self.L.vx_grid_wtable_cdm(ctypes.byref(cfg), int(dino), _hip.ptr(q), _hip.ptr(g), _hip.ptr(s_), _hip.ptr(wimg),
                                       _hip.stream_ptr())
        _hip.check(rc, "vx_grid_wtable_cdm")

    def grid_info_workspace(self, nb, P, G):
        return self._size("vx_grid_info_workspace_floats", nb, P, G)

    def grid_info_workspace_min(self, P, G):
        return self._size("vx_grid_info_workspace_min_floats", P, G)

    def grid_info(self, y, rows, nb, J, G, K, img, wimg, logw, loglik, info, gradient, ws, ws_floats):
        rc = self.L.vx_grid_info(_hip.ptr(y), _hip.ptr(rows), nb, J, G, K, _hip.ptr(img), _hip.ptr(wimg), _hip.ptr(logw),
                                 _hip.ptr(loglik), _hip.ptr(info), _hip.ptr(gradient), _hip.ptr(ws), int(ws_floats),
                                 _hip.stream_ptr())
        _hip.check(rc, "vx_grid_info")

    def grid_pairs_workspace(self, nb, J):
        return self._size("vx_grid_pairs_workspace_floats", nb, J)

    def grid_pairs_workspace_min(self, J):
        return self._size("vx_grid_pairs_workspace_min_floats", J)

    def grid_pairs_irt(self, cfg, y, rows, nb, theta_hat, a, b, c_un, d_un, n, s, ss, sp, ws, ws_floats):
        rc = self.L.vx_grid_pairs_irt(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(theta_hat), _hip.ptr(a), _hip.ptr(b),
                                      _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(n), _hip.ptr(s), _hip.ptr(ss), _hip.ptr(sp),
                                      _hip.ptr(ws), int(ws_floats), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_pairs_irt")

    def grid_pairs_cdm(self, cfg, dino, q, y, rows, nb, pattern, g, s_, n, s, ss, sp, ws, ws_floats):
        rc = self.L.vx_grid_pairs_cdm(ctypes.byref(cfg), int(dino), _hip.ptr(q), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(pattern),
                                      _hip.ptr(g), _hip.ptr(s_), _hip.ptr(n), _hip.ptr(s), _hip.ptr(ss), _hip.ptr(sp), _hip.ptr(ws),
                                      int(ws_floats), _hip.stream_ptr())
        _hip.check(rc, "vx_grid_pairs_cdm")

    def grid_fit_workspace(self, nb, J):
        return self._size("vx_grid_fit_workspace_floats", nb, J)

    def grid_fit_irt(self, cfg, y, rows, nb, theta_hat, a, b, c_un, d_un, person, item, ws, ws_floats):
        rc = self.L.vx_grid_fit_irt(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(theta_hat), _hip.ptr(a), _hip.ptr(b),
                                    _hip.ptr(c_un), _hip.ptr(d_un), _hip.ptr(person), _hip.ptr(item), _hip.ptr(ws), int(ws_floats),
                                    _hip.stream_ptr())
        _hip.check(rc, "vx_grid_fit_irt")

    def grid_point_irt(self, cfg, y, rows, nb, theta0, a, b, c_un, d_un, method, max_iter, tol, bound, step_cap, theta_hat, info,
                       status, iters):
        rc = self.L.vx_grid_point_irt(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(theta0), _hip.ptr(a), _hip.ptr(b),
                                      _hip.ptr(c_un), _hip.ptr(d_un), int(method), int(max_iter), float(tol), float(bound),
                                      float(step_cap), _hip.ptr(theta_hat), _hip.ptr(info), _hip.ptr(status), _hip.ptr(iters),
                                      _hip.stream_ptr())
        _hip.check(rc, "vx_grid_point_irt")

    def grid_fit_cdm(self, cfg, dino, q, y, rows, nb, pattern, g, s_, person, item, ws, ws_floats):
        rc = self.L.vx_grid_fit_cdm(ctypes.byref(cfg), int(dino), _hip.ptr(q), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(pattern),
                                    _hip.ptr(g), _hip.ptr(s_), _hip.ptr(person), _hip.ptr(item), _hip.ptr(ws), int(ws_floats),
                                    _hip.stream_ptr())
        _hip.check(rc, "vx_grid_fit_cdm")

    def sumscore_model_workspace(self, Js, G):
        return self._size("vx_sumscore_model_workspace_floats", Js, G)

    def sumscore_model(self, p1, p0, logw, Js, G, e1, e0, dist, ws, ws_floats):
        rc = self.L.vx_sumscore_model(_hip.ptr(p1), _hip.ptr(p0), _hip.ptr(logw), Js, G, _hip.ptr(e1), _hip.ptr(e0), _hip.ptr(dist),
                                      _hip.ptr(ws), int(ws_floats), _hip.stream_ptr())
        _hip.check(rc, "vx_sumscore_model")

    def sumscore_persons(self, y, rows, nb, J, items, Js, score):
        rc = self.L.vx_sumscore_persons(_hip.ptr(y), _hip.ptr(rows), nb, J, _hip.ptr(items), Js, _hip.ptr(score), _hip.stream_ptr())
        _hip.check(rc, "vx_sumscore_persons")

    def sumscore_observed(self, y, rows, nb, J, items, Js, score, o1):
        rc = self.L.vx_sumscore_observed(_hip.ptr(y), _hip.ptr(rows), nb, J, _hip.ptr(items), Js, _hip.ptr(score), _hip.ptr(o1),
                                         _hip.stream_ptr())
        _hip.check(rc, "vx_sumscore_observed")

    def pair_tables_workspace(self, nb, J):
        return self._size("vx_pair_tables_workspace_ints", nb, J)

    def pair_tables_chunks(self, nb, J):
        return self._size("vx_pair_tables_chunks", nb, J)

    def pair_tables(self, y, rows, nb, J, n11, n10, n01, n00, ws, ws_ints):
        rc = self.L.vx_pair_tables(_hip.ptr(y), _hip.ptr(rows), nb, J, _hip.ptr(n11), _hip.ptr(n10), _hip.ptr(n01), _hip.ptr(n00),
                                   _hip.ptr(ws), int(ws_ints), _hip.stream_ptr())
        _hip.check(rc, "vx_pair_tables")

    def cdm_sf_workspace(self, cfg, nb):
        return self._size("vx_cdm_sf_workspace_floats", ctypes.byref(cfg), nb)

    def cdm_sf_grad(self, cfg, dino, clamp_t, prior_p, y, rows, nb, gid0, q, g, s_, u, attr_in, baseline, base_beta,
                    base_by_row, gu, log_r, attr_out, gitem, ws):
        rc = self.L.vx_cdm_sf_grad(ctypes.byref(cfg), int(dino), int(clamp_t), float(prior_p), _hip.ptr(y), _hip.ptr(rows), nb,
                                   gid0, _hip.ptr(q), _hip.ptr(g), _hip.ptr(s_), _hip.ptr(u), _hip.ptr(attr_in),
                                   _hip.ptr(baseline), float(base_beta), int(base_by_row), _hip.ptr(gu), _hip.ptr(log_r),
                                   _hip.ptr(attr_out), _hip.ptr(gitem), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_cdm_sf_grad")

    def irt1d_score_grad(self, nb, scale, elbo, eps, raw, rows, baseline, base_beta, base_by_row, log_r, gloc, graw):
        rc = self.L.vx_irt1d_score_grad(nb, float(scale), _hip.ptr(elbo), _hip.ptr(eps), _hip.ptr(raw), _hip.ptr(rows),
                                        _hip.ptr(baseline), float(base_beta), int(base_by_row), _hip.ptr(log_r),
                                        _hip.ptr(gloc), _hip.ptr(graw), _hip.stream_ptr())
        _hip.check(rc, "vx_irt1d_score_grad")

    def mvn_score_operands(self, cfg, nb, rows, kind, h, W22, b22, M, eps, ll, ent, baseline, base_beta, base_by_row, log_r, w,
                           gx, gxT, gdT):
        rc = self.L.vx_mvn_score_operands(ctypes.byref(cfg), nb, _hip.ptr(rows), int(kind), _hip.ptr(h), _hip.ptr(W22),
                                          _hip.ptr(b22), _hip.ptr(M), _hip.ptr(eps), _hip.ptr(ll), _hip.ptr(ent),
                                          _hip.ptr(baseline), float(base_beta), int(base_by_row), _hip.ptr(log_r), _hip.ptr(w),
                                          _hip.ptr(gx), _hip.ptr(gxT), _hip.ptr(gdT), _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_score_operands")

    def mvn_score_heads_workspace(self, cfg):
        """floats of the column image of the MFMA score kernel, or -1 when the shape is not its own"""
        return int(self.L.vx_mvn_score_heads_workspace_floats(ctypes.byref(cfg)))

    def mvn_score_heads(self, cfg, nb, rows, h, W22, b22, packws, eps, ll, ent, baseline, base_beta, base_by_row, log_r,
                        gxT, gdT, ws):
        rc = self.L.vx_mvn_score_heads(ctypes.byref(cfg), nb, _hip.ptr(rows), _hip.ptr(h), _hip.ptr(W22), _hip.ptr(b22),
                                       _hip.ptr(packws), _hip.ptr(eps), _hip.ptr(ll), _hip.ptr(ent),
                                       _hip.ptr(baseline), float(base_beta), int(base_by_row), _hip.ptr(log_r), _hip.ptr(gxT),
                                       _hip.ptr(gdT), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_mvn_score_heads")

    def mvn_score_diag(self, cfg, nb, rows, w, shared, gM):
        _hip.check(self.L.vx_mvn_score_diag(ctypes.byref(cfg), nb, _hip.ptr(rows), _hip.ptr(w), int(bool(shared)), _hip.ptr(gM),
                                            _hip.stream_ptr()), "vx_mvn_score_diag")

    def loo_baseline(self, lr_all, S, nb, s, out):
        _hip.check(self.L.vx_loo_baseline(_hip.ptr(lr_all), int(S), nb, int(s), _hip.ptr(out), _hip.stream_ptr()),
                   "vx_loo_baseline")

    def bin_enc_forward(self, cfg, y, rows, nb, enc, h, u):
        rc = self.L.vx_bin_enc_forward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(enc["fc1.weight"]),
                                       _hip.ptr(enc["fc1.bias"]), _hip.ptr(enc["fc2.weight"]), _hip.ptr(enc["fc2.bias"]),
                                       _hip.ptr(h), _hip.ptr(u), _hip.stream_ptr())
        _hip.check(rc, "vx_bin_enc_forward")

    def bin_enc_bwd_workspace(self, cfg, nb):
        return self._size("vx_bin_enc_bwd_workspace_floats", ctypes.byref(cfg), nb)

    def bin_enc_backward(self, cfg, y, rows, nb, enc, h, gu, genc, ws):
        rc = self.L.vx_bin_enc_backward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(enc["fc2.weight"]),
                                        _hip.ptr(h), _hip.ptr(gu), _hip.ptr(genc), _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_bin_enc_backward")

    def sm_enc_forward(self, cfg, y, rows, nb, enc, h, z):
        rc = self.L.vx_sm_enc_forward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(enc["fc1.weight"]),
                                      _hip.ptr(enc["fc1.bias"]), _hip.ptr(enc["fc2.weight"]), _hip.ptr(enc["fc2.bias"]),
                                      _hip.ptr(h), _hip.ptr(z), _hip.stream_ptr())
        _hip.check(rc, "vx_sm_enc_forward")

    def col_reduce(self, mode, v, nb, C, shift, out, ws):
        _hip.check(self.L.vx_col_reduce(int(mode), _hip.ptr(v), nb, int(C), _hip.ptr(shift), _hip.ptr(out), _hip.ptr(ws),
                                        _hip.stream_ptr()), "vx_col_reduce")

    def col_reduce_workspace(self, nb, C):
        return int(self.L.vx_col_reduce_workspace_floats(nb, int(C)))

    def vaeccdm_workspace(self, cfg, nb):
        return self._size("vx_vaeccdm_workspace_floats", ctypes.byref(cfg), nb)

    def vaeccdm_grad(self, cfg, dino, y, rows, nb, q, g, s_, z, off, elbo, gla, gitem, ws):
        rc = self.L.vx_vaeccdm_grad(ctypes.byref(cfg), int(dino), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(q), _hip.ptr(g),
                                    _hip.ptr(s_), _hip.ptr(z), _hip.ptr(off), _hip.ptr(elbo), _hip.ptr(gla), _hip.ptr(gitem),
                                    _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_vaeccdm_grad")

    def sm_enc_bwd_workspace(self, cfg, nb):
        return self._size("vx_sm_enc_bwd_workspace_floats", ctypes.byref(cfg), nb)

    def sm_enc_backward(self, cfg, y, rows, nb, enc, h, z, off, T, gla, genc, ws):
        rc = self.L.vx_sm_enc_backward(ctypes.byref(cfg), _hip.ptr(y), _hip.ptr(rows), nb, _hip.ptr(enc["fc2.weight"]),
                                       _hip.ptr(h), _hip.ptr(z), _hip.ptr(off), _hip.ptr(T), _hip.ptr(gla), _hip.ptr(genc),
                                       _hip.ptr(ws), _hip.stream_ptr())
        _hip.check(rc, "vx_sm_enc_backward")

    def sum_into(self, v, n, alpha, out, ws, step_dev=None):
        rc = self.L.vx_sum(_hip.ptr(v), n, alpha, _hip.ptr(out), _hip.ptr(ws), _hip.ptr(step_dev), _hip.stream_ptr())
        _hip.check(rc, "vx_sum")

    def adam2(self, bufA, free, nA, segsA, bufB, nB, segsB, t, betas=(0.9, 0.999), eps=1e-8, t_dev=None, loss=None):
        arrA = (_hip.AdamSeg * len(segsA))(*[_hip.AdamSeg(b, e, lr, 0.0) for (b, e, lr) in segsA])
        arrB = (_hip.AdamSeg * len(segsB))(*[_hip.AdamSeg(b, e, lr, 0.0) for (b, e, lr) in segsB])
        src, ring = loss if loss is not None else (None, None)
        rc = self.L.vx_adam_step2(*[_hip.ptr(x) for x in bufA], _hip.ptr(free), nA, arrA, len(segsA),
                                  *[_hip.ptr(x) for x in bufB], nB, arrB, len(segsB), t, _hip.ptr(t_dev), betas[0], betas[1],
                                  eps, _hip.ptr(src), _hip.ptr(ring), _hip.stream_ptr())
        _hip.check(rc, "vx_adam_step2")

    def sum2_into(self, v1, v2, n, alpha, out, ws, step_dev=None):
        rc = self.L.vx_sum2(_hip.ptr(v1), _hip.ptr(v2), n, alpha, _hip.ptr(out), _hip.ptr(ws), _hip.ptr(step_dev),
                            _hip.stream_ptr())
        _hip.check(rc, "vx_sum2")

    def adam(self, p, g, m, v, free, n, segs, t, betas=(0.9, 0.999), eps=1e-8, t_dev=None, loss=None):
        arr = (_hip.AdamSeg * len(segs))(*[_hip.AdamSeg(b, e, lr, 0.0) for (b, e, lr) in segs])
        src, ring = loss if loss is not None else (None, None)
        rc = self.L.vx_adam_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), _hip.ptr(free), n, arr,
                                 len(segs), t, _hip.ptr(t_dev), betas[0], betas[1], eps, _hip.ptr(src), _hip.ptr(ring),
                                 _hip.stream_ptr())
        _hip.check(rc, "vx_adam_step")

    def philox_normals(self, out, gids, gid0, n, D, seed, step, stream):
        rc = self.L.vx_philox_normals(_hip.ptr(out), _hip.ptr(gids), gid0, n, D, seed, step, stream,
                                      _hip.stream_ptr())
        _hip.check(rc, "vx_philox_normals")


_ADAM_NOOP = {"weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
              "differentiable": False, "fused": None}


class LrSpec(object):
    """Per-tensor learning rates + MultiStepLR, as pyro.optim.Adam / PyroLRScheduler give them
    (vi.py:514, 639-640; test.py:321-327, 345-359)."""

    def __init__(self, lr, milestones=(), gamma=0.1, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.milestones, self.gamma, self.betas, self.eps = lr, tuple(milestones), gamma, betas, eps
        self.epoch = 0

    def args_of(self, name):
        """The torch.optim.Adam kwargs of one tensor: `lr` may be a float, a dict, or pyro's
        callable(module_name, param_name) -> dict; betas / eps ride in the same dict (torch defaults otherwise)."""
        if callable(self.lr):
            module = name.split("$$$")[0]
            stripped = name.split("$$$")[1] if "$$$" in name else name
            d = dict(self.lr(module, stripped))
        elif isinstance(self.lr, dict):
            d = dict(self.lr)
        else:
            d = {"lr": self.lr}
        for k, noop in _ADAM_NOOP.items():                 # torch.optim.Adam defaults spelled out change nothing
            if k in d and (d[k] is None if noop is None else d[k] == noop):
                del d[k]
        unknown = set(d) - {"lr", "betas", "eps"}
        if unknown:
            raise NotImplementedError("Adam option(s) %s are not on the HIP path" % sorted(unknown))
        return d

    def lr_of(self, name):
        base = self.args_of(name)["lr"]
        k = sum(1 for m in self.milestones if m <= self.epoch)
        return base * self.gamma ** k

    def hyper_of(self, name):
        d = self.args_of(name)
        b = d.get("betas", self.betas)
        return (float(b[0]), float(b[1])), float(d.get("eps", self.eps))

    def scheduler_step(self):
        self.epoch += 1


class _EngineBase(object):
    """State and optimiser plumbing shared by the IRT and HO-DINA engines.

    Replicated parameters live in ONE flat float32 buffer `P` (subclasses define the segments in
    `self.off` / `self.shape`); the gradient buffer `G` has one extra trailing slot for the loss so a
    single all-reduce carries everything.  Per-person variational rows (BBVI
    guides) live in `PP` = [loc: n | raw: n], sharded with the persons, never reduced across ranks."""

    pp_names = ("x_local", "x_scale")

    def _preamble(self, y_u8, backend, n_global, gid0, seed, group):
        """What every constructor starts with: the backend, this rank's shard of the responses and where it sits among the
        n_global persons."""
        self.be = backend if backend is not None else HipBackend()
        self._hip = isinstance(self.be, HipBackend)     # asked once: the CPU rehearsal backends of tests/ take narrower calls
        self.y = y_u8.contiguous()
        assert self.y.dtype == torch.uint8 and self.y.dim() == 2
        self.dev = self.y.device
        self.n_local, self.J = self.y.shape
        self.y_lik = None                    # the copy the likelihood reads when it is not self.y (IrtEngine._decide_shapes)
        self.N = int(n_global) if n_global is not None else self.n_local
        self.gid0 = int(gid0)
        self.seed, self.group = int(seed), group

    def _q_matrix(self, q, why="the subset tests of vi.py:78-81, 96-100 assume it"):
        q = torch.as_tensor(q, dtype=torch.float32)
        assert q.dim() == 2 and q.shape[1] == self.J
        if not bool(((q == 0) | (q == 1)).all()):
            raise ValueError("the Q-matrix must be binary (%s)" % why)
        self.K = int(q.shape[0])
        self.q = q.to(self.dev).contiguous()

    def _encoder_segments(self, shapes):
        """The encoder's tensors (`shapes`, in nn.Linear order) behind the item parameters, from a 256-byte boundary on;
        returns the end of the flat buffer."""
        o = (self.n_item + 63) // 64 * 64
        self.enc_shapes, self.enc_off0 = shapes, o
        for k, shp in shapes.items():
            self.off["encoder$$$" + k] = o
            self.shape["encoder$$$" + k] = shp
            o += int(np.prod(shp))
        self.n_enc = o - self.enc_off0
        return o

    def _fill_encoder(self, init, J, H):
        """The encoder's initial values `init`, given over J items and H hidden units, into segments that may be larger: zeros
        behind them in every tensor -- phantom items are zero columns of fc1.weight, phantom hidden units zero rows of fc1 and
        zero columns of the heads, phantom dimensions zero rows of the heads."""
        for k, full in self.enc_shapes.items():
            w = torch.as_tensor(init[k], dtype=torch.float32)
            w = w.reshape((H, J) if k == "fc1.weight" else (-1, H) if k.endswith("weight") else (-1,))
            self.view("encoder$$$" + k).copy_(_grown(w, full).reshape(-1))

    def _init_g_s(self):
        """g = s = 0.1 through the interval(0, 1) transform (vi.py:748-749, 844-845, 875-876, 901-904)."""
        for nme in ("g", "s"):
            self.view(nme).fill_(float(np.float32(_logit(np.float32(0.1)))))

    def _alloc(self, n_params, n_local, per_person):
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.n_params = n_params
        self.P = torch.zeros(n_params, **f32)
        self.G = torch.zeros(n_params + 1, **f32)
        self.M = torch.zeros(n_params, **f32)
        self.V = torch.zeros(n_params, **f32)
        self.free = torch.ones(n_params, **f32)
        self.per_person = per_person
        if per_person:
            if not hasattr(self, "pp_shape"):
                self.pp_shape = {self.pp_names[0]: (n_local, 1), self.pp_names[1]: (n_local, 1)}
            self.pp_off, o = {}, 0
            for nme in self.pp_names:
                if nme in self.pp_shape:
                    self.pp_off[nme] = o
                    o += int(np.prod(self.pp_shape[nme]))
            self.pp_len = o
            self.PP = torch.zeros(self.pp_len, **f32)
            self.GP = torch.zeros(self.pp_len, **f32)
            self.MP = torch.zeros(self.pp_len, **f32)
            self.VP = torch.zeros(self.pp_len, **f32)
        self._ws = {}
        # the losses of the last LOSS_RING steps: what step() returns is slot t % LOSS_RING, written by the optimiser launch
        self.loss_ring = torch.zeros(LOSS_RING, **f32)
        self.sum_ws = torch.empty(1024, **f32)
        self.last = {}
        self.events = None               # bench.py: list collecting (phase, start_event, end_event)
        self.t = 0                       # optimiser step counter (Adam bias correction, Philox step)
        self._step_dev = None            # while a capture records: the device step counter the kernels read
        self._capture_ring = None        # ... and the pinned rows ring a captured subsampled step may fetch its draw from
        self._fused_tail = None          # the optimiser step armed for the step kernel's last launch (_grads_and_optim)
        self._graphs, self._graph = {}, None                 # captured forms (_step_graph), the one last replayed
        self._ctr = self._pin_ring = None
        self._n_pad = n_local            # persons the full-batch kernels are launched over (phantoms: IrtEngine._pad_persons)
        self._yT = self._y_pad = self._y_pad_lik = None      # copies of the responses made on first use

    def _enc(self):
        return {k: self.view("encoder$$$" + k) for k in self.enc_shapes}

    def all_names(self):
        return self.names() + (list(self.pp_off) if self.per_person else [])

    def _call(self, rows, b_global):
        """(persons of this call, plate scale N / global batch, the step_dev argument of a captured step's calls)."""
        nb = self.n_local if rows is None else int(rows.numel())
        Bg = int(b_global) if b_global is not None else (self.N if rows is None else nb)
        return nb, float(self.N) / float(Bg), ({"step_dev": self._step_dev} if self._step_dev is not None else {})

    def view(self, name, buf=None):
        buf = self.P if buf is None else buf
        o = self.off[name]
        return buf[o:o + int(np.prod(self.shape[name]))]

    def unconstrained(self, name, buf=None):
        if self.per_person and name in self.pp_off:
            b = self.PP if buf is None else buf
            o = self.pp_off[name]
            return b[o:o + int(np.prod(self.pp_shape[name]))].reshape(self.pp_shape[name])
        return self.view(name, buf).reshape(self.shape[name])

    def _item_major_y(self, rows, key="_yT", y=None):
        """Item-major copy of the responses ([J + 1][stride] bytes, stride = n_local rounded up to 64; row J and the
        columns past n_local hold 254 = "outside the problem") for the dimension-major fc1 gradient kernel and the bf16-MFMA
        likelihood kernel (include/vipsy_amd.h, vx_irt_lik_grad): made once (the responses never change) and kept as
        self.<key>; full batches only.  y: the responses to copy, by default the likelihood's."""
        if rows is not None or self.n_local == 0:
            return None
        if getattr(self, key) is None:
            y = self._padded_y(lik=True) if y is None else y     # (the shard's own responses unless persons / items are padded)
            stride = (y.shape[0] + 63) // 64 * 64
            yT = torch.full((y.shape[1] + 1, stride), 254, dtype=torch.uint8, device=self.dev)
            yT[:y.shape[1], :y.shape[0]] = y.t()
            setattr(self, key, yT)
        return getattr(self, key)

    def _padded_y(self, lik=False):
        """The responses with the phantom persons of _pad_persons appended (made once; the responses themselves when none
        are).  lik: the copy the likelihood reads (phantom ITEMS absent instead of zero, IrtEngine._decide_shapes)."""
        y = self.y_lik if (lik and self.y_lik is not None) else self.y
        n_pad = self._n_pad
        if n_pad == self.n_local:
            return y
        key = "_y_pad_lik" if y is not self.y else "_y_pad"
        if getattr(self, key) is None:
            setattr(self, key, torch.cat([y, torch.full((n_pad - self.n_local, self.J), 255, dtype=torch.uint8, device=self.dev)]))
        return getattr(self, key)

    def _buf(self, key, n):
        t = self._ws.get(key)
        if t is None or t.numel() < n:
            t = torch.empty(max(int(n), 1), dtype=torch.float32, device=self.dev)
            self._ws[key] = t
        return t

    def _phase(self, name):
        return _Phase(self.events, name)

    # -- the grid family (grid.py: GridMixin): the classes without it refuse ----------------------
    def _no_grid(self, *args, **kw):
        raise NotImplementedError("%s has no grid scores: its pattern prior depends on a continuous latent, on the other "
                                  "persons of the batch, or it has no enumerated likelihood (IrtEngine with x_feature <= 3 and "
                                  "CcdmEngine have them)" % type(self).__name__)

    score = expected_counts = plausible_values = item_fit = marginal_loglik = fit_em = item_information = item_se = _no_grid
    fit_population = _no_grid
    residual_sums = local_dependence = _no_grid
    pair_tables = ld_x2 = _no_grid
    fit_sums = person_fit = item_msq = _no_grid
    group_counts = dif = _no_grid
    sumscore_tables = sx2 = score_table = _no_grid
    point_estimates = _no_grid
    score_bifactor = bifactor_structure = _no_grid
    expected_counts_bifactor = fit_em_bifactor = _no_grid

    def _gather_pp(self, rows, nb):
        """loc/raw (and their gradient targets) of the batch rows of a per-person guide."""
        n = self.n_local
        if rows is None:
            return self.PP[:n], self.PP[n:], self.GP[:n], self.GP[n:]
        return (self.PP[:n][rows].contiguous(), self.PP[n:][rows].contiguous(),
                self._buf("gloc", nb), self._buf("graw", nb))

    def _scatter_pp(self, rows, nb, gloc, graw):
        """Dense per-person gradients: zero off the batch, exactly what autograd hands the per-tensor
        Adam of the reference."""
        if rows is not None:
            n = self.n_local
            self.GP.zero_()
            self.GP[:n].index_add_(0, rows, gloc[:nb])
            self.GP[n:].index_add_(0, rows, graw[:nb])

    def _allreduce(self, t, op=None):
        """SUM (or `op`) of `t` over the ranks of `group`; nothing without one."""
        if self.group is not None:
            op = torch.distributed.ReduceOp.SUM if op is None else op
            if t.is_cuda and torch.distributed.get_backend(self.group) == "gloo":
                host = t.cpu()                               # rehearsal of N ranks on fewer GPUs: gloo reduces on the host
                torch.distributed.all_reduce(host, op=op, group=self.group)
                t.copy_(host)
            else:                                            # the product path: RCCL (backend "nccl") on the device buffer
                torch.distributed.all_reduce(t, op=op, group=self.group)

    def allreduce(self):
        """The one exchange of a step: SUM of [gradients | loss] over the ranks that share this problem.  Sharding is
        explicit -- `group` handed to the constructor -- never inferred from global torch.distributed state, so that
        independent problems (replications, vipsy_amd/harness.py) can run side by side under one process group."""
        self._allreduce(self.G)

    def _optim_segments(self, lrs):
        """The optimiser's (begin, end, lr) segments grouped by (betas, eps): of P, and of PP ({} without per-person rows)."""
        by_hyper, pp_hyper = {}, {}
        for name in self.names():
            o = self.off[name]
            by_hyper.setdefault(lrs.hyper_of(name), []).append((o, o + int(np.prod(self.shape[name])), float(lrs.lr_of(name))))
        if self.per_person:
            for nme, o in self.pp_off.items():
                pp_hyper.setdefault(lrs.hyper_of(nme), []).append((o, o + int(np.prod(self.pp_shape[nme])), float(lrs.lr_of(nme))))
        return by_hyper, pp_hyper

    def apply_optim(self, lrs):
        """Adam on the unconstrained leaves with the `free` mask (vi.py:508-514)."""
        self.t += 1
        by_hyper, pp_hyper = self._optim_segments(lrs)
        sd = self._step_dev
        kw = {"t_dev": sd} if sd is not None else {}         # captured step: Adam's t = the (already advanced) device counter
        if self._hip:                                        # the first optimiser launch also files the step's loss in the ring
            kw["loss"] = (self.G[self.n_params:self.n_params + 1], self.loss_ring)
        if len(by_hyper) == 1 and len(pp_hyper) == 1 and list(by_hyper) == list(pp_hyper):
            (betas, eps), segs = next(iter(by_hyper.items()))          # the usual case: one launch for both buffers
            self.be.adam2((self.P, self.G, self.M, self.V), self.free, self.n_params, _merge_segments(segs),
                          (self.PP, self.GP, self.MP, self.VP), self.pp_len, _merge_segments(pp_hyper[(betas, eps)]),
                          self.t, betas, eps, **kw)
            kw.pop("loss", None)
        else:
            for (betas, eps), segs in by_hyper.items():     # one launch per distinct (betas, eps): normally one
                self.be.adam(self.P, self.G, self.M, self.V, self.free, self.n_params, _merge_segments(segs), self.t, betas, eps, **kw)
                kw.pop("loss", None)
            for (betas, eps), segs in pp_hyper.items():
                self.be.adam(self.PP, self.GP, self.MP, self.VP, None, self.pp_len, _merge_segments(segs), self.t, betas, eps, **kw)
                kw.pop("loss", None)
        if not self._hip or "loss" in kw:
            # the CPU rehearsal backends of tests/ -- or a HIP step that launched no optimiser kernel at all (no trainable
            # segment): nothing filed the loss, so it is copied into its slot here
            self.loss_ring[self.t % LOSS_RING] = self.G[self.n_params]

    def _fused_tail_args(self, lrs, rows, eps, S):
        """The optimiser step for the step kernel's last launch to run (IrtEngine), or None: loss_and_grads | all-reduce |
        optimiser stay apart."""
        return None

    def _take_fused_tail(self):
        """{'adam': ...} for the step kernel's call when step() armed the fused tail (once: the call consumes it)."""
        ft, self._fused_tail = self._fused_tail, None
        if ft is None:
            return {}
        self._fused_done = True
        return {"adam": ft}

    def _grads_and_optim(self, lrs, rows, b_global, eps=None):
        """One particle's loss_and_grads, the all-reduce and the optimiser -- or, on one rank with a D = 1 per-person
        guide, all of it inside loss_and_grads (the optimiser rides in the step's last launch)."""
        self._fused_tail, self._fused_done = self._fused_tail_args(lrs, rows, eps, 1), False
        try:
            self.loss_and_grads(rows, b_global, eps, 0)
        finally:
            self._fused_tail = None
        if self._fused_done:
            self.t += 1                                      # (what apply_optim does first; the launch filed the loss in the ring)
            return
        with self._phase("allreduce"):
            self.allreduce()
        with self._phase("optimizer"):
            self.apply_optim(lrs)

    def step_loss(self):
        """The loss of the step just taken as a 0-d device tensor (no host sync): its slot of the ring, not overwritten for
        the next LOSS_RING - 1 steps -- a list of returned losses holds distinct values."""
        return self.loss_ring[self.t % LOSS_RING]

    # -- the whole step as one HIP graph ---------------------------------------------------------
    # A D = 1 full-batch step is a handful of 10-100 us kernels, a subsampled amortized step (the reference's own usage:
    # subsample_size = 100, test.py:338) ~25 launches around kernels of 5-80 us, and a 125 k-person shard of the headline ~25
    # launches around 1.3 ms of large kernels: launched one by one the host (Python + ctypes, ~10 us a launch) and the gaps
    # between short kernels are a fixed cost per step.  Nothing in such a step changes from call to call except the step count
    # (Philox counter, Adam bias corrections) -- read from a device word that the step's last reduction advances -- and, for a
    # subsample, the row indices -- copied into a fixed device buffer before the replay.  So the step is captured once per
    # FORM (full batch; or a subsample of nb rows out of b_global) and replayed.  A new learning rate (scheduler milestone)
    # or a re-allocated workspace captures again.
    #
    # Sharded persons (a process group): by default the step is TWO replays around the eager all-reduce -- loss_and_grads |
    # all_reduce(G) | optimiser -- three host calls instead of ~30, and no collective inside a capture.  VX_GRAPH_COLLECTIVE=1
    # captures the RCCL all-reduce into ONE graph (RCCL collectives are capturable); that form has not run on any hardware this
    # build could reach, so it is opt-in, and a capture that fails with a collective inside it RAISES: the communicator may be
    # unusable after a half-recorded collective, so the process must not carry on (no eager retry).
    use_graph = True

    def _graph_mode(self, rows, b_global, eps, S):
        """The captured form this call can replay -- ('full' | 'rows', nb, b_global) and, with S > 1 particles, S as a fourth
        entry -- or None for an eager step."""
        if not (self.use_graph and eps is None and self.events is None and self._hip):
            return None
        if S > 1:
            # Trace_ELBO(num_particles = S) (test.py:430: 20, test.py:607: 10): the S passes, their accumulation and the one
            # optimiser step as ONE graph.  Every particle draws its own subsample: S host index
            # tensors of one length, staged with one copy
            if rows is None:
                r0 = None
            elif (isinstance(rows, (list, tuple)) and len(rows) == S and all(torch.is_tensor(r) and not r.is_cuda for r in rows)
                  and len({int(r.numel()) for r in rows}) == 1):
                r0 = rows[0]
            else:
                return None
            base = self._graph_mode(r0, b_global, None, 1)
            return None if base is None else base + (S,)
        if rows is None:
            full = b_global is None or int(b_global) == self.N
            return ("full", self.n_local, self.N) if full and self._replayable(True) else None
        if not isinstance(rows, (list, tuple)) and self.n_local > 0 and self._replayable(False):
            nb = int(rows.numel())
            return ("rows", nb, int(b_global) if b_global is not None else nb)
        return None

    def _replayable(self, full):
        """Whether this engine's step replays a captured graph: its full batch (full) or a subsample (not full)."""
        return False

    def _graphable(self):
        """Whether the full-batch step of this engine replays a graph (tests, bench.py)."""
        return self._graph_mode(None, None, None, 1) is not None

    def _one_graph(self):
        """One graph for the whole step (no group, or the opt-in captured RCCL all-reduce) or two around an eager all-reduce."""
        if self.group is None:
            return True
        return (torch.distributed.get_backend(self.group) == "nccl" and os.environ.get("VX_GRAPH_COLLECTIVE", "0") == "1")

    def _graph_key(self, lrs):
        """Everything a captured step bakes into its kernel arguments: the (begin, end, lr) segments and (betas, eps) of
        every leaf as apply_optim computes them now (a new fit(), a scheduler milestone or a callable optim_args whose
        answer changed all change it), and the addresses of the buffers the kernels were handed (a workspace that
        _buf() has re-allocated since the capture would leave the graph writing into the old one)."""
        hyp = tuple((name, float(lrs.lr_of(name))) + lrs.hyper_of(name) for name in self.all_names())
        ptrs = tuple(sorted((k, t.data_ptr()) for k, t in self._ws.items()))
        return hyp, ptrs, self._one_graph()

    # the pinned host ring a captured subsampled step fetches its draw from: 16 slots, an event behind every 4th replay (a
    # record between two replays costs the GPU ~4 us of gap; tools/ring_sweep.sh: 8 / 1: 173.7 us a B = 100 step, 16 / 4: 168.9)
    rows_ring_slots = 16
    rows_ring_event_every = 4

    def _stage_rows(self, rows, buf, st=None, t=None):
        """The step's row indices into the fixed device buffer the captured kernels read.  Host indices (what the fit loop
        draws) go through a small ring of pinned buffers: one asynchronous copy, no staging allocation, no sync unless the
        GPU is a whole ring behind.  A form whose capture reads the ring itself (st["ring"]: vx_irt_cfg.rows_ring) only has
        the draw written into slot t % slots -- the replay fetches it."""
        if isinstance(rows, (list, tuple)):                  # S particles, S draws: [S][nb] in one buffer, one copy
            rows = torch.cat([r.reshape(-1) for r in rows])
        nb = buf.numel()
        if st is not None and st.get("ring") is not None:
            if rows.is_cuda:
                rows = rows.cpu()
            # the replay that last read this slot (step t - slots, if this form ran it) has finished once the OLDEST event
            # recorded at or behind that step has: events follow every `every`-th replay, so the host still runs
            # slots - every steps ahead of the GPU
            slot = (self.t if t is None else t) % self.rows_ring_slots
            lo, evs = st["ring_read"][slot], st["ring_ev"]
            if lo is not None:                               # the step that last read this slot
                for k in [k for k in evs if k < lo]:
                    del evs[k]
                if evs:
                    evs[min(evs)].synchronize()
                else:
                    torch.cuda.current_stream().synchronize()
                st["ring_read"][slot] = None
            st["ring"][slot, :nb].copy_(rows.reshape(-1))
            return
        if rows.is_cuda:
            buf.copy_(rows)
            return
        ring = self._pin_ring
        if ring is None or ring[0][0].numel() < nb:
            ring = self._pin_ring = [[torch.empty(max(nb, 1024), dtype=torch.int64).pin_memory(), None] for _ in range(8)]
            self._pin_i = 0
        slot = ring[self._pin_i]
        self._pin_i = (self._pin_i + 1) % len(ring)
        if slot[1] is not None:
            slot[1].synchronize()                            # the copy that last read this slot has run
        else:
            slot[1] = torch.cuda.Event()
        slot[0][:nb].copy_(rows.reshape(-1))
        buf.copy_(slot[0][:nb], non_blocking=True)
        slot[1].record()

    def _step_graph(self, lrs, mode, rows):
        st = self._graphs[mode]
        self._graph = st                                     # (the form last replayed: what tests / bench.py look at)
        key = self._graph_key(lrs)
        if st["graph"] is None or st["key"] != key:
            if self._ctr is None:
                self._ctr, self._ctr_t = torch.zeros(1, dtype=torch.int32, device=self.dev), None
            rows_buf = None
            ring = None
            S = mode[3] if len(mode) > 3 else 1
            if mode[0] == "rows":
                rows_buf = st.get("rows")
                if rows_buf is None:
                    rows_buf = torch.zeros(mode[1] * S, dtype=torch.int64, device=self.dev)
                self._stage_rows(rows, rows_buf)             # valid indices while the capture records
                ring = st.get("ring")
                if ring is None and S == 1 and not rows.is_cuda:
                    ring = torch.zeros(self.rows_ring_slots, max(int(mode[1]), 1), dtype=torch.int64).pin_memory()
            one = self._one_graph()
            torch.cuda.synchronize()
            gA, gB = torch.cuda.CUDAGraph(), None
            t0 = self.t
            self._step_dev = self._ctr
            self._capture_ring, self._capture_ring_used = ring, False
            try:
                # (thread-local capture mode: a process group's watchdog thread may query its events while this thread records)
                with torch.cuda.graph(gA, capture_error_mode="thread_local"):
                    # reads the counter as the Philox step, then advances it
                    if S > 1:
                        self._particles(S, lambda sidx: None if rows_buf is None else rows_buf[sidx * mode[1]:(sidx + 1) * mode[1]],
                                        mode[2] if mode[0] == "rows" else None, lambda sidx: None)
                        if one:
                            self.allreduce()
                            self.apply_optim(lrs)
                    elif one:
                        self._grads_and_optim(lrs, rows_buf, mode[2] if mode[0] == "rows" else None)   # (Adam's t: the counter)
                    else:
                        self.loss_and_grads(rows_buf, mode[2] if mode[0] == "rows" else None, None, 0)
                if not one:
                    gB = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gB, pool=gA.pool(), capture_error_mode="thread_local"):
                        self.apply_optim(lrs)
            except Exception as e:
                if one and self.group is not None:
                    raise RuntimeError("capturing the step with its RCCL all-reduce failed; the communicator may be unusable "
                                       "after a half-recorded collective, so this process must not carry on -- run again "
                                       "without VX_GRAPH_COLLECTIVE=1 (two replays around an eager all-reduce)") from e
                if self.group is not None and os.environ.get("VX_GRAPH_STRICT", "0") != "1":
                    # no collective was being recorded: the communicator is untouched and the same kernels can be launched one
                    # by one.  Sharded steps have never been captured next to a live RCCL communicator on the builder's boxes
                    # (one GPU each), so a failure here degrades -- loudly -- to the eager step instead of ending the job.
                    raise _GraphCaptureFailed(repr(e)) from e
                raise
            finally:
                self._step_dev = None
                self._capture_ring = None
                self.t = t0                                  # capture records, it does not run
            if not self._capture_ring_used:
                ring = None                                  # (this engine's forward does not read a ring: the copy stays)
            if st.get("ring_ev"):
                torch.cuda.current_stream().synchronize()
            st.update(graph=gA, tail=gB, key=key, rows=rows_buf, ring=ring, ring_ev={} if ring is not None else None,
                      ring_read=[None] * self.rows_ring_slots)
        if mode[0] == "rows":
            self._stage_rows(rows, st["rows"], st)
        if self._ctr_t != self.t:                            # (re)seed the device counter
            self._ctr.fill_(self.t)
        st["graph"].replay()
        if st["tail"] is not None:
            self.allreduce()
            st["tail"].replay()
        if st.get("ring") is not None:
            st["ring_read"][self.t % self.rows_ring_slots] = self.t
            if (self.t + 1) % self.rows_ring_event_every == 0:
                ev = st["ring_ev"][self.t] = torch.cuda.Event()
                ev.record()
        self.t += 1
        self._ctr_t = self.t
        return self.step_loss()

    # -- several steps of a fit loop from ONE replay ----------------------------------------------
    # Between two replays the GPU idles 6-9 us (the end of a graph releases to the system scope, the next one starts behind
    # it): a fifth of BASELINE config 2's 42 us step, 5 % of the reference's own B = 100 step.  Nothing a step needs from the
    # host is made by the step before it -- the Philox step and Adam's t come from the device counter, a subsample's rows from
    # the pinned ring (slot = counter % slots), the loss goes into the ring -- so graph_steps consecutive steps are captured
    # as one graph and a fit loop replays that (steps(): same kernels, same order, same bits as step() called in a loop --
    # except where IrtEngine.steps pads a subsample, see there).
    graph_steps = 4

    def _steps_form(self, lrs, rows_seq, b_global, scheduler):
        """The single-step form whose K-step graph can take the next K = graph_steps steps of a fit loop, or None."""
        K = self.graph_steps
        if K < 2 or len(rows_seq) < K or not self._graphs or not self._one_graph():
            return None
        mode = self._graph_mode(rows_seq[0], b_global, None, 1)
        if mode is None or any(self._graph_mode(r, b_global, None, 1) != mode for r in rows_seq[1:K]):
            return None
        st = self._graphs.get(mode)
        if st is None or st.get("graph") is None or st.get("key") != self._graph_key(lrs):
            return None                                      # (the form's first steps run one by one: eager, then its own capture)
        if mode[0] == "rows" and (st.get("ring") is None or any(r.is_cuda for r in rows_seq[:K])):
            return None
        if scheduler and any(lrs.epoch < m <= lrs.epoch + K - 1 for m in lrs.milestones):
            return None                                      # a milestone inside the K steps: their learning rates differ
        return mode

    def capture_steps(self, lrs, rows=None, b_global=None):
        """Captures the graph_steps-step graph of this form now (nothing runs), so that the first steps() call of a timed loop
        does not pay for it; True when the form has one afterwards (its single-step graph must exist: two steps taken)."""
        mode = self._steps_form(lrs, [rows] * self.graph_steps, b_global, False)
        if mode is None:
            return False
        return self._steps_capture(lrs, mode) is not None

    def _steps_capture(self, lrs, mode):
        st, K = self._graphs[mode], self.graph_steps
        mk = st.get("multi")
        key = (self._graph_key(lrs), K)
        if mk is None or mk["key"] != key:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            t0 = self.t
            self._step_dev = self._ctr
            self._capture_ring, self._capture_ring_used = st.get("ring"), False
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for _ in range(K):                        # (with a group: the captured collective inside)
                        self._grads_and_optim(lrs, st.get("rows"), mode[2] if mode[0] == "rows" else None)
            except Exception as e:
                # as in _step_graph: with a collective inside the capture the communicator may be unusable -- no way on; a
                # capture WITHOUT one (a second private pool that does not fit, a driver refusing the K-fold graph) leaves
                # nothing half-done: the form keeps its single-step graph and the fit loop takes the steps one by one
                if self.group is not None and self._one_graph():
                    raise RuntimeError("capturing %d steps with their RCCL all-reduce failed; the communicator may be unusable "
                                       "after a half-recorded collective -- run again without VX_GRAPH_COLLECTIVE=1" % K) from e
                if os.environ.get("VX_GRAPH_STRICT", "0") == "1":
                    raise
                import warnings
                warnings.warn("capturing %d steps as one graph failed (%r): this engine replays its steps one at a time from "
                              "now on (same results)" % (K, e))
                self.graph_steps = 1
                return None
            finally:
                self._step_dev = None
                self._capture_ring = None
                self.t = t0
            mk = st["multi"] = {"graph": g, "key": key}
        return mk

    def _steps_graph(self, lrs, mode, rows_seq, scheduler):
        st, K = self._graphs[mode], self.graph_steps
        self._graphs[mode] = self._graphs.pop(mode)          # most recently used last
        self._graph = st
        mk = self._steps_capture(lrs, mode)
        if mk is None:                                       # the K-step capture failed and was withdrawn: single steps
            return None
        t0 = self.t
        if mode[0] == "rows":
            for j in range(K):
                self._stage_rows(rows_seq[j], st["rows"], st, t=t0 + j)
        if self._ctr_t != self.t:
            self._ctr.fill_(self.t)
        mk["graph"].replay()
        if st.get("ring") is not None:
            for j in range(K):
                st["ring_read"][(t0 + j) % self.rows_ring_slots] = t0 + j
            ev = st["ring_ev"][t0 + K - 1] = torch.cuda.Event()      # (behind all K steps)
            ev.record()
        self.t += K
        self._ctr_t = self.t
        if scheduler:
            for _ in range(K):
                lrs.scheduler_step()
        return [self.loss_ring[(t0 + j + 1) % LOSS_RING] for j in range(K)]

    def steps(self, lrs, rows_seq, b_global=None, scheduler=False):
        """len(rows_seq) consecutive steps of a fit loop -- what step(lrs, rows=r, b_global=b_global) for r in rows_seq does,
        each followed by lrs.scheduler_step() when `scheduler` (vi.py:639-640) -- with the same results bit for bit, replayed
        graph_steps at a time from one graph where the form allows (tests/test_gpu_parity.py::
        test_steps_replayed_four_at_a_time_equal_single_steps, tests/test_gpu_fit_path.py::
        test_unpadded_steps_vs_oracle_and_bit_equal_to_step_in_a_loop).  A subclass that launches the steps over other rows
        than it was handed (IrtEngine.steps: a subsample that is no multiple of 4) promises the oracle's results within the
        parity tolerance instead, not step()'s bits.  rows_seq: one entry per step (None = the full batch, or host / device
        int64 LOCAL row indices).  Returns the losses, one 0-d device tensor per step (slots of the loss ring: the last
        LOSS_RING - 1 of them stay valid)."""
        out, i, n = [], 0, len(rows_seq)
        while i < n:
            mode = self._steps_form(lrs, rows_seq[i:], b_global, scheduler)
            if mode is not None:
                K = self.graph_steps
                got = self._steps_graph(lrs, mode, rows_seq[i:i + K], scheduler)
                if got is not None:
                    out += got
                    i += K
                    continue
            out.append(self.step(lrs, rows=rows_seq[i], b_global=b_global))
            if scheduler:
                lrs.scheduler_step()
            i += 1
        return out

    graph_max_row_forms = 8

    def _evict_graph_forms(self):
        """Every distinct (nb, b_global) subsample form holds a captured graph, its private pool and a rows buffer.  A fit loop
        has one form per rank; a caller whose local row count varies from step to step would otherwise keep one per count for
        ever: beyond graph_max_row_forms the least recently used 'rows' forms are dropped, graph and buffer."""
        forms = [m for m in self._graphs if m[0] == "rows"]
        for m in forms[:max(0, len(forms) - self.graph_max_row_forms)]:
            st = self._graphs.pop(m)
            if self._graph is st:
                self._graph = None
            # a replay of this form may still be queued: it reads the pinned rows ring through a raw device pointer (no event
            # of torch's host allocator guards that use) and runs out of the graph's private pool -- wait for the newest event
            # recorded behind its replays, or for the stream when there is none, before any of it can be handed out again
            evs = st.get("ring_ev")
            if evs:
                evs[max(evs)].synchronize()
            elif st.get("graph") is not None and self.dev.type == "cuda":
                torch.cuda.current_stream().synchronize()
            st.clear()                                       # releases the CUDAGraph objects (and their pool) and the rows buffer

    def _mean_of_passes(self, S, one_pass):
        """one_pass(sidx) for sidx < S and the mean of the G / GP they leave: surrogate / num_particles,
        summed into zeroed accumulators with weight 1 / S and copied back."""
        accG = torch.zeros_like(self.G)
        accP = torch.zeros_like(self.GP) if self.per_person else None
        for sidx in range(S):
            one_pass(sidx)
            accG.add_(self.G, alpha=1.0 / S)
            if accP is not None:
                accP.add_(self.GP, alpha=1.0 / S)
        self.G.copy_(accG)
        if accP is not None:
            self.GP.copy_(accP)

    def _particles(self, S, rows_of, b_global, eps_of):
        """S passes of loss_and_grads (particle sidx = Philox stream sidx) and their mean in G / GP.  While a capture records,
        every pass's last launch advances the device step counter: it is set back behind all but the last, so that the S
        particles share the step and the optimiser sees step + 1."""
        sd = self._step_dev

        def one_pass(sidx):
            self.loss_and_grads(rows_of(sidx), b_global, eps_of(sidx), sidx)
            if sd is not None and sidx < S - 1:
                sd.sub_(1)
        self._mean_of_passes(S, one_pass)

    def _score_pass(self, key, nb, stream_id, baseline_buf, guide_grads):
        """What a pass of the score-function estimator hands its kernel: (log_r, control variate, decay rate or -1,
        indexed-by-row flag).  log_r is buffer `key` -- in the first pass of 'loo' (guide_grads False) one per particle -- and
        is recorded as self.last_log_r; baseline_buf: the leave-one-out means of 'loo's second pass."""
        log_r = self.last_log_r = self._buf("%s%d" % (key, stream_id) if not guide_grads else key, nb)
        if baseline_buf is not None:
            return log_r, baseline_buf, -1.0, 0
        if self.baseline == "avg":
            return log_r, self.base, (self.baseline_beta if guide_grads else -1.0), 1
        return log_r, None, -1.0, 0

    # -- the 1-D normal encoder (NormEncoder, vi.py:417-455) in front of a step kernel: IrtEngine x_feature == 1, HoDinaEngine --
    def _norm_enc_forward(self, cfg, y, rows, nb):
        """The encoder's forward call over nb persons of y; returns what the backward call takes up again: the arguments the two
        share, fw = {h, loc, raw [, packws]}, the gradient targets gloc / graw the step kernel fills in between, the workspace."""
        fw = {"h": self._buf("h", nb * self.H), "loc": self._buf("loc", nb), "raw": self._buf("raw", nb)}
        n_pk = self.be.norm_enc_pack_floats(cfg)
        if n_pk > 0:
            fw["packws"] = self._buf("nenc_packws", n_pk)            # the forward's fp16-pair images of W1 (large batches)
        ne = SimpleNamespace(args=(cfg, y, rows, nb, self._enc()), fw=fw, gloc=self._buf("gloc", nb), graw=self._buf("graw", nb),
                             ws=self._buf("nencb_ws", self.be.norm_enc_bwd_workspace(cfg, nb)))
        with self._phase("guide_forward"):
            self.be.norm_enc_forward(*ne.args, fw)
        return ne

    def _norm_enc_backward(self, ne, yT):
        """... and its backward call (inside the caller's guide_backward phase); yT: the item-major responses, or None."""
        self.be.norm_enc_backward(*ne.args, ne.fw["h"], ne.gloc, ne.graw, self.G[self.enc_off0:self.enc_off0 + self.n_enc],
                                  ne.ws, yT=yT)

    def _zero_phantom_unit_grads(self):
        """Phantom hidden units of a three-layer encoder (fc1, two heads): their activation is softplus(0) = log 2, not zero,
        so their COLUMNS of both heads' weight gradients are zeroed behind the backward call and the columns stay zero."""
        if self.amortized and self.H != self.H_model:
            for k in ("fc21.weight", "fc22.weight"):
                self.view("encoder$$$" + k, self.G).view(-1, self.H)[:, self.H_model:].zero_()

    def _loo_step(self, lrs, rows, b_global, eps, S):
        """A step with the leave-one-out control variate of the score-function estimator (baseline 'loo', S >= 2 particles
        sharing the step's subsample): a first pass records log_r of every particle in self.last_log_r -- the same Philox draws
        as the second pass: the particle index is the Philox stream -- and the second pass takes each particle's baseline
        from the others' mean (vx_loo_baseline)."""
        rows = self._rows_on_device(rows)
        r = rows[0] if isinstance(rows, (list, tuple)) else rows
        nb = self.n_local if r is None else int(r.numel())

        def eps_of(sidx):
            return eps[sidx] if isinstance(eps, (list, tuple)) else eps
        lr_all = self._buf("loo_lr_all", S * nb)
        for sidx in range(S):
            self.loss_and_grads(r, b_global, eps_of(sidx), sidx, guide_grads=False)
            lr_all[sidx * nb:(sidx + 1) * nb].copy_(self.last_log_r[:nb])
        loo = self._buf("loo", nb)

        def one_pass(sidx):
            self.be.loo_baseline(lr_all, S, nb, sidx, loo)
            self.loss_and_grads(r, b_global, eps_of(sidx), sidx, baseline_buf=loo)
        self._mean_of_passes(S, one_pass)
        self.allreduce()
        self.apply_optim(lrs)
        return self.step_loss()

    def _rows_on_device(self, rows):
        """Host row indices (the fit loop's draw) for an eager step."""
        if rows is None or isinstance(rows, (list, tuple)):
            return [self._rows_on_device(r) for r in rows] if isinstance(rows, (list, tuple)) else None
        return rows if rows.device == self.dev else rows.to(self.dev)

    def step(self, lrs, rows=None, b_global=None, eps=None, num_particles=1):
        """loss_and_grads + optimiser, the body of SVI.step (vi.py:505-516).  `rows` (and `eps`) may be
        lists with one entry per particle: every particle draws its own subsample.
        rows: int64 LOCAL row indices, on the device or on the host (a captured step copies host indices itself).
        Returns the loss as a 0-d device tensor (no host sync, no launch of its own: the optimiser launch files it in a ring of
        LOSS_RING slots, see step_loss())."""
        S = int(num_particles)
        mode = self._graph_mode(rows, b_global, eps, S)
        if mode is not None:
            if mode in self._graphs:
                self._graphs[mode] = self._graphs.pop(mode)  # most recently used last (dicts keep insertion order)
                try:
                    return self._step_graph(lrs, mode, rows)
                except _GraphCaptureFailed as e:
                    import warnings
                    warnings.warn("HIP graph capture of the sharded step failed (%s): this rank steps kernel by kernel from "
                                  "here on (VX_GRAPH_STRICT=1 makes this an error)" % e)
                    self.use_graph = False                   # (same kernels, same results: launched one by one)
                    self.graph_fallback = str(e)
                    del self._graphs[mode]
                    mode = None
            if mode is not None:
                self._graphs[mode] = {"graph": None}         # the first step of a form runs eagerly: workspaces and lists get built
                self._graph = self._graphs[mode]
                self._evict_graph_forms()
        rows = self._rows_on_device(rows)
        if S == 1:
            self._grads_and_optim(lrs, rows[0] if isinstance(rows, (list, tuple)) else rows, b_global,
                                  eps[0] if isinstance(eps, (list, tuple)) else eps)
            return self.step_loss()
        else:
            self._particles(S, lambda sidx: rows[sidx] if isinstance(rows, (list, tuple)) else rows, b_global,
                            lambda sidx: eps[sidx] if isinstance(eps, (list, tuple)) else eps)
        with self._phase("allreduce"):
            self.allreduce()
        with self._phase("optimizer"):
            self.apply_optim(lrs)
        return self.step_loss()


class _GraphCaptureFailed(RuntimeError):
    """Capture of a sharded step (no collective inside) failed; _EngineBase.step() falls back to the eager step."""


class IrtEngine(GridMixin, _EngineBase):
    """IRT ELBO-gradient step (VIRT / VaeIRT of the reference, vi.py:536-723) on one rank.

    Flat parameter buffer: [a: D*J | b: J | c_un: J | d_un: J | encoder (nn.Linear order, amortized only)]."""

    # test seams, read from the environment once at import; an instance attribute overrides one (eng.pad_batch = False)
    pad_items = os.environ.get("VX_PAD_ITEMS", "1") != "0"          # 0 = the kernels see the problem's own item count
    pad_hidden = os.environ.get("VX_PAD_HIDDEN", "1") != "0"        # 0 = the kernels see the encoder's own width
    pad_dims = os.environ.get("VX_PAD_DIMS", "1") != "0"            # 0 = the kernels see the model's own dimensions
    pad_persons = os.environ.get("VX_PAD_PERSONS", "1") != "0"      # 0 = a full batch is launched over the shard's own count
    pad_batch = os.environ.get("VX_PAD_BATCH", "1") != "0"          # 0 = a subsample is launched over its own size
    score_mfma = os.environ.get("VX_SCORE_MFMA", "1") != "0"        # 0 = the scalar score-operand kernel for every shape
    graph_max_persons = int(os.environ.get("VX_GRAPH_MAX_PERSONS", str(1 << 40)))    # (_replayable)

    def __init__(self, y_u8, model="irt_2pl", D=1, Dc=1.0, n_global=None, gid0=0, amortized=False, H=64,
                 share_cov=False, a_free=None, a0=None, b0=None, encoder_init=None, seed=1234, group=None,
                 backend=None, observed_lists=True, estimator="pathwise", baseline="none", baseline_beta=0.9):
        """group: the torch.distributed process group whose ranks SHARE this problem (each holds a contiguous shard of
        persons: y_u8 = rows gid0 .. gid0 + n_local of the n_global); None = this process owns the whole problem.
        observed_lists: D = 1, full batch, >= 50 % missing -> step on compacted lists of observed cells.
        estimator: 'pathwise' = what pyro's Trace_ELBO does for the reference's Normal guides (vi.py:684,693,705,715,723);
        'score' (BASELINE.json north_star; every guide of this engine) = the score-function (REINFORCE) gradient of the
        guide, (log_r_i - baseline_i) d log q / d phi, with baseline 'none', 'avg' (per-person decaying average of log_r, rate
        baseline_beta) or 'loo' (leave-one-out mean over the particles of a step, num_particles >= 2; the particles then share
        the step's subsample).  The item gradients are the pathwise ones in every mode."""
        if estimator not in ("pathwise", "score"):
            raise ValueError("estimator must be 'pathwise' or 'score'")
        if baseline not in ("none", "avg", "loo"):
            raise ValueError("baseline must be 'none', 'avg' or 'loo'")
        self.estimator, self.baseline, self.baseline_beta = estimator, baseline, float(baseline_beta)
        self._preamble(y_u8, backend, n_global, gid0, seed, group)
        self.observed_lists = bool(observed_lists) and estimator == "pathwise"
        self.model, self.Dc, self.share_cov = model, float(Dc), bool(share_cov)
        self._decide_shapes(int(D), bool(amortized), int(H))
        J, Dd = self.J, self.D
        self.off = {"a": 0, "b": Dd * J, "c": Dd * J + J, "d": Dd * J + 2 * J}
        self.shape = {"a": (Dd, J), "b": (1, J), "c": (1, J), "d": (1, J)}
        self.n_item = Dd * J + 3 * J
        if self.amortized:
            T = Dd * (Dd + 1) // 2 if Dd > 1 else 1
            o = self._encoder_segments({"fc1.weight": (self.H, J), "fc1.bias": (self.H,), "fc21.weight": (Dd, self.H),
                                        "fc21.bias": (Dd,), "fc22.weight": (T, self.H), "fc22.bias": (T,)})
        else:
            o = self.n_item
            if Dd > 1:                                    # VIRT.guide for x_feature > 1 (vi.py:706-723)
                if self.share_cov:                        # one (D, D) Cholesky factor, replicated like an item parameter
                    o = (self.n_item + 63) // 64 * 64
                    self.off["x_scale"] = o
                    self.shape["x_scale"] = (Dd, Dd)
                    o += Dd * Dd
                    self.pp_shape = {"x_local": (self.n_local, Dd)}
                else:
                    self.pp_shape = {"x_local": (self.n_local, Dd), "x_scale": (self.n_local, Dd, Dd)}
        self._alloc(o, self.n_local, per_person=not self.amortized)
        self._fill_initial_values(a0, b0, a_free, encoder_init, seed)
        self.base = (torch.zeros(max(self.n_local, 1), dtype=torch.float32, device=self.dev)
                     if (estimator == "score" and baseline == "avg") else None)
        self._sp = self._y_ext = self._y_ext_lik = None      # made on first use (_sparse_lists, _pad_batch)
        self._phantom_rows = 0                               # phantom rows at the tail of the subsamples steps() is running
        # the pass of this guide (loss_and_grads), by name: a bound method kept on the instance would be a reference cycle
        self._guide_pass = "_pass_1d" if self.D == 1 else ("_pass_mvn_enc" if self.amortized else "_pass_mvn_pp")

    def _decide_shapes(self, D, amortized, H):
        """The shapes the kernels see -- self.J, self.D, self.H, at or above the problem's own J_items, D_model, H_model -- and,
        with phantom items, the two copies of the responses.  Three kinds of phantom are decided here, each beside the argument
        why it is harmless; phantom persons and phantom subsample rows depend on the call (_pad_persons, _pad_batch)."""
        mfma = amortized and self._hip                             # the kernels whose shape conditions the phantoms meet
        self.J_items, self.D_model, self.H_model = self.J, D, (H if amortized else 0)     # the problem's own
        if mfma and 0 < H < 64 and self.pad_hidden:
            # PHANTOM HIDDEN UNITS up to 64, the width the MFMA kernels are built for (hidden_dim 32: 23.6 ms a step where 64
            # takes 2.4, tools/hidden_cliffs.py).  A phantom unit has a zero row of fc1 (weight and bias) and zero columns in
            # both heads.  Its activation is softplus(0) = log 2, not zero (vi.py:430,447), so the heads' columns WOULD take
            # gradients: they are zeroed behind the backward call (_zero_phantom_head_grads) and the columns stay zero; d ELBO /
            # d h_u is a sum over head rows times those zero columns, so fc1's row takes no gradient at all.
            H = 64
        if mfma and H == 64 and self.J_items % 4 != 0 and self.J_items > 0 and self.pad_items:
            # PHANTOM ITEMS up to a multiple of 4: the MFMA kernels of the amortized guides read response rows in
            # 16-byte pieces and refuse other item counts (J = 499: 18.0 ms a step where J = 500 takes 2.1, tools/shape_cliffs.py).
            # A phantom item is ABSENT for the likelihood (byte 254, "outside the problem": no log-probability, no gradient)
            # and ZERO for the encoder (its input and the fc1 gradient's activation), so there are two copies of the responses:
            # self.y (phantom byte 0) for the guide's forward / backward calls, self.y_lik (254) for the likelihood call and
            # the item-major copy.  Its parameters -- a column of a, entries of b / c / d, a column of fc1.weight -- take
            # zero gradients for ever (Adam leaves them where they start) and are not visible through unconstrained() / param().
            # (The observed-cell lists of the 1-D step count a phantom among a person's J - n_observed unobserved items, each
            # of which carries the reference's constant log Bern(0 | clamp(0)) = -1.19e-7: 1e-9 of a person's ELBO.)
            pad = (-self.J_items) % 4
            self.y_lik = torch.cat([self.y, torch.full((self.n_local, pad), 254, dtype=torch.uint8, device=self.dev)], 1).contiguous()
            self.y = torch.cat([self.y, torch.zeros((self.n_local, pad), dtype=torch.uint8, device=self.dev)], 1).contiguous()
        self.J = int(self.y.shape[1])                              # items the kernels see (J_items + phantoms)
        if mfma and D > 1 and D % 4 != 0 and D + 3 <= 124 and H == 64 and self.pad_dims:
            # PHANTOM DIMENSIONS up to a multiple of 4 (the MFMA kernels' other shape condition: D = 99: 31 ms a step where
            # D = 100 takes 2.1).  A phantom dimension k has a_k = 0 for ever (free mask 0: it never reaches a logit) and head
            # rows (fc21 row k, the fc22 rows (k, .), their biases) that start at ZERO and are kept there by zeroing their
            # gradients behind the backward call: mu_k = 0, L_kk = e^0 = 1, L_kl = 0, so x_k = eps_k and the phantom's
            # terms of the ELBO cancel (-x_k^2 / 2 from the prior, +eps_k^2 / 2 + M_kk from the entropy), and the shared
            # hidden layer gets nothing from it (its rows of the head weights are what the hidden gradient multiplies by).
            # The draws of the real dimensions are the same (Philox blocks of four dimensions), tril order puts the real
            # fc22 rows first.  Not visible through unconstrained() / param().
            D = (D + 3) // 4 * 4
        self.D, self.amortized, self.H = D, amortized, H if amortized else 0      # dimensions, hidden units the kernels see

    def _fill_initial_values(self, a0, b0, a_free, encoder_init, seed):
        """The reference's initial values (vi.py:567-587) over the problem's own items, dimensions and hidden units; every
        phantom's parameters start at zero (_decide_shapes says why they stay there)."""
        model, J, Dd, Ji, Dm = self.model, self.J, self.D, self.J_items, self.D_model
        a_init = torch.ones(Dm, Ji) if a0 is None else torch.as_tensor(a0, dtype=torch.float32).reshape(Dm, Ji).clone()
        if a_free is None and Dm > 1:
            af = torch.ones(Dm, Ji)
            for i in range(Dm):
                af[i, Ji - i:] = 0                                 # vi.py:570-572
            a_init = a_init * af                                   # also a user-supplied a0 is zeroed there (vi.py:571)
            a_free = af
        if Dd != Dm and a_free is None:
            a_free = torch.ones(Dm, Ji)
        if model != "irt_1pl":
            self.view("a").copy_(_grown(a_init, (Dd, J)).reshape(-1))
            if a_free is not None:
                self.view("a", self.free).copy_(_grown(torch.as_tensor(a_free, dtype=torch.float32).reshape(Dm, Ji), (Dd, J)).reshape(-1))
        if b0 is not None:
            self.view("b").copy_(_grown(torch.as_tensor(b0, dtype=torch.float32).reshape(1, Ji), (1, J)).reshape(-1))
        if model in ("irt_3pl", "irt_4pl"):
            self.view("c").fill_(float(np.float32(_logit(np.float32(0.1)))))
        if model == "irt_4pl":
            self.view("d").fill_(float(np.float32(_logit(np.float32(1.0) - np.float32(0.1)))))
        if self.amortized:
            self._fill_encoder(default_encoder_init(Ji, Dm, self.H_model, seed) if encoder_init is None else encoder_init,
                               Ji, self.H_model)

    def _dim_major(self, cfg, n):
        """Whether the dimension-major backward kernels take n persons of this shape: the backward call then reads gxT and gdT
        and no gx, and a phantom person or row can leave the step as a column of those two (_take_out_phantoms)."""
        return self.be.mvn_enc_bwd_layout(cfg, n) == 1 and self.be.mvn_enc_bwd_gd_offset(cfg, n) >= 0

    def _pad_batch(self, rows, b_global, eps):
        """A SUBSAMPLE whose size is no multiple of 4 (B = 50: 315 us a step where B = 100 takes 144 -- the person-major
        generation of the backward kernels) is drawn 1-3 rows longer: the extra rows point at ONE phantom person behind the
        shard's own (index n_local of an extended copy of the responses, every response missing), and loss_and_grads takes
        them out behind the likelihood by their index (columns of gxT / gdT, entries of ll / ent times 0), as _pad_persons
        does for a full batch.  The plate scale stays the caller's: b_global is made explicit.  Amortized multivariate guide,
        pathwise estimator, HIP backend; rows: one tensor or a list of them.  Only steps() pads: step() launches a subsample
        over its own size."""
        if (rows is None or eps is not None or not self.pad_batch or not (self.amortized and self.D > 1 and self.H == 64)
                or not self._hip or self.estimator != "pathwise"):
            return rows, b_global
        many = isinstance(rows, (list, tuple))
        rs = list(rows) if many else [rows]
        if not rs or not all(torch.is_tensor(r) for r in rs) or len({int(r.numel()) for r in rs}) != 1:
            return rows, b_global
        n = int(rs[0].numel())
        pad = (-n) % 4
        if pad == 0 or n == 0:
            return rows, b_global
        cfg = self.be.cfg(self.model, self.D, self.J, self.H, self.Dc, 1.0, self.seed, 0, 0)
        if not self._dim_major(cfg, n + pad):
            return rows, b_global
        if self._y_ext is None:
            miss = torch.full((1, self.J), 255, dtype=torch.uint8, device=self.dev)
            self._y_ext = torch.cat([self.y, miss]).contiguous()
            self._y_ext_lik = self._y_ext if self.y_lik is None else torch.cat([self.y_lik, miss]).contiguous()
        rs = [torch.cat([r.reshape(-1), torch.full((pad,), self.n_local, dtype=r.dtype, device=r.device)]) for r in rs]
        return (rs if many else rs[0]), (n if b_global is None else b_global)

    def step(self, lrs, rows=None, b_global=None, eps=None, num_particles=1):
        """The common step (_EngineBase.step), or the two passes over the particles of the leave-one-out control variate
        (score-function estimator, baseline 'loo', _loo_step).  A subsample is launched over its own size (steps() pads)."""
        S = int(num_particles)
        if self.estimator == "score" and self.baseline == "loo" and S >= 2:
            return self._loo_step(lrs, rows, b_global, eps, S)
        return super().step(lrs, rows=rows, b_global=b_global, eps=eps, num_particles=S)

    def steps(self, lrs, rows_seq, b_global=None, scheduler=False):
        """_EngineBase.steps over subsamples padded to a multiple of 4 rows (_pad_batch) when all have one size.  Where nothing
        is padded the results are those of step() in a loop, bit for bit.  Where rows are padded the steps run other kernels
        over other row counts than step() does, so the bits differ: both are within the parity tolerance of the oracle, loss
        by loss and gradient by gradient (tests/test_gpu_fit_path.py::test_padded_steps_vs_oracle_at_frozen_parameters, and
        test_trained_trajectory_through_padded_steps_within_1e3_of_cpu_reference for the trained parameters)."""
        phantoms = 0
        if rows_seq and all(torch.is_tensor(r) for r in rows_seq) and len({int(r.numel()) for r in rows_seq}) == 1:
            n = int(rows_seq[0].numel())
            padded, b_global = self._pad_batch(list(rows_seq), b_global, None)   # (a list: the same rule as for particles)
            rows_seq, phantoms = padded, int(padded[0].numel()) - n
        self._phantom_rows = phantoms                        # loss_and_grads refuses a launch that could not take them out
        try:
            return super().steps(lrs, rows_seq, b_global=b_global, scheduler=scheduler)
        finally:
            self._phantom_rows = 0

    def _pad_persons(self, rows, eps, cfg=None):
        """How many PHANTOM persons (0-7) the full-batch kernels of an amortized guide are launched over behind the shard's
        own: up to the next multiple of 8.  The dimension-major operands of the large-batch kernels are rows of `nb` floats
        (fp16 planes: `nb` halves) read in 16-byte pieces, so a count that is not a multiple of 8 sends the head weight gradient
        (and, below a multiple of 4, everything) to the fp32-MFMA generation: 13.9 ms a step at 1 000 004 persons, 26.3 at
        999 999, against 9.1 at 1 000 000 (the 1-D guide's encoder: 2.0 against 0.87 ms at 999 999 x 500).  A phantom has every
        response missing (byte 255: a finite guide sample, no likelihood term) and is zeroed out of the step in front of the
        guide's backward call (_take_out_phantoms; _pass_1d: gloc / graw), so it adds nothing to any gradient or to the loss.
        Pathwise estimator, HIP backend, the kernels' own draws, full batch only.  cfg: the multivariate guide's, whose backward
        must take the padded count dimension-major (the phantoms leave as columns of its operands); the 1-D guide: None."""
        n = self.n_local
        if (rows is not None or eps is not None or n % 8 == 0 or n < 8 or not self._hip
                or self.estimator != "pathwise" or not self.pad_persons):
            return 0
        pad = (-n) % 8
        return pad if (cfg is None or self._dim_major(cfg, n + pad)) else 0

    @staticmethod
    def _take_out_phantoms(D, nb, gxT, gdT, ll, ent, n_valid=None, keep=None):
        """Where phantoms leave a multivariate step, behind the likelihood: their columns of gxT / gdT ([D][nb]: all the
        backward kernels see of a person) and their entries of ll / ent.  Phantom PERSONS stand behind the n_valid real ones and
        are zeroed, whatever the kernels left there; phantom ROWS of a padded subsample stand wherever the draw put them and are
        multiplied by keep (0 for a phantom, 1 for a row of the shard).  They occur in different steps and stay two operations."""
        gxm, gdm = gxT[:nb * D].view(D, nb), gdT[:nb * D].view(D, nb)
        if n_valid is not None:
            for t in (gxm[:, n_valid:], gdm[:, n_valid:], ll[n_valid:nb], ent[n_valid:nb]):
                t.zero_()
        if keep is not None:
            for t in (gxm, gdm, ll[:nb], ent[:nb]):
                t.mul_(keep)

    def _sparse_lists(self, rows):
        """Observed-cell lists for the D = 1 kernel (include/vipsy_amd.h, vx_irt1d_sparse_grad): built once -- the
        responses never change -- and only when most cells are missing and the batch is the whole shard.  Persons are
        placed in slots sorted by list length inside windows of 4096, so the 64 lists a wave walks end together."""
        if rows is not None or self.n_local == 0 or self.J > 1024 or not self.observed_lists:
            return None
        if self._sp is None:
            y, n, J = (self.y_lik if self.y_lik is not None else self.y), self.n_local, self.J
            frac = float((y == 255).sum().item()) / float(n * J)
            if frac < 0.5:
                self._sp = False
            else:
                ng = (n + 63) // 64
                cnt = torch.full((ng * 64,), -1, dtype=torch.int64, device=self.dev)             # -1: empty slot, sorts last
                cnt[:n] = (y < 254).sum(1)                                                     # (254: a phantom item, absent)
                slot = torch.arange(ng * 64, device=self.dev)
                perm = torch.argsort((slot // 4096) * (J + 2) + (J - cnt), stable=True)           # slot -> person
                cnt_s = cnt[perm].clamp_(min=0)
                pidx = torch.where(perm < n, perm, torch.full_like(perm, -1)).to(torch.int32).contiguous()
                Lq = max(1, (int(cnt_s.max().item()) + 3) // 4)
                W = min(J, 4 * Lq)
                pent = torch.full((ng * 64, 4 * Lq), -1, dtype=torch.int16, device=self.dev)      # 0xFFFF = past the end
                ar = torch.arange(W, device=self.dev)[None, :]
                for lo in range(0, ng * 64, 65536):                                               # bounded temporaries
                    hi = min(ng * 64, lo + 65536)
                    yc = y[perm[lo:hi].clamp(max=n - 1)]
                    order = torch.argsort((yc >= 254).to(torch.uint8), dim=1, stable=True)[:, :W]  # observed items first
                    code = order.to(torch.int32) | ((torch.gather(yc, 1, order) == 1).to(torch.int32) << 15)
                    code = torch.where(ar < cnt_s[lo:hi, None], code, torch.full_like(code, 0xFFFF))
                    pent[lo:hi, :W] = code.to(torch.int16)                                        # wraps: bit pattern kept
                pent = pent.reshape(ng, 64, Lq, 4).permute(0, 2, 1, 3).contiguous()
                glen = ((cnt_s.reshape(ng, 64).max(1).values + 3) // 4).to(torch.int32).contiguous()
                self._sp = {"pent": pent, "glen": glen, "Lq": Lq, "pidx": pidx, "n_groups": ng, "missing": frac}
        return self._sp or None

    # -- the optimiser inside the step's last launch (one rank, D = 1 per-person guides) --------------
    fuse_tail = True

    def _fused_tail_args(self, lrs, rows, eps, S):
        """What vx_irt1d_grad_adam needs to run Adam in the launch that sums the step's slabs -- or None when this step has
        to keep loss_and_grads | all-reduce | optimiser apart (a process group, an amortized or multivariate guide, a
        subsample whose gradients are scattered afterwards, the score-function estimator, more than one (betas, eps))."""
        if not (self.fuse_tail and self.group is None and S == 1 and rows is None and self._hip and self.D == 1 and not self.amortized and self.per_person
                and self.estimator == "pathwise" and self.events is None and self.n_params == 4 * self.J):
            return None
        by_hyper, pp_hyper = self._optim_segments(lrs)
        if not (len(by_hyper) == 1 and len(pp_hyper) == 1 and list(by_hyper) == list(pp_hyper)):
            return None
        (betas, eps_), segs = next(iter(by_hyper.items()))
        return {"A": (self.P, self.M, self.V, self.free, self.n_params, _merge_segments(segs)),
                "B": (self.PP, self.GP, self.MP, self.VP, self.pp_len, _merge_segments(pp_hyper[(betas, eps_)])),
                "t": self.t + 1, "betas": betas, "eps": eps_, "loss_ring": self.loss_ring}

    def _replayable(self, full):
        # the pathwise estimator, every guide.  D = 1 per-person guide: a full batch is a handful of 10-100 us kernels; a
        # subsample's gradients are scattered into zeroed dense ones.  The amortized 1-D guide (VaeIRT x_feature == 1; the
        # reference's Irt2PLMissing.test_ai draws 100 rows a step): the step kernel's slab sum advances the counter, nothing
        # behind it reads it but Adam.  VIRT with x_feature > 1 (vi.py:706-723; the CFA demo of test.py:420-430 draws 100
        # rows a particle): the backward kernel scatters the batch's rows into the zeroed per-person gradients itself.
        # The amortized multivariate guide: a large shard runs short kernels BESIDE long ones on a second stream (the last
        # chip round of the forward and the hidden gradient, the fc1 gradient); the capture keeps those branches as graph
        # edges.  Until round 5 the replayed 1M step was the slower one (10.7 against 10.1 ms) and shards above 300 k ran
        # eagerly; with the round-6 kernels it is the faster one at every size measured (tools/step_events_cost.py: 8.97
        # against 9.00 ms at 1M, 4.53 against 4.65 at 500 k, 1.46 against 1.63 at 125 k), so every shard replays.
        # VX_GRAPH_MAX_PERSONS remains as the switch back for its full batch
        if self.estimator != "pathwise":
            return False
        return not (full and self.amortized and self.D > 1 and self.n_local > self.graph_max_persons)

    def unconstrained(self, name, buf=None):
        u = super().unconstrained(name, buf)
        if self.J != self.J_items and name in ("a", "b", "c", "d", "encoder$$$fc1.weight"):
            u = u[..., :self.J_items]                              # (phantom items are nobody's business)
        if self.D != self.D_model:                                 # (nor are phantom dimensions)
            if name == "a" or name.startswith("encoder$$$fc21"):
                u = u[:self.D_model]
            elif name.startswith("encoder$$$fc22"):
                u = u[:self.D_model * (self.D_model + 1) // 2]
        if self.amortized and self.H != self.H_model:              # (nor phantom hidden units)
            if name.startswith("encoder$$$fc1."):
                u = u[:self.H_model]
            elif name in ("encoder$$$fc21.weight", "encoder$$$fc22.weight"):
                u = u[:, :self.H_model]
        return u

    def _zero_phantom_head_grads(self):
        """Phantom dimensions: the gradients of their head rows go back to zero; phantom hidden units: the gradients of their
        head columns (_decide_shapes)."""
        Dm, H = self.D_model, self.H
        if self.D != Dm:
            Tm = Dm * (Dm + 1) // 2
            for k, lo in (("fc21.weight", Dm * H), ("fc21.bias", Dm), ("fc22.weight", Tm * H), ("fc22.bias", Tm)):
                self.view("encoder$$$" + k, self.G)[lo:].zero_()
        self._zero_phantom_unit_grads()

    # -- parameter access (constrained values as pyro.param(name) returns them) -----------------
    def names(self):
        out = ["b"]
        if self.model != "irt_1pl":
            out.append("a")
        if self.model in ("irt_3pl", "irt_4pl"):
            out.append("c")
        if self.model == "irt_4pl":
            out.append("d")
        if self.amortized:
            out += ["encoder$$$" + k for k in ENC_KEYS]
        elif self.D > 1 and self.share_cov:
            out.append("x_scale")
        return out

    def param(self, name):
        u = self.unconstrained(name)
        if name in ("c", "d"):
            return torch.sigmoid(u)
        if name == "x_scale":
            if self.D == 1:
                return torch.exp(u)
            diag = torch.diagonal(u, dim1=-2, dim2=-1)                # lower_cholesky transform (vi.py:712,720)
            return torch.tril(u, -1) + torch.diag_embed(torch.exp(diag))
        return u.clone()

    population = None            # fit_population()'s result: {"gamma" [p][D], "sigma" [D][D], "intercept"}

    def score(self, y_u8=None, rows=None, nodes=61, span=6.0, covariates=None):
        """Person scores by quadrature over a grid (score_grid): for each scored row the posterior mean `eap` (n, D) and
        standard deviation `psd` (n, D) of the latent under the N(0, I) prior and the item parameters as they stand, the
        marginal log-likelihood `loglik` (n,) and the MAP grid node `node` (n,).  y_u8: responses to score ([n, item_size]
        uint8, 255 = missing), by default the training responses; rows: indices into them.  Exact and deterministic, needs
        no guide: new respondents are scored like training ones.  The model's own items and dimensions only -- phantom
        items / dimensions of a padded engine are not in the tables.  x_feature <= 3 and nodes ** x_feature <= 1024.
        covariates ([rows of y_u8][p], indexed by `rows` where rows is given): score under each person's own prior
        N(Gamma^T x_i, Sigma) of the population fit_population() estimated, instead of N(0, I); then also `cov` (n, D, D), the
        posterior covariance (psd = the square roots of its diagonal), and `prior_mean` (n, D) = Gamma^T x_i."""
        if covariates is not None:
            call, tilt, mu = self._population_call(y_u8, rows, nodes, span, covariates)
            out = self._grid_posterior_cond(call, tilt)
            cov = tri_to_full(out["cov"], call.D)
            return {"eap": out["mean"], "psd": torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1)).contiguous(),
                    "loglik": out["logjoint"] - out["lognorm"], "node": out["node"], "cov": cov, "prior_mean": mu}
        out = self._grid_posterior(self._grid_call(y_u8, rows, nodes, span))
        return {"eap": out["mean"], "psd": out["sd"], "loglik": out["loglik"], "node": out["node"]}

    def bifactor_structure(self, general=0):
        """The bifactor / testlet structure of this model, read from the engine's free mask (a_free, or the triangular default)
        and the loadings as they stand, on the host (grid.bifactor_structure): {"general", "specific_dims", "testlet" (the column
        of specific_dims an item loads on; -1: the general dimension alone), "sizes"}.  The model's own items and dimensions.
        Every x_feature = 2 model is a bifactor with one specific dimension; the default mask of x_feature >= 3 is refused."""
        if self.model == "irt_1pl" or self.D_model < 2:
            return bifactor_structure(np.zeros((1, 1)), np.zeros((1, 1)), self.model, general)      # (raises)
        return bifactor_structure(self.unconstrained("a", self.free).cpu().numpy(), self.unconstrained("a").cpu().numpy(),
                                  self.model, general)

    def score_bifactor(self, y_u8=None, rows=None, nodes=(61, 21), span=(6.0, 4.0), general=0, specific=False, covariates=None):
        """Exact grid scores of a bifactor / testlet model (bifactor_structure(general)), any x_feature >= 2: given the general
        node the testlets are independent, each a one-dimensional integral over its own specific factor (Gibbons & Hedeker), so
        the work is that of ONE two-dimensional grid of nodes = (Gg, Gh) points (grid.bifactor_grid) whatever the number of
        specific dimensions.  y_u8 / rows, missing codes, new respondents, phantoms and the shard of a process group as score().
        Returns `loglik` (n,), `eap_general`, `psd_general` (n,) and `node` (n,) int32, the MAP node of the general MARGINAL
        posterior (ties: the lowest); with specific=True also `eap_specific`, `psd_specific` (n, S) and `specific_dims` [S], the
        model dimension behind each column -- a second kernel that recomputes the tiles, so the MFMA work doubles.  A specific
        dimension without items gets the moments of the grid prior.  The item order is free: the responses are permuted into
        the testlet layout on the device, grid.bifactor_slab_persons() persons at a time.  Deterministic: the same call gives
        the same bits, and so does a person reached through `rows`.
        ValueError beyond 2 <= Gg <= 256, 1 <= Gh <= 32, 1 024 items or an operand image of 512 MB (Gg x item chunks x 4 KB)."""
        if covariates is not None:
            raise NotImplementedError("score_bifactor with covariates=: the latent regression of fit_population() is built for "
                                      "x_feature <= 3 and the tensor-product grid of score()")
        bf = self._bifactor_call(y_u8, rows, nodes, span, general)
        bf.fill()
        n, S, Gg, KC, plan, dev = bf.n, len(bf.st["specific_dims"]), bf.Gg, bf.KC, bf.plan, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"loglik": torch.empty(n, **f32), "eap_general": torch.empty(n, **f32), "psd_general": torch.empty(n, **f32),
               "node": torch.empty(n, dtype=torch.int32, device=dev)}
        if specific:
            # a dimension without items: the moments of the grid prior
            v = np.exp(bf.logv_np.astype(np.float64))
            v = v / v.sum()
            m1 = float((v * bf.u_np).sum())
            sd0 = float(np.sqrt(max((v * bf.u_np.astype(np.float64) ** 2).sum() - m1 * m1, 0.0)))
            out["eap_specific"] = torch.full((n, S), m1, **f32)
            out["psd_specific"] = torch.full((n, S), sd0, **f32)
            out["specific_dims"] = bf.st["specific_dims"]
            real = np.flatnonzero(plan["tl_column"] >= 0)
            real_t, cols_t = torch.from_numpy(real).to(dev), torch.from_numpy(plan["tl_column"][real]).to(dev)
        for s0, s1, yp in bf.slabs():
            fws = torch.empty(self.be.grid_bifactor_workspace(s1 - s0, Gg), **f32) if specific else None
            self.be.grid_bifactor(yp, s1 - s0, KC, plan["tl_start"], bf.tl_dev, bf.img, bf.logw, bf.theta, bf.logv, bf.u,
                                  out["loglik"][s0:s1], out["eap_general"][s0:s1], out["psd_general"][s0:s1], out["node"][s0:s1], fws)
            if specific:
                ms = torch.empty(len(plan["tl_column"]), s1 - s0, **f32)
                ss = torch.empty_like(ms)
                self.be.grid_bifactor_specific(yp, s1 - s0, KC, Gg, plan["tl_start"], bf.tl_dev, bf.img, bf.logv, bf.u,
                                               out["loglik"][s0:s1], fws, ms, ss)
                out["eap_specific"][s0:s1, cols_t] = ms[real_t].t()
                out["psd_specific"][s0:s1, cols_t] = ss[real_t].t()
        return out

    def _bifactor_call(self, y_u8, rows, nodes, span, general, params=None):
        """What score_bifactor, expected_counts_bifactor and fit_em_bifactor share (grid.BifactorCall): the two axes, the structure
        and the testlet layout, the responses and rows, the operand image (bf.fill() tabulates `params` into it: compact a
        [D_model][J_items], b, c_un, d_un or None -- by default the leaves as they stand) and bf.slabs(), the responses permuted
        into the layout, grid.bifactor_slab_persons() persons at a time."""
        theta_np, logw_np, u_np, logv_np = bifactor_grid(nodes, span)
        st = self.bifactor_structure(general)
        plan = bifactor_plan(st["testlet"], st["specific_dims"], theta_np.shape[0])
        J, Dm, KC = self.J_items, self.D_model, plan["KC"]
        y, rows = self._score_inputs(y_u8, rows, J)
        n = int(y.shape[0]) if rows is None else int(rows.numel())
        dev = self.dev
        theta, logw, u, logv = (torch.from_numpy(t).to(dev) for t in (theta_np, logw_np, u_np, logv_np))
        col, sdim, tl_dev = (torch.from_numpy(plan[k]).to(dev) for k in ("col", "sdim", "tl_start"))
        if params is None:
            flat = lambda name: self.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
            params = (self.unconstrained("a").contiguous(), flat("b"), flat("c") if self.model in ("irt_3pl", "irt_4pl") else None,
                      flat("d") if self.model == "irt_4pl" else None)
        cfg = self.be.cfg(self.model, Dm, J, 0, self.Dc, 1.0, 0, 0, 0)
        img = torch.empty(self.be.grid_bifactor_image_bytes(len(theta_np), KC), dtype=torch.uint8, device=dev)
        # slot -> column of the responses, the padding slots to one more column of 254 ("outside the problem")
        src = torch.where(col >= 0, col, torch.full_like(col, J)).long()
        slab = bifactor_slab_persons(KC)

        def fill():
            self.be.grid_table_bifactor(cfg, theta, u, st["general"], col, sdim, KC, *params, img)

        def slabs():
            for s0 in range(0, n, slab):
                s1 = min(n, s0 + slab)
                ys = y[s0:s1] if rows is None else y[rows[s0:s1]]
                yield s0, s1, torch.cat([ys, torch.full((s1 - s0, 1), 254, dtype=torch.uint8, device=dev)], 1)[:, src].contiguous()

        return BifactorCall(st=st, plan=plan, n=n, J=J, KC=KC, Gg=len(theta_np), Gh=len(u_np), theta=theta, logw=logw, u=u, logv=logv,
                            u_np=u_np, logv_np=logv_np, col=col, tl_dev=tl_dev, img=img, fill=fill, slabs=slabs)

    def _bifactor_estep(self, bf, buf):
        """One E-step over a filled BifactorCall into the buffers of _bifactor_buffers: per slab of persons vx_grid_bifactor with
        fws, then vx_grid_bifactor_counts (the first slab writes the tables, the others add to them, in person order); the
        float32 device sum of loglik, as _em_loop takes it, into buf["total"][0]."""
        be, plan = self.be, bf.plan
        for k, (s0, s1, yp) in enumerate(bf.slabs()):
            nb = s1 - s0
            fws = buf["fws"][:be.grid_bifactor_workspace(nb, bf.Gg)]
            ll = buf["loglik"][s0:s1]
            be.grid_bifactor(yp, nb, bf.KC, plan["tl_start"], bf.tl_dev, bf.img, bf.logw, bf.theta, bf.logv, bf.u, ll,
                             buf["mean"][s0:s1], buf["sd"][s0:s1], buf["node"][s0:s1], fws)
            ws = buf["ws"][:be.grid_bifactor_counts_workspace(nb, bf.KC, bf.Gg, len(plan["tl_column"]))]
            be.grid_bifactor_counts(yp, nb, bf.KC, bf.Gg, plan["tl_start"], bf.tl_dev, bf.col, bf.J, bf.img, bf.logv, ll, fws, k > 0,
                                    buf["n1"], buf["n0"], buf["mass"], buf["mass_s"], ws)
        be.sum_into(buf["loglik"], bf.n, 1.0, buf["total"][:1], buf["sum_ws"])

    def _bifactor_buffers(self, bf):
        """Every buffer of _bifactor_estep, made once: sized for the largest slab of persons (the first)."""
        be = self.be
        f32 = dict(dtype=torch.float32, device=self.dev)
        nb, n_tl, GG = min(bf.n, bifactor_slab_persons(bf.KC)), len(bf.plan["tl_column"]), bf.Gg * bf.Gh
        return {"loglik": torch.empty(bf.n, **f32), "mean": torch.empty(bf.n, **f32), "sd": torch.empty(bf.n, **f32),
                "node": torch.empty(bf.n, dtype=torch.int32, device=self.dev),
                "fws": torch.empty(be.grid_bifactor_workspace(nb, bf.Gg), **f32),
                "ws": torch.empty(be.grid_bifactor_counts_workspace(nb, bf.KC, bf.Gg, n_tl), **f32),
                "n1": torch.empty(bf.J, GG, **f32), "n0": torch.empty(bf.J, GG, **f32), "mass": torch.empty(bf.Gg, **f32),
                "mass_s": torch.empty(n_tl, GG, **f32), "total": torch.zeros(2, **f32), "sum_ws": torch.empty(1024, **f32)}

    def expected_counts_bifactor(self, y_u8=None, rows=None, nodes=(41, 21), span=(6.0, 4.0), general=0):
        """The expected-count tables of a bifactor / testlet model (the Bock-Aitkin E-step over the grid of score_bifactor): given
        the general node the posterior of a testlet over (theta_g, u_h) is a two-dimensional table and every item belongs to one
        testlet, so an item's counts live on the Gg x Gh grid of its own testlet whatever x_feature is.  Returns device tensors
        `n1`, `n0` [J][Gg][Gh] = the posterior mass at (general node g, node h of the item's own specific dimension) of the
        persons who answered item j correctly / wrongly (an item that loads on the general dimension alone: post(g) v_h), `prob`
        [J][Gg][Gh] = P(y_j = 1 | theta_g, u_h) as the operand image holds it, `mass` [Gg] the general marginal posterior mass,
        `mass_specific` [S][Gg][Gh] the joint mass of (theta, u_s) by column of specific_dims (a dimension without items: the grid
        prior times `mass`), `loglik` (the float32 device sum of the persons' marginal log-likelihoods) and `theta`, `logw`,
        `u`, `logv`, the axes.  Inputs, limits and refusals as score_bifactor; one rank only.  Deterministic: the same call
        gives the same bits (vx_grid_bifactor_counts)."""
        self._one_rank_only("expected_counts_bifactor over a process group: the tables are the sums over the local shard's "
                            "persons and the cross-rank sum is not built")
        bf = self._bifactor_call(y_u8, rows, nodes, span, general)
        bf.fill()
        buf = self._bifactor_buffers(bf)
        self._bifactor_estep(bf, buf)
        J, Gg, Gh, S, plan = bf.J, bf.Gg, bf.Gh, len(bf.st["specific_dims"]), bf.plan
        # P(y = 1) out of the image: the general node in the place of the node tile, h in the place of the node in it, by slot
        slot = np.empty(J, np.int64)
        slot[plan["col"][plan["col"] >= 0]] = np.flatnonzero(plan["col"] >= 0)
        prob = grid_image_prob(bf.img, 16 * bf.KC, 32 * Gg).view(16 * bf.KC, Gg, 32)[torch.from_numpy(slot).to(self.dev)][:, :, :Gh]
        v = torch.exp(bf.logv.to(torch.float64))
        mass_specific = (buf["mass"].to(torch.float64)[None, :, None] * v[None, None, :]).to(torch.float32).repeat(S, 1, 1)
        real = np.flatnonzero(plan["tl_column"] >= 0)
        if real.size:
            mass_specific[torch.from_numpy(plan["tl_column"][real]).to(self.dev)] = buf["mass_s"].view(-1, Gg, Gh)[
                torch.from_numpy(real).to(self.dev)]
        return {"n1": buf["n1"].view(J, Gg, Gh), "n0": buf["n0"].view(J, Gg, Gh), "prob": prob.contiguous(), "mass": buf["mass"],
                "mass_specific": mass_specific, "loglik": buf["total"][0].clone(), "theta": bf.theta, "logw": bf.logw, "u": bf.u,
                "logv": bf.logv}

    def fit_em_bifactor(self, max_iter=100, tol=1e-6, newton=4, nodes=(41, 21), span=(6.0, 4.0), general=0, prior=None,
                        progress=False):
        """Marginal maximum likelihood of a bifactor / testlet model (bifactor_structure(general)), any x_feature >= 2, by
        Bock-Aitkin EM over the grid of score_bifactor: each iteration tabulates the items as they stand (vx_grid_table_bifactor),
        scores the training responses (vx_grid_bifactor), takes the expected counts of every item on the Gg x Gh grid of its
        own testlet (vx_grid_bifactor_counts) and refits the item to them by `newton` Newton steps of fit_em's M-step with TWO
        dimensions -- the general loading and the item's own specific loading (vx_grid_mstep_irt; with `prior`
        vx_grid_mstep_irt_map) -- so nodes[0] * nodes[1] <= 1024, the M-step's node limit.  Stopping rule, return ({"loglik",
        "iterations", "converged"}, with `prior` also "logpost"), and what is left alone (the guide, Adam's state, the step
        count) as fit_em; loglik[0] is the sum of score_bifactor(nodes=, span=)["loglik"] before the call.  The loadings follow
        the engine's free mask; the specific rows of the other testlets stay 0.
        prior: fit_em's (irt_3pl / irt_4pl need it, with fit_em's rules); a prior on "a" shaped like the leaf is gathered like
        the loadings.  A testlet of ONE item has no identified specific loading: ValueError unless prior["a"] has a finite sd
        on it.  One rank only."""
        self._em_refusals(max_iter, newton)
        st = self.bifactor_structure(general)
        if prior is None and self.model != "irt_2pl":
            raise NotImplementedError("fit_em_bifactor for %s: %s" % (self.model, self._UNPENALISED_ONLY))
        Gg, Gh = (len(v) for v in bifactor_grid(nodes, span)[0::2])
        if Gg * Gh > BIFACTOR_EM_NODES:
            raise ValueError("fit_em_bifactor takes nodes[0] * nodes[1] <= %d, the node limit of the M-step (got %d x %d = %d); "
                             "(41, 21) is the default" % (BIFACTOR_EM_NODES, Gg, Gh, Gg * Gh))
        J, Dm, dev = self.J_items, self.D_model, self.dev
        sd_np, has_np = bifactor_em_index(st)
        pr_np = None if prior is None else bifactor_em_prior(prior, self.model, Dm, J, st["general"], sd_np, has_np)
        for s in np.flatnonzero(st["sizes"] == 1):
            j = int(np.flatnonzero(st["testlet"] == s)[0])
            if pr_np is None or not pr_np[1, 2, j] > 0:
                raise ValueError("dimension %d has ONE item (item %d): a testlet of one item has no identified specific loading -- "
                                 "free the item from it, or pass prior={'a': (mean, sd)} with a finite sd"
                                 % (int(st["specific_dims"][s]), j))
        a = self.unconstrained("a").contiguous().clone()
        b = self.unconstrained("b").reshape(-1).contiguous().clone()
        c = self.unconstrained("c").reshape(-1).contiguous().clone() if self.model in ("irt_3pl", "irt_4pl") else None
        d = self.unconstrained("d").reshape(-1).contiguous().clone() if self.model == "irt_4pl" else None
        sd, has = torch.from_numpy(sd_np).to(dev), torch.from_numpy(has_np).to(dev)
        free2 = bifactor_gather(self.unconstrained("a", self.free).contiguous(), st["general"], sd, has)
        pr = None if pr_np is None else torch.from_numpy(pr_np).to(dev)
        lprior = None if prior is None else torch.zeros(J, dtype=torch.float32, device=dev)
        bf = self._bifactor_call(None, None, nodes, span, general, params=(a, b, c, d))
        buf = self._bifactor_buffers(bf)
        theta2 = torch.stack([bf.theta[:, None].expand(Gg, Gh), bf.u[None, :].expand(Gg, Gh)], 2).reshape(Gg * Gh, 2).contiguous()
        cfg2 = self.be.cfg(self.model, 2, J, 0, self.Dc, 1.0, 0, 0, 0)

        def iteration():
            bf.fill()
            self._bifactor_estep(bf, buf)
            a2 = bifactor_gather(a, st["general"], sd, has)
            if prior is None:
                self.be.grid_mstep_irt(cfg2, theta2, Gg * Gh, buf["n1"], buf["n0"], free2, a2, b, newton)
            else:
                self.be.grid_mstep_irt_map(cfg2, theta2, Gg * Gh, buf["n1"], buf["n0"], free2, a2, b, c, d, pr, newton, lprior)
            bifactor_scatter(a, a2, st["general"], sd, has)

        leaves = {k: v for k, v in (("a", a), ("b", b), ("c", c), ("d", d)) if v is not None}
        return self._em_history(iteration, buf["total"], buf["sum_ws"], leaves, max_iter, tol, progress, lprior)

    def _population_call(self, y_u8, rows, nodes, span, covariates):
        """The GridCall of a conditioned score: the nodes of score() with the log-weights of engine.population's Sigma, the tilt
        Lambda Gamma^T x_i [n][D] float32 by batch position and the prior means Gamma^T x_i."""
        pop = self.population
        if pop is None:
            raise ValueError("covariates need a fitted population: call fit_population() first")
        if isinstance(nodes, (tuple, list)):
            raise ValueError("a conditioned score takes `nodes` points a dimension: the population sets the log-weights")
        call = self._grid_call(y_u8, rows, nodes, span)
        X = self._design(covariates, int(call.y.shape[0]), pop["intercept"], pop["gamma"].shape[0])
        if call.rows is not None:
            X = X[call.rows]
        mu = X @ torch.from_numpy(pop["gamma"]).to(self.dev)
        tilt = (mu @ torch.from_numpy(np.linalg.inv(pop["sigma"])).to(self.dev)).to(torch.float32).contiguous()
        logw = torch.from_numpy(population_logw(call.theta.cpu().numpy(), pop["sigma"])).to(self.dev)
        return call._replace(logw=logw), tilt, mu.to(torch.float32)

    def fit_population(self, covariates, rows=None, max_iter=200, tol=1e-7, intercept=True, nodes=61, span=6.0, progress=False):
        """The latent regression (conditioning model) of the training responses on `covariates` ([training rows][p], float,
        finite; intercept: a column of ones in front): theta_i ~ N(Gamma^T x_i, Sigma), fitted by EM with the item parameters
        fixed as they stand -- each iteration scores the rows under their own priors (vx_grid_posterior_cond) and solves the
        normal equations of the posterior means, Sigma' = the mean of the posterior covariances plus the residuals' cross
        products -- from Gamma = 0, Sigma = I, until the log-likelihood sum_i log p(y_i | x_i) changes by no more than tol times
        its size between two iterations, or for max_iter iterations.  rows: the training rows to fit on (default all).
        Returns {"gamma": float64 numpy [p][D], "sigma": [D][D], "loglik": [floats], "iterations", "converged"}, loglik[k] under
        the parameters iteration k STARTED from (as fit_em reports it), and keeps the result as `engine.population`, which
        score(covariates=...) and plausible_values(covariates=...) condition on.  All four models, x_feature <= 3; one rank.
        Nothing else of the engine changes: the leaves, the guide, Adam's state and the step count stay.
        ValueError: X^T X not positive definite; fewer persons than p + D + 1; a diagonal entry of Sigma below (half the node
        spacing)^2 or a singular Sigma (the grid cannot resolve such a population); max_i |mu_id| + 4 sqrt(Sigma_dd) beyond span (raise span)."""
        self._one_rank_only("fit_population over a process group: the M-step's sums are the local shard's and the cross-rank sum "
                            "is not built")
        self._int_in("max_iter", max_iter, 1)
        if isinstance(nodes, (tuple, list)):
            raise ValueError("fit_population takes `nodes` points a dimension: the population sets the log-weights")
        call = self._grid_call(None, rows, nodes, span)
        X = self._design(covariates, int(call.y.shape[0]), bool(intercept))
        if call.rows is not None:
            X = X[call.rows].contiguous()
        n, p, D = call.n, int(X.shape[1]), call.D
        if n < p + D + 1:
            raise ValueError("fit_population needs at least p + D + 1 = %d persons (got %d)" % (p + D + 1, n))
        out = self._population_em(call, X, design_cholesky(X), 2.0 * float(span) / (int(nodes) - 1), float(span), max_iter,
                                  float(tol), progress)
        self.population = {"gamma": out["gamma"], "sigma": out["sigma"], "intercept": bool(intercept)}
        return out

    def _grid_call(self, y_u8, rows, nodes=61, span=6.0, params=None):
        """The GridCall of score() and its kin.  params: the tensors to tabulate, compact (a [D_model][J_items] or None, b, c_un,
        d_un [J_items] or None) -- by default the leaves as they stand, the problem's own items."""
        if self.D_model > SCORE_MAX_DIMS:
            raise NotImplementedError("grid scores need x_feature <= %d (this model has %d): a tensor-product grid of n nodes "
                                      "a dimension has n**D points" % (SCORE_MAX_DIMS, self.D_model))
        theta_np, logw_np = score_grid(self.D_model, nodes, span)
        J, Dm = self.J_items, self.D_model
        y, rows = self._score_inputs(y_u8, rows, J)
        theta, logw = torch.from_numpy(theta_np).to(self.dev), torch.from_numpy(logw_np).to(self.dev)
        if params is None:
            flat = lambda name: self.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
            params = (self.unconstrained("a").contiguous() if self.model != "irt_1pl" else None, flat("b"),
                      flat("c") if self.model in ("irt_3pl", "irt_4pl") else None, flat("d") if self.model == "irt_4pl" else None)
        cfg = self.be.cfg(self.model, Dm, J, 0, self.Dc, 1.0, 0, 0, 0)
        return GridCall(y, rows, J, theta, logw,
                        lambda img: self.be.grid_table_irt(cfg, theta, int(theta.shape[0]), *params, img), cfg)

    def plausible_values(self, y_u8=None, rows=None, draws=5, seed=0, nodes=61, span=6.0, covariates=None):
        """Plausible values: `draws` independent draws of each scored row's latent from its posterior on the grid of score()
        (the N(0, I) prior times the likelihood under the item parameters as they stand): `theta` float32 (n, draws, D), the
        coordinates of the drawn nodes, and `node` int32 (n, draws).  Inputs, grid and refusals as score().  draws: 1 .. 1024;
        seed: 0 .. 2**64 - 1.  A draw is a function of (seed, row, node, draw index) alone -- the training rows are keyed by
        their global person id, rows of `y_u8` by their index in it -- so more draws extend fewer, `rows` picks the full
        call's rows, and the shards of a process group draw independently.
        The draws sit ON grid nodes: their resolution is the node spacing (2 span / (nodes - 1) a dimension); ask for more
        nodes for finer draws.  They are taken under the item parameters as they stand, as fixed: the uncertainty of the item
        parameters is not in them.
        covariates (as score() takes them): draw under each person's own prior N(Gamma^T x_i, Sigma) of the population
        fit_population() estimated -- the conditioning model a regression of the draws on those covariates needs, without
        which its slopes are attenuated by about the test's reliability.  The noise is keyed as before."""
        draws, seed = self._draw_args(draws, seed)
        if covariates is not None:
            call, tilt, _ = self._population_call(y_u8, rows, nodes, span, covariates)
            node, theta = self._grid_draws_cond(call, tilt, draws, seed, self.gid0 if y_u8 is None else 0)
            return {"theta": theta, "node": node}
        node, theta = self._grid_draws(self._grid_call(y_u8, rows, nodes, span), draws, seed, self.gid0 if y_u8 is None else 0)
        return {"theta": theta, "node": node}

    def expected_counts(self, y_u8=None, rows=None, nodes=61, span=6.0, covariates=None):
        """The expected-count tables of the scored rows over the grid of score() (the Bock-Aitkin E-step): `n1`, `n0` [J][G] =
        the posterior mass at node g of the persons who answered item j correctly / wrongly, `mass` [G] = the posterior mass
        of all scored persons, `prob` [J][G] = P(y_j = 1 | node g) as the tables hold it, `theta` [G][D] and `logw` [G].
        Inputs and refusals as score(); the model's own items only.  Deterministic: the same call gives the same bits.
        covariates (as score() takes them): the tables under each person's own prior N(Gamma^T x_i, Sigma) of the population
        fit_population() estimated (vx_grid_posterior_cond, vx_grid_counts_cond with one segment); `logw` is then that
        population's shared log-weight.  Without them nothing changes, bits included."""
        if covariates is not None:
            call, tilt, _ = self._population_call(y_u8, rows, nodes, span, covariates)
            out = self._grid_counts_cond(call, tilt, np.array([0, call.n], np.int64))
            out["n1"], out["n0"], out["mass"] = out["n1"][0], out["n0"][0], out["mass"][0]
        else:
            call = self._grid_call(y_u8, rows, nodes, span)
            out = self._grid_counts(call)
        out["theta"], out["logw"] = call.theta, call.logw
        return out

    def _group_refusals(self, covariates, impact):
        if impact is not None and not isinstance(impact, (bool, np.bool_)):
            raise ValueError("impact must be True, False or None")
        if covariates is not None and impact:
            raise ValueError("covariates= scores under engine.population as it stands; impact must then be None or False")
        if covariates is not None and self.population is None:
            raise ValueError("covariates need a fitted population: call fit_population() first")

    def _group_prior(self, call, seg_start, covariates, impact, nodes=61, span=6.0):
        """The prior of GridMixin.dif / group_counts for a call whose rows are sorted by group (seg_start): (the call under that
        prior's log-weights, the tilt [n][D] by batch position or None for N(0, I), group_mean [H][D], sigma [D][D])."""
        H, D, n = len(seg_start) - 1, call.D, call.n
        counts = np.diff(seg_start)
        if covariates is not None:
            cond, tilt, mu = self._population_call(call.y, call.rows, nodes, span, covariates)
            mu = mu.cpu().numpy().astype(np.float64)
            return cond, tilt, np.add.reduceat(mu, seg_start[:-1], axis=0) / counts[:, None], np.array(self.population["sigma"])
        if impact is not None and not impact:
            return call, None, np.zeros((H, D)), np.eye(D)
        if isinstance(nodes, (tuple, list)):
            raise ValueError("dif(impact=True) takes `nodes` points a dimension: the fitted population sets the log-weights")
        if n < H + D + 1:
            raise ValueError("dif(impact=True) fits %d group means and Sigma: it needs at least %d persons (got %d)"
                             % (H, H + D + 1, n))
        gidx = torch.from_numpy(np.repeat(np.arange(H), counts)).to(self.dev)
        X = torch.zeros(n, H, dtype=torch.float64, device=self.dev)              # the intercept and a dummy for every label but the first
        X[torch.arange(n, device=self.dev), gidx] = 1.0
        X[:, 0] = 1.0
        fit = self._population_em(call, X, design_cholesky(X), 2.0 * float(span) / (int(nodes) - 1), float(span), 200, 1e-7, False)
        gamma, sigma = fit["gamma"], fit["sigma"]
        group_mean = gamma.copy()
        group_mean[1:] += gamma[0]
        lam = torch.from_numpy(np.linalg.inv(sigma)).to(self.dev)
        tilt = (torch.from_numpy(group_mean).to(self.dev)[gidx] @ lam).to(torch.float32).contiguous()
        logw = torch.from_numpy(population_logw(call.theta.cpu().numpy(), sigma)).to(self.dev)
        return call._replace(logw=logw), tilt, group_mean, sigma

    # what fit_em() without prior= and dif(refit=True) say to irt_3pl / irt_4pl, in the same words
    _UNPENALISED_ONLY = ("with a guessing or slipping asymptote the M-step is not concave and wants priors on the items; only irt_1pl "
                         "and irt_2pl have it without them -- fit_em(prior=...) refits irt_3pl / irt_4pl under item priors "
                         "(dif(refit=True) takes none)")

    def _group_refit_check(self):
        if self.model not in ("irt_1pl", "irt_2pl"):
            raise NotImplementedError("dif(refit=True) for %s: %s" % (self.model, self._UNPENALISED_ONLY))

    def _group_refit(self, call, n1, n0, newton):
        """Every group's items from the pooled values by `newton` steps of vx_grid_mstep_irt on that group's tables."""
        two = self.model != "irt_1pl"
        H = int(n1.shape[0])
        b0 = self.unconstrained("b").reshape(-1).contiguous()
        b_g = b0[None, :].repeat(H, 1)
        a0 = self.unconstrained("a").contiguous() if two else torch.ones(self.D_model, self.J_items, device=self.dev)
        a_g = a0[None].repeat(H, 1, 1)
        free = self.unconstrained("a", self.free).contiguous().clone() if two else None
        for h in range(H):
            self.be.grid_mstep_irt(call.cfg, call.theta, call.G, n1[h], n0[h], free, a_g[h] if two else None, b_g[h], newton)
        b_np = b_g.cpu().numpy().astype(np.float64)
        return {"b_group": b_np, "a_group": a_g.cpu().numpy().astype(np.float64),
                "delta_b": b_np - b0.cpu().numpy().astype(np.float64)[None, :]}

    def fit_em(self, max_iter=100, tol=1e-6, newton=4, progress=False, nodes=61, span=6.0, prior=None):
        """Marginal maximum likelihood of a and b by Bock-Aitkin EM over the grid of score(): each iteration scores the training
        responses under the item parameters as they stand (the E-step: vx_grid_posterior, vx_grid_counts) and refits every
        item to its expected counts by `newton` Newton steps (the M-step: vx_grid_mstep_irt), until the marginal log-likelihood
        rises by no more than tol times its size between two iterations, or for max_iter iterations.  Returns {"loglik":
        [floats], "iterations", "converged"}; loglik[k] is the marginal log-likelihood under the parameters iteration k
        STARTED from (it falls out of the E-step), so loglik[0] is what marginal_loglik() gave before the call.
        No guide is involved and none is changed: the encoder or the per-person rows, Adam's moments and the step count stay as
        they are, and a later fit() goes on from the refitted items.  The loadings follow the engine's own free mask (a_free, or
        the triangular default of x_feature > 1); the phantom items and dimensions of a padded engine are neither read nor
        written.  1PL and 2PL with x_feature <= 3; an item nobody answered keeps its values; an item whose observed answers
        are all equal has no finite maximiser and ends where the clamp of the response function, +-logit(1 - eps32) on z,
        holds at every node -- there the step kernels' `inside` test fails, so a later fit() sees a zero gradient for it.
        prior (Bayes-modal EM; all four models): a dict over "a", "b", "c", "d" of (mean, sd) -- normal priors on the
        UNCONSTRAINED scale of the leaves (c_un = logit c, d_un = logit d), each a scalar or an array shaped like the leaf;
        sd = inf or an absent key: no prior (grid.em_prior checks the argument).  The M-step is then the penalised one of
        vx_grid_mstep_irt_map, for 1PL and 2PL too, and c / d are refitted with a and b.  irt_3pl needs a finite sd on "c" and
        irt_4pl on "c" and "d": the likelihood alone does not pin an asymptote.  The return gains "logpost": logpost[k] =
        loglik[k] + the log prior (constants dropped) at the parameters iteration k started from, and convergence is judged
        on it -- the quantity this EM raises; loglik[0] is still marginal_loglik() before the call.  Without `prior` nothing
        changes: 1PL / 2PL take vx_grid_mstep_irt, and irt_3pl / irt_4pl refuse."""
        self._em_refusals(max_iter, newton)
        if prior is None and self.model not in ("irt_1pl", "irt_2pl"):
            raise NotImplementedError("fit_em for %s: %s" % (self.model, self._UNPENALISED_ONLY))
        if self.D_model > SCORE_MAX_DIMS:
            raise NotImplementedError("fit_em needs x_feature <= %d (this model has %d): a tensor-product grid of n nodes a "
                                      "dimension has n**D points" % (SCORE_MAX_DIMS, self.D_model))
        # compact copies ([D_model][J_items], [J_items]) the tables and the M-step work on: the leaves may be strided views
        two = self.model != "irt_1pl"
        a = self.unconstrained("a").contiguous().clone() if two else None
        free = self.unconstrained("a", self.free).contiguous().clone() if two else None
        b = self.unconstrained("b").reshape(-1).contiguous().clone()
        pr = None if prior is None else torch.from_numpy(em_prior(prior, self.model, self.D_model, self.J_items)).to(self.dev)
        c = self.unconstrained("c").reshape(-1).contiguous().clone() if self.model in ("irt_3pl", "irt_4pl") else None
        d = self.unconstrained("d").reshape(-1).contiguous().clone() if self.model == "irt_4pl" else None
        lprior = None if prior is None else torch.zeros(self.J_items, dtype=torch.float32, device=self.dev)
        call = self._grid_call(None, None, nodes, span, params=(a, b, c, d))
        if prior is None:
            mstep = lambda n1, n0: self.be.grid_mstep_irt(call.cfg, call.theta, call.G, n1, n0, free, a, b, newton)
        else:
            mstep = lambda n1, n0: self.be.grid_mstep_irt_map(call.cfg, call.theta, call.G, n1, n0, free, a, b, c, d, pr, newton,
                                                              lprior)
        leaves = {k: v for k, v in (("a", a), ("b", b), ("c", c), ("d", d)) if v is not None}
        return self._em_loop(call, mstep, leaves, max_iter, tol, progress, lprior=lprior)

    def _info_call(self, y_u8, rows, nodes=61, span=6.0, prior=None):
        """What GridMixin.item_information needs of this class: the GridCall, K (columns an item: b, then a_0 .. a_{D-1}; 1PL: b),
        the filler of the derivative tables and the free mask over the dense layout.  With `prior` (fit_em's, checked here by
        grid.em_prior before anything is computed) all four models are served: c_un (3PL up) and d_un (4PL) follow the loadings,
        K = D + 2 / D + 3, both always free, and the filler is vx_grid_wtable_irt_map on compact copies of the leaves."""
        if prior is None and self.model not in ("irt_1pl", "irt_2pl"):
            raise NotImplementedError("item_information / item_se for %s: the derivative tables are those of the logistic link of "
                                      "fit_em's M-step, which a guessing or slipping asymptote does not have; only irt_1pl and "
                                      "irt_2pl have them without item priors -- pass prior= (fit_em's) for the matrix at the "
                                      "Bayes-modal fit" % self.model)
        if prior is not None and self.D_model <= SCORE_MAX_DIMS:
            em_prior(prior, self.model, self.D_model, self.J_items)          # (beyond three dimensions _grid_call refuses)
        call = self._grid_call(y_u8, rows, nodes, span)
        two = self.model != "irt_1pl"
        extra = 0 if prior is None else {"irt_3pl": 1, "irt_4pl": 2}.get(self.model, 0)
        K = (self.D_model + 1 if two else 1) + extra
        a = self.unconstrained("a").contiguous() if two else None
        b = self.unconstrained("b").reshape(-1).contiguous()
        free = torch.ones(self.J_items, K, dtype=torch.bool, device=self.dev)
        if two:
            free[:, 1:1 + self.D_model] = (self.unconstrained("a", self.free) != 0).t()
        if prior is None:
            return call, K, lambda wimg: self.be.grid_wtable_irt(call.cfg, call.theta, call.G, a, b, wimg), free.reshape(-1)
        c = self.unconstrained("c").reshape(-1).contiguous() if extra >= 1 else None
        d = self.unconstrained("d").reshape(-1).contiguous() if extra == 2 else None
        return call, K, lambda wimg: self.be.grid_wtable_irt_map(call.cfg, call.theta, call.G, a, b, c, d, wimg), free.reshape(-1)

    def _info_prior(self, prior, free):
        """The prior's share of item_information(prior=) over the dense layout of _info_call, float64 numpy [P]: the precisions
        1 / sd^2 as grid.em_prior gives them and the gradient of the log prior, -precision (p - mean), at the leaves as they
        stand; both zero where the unknown is not free (free: bool [P]) or has no prior."""
        J, D = self.J_items, self.D_model
        pr = em_prior(prior, self.model, D, J).astype(np.float64)
        rows, leaves = [0], [self.unconstrained("b").reshape(1, J)]
        if self.model != "irt_1pl":
            rows += list(range(1, 1 + D))
            leaves.append(self.unconstrained("a").reshape(D, J))
        if self.model in ("irt_3pl", "irt_4pl"):
            rows.append(4)
            leaves.append(self.unconstrained("c").reshape(1, J))
        if self.model == "irt_4pl":
            rows.append(5)
            leaves.append(self.unconstrained("d").reshape(1, J))
        p = torch.cat(leaves, 0).detach().cpu().numpy().astype(np.float64)      # [K][J]
        prec = np.where(np.asarray(free, bool).reshape(J, len(rows)), pr[1, rows].T, 0.0)
        grad = -prec * (p.T - pr[0, rows].T)
        return prec.reshape(-1), grad.reshape(-1)

    def _pairs_call(self, y_u8, rows, nodes=61, span=6.0):
        """What GridMixin.residual_sums needs of this class: the GridCall (all four models; x_feature > 3 is refused with the
        wording of score()), the name under which the point estimate is returned, its key in _grid_posterior's output, and the
        pairs call over compact copies of the engine's own items, as _grid_call makes them."""
        call = self._grid_call(y_u8, rows, nodes, span)
        flat = lambda name: self.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
        params = (self.unconstrained("a").contiguous() if self.model != "irt_1pl" else None, flat("b"),
                  flat("c") if self.model in ("irt_3pl", "irt_4pl") else None, flat("d") if self.model == "irt_4pl" else None)
        return call, "theta_hat", "mean", lambda est, t, ws, ws_floats: self.be.grid_pairs_irt(
            call.cfg, call.y, call.rows, call.n, est, *params, t["n"], t["s"], t["ss"], t["sp"], ws, ws_floats)

    def _fit_call(self, y_u8, rows, nodes=61, span=6.0):
        """What GridMixin.fit_sums needs of this class, shaped like _pairs_call: the GridCall (all four models; x_feature > 3 is
        refused with the wording of score()), the name and the key of the point estimate, and the fit call over compact copies of
        the engine's own items."""
        call = self._grid_call(y_u8, rows, nodes, span)
        flat = lambda name: self.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
        params = (self.unconstrained("a").contiguous() if self.model != "irt_1pl" else None, flat("b"),
                  flat("c") if self.model in ("irt_3pl", "irt_4pl") else None, flat("d") if self.model == "irt_4pl" else None)
        return call, "theta_hat", "mean", lambda est, person, item, ws, ws_floats: self.be.grid_fit_irt(
            call.cfg, call.y, call.rows, call.n, est, *params, person, item, ws, ws_floats)

    def _point_refusals(self, method):
        """wle beyond one dimension (x_feature > 3 is left to _grid_call, which refuses in the words of score())."""
        if method == "wle" and 1 < self.D_model <= SCORE_MAX_DIMS:
            raise NotImplementedError("the weighted likelihood estimate ('wle') needs x_feature = 1 (this model has %d): the "
                                      "multidimensional Firth term needs M^-1 inside the item sum; it is not built -- 'ml' and "
                                      "'map' serve x_feature <= %d" % (self.D_model, SCORE_MAX_DIMS))

    def _point_run(self, call, theta0, method, max_iter=32, tol=1e-6, bound=None):
        """vx_grid_point_irt over a call, from theta0 [n][D] (float32 on the device), on compact copies of the engine's own items
        as _fit_call makes them and in buffers of its own: device tensors `theta_hat` (n, D), `info` [D (D + 1) / 2][n], `status`
        and `iters` (n,) int32.  bound None: the reach of the call's nodes."""
        n, D = call.n, call.D
        if bound is None:
            bound = float(call.theta.abs().max())
        flat = lambda name: self.unconstrained(name).reshape(-1).contiguous()      # noqa: E731
        params = (self.unconstrained("a").contiguous() if self.model != "irt_1pl" else None, flat("b"),
                  flat("c") if self.model in ("irt_3pl", "irt_4pl") else None, flat("d") if self.model == "irt_4pl" else None)
        out = {"theta_hat": torch.empty(n, D, dtype=torch.float32, device=self.dev),
               "info": torch.empty(D * (D + 1) // 2, n, dtype=torch.float32, device=self.dev),
               "status": torch.empty(n, dtype=torch.int32, device=self.dev), "iters": torch.empty(n, dtype=torch.int32, device=self.dev)}
        self.be.grid_point_irt(call.cfg, call.y, call.rows, n, theta0.contiguous(), *params, POINT_METHODS[method], max_iter, tol, bound,
                               POINT_STEP_CAP, out["theta_hat"], out["info"], out["status"], out["iters"])
        return out

    def point_estimates(self, y_u8=None, rows=None, method="wle", max_iter=32, tol=1e-6, bound=None, nodes=61, span=6.0,
                        covariates=None):
        """Likelihood-based person scores: for each scored row the estimate `theta_hat` (n, D) that Fisher scoring reaches from
        the grid EAP of score(), over the items the person answered and under the item parameters as they stand
        (vx_grid_point_irt) -- method "ml", the maximum of the likelihood; "map", of the likelihood times the N(0, I) prior of
        score(); "wle" (x_feature = 1), Warm's weighted likelihood estimate, the score PISA, TIMSS, ConQuest and TAM report
        (for 1PL / 2PL Firth's penalised score) -- with its standard error.  Unlike the EAP it is not shrunk towards the prior
        mean (ml, wle) and not tied to the node spacing.  A step is capped at 1 a coordinate and theta is kept in [-bound,
        bound] (bound None: span); a person stops when the step falls to tol or below.
        Returns numpy: `theta_hat` float32 (n, D); `info` float64 (n, D, D), the likelihood's expected information at
        theta_hat (without the prior, for every method); `cov` = M^-1 with M = info (+ I for "map") and `se` (n, D) = the square
        roots of its diagonal, inverted in float64; `status` int32 (n,) -- POINT_STATUS names the codes: 0 converged, 1 at_bound
        (the ML estimate of an all-correct or all-wrong row lies beyond the bound: theta_hat sits on it, se is the finite value
        there), 2 max_iter, 3 singular, 4 empty (the person answered nothing: theta_hat NaN) --; `iterations` (n,), the
        evaluations taken; `n_converged`; and `reliability` (D,) = 1 - mean(se^2) / var(theta_hat) over the converged persons, the
        person separation reliability of a TAM / ConQuest report (NaN with fewer than two).  se and cov are NaN where status is
        empty or singular.  Inputs, data contract, grid and refusals as score(); with a process group this rank's shard.  Works
        in buffers of its own: nothing of the engine changes.  Deterministic: the same call gives the same bits, and a
        person's result does not depend on the persons scored beside it.
        Not built: "wle" with x_feature > 1 (the multidimensional Firth term needs M^-1 inside the item sum), covariates=
        (a MAP under the population of fit_population), Snijders' correction, observed-information standard errors."""
        if method not in POINT_METHODS:
            raise ValueError("method must be one of %s (got %r)" % (", ".join(repr(k) for k in sorted(POINT_METHODS)), method))
        max_iter = self._int_in("max_iter", max_iter, 1, POINT_MAX_ITERS)
        for name, v in (("tol", tol), ("bound", span if bound is None else bound)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v) or not v > 0:
                raise ValueError("%s must be a positive finite number" % name)
        if covariates is not None:
            raise NotImplementedError("point_estimates with covariates=: the estimates are taken under the likelihood alone (ml, "
                                      "wle) or the N(0, I) prior of score() (map); a MAP under the population of "
                                      "fit_population() is not built")
        self._point_refusals(method)
        call = self._grid_call(y_u8, rows, nodes, span)
        theta0 = self._grid_posterior(call)["mean"]
        pt = self._point_run(call, theta0, method, max_iter, float(tol), float(span if bound is None else bound))
        return point_estimates_host(pt["theta_hat"].cpu().numpy(), pt["info"].cpu().numpy(), pt["status"].cpu().numpy(),
                                    pt["iters"].cpu().numpy(), method)

    def _sx2_params(self, items):
        """The free parameters of each listed item, for the df of GridMixin.sx2: b; for 2PL and up the item's free loadings; the
        lower asymptote of 3PL / 4PL and the upper one of 4PL."""
        k = np.ones(len(items), np.int64)
        if self.model != "irt_1pl":
            free = self.unconstrained("a", self.free).reshape(self.D_model, -1).cpu().numpy()
            k += (free[:, items] != 0).sum(0)
        return k + {"irt_3pl": 1, "irt_4pl": 2}.get(self.model, 0)

    @staticmethod
    def _score_table_leaves(out):
        return out

    def _se_leaves(self, se):
        """Dense [P] -> the leaves' shapes: b (1, J) and, for 2PL up, a (D, J).  The layout of item_se(prior=) for irt_3pl /
        irt_4pl (K = D + 2 / D + 3) also has c_un (and d_un) (1, J) and, by the delta method, c (and d) on the probability scale:
        se x (1 - x), x the asymptote as the tables cap it."""
        se = se.reshape(self.J_items, -1)
        D = self.D_model
        out = {"b": se[:, 0].reshape(1, -1).copy()}
        if self.model != "irt_1pl":
            out["a"] = se[:, 1:1 + D].T.copy()
        eps = float(np.finfo(np.float32).eps)
        for n, k in enumerate(("c", "d")[:max(se.shape[1] - (D + 1), 0)]):
            un = self.unconstrained(k).detach().cpu().numpy().astype(np.float64).reshape(1, -1)
            x, om = np.minimum(1.0 / (1.0 + np.exp(-un)), 1.0 - eps), np.maximum(1.0 / (1.0 + np.exp(un)), eps)
            out[k + "_un"] = se[:, D + 1 + n].reshape(1, -1).copy()
            out[k] = out[k + "_un"] * x * om
        return out

    # -- one ELBO-gradient step ------------------------------------------------------------------
    def loss_and_grads(self, rows=None, b_global=None, eps=None, stream_id=0, baseline_buf=None, guide_grads=True):
        """Fills self.G (flat grads + loss slot) and per-person grads for ONE particle.
        rows: int64 device tensor of LOCAL row indices (None = all local rows, i.e. full batch).
        baseline_buf / guide_grads: the 'loo' mode of the score-function estimator (step())."""
        nb, scale, sdc = self._call(rows, b_global)       # (sdc: a captured step's count lives in device memory)
        model = self.model
        getattr(self, self._guide_pass)(SimpleNamespace(                 # what every pass starts from
            rows=rows, eps=eps, stream_id=stream_id, score=(baseline_buf, guide_grads), nb=nb, scale=scale, sdc=sdc,
            cfg=self.be.cfg(model, self.D, self.J, self.H, self.Dc, scale, self.seed, self.t, stream_id, **sdc),
            items=(self.view("a") if model != "irt_1pl" else None, self.view("b"),              # a, b, c_un, d_un
                   self.view("c") if model in ("irt_3pl", "irt_4pl") else None, self.view("d") if model == "irt_4pl" else None),
            gitem=self.G[:self.n_item], lossslot=self.G[self.n_params:self.n_params + 1]))

    def _pass_mvn_pp(self, c):
        """The per-person multivariate guide (VIRT, x_feature > 1): forward, likelihood, [score operands,] backward, loss."""
        be, cfg, rows, nb = self.be, c.cfg, c.rows, c.nb
        D, n, score = self.D, self.n_local, self.estimator == "score"
        fw = {"x": self._buf("x", nb * D), "eps": self._buf("eps", nb * D), "ent": self._buf("ent", nb)}
        gx, ll = self._buf("gx", nb * D), self._buf("ll", nb)
        lik_ws = self._buf("lik_ws", be.lik_workspace(cfg, nb))
        loc = self.PP[:n * D]
        if self.share_cov:
            Mq, gM = self.view("x_scale"), self.view("x_scale", self.G)
        else:
            Mq, gM = self.PP[n * D:], self.GP[n * D:]
        with self._phase("guide_forward"):
            be.mvn_bbvi_forward(cfg, nb, rows, self.gid0, loc, Mq, self.share_cov, c.eps, fw["x"], fw["eps"], fw["ent"])
        with self._phase("likelihood"):
            be.lik_grad(cfg, self.y, rows, nb, fw["x"], *c.items, gx, ll, c.gitem, lik_ws)
        cfg_b = cfg
        if score:
            # the guide's score-function gradient in place of the pathwise one: gx <- w_i L_i^-T eps_i, and the diagonal
            # term -w_i in place of the entropy's +scale (k_mvn_score.hip); item gradients and loss stand
            with self._phase("mvn_score"):
                w_sf = self._buf("sf_w", nb)
                log_r, base, beta, by_row = self._score_pass("sf_lr", nb, c.stream_id, *c.score)
                be.mvn_score_operands(cfg, nb, rows, 2 if self.share_cov else 1, None, None, None, Mq, fw["eps"], ll,
                                      fw["ent"], base, beta, by_row, log_r, w_sf, gx, None, None)
            cfg_b = be.cfg(self.model, self.D, self.J, self.H, self.Dc, 0.0, self.seed, self.t, c.stream_id)
        with self._phase("guide_backward"):
            self.GP.zero_()                                       # dense per-person grads: zero off the batch
            if self.share_cov:
                gM.zero_()
            be.mvn_bbvi_backward(cfg_b, nb, rows, Mq, self.share_cov, gx, fw["eps"], self.GP[:n * D], gM,
                                 self._buf("bbvi_ws", be.mvn_bbvi_bwd_workspace(cfg, nb, self.share_cov)))
            if score:
                be.mvn_score_diag(cfg, nb, rows, w_sf, self.share_cov, gM)
        be.sum2_into(ll, fw["ent"], nb, -c.scale, c.lossslot, self.sum_ws, **c.sdc)   # loss = -scale * sum_i (ll_i + ent_i)
        self.last = {"fw": fw, "gx": gx, "ll": ll, "nb": nb}

    def _pass_mvn_enc(self, c):
        """The amortized multivariate guide (VaeIRT, x_feature > 1: the headline workload), a function a stage."""
        p = self._mvn_enc_plan(c)
        keep = self._mvn_enc_forward(c, p)
        self._mvn_enc_likelihood(c, p, keep)
        if self.estimator == "score":
            self._mvn_enc_score(c, p)
        self._mvn_enc_backward(c, p)
        self.last = {"fw": p.fw, "gx": p.gx, "gxT": p.gxT, "ll": p.ll, "nb": p.nb, "n_valid": p.n_valid - p.phantom_rows}

    def _mvn_enc_plan(self, c):
        """Everything the call decides, before its first launch: the persons it is launched over (nb, n_valid of them the
        batch's own), the copies of the responses the guide (y_k) and the likelihood (y_l) read, the buffers, whether the shape
        has a person-major gx, a gdT, operand maxima (opmax), forward-written bf16 terms of hT (fw["hs"]) -- and the refusal."""
        be, cfg, rows, eps, nb, D, H = self.be, c.cfg, c.rows, c.eps, c.nb, self.D, self.H
        if eps is not None and D != self.D_model:      # a caller's draws are the model's: the phantom dimensions draw zero
            eps = _grown(eps.reshape(nb, self.D_model).to(device=self.dev, dtype=torch.float32), (nb, D))
        phantom_rows = self._phantom_rows if rows is not None else 0
        # rows of a padded subsample may point at the phantom person behind the shard's own (_pad_batch)
        ext = rows is not None and self._y_ext is not None
        y_k, y_l = (self._y_ext, self._y_ext_lik) if ext else (self.y, self.y_lik if self.y_lik is not None else self.y)
        if phantom_rows and not (ext and self._dim_major(cfg, nb)):
            # the phantoms leave the step as columns of gxT / gdT: a launch without those operands would carry their
            # entropy and prior into the loss and their gradients into the encoder's
            raise RuntimeError("a subsample padded with %d phantom rows cannot be launched over %d rows of %s, D = %d, "
                               "J = %d, H = %d: the dimension-major backward kernels do not take this shape"
                               % (phantom_rows, nb, self.model, self.D, self.J, self.H))
        n_valid = nb
        if rows is None and eps is None:
            self._n_pad = nb = n_valid + self._pad_persons(rows, eps, cfg)
            if nb != n_valid:                          # phantom persons up to a multiple of 8
                y_k, y_l = self._padded_y(), self._padded_y(lik=True)
        fw = {"h": self._buf("h", nb * H), "x": self._buf("x", nb * D), "eps": self._buf("eps", nb * D),
              "ldT": self._buf("ldT", nb * D), "ent": self._buf("ent", nb)}
        fw["packws"] = self._buf("packws", be.mvn_pack_floats(cfg))
        # dimension-major copies (person-contiguous rows) for the DMA-staged weight-gradient kernel
        fw["hT"], fw["epsT"] = self._buf("hT", nb * H), self._buf("epsT", nb * D)
        gxT = self._buf("gxT", nb * D)
        yT = self._item_major_y(rows)
        if yT is not None:
            fw["yT"] = yT
            n_img = be.lik_ximg_bytes(cfg, nb)        # x once more as the likelihood kernel's operand image
            if n_img > 0:
                fw["ximg"] = self._buf("ximg", (n_img + 3) // 4)
        gx, ll = self._buf("gx", nb * D), self._buf("ll", nb)
        if be.mvn_enc_bwd_layout(cfg, nb) == 1:
            gx = None                                  # the backward kernels read gxT only
        lik_ws = self._buf("lik_ws", be.lik_workspace(cfg, nb))
        encb_ws = self._buf("encb_ws", be.mvn_enc_bwd_workspace(cfg, nb))
        hs_off = be.mvn_enc_bwd_hs_offset(cfg, nb)     # the weight-gradient kernel's bf16 terms of hT, written by the forward
        if hs_off >= 0:
            fw["hs"] = encb_ws[hs_off:hs_off + nb * 64]
        gd_off = be.mvn_enc_bwd_gd_offset(cfg, nb)     # the backward's DIAG-row operand, made in the likelihood's last pass
        gdT = encb_ws[gd_off:gd_off + nb * D] if gd_off >= 0 else None
        # the step's largest |gx|, |gd|, |eps| (the head weight gradient's power of two), collected by the likelihood's last
        # pass into words of packws that the forward call cleared -- unless the score-function mode replaces gxT / gdT
        opmax = None
        if gdT is not None and self.estimator == "pathwise" and self._hip:
            om = be.mvn_pack_opmax_offset(cfg, nb)
            if om >= 0:
                opmax = fw["packws"][om:om + 3]
        return SimpleNamespace(nb=nb, n_valid=n_valid, phantom_rows=phantom_rows, ext=ext, eps=eps, y_k=y_k, y_l=y_l, fw=fw,
                               enc=self._enc(), gx=gx, gxT=gxT, gdT=gdT, ll=ll, yT=yT, opmax=opmax, lik_ws=lik_ws, encb_ws=encb_ws,
                               lik_hip={"opmax": opmax} if self._hip else {})     # (the other backends' lik_grad is narrower)

    def _mvn_enc_forward(self, c, p):
        """The forward call; returns `keep`: 0 for the phantom rows of a padded subsample, 1 for the others (or None)."""
        with self._phase("guide_forward"):
            cfg_f = c.cfg
            ring = self._capture_ring
            if ring is not None and c.rows is not None and self._step_dev is not None and self._hip:
                # a captured subsampled step: the forward call's first launch fetches the step's draw from the pinned
                # host ring (vx_irt_cfg.rows_ring) -- no copy in front of every replay
                cfg_f = self.be.cfg(self.model, self.D, self.J, self.H, self.Dc, c.scale, self.seed, self.t, c.stream_id,
                                    step_dev=self._step_dev, rows_ring=ring)
                self._capture_ring_used = True
            self.be.mvn_enc_forward(cfg_f, p.y_k, c.rows, p.nb, self.gid0, p.enc, p.eps, p.fw)
        # behind the forward call: in a captured step `rows` holds this step's draw only once the forward's first launch has
        # fetched it from the ring (in front of it: the draw of the step before)
        return (c.rows != self.n_local).to(torch.float32) if p.ext else None

    def _mvn_enc_likelihood(self, c, p, keep):
        """The likelihood call and, behind it, the phantoms taken out: nothing later in the step sees them but as zeros."""
        fw, dm = p.fw, p.gdT is not None
        with self._phase("likelihood"):
            self.be.lik_grad(c.cfg, p.y_l, c.rows, p.nb, fw["x"], *c.items, p.gx, p.ll, c.gitem, p.lik_ws,
                             gxT=p.gxT, yT=p.yT, ximg=fw.get("ximg"), epsT=fw["epsT"] if dm else None,
                             ldT=fw["ldT"] if dm else None, gdT=p.gdT, **p.lik_hip)
            # (a padded subsample's rows without phantoms on a shape that has no gdT pass by: nothing to take out; rows WITH
            # phantoms on such a shape were refused by the plan)
            n_valid = p.n_valid if p.nb != p.n_valid else None
            keep = keep if (dm and p.gx is None) else None
            if n_valid is not None or keep is not None:
                self._take_out_phantoms(self.D, p.nb, p.gxT, p.gdT, p.ll, fw["ent"], n_valid, keep)

    def _mvn_enc_score(self, c, p):
        """gxT, gdT <- the score-function operands (k_mvn_score.hip); item gradients and loss stand."""
        be, cfg, fw, nb, W22, b22 = self.be, c.cfg, p.fw, p.nb, p.enc["fc22.weight"], p.enc["fc22.bias"]
        if p.gx is not None or p.gdT is None:
            raise NotImplementedError("the score-function estimator of the amortized multivariate guide runs on the "
                                      "dimension-major backward kernels: hidden_dim 64, x_feature % 4 == 0 (<= 124), "
                                      "item_size % 4 == 0, batch % 4 == 0")
        with self._phase("mvn_score"):
            log_r, base, beta, by_row = self._score_pass("sf_lr", nb, c.stream_id, *c.score)
            n_sh = be.mvn_score_heads_workspace(cfg) if (self._hip and self.score_mfma) else -1
            if n_sh > 0:
                # u = L^-T eps on the fp16 MFMA, the head rows in column order (k_mvn_score_b.hip)
                be.mvn_score_heads(cfg, nb, c.rows, fw["h"], W22, b22, fw["packws"], fw["eps"], p.ll, fw["ent"], base, beta,
                                   by_row, log_r, p.gxT, p.gdT, self._buf("score_img", n_sh))
            else:
                be.mvn_score_operands(cfg, nb, c.rows, 0, fw["h"], W22, b22, None, fw["eps"], p.ll, fw["ent"], base, beta,
                                      by_row, log_r, None, None, p.gxT, p.gdT)

    def _mvn_enc_backward(self, c, p):
        """The backward call and the loss = -scale * sum_i (ll_i + ent_i): on the HIP backend from the call's last launch -- a
        captured step's counter advances there, behind every kernel that read it."""
        loss = (p.ll, p.fw["ent"], -c.scale, c.lossslot, self.sum_ws)
        hip = {"opmax_ready": p.opmax is not None, "loss": loss} if self._hip else {}     # (the other backends' calls are narrower)
        with self._phase("guide_backward"):
            self.be.mvn_enc_backward(c.cfg, p.y_k, c.rows, p.nb, p.enc, p.fw, p.gx,
                                     self.G[self.enc_off0:self.enc_off0 + self.n_enc], p.encb_ws, gxT=p.gxT,
                                     gd_ready=p.gdT is not None, **hip)
        if not self._hip:
            self.be.sum2_into(p.ll, p.fw["ent"], p.nb, -c.scale, c.lossslot, self.sum_ws, **c.sdc)
        self._zero_phantom_head_grads()

    def _pass_1d(self, c):
        """x_feature == 1, per-person guide (VIRT) or NormEncoder (VaeIRT) in front of the one step kernel.  The flat item
        layout [a: J | b: J | c: J | d: J] IS the kernel's gradient layout: written in place."""
        be, cfg, rows, eps, nb = self.be, c.cfg, c.rows, c.eps, c.nb
        i1d_ws = self._buf("i1d_ws", be.irt1d_workspace(cfg, nb))
        elbo = self._buf("elbo", nb)
        if self.amortized:
            # phantom persons for the ENCODER's kernels only: the step kernel runs over the shard's own, and their entries of
            # gloc / graw -- all the encoder's backward sees of a person -- are zeroed in front of it
            nb_e, y_e = nb + self._pad_persons(rows, eps), self.y
            if nb_e != nb:
                self._n_pad = nb_e
                y_e = self._padded_y()
            ne = self._norm_enc_forward(cfg, y_e, rows, nb_e)
            loc, raw, gloc, graw = ne.fw["loc"], ne.fw["raw"], ne.gloc, ne.graw
        else:
            loc, raw, gloc, graw = self._gather_pp(rows, nb)
        lists = self._sparse_lists(rows)
        with self._phase("irt1d"):
            if lists is not None:                      # mostly-missing responses: observed cells only
                sp_ws = self._buf("i1d_sp_ws", be.irt1d_sparse_workspace(cfg, lists["n_groups"]))
                be.irt1d_sparse_grad(cfg, lists, self.gid0, loc, raw, eps, *c.items,
                                     gloc, graw, elbo, c.gitem, sp_ws, loss=c.lossslot, **c.sdc, **self._take_fused_tail())
            else:
                be.irt1d_grad(cfg, self.y_lik if self.y_lik is not None else self.y, rows, nb, self.gid0, loc, raw, eps,
                              *c.items, gloc, graw, elbo, c.gitem, i1d_ws, loss=c.lossslot, **c.sdc,
                              **self._take_fused_tail())
        if self.estimator == "score":
            # score-function gradient of the guide in place of the pathwise one (the step kernel's item gradients and
            # loss stand); the draws are the step's own Philox normals, keyed by the global person id
            with self._phase("irt1d_score"):
                if eps is None:
                    eps = self._buf("sf_eps", nb)
                    be.philox_normals(eps, None if rows is None else (rows + self.gid0), self.gid0, nb, 1, self.seed, self.t,
                                      c.stream_id)
                log_r, base, beta, by_row = self._score_pass("sf_lr", nb, c.stream_id, *c.score)
                be.irt1d_score_grad(nb, c.scale, elbo, eps, raw, rows, base, beta, by_row, log_r, gloc, graw)
        if self.amortized:
            with self._phase("guide_backward"):
                if nb_e != nb:
                    gloc[nb:nb_e].zero_()
                    graw[nb:nb_e].zero_()
                self._norm_enc_backward(ne, self._item_major_y(rows))
                self._zero_phantom_head_grads()
        else:
            self._scatter_pp(rows, nb, gloc, graw)
        self.last = {"elbo": elbo, "nb": nb}                # the loss itself came out of the kernel's reduction


class HoDinaEngine(_EngineBase):
    """HO-DINA ELBO-gradient step with exact enumeration (VCHoDina / VaeCHoDina, vi.py:894-981).

    Flat parameter buffer: [g_un: J | s_un: J | lam0: K | lam1_un: K | encoder (amortized only)];
    per-person rows theta_local / log theta_scale for the BBVI guide (vi.py:928-929)."""

    pp_names = ("theta_local", "theta_scale")

    def __init__(self, y_u8, q, n_global=None, gid0=0, amortized=False, H=64, encoder_init=None, seed=1234,
                 group=None, backend=None):
        self._preamble(y_u8, backend, n_global, gid0, seed, group)
        self._q_matrix(q, "the subset test of vi.py:78-81 assumes it")
        self.amortized, self.H = bool(amortized), int(H) if amortized else 0
        # The amortized guide's ENCODER on the MFMA kernels whatever the item count and width (the reference's HO-DINA has 30
        # items: its full-batch step took 0.81 ms at 200 k persons where 32 items take 0.24, tools/hodina_cliffs.py): the
        # encoder and the HO-DINA kernel are separate calls with separate configurations, so only the ENCODER sees phantom
        # items (J_enc, a copy of the responses with zero columns behind) and phantom hidden units (zero fc1 rows, zero head
        # columns whose gradients are zeroed behind the backward call: softplus(0) = log 2) -- IrtEngine._decide_shapes has the
        # argument; the HO-DINA kernel keeps the problem's own items and responses.
        self.H_model, self.J_enc, self.y_enc = self.H, self.J, self.y
        if self.amortized and self._hip and self.pad_encoder:
            if 0 < self.H < 64:
                self.H = 64
            if self.H == 64 and self.J % 4 != 0:
                self.J_enc = (self.J + 3) // 4 * 4
                self.y_enc = torch.cat([self.y, torch.zeros((self.n_local, self.J_enc - self.J), dtype=torch.uint8,
                                                            device=self.dev)], 1).contiguous()
        J, K = self.J, self.K
        self.off = {"g": 0, "s": J, "lam0": 2 * J, "lam1": 2 * J + K}
        self.shape = {"g": (1, J), "s": (1, J), "lam0": (1, K), "lam1": (1, K)}
        self.n_item = 2 * J + 2 * K
        o = self.n_item
        if self.amortized:
            o = self._encoder_segments({"fc1.weight": (self.H, self.J_enc), "fc1.bias": (self.H,), "fc21.weight": (1, self.H),
                                        "fc21.bias": (1,), "fc22.weight": (1, self.H), "fc22.bias": (1,)})
        self._alloc(o, self.n_local, per_person=not self.amortized)
        self._yT_enc = None
        # vi.py:901-904: lam0 = 0, lam1 = 1 (positive -> log 1 = 0), g = s = 0.1 (interval(0,1) -> logit)
        self._init_g_s()
        if self.amortized:
            self._fill_encoder(default_encoder_init(J, 1, self.H_model, seed) if encoder_init is None else encoder_init,
                               J, self.H_model)

    pad_encoder = os.environ.get("VX_PAD_ENCODER", "1") != "0"      # test seam: 0 = the encoder in the problem's own shape

    def unconstrained(self, name, buf=None):
        u = super().unconstrained(name, buf)
        if self.amortized and name.startswith("encoder$$$"):       # (phantom items / hidden units are nobody's business)
            if name == "encoder$$$fc1.weight":
                u = u[:self.H_model, :self.J]
            elif name == "encoder$$$fc1.bias":
                u = u[:self.H_model]
            elif name.endswith("weight"):
                u = u[:, :self.H_model]
        return u

    def _item_major_y_enc(self, rows):
        """The encoder's item-major responses (_item_major_y over the encoder's copy: phantom item rows hold byte 0)."""
        return self._item_major_y(rows) if self.J_enc == self.J else self._item_major_y(rows, "_yT_enc", self.y_enc)

    def names(self):
        out = ["g", "s", "lam0", "lam1"]
        if self.amortized:
            out += ["encoder$$$" + k for k in ENC_KEYS]
        return out

    def param(self, name):
        u = self.unconstrained(name)
        if name in ("g", "s"):
            return torch.sigmoid(u)
        if name in ("lam1", "theta_scale"):
            return torch.exp(u)
        return u.clone()

    def _replayable(self, full):
        # the enumerated HO-DINA step (either guide): three or six launches; a subsample with the amortized guide
        # (VaeCHoDina, test.py:598-607: 20 rows, 10 particles)
        return full or self.amortized

    def loss_and_grads(self, rows=None, b_global=None, eps=None, stream_id=0):
        be = self.be
        nb, scale, sdc = self._call(rows, b_global)       # (sdc: a captured step's count lives in device memory)
        cfg = be.hodina_cfg(self.K, self.J, self.H, scale, self.seed, self.t, stream_id, **sdc)
        elbo = self._buf("elbo", nb)
        ws = self._buf("hd_ws", be.hodina_workspace(cfg, nb))
        lossslot = self.G[self.n_params:self.n_params + 1]
        if self.amortized:
            icfg = be.cfg("irt_2pl", 1, self.J_enc, self.H, 1.0, scale, self.seed, self.t, stream_id)
            ne = self._norm_enc_forward(icfg, self.y_enc, rows, nb)
            loc, raw, gloc, graw = ne.fw["loc"], ne.fw["raw"], ne.gloc, ne.graw
        else:
            loc, raw, gloc, graw = self._gather_pp(rows, nb)
        with self._phase("hodina"):
            be.hodina_grad(cfg, self.y, rows, nb, self.gid0, loc, raw, eps, self.q, self.view("lam0"),
                           self.view("lam1"), self.view("g"), self.view("s"), gloc, graw, elbo,
                           self.G[:self.n_item], ws)
        if self.amortized:
            with self._phase("guide_backward"):
                self._norm_enc_backward(ne, self._item_major_y_enc(rows))
                # (the heads have one row here: the helper's columns [:, H_model:] of [1][H] are the elements [H_model:])
                self._zero_phantom_unit_grads()
        else:
            self._scatter_pp(rows, nb, gloc, graw)
        be.sum_into(elbo, nb, -scale, lossslot, self.sum_ws, **sdc)   # (a captured step's counter advances here)
        self.last = {"elbo": elbo, "nb": nb}


class CcdmEngine(GridMixin, _EngineBase):
    """Pattern-enumerated DINA / DINO with the uniform pattern prior and an empty guide (VCCDM, vi.py:819-865).
    Flat parameter buffer: [g_un: J | s_un: J]; no per-person state, no random numbers."""

    pp_names = ()

    def __init__(self, y_u8, q, cdm="dina", n_global=None, gid0=0, seed=1234, group=None, backend=None):
        if cdm not in ("dina", "dino"):
            raise ValueError("model must be 'dina' or 'dino' (BaseCDM.CDM_FUN, vi.py:728-731)")
        self._preamble(y_u8, backend, n_global, gid0, seed, group)
        self._q_matrix(q)
        self.cdm, self.amortized, self.H = cdm, False, 0
        J = self.J
        self.off = {"g": 0, "s": J}
        self.shape = {"g": (1, J), "s": (1, J)}
        self.n_item = 2 * J
        self._alloc(self.n_item, self.n_local, per_person=False)
        self._init_g_s()                                                     # vi.py:844-845: g = s = 0.1

    def names(self):
        return ["g", "s"]

    def param(self, name):
        return torch.sigmoid(self.unconstrained(name))

    def score(self, y_u8=None, rows=None):
        """Classification of each scored row under the uniform pattern prior (the clamped Categorical of the step) and the
        item parameters as they stand: `attr_prob` (n, K) posterior mastery probabilities, `pattern` (n,) the most probable
        pattern (bit k = attribute k), `loglik` (n,) the marginal log-likelihood.  y_u8 / rows as IrtEngine.score."""
        out = self._grid_posterior(self._grid_call(y_u8, rows))
        return {"attr_prob": out["mean"], "pattern": out["node"], "loglik": out["loglik"]}

    def _grid_call(self, y_u8, rows, params=None):
        """The GridCall of score() and its kin: the nodes are the 2^K patterns.  params: the (g_un, s_un) [J] to tabulate, by
        default the leaves as they stand."""
        K, J, C = self.K, self.J, 1 << self.K
        y, rows = self._score_inputs(y_u8, rows, J)
        bits = ((torch.arange(C, device=self.dev)[:, None] >> torch.arange(K, device=self.dev)[None, :]) & 1)
        coord = bits.to(torch.float32).contiguous()
        eps32 = float(np.finfo(np.float32).eps)
        logw = torch.full((C,), 1.0 / C, dtype=torch.float32, device=self.dev).clamp(eps32, 1.0 - eps32).log()
        cfg = self.be.hodina_cfg(K, J, 0, 1.0, 0, 0, 0)
        g, s_ = params if params is not None else (self.view("g"), self.view("s"))
        return GridCall(y, rows, J, coord, logw,
                        lambda img: self.be.grid_table_cdm(cfg, self.cdm == "dino", self.q, g, s_, img), cfg)

    def plausible_values(self, y_u8=None, rows=None, draws=5, seed=0):
        """Plausible values: `draws` independent draws of each scored row's attribute pattern from its posterior over the 2^K
        patterns (the uniform prior of score() times the likelihood under the item parameters as they stand): `attr` float32
        (n, draws, K), the attribute bits of the drawn patterns, and `pattern` int32 (n, draws).  y_u8 / rows, draws, seed and
        the keying of the noise as IrtEngine.plausible_values.  The nodes here ARE the patterns: nothing is discretised.  The
        draws are taken under the item parameters as they stand, as fixed: their uncertainty is not in them."""
        draws, seed = self._draw_args(draws, seed)
        node, attr = self._grid_draws(self._grid_call(y_u8, rows), draws, seed, self.gid0 if y_u8 is None else 0)
        return {"attr": attr, "pattern": node}

    def expected_counts(self, y_u8=None, rows=None):
        """The expected-count tables of the scored rows over the 2^K patterns (IrtEngine.expected_counts): `n1`, `n0` [J][2^K],
        `mass` [2^K], `prob` [J][2^K] = P(y_j = 1 | pattern) and `patterns` [2^K][K], the attribute bits of every node."""
        call = self._grid_call(y_u8, rows)
        out = self._grid_counts(call)
        out["patterns"] = call.theta
        return out

    def point_estimates(self, *args, **kw):
        raise NotImplementedError("%s has no point_estimates: the point estimate of an attribute pattern is the MAP pattern "
                                  "score() already returns (`pattern`); ML / MAP / WLE by Fisher scoring belong to a continuous "
                                  "latent (IrtEngine with x_feature <= 3)" % type(self).__name__)

    def score_bifactor(self, *args, **kw):
        raise NotImplementedError("%s has no score_bifactor: a bifactor / testlet structure is one of continuous dimensions "
                                  "(IrtEngine with x_feature >= 2); the attribute patterns are scored by score()" % type(self).__name__)

    bifactor_structure = expected_counts_bifactor = fit_em_bifactor = score_bifactor

    def _group_refusals(self, covariates, impact):
        if covariates is not None or impact:
            raise NotImplementedError("dif with impact=True or covariates= on %s: there is no latent regression for attribute "
                                      "patterns (fit_population); the groups are scored under the uniform pattern prior"
                                      % type(self).__name__)

    def _group_prior(self, call, seg_start, covariates, impact):
        """GridMixin.dif / group_counts score every group under the uniform pattern prior: the zero tilt."""
        return call, None, None, None

    def _group_refit_check(self):
        raise NotImplementedError("dif(refit=True) on %s: the group refit is the Newton M-step of irt_1pl / irt_2pl "
                                  "(vx_grid_mstep_irt); only IrtEngine has it" % type(self).__name__)

    def fit_em(self, max_iter=100, tol=1e-6, newton=4, progress=False, prior=None):
        """Marginal maximum likelihood of g and s by EM over the 2^K patterns (IrtEngine.fit_em): the E-step of
        expected_counts(), then the closed-form M-step of vx_grid_mstep_cdm.  The enumerated ELBO of this class with its empty
        guide IS the marginal likelihood: this is a second optimiser of what fit() descends.  The pattern distribution stays the
        uniform prior; Adam's moments and the step count stay as they are.  `newton` is accepted for a common signature and
        unused.  An estimate of exactly 0 or 1 sits at the clamp, +-logit(1 - eps32), where the step kernels give it a zero
        gradient afterwards.  `prior` (IrtEngine.fit_em's item priors) is refused: the closed form has none."""
        self._em_refusals(max_iter, newton)
        if prior is not None:
            raise ValueError("fit_em(prior=) on %s: the priors are those of the IRT item parameters (IrtEngine); the closed-form "
                             "M-step of DINA / DINO takes none" % type(self).__name__)
        dino = self.cdm == "dino"
        g, s_ = self.view("g").clone(), self.view("s").clone()
        call = self._grid_call(None, None, params=(g, s_))
        return self._em_loop(call, lambda n1, n0: self.be.grid_mstep_cdm(call.cfg, dino, self.q, n1, n0, g, s_), {"g": g, "s": s_},
                             max_iter, tol, progress)

    def _info_call(self, y_u8, rows, prior=None):
        """What GridMixin.item_information needs of this class: two columns an item, g_un and s_un, both free.  `prior`
        (IrtEngine's item priors) is refused as fit_em refuses it."""
        if prior is not None:
            raise ValueError("item_information / item_se(prior=) on %s: the priors are those of the IRT item parameters "
                             "(IrtEngine); the fit of DINA / DINO takes none" % type(self).__name__)
        call = self._grid_call(y_u8, rows)
        g, s_ = self.view("g"), self.view("s")
        return call, 2, lambda wimg: self.be.grid_wtable_cdm(call.cfg, self.cdm == "dino", self.q, g, s_, wimg), \
            torch.ones(2 * self.J, dtype=torch.bool, device=self.dev)

    def _pairs_call(self, y_u8, rows):
        """What GridMixin.residual_sums needs of this class (IrtEngine._pairs_call): the point estimate is the MAP pattern."""
        call = self._grid_call(y_u8, rows)
        g, s_ = self.view("g").contiguous(), self.view("s").contiguous()
        return call, "pattern", "node", lambda est, t, ws, ws_floats: self.be.grid_pairs_cdm(
            call.cfg, self.cdm == "dino", self.q, call.y, call.rows, call.n, est, g, s_, t["n"], t["s"], t["ss"], t["sp"], ws, ws_floats)

    def _fit_call(self, y_u8, rows):
        """What GridMixin.fit_sums needs of this class (IrtEngine._fit_call): the point estimate is the MAP pattern."""
        call = self._grid_call(y_u8, rows)
        g, s_ = self.view("g").contiguous(), self.view("s").contiguous()
        return call, "pattern", "node", lambda est, person, item, ws, ws_floats: self.be.grid_fit_cdm(
            call.cfg, self.cdm == "dino", self.q, call.y, call.rows, call.n, est, g, s_, person, item, ws, ws_floats)

    def _sx2_params(self, items):
        """Two free parameters an item (g, s), for the df of GridMixin.sx2."""
        return np.full(len(items), 2, np.int64)

    @staticmethod
    def _score_table_leaves(out):
        """The nodes are the patterns with 0 / 1 coordinates: the posterior mean of a coordinate is the mastery probability."""
        out["attr_prob"] = out.pop("eap")
        del out["psd"]
        return out

    def _se_leaves(self, se):
        """Dense [P] -> g_un, s_un (1, J) and, by the delta method, g and s on the probability scale: se x (1 - x)."""
        se = se.reshape(self.J, 2)
        out = {"g_un": se[:, 0].reshape(1, -1).copy(), "s_un": se[:, 1].reshape(1, -1).copy()}
        for k in ("g", "s"):
            x = self.param(k).detach().cpu().numpy().astype(np.float64).reshape(1, -1)
            out[k] = out[k + "_un"] * x * (1.0 - x)
        return out

    def _replayable(self, full):
        # VCCDM (vi.py:819-865; test.py:560,585,624: 100-1500 rows a step): no guide, no random numbers -- the pattern
        # kernel, the loss sum (which advances the counter Adam reads) and the optimiser
        return True

    def loss_and_grads(self, rows=None, b_global=None, eps=None, stream_id=0):
        be = self.be
        nb, scale, sdc = self._call(rows, b_global)       # (sdc: a captured step's loss sum advances the device counter)
        cfg = be.hodina_cfg(self.K, self.J, 0, scale, self.seed, self.t, stream_id)
        elbo = self._buf("elbo", nb)
        ws = self._buf("cd_ws", be.ccdm_workspace(cfg, nb))
        with self._phase("ccdm"):
            be.ccdm_grad(cfg, self.cdm == "dino", self.y, rows, nb, self.q, self.view("g"), self.view("s"), elbo,
                         self.G[:self.n_item], ws)
        be.sum_into(elbo, nb, -scale, self.G[self.n_params:self.n_params + 1], self.sum_ws, **sdc)
        self.last = {"elbo": elbo, "nb": nb}


class VaeCcdmEngine(_EngineBase):
    """VaeCCDM (vi.py:866-891): pattern-enumerated DINA / DINO with the SoftmaxEncoder prior (vi.py:473-485).  The encoder's
    softmax runs over the BATCH (dim = 0), so a step needs three batch-wide reductions of C = 2^K floats (column max, column
    sum of exponentials, column sum of the prior gradients) -- all-reduced over the ranks when the persons are sharded.
    Missing responses stay in the observation as -1, as in the reference.  Flat buffer: [g_un: J | s_un: J | encoder]."""

    pp_names = ()

    def __init__(self, y_u8, q, cdm="dina", n_global=None, gid0=0, H=64, encoder_init=None, seed=1234, group=None,
                 backend=None):
        if cdm not in ("dina", "dino"):
            raise ValueError("model must be 'dina' or 'dino' (BaseCDM.CDM_FUN, vi.py:728-731)")
        self._preamble(y_u8, backend, n_global, gid0, seed, group)
        self._q_matrix(q)
        self.C = 1 << self.K
        self.cdm, self.amortized, self.H = cdm, True, int(H)
        J, C = self.J, self.C
        self.off = {"g": 0, "s": J}
        self.shape = {"g": (1, J), "s": (1, J)}
        self.n_item = 2 * J
        o = self._encoder_segments({"fc1.weight": (self.H, J), "fc1.bias": (self.H,), "fc2.weight": (C, self.H), "fc2.bias": (C,)})
        self._alloc(o, self.n_local, per_person=False)
        self._init_g_s()                                                     # vi.py:875-876
        # (the BinEncoder's nn.Linear shapes with C outputs)
        self._fill_encoder(default_bin_encoder_init(J, C, self.H, seed) if encoder_init is None else encoder_init, J, self.H)

    def names(self):
        return ["g", "s"] + ["encoder$$$" + k for k in BIN_ENC_KEYS]

    def param(self, name):
        u = self.unconstrained(name)
        return torch.sigmoid(u) if name in ("g", "s") else u.clone()

    def _replayable(self, full):
        # on one rank (VaeCCDM, vi.py:868-891; test.py:565,629: 100 or 50 rows a step): no random numbers; the softmax over
        # the batch is three column reductions on the device (sharded, they are small all-reduces between kernels: eager)
        return self.group is None

    def loss_and_grads(self, rows=None, b_global=None, eps=None, stream_id=0):
        be = self.be
        nb, scale, sdc = self._call(rows, b_global)       # (sdc: a captured step's loss sum advances the device counter)
        C, H = self.C, self.H
        cfg = be.hodina_cfg(self.K, self.J, H, scale, self.seed, self.t, stream_id)
        enc = self._enc()
        h, z, gla = self._buf("vc_h", nb * H), self._buf("vc_z", nb * C), self._buf("vc_gla", nb * C)
        m, Z, T = self._buf("vc_m", C), self._buf("vc_Z", C), self._buf("vc_T", C)
        cws = self._buf("vc_cws", be.col_reduce_workspace(max(nb, 1), C))
        elbo = self._buf("elbo", nb)
        ws = self._buf("vc_ws", be.vaeccdm_workspace(cfg, nb))
        with self._phase("guide_forward"):
            be.sm_enc_forward(cfg, self.y, rows, nb, enc, h, z)
            be.col_reduce(0, z, nb, C, None, m, cws)                      # column maximum over the batch ...
            self._allreduce(m[:C], torch.distributed.ReduceOp.MAX)       # ... of every rank
            be.col_reduce(1, z, nb, C, m, Z, cws)
            self._allreduce(Z[:C])
            off = self._buf("vc_off", C)
            torch.add(m[:C], torch.log(Z[:C]), out=off[:C])               # attr_p = exp(z - off)
        with self._phase("vaeccdm"):
            be.vaeccdm_grad(cfg, self.cdm == "dino", self.y, rows, nb, self.q, self.view("g"), self.view("s"), z, off, elbo,
                            gla, self.G[:self.n_item], ws)
        with self._phase("guide_backward"):
            be.col_reduce(2, gla, nb, C, None, T, cws)
            self._allreduce(T[:C])
            bws = self._buf("vc_bws", be.sm_enc_bwd_workspace(cfg, nb))
            be.sm_enc_backward(cfg, self.y, rows, nb, enc, h, z, off, T, gla,
                               self.G[self.enc_off0:self.enc_off0 + self.n_enc], bws)
        be.sum_into(elbo, nb, -scale, self.G[self.n_params:self.n_params + 1], self.sum_ws, **sdc)
        self.last = {"elbo": elbo, "nb": nb}


BIN_ENC_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
CDM_REF_PRIOR = 1.5          # vi.py:753: Bernoulli(torch.ones(..) + 0.5) -- probability 1.5, clamped by log_prob


class CdmSfEngine(_EngineBase):
    """Bernoulli-guide DINA / DINO with the score-function (REINFORCE) estimator: VCDM / VaeCDM (vi.py:726-816).

    Flat parameter buffer: [g_un: J | s_un: J | BinEncoder (amortized only)]; per-person rows `attr_p` (n, K) logits of the
    guide probabilities for VCDM (vi.py:811).  baseline: 'none' = pyro's Trace_ELBO; 'avg' = per-person decaying average
    of log_r (rate `baseline_beta`); 'loo' = leave-one-out mean over the particles of a step (all particles then share the
    step's subsample).  attr_prior: probability of mastering an attribute under the model prior; None reproduces the
    reference's Bernoulli(1.5)."""

    pp_names = ("attr_p",)

    def __init__(self, y_u8, q, cdm="dina", n_global=None, gid0=0, amortized=False, H=64, encoder_init=None, seed=1234,
                 group=None, backend=None, attr_prior=None, baseline="none", baseline_beta=0.9):
        if cdm not in ("dina", "dino"):
            raise ValueError("model must be 'dina' or 'dino' (BaseCDM.CDM_FUN, vi.py:728-731)")
        if baseline not in ("none", "avg", "loo"):
            raise ValueError("baseline must be 'none', 'avg' or 'loo'")
        self._preamble(y_u8, backend, n_global, gid0, seed, group)
        if bool((self.y > 1).any()):
            raise ValueError("VCDM / VaeCDM need complete 0/1 responses: the reference hands them to the likelihood "
                             "unmasked (vi.py:756), a missing cell makes its loss NaN")
        self._q_matrix(q)
        self.cdm, self.amortized, self.H = cdm, bool(amortized), int(H) if amortized else 0
        self.attr_prior = CDM_REF_PRIOR if attr_prior is None else float(attr_prior)
        self.baseline, self.baseline_beta = baseline, float(baseline_beta)
        J, K = self.J, self.K
        self.off = {"g": 0, "s": J}
        self.shape = {"g": (1, J), "s": (1, J)}
        self.n_item = 2 * J
        o = self.n_item
        if self.amortized:
            o = self._encoder_segments({"fc1.weight": (self.H, J), "fc1.bias": (self.H,), "fc2.weight": (K, self.H), "fc2.bias": (K,)})
        self.pp_shape = {"attr_p": (self.n_local, K)}
        self._alloc(o, self.n_local, per_person=not self.amortized)
        self._init_g_s()                                                     # vi.py:748-749: g = s = 0.1
        if self.amortized:
            self._fill_encoder(default_bin_encoder_init(J, K, self.H, seed) if encoder_init is None else encoder_init, J, self.H)
        self.base = torch.zeros(max(self.n_local, 1), dtype=torch.float32, device=self.dev) if baseline == "avg" else None

    def names(self):
        return ["g", "s"] + (["encoder$$$" + k for k in BIN_ENC_KEYS] if self.amortized else [])

    def param(self, name):
        u = self.unconstrained(name)
        if name in ("g", "s"):
            return torch.sigmoid(u)
        if name == "attr_p":                                                   # unit_interval: clamped sigmoid
            return torch.clamp(torch.sigmoid(u), min=float(np.finfo(np.float32).tiny), max=1.0 - float(np.finfo(np.float32).eps))
        return u.clone()

    def loss_and_grads(self, rows=None, b_global=None, eps=None, stream_id=0, baseline_buf=None, guide_grads=True):
        """One particle.  `eps`: uint8 (nb, K) attribute draws to replay, or None (drawn in the kernel from Philox, keyed
        by the global person id).  baseline_buf / guide_grads: the 'loo' mode (step(), _loo_step)."""
        be = self.be
        nb, scale, sdc = self._call(rows, b_global)       # (sdc: a captured step's count lives in device memory)
        K = self.K
        cfg = be.hodina_cfg(K, self.J, self.H, scale, self.seed, self.t, stream_id, **sdc)
        ws = self._buf("cs_ws", be.cdm_sf_workspace(cfg, nb))
        gu = self._buf("cs_gu", nb * K)
        if self.amortized:
            enc = self._enc()
            h, u = self._buf("cs_h", nb * self.H), self._buf("cs_u", nb * K)
            with self._phase("guide_forward"):
                be.bin_enc_forward(cfg, self.y, rows, nb, enc, h, u)
        else:
            u = self.PP if rows is None else self.PP.reshape(self.n_local, K)[rows].contiguous().reshape(-1)
        log_r, base, beta, by_row = self._score_pass("cs_lr", nb, stream_id, baseline_buf, guide_grads)
        with self._phase("cdm_sf"):
            be.cdm_sf_grad(cfg, self.cdm == "dino", not self.amortized, self.attr_prior, self.y, rows, nb, self.gid0, self.q,
                           self.view("g"), self.view("s"), u, eps, base, beta, by_row, gu, log_r, None,
                           self.G[:self.n_item], ws)
        if guide_grads:
            if self.amortized:
                with self._phase("guide_backward"):
                    bw = self._buf("cs_bws", be.bin_enc_bwd_workspace(cfg, nb))
                    be.bin_enc_backward(cfg, self.y, rows, nb, enc, h, gu,
                                        self.G[self.enc_off0:self.enc_off0 + self.n_enc], bw)
            elif rows is None:
                self.GP.copy_(gu[:nb * K])
            else:                                              # dense per-person gradient: zero off the batch (vi.py:811)
                self.GP.zero_()
                self.GP.reshape(self.n_local, K).index_add_(0, rows, gu[:nb * K].reshape(nb, K))
        be.sum_into(log_r, nb, -1.0, self.G[self.n_params:self.n_params + 1], self.sum_ws, **(sdc if guide_grads else {}))
        self.last = {"log_r": log_r, "gu": gu, "nb": nb}

    def step(self, lrs, rows=None, b_global=None, eps=None, num_particles=1):
        """The common step (_EngineBase.step), or the two passes over the particles of the leave-one-out control variate
        (baseline 'loo', _loo_step)."""
        S = int(num_particles)
        if self.baseline == "loo" and S >= 2:
            return self._loo_step(lrs, rows, b_global, eps, S)
        return super().step(lrs, rows=rows, b_global=b_global, eps=eps, num_particles=S)

    def _replayable(self, full):
        # VCDM / VaeCDM (vi.py:733-816; test.py:522-549: 100 or 1000 rows a step): the Bernoulli draws' Philox step and Adam's
        # t from the device counter that the loss sum advances (k_cdm_sf reads vx_hodina_cfg.step_dev); the per-person
        # guide's gather / scatter of the batch rows are torch index kernels inside the capture.  Not the two passes of 'loo'
        return self.baseline != "loo"


def default_bin_encoder_init(J, K, H, seed):
    """nn.Linear default initialisation for BinEncoder (vi.py:458-470), drawn on the host."""
    g = torch.Generator().manual_seed(int(seed) + 7919)

    def lin(out_f, in_f):
        k = 1.0 / math.sqrt(in_f)
        return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * k, (torch.rand(out_f, generator=g) * 2 - 1) * k
    w1, b1 = lin(H, J)
    w2, b2 = lin(K, H)
    return {"fc1.weight": w1, "fc1.bias": b1, "fc2.weight": w2, "fc2.bias": b2}


class _Phase(object):
    """Brackets a phase with HIP events on the current stream when bench.py asks for it."""

    def __init__(self, sink, name):
        self.sink, self.name = sink, name

    def __enter__(self):
        if self.sink is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record()
            self.sink.append((self.name, self.e0, self.e1))
        return False


def _grown(t, shape):
    """t with zeros behind it in every dimension, up to `shape` (what a phantom's parameters start as)."""
    return torch.nn.functional.pad(t, [v for have, want in zip(reversed(t.shape), reversed(shape)) for v in (0, want - have)])


def _merge_segments(segs):
    segs = sorted(segs)
    out = []
    for b, e, lr in segs:
        if out and out[-1][1] == b and out[-1][2] == lr:
            out[-1] = (out[-1][0], e, lr)
        else:
            out.append((b, e, lr))
    return out


def default_encoder_init(J, D, H, seed):
    """nn.Linear default initialisation (kaiming-uniform with a = sqrt(5) => U(-1/sqrt(fan_in), +))
    for the encoder of vi.py:417-455, drawn on the host."""
    g = torch.Generator().manual_seed(int(seed) + 7919)
    T = D * (D + 1) // 2 if D > 1 else 1

    def lin(out_f, in_f):
        k = 1.0 / math.sqrt(in_f)
        w = (torch.rand(out_f, in_f, generator=g) * 2 - 1) * k
        b = (torch.rand(out_f, generator=g) * 2 - 1) * k
        return w, b
    w1, b1 = lin(H, J)
    w21, b21 = lin(D, H)
    w22, b22 = lin(T, H)
    return {"fc1.weight": w1, "fc1.bias": b1, "fc21.weight": w21, "fc21.bias": b21, "fc22.weight": w22,
            "fc22.bias": b22}
