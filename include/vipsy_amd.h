/*
 * vipsy_amd C ABI -- the drop-in boundary for the ELBO-gradient hot path on MI355X (gfx950).
 *
 * The reference (inuyasha2012/vipsy) has no native boundary: the op being replaced is
 *     loss = svi.step(data)                                   vi.py:503-516, called from
 *     BaseIRT.fit vi.py:634-638 / VCHoDina.fit vi.py:937-942
 * whose arithmetic lives in pyro-ppl 1.4.0 (Trace_ELBO / TraceEnum_ELBO + pyro.optim.Adam).
 * This header is what a binding for that op links against: plain C, device pointers and sizes,
 * no torch types.  Every entry point
 *   - is asynchronous on the hipStream_t passed as `void* stream`,
 *   - allocates nothing and never synchronises (graph-capturable),
 *   - borrows device memory owned by the caller (PyTorch-ROCm in our host code),
 *   - returns 0 on success, a hipError_t (>0) from the launch, or a VX_E* code (<0) for bad
 *     arguments.
 *
 * One step of the reference loop maps to, in order (vipsy_amd/engine.py drives exactly this):
 *   guide forward  (encoder / per-person variational rows -> x, entropy)   vi.py:673-723
 *   model likelihood + gradients                                             vi.py:574-625
 *   guide backward (encoder weight grads / per-person grads)
 *   [multi-GPU: one RCCL all-reduce of the flat gradient buffer -- done by the host]
 *   optimiser on the unconstrained leaves, `free` mask applied               vi.py:508-514
 *
 * Data contract: responses are uint8, 1 byte per cell: 0, 1, or 255 = missing (the reference
 * holds float32 with NaN, vi.py:621).  All parameters / state are float32, unconstrained
 * (vi.py:510).  Persons are rows; a rank owns the contiguous shard [gid0, gid0 + n_local).
 */
#ifndef VIPSY_AMD_H
#define VIPSY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_OK 0
#define VX_EINVAL (-1)       /* bad argument / unsupported shape */
#define VX_EUNIMPL (-2)
#define VX_ABI_VERSION 9

enum vx_model { VX_IRT_1PL = 1, VX_IRT_2PL = 2, VX_IRT_3PL = 3, VX_IRT_4PL = 4 }; /* vi.py:538-543 */

/* Problem description shared by the IRT entry points (BaseIRT.__init__, vi.py:545-572). */
typedef struct vx_irt_cfg {
    int32_t model;       /* enum vx_model */
    int32_t D;           /* x_feature: latent dimensions */
    int32_t J;           /* item_size */
    int32_t H;           /* encoder hidden_dim (amortized guides; <= 128), else 0 */
    float   Dc;          /* the scalar `D` of vi.py:549 (1 or 1.702) */
    float   scale;       /* plate scale N_global / B_global */
    uint64_t seed;       /* Philox key */
    uint32_t step;       /* Philox counter word 2: optimisation step */
    uint32_t stream;     /* Philox counter word 3 high half: particle index */
    const uint32_t* step_dev; /* or NULL: the step counter in DEVICE memory -- vx_mvn_enc_forward / vx_mvn_bbvi_forward read the Philox step from it
                            instead of `step`, so that a whole step can be captured once in a HIP graph and replayed
                            (vx_sum2 advances it, vx_adam_step reads it; the D = 1 entry points take it as an argument) */
    const int64_t* rows_ring; /* or NULL.  A captured subsampled step (test.py:338-343: a new draw of B rows every step) needs its
                            row indices on the device without a copy of its own in front of every replay: the host writes
                            the draw of step t into slot t % rows_ring_slots of this PINNED HOST buffer
                            ([rows_ring_slots][rows_ring_stride] int64), and vx_mvn_enc_forward -- with step_dev, and `rows`
                            then being the DEVICE buffer the kernels of the step read -- first copies slot
                            *step_dev % rows_ring_slots into `rows` (nb indices), inside its first launch where it can.  The
                            host must not rewrite a slot before the step that read it has finished. */
    int64_t rows_ring_stride;
    int32_t rows_ring_slots;
    int32_t _pad;
} vx_irt_cfg;

int vx_abi_version(void);
const char* vx_build_info(void);

/* ---- Measurement aid (no reference counterpart; used by bench.py only).  While enabled, the entry points record a
 * pair of HIP events on their launch stream around each of the large kernels; vx_prof_read synchronises on them and
 * returns the kernel's name, its mean duration and the number of launches seen since vx_prof_enable(1).  Disabled
 * (the default) nothing is recorded and no entry point synchronises.
 *   on = 0: off, what was recorded is dropped;  1: on, what was recorded is dropped;
 *   on = 3: PAUSE (off, the records stay);  2: RESUME (on, the records stay) -- bench.py brackets a SAMPLE of the timed steps:
 *   an event pair around a kernel costs the stream a few microseconds (25 pairs a step: 0.11 ms of the 9.0 ms headline step). */
int vx_prof_enable(int on);
int vx_prof_count(void);
int vx_prof_read(int slot, char* name, int name_cap, float* mean_ms, int* launches);
/* persons the last launch of that kernel took when the batch is divided between two kernels (the amortized forward gives
 * whole chip rounds to k_mvn_enc_fwd_b2 and a short last round to k_mvn_enc_fwd_b); 0 = the whole batch */
int vx_prof_units(int slot, int64_t* units);

/* ---- RNG: eps[i, d] = N(0,1) keyed by the GLOBAL person id (Philox4x32-10 + Box-Muller).
 * gids == NULL means gid = gid0 + i.  Also used by tests to hand the oracle identical eps. */
int vx_philox_normals(float* eps /*[n][D]*/, const int64_t* gids, int64_t gid0, int64_t n, int32_t D,
                      uint64_t seed, uint32_t step, uint32_t stream, void* hip_stream);
/* raw Philox words for bit-exact checks against the oracle: out[i][4] for counter (i, 0, step, stream<<16) */
int vx_philox_raw(uint32_t* out /*[n][4]*/, int64_t gid0, int64_t n, uint64_t seed, uint32_t step,
                  uint32_t stream, void* hip_stream);

/* ---- amortized multivariate-normal guide, forward (MvnEncoder.forward + rsample of
 * MultivariateNormal(loc, scale_tril=LowerCholeskyTransform(M)); vi.py:438-455, 685-693).
 *   rows   : local row index of each batch member (NULL = 0..nb-1), gids for the RNG = gid0+row
 *   eps_in : if non-NULL use these draws instead of generating them (parity tests)
 * Outputs (all [nb][...], float32): h = softplus(fc1), x = loc + L eps, eps, ldT[D][nb] =
 * exp(diag M) stored dimension-major, ent[i] = 0.5|eps_i|^2 + sum_k M_kk (= log p/q constants
 * cancelled). */
int vx_mvn_enc_forward(const vx_irt_cfg* cfg, const uint8_t* y /*[n_local][J]*/, const int64_t* rows,
                       int64_t nb, int64_t gid0,
                       const float* W1 /*[H][J]*/, const float* b1, const float* W21 /*[D][H]*/,
                       const float* b21, const float* W22 /*[T][H]*/, const float* b22,
                       const float* eps_in, float* h /*[nb][H]*/, float* x /*[nb][D]*/,
                       float* eps /*[nb][D]*/, float* ldT /*[D][nb]*/, float* ent /*[nb]*/,
                       float* hT /*[H][nb] or NULL*/, float* epsT /*[D][nb] or NULL*/,
                       float* packws /*vx_mvn_pack_floats(cfg) floats or NULL*/,
                       uint8_t* ximg /*vx_irt_lik_ximg_bytes(cfg, nb) bytes or NULL*/,
                       uint16_t* hs /*[2][64][nb] fp16 or NULL*/, void* hip_stream);
/* hs (optional, with hT, hidden_dim 64): the two fp16 terms of hT 2^sh (the power of two that `packws` carries for h), the
 * operand of the head weight-gradient kernel -- point it at workspace + vx_mvn_enc_bwd_hs_offset(cfg, nb) of the backward
 * call and set bit 1 of its gd_ready. */
/* ximg (optional, vx_irt_lik_ximg_bytes(cfg, nb) > 0 only: 96 <= D <= 111, 1PL / 2PL link): x once more, as the pre-split
 * operand image of the fp16-MFMA likelihood kernel (two fp16 terms of x 2^7 per value, in that kernel's LDS tile order,
 * followed by one overflow word that the writers raise for a latent of |x| >= 511.75); hand the same buffer to
 * vx_irt_lik_grad, which otherwise makes it itself. */
/* hT / epsT: optional dimension-major copies of h and eps (person-contiguous rows) for the weight-gradient kernel
 * of vx_mvn_enc_backward; written only by the packed fast path (H == 64, D % 4 == 0, J % 4 == 0). */
/* `packws` holds this step's packed copy of the head weights (a re-ordering of fc22 | fc21 rows that the
 * fast kernels use, see vipsy_amd/csrc/k_pack.hip), their fp16-pair operand images and the powers of two of the
 * f16x2 operands; forward fills it, the matching backward call of the SAME step reads it. */
int64_t vx_mvn_pack_floats(const vx_irt_cfg* cfg);
/* float offset inside packws of the three words that collect the step's largest |gx|, |gd|, |eps| (vx_irt_lik_grad's opmax;
 * cleared by vx_mvn_enc_forward), or -1 when this (cfg, nb) does not run the f16x2 kernels that use them */
int64_t vx_mvn_pack_opmax_offset(const vx_irt_cfg* cfg, int64_t nb);

/* ---- model likelihood + gradients for D >= 2 (irt_2pl..4pl + _get_p_data mask + Bernoulli
 * log-lik; vi.py:32-66, 596-625).  Consumes x, produces
 *   gx[nb][D]      d ELBO / d x  = scale * (R A^T - x)          (likelihood + N(0,I) prior)
 *   ll[nb]         per-person  log p(y_i | x_i) - 0.5 |x_i|^2
 *   gitem          gradient of the LOSS (= -ELBO), float [D*J + 3*J] laid out
 *                  [a: D*J | b: J | c_un: J | d_un: J]  (c/d w.r.t. the unconstrained leaves,
 *                  zero for models without them); summed over this rank's batch only.
 * `workspace`: vx_irt_lik_workspace_floats(cfg, nb) floats of scratch (partial slabs). */
int64_t vx_irt_lik_workspace_floats(const vx_irt_cfg* cfg, int64_t nb);
/* size of the optional x operand image (0: this shape does not use one) */
int64_t vx_irt_lik_ximg_bytes(const vx_irt_cfg* cfg, int64_t nb);
int vx_irt_lik_grad(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                    const float* x /*[nb][D]*/, const float* a /*[D][J]*/, const float* b /*[J]*/,
                    const float* c_un /*[J] or NULL*/, const float* d_un /*[J] or NULL*/,
                    float* gx /*[nb][D] or NULL*/, float* gxT /*[D][nb] or NULL*/, float* ll /*[nb]*/,
                    float* gitem /*[D*J + 3*J]*/, float* workspace,
                    const uint8_t* yT /*[J + 1][yT_stride] or NULL*/, int64_t yT_stride,
                    const uint8_t* ximg /*as written by vx_mvn_enc_forward, or NULL*/,
                    const float* epsT /*[D][nb] or NULL*/, const float* ldT /*[D][nb] or NULL*/,
                    float* gdT /*[D][nb] or NULL: fused output gxT * epsT * ldT + scale*/,
                    uint32_t* opmax /*[3] or NULL, with gdT*/, void* hip_stream);
/* gx and gxT are the same gradient in person-major / dimension-major order; at least one must be given.
 * gdT (optional, with gxT, epsT, ldT; nb * D % 4 == 0): the DIAG-row operand of the dimension-major guide-backward kernels,
 * written in the same pass over gxT -- point it at workspace + vx_mvn_enc_bwd_gd_offset(cfg, nb) of the backward call and
 * hand that call gd_ready = 1.
 * opmax (optional, with gdT): three words that receive, by integer atomicMax on the float bits, the largest |gx|, |gd| and
 * |eps| of the batch -- what the f16x2 head weight-gradient kernel takes its power of two from.  Point it at packws +
 * vx_mvn_pack_opmax_offset(cfg) (cleared by the forward call of the step) and set bit 2 of the backward call's gd_ready: the
 * head weight gradient then starts beside the hidden gradient instead of behind it.
 * yT (optional, full batches only: rows == NULL): the responses item-major -- row j = item j over the batch rows, row J
 * and every column past nb filled with 254 ("outside the problem"), yT_stride % 64 == 0 and >= nb rounded up to 64.
 * With it, 96 <= D <= 111 runs on the MFMA kernels -- 1PL / 2PL: k_irt_lik_h.hip (fp32 results from two fp16 terms per
 * operand, three products; a batch with a latent of |x| >= 511.75 is taken by k_irt_lik_b.hip instead, decided on the
 * device), 3PL / 4PL: k_irt_lik_b.hip (three bf16 terms, six products); the same buffer serves vx_mvn_enc_backward / vx_norm_enc_backward (which read rows 0..J-1). */

/* ---- amortized MVN guide, backward: encoder weight gradients of the LOSS from gx.
 * genc = d LOSS / d encoder parameters, flat in the nn.Linear order of vi.py:442-444:
 *   [W1: H*J | b1: H | W21: D*H | b21: D | W22: T*H | b22: T],  T = D(D+1)/2. */
int64_t vx_mvn_enc_param_floats(const vx_irt_cfg* cfg);          /* length of genc */
int64_t vx_mvn_enc_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb);
/* 1: this (cfg, nb) runs on the dimension-major kernels when hT, epsT and gxT are supplied (gx may then be NULL and
 * the likelihood call needs to produce gxT only); 0: the person-major kernels, which need gx. */
int vx_mvn_enc_bwd_layout(const vx_irt_cfg* cfg, int64_t nb);
int vx_mvn_enc_backward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                        const float* W21, const float* W22,
                        const float* h, const float* eps, const float* ldT, const float* gx,
                        const float* hT /*or NULL*/, const float* epsT /*or NULL*/, const float* gxT /*or NULL*/,
                        const uint8_t* yT /*[>= J][yT_stride] item-major copy of y (pad bytes 0 or 254), or NULL*/, int64_t yT_stride,
                        float* genc, float* workspace, const float* packws,
                        int32_t gd_ready /*bit 0: vx_irt_lik_grad already wrote gdT into the workspace; bit 1:
                                           vx_mvn_enc_forward already wrote hs there; bit 2: the operand maxima are in packws
                                           (vx_irt_lik_grad's opmax)*/, void* hip_stream);
/* The same call, and the loss of the step with it: loss[0] = loss_alpha * (sum ll + sum ent) over the nb persons of the
 * batch -- what vx_sum2 computes, bit for bit (vi.py:516, the value svi.step returns) -- from the call's LAST launch, and the
 * device step counter of a captured step (cfg->step_dev) advanced there as vx_sum2 would.  A B = 100 step (test.py:338) is
 * a dozen launches of which this saves one; batches above 4 096 persons run vx_sum2's two launches behind the gradients.
 * sum_workspace: vx_sum_workspace_floats() floats. */
int vx_mvn_enc_backward_loss(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                             const float* W21, const float* W22,
                             const float* h, const float* eps, const float* ldT, const float* gx,
                             const float* hT /*or NULL*/, const float* epsT /*or NULL*/, const float* gxT /*or NULL*/,
                             const uint8_t* yT /*or NULL*/, int64_t yT_stride, float* genc, float* workspace,
                             const float* packws, int32_t gd_ready, const float* ll /*[nb]*/, const float* ent /*[nb]*/,
                             float loss_alpha, float* loss /*[1]*/, float* sum_workspace, void* hip_stream);
/* float offset of gdT[D][nb] inside the backward workspace, or -1 when this (cfg, nb) has no such operand */
int64_t vx_mvn_enc_bwd_gd_offset(const vx_irt_cfg* cfg, int64_t nb);
/* float offset of hs[2][64][nb] (fp16) inside the backward workspace, or -1 when this (cfg, nb) does not use it */
int64_t vx_mvn_enc_bwd_hs_offset(const vx_irt_cfg* cfg, int64_t nb);
/* With hT, epsT and gxT (the dimension-major copies made by the forward / likelihood calls) the head weight
 * gradients run on the DMA-staged kernel of k_mvn_bwd_t.hip; without them on the person-major one.
 * yT (full batch only, rows == NULL, yT_stride % 16 == 0): the responses item-major, which lets the fc1 weight
 * gradient read 16 persons of an item with one 16-byte LDS load; the responses never change, so the host
 * transposes them once. */

/* ---- D = 1 models (irt_1pl..4pl, Normal guide; vi.py:588-595, 677-684, 701-705), fused:
 * x = loc + exp(raw) eps, likelihood, prior, entropy, gradients w.r.t. loc/raw and the items.
 *   loc/raw: [nb] (already gathered for BBVI minibatches, or encoder outputs)
 *   outputs: gloc[nb], graw[nb] = d LOSS / d loc, d raw;  elbo[nb] = per-person
 *            log p(y|x) + log p(x) - log q(x) (unscaled);
 *   gitem:   d LOSS / d [a: J | b: J | c_un: J | d_un: J] for this rank's batch (a = 0 for 1PL).
 * J <= 1024.  workspace: vx_irt1d_workspace_floats(cfg, nb) floats -- size it with THAT call, not by hand: behind the
 *   n_slabs x (4 J + 1) slab words the step kernels (vx_irt1d_grad and vx_irt1d_sparse_grad alike, with or without the
 *   *_adam tail) leave Adam's count in one trailing word, slabs[n_slabs * (4 J + 1)], for k_reduce_adam; the size query
 *   includes it (+ 4 floats).  A buffer of n_slabs * (4 J + 1) floats is 4 bytes short.
 * loss (or NULL): receives d LOSS itself, -scale * sum(elbo), summed in a fixed order.
 * step_dev (or NULL): the step counter in DEVICE memory -- the kernel reads the Philox step from it instead of cfg->step,
 * and the call ADVANCES it by one when the gradients are done (so vx_adam_step's t_dev may point at the same word: Adam's
 * count is the step + 1).  Lets a whole step be captured once in a HIP graph and replayed. */
int64_t vx_irt1d_workspace_floats(const vx_irt_cfg* cfg, int64_t nb);
int vx_irt1d_grad(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                  const float* loc, const float* raw, const float* eps_in,
                  const float* a, const float* b, const float* c_un, const float* d_un,
                  float* gloc, float* graw, float* elbo, float* gitem, float* loss, uint32_t* step_dev,
                  float* workspace, void* hip_stream);

/* Score-function (REINFORCE) estimator with a control-variate baseline for the Normal guide of the D = 1 models
 * (BASELINE.json north_star).  The reference takes pathwise gradients for these guides (vi.py:684,705:
 * Normal has rsample), so this mode has no reference output to match: an opt-in of this build (IrtEngine(estimator=
 * "score")), checked against oracle/vi_oracle.py::irt_particle(estimator="score").  Called AFTER vx_irt1d_grad of the same
 * batch (whose item gradients and loss stand): overwrites gloc / graw [nb] with
 *     d LOSS / d loc_i = -(log_r_i - baseline_i) eps_i exp(-raw_i),   d LOSS / d raw_i = -(log_r_i - baseline_i) (eps_i^2 - 1),
 *     log_r_i = scale * elbo[i].
 * eps[nb]: the draws the step used (vx_philox_normals with the step's seed / step / stream, or the caller's own);
 * baseline: NULL, an explicit control variate in batch order (base_beta < 0), or a decaying average updated after use
 * (base_beta >= 0: baseline <- beta baseline + (1 - beta) log_r), indexed by rows[i] when base_by_row != 0 and rows != NULL;
 * log_r: optional output [nb]. */
int vx_irt1d_score_grad(int64_t nb, float scale, const float* elbo, const float* eps, const float* raw, const int64_t* rows,
                        float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* gloc, float* graw,
                        void* hip_stream);

/* Score-function estimator for the multivariate Normal guides, x_feature > 1 (same standing as vx_irt1d_score_grad: an opt-in
 * of this build, IrtEngine(estimator="score"); oracle/vi_oracle.py::irt_particle).  With u_i = L_i^-T eps_i the score of the
 * guide has the pathwise gradient's shape -- d log q / d loc = u, / d L_kc = u_k eps_c, / d M_kk = u_k eps_k L_kk - 1 -- so
 * this call, made AFTER the forward and the likelihood of the same batch (whose item gradients and loss stand), only writes
 * the operands the guide-backward kernels take in place of d ELBO / d x:
 *     w[i] = log_r_i - baseline_i,  log_r_i = cfg->scale (ll[i] + ent[i])        (baseline arguments as vx_irt1d_score_grad)
 *     gx[nb][D], gxT[D][nb] = w_i u_i;   gdT[D][nb] = w_i (u_ik eps_ik L_kk - 1)   (the DIAG-row operand; any may be NULL)
 * kind 0: L from the encoder heads (h [nb][H], W22 [T][H], b22 [T]); hand gxT / gdT to vx_mvn_enc_backward (gd_ready bit 0),
 * which must be on the dimension-major kernels (vx_mvn_enc_bwd_layout == 1).  kind 1 / 2: L from M [n_local][D][D] (rows
 * index it) / the shared M [D][D]; run vx_mvn_bbvi_backward on gx with cfg->scale = 0, then vx_mvn_score_diag adds the
 * diagonal term (+ w_i on the person's own M_kk, + sum_i w_i on the shared one). */
int vx_mvn_score_operands(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, int32_t kind, const float* h,
                          const float* W22, const float* b22, const float* M, const float* eps, const float* ll,
                          const float* ent, float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* w,
                          float* gx, float* gxT, float* gdT, void* hip_stream);
int vx_mvn_score_diag(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* w, int32_t shared, float* gM,
                      void* hip_stream);
/* The kind-0 operands (L from the encoder heads) on the fp16 MFMA, for the shapes the f16x2 guide kernels take (hidden_dim 64,
 * x_feature % 4 == 0, 8 <= x_feature <= 124): u = L^-T eps as a back-substitution over COLUMN tiles of the head GEMM the
 * forward runs, 32 persons a wave (k_mvn_score_b.hip).  Same outputs as vx_mvn_score_operands(kind 0) with gx / w = NULL, to
 * the f16x2 products' 2^-22.  Made AFTER vx_mvn_enc_forward of the same batch and parameters:
 *   packws: the forward's pack workspace (the powers of two of its operands are read from its scale block);
 *   h[nb][64], eps[nb][D]: the forward's outputs (L_kk = exp(M_kk) is recomputed with the rows below it);
 *   workspace: vx_mvn_score_heads_workspace_floats(cfg) floats (the column-ordered weight image, rebuilt every call).
 * VX_EINVAL for any other shape (the caller then uses vx_mvn_score_operands). */
int64_t vx_mvn_score_heads_workspace_floats(const vx_irt_cfg* cfg);
int vx_mvn_score_heads(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* h, const float* W22, const float* b22,
                       const float* packws, const float* eps, const float* ll, const float* ent,
                       float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* gxT, float* gdT,
                       float* workspace, void* hip_stream);

/* ---- black-box MVN guide with per-person or shared Cholesky rows (VIRT.guide, x_feature > 1, vi.py:706-723).
 *   loc: [n_local][D];  M: [n_local][D][D] unconstrained (shared == 0) or [D][D] (shared == 1, share_cov=True)
 *   forward : x[nb][D] = loc[row] + L eps, eps[nb][D], ent[nb] = 0.5|eps|^2 + sum_k M_kk
 *   backward: gloc[n_local][D], gM (same shape as M) = d LOSS / d loc, M for the batch rows; the caller zeroes
 *             both buffers first (dense per-person gradients, zero off the batch; shared M accumulates). */
int vx_mvn_bbvi_forward(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, int64_t gid0, const float* loc,
                        const float* M, int32_t shared, const float* eps_in, float* x, float* eps, float* ent,
                        void* hip_stream);
int64_t vx_mvn_bbvi_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb, int32_t shared);
int vx_mvn_bbvi_backward(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* M, int32_t shared,
                         const float* gx, const float* eps, float* gloc, float* gM,
                         float* workspace /*shared == 1: per-block slabs, summed in fixed order into gM (overwritten)*/,
                         void* hip_stream);

/* ---- amortized Normal guide for ONE latent dimension (NormEncoder, vi.py:417-435; VaeIRT with
 * x_feature == 1, vi.py:677-684, and VaeCHoDina, vi.py:968-981).  cfg->J, cfg->H are used.
 *   forward : h[nb][H] = softplus(fc1 yin), loc[nb] = fc21 h, raw[nb] = fc22 h  (scale = exp(raw))
 *   backward: genc = d LOSS / d [W1: H*J | b1: H | W21: H | b21: 1 | W22: H | b22: 1] from
 *             gloc / graw = d LOSS / d loc, raw (as produced by vx_irt1d_grad / vx_hodina_grad). */
int64_t vx_norm_enc_param_floats(const vx_irt_cfg* cfg);
/* packws (optional): vx_norm_enc_pack_floats(cfg) floats of scratch, 16-byte aligned.  With it a large batch runs fc1 from
 * fp16-pair images of W1 made once per call (two small launches) instead of re-splitting W1 in every workgroup: 0.37 ->
 * 0.1x ms at 1M x 500.  NULL, or a batch below 4 096 persons: the kernels that need no scratch. */
int64_t vx_norm_enc_pack_floats(const vx_irt_cfg* cfg);           /* 0: this shape has no such kernel */
int vx_norm_enc_forward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                        const float* W1, const float* b1, const float* W21, const float* b21,
                        const float* W22, const float* b22, float* h, float* loc, float* raw,
                        float* packws /*or NULL*/, void* hip_stream);
int64_t vx_norm_enc_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb);
int vx_norm_enc_backward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                         const float* W21, const float* W22, const float* h, const float* gloc,
                         const float* graw, const uint8_t* yT /*[J][yT_stride] or NULL*/, int64_t yT_stride,
                         float* genc, float* workspace, void* hip_stream);

/* ---- D = 1 models on OBSERVED cells only (full batch; for heavily masked data, BASELINE config 4).  The responses
 * never change, so the host compacts them once (vipsy_amd/engine.py::_sparse_lists) into groups of 64 person SLOTS:
 *   pidx [n_groups][64] int32: the person (row of loc / raw / gloc / graw / elbo) in the slot, -1 = empty.  Any order
 *        works; lists of similar length in one group waste no lanes (the host sorts windows of persons by length);
 *   pent [n_groups][Lq][64][4] uint16: the slot's list in quads, entry = item | y << 15, 0xFFFF past its end
 *        (an empty slot's list is all 0xFFFF);
 *   glen [n_groups] int32: quads in the longest list of the group (<= Lq).
 * Same outputs as vx_irt1d_grad, one pass; item gradients are summed with integer atomics (bit-reproducible).
 * workspace: vx_irt1d_sparse_workspace_floats(cfg, n_groups) floats.  J <= 1024. */
int64_t vx_irt1d_sparse_workspace_floats(const vx_irt_cfg* cfg, int64_t n_groups);
int vx_irt1d_sparse_grad(const vx_irt_cfg* cfg, const uint16_t* pent, const int32_t* glen, int32_t Lq,
                         const int32_t* pidx, int64_t n_groups, int64_t gid0, const float* loc, const float* raw,
                         const float* eps_in, const float* a, const float* b, const float* c_un, const float* d_un,
                         float* gloc, float* graw, float* elbo, float* gitem, float* loss /*or NULL*/,
                         uint32_t* step_dev /*or NULL*/, float* workspace, void* hip_stream);

/* ---- HO-DINA with exact enumeration of the 2^K attribute patterns (VCHoDina / VaeCHoDina model,
 * vi.py:897-923, under TraceEnum_ELBO; guide theta ~ Normal(loc, exp(raw)), vi.py:925-934 / 968-981).
 *   q: [K][J] float 0/1 Q-matrix (vi.py:741);  lam0 [K], lam1_un [K] (positive -> exp), g_un / s_un [J]
 *   (interval(0,1) -> sigmoid).  K <= 10, J <= 1024.
 * Outputs: gloc / graw [nb] = d LOSS / d loc, raw;  elbo[nb] per-person ELBO terms (unscaled);
 *   gitem = d LOSS / d [g_un: J | s_un: J | lam0: K | lam1_un: K] for this rank's batch. */
typedef struct vx_hodina_cfg {
    int32_t K, J, H, _pad;
    float scale, _pad2;
    uint64_t seed;
    uint32_t step, stream;
    const uint32_t* step_dev; /* or NULL: the step counter in DEVICE memory (a captured step), read instead of `step`; vx_sum
                                 advances it behind the gradients, vx_adam_step reads it as t_dev */
} vx_hodina_cfg;
int64_t vx_hodina_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_hodina_grad(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                   const float* loc, const float* raw, const float* eps_in, const float* q,
                   const float* lam0, const float* lam1_un, const float* g_un, const float* s_un,
                   float* gloc, float* graw, float* elbo, float* gitem, float* workspace, void* hip_stream);

/* ---- VCCDM: pattern-enumerated DINA / DINO with the uniform pattern prior and an empty guide (vi.py:819-865;
 * dina vi.py:69-83, dino vi.py:86-101 -- the latter reproduced with its in-place sequencing: items that need a
 * single attribute always get eta = 0).  cfg: K, J, scale (seed / step / stream unused).
 *   elbo[nb] = log sum_c (1/C) prod_j Bern(y_ij | p_cj);  gitem = d LOSS / d [g_un: J | s_un: J]. */
int64_t vx_ccdm_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_ccdm_grad(const vx_hodina_cfg* cfg, int32_t dino, const uint8_t* y, const int64_t* rows, int64_t nb,
                 const float* q /*[K][J]*/, const float* g_un, const float* s_un, float* elbo, float* gitem,
                 float* workspace, void* hip_stream);

/* ---- VCDM / VaeCDM: Bernoulli-guide DINA / DINO with the score-function (REINFORCE) estimator (vi.py:726-816),
 * as pyro's Trace_ELBO treats a non-reparameterised guide site; cfg: K, J, scale, seed, step, stream.
 *   u[nb][K]        guide logits in batch order (rows of the `attr_p` leaf gathered by the host, or the encoder output);
 *                   clamp_t = 1 when they come from a unit_interval leaf (SigmoidTransform clamps the probability)
 *   attr_in[nb][K]  the 0/1 draws to replay, or NULL: drawn in the kernel (Philox block k >> 2, word k & 3 of the person)
 *   prior_p         probability of attr = 1 under the model prior BEFORE clamping -- 1.5 reproduces vi.py:753
 *   baseline        control variate subtracted from log_r in the score term, or NULL (pyro's Trace_ELBO: none); indexed
 *                   by the local person row (base_by_row = 1) or the batch position; base_beta >= 0 turns it into a per-person
 *                   decaying average: baseline <- beta baseline + (1 - beta) log_r after use (any baseline that does not
 *                   depend on the person's own draw keeps the estimator unbiased)
 * Outputs: log_r[nb] = scale (log prior + log lik - log q) per person; gu[nb][K] = d LOSS / d u (one particle, unaveraged);
 *   attr_out (optional) the draws; gitem = d LOSS / d [g_un: J | s_un: J].  Responses must be complete (0 / 1): the
 *   reference passes them unmasked (vi.py:756).  Item gradients come from integer (eta, y) counts: order-independent. */
int64_t vx_cdm_sf_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_cdm_sf_grad(const vx_hodina_cfg* cfg, int32_t dino, int32_t clamp_t, float prior_p, const uint8_t* y,
                   const int64_t* rows, int64_t nb, int64_t gid0, const float* q /*[K][J]*/, const float* g_un,
                   const float* s_un, const float* u, const uint8_t* attr_in, float* baseline, float base_beta,
                   int32_t base_by_row, float* gu, float* log_r, uint8_t* attr_out, float* gitem, float* workspace,
                   void* hip_stream);
/* leave-one-out control variate over the S >= 2 particles of a step: out[i] = mean_{s' != s} lr_all[s'][i] */
int vx_loo_baseline(const float* lr_all /*[S][nb]*/, int32_t S, int64_t nb, int32_t s, float* out, void* hip_stream);
/* BinEncoder of VaeCDM (vi.py:458-470): h[nb][H] = softplus(W1 yin + b1), u[nb][K] = W2 h + b2 (logits; H <= 128).
 * genc = d LOSS / d [W1: H*J | b1: H | W2: K*H | b2: K] from gu = d LOSS / d u. */
int64_t vx_bin_enc_param_floats(const vx_hodina_cfg* cfg);
int vx_bin_enc_forward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W1,
                       const float* b1, const float* W2, const float* b2, float* h, float* u, void* hip_stream);
int64_t vx_bin_enc_bwd_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_bin_enc_backward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W2,
                        const float* h, const float* gu, float* genc, float* workspace, void* hip_stream);

/* ---- synthetic response matrices with the distributions of the reference's Random* generators (vi.py:120-412), written
 * straight into the uint8 storage contract; benchmark / test INPUT (never in a timed region).  Every draw is a Philox word
 * keyed by the GLOBAL person id (gid0 + row): a data set does not depend on the sharding.  cfg->seed keys the draws.
 *   vx_synth_irt: y ~ Bern(c + (d - c) sigmoid(Dc (x.a + b))); x = x_in or N(0, 1) drawn here (x_out optional);
 *                 `missing` = MCAR rate of 255 cells.  a [D][J], b / c / d [J] are the CONSTRAINED item parameters.
 *   vx_synth_cdm: DINA / DINO (the reference's dino(), vi.py:86-101) / HO-DINA responses; attributes ~ Bern(attr_p) or
 *                 Bern(sigmoid(theta lam1 + lam0)), theta ~ N(0, 1) (hodina = 1); attr_out [nb][K], theta_out [nb] optional. */
int vx_synth_irt(const vx_irt_cfg* cfg, int64_t nb, int64_t gid0, const float* x_in, const float* a, const float* b,
                 const float* c, const float* d, float missing, uint8_t* y, float* x_out, void* hip_stream);
int vx_synth_cdm(const vx_hodina_cfg* cfg, int32_t dino, int32_t hodina, float attr_p, int64_t nb, int64_t gid0,
                 const float* q, const float* g, const float* s, const float* lam0, const float* lam1, float missing,
                 uint8_t* y, uint8_t* attr_out, float* theta_out, void* hip_stream);

/* ---- VaeCCDM (vi.py:866-891): enumerated DINA / DINO whose pattern prior is Categorical(attr_p[i]), attr_p =
 * softmax(fc2(relu(fc1(data_))), dim = 0) -- the SoftmaxEncoder (vi.py:473-485) normalises over the BATCH -- and whose missing
 * responses stay in the observation as -1 (no mask, vi.py:882-891).  C = 2^K patterns; cfg: K, J, H, scale.  One step =
 *   vx_sm_enc_forward                      h[nb][H] = relu(..), z[nb][C] = fc2 scores
 *   vx_col_reduce(0, z) -> m[C]            column maximum over the batch          [+ all-reduce MAX over the ranks]
 *   vx_col_reduce(1, z, shift = m) -> Z[C] column sum of exp(z - m)               [+ all-reduce SUM]; off = m + log Z (host)
 *   vx_vaeccdm_grad                        elbo[nb], gitem, gla[nb][C] = d ELBO / d log attr_p (scaled)
 *   vx_col_reduce(2, gla) -> T[C]          column sums                            [+ all-reduce SUM]
 *   vx_sm_enc_backward                     genc = d LOSS / d [W1: H*J | b1: H | W2: C*H | b2: C]  (overwrites gla) */
int64_t vx_sm_enc_param_floats(const vx_hodina_cfg* cfg);
int vx_sm_enc_forward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W1,
                      const float* b1, const float* W2, const float* b2, float* h, float* z, void* hip_stream);
int64_t vx_col_reduce_workspace_floats(int64_t nb, int32_t C);
int vx_col_reduce(int32_t mode /*0 max, 1 sum exp(v - shift), 2 sum*/, const float* v /*[nb][C]*/, int64_t nb, int32_t C,
                  const float* shift /*[C], mode 1*/, float* out /*[C]*/, float* workspace, void* hip_stream);
int64_t vx_vaeccdm_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_vaeccdm_grad(const vx_hodina_cfg* cfg, int32_t dino, const uint8_t* y, const int64_t* rows, int64_t nb,
                    const float* q, const float* g_un, const float* s_un, const float* z /*[nb][C]*/,
                    const float* off /*[C]*/, float* elbo, float* gla /*[nb][C]*/, float* gitem, float* workspace,
                    void* hip_stream);
int64_t vx_sm_enc_bwd_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb);
int vx_sm_enc_backward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W2,
                       const float* h, const float* z, const float* off, const float* T, float* gla, float* genc,
                       float* workspace, void* hip_stream);

/* ---- Person scores by quadrature over a fixed grid of latent nodes (no reference counterpart: the reference stops at fit()).
 * For a response row y_i and G nodes with normalised log-weights logw[G] and coordinates coord[G][D]:
 *     ll[i][g]  = sum_j log P(y_ij | node g)                      (missing cells: the reference's constant, as in the step)
 *     loglik[i] = log sum_g exp(logw[g] + ll[i][g])               the marginal log-likelihood of the row
 *     mean[i][D], sd[i][D]                                        posterior mean (EAP) and standard deviation (PSD) of coord
 *     argmax[i]                                                   the node that maximises logw + ll (ties: the lowest index)
 * Exact and deterministic -- no guide, no random numbers: the item parameters are all it takes, so respondents that were
 * not in the training data are scored like those that were.  Two steps:
 *   1. vx_grid_table_irt / vx_grid_table_cdm fill `img` (vx_grid_image_bytes(J, G) bytes, 16-byte aligned) with the tables
 *      T1[j][g] = log P(y_j = 1 | g), T0[j][g] = log P(y_j = 0 | g) as the fp16-pair operand image of the main kernel.
 *        IRT: nodes theta[G][D]; item parameters as the step kernels take them (a [D][J] -- unused for 1PL, which needs D = 1 --,
 *             b, unconstrained c_un / d_un for 3PL / 4PL); z = Dc (theta_g . a_j + b_j) through the cell of the step kernels.
 *             cfg: model, D, J, Dc.
 *        DINA / DINO: the nodes are the G = 2^K patterns in the order of all_attrs (bit k of g = attribute k; their coordinates
 *             are the attribute bits, D = K); q, g_un, s_un as vx_ccdm_grad takes them; dino: 0 / 1.  cfg: K, J.
 *   2. vx_grid_posterior: rows (or NULL) picks the persons, y is [n_local][J] (254 = a cell outside the problem: adds nothing).
 *      The log-likelihoods are a GEMM of 0/1 indicators with the tables on v_mfma_f32_32x32x16_f16; node tiles are combined by
 *      an online log-sum-exp with the moments taken about the running MAP node, nothing of size [nb][G] touches memory, and
 *      every sum runs in a fixed order: the same call gives the same bits, and a person gives the same bits through `rows`.
 * Limits: 1 <= J <= 1024, 1 <= G <= 1024, 1 <= D (K) <= 10, nb >= 1; VX_EINVAL beyond them. */
int64_t vx_grid_image_bytes(int32_t J, int32_t G);
int vx_grid_table_irt(const vx_irt_cfg* cfg, const float* theta /*[G][D]*/, int32_t G, const float* a /*[D][J] or NULL (1PL)*/,
                      const float* b /*[J]*/, const float* c_un /*[J] or NULL*/, const float* d_un /*[J] or NULL*/,
                      void* img, void* hip_stream);
int vx_grid_table_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q /*[K][J]*/, const float* g_un, const float* s_un,
                      void* img, void* hip_stream);
int vx_grid_posterior(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                      int32_t D, const void* img, const float* logw /*[G]*/, const float* coord /*[G][D]*/,
                      float* loglik /*[nb]*/, float* mean /*[nb][D]*/, float* sd /*[nb][D]*/, int32_t* argmax /*[nb]*/,
                      void* hip_stream);

/* ---- Grid scores of a bifactor / testlet model: one general dimension every item loads on and S specific dimensions, each loaded
 * on by the items of one testlet only.  Given the general node the testlets are independent, and each is a one-dimensional
 * integral over its own specific factor (Gibbons & Hedeker 1992), so with Gg general nodes (logw, coord) and Gh specific nodes
 * (logv, u; both sets of log-weights normalised)
 *     m[i][s][g] = log sum_h exp(logv[h] + sum_{j in s} log P(y_ij | coord[g], u[h]))     the bracket of testlet s
 *     F[i][g]    = logw[g] + (#missing_i) VX_LOGP_MISSING + sum_s m[i][s][g]              (the constant enters once)
 *     loglik[i]  = log sum_g exp(F[i][g])                                              the marginal log-likelihood of the row
 *     mean[i], sd[i]                     EAP and PSD of the general dimension: the moments of coord under post[i][g] = exp(F - loglik)
 *     argmax[i]                          the node that maximises F, the general MARGINAL posterior (ties: the lowest index)
 *     mean_s[s][i] = sum_g post[i][g] E[u | g, y_is],  E[u | g, y_is] = sum_h u[h] exp(logv[h] + ll_is(g, h) - m[i][s][g])
 *     sd_s[s][i]   = sqrt(sum_g post[i][g] E[u^2 | g, y_is] - mean_s^2)
 * -- the work of ONE two-dimensional grid whatever S is: nothing of size Gg Gh^S exists anywhere.
 * Testlet layout: the items testlet after testlet, each padded to whole chunks of 16; testlet t holds the chunks tl_start[t] ..
 * tl_start[t + 1] - 1 of the KC = tl_start[n_tl] chunks; the items that load on the general dimension alone form one more
 * (pseudo-)testlet, whose table does not depend on h.  Slot jp of the layout holds item col[jp] of the model (-1: padding) whose
 * specific dimension is sdim[jp] (-1: none).  tl_start is read on the HOST (int32 [n_tl + 1], strictly increasing from 0 to KC; it
 * is checked, and not used after the call returns); tl_start_dev is the same table in device memory.
 *   1. vx_grid_table_bifactor fills `img` (vx_grid_bifactor_image_bytes(Gg, KC) bytes, 16-byte aligned): [Gg][KC][4: T1 head, T1
 *      low, T0 head, T0 low][64 lanes][8 fp16], the layout of vx_grid_table_irt with the general node in the place of the node
 *      tile and the specific node h in the place of the node in it; rows >= Gh and padding slots are zero.  z = Dc (b_j +
 *      a[general][j] coord[g] + a[sdim][j] u[h]) through the cell of the step kernels; a [D][J], b, c_un, d_un as the step takes
 *      them.  cfg: model (2 .. 4), D (>= 2), J, Dc.  col and sdim are int32 [16 KC] in DEVICE memory.
 *   2. vx_grid_bifactor: y is [nb][16 KC] u8 IN THE TESTLET LAYOUT (the caller permutes the columns; padding slots hold 254).
 *      fws NULL, or vx_grid_bifactor_workspace_floats(nb, Gg) floats that receive F, [unit of 64 persons][Gg][64].
 *   3. vx_grid_bifactor_specific (optional): same y, layout, image; loglik and fws as step 2 left them.  mean_s, sd_s are
 *      [n_tl][nb], the pseudo-testlet's row included.  It recomputes the tiles: the MFMA work of step 2 once more.
 * The sums of a testlet run on v_mfma_f32_32x32x16_f16 (fp16 head + low of T 2^10, four MFMAs a chunk), the person on the lane;
 * the log-sum-exp over h is a loop over the lane's accumulator registers and one exchange with lane ^ 32.  Nothing of size
 * [nb][Gg Gh] touches memory, there are no atomics, and every sum runs in a fixed order (chunks, h, testlets, g ascending) that
 * depends on neither the person's place in the batch nor the launch: the same call gives the same bits.
 * Limits: 2 <= Gg <= 256, 1 <= Gh <= 32, 1 <= n_tl <= KC <= 1024, 1 <= J <= 1024, 2 <= D <= 4096, 0 <= general < D, nb >= 1, image
 * <= 512 MB; VX_EINVAL beyond them. */
int64_t vx_grid_bifactor_image_bytes(int32_t Gg, int32_t KC);
int64_t vx_grid_bifactor_workspace_floats(int64_t nb, int32_t Gg);
int vx_grid_table_bifactor(const vx_irt_cfg* cfg, const float* coord /*[Gg]*/, int32_t Gg, const float* u /*[Gh]*/, int32_t Gh,
                           int32_t general, const int32_t* col /*[16 KC], device*/, const int32_t* sdim /*[16 KC], device*/,
                           int32_t KC, const float* a /*[D][J]*/, const float* b /*[J]*/, const float* c_un /*[J] or NULL*/,
                           const float* d_un /*[J] or NULL*/, void* img, void* hip_stream);
int vx_grid_bifactor(const uint8_t* y /*[nb][16 KC]*/, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh,
                     const int32_t* tl_start /*[n_tl + 1], HOST*/, int32_t n_tl, const int32_t* tl_start_dev /*[n_tl + 1]*/,
                     const void* img, const float* logw /*[Gg]*/, const float* coord /*[Gg]*/, const float* logv /*[Gh]*/,
                     const float* u /*[Gh]*/, float* loglik /*[nb]*/, float* mean /*[nb]*/, float* sd /*[nb]*/,
                     int32_t* argmax /*[nb]*/, float* fws /*or NULL*/, void* hip_stream);
int vx_grid_bifactor_specific(const uint8_t* y /*[nb][16 KC]*/, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh,
                              const int32_t* tl_start /*[n_tl + 1], HOST*/, int32_t n_tl, const int32_t* tl_start_dev,
                              const void* img, const float* logv /*[Gh]*/, const float* u /*[Gh]*/, const float* loglik /*[nb]*/,
                              const float* fws, float* mean_s /*[n_tl][nb]*/, float* sd_s /*[n_tl][nb]*/, void* hip_stream);

/* ---- Expected counts of a bifactor / testlet model (the Bock-Aitkin E-step of a marginal maximum-likelihood fit), in the notation
 * above, with ll_is(g, h) the log-likelihood of testlet s at (coord[g], u[h]), loglik and fws (F) as vx_grid_bifactor left them:
 *     post[i][g]      = exp(F[i][g] - loglik[i])                           r_is(g, h) = exp(logv[h] + ll_is(g, h) - m[i][s][g])
 *     n1[j][g Gh + h] = sum_i [y_ij == 1] post[i][g] r_{i,s(j)}(g, h)       n0 likewise with [y_ij == 0]
 *     mass[g]         = sum_i post[i][g]                                   mass_s[t][g Gh + h] = sum_i post[i][g] r_it(g, h)
 * Given the general node the posterior of a testlet over (g, h) is a two-dimensional table and every item belongs to one testlet,
 * so an item's counts live on the Gg x Gh grid of its own testlet whatever S is; an item of the pseudo-testlet has r = exp(logv[h]).
 * y, the layout, tl_start / tl_start_dev, col (int32 [16 KC], device), img, logv as vx_grid_bifactor and vx_grid_table_bifactor
 * take them.  n1, n0 are [J][Gg Gh] in the MODEL's item order (slot jp of the layout goes to item col[jp]; every item must hold
 * one slot), mass_s [n_tl][Gg Gh] in the layout's testlet order, the pseudo-testlet included, or NULL.  accumulate = 0: the tables
 * are written; 1: this call's sums are added to what they hold -- a caller that loops over slabs of persons gets their sum in
 * person order.  255 enters neither table, 254 adds nothing, a person with no response adds their prior to mass and mass_s.
 * m and r are formed with the arithmetic that formed F, so a person's weights sum to 1 to rounding.  The contraction over persons
 * runs on v_mfma_f32_32x32x16_f16 (p 2^14 as an fp16 head and low term, fp32 accumulation), [y == 1] and [y == 0] of a chunk of
 * 16 items in the two halves of one fragment.  Nothing of size [nb][Gg Gh] touches memory.  No float atomics: the partial tables
 * of the person chunks go to slabs in `workspace` (vx_grid_bifactor_counts_workspace_floats(nb, KC, Gg, n_tl) floats, 16-byte
 * aligned) and are added in ascending order; every sum has a fixed order and the same call gives the same bits.  The cut of the
 * persons depends on (nb, Gg) alone: a testlet's tables do not depend on the other testlets of the layout except through F and
 * loglik.  Limits as vx_grid_bifactor, accumulate in {0, 1}; VX_EINVAL beyond them and for NULL or misaligned pointers. */
int64_t vx_grid_bifactor_counts_workspace_floats(int64_t nb, int32_t KC, int32_t Gg, int32_t n_tl);
int vx_grid_bifactor_counts(const uint8_t* y /*[nb][16 KC]*/, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh,
                            const int32_t* tl_start /*[n_tl + 1], HOST*/, int32_t n_tl, const int32_t* tl_start_dev,
                            const int32_t* col /*[16 KC], device*/, int32_t J, const void* img, const float* logv /*[Gh]*/,
                            const float* loglik /*[nb]*/, const float* fws, int32_t accumulate, float* n1 /*[J][Gg Gh]*/,
                            float* n0 /*[J][Gg Gh]*/, float* mass /*[Gg]*/, float* mass_s /*[n_tl][Gg Gh] or NULL*/,
                            float* workspace, void* hip_stream);

/* ---- Plausible values: draws of a person's node from the grid posterior p_i(g) ~ exp(logw[g] + ll[i][g]) of vx_grid_posterior
 * (same y, rows, nb, img, logw), by the Gumbel-max rule: node[i][m] = argmax_g (logw[g] + ll[i][g] + noise(r, g, m)), ties to the
 * lowest g.  No normalisation, no second pass, nothing of size [nb][G] touches memory, no workspace, no atomics.  The noise is
 * counter-based: with r = row_offset + row (row = rows[i] where rows is given, else i) and m the absolute draw index,
 *     w = philox4x32_10(lo32(r), hi32(r), g, (PV_STREAM << 16) | (m >> 2); key lo32(seed), hi32(seed)),   x = word m & 3 of w,
 *     u = ((x >> 9) + 0.5) 2^-23  (exact in float32, 2^-24 <= u <= 1 - 2^-24),   noise = -log(-log(u)),
 * so a draw depends on (seed, r, g, m) alone: not on the batch, on `rows`, or on how the draws are cut into launches (16 a
 * launch, k_grid_draw.hip).  Writes node[i * stride + m] for draw0 <= m < draw0 + ndraws and nothing else.
 * Limits: those of vx_grid_posterior (1 <= J <= 1024, 1 <= G <= 1024, nb >= 1), 1 <= ndraws, draw0 >= 0,
 * draw0 + ndraws <= stride, draw0 + ndraws <= 1024; VX_EINVAL beyond them. */
int vx_grid_draw(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                 const void* img, const float* logw /*[G]*/, uint64_t seed, int64_t row_offset, int32_t draw0, int32_t ndraws,
                 int64_t stride, int32_t* node /*[nb][stride]*/, void* hip_stream);

/* ---- Conditioned grid posteriors and draws: vx_grid_posterior / vx_grid_draw under a prior that differs from person to person,
 * theta_i ~ N(mu_i, Sigma) (the latent regression mu_i = Gamma^T x_i of IrtEngine.fit_population).  On the grid its log density is
 * logw[g] + tilt[i] . coord[g] + const_i with logw[g] = -1/2 coord[g]^T Sigma^-1 coord[g] (any shift) and tilt[i] = Sigma^-1 mu_i,
 * [nb][D] by BATCH POSITION (row i of the call, not rows[i]).  With f[i][g] = (logw[g] + ll[i][g]) + tilt[i] . coord[g] and
 * h[i][g] = logw[g] + tilt[i] . coord[g]:
 *     logjoint[i] = log sum_g exp f[i][g]      lognorm[i] = log sum_g exp h[i][g]      (loglik_i = logjoint[i] - lognorm[i])
 *     mean[i][D], argmax[i]                    as vx_grid_posterior, of this f
 *     cov[i][D (D + 1) / 2]                    the posterior covariance of coord, upper triangle row by row (00, 01, 02, 11, 12, 22)
 * A zero tilt gives vx_grid_posterior's loglik, mean and argmax in logjoint, mean and argmax bit for bit, sqrtf(cov_dd) its sd, and
 * vx_grid_draw's nodes; noise, keys (seed, row_offset + row, node, draw) and ties of the draws are vx_grid_draw's, and a draw does
 * not depend on how the draws are cut into launches.  No atomics, no workspace, every sum in a fixed order: the same call gives the
 * same bits, and a person gives the same bits through `rows`.
 * Limits: those of vx_grid_posterior / vx_grid_draw with 1 <= D <= 3; VX_EINVAL beyond them. */
int vx_grid_posterior_cond(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                           int32_t D, const void* img, const float* logw /*[G]*/, const float* coord /*[G][D]*/,
                           const float* tilt /*[nb][D]*/, float* logjoint /*[nb]*/, float* lognorm /*[nb]*/, float* mean /*[nb][D]*/,
                           float* cov /*[nb][D (D + 1) / 2]*/, int32_t* argmax /*[nb]*/, void* hip_stream);
int vx_grid_draw_cond(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                      int32_t D, const void* img, const float* logw /*[G]*/, const float* coord /*[G][D]*/,
                      const float* tilt /*[nb][D]*/, uint64_t seed, int64_t row_offset, int32_t draw0, int32_t ndraws,
                      int64_t stride, int32_t* node /*[nb][stride]*/, void* hip_stream);

/* ---- Expected counts from the grid posteriors (the Bock-Aitkin E-step; the per-item half of what vx_grid_posterior gives per
 * person).  With p_i(g) = exp(logw[g] + ll[i][g] - loglik[i]), loglik being vx_grid_posterior's output for the same y, rows, nb,
 * img and logw:
 *     n1[j][g] = sum_i p_i(g) [y_ij == 1]      n0[j][g] = sum_i p_i(g) [y_ij == 0]      mass[g] = sum_i p_i(g)
 * They are the gradient of sum_i loglik[i] with respect to the tables T1 / T0, the data of the empirical item characteristic
 * curve and of the RMSD / MD item-fit statistics, and (mass) the estimated latent distribution.  A 255 cell adds the missing
 * constant to ll and enters neither table, a 254 cell adds nothing anywhere; a person with no response adds their prior to mass.
 * Two chained products on v_mfma_f32_32x32x16_f16 (p as an fp16 pair), nothing of size [nb][G] touches memory; the persons go
 * to chunks whose slabs (workspace: vx_grid_counts_workspace_floats(nb, J, G) floats) are added in a fixed order, no atomics:
 * the same call gives the same bits.  Limits as vx_grid_posterior: 1 <= J <= 1024, 1 <= G <= 1024, nb >= 1; VX_EINVAL beyond. */
int64_t vx_grid_counts_workspace_floats(int64_t nb, int32_t J, int32_t G);
int vx_grid_counts(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                   const void* img, const float* logw /*[G]*/, const float* loglik /*[nb]*/, float* n1 /*[J][G]*/,
                   float* n0 /*[J][G]*/, float* mass /*[G]*/, float* workspace, void* hip_stream);

/* ---- Expected counts under a prior of each person's own, a table set a SEGMENT of the persons: vx_grid_counts for the
 * conditioned posterior of vx_grid_posterior_cond, and the E-step of the item-by-group fit statistics (differential item
 * functioning).  With p_i(g) = exp(f[i][g] - logjoint[i]), f[i][g] = (logw[g] + ll[i][g]) + tilt[i] . coord[g] as defined there
 * and logjoint that entry's output for the same y, rows, nb, img, logw, coord and tilt (tilt and logjoint by BATCH POSITION), the
 * batch positions are cut into n_seg consecutive segments [seg_start[s], seg_start[s + 1]) and
 *     n1[s][j][g] = sum_{i in s} p_i(g) [y_ij == 1]    n0[s][j][g] = sum_{i in s} p_i(g) [y_ij == 0]    mass[s][g] = sum_{i in s} p_i(g)
 * An empty segment (equal neighbours in seg_start) gets zeros.  Response bytes as vx_grid_counts; a person with no response adds
 * exp(h[i][g] - lognorm[i]), their conditioned prior, to the mass of their segment.
 * seg_start is HOST memory, int64 [n_seg + 1]: the call checks it, plans the launch from it and hands the plan to the device
 * in kernel arguments -- it is not read after the call returns, nothing is copied, allocated or waited for.  ONE launch covers
 * all segments: a workgroup never mixes two; the chunks of a segment write slabs of their own into the workspace
 * (vx_grid_counts_cond_workspace_floats(nb, n_seg, J, G) floats, 16-byte aligned: enough for any cut of nb into n_seg segments),
 * which a second launch adds in ascending order.  No atomics, every sum in a fixed order: the same call gives the same bits, and a
 * segment's tables do not depend on the other segments' persons.  With n_seg = 1 and a zero tilt the three tables are
 * vx_grid_counts' bit for bit (logjoint = its loglik).
 * Limits: those of vx_grid_counts, 1 <= D <= 3, 1 <= n_seg <= 4096, seg_start[0] = 0, seg_start[n_seg] = nb, seg_start
 * non-decreasing; VX_EINVAL beyond any of them. */
int64_t vx_grid_counts_cond_workspace_floats(int64_t nb, int32_t n_seg, int32_t J, int32_t G);
int vx_grid_counts_cond(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G,
                        int32_t D, const void* img, const float* logw /*[G]*/, const float* coord /*[G][D]*/,
                        const float* tilt /*[nb][D]*/, const float* logjoint /*[nb]*/, const int64_t* seg_start /*HOST [n_seg + 1]*/,
                        int32_t n_seg, float* n1 /*[n_seg][J][G]*/, float* n0 /*[n_seg][J][G]*/, float* mass /*[n_seg][G]*/,
                        float* workspace, void* hip_stream);

/* ---- The M-step of the Bock-Aitkin EM on those tables (marginal maximum likelihood of the item parameters; with the E-step of
 * vx_grid_posterior + vx_grid_counts one EM iteration).  Every item is a problem of its own; a and b / g_un and s_un are updated
 * in place, [D][J] / [J] as the table builders take them, and nothing else is written.
 *   vx_grid_mstep_irt (cfg: model 1 | 2, D <= 3, J, Dc): item j maximises
 *         Q_j = sum_g n1[j][g] log P_j(g) + n0[j][g] log(1 - P_j(g)),   z = Dc (theta_g . a_j + b_j)   (1PL: z = Dc (theta_g + b_j))
 *     through the cell of the tables (z clamped to +-logit(1 - eps32); a clamped node adds nothing to gradient or curvature) by
 *     `newton` Newton (= Fisher scoring) steps inside the one launch, one wave an item.  a_free[d][j] == 0 takes that loading out
 *     of the system: it is not written.  A step is accepted when Q does not fall by more than 1e-6 |Q|, else halved, at most 8
 *     times, else the item stops; a step longer than 4 in its largest component is scaled down to 4 (an item whose observed
 *     answers are all equal has its maximum at infinity: it ends finite, with every node at the clamp).  An item nobody answered
 *     (sum_g n = 0) or a pivot that is not positive: the values keep their bits.  A parameter left where the clamp is active
 *     everywhere has zero gradient in the step kernels afterwards.
 *   vx_grid_mstep_cdm (cfg: K, J; dino, q as vx_grid_table_cdm): the closed form.  With R0 / W0 = the sums of n1 / n0 over the
 *     patterns of eta = 0 and R1 / W1 those over eta = 1 (eta as the tables have it, DINO's single-attribute rule included):
 *         g_un[j] = log R0 - log W0      s_un[j] = log W1 - log R1      clamped to +-logit(1 - eps32);
 *     a class without mass (R + W = 0) leaves its parameter untouched.
 * Every sum runs in a fixed order, no atomics: the same call gives the same bits.
 * Limits: 1 <= J <= 1024, 1 <= G <= 1024, 1 <= D <= 3, model 1 or 2, 1 <= newton <= 64, K <= 10; VX_EINVAL beyond. */
int vx_grid_mstep_irt(const vx_irt_cfg* cfg, const float* theta /*[G][D]*/, int32_t G, const float* n1 /*[J][G]*/,
                      const float* n0 /*[J][G]*/, const float* a_free /*[D][J] or NULL = all free*/,
                      float* a /*[D][J] in/out, NULL for 1PL*/, float* b /*[J] in/out*/, int32_t newton, void* hip_stream);
int vx_grid_mstep_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q /*[K][J]*/, const float* n1 /*[J][2^K]*/,
                      const float* n0 /*[J][2^K]*/, float* g_un /*[J] in/out*/, float* s_un /*[J] in/out*/, void* hip_stream);

/* ---- The penalised M-step (Bayes-modal EM; k_grid_mstep_map.hip): vx_grid_mstep_irt for models 1 .. 4 with a normal prior on
 * every unknown.  Item j maximises, over p = (b, a_0 .. a_{D-1}, c_un, d_un) as far as the model has them,
 *         Q_j = sum_g n1[j][g] log P_j(g) + n0[j][g] log Q_j(g) - 1/2 sum_k prec_k (p_k - mean_k)^2
 * by `newton` steps of Fisher scoring inside the one launch, one wave an item.  1PL / 2PL: the cell of vx_grid_mstep_irt.
 * 3PL / 4PL: P = c + (d - c) s(z), Q = (1 - d) + (d - c) s(-z) in the arithmetic of the tables (c, d and 1 - d from the logits,
 * capped as vx_grid_table_irt caps them; P and Q clamped to [eps32, 1 - eps32], a clamped node adds its log term and nothing to
 * gradient or curvature).  d <= c is not excluded by a constraint: the prior keeps the asymptotes apart.
 * Step control is vx_grid_mstep_irt's, applied to the penalised Q_j (1e-6 |Q_j|, at most 8 halvings, cap 4).  a_free[d][j] == 0:
 * that loading is not an unknown and is not written.  An item nobody answered keeps its bits; on a pivot that is not positive
 * or not finite an item stops where it is.  a, b, c_un, d_un are updated in place; nothing else is written but lprior.
 *   prior   float [2][6][J] on the device: prior[k][j] the mean and prior[6 + k][j] the precision (1 / sd^2) of unknown k of item
 *           j; k = 0: b, 1 .. 3: a_0 .. a_2, 4: c_un, 5: d_un -- six rows each in every model; rows of unknowns the model, D or
 *           a_free does not have are not read.  Precision 0 = no prior on that unknown (its mean must still be finite).  The
 *           precisions must be >= 0 and finite; the call cannot look into device memory, so this is the caller's duty.
 *   lprior  NULL or float [J]: -1/2 sum_k prec_k (p_k - mean_k)^2 over the item's free unknowns at the parameters the call
 *           STARTED from (constants dropped); written for every item, answered or not.
 * Every sum runs in a fixed order, no atomics: the same call gives the same bits, and an item's bits do not depend on the other
 * items of the launch.
 * Limits: model 1 .. 4 (c_un from 3, d_un for 4, a from 2), 1 <= D <= 3, 1 <= J <= 1024, 1 <= G <= 1024, 1 <= newton <= 64,
 * prior not NULL; VX_EINVAL beyond. */
int vx_grid_mstep_irt_map(const vx_irt_cfg* cfg, const float* theta /*[G][D]*/, int32_t G, const float* n1 /*[J][G]*/,
                          const float* n0 /*[J][G]*/, const float* a_free /*[D][J] or NULL = all free*/,
                          float* a /*[D][J] in/out, NULL for 1PL*/, float* b /*[J] in/out*/, float* c_un /*[J] in/out, model >= 3*/,
                          float* d_un /*[J] in/out, model 4*/, const float* prior /*[2][6][J]*/, int32_t newton,
                          float* lprior /*[J] or NULL*/, void* hip_stream);

/* ---- The cross-product (BHHH) information of the item parameters from the grid posteriors: with Fisher's identity the marginal
 * score of person i for parameter k of item j is
 *     s_i[(j,k)] = sum_g p_i(g) ( [y_ij == 1] W1[g][(j,k)] - [y_ij == 0] W0[g][(j,k)] ),   W1 = (1 - P_j(g)) u_jgk,  W0 = P_j(g) u_jgk,
 * p_i(g) as vx_grid_counts forms it, u_g = Dc (1, theta_g) for the IRT links, ([eta = 0], -[eta = 1]) for DINA / DINO on the
 * unconstrained g / s scale.  info = sum_i s_i s_i^T [P][P], symmetric bit for bit, over the DENSE parameter layout: column
 * c = j K + k with K = D + 1 (k = 0: b, k = 1 + d: a_d) for 2PL, 1 for 1PL, 2 (g_un, s_un) for DINA / DINO; 3PL / 4PL (the tables of
 * vx_grid_wtable_irt_map) add k = D + 1: c_un and, for 4PL, k = D + 2: d_un, K = D + 2 / D + 3 <= 6; P = J K <= 4096;
 * gradient = sum_i s_i [P], the gradient of the marginal log-likelihood -- by construction what the M-step of vx_grid_mstep_irt
 * forms from n1 / n0: P, 1 - P and the clamp come from its cell (a node where the z clamp is active contributes 0).  Both are taken
 * AT THE PARAMETERS AS THEY STAND; the inverse of info is a covariance only at the marginal maximum.
 *   1. vx_grid_wtable_irt (cfg: model 1 | 2, D <= 3, J, Dc) / vx_grid_wtable_cdm (cfg: K, J) fill `wimg` (vx_grid_wimage_bytes(P, G)
 *      bytes, 16-byte aligned) with W1 / W0 as fp16-pair operand images, scaled by a power of two that the image carries.
 *      vx_grid_wtable_irt_map (cfg: model 1 .. 4) is the table at the fit of vx_grid_mstep_irt_map.  Models 1 and 2: the image of
 *      vx_grid_wtable_irt, byte for byte.  Models 3 and 4: the cell of that M-step (c, d, 1 - d capped, P = c + (d - c) s(z),
 *      Q = (1 - d) + (d - c) s(-z), a node with P or Q below eps32 contributes 0), W1 = v / P and W0 = v / Q with v the derivative
 *      of P: (d - c) s(z) s(-z) Dc (1, theta_g) for b and a, s(-z) c (1 - c) for c_un, s(z) d (1 - d) for d_un.  `gradient` is then
 *      the likelihood part of what vx_grid_mstep_irt_map forms from n1 / n0.  A 3PL entry stays below max(1, Dc max(1, |theta|_inf)),
 *      but a 4PL entry grows like 1 / (d - c) and d <= c is admissible: the power of two comes from the table's own largest
 *      magnitude, found in a first pass by an integer maximum (no float atomics: the same call gives the same bits), and the
 *      image carries |W 2^s| < 2^15.  It refuses J K > 4096.
 *   2. vx_grid_info: y, rows, nb, img, logw as vx_grid_posterior took them and loglik as it returned it.  Three chained products on
 *      v_mfma_f32_32x32x16_f16 (fp16 pairs, fp32 accumulation): the log-likelihoods, p W (over nodes) and S^T S (over persons).
 *      Nothing of size [nb][G] touches memory; S [persons][P] lives in `workspace` as fp16 pairs, a slab of persons (a multiple of
 *      256) at a time -- as many as ws_floats allow --, and the slabs' matrices are added in person order.  No atomics: the same
 *      call with the same ws_floats gives the same bits.  vx_grid_info_workspace_floats(nb, P, G): the preferred size (one slab
 *      where 512 MB allow it); vx_grid_info_workspace_min_floats(P, G): the smallest accepted.  workspace is 16-byte aligned.
 * Persons' 254 / 255 cells contribute nothing.  Limits: 1 <= J <= 1024, 1 <= G <= 1024, 1 <= K <= 6, J K <= 4096, nb >= 1, ws_floats at least the
 * minimum; VX_EINVAL beyond. */
int64_t vx_grid_wimage_bytes(int32_t P, int32_t G);
int vx_grid_wtable_irt(const vx_irt_cfg* cfg, const float* theta /*[G][D]*/, int32_t G, const float* a /*[D][J] or NULL (1PL)*/,
                       const float* b /*[J]*/, void* wimg, void* hip_stream);
int vx_grid_wtable_irt_map(const vx_irt_cfg* cfg, const float* theta /*[G][D]*/, int32_t G, const float* a /*[D][J] or NULL (1PL)*/,
                           const float* b /*[J]*/, const float* c_un /*[J], model >= 3*/, const float* d_un /*[J], model 4*/,
                           void* wimg, void* hip_stream);
int vx_grid_wtable_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q /*[K][J]*/, const float* g_un, const float* s_un,
                       void* wimg, void* hip_stream);
int64_t vx_grid_info_workspace_floats(int64_t nb, int32_t P, int32_t G);
int64_t vx_grid_info_workspace_min_floats(int32_t P, int32_t G);
int vx_grid_info(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J, int32_t G, int32_t K,
                 const void* img, const void* wimg, const float* logw /*[G]*/, const float* loglik /*[nb]*/, float* info /*[P][P]*/,
                 float* gradient /*[P]*/, float* workspace, int64_t ws_floats, void* hip_stream);

/* ---- Local dependence: the pairwise-complete residual sums behind Yen's Q3.  With m_ij = [y_ij < 2] (254 / 255 cells are not
 * observed), r_ij = m_ij (y_ij - P_ij) and I_jk the persons with m_ij m_ik = 1, four float32 tables [J][J] on the device:
 *     n[j][k] = |I_jk|     s[j][k] = sum_{I_jk} r_ij     ss[j][k] = sum_{I_jk} r_ij^2     sp[j][k] = sum_{I_jk} r_ij r_ik
 * n and sp are symmetric bit for bit (computed for the upper triangle and mirrored); s and ss belong to the ROW item and are not.
 * From them cov = sp - s s^T / n, v = ss - s^2 / n, q3 = cov / sqrt(v v^T) (float64 on the host: vipsy_amd.grid.pair_q3_host).
 *   vx_grid_pairs_irt (cfg: model 1..4, D <= 3, J, Dc): P_ij = c_j + (d_j - c_j) sigmoid(Dc (theta_hat_i . a_j + b_j)), z formed as
 *     vx_grid_table_irt forms it (b first, then the dimensions; 1PL: a = 1), c = sigmoid(c_un), d = sigmoid(d_un), 0 and 1 where
 *     the model has neither (the pointer may then be NULL).  theta_hat [nb][D] goes by batch position: the `mean` of
 *     vx_grid_posterior for the same y, rows and nb.
 *   vx_grid_pairs_cdm (cfg: K <= 10, J; dino, q as vx_grid_table_cdm): P_ij = eta_j(pattern_i) ? 1 - s_j : g_j, pattern [nb] by
 *     batch position: the `argmax` of vx_grid_posterior.
 * Products over persons on v_mfma_f32_32x32x16_f16: r and r^2 as fp16 pairs of the value times 2^10, m exact, fp32 accumulation.
 * The operand fragments of a slab of persons (a multiple of 256, as many as ws_floats allow) live in `workspace`; the slab's
 * chunks are added in ascending order and the slabs in person order, no atomics: the same call with the same ws_floats gives
 * the same bits.  Nothing of size persons x items is held outside `workspace`.  vx_grid_pairs_workspace_floats(nb, J): the
 * preferred size (one slab where 512 MB allow it); vx_grid_pairs_workspace_min_floats(J): the smallest accepted (one slab of 256
 * persons, one chunk).  workspace is 16-byte aligned.  n is exact while a call scores at most 2^24 persons (fp32 counts).
 * Limits: model 1..4, 1 <= D <= 3, K <= 10, 1 <= J <= 1024, nb >= 1, ws_floats at least the minimum; VX_EINVAL beyond. */
int64_t vx_grid_pairs_workspace_floats(int64_t nb, int32_t J);
int64_t vx_grid_pairs_workspace_min_floats(int32_t J);
int vx_grid_pairs_irt(const vx_irt_cfg* cfg, const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb,
                      const float* theta_hat /*[nb][D]*/, const float* a /*[D][J] or NULL (1PL)*/, const float* b /*[J]*/,
                      const float* c_un /*[J] or NULL*/, const float* d_un /*[J] or NULL*/, float* n /*[J][J]*/, float* s /*[J][J]*/,
                      float* ss /*[J][J]*/, float* sp /*[J][J]*/, float* workspace, int64_t ws_floats, void* hip_stream);
int vx_grid_pairs_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q /*[K][J]*/, const uint8_t* y /*[n_local][J]*/,
                      const int64_t* rows /*[nb] or NULL*/, int64_t nb, const int32_t* pattern /*[nb]*/, const float* g_un,
                      const float* s_un, float* n /*[J][J]*/, float* s /*[J][J]*/, float* ss /*[J][J]*/, float* sp /*[J][J]*/,
                      float* workspace, int64_t ws_floats, void* hip_stream);

/* ---- Person fit: the sums behind lz (Drasgow-Levine-Williams) and the infit / outfit mean squares, per person and per item, in
 * one pass over persons x items.  Observed cells only (y < 2).  P_ij is the probability vx_grid_pairs_* takes the residual from
 * (same cfg, parameters, theta_hat / pattern and limits), Q = 1 - P formed on its own, never by subtraction, and per cell
 *     lambda = log(P / Q)   l = y ? log P : log Q   eps = P log P + Q log Q   nu = P Q lambda^2
 *     r2 = y ? Q^2 : P^2    w = P Q                 zeta = y ? Q / P : P / Q  (= r2 / w)
 *   person [7][nb]: n (answered items), l0 = sum l, e = sum eps, v = sum nu, sr2 = sum r2, sw = sum w, sz2 = sum zeta over the
 *     items the person answered, by batch position;
 *   item [4][J]: n, sr2, sw, sz2 over the persons who answered the item.
 * lz = (l0 - e) / sqrt(v), outfit = sz2 / n, infit = sr2 / sw (float64 on the host: vipsy_amd.grid.person_fit_host /
 * item_msq_host).  A person or item without answers has exact zeros in its sums.  workspace holds one partial [4][J] per
 * workgroup, vx_grid_fit_workspace_floats(nb, J) floats; the number of workgroups depends on nb alone and every sum has a fixed
 * order, no atomics: the same call gives the same bits on every device.  n is exact while a call scores at most 2^24 persons.
 * Limits: model 1..4, 1 <= D <= 3, K <= 10, 1 <= J <= 1024, nb >= 1, ws_floats at least the size above; VX_EINVAL beyond. */
int64_t vx_grid_fit_workspace_floats(int64_t nb, int32_t J);
int vx_grid_fit_irt(const vx_irt_cfg* cfg, const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb,
                    const float* theta_hat /*[nb][D]*/, const float* a /*[D][J] or NULL (1PL)*/, const float* b /*[J]*/,
                    const float* c_un /*[J] or NULL*/, const float* d_un /*[J] or NULL*/,
                    float* person /*[7][nb]: n, l0, e, v, sr2, sw, sz2*/, float* item /*[4][J]: n, sr2, sw, sz2*/,
                    float* workspace, int64_t ws_floats, void* hip_stream);
int vx_grid_fit_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q /*[K][J]*/, const uint8_t* y /*[n_local][J]*/,
                    const int64_t* rows /*[nb] or NULL*/, int64_t nb, const int32_t* pattern /*[nb]*/, const float* g_un,
                    const float* s_un, float* person /*[7][nb]*/, float* item /*[4][J]*/, float* workspace, int64_t ws_floats,
                    void* hip_stream);

/* ---- Point estimates: the ML, MAP and Warm's weighted-likelihood (WLE) estimate of every scored person by Fisher scoring, from
 * theta0 [nb][D] (by batch position; the `mean` of vx_grid_posterior), over the observed cells of the person's row (y < 2) under
 * the item parameters as they stand (cfg, parameters and limits as vx_grid_fit_irt).  With z = Dc (theta . a + b), P = c + (d - c)
 * sigmoid(z), Q = (1 - d) + (d - c) sigmoid(-z), P_z = (d - c) sigmoid(z) sigmoid(-z):
 *     g_d = Dc sum_j a_jd (y_j ? Q_j : -P_j) P_z / (P_j Q_j)        I_de = Dc^2 sum_j a_jd a_je P_z^2 / (P_j Q_j)
 *   method VX_POINT_ML: g, M = I;  VX_POINT_MAP: g - theta, M = I + 1 (the N(0, I) prior);  VX_POINT_WLE (D = 1): g + J / (2 I),
 *   M = I, J = sum_j P'_j P''_j / (P_j Q_j) (Warm 1989; Firth's penalised score for 1PL / 2PL).
 * An evaluation at theta gives delta = M^-1 g (Cholesky); a person stops AT THE POINT OF THE EVALUATION with status
 *     VX_POINT_CONVERGED  max |delta| <= tol (before the cap)
 *     VX_POINT_AT_BOUND   on two consecutive evaluations a coordinate sits on +-bound and delta points outward
 *     VX_POINT_MAX_ITER   the max_iter-th evaluation did neither
 *     VX_POINT_SINGULAR   a pivot (or the step) is not positive and finite
 *     VX_POINT_EMPTY      no observed cell: theta_hat NaN, info 0, iters 0
 *   and otherwise moves to clamp(theta + delta min(1, step_cap / max |delta|), -bound, bound) (theta0 is clamped alike).
 * theta_hat [nb][D]; info [D (D + 1) / 2][nb]: the upper triangle (00, 01, 02, 11, 12, 22) of I at theta_hat -- the likelihood's,
 * without the prior, for every method; status, iters (the evaluations) [nb] int32.  A person's results depend on its own row
 * and start alone -- not on the persons scored beside it -- every sum has a fixed order, the grid depends on nb alone, there is
 * no atomic: the same call gives the same bits.  y is read once a person; no workspace.
 * Limits: model 1..4, 1 <= D <= 3 (wle: D = 1), 1 <= J <= 1024, nb >= 1, 1 <= max_iter <= 255, tol, bound and step_cap positive
 * and finite; VX_EINVAL beyond, before anything is read. */
#define VX_POINT_ML 0
#define VX_POINT_MAP 1
#define VX_POINT_WLE 2
#define VX_POINT_CONVERGED 0
#define VX_POINT_AT_BOUND 1
#define VX_POINT_MAX_ITER 2
#define VX_POINT_SINGULAR 3
#define VX_POINT_EMPTY 4
int vx_grid_point_irt(const vx_irt_cfg* cfg, const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb,
                      const float* theta0 /*[nb][D]*/, const float* a /*[D][J] or NULL (1PL)*/, const float* b /*[J]*/,
                      const float* c_un /*[J] or NULL*/, const float* d_un /*[J] or NULL*/, int32_t method, int32_t max_iter,
                      float tol, float bound, float step_cap, float* theta_hat /*[nb][D]*/, float* info /*[D (D + 1) / 2][nb]*/,
                      int32_t* status /*[nb]*/, int32_t* iters /*[nb]*/, void* hip_stream);

/* ---- Summed-score tables (k_sumscore.hip): the model side of Orlando & Thissen's S-X2 item fit and of the score -> latent
 * conversion table, by the Lord-Wingersky recursion, and the observed side, over a list of Js items.
 * vx_sumscore_model: p1, p0 [Js][G] = P(y_j = 1 | node g) and P(y_j = 0 | node g) of the listed items (both given; p0 is never
 *   formed as 1 - p1), w_g = exp(logw[g]).  With S(s | g) the probability of the summed score s at node g -- S = delta_0, then for
 *   every item in ascending order S'[s] = p0 S[s] + p1 S[s - 1] -- and S_-j the same without item j:
 *     e1[j][s] = sum_g w_g p1[j][g] S_-j(s - 1 | g)   e0[j][s] = sum_g w_g p0[j][g] S_-j(s | g)     float32 [Js][Js + 1]
 *     dist[g][s] = S(s | g) over all Js items, float32 [G][Js + 1]; NULL: not computed.
 *   e1[j][0], e0[j][Js] and every entry above the number of folded items are exact zeros; e1[j][s] + e0[j][s] = P(score = s).
 *   workspace: vx_sumscore_model_workspace_floats(Js, G) floats, the slabs of the node chunks, added in ascending order
 *   (vx_reduce_slabs).  The chunking depends on Js and G alone, there is no atomic: the same call gives the same bits.
 * vx_sumscore_persons: score[i] = the number of 1s of person rows[i] (rows NULL: i) over the listed columns of y (items[k], int32,
 *   ascending; NULL: the first Js columns), or -1 unless every listed cell is 0 or 1 (255 and 254 take the person out).
 * vx_sumscore_observed: o1[k][s] = the persons i with score[i] = s and y[rows[i]][items[k]] = 1, int32 [Js][Js + 1], zeroed by
 *   the entry; rows and score [nb] are the complete persons, best sorted by score (the counts are right in any order; integer
 *   atomics, the same bits in any order).  A score outside 0 .. Js counts nothing.
 * Limits: 1 <= Js <= 1023, 1 <= G <= 1024, Js <= J <= 4096, nb >= 0 (vx_sumscore_model_workspace_floats: -1 beyond);
 * VX_EINVAL beyond, before anything is read. */
int64_t vx_sumscore_model_workspace_floats(int32_t Js, int32_t G);
int vx_sumscore_model(const float* p1 /*[Js][G]*/, const float* p0 /*[Js][G]*/, const float* logw /*[G]*/, int32_t Js, int32_t G,
                      float* e1 /*[Js][Js + 1]*/, float* e0 /*[Js][Js + 1]*/, float* dist /*[G][Js + 1] or NULL*/,
                      float* workspace, int64_t ws_floats, void* hip_stream);
int vx_sumscore_persons(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J,
                        const int32_t* items /*[Js] or NULL*/, int32_t Js, int32_t* score /*[nb]*/, void* hip_stream);
int vx_sumscore_observed(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb]*/, int64_t nb, int32_t J,
                         const int32_t* items /*[Js] or NULL*/, int32_t Js, const int32_t* score /*[nb]*/,
                         int32_t* o1 /*[Js][Js + 1]*/, void* hip_stream);

/* ---- Pairwise 2 x 2 tables (k_pair_tables.hip): the observed side of Chen & Thissen's LD X2.  With u_ij = [y_ij == 1], z_ij =
 * [y_ij == 0] (every byte >= 2 is not observed, 254 and 255 among them) over the persons rows[i] (rows NULL: i), i < nb, and I_jk
 * the persons with both cells observed: n_ab[j][k] = |{i in I_jk : y_ij = a, y_ik = b}|, that is n11 = u^T u, n10 = u^T z, n01 =
 * z^T u, n00 = z^T z, four full int32 [J][J], zeroed by the entry.  n11 and n00 are symmetric, n10[j][k] = n01[k][j]; on the
 * diagonal n10 = n01 = 0 and n11[j][j], n00[j][j] are the item's counts of 1s and 0s.  The products run on the 32x32x32 int8 MFMA
 * with int32 accumulators straight from the person-major y (transposed on chip: there is no fragment workspace), and the person
 * chunks' sums meet in the tables by integer atomics: exact up to 2^31 - 1 persons, the same bits in any order and on every call.
 * vx_pair_tables_workspace_ints: the int32 the call wants as workspace -- 0 as built (workspace may then be NULL) -- or -1.
 * vx_pair_tables_chunks: the person chunks a pair of item groups is cut into for (nb, J): the launch plan, for tests and probes.
 * Limits: 1 <= J <= 1024, 1 <= nb <= 2^31 - 1 (the queries: -1 beyond), y and the tables non-null, ws_ints at least the query's
 * answer; VX_EINVAL beyond, before the HIP runtime is touched. */
int64_t vx_pair_tables_workspace_ints(int64_t nb, int32_t J);
int64_t vx_pair_tables_chunks(int64_t nb, int32_t J);
int vx_pair_tables(const uint8_t* y /*[n_local][J]*/, const int64_t* rows /*[nb] or NULL*/, int64_t nb, int32_t J,
                   int32_t* n11 /*[J][J]*/, int32_t* n10 /*[J][J]*/, int32_t* n01 /*[J][J]*/, int32_t* n00 /*[J][J]*/,
                   int32_t* workspace /*or NULL*/, int64_t ws_ints, void* hip_stream);

/* ---- slab reduction: out[i] = alpha * sum_s slabs[s][i]  (fixed order -> deterministic) */
int vx_reduce_slabs(const float* slabs, int64_t n_slabs, int64_t len, float alpha, float* out,
                    void* hip_stream);
/* out[0] = alpha * sum(v) (fixed-order two-stage tree; used for the loss);
 * workspace: vx_sum_workspace_floats() floats */
int64_t vx_sum_workspace_floats(void);
int vx_sum(const float* v, int64_t n, float alpha, float* out, float* workspace, uint32_t* step_dev /*or NULL: advanced by
           one in the last launch, as vx_sum2 does*/, void* hip_stream);
/* out[0] = alpha * (sum v1 + sum v2), both of length n, in one pass (the loss of the MVN guides: log-lik + entropy).
 * step_dev (or NULL): the device step counter of a captured step (vx_irt_cfg.step_dev): advanced by one here, the last
 * launch of loss-and-gradients, so that vx_adam_step's t_dev may point at the same word (Adam's count is the step + 1). */
int vx_sum2(const float* v1, const float* v2, int64_t n, float alpha, float* out, float* workspace, uint32_t* step_dev,
            void* hip_stream);

/* ---- optimiser: torch.optim.Adam on a flat float32 buffer split into segments with their own
 * learning rate (pyro.optim.Adam with callable optim_args; vi.py:514, test.py:345-350), optional
 * 0/1 `free` mask multiplied into the gradient first (vi.py:511-512).
 * t: the 1-based step count of the bias corrections; t_dev (or NULL): the same count in DEVICE memory, read by the
 * kernel instead of t (captured steps, see vx_irt1d_grad).
 * loss_src / loss_ring (or NULL): the launch also copies *loss_src (the step's loss slot, all-reduced by then) into
 * loss_ring[t % VX_LOSS_RING] -- the value `svi.step` returns (vi.py:516) then stays readable for VX_LOSS_RING - 1 further
 * steps without a copy launch of its own, in eager and in replayed steps alike. */
#define VX_LOSS_RING 64
typedef struct vx_adam_seg { int64_t begin, end; float lr; float _pad; } vx_adam_seg;
int vx_adam_step(float* p, const float* g, float* m, float* v, const float* free_mask /*or NULL*/,
                 int64_t n, const vx_adam_seg* segs /*host*/, int32_t n_segs, int32_t t, const uint32_t* t_dev,
                 float beta1, float beta2, float eps, const float* loss_src, float* loss_ring /*[VX_LOSS_RING]*/,
                 void* hip_stream);
/* the same for TWO buffers in one launch: A with its free mask (the replicated leaves), B without (the per-person rows
 * of a BBVI guide); same t, betas and eps for both */
int vx_adam_step2(float* pA, const float* gA, float* mA, float* vA, const float* freeA /*or NULL*/, int64_t nA,
                  const vx_adam_seg* segsA, int32_t n_segsA, float* pB, const float* gB, float* mB, float* vB, int64_t nB,
                  const vx_adam_seg* segsB, int32_t n_segsB, int32_t t, const uint32_t* t_dev, float beta1, float beta2,
                  float eps, const float* loss_src, float* loss_ring /*[VX_LOSS_RING]*/, void* hip_stream);

/* ---- a D = 1 step on ONE rank with its optimiser: vx_irt1d_grad / vx_irt1d_sparse_grad and vx_adam_step2 in one call,
 * the slab sum and Adam in ONE launch (three graph nodes a step become two; BASELINE config 2: 38.7 -> ~33 us).  What
 * SVI.step does between loss_and_grads and optim(params) (vi.py:505-514) needs no other rank here -- with a process group
 * the all-reduce sits between the two and the separate calls are used.
 *   A = the item leaves: pA / mA / vA / freeA of exactly 4 J floats, gradient = gitem (still written);
 *   B = the per-person rows [loc | raw] (may be empty: nB = 0): gradients gB as written by the step kernel;
 *   t: Adam's 1-based count (ignored with step_dev: the count is then the device counter + 1, which the call advances);
 *   loss_ring (or NULL): loss[0] is also filed in loss_ring[t % VX_LOSS_RING].
 * Same sums in the same order, same Adam arithmetic: the results are those of the separate calls, bit for bit.
 * workspace as for the separate calls (vx_irt1d_workspace_floats / vx_irt1d_sparse_workspace_floats). */
typedef struct vx_adam_tail {
    float* pA; float* mA; float* vA; const float* freeA /*or NULL*/; int64_t nA; const vx_adam_seg* segsA /*host*/;
    float* pB; const float* gB; float* mB; float* vB; int64_t nB; const vx_adam_seg* segsB /*host*/;
    int32_t n_segsA, n_segsB, t;
    float beta1, beta2, eps;
    float* loss_ring /*[VX_LOSS_RING] or NULL*/;
} vx_adam_tail;
int vx_irt1d_grad_adam(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                       const float* loc, const float* raw, const float* eps_in, const float* a, const float* b,
                       const float* c_un, const float* d_un, float* gloc, float* graw, float* elbo, float* gitem,
                       float* loss, uint32_t* step_dev /*or NULL*/, float* workspace, const vx_adam_tail* opt,
                       void* hip_stream);
int vx_irt1d_sparse_grad_adam(const vx_irt_cfg* cfg, const uint16_t* pent, const int32_t* glen, int32_t Lq,
                              const int32_t* pidx, int64_t n_groups, int64_t gid0, const float* loc, const float* raw,
                              const float* eps_in, const float* a, const float* b, const float* c_un, const float* d_un,
                              float* gloc, float* graw, float* elbo, float* gitem, float* loss,
                              uint32_t* step_dev /*or NULL*/, float* workspace, const vx_adam_tail* opt, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VIPSY_AMD_H */
