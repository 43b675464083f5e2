// The cross-product (BHHH) information of the item parameters from the grid posteriors.  With Fisher's identity the marginal
// score of person i for parameter k of item j is
//
//     s_i[(j,k)] = sum_g p_i(g) ( [y_ij == 1] W1[g][(j,k)] - [y_ij == 0] W0[g][(j,k)] ),     W1 = (1 - P_j(g)) u_jgk,  W0 = P_j(g) u_jgk
//
// p_i(g) the posterior k_grid_counts.hip forms, u_g = Dc (1, theta_g) for the IRT links and ([eta = 0], -[eta = 1]) for DINA /
// DINO on the unconstrained g / s scale.  info = sum_i s_i s_i^T, gradient = sum_i s_i.  Dense parameter layout: column
// c = j K + k, K = D + 1 (k = 0: b, k = 1 + d: a_d) for 2PL, 1 for 1PL, 2 (g_un, s_un) for DINA / DINO; 3PL / 4PL add k = D + 1:
// c_un and k = D + 2: d_un (K = D + 2 / D + 3 <= 6), with W1 = v / P, W0 = v / Q, v = dP / d(unknown) of the penalised M-step's cell
// (gi_asym_cell) -- the same identity, and the 2PL tables are its case c = 0, d = 1.  P = J K <= 4096.
// Three chained products on v_mfma_f32_32x32x16_f16, fp16 pairs, fp32 accumulation:
//
//   tables    k_grid_wtable_irt / k_grid_wtable_cdm write W1 and W0 as the operand image of product 2, [node tile][k-step][parameter
//             tile][W1 head, W1 low, W0 head, W0 low][64 lanes][8 fp16]: lane l, element e is parameter 32 pt + (l & 31) at node
//             32 nt + 16 s + 8 (e >> 2) + 4 (l >> 5) + (e & 3) -- the order in which an accumulator of k_grid_post's orientation holds
//             its nodes.  P, 1 - P and the clamp are the M-step's: gm_cell (a node where the z clamp is active contributes 0),
//             gp_cdm_eta / gp_cdm_qpat.  Values times 2^s, s = f16_scale_exp(Dc max(1, |theta|_inf)) (|W| <= that bound, and so is
//             |s_i|: sum_g p = 1); 2^s and 2^-s sit in the image's 16-byte trailer, where the kernels read them.
//             k_grid_wtable_irt_asym (3PL / 4PL): the same image and trailer, s from the table's own largest magnitude, found
//             in a first pass (no closed bound: a 4PL entry grows like 1 / (d - c)); the image carries |W 2^s| < 2^15.
//   1 + 2     k_grid_pscores: a workgroup takes 64 persons at a time.  Its waves share the node passes of k_grid_post's operand
//             phase (GP_UNIT_* / GP_PASS / GP_INDICATORS, unchanged: person on the lane, 16 nodes of a tile in the registers),
//             form p = exp(f - loglik_i) as k_grid_counts does and leave p 2^14 as fp16 pairs in LDS: registers 0..7 and 8..15 of an
//             accumulator ARE two A fragments with k = nodes.  Then the waves share the parameter tiles: B1 = p W1, B0 = p W0 over
//             all node tiles (hh, hl, lh), S = [y = 1] B1 - [y = 0] B0 by byte gathers of y for the lane's item.  That accumulator
//             has the parameter on the lane and 16 persons in the registers: split, it is the pair of fragments product 3 needs,
//             with k = persons.  They go to the workspace as [unit of 32 persons][parameter tile][k-step][head, low][64 lanes] x 16 B
//             (4 B an entry of S).  Nothing of size persons x nodes touches memory.  Persons past nb and responses 254 / 255 give
//             exact zeros; column P (always inside the padding: PT = (P + 32) / 32 tiles) is 2^s for valid persons, so that product 3
//             also yields the gradient.  Beyond 512 nodes the LDS holds one person tile at a time and the operand phase runs twice.
//   3         k_grid_xprod: the SYRK over persons, output-stationary blocks of 4 x 4 parameter tiles, upper triangle only, three
//             products a tile pair; the slab's person units go to chunks whose partial tiles are added in ascending order
//             (vx_reduce_slabs), the slabs of a call in person order (k_info_add), no float atomics: the same call gives the same
//             bits.  k_info_finish takes the scale off, writes the upper triangle and its mirror (a diagonal tile's upper half
//             only: the matrix is symmetric bit for bit) and the gradient.
// Persons a slab, chunks a slab and the parts of the workspace are slab_plan's (SlabPlan, grid_plan.h: the one plan this file and
// k_grid_pairs.hip share), walked by grid_slab_loop (vx_abi.hip).
#pragma once
#include "k_grid_counts.hip"
#include "k_grid_mstep.hip"

// GI_BT, GI_TILE, GI_MAX_BLOCKS, gi_pt, gi_pairs and gi_pair_index are in grid_plan.h, beside gi_slab_plan
#define GI_MAXP 4096
#define GI_MAXK 6                       // 4PL in three dimensions: b, a_0 .. a_2, c_un, d_un
#define GI_LDS_NT 16                    // node tiles up to which the LDS holds p of both person tiles of a unit

__host__ __device__ inline int64_t gi_wimage_frag_bytes(int P, int G) { return (int64_t)gp_nt(G) * 2 * gi_pt(P) * 4 * 64 * 16; }
inline int gi_nsub(int G) { return gp_nt(G) > GI_LDS_NT ? 2 : 1; }
inline size_t gi_lds_bytes(int G) {
    const int NT = gp_nt(G);
    // p fragments [person tiles kept][NT][2 k-steps][head, low][64 lanes] x 16 B; logw [NT * 32]; rows int64 [64]
    return (size_t)(GP_MT / gi_nsub(G)) * NT * 4 * 64 * 16 + (size_t)NT * 32 * 4 + 64 * 8;
}

// one cell -> its four fp16 words in the W image (values already scaled)
__device__ __forceinline__ void gi_put(uint16_t* __restrict__ wimg, int PT, int gp, int cp, float w1, float w0) {
    const int nt = gp >> 5, s = (gp >> 4) & 1, q = gp & 15, h = (q >> 2) & 1, e = ((q >> 3) << 2) | (q & 3);
    const int pt = cp >> 5, lane = (cp & 31) + 32 * h;
    const int64_t base = (((((int64_t)nt * 2 + s) * PT + pt) * 4) * 64 + lane) * 8 + e;
    uint16_t h1, l1, h0, l0;
    split2h_bits(w1, h1, l1);
    split2h_bits(w0, h0, l0);
    wimg[base] = h1; wimg[base + 512] = l1; wimg[base + 1024] = h0; wimg[base + 1536] = l0;
}

// 2^s for |values| <= bound, from every thread of the block alike; block 0 leaves (2^s, 2^-s) in the trailer
__device__ __forceinline__ float gi_scale(float bound, float* __restrict__ trailer) {
    const int s = f16_scale_exp(bound);
    const float sc = ldexpf(1.0f, s);
    if (blockIdx.x == 0 && threadIdx.x == 0) { trailer[0] = sc; trailer[1] = ldexpf(1.0f, -s); trailer[2] = 0.f; trailer[3] = 0.f; }
    return sc;
}

// IRT: z and the cell as gm_eval has them (b first, then the dimensions; 1PL: a = 1), u = Dc (1, theta_g)
template <int MODEL>
__global__ __launch_bounds__(256) void k_grid_wtable_irt(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                         const float* __restrict__ a, const float* __restrict__ b,
                                                         uint16_t* __restrict__ wimg, float* __restrict__ trailer) {
    __shared__ float red[256];
    float tmax = 1.0f;
    for (int i = threadIdx.x; i < G * D; i += 256) tmax = fmaxf(tmax, fabsf(theta[i]));
    red[threadIdx.x] = tmax;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const float sc = gi_scale(fabsf(Dc) * red[0], trailer);
    const int K = (MODEL == 1) ? 1 : D + 1, P = J * K, PT = gi_pt(P), PP = PT * 32, total = gp_nt(G) * 32 * PP;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / PP, cp = idx - gp * PP;
        float w1 = 0.f, w0 = 0.f;
        if (gp < G && cp < P) {
            const int j = cp / K, k = cp - j * K;
            float sz = b[j];
            if (MODEL == 1) {
                sz = fmaf(theta[(int64_t)gp * D], 1.f, sz);
            } else {
                for (int d = 0; d < D; ++d) sz = fmaf(theta[(int64_t)gp * D + d], a[(int64_t)d * J + j], sz);
            }
            float lp1, lp0, om, pr;
            gm_cell(Dc * sz, lp1, lp0, om, pr);
            const float u = Dc * (k == 0 ? 1.f : theta[(int64_t)gp * D + (k - 1)]);
            w1 = om * u * sc;
            w0 = pr * u * sc;
        }
        gi_put(wimg, PT, gp, cp, w1, w0);
    }
}

// 3PL / 4PL: one cell of column k of item j at node gp, unscaled.  The arithmetic of gm_eval<3 | 4> (k_grid_mstep.hip) said again:
// the asymptotes capped as there, z in its order, v = dP / d(unknown k), W1 = v / Pc, W0 = v / Qc, both 0 where the node is not inside
template <int MODEL>
__device__ __forceinline__ void gi_asym_cell(int D, int J, float Dc, const float* __restrict__ theta, const float* __restrict__ a,
                                             const float* __restrict__ b, const float* __restrict__ c_un,
                                             const float* __restrict__ d_un, int gp, int j, int k, float& w1, float& w0) {
    const float c = fminf(sigmoidf_(c_un[j]), 1.0f - VX_EPS32);
    float dd = 1.f, omd = 0.f;
    if (MODEL == 4) {
        dd = fminf(sigmoidf_(d_un[j]), 1.0f - VX_EPS32);
        omd = fmaxf(sigmoidf_(-d_un[j]), VX_EPS32);
    }
    const float dmc = dd - c;
    float sz = b[j];
    for (int d = 0; d < D; ++d) sz = fmaf(theta[(int64_t)gp * D + d], a[(int64_t)d * J + j], sz);
    const float z = Dc * sz;
    const float e = __expf(-fabsf(z));
    const float r = fast_rcp(1.0f + e);
    const float sg = (z >= 0.f) ? r : e * r;                        // sigmoid(z)
    const float sn = (z >= 0.f) ? e * r : r;                        // sigmoid(-z), no cancellation
    const float P = c + dmc * sg;
    const float Q = omd + dmc * sn;
    const bool inside = (P >= VX_EPS32) && (Q >= VX_EPS32);
    const float Pc = fminf(fmaxf(P, VX_EPS32), 1.0f - VX_EPS32);
    const float Qc = fminf(fmaxf(Q, VX_EPS32), 1.0f - VX_EPS32);
    float v;
    if (k <= D) v = dmc * sg * sn * (Dc * (k == 0 ? 1.f : theta[(int64_t)gp * D + (k - 1)]));
    else if (k == D + 1) v = sn * (c * (1.0f - c));
    else v = sg * (dd * omd);
    w1 = inside ? v * fast_rcp(Pc) : 0.f;
    w0 = inside ? v * fast_rcp(Qc) : 0.f;
}

// IRT with asymptotes (MODEL 3 | 4), K = D + MODEL - 1 columns an item: b, a_0 .. a_{D-1}, c_un, then d_un.  No bound in closed
// form serves these tables: 3PL entries stay below max(1, Dc max(1, |theta|_inf)), but W0 of c_un and W1 of d_un of a 4PL item grow
// like 1 / (d - c), and d <= c is admissible.  So the scale comes from the table itself, in two launches of this kernel around
// k_grid_wscale: FILL = false takes the largest |W1|, |W0| of the launch's cells -- a block's by fmaxf in LDS, the blocks' by an
// integer maximum on the bit patterns of those non-negative floats in trailer[2] (zeroed before; no float atomics: whatever
// the order, the same bits) --, k_grid_wscale turns it into the trailer (2^s, 2^-s, 0, 0) with s = f16_scale_exp(that maximum),
// and FILL = true writes the image at that scale.  The image then carries |W 2^s| < 2^15, and so does S: sum_g p = 1.
template <int MODEL, bool FILL>
__global__ __launch_bounds__(256) void k_grid_wtable_irt_asym(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                              const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ c_un, const float* __restrict__ d_un,
                                                              uint16_t* __restrict__ wimg, float* trailer) {
    const int K = D + MODEL - 1, P = J * K, PT = gi_pt(P), PP = PT * 32, total = gp_nt(G) * 32 * PP;
    const float sc = FILL ? trailer[0] : 1.0f;
    float m = 0.f;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / PP, cp = idx - gp * PP;
        float w1 = 0.f, w0 = 0.f;
        if (gp < G && cp < P) {
            const int j = cp / K, k = cp - j * K;
            gi_asym_cell<MODEL>(D, J, Dc, theta, a, b, c_un, d_un, gp, j, k, w1, w0);
        }
        if (FILL) gi_put(wimg, PT, gp, cp, w1 * sc, w0 * sc);
        else m = fmaxf(m, fmaxf(fabsf(w1), fabsf(w0)));
    }
    if (!FILL) {
        __shared__ float red[256];
        red[threadIdx.x] = m;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0) atomicMax((unsigned int*)(trailer + 2), __float_as_uint(red[0]));
    }
}

// trailer[2] = the largest magnitude of the table (k_grid_wtable_irt_asym<., false>) -> the trailer as gi_scale leaves it
__global__ void k_grid_wscale(float* __restrict__ trailer) {
    const int s = f16_scale_exp(trailer[2]);
    trailer[0] = ldexpf(1.0f, s); trailer[1] = ldexpf(1.0f, -s); trailer[2] = 0.f; trailer[3] = 0.f;
}

// DINA / DINO: P and 1 - P as k_grid_table_cdm has them; a parameter at the Bernoulli clamp contributes 0
__global__ __launch_bounds__(256) void k_grid_wtable_cdm(int K, int J, int dino, const float* __restrict__ q,
                                                         const float* __restrict__ g_un, const float* __restrict__ s_un,
                                                         uint16_t* __restrict__ wimg, float* __restrict__ trailer) {
    const float sc = gi_scale(1.0f, trailer);
    const int G = 1 << K, P = 2 * J, PT = gi_pt(P), PP = PT * 32, total = gp_nt(G) * 32 * PP;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / PP, cp = idx - gp * PP;
        float w1 = 0.f, w0 = 0.f;
        if (gp < G && cp < P) {
            const int j = cp >> 1, k = cp & 1;
            const bool eta = gp_cdm_eta(dino, gp_cdm_qpat(q, K, J, j), gp);
            if ((k == 1) == eta) {                                  // g_un acts where eta = 0, s_un where eta = 1
                const float un = eta ? s_un[j] : g_un[j];
                const float hi = sigmoidf_(un), lo = sigmoidf_(-un);
                if (hi <= 1.0f - VX_EPS32 && lo >= VX_EPS32) {
                    // eta = 0: P = g = hi, 1 - P = lo, u = 1;  eta = 1: P = 1 - s = lo, 1 - P = s = hi, u = -1
                    w1 = (eta ? -hi : lo) * sc;
                    w0 = (eta ? -lo : hi) * sc;
                }
            }
        }
        gi_put(wimg, PT, gp, cp, w1, w0);
    }
}

// S of a slab of persons.  y, rows, loglik start at the slab's first person; nb = its persons.
__global__ __launch_bounds__(GP_THREADS) void k_grid_pscores(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                             int64_t nb, int J, int G, int K, int P,
                                                             const uint4* __restrict__ img, const uint4* __restrict__ wimg,
                                                             const float* __restrict__ trailer, const float* __restrict__ logw,
                                                             const float* __restrict__ loglik, uint4* __restrict__ S, int nsub) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gi_smem[];
    const int KC = gp_kc(J), NT = gp_nt(G), PT = gi_pt(P), mts = GP_MT / nsub;
    uint4* pbuf = (uint4*)gi_smem;
    float* lw = (float*)(pbuf + (size_t)mts * NT * 4 * 64);
    int64_t* rowbuf = (int64_t*)(lw + NT * 32);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    for (int i = tid; i < NT * 32; i += GP_THREADS) lw[i] = (i < G) ? logw[i] : -__builtin_inff();
    const float one = trailer[0];                                   // the constant column: 1 at the scale of S
    __syncthreads();
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        GP_UNIT_STATE;
        float lk[GP_MT];
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GP_UNIT_PERSON(mt);
            const bool valid = pid[mt] < nb;
            lk[mt] = valid ? loglik[pid[mt]] : __builtin_inff();    // f - inf = -inf: p = 0
            if (wave == 0 && half == 0) rowbuf[mt * 32 + l31] = valid ? row : (int64_t)-1;
        }
        // GP_PASS counts the missing cells in its pass at node tile 0, which is wave 0's: the other waves count theirs here
        if (wave != 0 && wave * GP_NTG < NT) {
            for (int kc = 0; kc < KC; ++kc) {
                const int j0 = kc * 16 + 8 * half;
#pragma unroll
                for (int mt = 0; mt < GP_MT; ++mt) {
                    f16x8 f1, f0;
                    GP_INDICATORS(yr[mt], J, j0, f1, f0, nmiss[mt] +=)
                    (void)f1; (void)f0;
                }
            }
#pragma unroll
            for (int mt = 0; mt < GP_MT; ++mt) {
                const int tot = nmiss[mt] + __shfl_xor(nmiss[mt], 32, 64);
                miss[mt] = (float)tot * VX_LOGP_MISSING;
            }
        }
        for (int sub = 0; sub < nsub; ++sub) {
            const int mt_lo = sub * mts, mt_hi = mt_lo + mts;
            if (wave == 0) {
#pragma unroll
                for (int mt = 0; mt < GP_MT; ++mt) nmiss[mt] = 0;   // (its pass at node tile 0 counts again)
            }
            // ---- (1) the node passes of this wave: p of the unit as fragments in LDS
            for (int ng = wave * GP_NTG; ng < NT; ng += GP_WAVES * GP_NTG) {
                f32x16 acc[GP_MT][GP_NTG];
                GP_PASS(acc)
#pragma unroll
                for (int t = 0; t < GP_NTG; ++t) {
                    if (ng + t < NT) {
                        const int g0 = (ng + t) * 32 + 4 * half;
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            if (mt >= mt_lo && mt < mt_hi) {
                                float pv[16];
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const int g = g0 + (r & 3) + 8 * (r >> 2);
                                    const float f = fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g];
                                    pv[r] = __expf(f - lk[mt]);
                                }
#pragma unroll
                                for (int s = 0; s < 2; ++s) {
                                    float v[8];
#pragma unroll
                                    for (int e = 0; e < 8; ++e) v[e] = pv[8 * s + e];
                                    f16x8 fh, fl;
                                    split2h_frag(v, GC_PSCALE, fh, fl);
                                    uint4* dst = pbuf + ((((mt - mt_lo) * NT + (ng + t)) * 2 + s) * 2) * 64 + lane;
                                    dst[0] = __builtin_bit_cast(uint4, fh);
                                    dst[64] = __builtin_bit_cast(uint4, fl);
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads();
            // ---- (2) the parameter tiles of this wave: B1, B0 over all node tiles, S, its fragments
            for (int pt = wave; pt < PT; pt += GP_WAVES) {
                f32x16 b1[GP_MT], b0[GP_MT];
#pragma unroll
                for (int mt = 0; mt < GP_MT; ++mt) { b1[mt] = zero16(); b0[mt] = zero16(); }
                for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const uint4* wp = wimg + ((((int64_t)nt * 2 + s) * PT + pt) * 4) * 64 + lane;
                        const f16x8 w1h = __builtin_bit_cast(f16x8, wp[0]), w1l = __builtin_bit_cast(f16x8, wp[64]);
                        const f16x8 w0h = __builtin_bit_cast(f16x8, wp[128]), w0l = __builtin_bit_cast(f16x8, wp[192]);
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            if (mt >= mt_lo && mt < mt_hi) {
                                const uint4* pp = pbuf + ((((mt - mt_lo) * NT + nt) * 2 + s) * 2) * 64 + lane;
                                const f16x8 ph = __builtin_bit_cast(f16x8, pp[0]), pl = __builtin_bit_cast(f16x8, pp[64]);
                                b1[mt] = mfma_f16(ph, w1h, b1[mt]);
                                b1[mt] = mfma_f16(ph, w1l, b1[mt]);
                                b1[mt] = mfma_f16(pl, w1h, b1[mt]);
                                b0[mt] = mfma_f16(ph, w0h, b0[mt]);
                                b0[mt] = mfma_f16(ph, w0l, b0[mt]);
                                b0[mt] = mfma_f16(pl, w0h, b0[mt]);
                            }
                        }
                    }
                }
                const int c = pt * 32 + l31;
                const int j = c < P ? c / K : 0;
#pragma unroll
                for (int mt = 0; mt < GP_MT; ++mt) {
                    if (mt >= mt_lo && mt < mt_hi) {
                        float sv[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int64_t rr = rowbuf[mt * 32 + crow32(r, half)];
                            if (c < P) {
                                const unsigned yy = rr >= 0 ? (unsigned)y[rr * J + j] : 254u;
                                // p 2^14 W 2^s 2^-14: S at the scale of W
                                sv[r] = (yy == 1u) ? b1[mt][r] * GC_PUNSCALE : ((yy == 0u) ? -(b0[mt][r] * GC_PUNSCALE) : 0.f);
                            } else {
                                sv[r] = (c == P && rr >= 0) ? one : 0.f;
                            }
                        }
#pragma unroll
                        for (int s = 0; s < 2; ++s) {
                            float v[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = sv[8 * s + e];
                            f16x8 fh, fl;
                            split2h_frag(v, 1.0f, fh, fl);
                            uint4* dst = S + ((((unit * GP_MT + mt) * PT + pt) * 2 + s) * 2) * 64 + lane;
                            dst[0] = __builtin_bit_cast(uint4, fh);
                            dst[64] = __builtin_bit_cast(uint4, fl);
                        }
                    }
                }
            }
            __syncthreads();                                        // the next pass rewrites the LDS
        }
    }
}

// S^T S of a slab: workgroup = (block of GI_BT x GI_BT parameter tiles of the upper triangle, chunk of person units); wave w holds
// row tile GI_BT ba + w against the block's GI_BT column tiles.  A fragment of S serves as A (its tile's parameters as rows) and
// as B (as columns) alike: k = the same persons in the same slots.  Tile (pa <= pb) of chunk c goes to slab c at gi_pair_index,
// as the accumulator holds it: [register][lane].
__global__ __launch_bounds__(256) void k_grid_xprod(const uint4* __restrict__ S, int PT, int nbb, int64_t n_units,
                                                    int64_t units_per_chunk, float* __restrict__ slabs, int64_t slab_len) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_bp = (int64_t)nbb * (nbb + 1) / 2;
    const int64_t chunk = blockIdx.x / n_bp;
    int rem = (int)(blockIdx.x % n_bp), ba = 0;
    while (rem >= nbb - ba) { rem -= nbb - ba; ++ba; }
    const int bb = ba + rem;
    const int pa = ba * GI_BT + wave;
    if (pa >= PT) return;
    const int64_t u0 = chunk * units_per_chunk;
    const int64_t u1 = u0 + units_per_chunk < n_units ? u0 + units_per_chunk : n_units;
    f32x16 acc[GI_BT];
#pragma unroll
    for (int i = 0; i < GI_BT; ++i) acc[i] = zero16();
    for (int64_t u = u0; u < u1; ++u) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint4* ap = S + (((u * PT + pa) * 2 + s) * 2) * 64 + lane;
            const f16x8 ah = __builtin_bit_cast(f16x8, ap[0]), al = __builtin_bit_cast(f16x8, ap[64]);
#pragma unroll
            for (int i = 0; i < GI_BT; ++i) {
                const int pb = bb * GI_BT + i;
                if (pb < PT && pb >= pa) {
                    const uint4* bp = S + (((u * PT + pb) * 2 + s) * 2) * 64 + lane;
                    const f16x8 bh = __builtin_bit_cast(f16x8, bp[0]), bl = __builtin_bit_cast(f16x8, bp[64]);
                    acc[i] = mfma_f16(ah, bh, acc[i]);
                    acc[i] = mfma_f16(ah, bl, acc[i]);
                    acc[i] = mfma_f16(al, bh, acc[i]);
                }
            }
        }
    }
    float* slab = slabs + chunk * slab_len;
#pragma unroll
    for (int i = 0; i < GI_BT; ++i) {
        const int pb = bb * GI_BT + i;
        if (pb < PT && pb >= pa) {
            float* dst = slab + gi_pair_index(PT, pa, pb) * GI_TILE + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r * 64] = acc[i][r];
        }
    }
}

// the running sum of the slabs' tiles, in person order
__global__ __launch_bounds__(256) void k_info_add(float* __restrict__ acc, const float* __restrict__ part, int64_t n, int first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        acc[i] = first ? part[i] : acc[i] + part[i];
}

// tiles -> info [P][P] (the upper triangle and its mirror) and gradient [P] (column P); the scale of S comes off twice
__global__ __launch_bounds__(256) void k_info_finish(const float* __restrict__ tiles, int P, int PT, const float* __restrict__ trailer,
                                                     float* __restrict__ info, float* __restrict__ gradient) {
    const float un = trailer[1] * trailer[1];
    const int64_t total = (int64_t)P * (P + 1);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int i = (int)(idx / (P + 1)), c = (int)(idx - (int64_t)i * (P + 1));
        if (c < i) continue;
        const int pa = i >> 5, m = i & 31, pb = c >> 5, n = c & 31;
        const int half = (m >> 2) & 1, r = (m & 3) + 4 * (m >> 3);
        const float v = tiles[gi_pair_index(PT, pa, pb) * GI_TILE + r * 64 + n + 32 * half] * un;
        if (c == P) {
            gradient[i] = v;
        } else {
            info[(int64_t)i * P + c] = v;
            info[(int64_t)c * P + i] = v;
        }
    }
}
