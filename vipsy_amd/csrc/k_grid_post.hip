// Grid posteriors: person scores by quadrature over a fixed set of latent nodes (EAP, PSD, marginal log-likelihood, MAP
// node) for the low-dimensional IRT models and the pattern-enumerated DINA / DINO.  No guide is involved: the item
// parameters and a response row are all a person needs, so training rows and new respondents take the same path.
//
//     ll[i][g] = sum_j [y_ij == 1] T1[j][g] + [y_ij == 0] T0[j][g] + (#missing_i) VX_LOGP_MISSING
//
// is a GEMM whose one operand is a 0/1 indicator (exact in fp16) and whose other operand is a small table, T1 = log P(y_j = 1 |
// node g), T0 = log P(y_j = 0 | node g), split into two fp16 terms of T 2^10 (f16x2, vx_common.h; |T| <= -log eps32 = 15.95, so
// the scaled heads stay below 2^14 and the low terms of the smallest entries, -1.2e-7, still land on fp16 subnormals the MFMA
// honours): two products an indicator on v_mfma_f32_32x32x16_f16, fp32 accumulation.
//
// Orientation: the TABLE is the A operand (rows = nodes) and the INDICATOR the B operand (columns = persons), so an accumulator
// tile has its person on the lane and 16 nodes in the lane's registers (the other 16 in lane ^ 32).  Everything a person needs
// over the nodes -- running maximum, sums, moments -- is then a loop over a lane's own registers; the two half-states meet
// once, at the end.  Nothing of size [n][G] ever leaves the registers.
//
// Operand image (k_grid_table_*): [NT node tiles][KC item chunks][4: T1 head, T1 low, T0 head, T0 low][64 lanes][8 fp16] --
// lane l, element e of (nt, kc) is node 32 nt + (l & 31), item 16 kc + 8 (l >> 5) + e: one 16-byte load a lane is one
// fragment.  Nodes >= G and items >= J are ZERO rows (and carry log-weight -inf in the main kernel): ragged edges live in
// the tables, not in the loops.
//
// Shared with k_grid_draw.hip and k_grid_counts.hip, which include this file: the byte-to-indicator decoding (GP_INDICATORS, all
// three) and the operand phase of the person-on-lane kernels (GP_UNIT_STATE / GP_UNIT_PERSON / GP_PASS; posterior and draw).
//
// Limits (vx_grid_*: VX_EINVAL beyond): J <= 1024, G <= 1024, D <= 10, nb >= 1.
#pragma once
#include "vx_common.h"
#include "k_hodina.hip"
#include "grid_plan.h"                   // gp_nt, and the launch plans of the family

#define GP_THREADS 256
#define GP_WAVES (GP_THREADS / 64)
#define GP_MT 2                  // person tiles (32 persons) a wave carries: one table fragment serves both
#define GP_NTG 2                 // node tiles per pass over the items (61 nodes = one pass)
#define GP_MAXJ 1024
#define GP_MAXG 1024
#define GP_MAXD 10
#define GP_SCALE 1024.0f         // 2^10 into the fp16 split ...
#define GP_UNSCALE 0.0009765625f // ... and off the fp32 accumulator (exact)
#define GP_NEG (-3.0e38f)        // "no node yet": below every reachable log-weight + log-likelihood (>= -1024 * 16 - 88)

__host__ __device__ inline int gp_kc(int J) { return (J + 15) / 16; }
__host__ __device__ inline int64_t gp_image_bytes(int J, int G) { return (int64_t)gp_nt(G) * gp_kc(J) * 4 * 64 * 16; }

// one table cell -> its four fp16 words in the image
__device__ __forceinline__ void gp_put(uint16_t* __restrict__ img, int KC, int gp, int jp, float t1, float t0) {
    const int nt = gp >> 5, m = gp & 31, kc = jp >> 4, hh = (jp >> 3) & 1, e = jp & 7;
    const int64_t base = ((((int64_t)nt * KC + kc) * 4) * 64 + (m + 32 * hh)) * 8 + e;
    uint16_t h1, l1, h0, l0;
    split2h_bits(t1 * GP_SCALE, h1, l1);
    split2h_bits(t0 * GP_SCALE, h0, l0);
    img[base] = h1; img[base + 512] = l1; img[base + 1024] = h0; img[base + 1536] = l0;
}

// IRT: z = Dc (theta_g . a_j + b_j) (1PL: Dc (theta + b)), the cell of the step kernels with y = 1 and y = 0 -- a person scored
// at node theta gets the log-likelihood the step would give at x = theta, clamp included.
template <int MODEL>
__global__ __launch_bounds__(256) void k_grid_table_irt(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                        const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ c_un, const float* __restrict__ d_un,
                                                        uint16_t* __restrict__ img) {
    const int KC = gp_kc(J), JP = KC * 16, total = gp_nt(G) * 32 * JP;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / JP, jp = idx - gp * JP;
        float t1 = 0.f, t0 = 0.f;
        if (gp < G && jp < J) {
            float s = b[jp];
            if (MODEL == 1) {
                s += theta[(int64_t)gp * D];
            } else {
                for (int d = 0; d < D; ++d) s = fmaf(theta[(int64_t)gp * D + d], a[(int64_t)d * J + jp], s);
            }
            const float z = Dc * s;
            const float c = (MODEL >= 3) ? fminf(sigmoidf_(c_un[jp]), 1.0f - VX_EPS32) : 0.f;
            const float dd = (MODEL >= 4) ? fminf(sigmoidf_(d_un[jp]), 1.0f - VX_EPS32) : 1.0f;
            const float omd = (MODEL >= 4) ? fmaxf(sigmoidf_(-d_un[jp]), VX_EPS32) : 0.f;
            float dz, dc, ddd;
            irt_cell<MODEL>(z, 1u, c, dd, omd, t1, dz, dc, ddd);
            irt_cell<MODEL>(z, 0u, c, dd, omd, t0, dz, dc, ddd);
        }
        gp_put(img, KC, gp, jp, t1, t0);
    }
}

// The attributes item j needs, as a bit pattern, and eta of a pattern for it (shared with k_grid_mstep.hip): DINA -- every needed
// attribute held; DINO -- any of them, with the reference's in-place sequencing: single-attribute items always get eta = 0.
__device__ __forceinline__ int gp_cdm_qpat(const float* __restrict__ q, int K, int J, int j) {
    int qpat = 0;
    for (int k = 0; k < K; ++k)
        if (q[(int64_t)k * J + j] != 0.f) qpat |= (1 << k);
    return qpat;
}
__device__ __forceinline__ bool gp_cdm_eta(int dino, int qpat, int pattern) {
    return dino ? (__popc(qpat) >= 2 && (pattern & qpat) != 0) : ((pattern & qpat) == qpat);
}

// DINA / DINO: node c = attribute pattern (bit k = attribute k, the order of all_attrs); eta as k_hodina has it (DINO with the
// reference's in-place sequencing: single-attribute items always get eta = 0), the Bernoulli clamp of bern_const.
__global__ __launch_bounds__(256) void k_grid_table_cdm(int K, int J, int dino, const float* __restrict__ q,
                                                        const float* __restrict__ g_un, const float* __restrict__ s_un,
                                                        uint16_t* __restrict__ img) {
    const int G = 1 << K, KC = gp_kc(J), JP = KC * 16, total = gp_nt(G) * 32 * JP;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / JP, jp = idx - gp * JP;
        float t1 = 0.f, t0 = 0.f;
        if (gp < G && jp < J) {
            const bool eta = gp_cdm_eta(dino, gp_cdm_qpat(q, K, J, jp), gp);
            const float gj = fminf(sigmoidf_(g_un[jp]), 1.0f - VX_EPS32), og = fmaxf(sigmoidf_(-g_un[jp]), VX_EPS32);
            const float sj = fminf(sigmoidf_(s_un[jp]), 1.0f - VX_EPS32), os = fmaxf(sigmoidf_(-s_un[jp]), VX_EPS32);
            const float P = eta ? os : gj, Q = eta ? sj : og;
            float dP;
            bern_const(P, Q, 1u, t1, dP);
            bern_const(P, Q, 0u, t0, dP);
        }
        gp_put(img, KC, gp, jp, t1, t0);
    }
}

// Eight response bytes from p (any alignment) as two words: three ALIGNED dword loads and two v_alignbyte instead of eight byte
// loads.  A dword is loaded only if it starts before `end` (the end of the row), so every load holds at least one byte of the
// row -- an aligned dword cannot straddle a page, nothing unmapped is touched -- and bytes past the row are the caller's to mask.
__device__ __forceinline__ void gp_load8(const uint8_t* p, const uint8_t* end, uint32_t& lo, uint32_t& hi) {
    const unsigned sh = (unsigned)((uintptr_t)p & 3u);
    const uint8_t* q = p - sh;
    const uint32_t w0 = (q < end) ? *(const uint32_t*)q : 0u;
    const uint32_t w1 = (q + 4 < end) ? *(const uint32_t*)(q + 4) : 0u;
    const uint32_t w2 = (sh != 0u && q + 8 < end) ? *(const uint32_t*)(q + 8) : 0u;
    lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
    hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
}

// The operand phase of the grid kernels, written once.  These are macros, not inline functions: a helper is simplified on its
// own before it is inlined, the loops then reach the back end in another shape, and k_grid_draw, which sits at the edge of its
// register budget, pays for it (measured: docs/NOTEBOOK.md).  Expanded in place the kernels compile to what they were.
//
// GP_INDICATORS: the indicator fragments of one response row at items j0 .. j0 + 7 (a lane's eight of item chunk kc: j0 = 16 kc +
// 8 half): f1[e] = [y == 1], f0[e] = [y == 0], exact in fp16; COUNT, a statement prefix such as `nmiss +=`, takes 1 for every
// cell of the eight that is 255 (missing).  Bytes at or past J are 254 -- outside the problem: in neither fragment and not missing.
#define GP_INDICATORS(yr, J, j0, f1, f0, COUNT)                                                                        \
    {                                                                                                                  \
        uint32_t yw[2];                                                                                                \
        gp_load8((yr) + (j0), (yr) + (J), yw[0], yw[1]);                                                               \
        const int nv = (J) - (j0);                                    /* items of the row from j0 on (<= 0: none) */   \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                \
            const unsigned yy = (e < nv) ? ((yw[e >> 2] >> (8 * (e & 3))) & 0xffu) : 254u;                             \
            (f1)[e] = (yy == 1u) ? (_Float16)1.0f : (_Float16)0.0f;                                                    \
            (f0)[e] = (yy == 0u) ? (_Float16)1.0f : (_Float16)0.0f;                                                    \
            COUNT (yy == 255u) ? 1 : 0;                                                                                \
        }                                                                                                              \
    }

// The person-on-lane kernels (k_grid_post, k_grid_draw): a wave's unit is GP_MT tiles of 32 persons.  GP_UNIT_STATE declares what
// the operand phase keeps of them (its two halves apart for k_grid_draw, see there); GP_UNIT_PERSON(mt), inside the kernel's own loop over the tiles, sets it up: person pid[mt] =
// 32 GP_MT unit + 32 mt + (lane & 31), `row` = that person's index into y (in scope behind the macro) -- a person past the end
// reads a valid row, the first of the call, and is not stored -- and the missing count at zero.  Reads y, rows, nb, J, unit, l31.
#define GP_UNIT_ROWS                                                                                                   \
    const uint8_t* yr[GP_MT];                                                                                          \
    int64_t pid[GP_MT]
#define GP_UNIT_MISSING                                                                                                \
    int nmiss[GP_MT];                                                                                                  \
    float miss[GP_MT]
#define GP_UNIT_STATE GP_UNIT_ROWS; GP_UNIT_MISSING
#define GP_UNIT_PERSON(mt)                                                                                             \
    pid[mt] = unit * (32 * GP_MT) + mt * 32 + l31;                                                                     \
    const int64_t row = (pid[mt] < nb) ? (rows ? rows[pid[mt]] : pid[mt]) : (rows ? rows[0] : 0);                      \
    yr[mt] = y + row * J;                                                                                              \
    nmiss[mt] = 0; miss[mt] = 0.f

// GP_PASS(acc): the scaled ll of the unit at the node tiles ng .. ng + GP_NTG - 1 into f32x16 acc[GP_MT][GP_NTG] -- every sum
// over a fixed order of items that depends on neither the person's place in the batch nor the launch -- and, on the first pass
// (ng == 0), miss = (#missing) VX_LOGP_MISSING.  Reads img, J, KC, NT, ng, lane, half.
#define GP_PASS(acc)                                                                                                   \
    _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt)                                                               \
        _Pragma("unroll") for (int t = 0; t < GP_NTG; ++t) acc[mt][t] = zero16();                                      \
    for (int kc = 0; kc < KC; ++kc) {                                                                                  \
        f16x8 f1[GP_MT], f0[GP_MT];                                                                                    \
        const int j0 = kc * 16 + 8 * half;                                                                             \
        _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt)                                                           \
            GP_INDICATORS(yr[mt], J, j0, f1[mt], f0[mt], if (ng == 0) nmiss[mt] +=)                                    \
        _Pragma("unroll") for (int t = 0; t < GP_NTG; ++t) {                                                           \
            if (ng + t < NT) {                                                                                         \
                const uint4* p = img + (((int64_t)(ng + t) * KC + kc) * 4) * 64 + lane;                                \
                const f16x8 a1h = __builtin_bit_cast(f16x8, p[0]), a1l = __builtin_bit_cast(f16x8, p[64]);             \
                const f16x8 a0h = __builtin_bit_cast(f16x8, p[128]), a0l = __builtin_bit_cast(f16x8, p[192]);          \
                _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt) {                                                 \
                    acc[mt][t] = mfma_f16(a1h, f1[mt], acc[mt][t]);                                                    \
                    acc[mt][t] = mfma_f16(a1l, f1[mt], acc[mt][t]);                                                    \
                    acc[mt][t] = mfma_f16(a0h, f0[mt], acc[mt][t]);                                                    \
                    acc[mt][t] = mfma_f16(a0l, f0[mt], acc[mt][t]);                                                    \
                }                                                                                                      \
            }                                                                                                          \
        }                                                                                                              \
    }                                                                                                                  \
    if (ng == 0) {                                                                                                     \
        _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt) {                                                         \
            const int tot = nmiss[mt] + __shfl_xor(nmiss[mt], 32, 64);      /* the other half of the items */          \
            miss[mt] = (float)tot * VX_LOGP_MISSING;                                                                   \
        }                                                                                                              \
    }

// What a lane knows of its person over the nodes it has seen: the largest f = logw + ll and its node, and, with weights
// w = exp(f - m), the sums S0 = sum w, S1 = sum w (theta - ref), S2 = sum w (theta - ref)^2 about ref = the coordinates of
// THAT node.  The posterior's mass sits around its mode, so the moments about it are of the size of the variance itself:
// mean = ref + S1 / S0 and var = S2 / S0 - (S1 / S0)^2 cancel nothing that matters, wherever on the grid the person is
// (plain E[theta^2] - mean^2 loses the PSD of a person far from 0).  When a higher node turns up the sums move to it:
// rescaled by exp(m_old - m_new) and shifted by delta = ref_old - ref_new.
template <int DP>
struct GpState {
    float m, s0;
    int idx;
    float ref[DP], s1[DP], s2[DP];
};

template <int DP>
__device__ __forceinline__ void gp_move(GpState<DP>& st, float new_m, int new_idx, const float* __restrict__ new_ref) {
    const float sc = __expf(st.m - new_m);
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const float dl = st.ref[d] - new_ref[d];
        st.s2[d] = sc * fmaf(dl, fmaf(dl, st.s0, 2.0f * st.s1[d]), st.s2[d]);
        st.s1[d] = sc * fmaf(dl, st.s0, st.s1[d]);
        st.ref[d] = new_ref[d];
    }
    st.s0 *= sc;
    st.m = new_m;
    st.idx = new_idx;
}

// y u8 [n_local][J] (0 / 1 / 254 = outside the problem: nothing / 255 = missing: VX_LOGP_MISSING), rows or NULL.
// LDS: logw [NT * 32] (-inf past G), coord [NT * 32][DP] (zero past G and past D).
// A wave takes 64 persons at a time; every sum runs over a fixed order of items and nodes that depends on neither the
// person's place in the batch nor the launch: two calls give the same bits, and so does a person reached through `rows`.
template <int DP>
__global__ __launch_bounds__(GP_THREADS) void k_grid_post(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                          int64_t nb, int J, int G, int D, const uint4* __restrict__ img,
                                                          const float* __restrict__ logw, const float* __restrict__ coord,
                                                          float* __restrict__ loglik, float* __restrict__ mean,
                                                          float* __restrict__ sd, int32_t* __restrict__ argmax) {
    extern __shared__ __attribute__((aligned(16))) float gp_smem[];
    const int KC = gp_kc(J), NT = gp_nt(G), GP = NT * 32;
    float* lw = gp_smem;
    float* co = gp_smem + GP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    for (int i = tid; i < GP; i += GP_THREADS) {
        lw[i] = (i < G) ? logw[i] : -__builtin_inff();
#pragma unroll
        for (int d = 0; d < DP; ++d) co[i * DP + d] = (i < G && d < D) ? coord[(int64_t)i * D + d] : 0.f;
    }
    __syncthreads();
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave; unit < n_units; unit += (int64_t)gridDim.x * GP_WAVES) {
        GP_UNIT_STATE;
        GpState<DP> st[GP_MT];
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GP_UNIT_PERSON(mt);
            st[mt].m = GP_NEG; st[mt].s0 = 0.f; st[mt].idx = 0x7fffffff;
#pragma unroll
            for (int d = 0; d < DP; ++d) { st[mt].ref[d] = 0.f; st[mt].s1[d] = 0.f; st[mt].s2[d] = 0.f; }
        }
        for (int ng = 0; ng < NT; ng += GP_NTG) {
            f32x16 acc[GP_MT][GP_NTG];
            GP_PASS(acc)
            // the nodes of this pass, into the lane's running state
#pragma unroll
            for (int t = 0; t < GP_NTG; ++t) {
                if (ng + t < NT) {
                    const int g0 = (ng + t) * 32 + 4 * half;
#pragma unroll
                    for (int mt = 0; mt < GP_MT; ++mt) {
                        float f[16];
                        float tm = GP_NEG;
                        int ti = 0;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int g = g0 + (r & 3) + 8 * (r >> 2);
                            f[r] = fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g];
                            if (f[r] > tm) { tm = f[r]; ti = g; }                   // strict: ties stay with the lowest node
                        }
                        if (tm > st[mt].m) gp_move<DP>(st[mt], tm, ti, co + ti * DP);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int g = g0 + (r & 3) + 8 * (r >> 2);
                            const float w = __expf(f[r] - st[mt].m);
                            st[mt].s0 += w;
#pragma unroll
                            for (int d = 0; d < DP; ++d) {
                                const float dl = co[g * DP + d] - st[mt].ref[d];
                                const float wd = w * dl;
                                st[mt].s1[d] += wd;
                                st[mt].s2[d] = fmaf(wd, dl, st[mt].s2[d]);
                            }
                        }
                    }
                }
            }
        }
        // the two halves of a person's nodes: A = what lanes 0..31 hold, B = lanes 32..63; the sums move to the higher of the
        // two maxima (equal: the lower node) -- both lanes of a pair compute the same thing in the same order
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GpState<DP> ot;
            ot.m = __shfl_xor(st[mt].m, 32, 64);
            ot.s0 = __shfl_xor(st[mt].s0, 32, 64);
            ot.idx = __shfl_xor(st[mt].idx, 32, 64);
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                ot.ref[d] = __shfl_xor(st[mt].ref[d], 32, 64);
                ot.s1[d] = __shfl_xor(st[mt].s1[d], 32, 64);
                ot.s2[d] = __shfl_xor(st[mt].s2[d], 32, 64);
            }
            const bool other_wins = (ot.m > st[mt].m) || (ot.m == st[mt].m && ot.idx < st[mt].idx);
            GpState<DP> win = other_wins ? ot : st[mt];
            GpState<DP> los = other_wins ? st[mt] : ot;
            gp_move<DP>(los, win.m, win.idx, win.ref);
            const float s0 = win.s0 + los.s0;
            const float inv = 1.0f / s0;
            if (half == 0 && pid[mt] < nb) {
                loglik[pid[mt]] = win.m + logf(s0);
                argmax[pid[mt]] = win.idx;
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    if (d < D) {
                        const float m1 = (win.s1[d] + los.s1[d]) * inv;
                        const float m2 = (win.s2[d] + los.s2[d]) * inv;
                        mean[pid[mt] * D + d] = win.ref[d] + m1;
                        sd[pid[mt] * D + d] = sqrtf(fmaxf(fmaf(-m1, m1, m2), 0.f));
                    }
                }
            }
        }
    }
}
