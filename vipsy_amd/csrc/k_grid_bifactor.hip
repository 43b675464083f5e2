// Grid scores for bifactor / testlet models: one general dimension every item loads on, and S specific dimensions each of which
// only the items of one testlet load on.  The tensor-product grid of such a model has Gg Gh^S points, but given the general node
// the testlets are independent (Gibbons & Hedeker 1992), and each is a ONE-dimensional integral over its own specific factor:
//
//     L_i = sum_g w_g  prod_{j general-only} P(y_ij | theta_g)  prod_{s = 1..S} [ sum_h v_h prod_{j in s} P(y_ij | theta_g, u_h) ]
//
// -- the work of one two-dimensional grid (items x Gg x Gh), whatever S is.  In logs, with m_is(g) = logsumexp_h (log v_h +
// sum_{j in s} log P(y_ij | theta_g, u_h)) the bracket of testlet s,
//
//     F_i(g) = log w_g + (#missing_i) VX_LOGP_MISSING + sum_s m_is(g),        loglik_i = logsumexp_g F_i(g),
//
// F_i the log of the general MARGINAL posterior up to loglik_i: its moments are the general EAP / PSD, its argmax the node.
//
// Operand phase and orientation as k_grid_post.hip (the table is the A operand, the indicators the B operand, fp16 head + low of
// T 2^10 on v_mfma_f32_32x32x16_f16, four MFMAs a chunk, the person on the lane), with another meaning of a NODE TILE: tile g is
// the general node g, and its 32 rows are the specific nodes h = 0 .. Gh - 1.  Rows >= Gh are ZERO rows of the table -- not -inf:
// the -inf is the log-weight's, logv[h] = -inf past Gh, so they add exp(-inf) = 0 to a bracket.
//
// Operand image (k_grid_table_bifactor): [Gg][KC][4: T1 head, T1 low, T0 head, T0 low][64 lanes][8 fp16], the layout of
// k_grid_post.hip with KC counting the chunks of the TESTLET LAYOUT of the items: testlet after testlet, each padded to whole
// chunks of 16, chunks tl_start[t] .. tl_start[t + 1] - 1 for testlet t.  The general-only items form a pseudo-testlet whose table
// does not depend on h (its bracket is its log-likelihood plus log sum_h v_h = 0).  Slot jp of the layout holds item col[jp] of the
// model (-1: padding, a zero column) whose specific dimension is sdim[jp] (-1: none).
//
// The responses arrive IN the testlet layout: y u8 [nb][16 KC], padding slots 254 ("outside the problem": in neither indicator,
// not missing) -- the caller permutes them, a slab of persons at a time, so that GP_INDICATORS serves unchanged.
//
// After a testlet's chunks a person's 32 values over h sit in the lane's 16 accumulator registers and in lane ^ 32, so m is a
// loop over the lane's registers and one __shfl_xor(.., 32) each for the maximum and the sum.  Both lanes of a pair end up with
// the same bits (max and + of two floats commute), so F and the running state of GpState<1> are carried twice and never merged.
// Nothing of size persons x (Gg Gh) touches memory.  Every sum has a fixed order -- chunks ascending inside a testlet, the
// registers of h, testlets ascending, g ascending -- that depends on neither the person's place in the batch nor the launch.
//
// specific = true: k_grid_bifactor also leaves F_i(g), one float a person and GENERAL node, in a workspace [unit of 64
// persons][Gg][64] (a lane's store and load are coalesced), and k_grid_bifactor_spec -- testlet outer, g inner -- recomputes the
// tiles and accumulates, a person and testlet, the two scalars E1 = sum_g post_i(g) E[u | g, y_is] and E2 = sum_g post_i(g)
// E[u^2 | g, y_is], post_i(g) = exp(F_i(g) - loglik_i).  No per-testlet accumulator array, no limit on S; the MFMA work twice.
//
// Limits (vx_grid_bifactor*: VX_EINVAL beyond): 2 <= Gg <= 256, 1 <= Gh <= 32, KC <= 1024, J <= 1024, image <= 512 MB.
#pragma once
#include "k_grid_post.hip"

#define GB_NG 2                  // general nodes a pass over a testlet's chunks: one decoding of the indicators serves both

// The scaled sums of the unit over the chunks c0 .. c1 - 1 at the general nodes g0 .. g0 + GB_NG - 1 into f32x16 acc[GP_MT][GB_NG].
// Reads yr, JP, KC, Gg, img, lane, half.
#define GB_TESTLET(acc, g0, c0, c1)                                                                                    \
    _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt)                                                               \
        _Pragma("unroll") for (int t = 0; t < GB_NG; ++t) acc[mt][t] = zero16();                                       \
    for (int kc = (c0); kc < (c1); ++kc) {                                                                             \
        f16x8 f1[GP_MT], f0[GP_MT];                                                                                    \
        const int j0 = kc * 16 + 8 * half;                                                                             \
        _Pragma("unroll") for (int mt = 0; mt < GP_MT; ++mt)                                                           \
            GP_INDICATORS(yr[mt], JP, j0, f1[mt], f0[mt], gb_none +=)                                                  \
        _Pragma("unroll") for (int t = 0; t < GB_NG; ++t) {                                                            \
            if ((g0) + t < Gg) {                                                                                       \
                const uint4* p = img + (((int64_t)((g0) + t) * KC + kc) * 4) * 64 + lane;                              \
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
    }

// What both kernels keep in LDS: the testlets' chunk starts, and logv / u over the 32 rows of a tile (-inf / 0 past Gh)
#define GB_SHARED                                                                                                      \
    __shared__ int tls[GB_MAXKC + 1];                                                                                  \
    __shared__ float lv[32], uu[32]
#define GB_FILL_SHARED                                                                                                 \
    for (int i = tid; i <= n_tl; i += GP_THREADS) tls[i] = tl_start[i];                                                \
    if (tid < 32) {                                                                                                    \
        lv[tid] = (tid < Gh) ? logv[tid] : -__builtin_inff();                                                          \
        uu[tid] = (tid < Gh) ? u[tid] : 0.f;                                                                           \
    }

// The rows of the unit's persons in the testlet layout (a person past the end reads the first row and is not stored)
#define GB_UNIT_PERSON(mt)                                                                                             \
    pid[mt] = unit * (32 * GP_MT) + mt * 32 + l31;                                                                     \
    yr[mt] = y + ((pid[mt] < nb) ? pid[mt] : 0) * JP

// One table cell per (general node, specific node, slot): z = Dc (b_j + a_general,j theta_g + a_sdim,j u_h), the cell of
// k_grid_table_irt.  a [D][J], b, c_un, d_un [J]: the leaves as they stand; col, sdim int32 [16 KC].
template <int MODEL>
__global__ __launch_bounds__(256) void k_grid_table_bifactor(int D, int J, int Gg, int Gh, int KC, int general, float Dc,
                                                             const float* __restrict__ theta_g, const float* __restrict__ u,
                                                             const int32_t* __restrict__ col, const int32_t* __restrict__ sdim,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ c_un, const float* __restrict__ d_un,
                                                             uint16_t* __restrict__ img) {
    const int JP = KC * 16, total = Gg * 32 * JP;                  // (<= 2^26 cells: 8 bytes a cell, and the image <= 512 MB)
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int gp = idx / JP, jp = idx - gp * JP, g = gp >> 5, h = gp & 31;
        const int j = col[jp];
        float t1 = 0.f, t0 = 0.f;
        if (h < Gh && j >= 0 && j < J) {
            float s = fmaf(theta_g[g], a[(int64_t)general * J + j], b[j]);
            const int sd = sdim[jp];
            if (sd >= 0 && sd < D) s = fmaf(u[h], a[(int64_t)sd * J + j], s);
            const float z = Dc * s;
            const float c = (MODEL >= 3) ? fminf(sigmoidf_(c_un[j]), 1.0f - VX_EPS32) : 0.f;
            const float dd = (MODEL >= 4) ? fminf(sigmoidf_(d_un[j]), 1.0f - VX_EPS32) : 1.0f;
            const float omd = (MODEL >= 4) ? fmaxf(sigmoidf_(-d_un[j]), VX_EPS32) : 0.f;
            float dz, dc, ddd;
            irt_cell<MODEL>(z, 1u, c, dd, omd, t1, dz, dc, ddd);
            irt_cell<MODEL>(z, 0u, c, dd, omd, t0, dz, dc, ddd);
        }
        gp_put(img, KC, gp, jp, t1, t0);
    }
}

// v[r] = acc[r] 2^-10 + logv[h(r)] of a lane's 16 rows, and their maximum over both halves of the tile
#define GB_ROWS(a, v, mx)                                                                                              \
    float v[16];                                                                                                       \
    float mx = GP_NEG;                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                   \
        v[r] = fmaf((a)[r], GP_UNSCALE, lv[4 * half + (r & 3) + 8 * (r >> 2)]);                                        \
        mx = fmaxf(mx, v[r]);                                                                                          \
    }                                                                                                                  \
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64))

// y u8 [nb][16 KC] in the testlet layout; tl_start int32 [n_tl + 1] on the device; logw, coord [Gg]; logv, u [Gh]; fws NULL or
// [ceil(nb / 64)][Gg][64].  A wave takes 64 persons at a time.
__global__ __launch_bounds__(GP_THREADS) void k_grid_bifactor(const uint8_t* __restrict__ y, int64_t nb, int KC, int Gg, int Gh,
                                                              const int32_t* __restrict__ tl_start, int n_tl,
                                                              const uint4* __restrict__ img, const float* __restrict__ logw,
                                                              const float* __restrict__ coord, const float* __restrict__ logv,
                                                              const float* __restrict__ u, float* __restrict__ loglik,
                                                              float* __restrict__ mean, float* __restrict__ sd,
                                                              int32_t* __restrict__ argmax, float* __restrict__ fws) {
    GB_SHARED;
    __shared__ float lw[GB_MAXGG], co[GB_MAXGG];
    const int JP = KC * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    GB_FILL_SHARED
    for (int i = tid; i < Gg; i += GP_THREADS) { lw[i] = logw[i]; co[i] = coord[i]; }
    __syncthreads();
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave; unit < n_units; unit += (int64_t)gridDim.x * GP_WAVES) {
        GP_UNIT_ROWS;
        float miss[GP_MT];
        GpState<1> st[GP_MT];
        int gb_none = 0;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GB_UNIT_PERSON(mt);
            st[mt].m = GP_NEG; st[mt].s0 = 0.f; st[mt].idx = 0x7fffffff;
            st[mt].ref[0] = 0.f; st[mt].s1[0] = 0.f; st[mt].s2[0] = 0.f;
        }
        // the missing cells of the row, once: they enter every F as one constant
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            int nmiss = 0;
            for (int kc = 0; kc < KC; ++kc) {
                f16x8 d1, d0;
                GP_INDICATORS(yr[mt], JP, kc * 16 + 8 * half, d1, d0, nmiss +=)
                (void)d1; (void)d0;
            }
            miss[mt] = (float)(nmiss + __shfl_xor(nmiss, 32, 64)) * VX_LOGP_MISSING;
        }
        for (int g0 = 0; g0 < Gg; g0 += GB_NG) {
            float F[GP_MT][GB_NG];
#pragma unroll
            for (int mt = 0; mt < GP_MT; ++mt)
#pragma unroll
                for (int t = 0; t < GB_NG; ++t) F[mt][t] = ((g0 + t < Gg) ? lw[g0 + t] : 0.f) + miss[mt];
            for (int tl = 0; tl < n_tl; ++tl) {
                f32x16 acc[GP_MT][GB_NG];
                GB_TESTLET(acc, g0, tls[tl], tls[tl + 1])
#pragma unroll
                for (int t = 0; t < GB_NG; ++t) {
                    if (g0 + t < Gg) {
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            GB_ROWS(acc[mt][t], v, mx);
                            float s = 0.f;
#pragma unroll
                            for (int r = 0; r < 16; ++r) s += __expf(v[r] - mx);
                            s += __shfl_xor(s, 32, 64);
                            F[mt][t] += mx + logf(s);
                        }
                    }
                }
            }
            // the general nodes of this pass, into the running state (as k_grid_post folds a node; both halves alike)
#pragma unroll
            for (int t = 0; t < GB_NG; ++t) {
                if (g0 + t < Gg) {
                    const int g = g0 + t;
#pragma unroll
                    for (int mt = 0; mt < GP_MT; ++mt) {
                        const float f = F[mt][t];
                        if (f > st[mt].m) gp_move<1>(st[mt], f, g, co + g);          // strict: ties stay with the lowest node
                        const float w = __expf(f - st[mt].m);
                        const float dl = co[g] - st[mt].ref[0];
                        const float wd = w * dl;
                        st[mt].s0 += w;
                        st[mt].s1[0] += wd;
                        st[mt].s2[0] = fmaf(wd, dl, st[mt].s2[0]);
                    }
                    if (fws) fws[(unit * Gg + g) * 64 + lane] = half ? F[1][t] : F[0][t];      // person 32 half + l31 of the unit
                }
            }
        }
        (void)gb_none;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            if (half == 0 && pid[mt] < nb) {
                const float inv = 1.0f / st[mt].s0;
                const float m1 = st[mt].s1[0] * inv, m2 = st[mt].s2[0] * inv;
                loglik[pid[mt]] = st[mt].m + logf(st[mt].s0);
                argmax[pid[mt]] = st[mt].idx;
                mean[pid[mt]] = st[mt].ref[0] + m1;
                sd[pid[mt]] = sqrtf(fmaxf(fmaf(-m1, m1, m2), 0.f));
            }
        }
    }
}

// The specific moments: testlet outer, g inner.  loglik [nb] and fws as k_grid_bifactor left them; mean_s, sd_s [n_tl][nb]
// (testlet-major: a lane's stores are coalesced), the pseudo-testlet's row included (its table does not depend on h: the moments
// of the grid prior).
__global__ __launch_bounds__(GP_THREADS) void k_grid_bifactor_spec(const uint8_t* __restrict__ y, int64_t nb, int KC, int Gg, int Gh,
                                                                   const int32_t* __restrict__ tl_start, int n_tl,
                                                                   const uint4* __restrict__ img, const float* __restrict__ logv,
                                                                   const float* __restrict__ u, const float* __restrict__ loglik,
                                                                   const float* __restrict__ fws, float* __restrict__ mean_s,
                                                                   float* __restrict__ sd_s) {
    GB_SHARED;
    const int JP = KC * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    GB_FILL_SHARED
    __syncthreads();
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave; unit < n_units; unit += (int64_t)gridDim.x * GP_WAVES) {
        GP_UNIT_ROWS;
        float ll[GP_MT];
        int gb_none = 0;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GB_UNIT_PERSON(mt);
            ll[mt] = loglik[(pid[mt] < nb) ? pid[mt] : 0];
        }
        for (int tl = 0; tl < n_tl; ++tl) {
            float E1[GP_MT], E2[GP_MT];
#pragma unroll
            for (int mt = 0; mt < GP_MT; ++mt) { E1[mt] = 0.f; E2[mt] = 0.f; }
            for (int g0 = 0; g0 < Gg; g0 += GB_NG) {
                f32x16 acc[GP_MT][GB_NG];
                GB_TESTLET(acc, g0, tls[tl], tls[tl + 1])
#pragma unroll
                for (int t = 0; t < GB_NG; ++t) {
                    if (g0 + t < Gg) {
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            GB_ROWS(acc[mt][t], v, mx);
                            float s = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const float uh = uu[4 * half + (r & 3) + 8 * (r >> 2)];
                                const float e = __expf(v[r] - mx), eu = e * uh;
                                s += e;
                                s1 += eu;
                                s2 = fmaf(eu, uh, s2);
                            }
                            s += __shfl_xor(s, 32, 64);
                            s1 += __shfl_xor(s1, 32, 64);
                            s2 += __shfl_xor(s2, 32, 64);
                            const float pw = __expf(fws[(unit * Gg + g0 + t) * 64 + mt * 32 + l31] - ll[mt]) / s;
                            E1[mt] = fmaf(pw, s1, E1[mt]);
                            E2[mt] = fmaf(pw, s2, E2[mt]);
                        }
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < GP_MT; ++mt) {
                if (half == 0 && pid[mt] < nb) {
                    mean_s[(int64_t)tl * nb + pid[mt]] = E1[mt];
                    sd_s[(int64_t)tl * nb + pid[mt]] = sqrtf(fmaxf(fmaf(-E1[mt], E1[mt], E2[mt]), 0.f));
                }
            }
        }
        (void)gb_none;
    }
}
