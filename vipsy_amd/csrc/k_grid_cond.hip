// Conditioned grid posteriors: k_grid_post and k_grid_draw under a prior that differs from person to person -- the latent
// regression theta_i ~ N(Gamma^T x_i, Sigma) of IrtEngine.fit_population.  On the grid the log prior of a person with mean mu_i is
//
//     -1/2 theta_g^T Lambda theta_g + (Lambda mu_i) . theta_g + const_i,        Lambda = Sigma^-1:
//
// the shared log-weight logw[g] plus a TILT t_i . theta_g, t_i = Lambda mu_i of length D <= 3, plus a per-person normaliser.  The
// operand phase (GP_UNIT_* / GP_PASS of k_grid_post.hip), the image and the launch shape are those of the unconditioned kernels;
// what is here is the epilogue:
//
//     dot = t_0 c_0; dot = fmaf(t_d, c_d, dot), d = 1 .. D - 1              (c = coord[g], from LDS)
//     f   = (fmaf(acc, GP_UNSCALE, miss) + lw[g]) + dot                      the base term as k_grid_post parenthesises it
//     h   = lw[g] + dot                                                      the prior alone
//
// A zero tilt gives dot = +-0 and f = the bits of k_grid_post / k_grid_draw.
//
// Bit for bit with k_grid_post at a zero tilt means the same ROUNDINGS, and the library is built with floating-point contraction:
// where a product feeds a sum inside one basic block k_grid_post compiles to a fused multiply-add -- in the join the loser's moved
// sums times exp(m_los - m_win) added to the winner's, and ref + s1 / s0; in the node loop `s1[d] += w dl`, but only where the
// vectoriser has not paired that sum with `s0 += w` (gpc_s1_fused, read off the assembly of k_grid_post<1>, <2>, <3>).  This file
// spells those operations out, fmaf where k_grid_post fuses and a product rounded on its own (gpc_mul_rn) where it does not,
// instead of leaving them to where the compiler happens to put the block boundaries and the vector pairs of a longer epilogue;
// tests/test_gpu_pop.py holds the two kernels to each other on both builds of the library.
//
// If that test (test_zero_tilt_gives_the_unconditioned_bits) fails after a change of compiler -- `mean` or sqrt(cov_dd) off in the
// last bit for one D while `logjoint` and `argmax` still agree -- k_grid_post's choices have moved, not this file's arithmetic.
// Recipe: `make` keeps the device assembly beside the library (_lib/libvipsy_hip.gfx950.s).  In _Z11k_grid_postILi<D>EE..., D = 1, 2, 3:
//   1. The node loop (between the v_exp_f32 of one node and the next).  The sum s2 is always `v_mul wd = w dl` + `v_(pk_)fma s2 += wd
//      dl`.  For s1 look at what takes w as an operand: `v_pk_fma_f32 s1pair, w (op_sel broadcast), dlpair, s1pair` means FUSED for
//      that pair of d; `v_pk_add_f32 {s1, s0} += {wd, w}` means a SEPARATE product for that d.  Which d is which follows from the
//      ds_bpermute_b32 block of the join, which shuffles in source order: m, s0, idx, then ref[d], s1[d], s2[d] for d = 0, 1, ...
//      Set gpc_s1_fused to what is found.
//   2. The join (behind the v_rcp_f32 of 1 / s0).  Expected: `v_fmac win.s1 += sc * X`, `v_fmac win.s2 += sc * Y`, `v_fmac win.s0 +=
//      los.s0 * sc`, m1 = `v_mul inv, sum1`, mean = `v_fmac ref += inv * sum1`.  A v_mul + v_add in place of one of these v_fmac
//      means that product is no longer fused: write it as gpc_mul_rn and a sum in the join below.
//
// k_grid_post_cond<DP>, DP = D = 1, 2, 3: logjoint = lse_g f, lognorm = lse_g h (a second running log-sum-exp of the same shape,
// its halves joined as the first one's: the lower maximum's sum rescaled onto the higher), mean, argmax of f, and cov, the
// DP (DP + 1) / 2 upper-triangular second moments (00, 01, 02, 11, 12, 22) taken about the running MAP node as k_grid_post takes
// its diagonal: gpc_move carries the cross sums along, s2_de += dl_d s1_e + dl_e s1_d + dl_d dl_e s0, then the rescale.  A diagonal
// entry is fmaxf(fmaf(-m1, m1, m2), 0), the very expression k_grid_post takes the square root of; an off-diagonal entry is
// m2_de - m1_d m1_e.  The host forms loglik_i = logjoint_i - lognorm_i.  No atomics, no workspace, every sum in a fixed order.
//
// k_grid_draw_cond: k_grid_draw with coord [NT * 32][3] in LDS beside lw (zero past G and past D) and the tilt in GP_MT x 3
// registers (zero past D and for a person past the end), the staged f formed as above; noise, keys, fold and ties are
// k_grid_draw's.  One instantiation serves D = 1 .. 3: the padded terms add fmaf(0, 0, dot) = dot.
//
// Resources (hipcc of ROCm 7, -O3, gfx950, `make resources`): k_grid_post_cond<1> / <2> under (256, 2): 204 / 245 VGPRs, no AGPRs,
// no spill, occupancy 2 (left alone they take 197 / 246 + 64 AGPRs and one wave a SIMD); <3>: 256 VGPRs + 83 AGPRs, six vector
// registers parked in AGPRs, occupancy 1, as k_grid_post<3> (198 + 64).  NO scratch in any of them.  k_grid_draw_cond at PVC_CAP = 16
// draws a launch under (256, 2): 232 VGPRs (k_grid_draw: 225), 0 AGPRs, no vector spill, NO scratch, 75 scalar registers kept in
// lanes of a VGPR, occupancy 2 -- so the cap actually used is 16, k_grid_draw's, and the fall-back to 8 draws a launch was not needed.
#pragma once
#include "vx_common.h"
#include "k_grid_post.hip"
#include "k_grid_draw.hip"

#define GPC_MAXD 3               // dimensions of a conditioned call (SCORE_MAX_DIMS of grid.py)
// Draws a launch of k_grid_draw_cond (a multiple of 4).  16, as PV_CAP: no scratch there (the figures above); a draw does not
// depend on the cut into launches, so this number changes no result.
#define PVC_CAP 16

__host__ __device__ inline size_t pvc_lds_bytes(int G) {
    return ((size_t)gp_nt(G) * 32 * (1 + GPC_MAXD) + PV_FS_FLOATS) * sizeof(float);
}

// GpState with the full second moment: s2[k], k over the upper triangle row by row
template <int DP>
struct GpcState {
    float m, s0;
    int idx;
    float ref[DP], s1[DP], s2[DP * (DP + 1) / 2];
};

// (d, e), d <= e < D -> its place in the upper triangle of a D x D matrix, row by row
__host__ __device__ constexpr int gpc_tri(int D, int d, int e) { return d * D - d * (d - 1) / 2 + (e - d); }

template <int DP>
__device__ __forceinline__ void gpc_move(GpcState<DP>& st, float new_m, int new_idx, const float* __restrict__ new_ref) {
    const float sc = __expf(st.m - new_m);
    float dl[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) dl[d] = st.ref[d] - new_ref[d];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
#pragma unroll
        for (int e = 0; e < DP; ++e) {
            if (e < d) continue;
            const int k = gpc_tri(DP, d, e);
            if (e == d)
                st.s2[k] = sc * fmaf(dl[d], fmaf(dl[d], st.s0, 2.0f * st.s1[d]), st.s2[k]);      // gp_move's, bit for bit
            else
                st.s2[k] = sc * fmaf(dl[d], fmaf(dl[e], st.s0, st.s1[e]), fmaf(dl[e], st.s1[d], st.s2[k]));
        }
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        st.s1[d] = sc * fmaf(dl[d], st.s0, st.s1[d]);
        st.ref[d] = new_ref[d];
    }
    st.s0 *= sc;
    st.m = new_m;
    st.idx = new_idx;
}

// a product rounded on its own: no contraction into a sum that uses it
__device__ __forceinline__ float gpc_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// Whether k_grid_post<DP> forms `s1[d] += w dl` of its node loop as ONE fused operation (see the header): it does where the
// vectoriser pairs two of the s1 with each other (DP = 2; d = 1, 2 of DP = 3), and does not where it pairs s1[0] with s0 (DP = 1;
// d = 0 of DP = 3)
__host__ __device__ constexpr bool gpc_s1_fused(int DP, int d) { return DP == 2 || (DP == 3 && d > 0); }

// t . c over DP dimensions: the first product rounded on its own (see the header)
template <int DP>
__device__ __forceinline__ float gpc_dot(const float* t, const float* __restrict__ c) {
    float dot = __fmul_rn(t[0], c[0]);
#pragma unroll
    for (int d = 1; d < DP; ++d) dot = fmaf(t[d], c[d], dot);
    return dot;
}

// Arguments as k_grid_post, and tilt [nb][D] by BATCH POSITION (not through rows).  LDS as k_grid_post.
template <int DP>
__global__ __launch_bounds__(GP_THREADS, DP <= 2 ? 2 : 1) void k_grid_post_cond(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                               int64_t nb, int J, int G, int D, const uint4* __restrict__ img,
                                                               const float* __restrict__ logw, const float* __restrict__ coord,
                                                               const float* __restrict__ tilt, float* __restrict__ logjoint,
                                                               float* __restrict__ lognorm, float* __restrict__ mean,
                                                               float* __restrict__ cov, int32_t* __restrict__ argmax) {
    extern __shared__ __attribute__((aligned(16))) float gp_smem[];
    constexpr int TP = DP * (DP + 1) / 2;
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
        GpcState<DP> st[GP_MT];
        float tl[GP_MT][DP], hm[GP_MT], hs[GP_MT];            // the tilt; the prior's running maximum and sum
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GP_UNIT_PERSON(mt);
            st[mt].m = GP_NEG; st[mt].s0 = 0.f; st[mt].idx = 0x7fffffff;
            hm[mt] = GP_NEG; hs[mt] = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                st[mt].ref[d] = 0.f; st[mt].s1[d] = 0.f;
                tl[mt][d] = (pid[mt] < nb && d < D) ? tilt[pid[mt] * D + d] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < TP; ++k) st[mt].s2[k] = 0.f;
        }
        for (int ng = 0; ng < NT; ng += GP_NTG) {
            f32x16 acc[GP_MT][GP_NTG];
            GP_PASS(acc)
#pragma unroll
            for (int t = 0; t < GP_NTG; ++t) {
                if (ng + t < NT) {
                    const int g0 = (ng + t) * 32 + 4 * half;
#pragma unroll
                    for (int mt = 0; mt < GP_MT; ++mt) {
                        float f[16];
                        float tm = GP_NEG, th = GP_NEG;
                        int ti = 0;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int g = g0 + (r & 3) + 8 * (r >> 2);
                            const float dot = gpc_dot<DP>(tl[mt], co + g * DP);
                            f[r] = (fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g]) + dot;
                            if (f[r] > tm) { tm = f[r]; ti = g; }                   // strict: ties stay with the lowest node
                            th = fmaxf(th, lw[g] + dot);
                        }
                        if (tm > st[mt].m) gpc_move<DP>(st[mt], tm, ti, co + ti * DP);
                        if (th > hm[mt]) { hs[mt] *= __expf(hm[mt] - th); hm[mt] = th; }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int g = g0 + (r & 3) + 8 * (r >> 2);
                            const float w = __expf(f[r] - st[mt].m);
                            st[mt].s0 += w;
                            hs[mt] += __expf((lw[g] + gpc_dot<DP>(tl[mt], co + g * DP)) - hm[mt]);   // h again: the same bits
                            float dl[DP], wd[DP];
#pragma unroll
                            for (int d = 0; d < DP; ++d) {
                                dl[d] = co[g * DP + d] - st[mt].ref[d];
                                wd[d] = gpc_mul_rn(w, dl[d]);
                                st[mt].s1[d] = gpc_s1_fused(DP, d) ? fmaf(w, dl[d], st[mt].s1[d]) : st[mt].s1[d] + wd[d];
                            }
#pragma unroll
                            for (int d = 0; d < DP; ++d)
#pragma unroll
                                for (int e = 0; e < DP; ++e)
                                    if (e >= d) st[mt].s2[gpc_tri(DP, d, e)] = fmaf(wd[d], dl[e], st[mt].s2[gpc_tri(DP, d, e)]);
                        }
                    }
                }
            }
        }
        // the two halves of a person's nodes, as k_grid_post joins them; the prior's sum likewise: onto the higher maximum
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GpcState<DP> ot;
            ot.m = __shfl_xor(st[mt].m, 32, 64);
            ot.s0 = __shfl_xor(st[mt].s0, 32, 64);
            ot.idx = __shfl_xor(st[mt].idx, 32, 64);
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                ot.ref[d] = __shfl_xor(st[mt].ref[d], 32, 64);
                ot.s1[d] = __shfl_xor(st[mt].s1[d], 32, 64);
            }
#pragma unroll
            for (int k = 0; k < TP; ++k) ot.s2[k] = __shfl_xor(st[mt].s2[k], 32, 64);
            const float ohm = __shfl_xor(hm[mt], 32, 64), ohs = __shfl_xor(hs[mt], 32, 64);
            const bool other_wins = (ot.m > st[mt].m) || (ot.m == st[mt].m && ot.idx < st[mt].idx);
            const GpcState<DP> win = other_wins ? ot : st[mt];
            const GpcState<DP> los = other_wins ? st[mt] : ot;
            // the loser's sums moved to the winner's node and added, gp_move and the sum in one: the fused operations k_grid_post's
            // join compiles to, spelled out (see the header)
            const float sc = __expf(los.m - win.m);
            float dl[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) dl[d] = los.ref[d] - win.ref[d];
            const float s0 = fmaf(los.s0, sc, win.s0);
            const float inv = 1.0f / s0;
            const bool oh = ohm > hm[mt];
            const float hmax = oh ? ohm : hm[mt], hmin = oh ? hm[mt] : ohm;
            const float hsum = (oh ? ohs : hs[mt]) + (oh ? hs[mt] : ohs) * __expf(hmin - hmax);
            if (half == 0 && pid[mt] < nb) {
                logjoint[pid[mt]] = win.m + logf(s0);
                lognorm[pid[mt]] = hmax + logf(hsum);
                argmax[pid[mt]] = win.idx;
                float m1[DP];
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    const float sum1 = fmaf(sc, fmaf(dl[d], los.s0, los.s1[d]), win.s1[d]);
                    m1[d] = sum1 * inv;
                    if (d < D) mean[pid[mt] * D + d] = fmaf(sum1, inv, win.ref[d]);
                }
#pragma unroll
                for (int d = 0; d < DP; ++d) {
#pragma unroll
                    for (int e = 0; e < DP; ++e) {
                        if (e < d) continue;
                        const int k = gpc_tri(DP, d, e);
                        const float moved = (e == d) ? fmaf(dl[d], fmaf(dl[d], los.s0, los.s1[d] + los.s1[d]), los.s2[k])
                                                     : fmaf(dl[d], fmaf(dl[e], los.s0, los.s1[e]), fmaf(dl[e], los.s1[d], los.s2[k]));
                        const float m2 = fmaf(sc, moved, win.s2[k]) * inv;
                        const float c = (e == d) ? fmaxf(fmaf(-m1[d], m1[d], m2), 0.f) : fmaf(-m1[d], m1[e], m2);
                        if (e < D) cov[pid[mt] * (D * (D + 1) / 2) + gpc_tri(D, d, e)] = c;
                    }
                }
            }
        }
    }
}

// Arguments as k_grid_draw, and coord [G][D], tilt [nb][D] by batch position, 1 <= D <= 3.  LDS: pvc_lds_bytes.
__global__ __launch_bounds__(GP_THREADS, 2) void k_grid_draw_cond(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                                  int64_t nb, int J, int G, int D, const uint4* __restrict__ img,
                                                                  const float* __restrict__ logw, const float* __restrict__ coord,
                                                                  const float* __restrict__ tilt, uint64_t seed, int64_t row_offset,
                                                                  int base, int lo, int hi, int64_t stride,
                                                                  int32_t* __restrict__ node) {
    extern __shared__ __attribute__((aligned(16))) float pv_smem[];
    const int KC = gp_kc(J), NT = gp_nt(G), GP = NT * 32;
    float* lw = pv_smem;
    float* co = pv_smem + GP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    float* fs = pv_smem + GP * (1 + GPC_MAXD) + wave * (GP_MT * 16 * 64) + lane;  // this lane's column of the wave's staging
    for (int i = tid; i < GP; i += GP_THREADS) {
        lw[i] = (i < G) ? logw[i] : -__builtin_inff();
#pragma unroll
        for (int d = 0; d < GPC_MAXD; ++d) co[i * GPC_MAXD + d] = (i < G && d < D) ? coord[(int64_t)i * D + d] : 0.f;
    }
    __syncthreads();
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave; unit < n_units; unit += (int64_t)gridDim.x * GP_WAVES) {
        GP_UNIT_ROWS;
        uint32_t r_lo[GP_MT], r_hi[GP_MT];
        float bv[GP_MT][PVC_CAP];
        int bi[GP_MT][PVC_CAP];
        float tl[GP_MT][GPC_MAXD];
        GP_UNIT_MISSING;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GP_UNIT_PERSON(mt);
            const uint64_t r = (uint64_t)row_offset + (uint64_t)row;                // the noise's key goes by the ROW ...
            r_lo[mt] = (uint32_t)r; r_hi[mt] = (uint32_t)(r >> 32);
#pragma unroll
            for (int d = 0; d < GPC_MAXD; ++d) tl[mt][d] = (pid[mt] < nb && d < D) ? tilt[pid[mt] * D + d] : 0.f;   // ... the tilt by the batch position
#pragma unroll
            for (int s = 0; s < PVC_CAP; ++s) { bv[mt][s] = GP_NEG; bi[mt][s] = 0x7fffffff; }
        }
        for (int ng = 0; ng < NT; ng += GP_NTG) {
            f32x16 acc[GP_MT][GP_NTG];
            GP_PASS(acc)
#pragma unroll
            for (int t = 0; t < GP_NTG; ++t) {
                if (ng + t < NT) {
                    const int g0 = (ng + t) * 32 + 4 * half;
#pragma unroll
                    for (int mt = 0; mt < GP_MT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int g = g0 + (r & 3) + 8 * (r >> 2);
                            fs[(mt * 16 + r) * 64] = (fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g]) +
                                                     gpc_dot<GPC_MAXD>(tl[mt], co + g * GPC_MAXD);
                        }
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        const int g = g0 + (r & 3) + 8 * (r >> 2);                  // ascending in r, and from tile to tile
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            const float f = fs[(mt * 16 + r) * 64];
#pragma unroll
                            for (int q = 0; q < PVC_CAP / 4; ++q) {
                                const int m0 = base + 4 * q;
                                if (m0 + 3 >= lo && m0 < hi) {                      // (wave-uniform)
                                    const u32x4 w = philox4x32_10(r_lo[mt], r_hi[mt], (uint32_t)g,
                                                                  ((uint32_t)PV_STREAM << 16) | (uint32_t)(m0 >> 2), k0, k1);
                                    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                                    for (int k = 0; k < 4; ++k) {
                                        if (m0 + k >= lo && m0 + k < hi) {
                                            const float v = f + pv_gumbel(x[k]);
                                            if (v > bv[mt][4 * q + k]) { bv[mt][4 * q + k] = v; bi[mt][4 * q + k] = g; }   // strict: ties stay with the lowest node
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        // the two halves of a person's nodes: the higher value, on equal values the lower node
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
#pragma unroll
            for (int s = 0; s < PVC_CAP; ++s) {
                const int m = base + s;
                if (m >= lo && m < hi) {                                            // (wave-uniform)
                    const float ov = __shfl_xor(bv[mt][s], 32, 64);
                    const int oi = __shfl_xor(bi[mt][s], 32, 64);
                    const bool other_wins = (ov > bv[mt][s]) || (ov == bv[mt][s] && oi < bi[mt][s]);
                    if (half == 0 && pid[mt] < nb) node[pid[mt] * stride + m] = other_wins ? oi : bi[mt][s];
                }
            }
        }
    }
}
