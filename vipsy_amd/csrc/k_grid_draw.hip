// Plausible values: draws of a person's node from the grid posterior of k_grid_post.hip, p_i(g) ~ exp(logw[g] + ll[i][g]),
// by the Gumbel-max rule -- node = argmax_g (f_g + noise_g), f = logw + ll, noise = -log(-log u) -- which needs no
// normalisation, no second pass over the nodes and no cumulative sum across lanes: one more running maximum of the kind
// k_grid_post keeps for the MAP node, one a draw.  Nothing of size [n][G] leaves the chip, no atomics, no workspace.
//
// Operand phase: GP_UNIT_* / GP_PASS of k_grid_post.hip, what the posterior kernel runs (the image of vx_grid_table_*, indicator
// fragments by GP_INDICATORS, four v_mfma_f32_32x32x16_f16 an item chunk, the person on the lane, GP_MT person tiles a wave, GP_NTG node
// tiles a pass), and f is formed by the same expression, fmaf(acc, GP_UNSCALE, miss) + lw[g]: the bits the posterior kernel
// sees.  What is here is what differs: the LDS staging of f, the noise, the fold and the keys.
//
// Noise (restated in numpy by tests/pv_cases.py): with r = row_offset + row (row = the index into y, GP_UNIT_PERSON's: rows[pid] where
// rows is given, never the place in the batch), m the ABSOLUTE draw index and g the node,
//     w = philox4x32_10(lo32(r), hi32(r), g, (PV_STREAM << 16) | (m >> 2); key lo32(seed), hi32(seed)),   x = word m & 3 of w,
//     u = ((x >> 9) + 0.5) 2^-23 = (2 (x >> 9) + 1) 2^-24,        noise = -log(-log(u)).
// The odd numerator is below 2^24, so u is exact in float32 and lies in [2^-24, 1 - 2^-24]: noise in about [-2.82, 16.7],
// never infinite (u01() of vx_common.h rounds its top word to 1.0).  A draw depends on (seed, r, g, m) alone: not on the
// launch shape, the chunking of the draws, the batch or `rows`.  The inner logarithm is the library's logf: it is accurate
// RELATIVE to its result where u -> 1 (-log u -> 6e-8), which is what the outer logarithm turns into absolute error of the
// noise; the outer one is fast_log (L = -log u is a normal float in [6e-8, 16.7]; absolute error <= 1.5e-7 |log L| <= 2.5e-6,
// small beside the 1e-4 by which the tests tell two nodes apart).
//
// Fold: a lane keeps, for each of its GP_MT persons and each draw of the launch, the best perturbed value and its node over
// the lane's nodes, visited in ASCENDING order and replaced on strictly greater only (ties: the lowest node).  Nodes >= G
// carry -inf and never win.  The two halves of a person's nodes (lane ^ 32) meet once at the end: the higher value, on
// equal values the lower node.  Lanes with half == 0 store int32 node[pid][m].
//
// Code size: one (person, node, four draws) costs one Philox call (~90 VALU) and four times (two logarithms, the fold),
// ~180 instructions; unrolled over the 16 accumulator registers x GP_MT x GP_NTG x the draws of a launch that is several
// hundred KB of straight-line code against 64 KB of instruction cache.  So a node tile's f goes through a wave-private piece of
// LDS (each lane reads back what it wrote: no barrier), and the loop over a lane's 16 nodes is a real loop whose body holds
// the GP_MT persons x PV_CAP draws -- the state, bv / bi, is indexed by unrolled loops only and stays in registers.
//
// Draws a launch: PV_CAP = 16 (four Philox calls a node): the state is 2 x GP_MT x 16 = 64 registers beside the 64 of the
// accumulators.  vx_grid_posterior runs k_grid_post at two waves a SIMD (k_grid_post<1>: 152 VGPRs + 64 AGPRs of the 256 a wave
// has then -- the two files are one on gfx950); left alone the compiler takes 224 + 64 for this kernel and one wave a SIMD,
// so the second launch bound asks for two: hipcc (ROCm 7) -O3 then reports 225 VGPRs, 0 AGPRs, no vector spill, no scratch,
// 58 scalar registers kept in lanes of a VGPR (the round keys of Philox and the masks of the draw guards), occupancy 2.
// With PV_CAP = 8 it is 185 and occupancy 2 with or without the bound.  The launch covers the slots
// [base, base + PV_CAP), base a multiple of 4, and stores the draws lo <= m < hi; vx_grid_draw loops over the chunks.
//
// Limits: those of k_grid_post (J <= 1024, G <= 1024, nb >= 1), draws 0 <= m < 1024.
#pragma once
#include "vx_common.h"
#include "k_grid_post.hip"

#define PV_CAP 16                                  // draws a launch (a multiple of 4: one Philox call serves four)
#define PV_MAXDRAWS 1024                           // absolute draw indices: m >> 2 shares counter word 3 with PV_STREAM
#define PV_FS_FLOATS (GP_WAVES * GP_MT * 16 * 64)  // the staging of one node tile's f: [wave][person tile][register][lane]

__host__ __device__ inline size_t pv_lds_bytes(int G) { return ((size_t)gp_nt(G) * 32 + PV_FS_FLOATS) * sizeof(float); }

// uniform word -> Gumbel noise (see above)
__device__ __forceinline__ float pv_gumbel(uint32_t x) {
    const float u = (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f;
    return -fast_log(-logf(u));
}

__global__ __launch_bounds__(GP_THREADS, 2) void k_grid_draw(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                          int64_t nb, int J, int G, const uint4* __restrict__ img,
                                                          const float* __restrict__ logw, uint64_t seed, int64_t row_offset,
                                                          int base, int lo, int hi, int64_t stride, int32_t* __restrict__ node) {
    extern __shared__ __attribute__((aligned(16))) float pv_smem[];
    const int KC = gp_kc(J), NT = gp_nt(G), GP = NT * 32;
    float* lw = pv_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    float* fs = pv_smem + GP + wave * (GP_MT * 16 * 64) + lane;          // this lane's column of the wave's staging
    for (int i = tid; i < GP; i += GP_THREADS) lw[i] = (i < G) ? logw[i] : -__builtin_inff();
    __syncthreads();
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    for (int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave; unit < n_units; unit += (int64_t)gridDim.x * GP_WAVES) {
        GP_UNIT_ROWS;                        // GP_UNIT_STATE in two halves around the kernel's own: register assignment follows
        uint32_t r_lo[GP_MT], r_hi[GP_MT];   // the order of declaration, and in this order the kernel compiles to what it was
        float bv[GP_MT][PV_CAP];
        int bi[GP_MT][PV_CAP];
        GP_UNIT_MISSING;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GP_UNIT_PERSON(mt);
            const uint64_t r = (uint64_t)row_offset + (uint64_t)row;                // the noise's key, formed here: row is dead in the passes
            r_lo[mt] = (uint32_t)r; r_hi[mt] = (uint32_t)(r >> 32);
#pragma unroll
            for (int s = 0; s < PV_CAP; ++s) { bv[mt][s] = GP_NEG; bi[mt][s] = 0x7fffffff; }
        }
        for (int ng = 0; ng < NT; ng += GP_NTG) {
            f32x16 acc[GP_MT][GP_NTG];
            GP_PASS(acc)
            // the nodes of this pass, tile by tile: f through the lane's column of the staging, then node by node
#pragma unroll
            for (int t = 0; t < GP_NTG; ++t) {
                if (ng + t < NT) {
                    const int g0 = (ng + t) * 32 + 4 * half;
#pragma unroll
                    for (int mt = 0; mt < GP_MT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            fs[(mt * 16 + r) * 64] = fmaf(acc[mt][t][r], GP_UNSCALE, miss[mt]) + lw[g0 + (r & 3) + 8 * (r >> 2)];
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        const int g = g0 + (r & 3) + 8 * (r >> 2);                  // ascending in r, and from tile to tile
#pragma unroll
                        for (int mt = 0; mt < GP_MT; ++mt) {
                            const float f = fs[(mt * 16 + r) * 64];
#pragma unroll
                            for (int q = 0; q < PV_CAP / 4; ++q) {
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
            for (int s = 0; s < PV_CAP; ++s) {
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
