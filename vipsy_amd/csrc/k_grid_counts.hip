// Expected counts from the grid posteriors (the Bock-Aitkin E-step): with p_i(g) = exp(logw_g + ll_i(g) - loglik_i), the posterior
// of person i over the nodes (k_grid_post.hip gives ll and, as its output, loglik),
//
//     n1[j][g] = sum_i p_i(g) [y_ij == 1]      n0[j][g] = sum_i p_i(g) [y_ij == 0]      mass[g] = sum_i p_i(g)
//
// Two chained MFMA products on v_mfma_f32_32x32x16_f16, p never leaving the chip:
//
//   1. ll, TRANSPOSED against k_grid_post: the indicator is the A operand (lane = person l & 31, 8 items) and the table image's
//      fragment the B operand (lane = node l & 31, the same 8 items) -- the image and GP_INDICATORS serve as they are.  The accumulator
//      has the NODE on the lane and 16 persons in the lane's registers (rows crow32(r, half)).  p = exp(f - loglik_i) with
//      f = acc 2^-10 + miss_i + logw_g as the posterior kernel forms it: the normaliser is known, so there is no running
//      maximum and no cross-lane traffic.
//   2. tables[item][node] += indicator^T[item][person] p[person][node].  The contraction runs over persons, and an MFMA's k-slots
//      may hold them in any order as long as A and B agree: registers 0..7 and 8..15 of the accumulator of (1) ARE two B
//      fragments once p 2^14 is split into two fp16 terms (p <= 1: heads below 2^15, and the low term of every p that matters
//      -- p >= 2^-17 -- is a normal fp16; the scale comes off the fp32 sums exactly).  Slot e of lane half h in k-step s is
//      person 16 s + 8 (e >> 2) + 4 h + (e & 3) of the unit.  The A fragment is the 0/1 indicator of item l & 31 for those
//      eight persons: byte gathers from the response rows the workgroup has just read (L1 / L2).
//
// Output-stationary: a workgroup of eight waves owns NTG node tiles and a contiguous chunk of persons.  A round is 256 persons:
// every wave runs (1) for its own unit of 32 and leaves p as fragments in LDS; then every wave runs (2) over all eight units
// for ITS item tiles (tile = wave + 8 i, i < IT), whose accumulators stay in its registers for the whole chunk:
// 2 indicators x IT x NTG tiles of 16 registers, 128 at most.  Each (node group, chunk) writes its columns of slab `chunk`
// ([n1 | n0 | mass]); the slabs are added in ascending order by k_reduce_slabs.  Every sum has a fixed order: the same call
// gives the same bits.  No float atomics.
//
// Response bytes as in k_grid_post: 255 adds VX_LOGP_MISSING to ll and enters neither table, 254 adds nothing anywhere; a
// person with no response adds their prior to mass.
#pragma once
#include "k_grid_post.hip"

// GC_THREADS, GC_WAVES, GC_ROUND and the launch for (nb, J, G) -- GcPlan, gc_plan -- are in grid_plan.h
#define GC_PSCALE 16384.0f              // 2^14 into the fp16 split of p ...
#define GC_PUNSCALE 6.103515625e-05f    // ... and off the fp32 accumulators (exact)

template <int NTG>
constexpr size_t gc_lds_bytes() {
    // p fragments [waves][NTG][2 k-steps][head, low][64 lanes] x 16 B; rows int64 [waves][32]; miss, loglik [waves][32];
    // logw [NTG * 32]; mass partials [waves][NTG * 32]
    return (size_t)GC_WAVES * NTG * 4 * 64 * 16 + (size_t)GC_WAVES * 32 * 8 + 2 * (size_t)GC_WAVES * 32 * 4 + (size_t)NTG * 32 * 4 +
           (size_t)GC_WAVES * NTG * 32 * 4;
}

template <int IT, int NTG>
__global__ __launch_bounds__(GC_THREADS) void k_grid_counts(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                            int64_t nb, int J, int G, const uint4* __restrict__ img,
                                                            const float* __restrict__ logw, const float* __restrict__ loglik,
                                                            int n_groups, int64_t rounds_per_chunk, float* __restrict__ slabs,
                                                            int64_t slab_len) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gc_smem[];
    uint4* pbuf = (uint4*)gc_smem;
    int64_t* rowbuf = (int64_t*)(pbuf + GC_WAVES * NTG * 4 * 64);
    float* missb = (float*)(rowbuf + GC_WAVES * 32);
    float* lkb = missb + GC_WAVES * 32;
    float* lw = lkb + GC_WAVES * 32;
    float* massb = lw + NTG * 32;
    const int KC = gp_kc(J), NT = gp_nt(G), NIT = (J + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int grp = (int)(blockIdx.x % (unsigned)n_groups);
    const int64_t chunk = blockIdx.x / (unsigned)n_groups;
    const int nt0 = grp * NTG;
    if (tid < NTG * 32) {
        const int g = nt0 * 32 + tid;
        lw[tid] = (g < G) ? logw[g] : -__builtin_inff();
    }
    f32x16 c1[IT][NTG], c0[IT][NTG];
    float mass[NTG];
#pragma unroll
    for (int t = 0; t < NTG; ++t) {
        mass[t] = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) { c1[i][t] = zero16(); c0[i][t] = zero16(); }
    }
    __syncthreads();
    for (int64_t rd = 0; rd < rounds_per_chunk; ++rd) {
        const int64_t base = (chunk * rounds_per_chunk + rd) * GC_ROUND;          // the round's first person
        if (base >= nb) break;                                                    // (the same for every wave)
        // ---- (1) this wave's unit: ll of 32 persons at the group's nodes.  Persons past nb read a valid row and get p = 0.
        {
            const int64_t pid = base + wave * 32 + l31;
            const bool valid = pid < nb;
            const int64_t row = rows ? rows[valid ? pid : 0] : (valid ? pid : 0);
            const uint8_t* yr = y + row * J;
            f32x16 acc[NTG];
#pragma unroll
            for (int t = 0; t < NTG; ++t) acc[t] = zero16();
            int nmiss = 0;
            for (int kc = 0; kc < KC; ++kc) {
                const int j0 = kc * 16 + 8 * half;
                f16x8 f1, f0;
                GP_INDICATORS(yr, J, j0, f1, f0, nmiss +=)
#pragma unroll
                for (int t = 0; t < NTG; ++t) {
                    if (nt0 + t < NT) {
                        const uint4* p = img + (((int64_t)(nt0 + t) * KC + kc) * 4) * 64 + lane;
                        const f16x8 b1h = __builtin_bit_cast(f16x8, p[0]), b1l = __builtin_bit_cast(f16x8, p[64]);
                        const f16x8 b0h = __builtin_bit_cast(f16x8, p[128]), b0l = __builtin_bit_cast(f16x8, p[192]);
                        acc[t] = mfma_f16(f1, b1h, acc[t]);
                        acc[t] = mfma_f16(f1, b1l, acc[t]);
                        acc[t] = mfma_f16(f0, b0h, acc[t]);
                        acc[t] = mfma_f16(f0, b0l, acc[t]);
                    }
                }
            }
            const int tot = nmiss + __shfl_xor(nmiss, 32, 64);                    // the other half of the items
            if (half == 0) {
                missb[wave * 32 + l31] = (float)tot * VX_LOGP_MISSING;
                lkb[wave * 32 + l31] = valid ? loglik[pid] : __builtin_inff();    // f - inf = -inf: p = 0
                rowbuf[wave * 32 + l31] = valid ? row : (int64_t)-1;
            }
            __syncthreads();
            // the person constants of the lane's 16 registers: rows 8 q + 4 half + (0..3)
            float ms[16], lk[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 m4 = *(const f32x4*)(missb + wave * 32 + 8 * q + 4 * half);
                const f32x4 l4 = *(const f32x4*)(lkb + wave * 32 + 8 * q + 4 * half);
#pragma unroll
                for (int i = 0; i < 4; ++i) { ms[4 * q + i] = m4[i]; lk[4 * q + i] = l4[i]; }
            }
#pragma unroll
            for (int t = 0; t < NTG; ++t) {
                const float lwg = lw[t * 32 + l31];
                float pv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float f = fmaf(acc[t][r], GP_UNSCALE, ms[r]) + lwg;
                    pv[r] = (nt0 + t < NT) ? __expf(f - lk[r]) : 0.f;
                    mass[t] += pv[r];
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = pv[8 * s + e];
                    f16x8 fh, fl;
                    split2h_frag(v, GC_PSCALE, fh, fl);
                    uint4* dst = pbuf + (((wave * NTG + t) * 2 + s) * 2) * 64 + lane;
                    dst[0] = __builtin_bit_cast(uint4, fh);
                    dst[64] = __builtin_bit_cast(uint4, fl);
                }
            }
        }
        __syncthreads();
        // ---- (2) every unit of the round into this wave's item tiles
        for (int u = 0; u < GC_WAVES; ++u) {
            if (base + 32 * u >= nb) break;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                int64_t rr[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) rr[e] = rowbuf[u * 32 + 16 * s + 8 * (e >> 2) + 4 * half + (e & 3)];
                f16x8 bh[NTG], bl[NTG];
#pragma unroll
                for (int t = 0; t < NTG; ++t) {
                    const uint4* src = pbuf + (((u * NTG + t) * 2 + s) * 2) * 64 + lane;
                    bh[t] = __builtin_bit_cast(f16x8, src[0]);
                    bl[t] = __builtin_bit_cast(f16x8, src[64]);
                }
#pragma unroll
                for (int i = 0; i < IT; ++i) {
                    const int it = wave + GC_WAVES * i;
                    if (it < NIT) {
                        const int j = it * 32 + l31;
                        f16x8 a1, a0;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const unsigned yy = (j < J && rr[e] >= 0) ? (unsigned)y[rr[e] * J + j] : 254u;
                            a1[e] = (yy == 1u) ? (_Float16)1.0f : (_Float16)0.0f;
                            a0[e] = (yy == 0u) ? (_Float16)1.0f : (_Float16)0.0f;
                        }
#pragma unroll
                        for (int t = 0; t < NTG; ++t) {
                            if (nt0 + t < NT) {
                                c1[i][t] = mfma_f16(a1, bh[t], c1[i][t]);
                                c1[i][t] = mfma_f16(a1, bl[t], c1[i][t]);
                                c0[i][t] = mfma_f16(a0, bh[t], c0[i][t]);
                                c0[i][t] = mfma_f16(a0, bl[t], c0[i][t]);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();                                                          // the next round rewrites the LDS
    }
    // ---- the slab of this chunk: the group's node columns of n1, n0 and mass
    float* slab = slabs + chunk * slab_len;
    const int64_t JG = (int64_t)J * G;
#pragma unroll
    for (int t = 0; t < NTG; ++t) {
        const float m = mass[t] + __shfl_xor(mass[t], 32, 64);                    // the other 16 persons of every unit
        if (half == 0) massb[(wave * NTG + t) * 32 + l31] = m;
    }
    __syncthreads();
    if (tid < NTG * 32) {
        const int g = nt0 * 32 + tid;
        float m = 0.f;
        for (int w = 0; w < GC_WAVES; ++w) m += massb[w * NTG * 32 + tid];
        if (g < G) slab[2 * JG + g] = m;
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int it = wave + GC_WAVES * i;
        if (it < NIT) {
#pragma unroll
            for (int t = 0; t < NTG; ++t) {
                const int g = (nt0 + t) * 32 + l31;
                if (g < G) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = it * 32 + crow32(r, half);
                        if (j < J) {
                            slab[(int64_t)j * G + g] = c1[i][t][r] * GC_PUNSCALE;
                            slab[JG + (int64_t)j * G + g] = c0[i][t][r] * GC_PUNSCALE;
                        }
                    }
                }
            }
        }
    }
}
