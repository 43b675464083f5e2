// Expected counts under a prior of each person's own, a table set a SEGMENT of the persons: k_grid_counts (k_grid_counts.hip) with
// two additions -- the E-step of the item-by-group fit statistics (IrtEngine.dif) and of expected_counts(covariates=).
//
// TILT.  p_i(g) = exp(f[i][g] - logjoint[i]) with f[i][g] = (logw[g] + ll[i][g]) + tilt[i] . coord[g], the f of k_grid_post_cond
// (k_grid_cond.hip), whose output logjoint is the normaliser.  The accumulator of product (1) has the node on the lane and 16
// persons in the lane's registers, so coord[g] is a lane constant (GPC_MAXD registers a node tile, zero past D and past G) and the
// tilt a person constant: [GPC_MAXD][GC_ROUND] floats in LDS beside missb / lkb (zero past D and past the segment's end), read
// four persons at a time where f is formed.  dot = gpc_dot<GPC_MAXD> -- the first product rounded on its own, the rest fused --
// and
//
//     f = (fmaf(acc, GP_UNSCALE, miss) + lw[g]) + dot          p = __expf(f - logjoint)
//
// A zero tilt gives dot = +-0, f the bits of k_grid_counts' f, and -- the split of p, both products, the mass sums and the slab
// sums being k_grid_counts' line by line -- its tables bit for bit where the call has one segment (tests/test_gpu_dif.py holds
// the two kernels to each other).  There is no product next to a sum in what is added here, so nothing for the compiler to
// contract; gpc_dot spells its own roundings out.
//
// SEGMENTS.  The batch positions are cut into n_seg consecutive segments [seg_start[s], seg_start[s + 1]), each with tables of its
// own: n1[s][J][G], n0[s][J][G], mass[s][G].  A workgroup never mixes two segments: a chunk is `rounds_per_chunk` rounds of ONE
// segment, counted from the segment's first person, and a round that reaches the segment's end treats the rest as k_grid_counts
// treats persons past nb (p = 0: logjoint = +inf, a zero tilt, the row marked -1).  The host plans the chunks (gcc_plan,
// gcc_rounds_per_chunk): ONE bound R on the rounds of a chunk for the call -- gc_plan(nb)'s rounds_per_chunk, raised until the
// chunks of all segments fit gc_plan's cap of workgroups -- and segment s gets ceil(rounds_s / R) chunks, none if it is empty,
// among which its rounds are shared evenly: ceil(rounds_s / chunks_s) a chunk, which the kernel works out for itself.  With one
// segment that IS gc_plan (R = ceil(rounds / c) gives n = ceil(rounds / R) chunks of ceil(rounds / n) = R rounds, because n <= c
// and n R >= rounds).  The plan reaches the device as a table of 2 (n_seg + 1) int64 at the head of the
// workspace -- seg_start, then chunk_start, the running sum of the chunks -- written by k_gcc_table from kernel ARGUMENTS (256
// values a launch): no copy, no allocation, nothing that waits.  A workgroup finds its segment by bisection of chunk_start
// (uniform: scalar loads).  Every chunk of the launch exists, so every slab is written; k_reduce_segments adds the slabs of a
// segment in ascending order with the arithmetic of k_reduce_slabs (reduce_slabs_cols), segment = blockIdx.y; a segment without
// chunks gets zeros.  No atomics, every sum in a fixed order: the same call gives the same bits, and a segment's tables do not
// depend on what the other segments hold.
//
// Response bytes as in k_grid_counts: 255 adds VX_LOGP_MISSING to ll and enters neither table, 254 adds nothing anywhere; a person
// with no response adds exp(h - lognorm), their conditioned prior, to the mass of their segment (logjoint = lognorm there).
//
// Resources (hipcc of ROCm 7, -O3, gfx950, `make resources`) are in DESIGN.md section 6 beside k_grid_counts': no scratch, and
// no more than 256 vector registers a lane, so two waves a SIMD as k_grid_counts.
#pragma once
#include "k_util.hip"
#include "k_grid_counts.hip"
#include "k_grid_cond.hip"

#define GCC_MAXSEG 4096                 // segments of a call
#define GCC_TAB_VALUES 256              // int64 values a k_gcc_table launch carries in its arguments (2 KiB)

// The launch for (nb, n_seg, J, G) -- GccPlan, gcc_plan, gcc_chunks, gcc_rounds_per_chunk -- is in grid_plan.h
template <int NTG>
constexpr size_t gcc_lds_bytes() { return gc_lds_bytes<NTG>() + (size_t)GPC_MAXD * GC_ROUND * 4; }

struct GccTabArgs { int64_t v[GCC_TAB_VALUES]; };
__global__ __launch_bounds__(GCC_TAB_VALUES) void k_gcc_table(GccTabArgs a, int n, int64_t* __restrict__ tab) {
    if ((int)threadIdx.x < n) tab[threadIdx.x] = a.v[threadIdx.x];
}

// out[s][i] = sum over the slabs of segment s, ascending, as k_reduce_slabs sums them; tab: [seg_start | chunk_start]
__global__ __launch_bounds__(256) void k_reduce_segments(const float* __restrict__ slabs, const int64_t* __restrict__ tab, int n_seg,
                                                         int64_t stride, int64_t len, float* __restrict__ out) {
    __shared__ float part[4][64];
    const int64_t c0 = tab[n_seg + 1 + blockIdx.y], c1 = tab[n_seg + 2 + blockIdx.y];
    reduce_slabs_cols((int)blockIdx.x, (int)gridDim.x, part, slabs + c0 * stride, c1 - c0, stride, len, 1.0f,
                      out + (int64_t)blockIdx.y * len);
}

// Arguments as k_grid_counts, with coord [G][D], tilt [nb][D] and logjoint [nb] by BATCH POSITION, 1 <= D <= GPC_MAXD, and tab, the
// plan's table.  Grid: (chunks of all segments) x n_groups.  LDS: gcc_lds_bytes<NTG>().
template <int IT, int NTG>
__global__ __launch_bounds__(GC_THREADS) void k_grid_counts_cond(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int J,
                                                                 int G, int D, const uint4* __restrict__ img,
                                                                 const float* __restrict__ logw, const float* __restrict__ coord,
                                                                 const float* __restrict__ tilt, const float* __restrict__ logjoint,
                                                                 const int64_t* __restrict__ tab, int n_seg, int n_groups,
                                                                 float* __restrict__ slabs, int64_t slab_len) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gc_smem[];
    uint4* pbuf = (uint4*)gc_smem;
    int64_t* rowbuf = (int64_t*)(pbuf + GC_WAVES * NTG * 4 * 64);
    float* missb = (float*)(rowbuf + GC_WAVES * 32);
    float* lkb = missb + GC_WAVES * 32;
    float* lw = lkb + GC_WAVES * 32;
    float* massb = lw + NTG * 32;
    float* tiltb = massb + GC_WAVES * NTG * 32;                                   // [GPC_MAXD][GC_ROUND]
    const int KC = gp_kc(J), NT = gp_nt(G), NIT = (J + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int grp = (int)(blockIdx.x % (unsigned)n_groups);
    const int64_t chunk = blockIdx.x / (unsigned)n_groups;                        // over all segments
    const int nt0 = grp * NTG;
    // the segment of this chunk: the last s with chunk_start[s] <= chunk (an empty segment shares its start with the next one)
    const int64_t* cstart = tab + n_seg + 1;
    int slo = 0, shi = n_seg;                                                     // chunk_start[slo] <= chunk < chunk_start[shi]
    while (shi - slo > 1) {
        const int mid = (slo + shi) >> 1;
        if (cstart[mid] <= chunk) slo = mid; else shi = mid;
    }
    const int64_t seg0 = tab[slo], seg1 = tab[slo + 1];                           // its batch positions
    const int64_t lchunk = chunk - cstart[slo];                                   // the chunk within it
    // the segment's rounds shared evenly among its chunks (one segment: gc_plan's rounds_per_chunk, see gcc_plan)
    const int64_t schunks = cstart[slo + 1] - cstart[slo];
    const int64_t rounds_per_chunk = ((seg1 - seg0 + GC_ROUND - 1) / GC_ROUND + schunks - 1) / schunks;
    if (tid < NTG * 32) {
        const int g = nt0 * 32 + tid;
        lw[tid] = (g < G) ? logw[g] : -__builtin_inff();
    }
    float co[NTG][GPC_MAXD];                                                      // the lane's node, one a tile
#pragma unroll
    for (int t = 0; t < NTG; ++t) {
        const int g = (nt0 + t) * 32 + l31;
#pragma unroll
        for (int d = 0; d < GPC_MAXD; ++d) co[t][d] = (g < G && d < D) ? coord[(int64_t)g * D + d] : 0.f;
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
        const int64_t base = seg0 + (lchunk * rounds_per_chunk + rd) * GC_ROUND;  // the round's first person
        if (base >= seg1) break;                                                  // (the same for every wave)
        // ---- (1) this wave's unit: ll of 32 persons at the group's nodes.  Persons past the segment read a valid row and get p = 0.
        {
            const int64_t pid = base + wave * 32 + l31;
            const bool valid = pid < seg1;
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
                lkb[wave * 32 + l31] = valid ? logjoint[pid] : __builtin_inff();  // f - inf = -inf: p = 0
                rowbuf[wave * 32 + l31] = valid ? row : (int64_t)-1;
#pragma unroll
                for (int d = 0; d < GPC_MAXD; ++d) tiltb[d * GC_ROUND + wave * 32 + l31] = (valid && d < D) ? tilt[pid * D + d] : 0.f;
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
                for (int q = 0; q < 4; ++q) {
                    f32x4 t4[GPC_MAXD];                                            // the tilts of four persons, read where they are used
#pragma unroll
                    for (int d = 0; d < GPC_MAXD; ++d) t4[d] = *(const f32x4*)(tiltb + d * GC_ROUND + wave * 32 + 8 * q + 4 * half);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 4 * q + i;
                        const float tl[GPC_MAXD] = {t4[0][i], t4[1][i], t4[2][i]};
                        const float f = (fmaf(acc[t][r], GP_UNSCALE, ms[r]) + lwg) + gpc_dot<GPC_MAXD>(tl, co[t]);
                        pv[r] = (nt0 + t < NT) ? __expf(f - lk[r]) : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mass[t] += pv[r];
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
            if (base + 32 * u >= seg1) break;
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
