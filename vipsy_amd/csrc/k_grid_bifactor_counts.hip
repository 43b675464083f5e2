// Expected counts of a bifactor / testlet model (the Bock-Aitkin E-step behind fit_em_bifactor), in the notation of
// k_grid_bifactor.hip: F_i(g) is what k_grid_bifactor left in fws, loglik_i its output, m_is(g) the bracket of testlet s and
// ll_is(g, h) the testlet's log-likelihood.  Given the general node the posterior of testlet s over (g, h) is a two-dimensional
// table, and every item belongs to one testlet, so the counts of item j live on the Gg x Gh grid of ITS OWN testlet:
//
//     post_i(g)   = exp(F_i(g) - loglik_i)                            the general marginal posterior
//     r_is(g, h)  = exp(logv_h + ll_is(g, h) - m_is(g))               the posterior of u_s given g (sum_h r = 1)
//     p_is(g, h)  = post_i(g) r_is(g, h)
//     n1[j][g][h] = sum_i [y_ij == 1] p_{i,s(j)}(g, h)       n0 likewise with [y_ij == 0]
//     mass[g]     = sum_i post_i(g)                           mass_s[t][g][h] = sum_i p_it(g, h)
//
// An item of the pseudo-testlet has r = v_h: its table is post_i(g) v_h, out of the same code.
//
// Output-stationary: a workgroup of four waves owns (a chunk group: <= GBC_CG chunks of ONE testlet, a pair of general nodes,
// a chunk of persons), and each of its waves walks units of 64 persons.  Two chained products on v_mfma_f32_32x32x16_f16:
//
//   1. GB_TESTLET over ALL chunks of the testlet, then GB_ROWS, the sum of exp(v - mx) and its shuffle -- the very arithmetic that
//      formed F -- so that r = exp(v - mx) / s sums to 1 to rounding, and p = r exp(F - loglik).  The person is on the lane.
//   2. tables[row][h] += A[row][person] p[person][h] for every chunk of the group: the A fragment of a chunk of 16 items carries
//      [y == 1] of its items in rows 0 .. 15 and [y == 0] in rows 16 .. 31, so n1 and n0 of the chunk share one accumulator;
//      per 16 persons that is two MFMAs a chunk and node (p 2^14 as an fp16 head and low term, GC_PSCALE of k_grid_counts.hip).
//      The contraction runs over persons, which product 1 left on the LANE: p goes through a wave-private LDS region
//      (route A), rows = h, a dword = the fp16 pair of persons (l, 32 + l) of the unit -- the two tiles a lane carries, packed by
//      the one v_cvt_pk that splits them -- so that a lane of product 2 reads its B fragment as one 16-byte load.  Slot e of
//      lane half f in k-step s is person 32 (e & 1) + 8 s + 4 f + (e >> 1) of the unit; the A fragment gathers the same eight.
//      (Route B, product 1 transposed, would need the log-sum-exp over h ACROSS 32 lanes: five DPP steps for the maximum and five
//      for the sum a node and 16 persons, against 32 LDS stores and 8 LDS loads a node and 64 persons here.)
//
// The waves' accumulators meet in LDS in wave order; each (chunk group, node pair, person chunk) writes its cells of slab `person
// chunk` -- [n1 | n0: [16 KC slots][Gg][32] | mass_s [n_tl][Gg][32] | mass [Gg]], every cell by exactly one workgroup -- and
// k_grid_bifactor_counts_reduce adds the slabs in ascending order and scatters to the model's item order and the M-step's node
// order g Gh + h, dropping the padded h rows and the padding slots.  No float atomics; every sum in a fixed order: units
// ascending in a wave, waves ascending, slabs ascending.  The cut of the persons depends on (nb, Gg) alone (grid_plan.h), so a
// testlet's tables do not depend on the other testlets of the launch except through F and loglik.
//
// Response bytes: 255 enters neither table (its constant is in F), 254 adds nothing; a person with no response adds their prior
// to mass and mass_s.  Nothing of size persons x (Gg Gh) touches memory: the per-person inputs are y, loglik and fws.
#pragma once
#include "k_grid_bifactor.hip"
#include "k_grid_counts.hip"             // GC_PSCALE / GC_PUNSCALE

static_assert(GB_NG == GBC_NG && GP_WAVES == GBC_WAVES && GP_MT == 2, "grid_plan.h plans k_grid_bifactor_counts for this geometry");
#define GBC_PSTRIDE 36                   // dwords a row of p in LDS: 32 person pairs, padded (16-byte aligned rows)

__global__ __launch_bounds__(GP_THREADS) void k_grid_bifactor_counts(const uint8_t* __restrict__ y, int64_t nb, int KC, int Gg, int Gh,
                                                                     const int32_t* __restrict__ tl_start, int n_tl,
                                                                     const uint4* __restrict__ img, const float* __restrict__ logv,
                                                                     const float* __restrict__ loglik, const float* __restrict__ fws,
                                                                     int64_t units_per_chunk, float* __restrict__ slabs,
                                                                     int64_t slab_len) {
    GB_SHARED;
    __shared__ __attribute__((aligned(16))) uint32_t pbuf[GP_WAVES][2][32 * GBC_PSTRIDE];      // [wave][head, low][h][person pair]
    __shared__ float red[GBC_CG * GB_NG * 16 * 64];
    __shared__ float msb[GP_WAVES][GB_NG][33];                                                 // mass_s over h, then mass
    const int JP = KC * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    for (int i = tid; i <= n_tl; i += GP_THREADS) tls[i] = tl_start[i];
    if (tid < 32) {
        lv[tid] = (tid < Gh) ? logv[tid] : -__builtin_inff();
        uu[tid] = 0.f;
    }
    __syncthreads();
    // the chunk group of this workgroup: testlet tl, chunks c_lo .. c_hi - 1 (the same walk for every thread)
    int tl = 0, q = (int)blockIdx.x;
    for (; tl < n_tl - 1; ++tl) {
        const int ng = (tls[tl + 1] - tls[tl] + GBC_CG - 1) / GBC_CG;
        if (q < ng) break;
        q -= ng;
    }
    const int c_lo = tls[tl] + q * GBC_CG;
    const int c_hi = (c_lo + GBC_CG < tls[tl + 1]) ? c_lo + GBC_CG : tls[tl + 1];
    const bool first = (q == 0);                                                  // the testlet's first group: it owns mass_s[tl]
    const int g0 = (int)blockIdx.y * GB_NG;
    const int64_t chunk = blockIdx.z;
    const int64_t n_units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    const int64_t u_lo = chunk * units_per_chunk;
    const int64_t u_hi = (u_lo + units_per_chunk < n_units) ? u_lo + units_per_chunk : n_units;

    f32x16 cnt[GBC_CG][GB_NG];
    float ms[GB_NG][16], pm[GB_NG];
#pragma unroll
    for (int t = 0; t < GB_NG; ++t) {
        pm[t] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ms[t][r] = 0.f;
#pragma unroll
        for (int ci = 0; ci < GBC_CG; ++ci) cnt[ci][t] = zero16();
    }
    uint32_t* ph = pbuf[wave][0];
    uint32_t* pl = pbuf[wave][1];
    const int want = (l31 < 16) ? 1 : 0;                                          // rows 0 .. 15: [y == 1]; 16 .. 31: [y == 0]
    for (int64_t unit = u_lo + wave; unit < u_hi; unit += GP_WAVES) {
        GP_UNIT_ROWS;
        float ll[GP_MT];
        bool ok[GP_MT];
        int gb_none = 0;
#pragma unroll
        for (int mt = 0; mt < GP_MT; ++mt) {
            GB_UNIT_PERSON(mt);
            ok[mt] = pid[mt] < nb;
            ll[mt] = loglik[ok[mt] ? pid[mt] : 0];
        }
        // the A fragments of the group's chunks, the same for both nodes: slot e of k-step s is person 32 (e & 1) + 8 s + 4 half +
        // (e >> 1) of the unit (a person past the end reads the first row; their p is 0)
        f16x8 af[GBC_CG][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t pk = unit * (32 * GP_MT) + 32 * (e & 1) + 8 * s + 4 * half + (e >> 1);
                const uint8_t* yk = y + ((pk < nb) ? pk : 0) * JP + (l31 & 15);
#pragma unroll
                for (int ci = 0; ci < GBC_CG; ++ci) {
                    const unsigned yy = (c_lo + ci < c_hi) ? (unsigned)yk[(c_lo + ci) * 16] : 254u;
                    af[ci][s][e] = (yy == (unsigned)want) ? (_Float16)1.0f : (_Float16)0.0f;
                }
            }
        }
        f32x16 acc[GP_MT][GB_NG];
        GB_TESTLET(acc, g0, tls[tl], tls[tl + 1])
#pragma unroll
        for (int t = 0; t < GB_NG; ++t) {
            if (g0 + t < Gg) {
                float pv[GP_MT][16];
#pragma unroll
                for (int mt = 0; mt < GP_MT; ++mt) {
                    GB_ROWS(acc[mt][t], v, mx);
                    float e[16], s = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        e[r] = __expf(v[r] - mx);
                        s += e[r];
                    }
                    s += __shfl_xor(s, 32, 64);
                    const float post = ok[mt] ? __expf(fws[(unit * Gg + g0 + t) * 64 + mt * 32 + l31] - ll[mt]) : 0.f;
                    const float pw = post / s;
                    if (half == 0) pm[t] += post;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        pv[mt][r] = e[r] * pw;
                        ms[t][r] += pv[mt][r];
                    }
                }
                // p 2^14 of the persons (l31, 32 + l31) at the lane's 16 rows h, as fp16 pairs into the wave's region
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    uint32_t hh, lo;
                    split2h_pair(pv[0][r] * GC_PSCALE, pv[1][r] * GC_PSCALE, hh, lo);
                    const int h = crow32(r, half);
                    ph[h * GBC_PSTRIDE + l31] = hh;
                    pl[h * GBC_PSTRIDE + l31] = lo;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const f16x8 bh = __builtin_bit_cast(f16x8, *(const uint4*)(ph + l31 * GBC_PSTRIDE + 8 * s + 4 * half));
                    const f16x8 bl = __builtin_bit_cast(f16x8, *(const uint4*)(pl + l31 * GBC_PSTRIDE + 8 * s + 4 * half));
#pragma unroll
                    for (int ci = 0; ci < GBC_CG; ++ci) {
                        if (c_lo + ci < c_hi) {
                            cnt[ci][t] = mfma_f16(af[ci][s], bh, cnt[ci][t]);
                            cnt[ci][t] = mfma_f16(af[ci][s], bl, cnt[ci][t]);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();                                   // the next node rewrites the region
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        (void)gb_none;
    }
    // ---- the waves' accumulators, in wave order
    for (int w = 0; w < GP_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int ci = 0; ci < GBC_CG; ++ci)
#pragma unroll
                for (int t = 0; t < GB_NG; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* d = red + (((ci * GB_NG + t) * 16 + r) * 64 + lane);
                        *d = (w == 0) ? cnt[ci][t][r] : *d + cnt[ci][t][r];
                    }
        }
        __syncthreads();
    }
    // mass_s and mass of this wave: the 32 persons of a half-wave, by a fixed tree
#pragma unroll
    for (int t = 0; t < GB_NG; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = ms[t][r];
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
            if (l31 == 0) msb[wave][t][crow32(r, half)] = x;
        }
        float x = pm[t];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) msb[wave][t][32] = x;
    }
    __syncthreads();
    float* slab = slabs + chunk * slab_len;
    const int64_t off_ms = (int64_t)2 * JP * Gg * 32, off_mass = off_ms + (int64_t)n_tl * Gg * 32;
    if (tid < GB_NG * 33) {
        const int t = tid / 33, k = tid - t * 33, g = g0 + t;
        float x = 0.f;
        for (int w = 0; w < GP_WAVES; ++w) x += msb[w][t][k];
        if (g < Gg) {
            if (k < 32) {
                if (first) slab[off_ms + ((int64_t)tl * Gg + g) * 32 + k] = x;
            } else if (first && tl == 0) {
                slab[off_mass + g] = x;
            }
        }
    }
    for (int pi = wave; pi < GBC_CG * GB_NG; pi += GP_WAVES) {
        const int ci = pi / GB_NG, t = pi - ci * GB_NG, g = g0 + t;
        if (c_lo + ci < c_hi && g < Gg) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow32(r, half);
                const int64_t slot = (int64_t)(row >> 4) * JP + (c_lo + ci) * 16 + (row & 15);
                slab[(slot * Gg + g) * 32 + l31] = red[(pi * 16 + r) * 64 + lane] * GC_PUNSCALE;
            }
        }
    }
}

// out = (accumulate ? out : 0) + the slabs in ascending order, scattered: slot jp of the layout to item col[jp] (a padding slot
// or an item outside 0 .. J - 1: nowhere), node (g, h) to g Gh + h (h >= Gh: nowhere).  mass_s may be NULL.
__global__ __launch_bounds__(256) void k_grid_bifactor_counts_reduce(const float* __restrict__ slabs, int64_t n_slabs, int64_t slab_len,
                                                                     int KC, int Gg, int Gh, int n_tl, const int32_t* __restrict__ col,
                                                                     int J, int accumulate, float* __restrict__ n1,
                                                                     float* __restrict__ n0, float* __restrict__ mass,
                                                                     float* __restrict__ mass_s) {
    const int64_t half_len = (int64_t)KC * 16 * Gg * 32, off_ms = 2 * half_len, off_mass = off_ms + (int64_t)n_tl * Gg * 32;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slab_len; i += (int64_t)gridDim.x * 256) {
        float* out;
        const int h = (int)(i & 31);
        if (i < off_ms) {
            const int which = i >= half_len;
            const int64_t rem = (i - which * half_len) >> 5;
            const int g = (int)(rem % Gg), j = col[rem / Gg];
            if (h >= Gh || j < 0 || j >= J) continue;
            out = (which ? n0 : n1) + ((int64_t)j * Gg + g) * Gh + h;
        } else if (i < off_mass) {
            if (h >= Gh || !mass_s) continue;
            out = mass_s + ((i - off_ms) >> 5) * Gh + h;
        } else {
            out = mass + (i - off_mass);
        }
        float s = 0.f;
        for (int64_t k = 0; k < n_slabs; ++k) s += slabs[k * slab_len + i];
        *out = accumulate ? *out + s : s;
    }
}
