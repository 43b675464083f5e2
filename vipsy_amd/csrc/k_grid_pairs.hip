// Local dependence: the pairwise-complete residual sums behind Yen's Q3.  With m_ij = [y_ij < 2] (cells 254 / 255 are not observed),
// r_ij = m_ij (y_ij - P_ij) the residual at the person's point estimate -- the grid EAP for the IRT models, the MAP pattern for
// DINA / DINO -- and I_jk the persons who answered both j and k, four tables float32 [J][J]:
//
//     n[j][k] = |I_jk|      s[j][k] = sum_{I_jk} r_ij      ss[j][k] = sum_{I_jk} r_ij^2      sp[j][k] = sum_{I_jk} r_ij r_ik
//
// (s and ss belong to the ROW item and are not symmetric; n and sp are, bit for bit).  Every one of them is a product over persons
// of two of the three person x item matrices r, r^2 and m: n = m^T m, s = r^T m, ss = (r^2)^T m, sp = r^T r.  On
// v_mfma_f32_32x32x16_f16, r and r^2 as fp16 pairs of the value times 2^10 (|r| < 1: the heads stay below 2^10, the low terms of
// all but vanishing residuals stay normal fp16), m exact, fp32 accumulation:
//
//   cell      k_pair_frag<MODEL> / k_pair_frag_cdm: a workgroup takes units of 32 persons, stages their theta_hat (pattern) and row
//             numbers once in LDS, and its waves share the item tiles: a lane owns item 32 jt + (lane & 31), its parameters in
//             registers, and forms the cells of 16 persons -- two k-steps of eight, person 16 s + 8 (lane >> 5) + e of the unit in
//             element e -- by byte gathers of y through `rows`.  Five fragments a k-step, [unit][item tile][k-step][r head, r low,
//             r^2 head, r^2 low, m][64 lanes] x 16 B.  Persons past nb, items past J and cells >= 254 give exact zeros in all five.
//   products  k_pair_xprod: output-stationary, workgroup = (block of PP_BT x PP_BT item tiles of the upper triangle, chunk of person
//             units), a wave holds one row tile against PP_BC of the block's column tiles -- one tile pair a wave as shipped: six
//             accumulators, two waves a SIMD, which measured faster than two pairs a wave at one wave a SIMD.
//             A fragment serves as A (its items as rows) and as B (as columns) alike.  A tile pair (ta <= tb) takes twelve MFMAs a
//             k-step into six accumulators: sp (hh, hl, lh), n, s and ss of the row tile's items (r^T m, two each) and s and ss of
//             the column tile's items (m^T r: held transposed); a diagonal pair needs only the first four accumulators, eight
//             MFMAs.  Operands come from L2.
//   sums      the chunks' partial tiles are added in ascending order (vx_reduce_slabs), the slabs of a call in person order
//             (k_info_add), no atomics: the same call with the same workspace size gives the same bits.  k_pair_finish takes the
//             scales off (2^-20 for sp, 2^-10 for s and ss) and writes the upper triangle with its mirror (n, sp) or its transpose
//             partner (s, ss).  Persons a slab, chunks a slab and the parts of the workspace are slab_plan's (SlabPlan,
//             grid_plan.h: the one plan vx_grid_info shares), walked by the same grid_slab_loop (vx_abi.hip).
// n is exact while a call scores at most 2^24 persons (fp32 counts).
#pragma once
#include "k_grid_info.hip"

// PP_BT, PP_OPS, PP_ACC, PP_MAX_BLOCKS, PP_UNIT_FLOATS and pp_jt are in grid_plan.h, beside pp_slab_plan
#ifndef PP_BC
#define PP_BC 1                         // column tiles of the block a wave holds against its row tile (PP_BT / PP_BC waves a row)
#endif
#define PP_XWAVES (PP_BT * (PP_BT / PP_BC))
#define PP_MAXD 3
#define PP_SCALE 1024.0f                // 2^10 into the fp16 split of r and r^2 ...
#define PP_UNSCALE 0.0009765625f        // ... and off the sums (exact)

// the five fragments of one k-step from a lane's eight cells: rv = the residuals (0 where not observed), ob = observed
__device__ __forceinline__ void pp_store(uint4* __restrict__ dst, const float (&rv)[8], const bool (&ob)[8]) {
    float qv[8];
    f16x8 mv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        qv[e] = rv[e] * rv[e];
        mv[e] = ob[e] ? (_Float16)1.0f : (_Float16)0.0f;
    }
    f16x8 rh, rl, qh, ql;
    split2h_frag(rv, PP_SCALE, rh, rl);
    split2h_frag(qv, PP_SCALE, qh, ql);
    dst[0] = __builtin_bit_cast(uint4, rh);
    dst[64] = __builtin_bit_cast(uint4, rl);
    dst[128] = __builtin_bit_cast(uint4, qh);
    dst[192] = __builtin_bit_cast(uint4, ql);
    dst[256] = __builtin_bit_cast(uint4, mv);
}

// IRT: P = c + (d - c) sigmoid(Dc z), z as k_grid_table_irt forms it (b first, then the dimensions; 1PL: a = 1), c = sigmoid(c_un),
// d = sigmoid(d_un) (0 and 1 where the model has neither).  y, rows, theta_hat start at the slab's first person; nb = its persons.
template <int MODEL>
__global__ __launch_bounds__(256) void k_pair_frag(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                   int D, int J, float Dc, const float* __restrict__ theta_hat,
                                                   const float* __restrict__ a, const float* __restrict__ b,
                                                   const float* __restrict__ c_un, const float* __restrict__ d_un,
                                                   uint4* __restrict__ F, int64_t n_units) {
    __shared__ float th[32 * PP_MAXD];
    __shared__ int64_t rowbuf[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int JT = pp_jt(J);
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        if (tid < 32) {
            const int64_t pid = unit * 32 + tid;
            const bool valid = pid < nb;
            rowbuf[tid] = valid ? (rows ? rows[pid] : pid) : (int64_t)-1;
#pragma unroll
            for (int d = 0; d < PP_MAXD; ++d) th[tid * PP_MAXD + d] = (valid && d < D) ? theta_hat[pid * D + d] : 0.f;
        }
        __syncthreads();
        for (int jt = wave; jt < JT; jt += 4) {
            const int j = jt * 32 + l31;
            const bool have = j < J;
            const float bj = have ? b[j] : 0.f;
            float aj[PP_MAXD];
#pragma unroll
            for (int d = 0; d < PP_MAXD; ++d) aj[d] = (MODEL >= 2 && have && d < D) ? a[(int64_t)d * J + j] : 0.f;
            const float c = (MODEL >= 3 && have) ? sigmoidf_(c_un[j]) : 0.f;
            const float dd = (MODEL >= 4 && have) ? sigmoidf_(d_un[j]) : 1.0f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float rv[8];
                bool ob[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int p = 16 * s + 8 * half + e;
                    const int64_t rr = rowbuf[p];
                    const unsigned yy = (have && rr >= 0) ? (unsigned)y[rr * J + j] : 254u;
                    float sz = bj;
                    if (MODEL == 1) {
                        sz = fmaf(th[p * PP_MAXD], 1.f, sz);
                    } else {
#pragma unroll
                        for (int d = 0; d < PP_MAXD; ++d)
                            if (d < D) sz = fmaf(th[p * PP_MAXD + d], aj[d], sz);
                    }
                    const float pr = fmaf(dd - c, sigmoidf_(Dc * sz), c);
                    ob[e] = yy < 2u;
                    rv[e] = ob[e] ? (float)yy - pr : 0.f;
                }
                pp_store(F + (((unit * JT + jt) * 2 + s) * PP_OPS) * 64 + lane, rv, ob);
            }
        }
        __syncthreads();                                            // the next unit rewrites the LDS
    }
}

// DINA / DINO: P = eta_j(pattern) ? 1 - s_j : g_j, eta as the tables have it (gp_cdm_eta / gp_cdm_qpat)
__global__ __launch_bounds__(256) void k_pair_frag_cdm(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                       int K, int J, int dino, const float* __restrict__ q,
                                                       const int32_t* __restrict__ pattern, const float* __restrict__ g_un,
                                                       const float* __restrict__ s_un, uint4* __restrict__ F, int64_t n_units) {
    __shared__ int pat[32];
    __shared__ int64_t rowbuf[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int JT = pp_jt(J);
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        if (tid < 32) {
            const int64_t pid = unit * 32 + tid;
            const bool valid = pid < nb;
            rowbuf[tid] = valid ? (rows ? rows[pid] : pid) : (int64_t)-1;
            pat[tid] = valid ? pattern[pid] : 0;
        }
        __syncthreads();
        for (int jt = wave; jt < JT; jt += 4) {
            const int j = jt * 32 + l31;
            const bool have = j < J;
            const int qpat = have ? gp_cdm_qpat(q, K, J, j) : 0;
            const float p0 = have ? sigmoidf_(g_un[j]) : 0.f;       // eta = 0: g
            const float p1 = have ? sigmoidf_(-s_un[j]) : 0.f;      // eta = 1: 1 - s
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float rv[8];
                bool ob[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int p = 16 * s + 8 * half + e;
                    const int64_t rr = rowbuf[p];
                    const unsigned yy = (have && rr >= 0) ? (unsigned)y[rr * J + j] : 254u;
                    const float pr = gp_cdm_eta(dino, qpat, pat[p]) ? p1 : p0;
                    ob[e] = yy < 2u;
                    rv[e] = ob[e] ? (float)yy - pr : 0.f;
                }
                pp_store(F + (((unit * JT + jt) * 2 + s) * PP_OPS) * 64 + lane, rv, ob);
            }
        }
        __syncthreads();
    }
}

// The products of a slab: workgroup = (block of PP_BT x PP_BT item tiles of the upper triangle, chunk of person units); wave w
// holds row tile PP_BT ba + w / (PP_BT / PP_BC) against PP_BC column tiles of the block.  Tile pair (ta <= tb) of chunk c goes to
// slab c at gi_pair_index, its PP_ACC tiles one behind the other, each as the accumulator holds it: [register][lane].
__global__ __launch_bounds__(64 * PP_XWAVES) void k_pair_xprod(const uint4* __restrict__ F, int JT, int nbb, int64_t n_units,
                                                           int64_t units_per_chunk, float* __restrict__ slabs, int64_t slab_len) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_bp = (int64_t)nbb * (nbb + 1) / 2;
    const int64_t chunk = blockIdx.x / n_bp;
    int rem = (int)(blockIdx.x % n_bp), ba = 0;
    while (rem >= nbb - ba) { rem -= nbb - ba; ++ba; }
    const int bb = ba + rem;
    const int ta = ba * PP_BT + wave / (PP_BT / PP_BC), tb0 = bb * PP_BT + (wave % (PP_BT / PP_BC)) * PP_BC;
    if (ta >= JT) return;
    const int64_t u0 = chunk * units_per_chunk;
    const int64_t u1 = u0 + units_per_chunk < n_units ? u0 + units_per_chunk : n_units;
    f32x16 acc[PP_BC][PP_ACC];
#pragma unroll
    for (int i = 0; i < PP_BC; ++i)
#pragma unroll
        for (int t = 0; t < PP_ACC; ++t) acc[i][t] = zero16();
    for (int64_t u = u0; u < u1; ++u) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint4* ap = F + (((u * JT + ta) * 2 + s) * PP_OPS) * 64 + lane;
            const f16x8 arh = __builtin_bit_cast(f16x8, ap[0]), arl = __builtin_bit_cast(f16x8, ap[64]);
            const f16x8 aqh = __builtin_bit_cast(f16x8, ap[128]), aql = __builtin_bit_cast(f16x8, ap[192]);
            const f16x8 am = __builtin_bit_cast(f16x8, ap[256]);
#pragma unroll
            for (int i = 0; i < PP_BC; ++i) {
                const int tb = tb0 + i;
                if (tb < JT && tb >= ta) {
                    const uint4* bp = F + (((u * JT + tb) * 2 + s) * PP_OPS) * 64 + lane;
                    const f16x8 brh = __builtin_bit_cast(f16x8, bp[0]), brl = __builtin_bit_cast(f16x8, bp[64]);
                    const f16x8 bm = __builtin_bit_cast(f16x8, bp[256]);
                    acc[i][0] = mfma_f16(arh, brh, acc[i][0]);
                    acc[i][0] = mfma_f16(arh, brl, acc[i][0]);
                    acc[i][0] = mfma_f16(arl, brh, acc[i][0]);
                    acc[i][1] = mfma_f16(am, bm, acc[i][1]);
                    acc[i][2] = mfma_f16(arh, bm, acc[i][2]);
                    acc[i][2] = mfma_f16(arl, bm, acc[i][2]);
                    acc[i][3] = mfma_f16(aqh, bm, acc[i][3]);
                    acc[i][3] = mfma_f16(aql, bm, acc[i][3]);
                    if (tb != ta) {                                 // (a diagonal pair has these as the transposes of 2 and 3)
                        const f16x8 bqh = __builtin_bit_cast(f16x8, bp[128]), bql = __builtin_bit_cast(f16x8, bp[192]);
                        acc[i][4] = mfma_f16(am, brh, acc[i][4]);
                        acc[i][4] = mfma_f16(am, brl, acc[i][4]);
                        acc[i][5] = mfma_f16(am, bqh, acc[i][5]);
                        acc[i][5] = mfma_f16(am, bql, acc[i][5]);
                    }
                }
            }
        }
    }
    float* slab = slabs + chunk * slab_len;
#pragma unroll
    for (int i = 0; i < PP_BC; ++i) {
        const int tb = tb0 + i;
        if (tb < JT && tb >= ta) {
            float* dst = slab + gi_pair_index(JT, ta, tb) * (PP_ACC * GI_TILE) + lane;
#pragma unroll
            for (int t = 0; t < PP_ACC; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[t * GI_TILE + r * 64] = acc[i][t][r];
        }
    }
}

// element (m, n) of an accumulator tile as k_pair_xprod stores it
__device__ __forceinline__ int pp_elem(int m, int n) { return ((m & 3) + 4 * (m >> 3)) * 64 + n + 32 * ((m >> 2) & 1); }

// tiles -> the four tables [J][J]: the upper triangle and its mirror (n, sp: symmetric bit for bit) or its transpose partner
// (s, ss: the column item's sums over the same persons)
__global__ __launch_bounds__(256) void k_pair_finish(const float* __restrict__ tiles, int J, int JT, float* __restrict__ n,
                                                     float* __restrict__ s, float* __restrict__ ss, float* __restrict__ sp) {
    const int64_t total = (int64_t)J * J;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx / J), k = (int)(idx - (int64_t)j * J);
        if (k < j) continue;
        const int ta = j >> 5, tb = k >> 5, m = j & 31, c = k & 31;
        const float* t = tiles + gi_pair_index(JT, ta, tb) * (PP_ACC * GI_TILE);
        const int e = pp_elem(m, c);
        const int64_t jk = (int64_t)j * J + k, kj = (int64_t)k * J + j;
        const float vsp = t[e] * (PP_UNSCALE * PP_UNSCALE), vn = t[GI_TILE + e];
        sp[jk] = vsp; sp[kj] = vsp;
        n[jk] = vn; n[kj] = vn;
        s[jk] = t[2 * GI_TILE + e] * PP_UNSCALE;
        ss[jk] = t[3 * GI_TILE + e] * PP_UNSCALE;
        if (k != j) {
            const int e2 = (ta == tb) ? pp_elem(c, m) : e;
            const int o = (ta == tb) ? 2 : 4;
            s[kj] = t[o * GI_TILE + e2] * PP_UNSCALE;
            ss[kj] = t[(o + 1) * GI_TILE + e2] * PP_UNSCALE;
        }
    }
}
