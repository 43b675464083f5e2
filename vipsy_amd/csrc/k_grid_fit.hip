// Person fit and residual mean squares: the sums behind lz (Drasgow-Levine-Williams) and infit / outfit, per person and per item.
// Observed cells only (y < 2; 254 / 255 add nothing).  With P the model probability AT THE PERSON'S POINT ESTIMATE -- the grid EAP
// for the IRT models, the MAP pattern for DINA / DINO -- under the item parameters as they stand, Q = 1 - P and, per cell,
//
//     lambda = log(P / Q)    l = y ? log P : log Q    eps = P log P + Q log Q    nu = P Q lambda^2
//     r2 = y ? Q^2 : P^2     w = P Q                  zeta = r2 / w = y ? Q / P : P / Q
//
// person[7][nb]: n (answered items), l0 = sum l, e = sum eps, v = sum nu, sr2 = sum r2, sw = sum w, sz2 = sum zeta over the items
// the person answered; item[4][J]: n, sr2, sw, sz2 over the persons who answered the item.  lz = (l0 - e) / sqrt(v),
// outfit = sz2 / n, infit = sr2 / sw in float64 on the host (vipsy_amd.grid.person_fit_host / item_msq_host).
//
// Nothing here is formed by cancellation: Q never as 1 - P, r2 never from y - P.
//   1PL / 2PL   z = Dc (theta_hat . a + b), e = exp(-|z|), t = 1 + e: P and Q are 1 / t and e / t, lambda = z exactly,
//               log P = min(z, 0) - log1p(e), log Q = min(-z, 0) - log1p(e), log1p(e) = log(t) + (e - (t - 1)) / t (the second term
//               gives back what the rounding of t took), Q / P = exp(-z) = e or 1 / e.
//   3PL / 4PL   P = c + (d - c) sigmoid(z), Q = sigmoid(-d_un) + (d - c) sigmoid(-z) (3PL: d - c = sigmoid(-c_un)), the logs of both,
//               lambda their difference, zeta the quotient.  c, d - c and sigmoid(-d_un) are float pairs made in double once a
//               workgroup (LDS): a float's rounding of them would be the same in every cell of the item and add up in its sums.
//   DINA / DINO a cell is the 1PL cell at z = g_un (eta = 0) or z = -s_un (eta = 1): both sets of terms once per item tile, outside
//               the person loop, in double for the same reason.
// exp(-|z|) takes the product z log2(e) in two floats: the hardware exp2 alone would carry |z| / 2 ulp of the argument's rounding.
//
// k_fit_irt<MODEL> / k_fit_cdm: siblings of k_pair_frag.  A workgroup takes a contiguous chunk of units of 32 persons and stages a
// unit's row numbers and theta_hat (pattern) in LDS; its waves share the item tiles, a lane owns item 32 jt + (lane & 31) with
// the item's parameters in registers and forms the cells of the unit's persons 16 s + 8 (lane >> 5) + e, one s after the other,
// by byte gathers of y through `rows`.  Persons past nb, items past J and cells >= 254 add exact zeros.
//   person sums  7 x 8 accumulators a lane over the wave's item tiles; per unit and s one butterfly over the 32 item lanes that
//                halves the values a lane carries at each of its first three steps (9 shuffles a sum, not 40), then the four
//                waves through LDS in ascending order.
//   item sums    an LDS array [lane half][4][item] that only the owning lane touches, persons in ascending order; at the end the
//                two halves are added, low half first, into the workgroup's partial [4][J] of the workspace; the partials are
//                added in ascending order, in double, and rounded once (k_fit_items).  No atomics.
// The grid is a function of nb alone (gf_plan): the same call gives the same bits on every device.
// n is exact while a call scores at most 2^24 persons (fp32 counts).
#pragma once
#include "k_grid_pairs.hip"

// the launch of a call -- GfPlan, gf_plan, gf_ws_floats -- is in grid_plan.h, with GF_MAX_BLOCKS and GF_ITEM (n, sr2, sw, sz2)
#define GF_MAXD PP_MAXD
#define GF_PERSON 7                     // n, l0, e, v, sr2, sw, sz2

// what a cell adds, for either answer: everything but l, r2 and zeta is the same for both
struct GfTerms {
    float l1, l0;                       // log P, log Q
    float eps, nu, w;
    float r1, r0;                       // Q^2, P^2
    float z1, z0;                       // Q / P, P / Q
};

// exp(-|z|): z log2(e) as head + tail, exp2 of the head, the tail as a first-order factor
__device__ __forceinline__ float gf_exp_neg_abs(float z) {
    const float x = -fabsf(z);
    const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-08f;
    const float h = x * L2E_HI;
    const float l = fmaf(x, L2E_LO, fmaf(x, L2E_HI, -h));
    const float p = __builtin_amdgcn_exp2f(h);
    return fmaf(p, l * 0.6931471805599453f, p);
}

// the logistic cell at z: P = sigmoid(z), lambda = z
__device__ __forceinline__ GfTerms gf_logistic(float z) {
    GfTerms t;
    const bool pos = z >= 0.f;
    const float e = gf_exp_neg_abs(z);
    const float u = 1.0f + e;
    const float r = fast_rcp(u);                                    // the larger of P and Q
    const float er = e * r;                                         // the smaller
    const float l1p = fmaf(e - (u - 1.0f), r, fast_log(u));         // log1p(e)
    const float ie = fast_rcp(e);
    const float P = pos ? r : er, Q = pos ? er : r;
    t.l1 = fminf(z, 0.f) - l1p;
    t.l0 = fminf(-z, 0.f) - l1p;
    t.eps = fmaf(P, t.l1, Q * t.l0);
    t.w = er * r;
    t.nu = t.w * (z * z);
    t.r1 = Q * Q;
    t.r0 = P * P;
    t.z1 = pos ? e : ie;
    t.z0 = pos ? ie : e;
    return t;
}

struct GfCell {
    float l, eps, nu, r2, w, z2;
};
__device__ __forceinline__ GfCell gf_pick(const GfTerms& t, bool one) {
    GfCell c;
    c.l = one ? t.l1 : t.l0;
    c.eps = t.eps;
    c.nu = t.nu;
    c.r2 = one ? t.r1 : t.r0;
    c.w = t.w;
    c.z2 = one ? t.z1 : t.z0;
    return c;
}

// The logistic cell once more, in double and rounded at the end: DINA / DINO take it once per item tile, and whatever error its
// terms carry is the same for every person of the item -- it would add up, not average out, in the item sums.
__device__ __forceinline__ GfTerms gf_logistic_item(float zf) {
    GfTerms t;
    const double z = (double)zf;
    const bool pos = zf >= 0.f;
    const double e = exp(-fabs(z));
    const double r = 1.0 / (1.0 + e), er = e * r, l1p = log1p(e);
    const double P = pos ? r : er, Q = pos ? er : r;
    const double l1 = fmin(z, 0.0) - l1p, l0 = fmin(-z, 0.0) - l1p;
    t.l1 = (float)l1;
    t.l0 = (float)l0;
    t.eps = (float)(P * l1 + Q * l0);
    t.w = (float)(P * Q);
    t.nu = (float)(P * Q * z * z);
    t.r1 = (float)(Q * Q);
    t.r0 = (float)(P * P);
    t.z1 = (float)exp(-z);
    t.z0 = (float)exp(z);
    return t;
}

// The asymptotes of a 3PL / 4PL item as float pairs (head, tail), from double: c = sigmoid(c_un), omd = 1 - d = sigmoid(-d_un)
// (3PL: 0) and dmc = d - c (3PL: sigmoid(-c_un)).  In float alone each would carry its rounding into every cell of the item alike.
struct GfAsym {
    float c, cl, dmc, dmcl, omd, omdl;
};
__device__ __forceinline__ void gf_pair(double v, float& hi, float& lo) {
    hi = (float)v;
    lo = (float)(v - (double)hi);
}
template <int MODEL>
__device__ __forceinline__ GfAsym gf_asymptotes(float c_un, float d_un) {
    GfAsym a;
    const double c = 1.0 / (1.0 + exp(-(double)c_un));
    const double omd = MODEL == 4 ? 1.0 / (1.0 + exp((double)d_un)) : 0.0;
    const double dmc = MODEL == 4 ? 1.0 / (1.0 + exp(-(double)d_un)) - c : 1.0 / (1.0 + exp((double)c_un));
    gf_pair(c, a.c, a.cl);
    gf_pair(omd, a.omd, a.omdl);
    gf_pair(dmc, a.dmc, a.dmcl);
    return a;
}

#define GF_FLT_MIN 1.17549435e-38f        // the smallest normal float
// the 3PL / 4PL cell: P = c + (d - c) sigmoid(z) and Q = (1 - d) + (d - c) sigmoid(-z), each from positive terms
__device__ __forceinline__ GfCell gf_asymptote_cell(float z, const GfAsym& a, bool one) {
    const bool pos = z >= 0.f;
    const float e = gf_exp_neg_abs(z);
    const float r = fast_rcp(1.0f + e);
    const float er = e * r;
    const float sg = pos ? r : er, sn = pos ? er : r;
    const float P = fmaf(a.dmc, sg, a.c) + fmaf(a.dmcl, sg, a.cl), Q = fmaf(a.dmc, sn, a.omd) + fmaf(a.dmcl, sn, a.omdl);
    // lambda = log P - log Q as one fma over log2 P: what the compiler's contraction made of `lp - lq` before the branch below
    // was there, written out so that it does not depend on where the subtraction ends up
    const float l2p = __builtin_amdgcn_logf(P);
    const float lp = 0.6931471805599453f * l2p, lq = fast_log(Q);
    const float lam = fmaf(l2p, 0.6931471805599453f, -lq);
    GfCell o;
    o.l = one ? lp : lq;
    o.eps = fmaf(P, lp, Q * lq);
    o.w = P * Q;
    o.nu = o.w * (lam * lam);
    // Beyond |z| = 87 sigmoid(-|z|) is no normal float: with c = 0 (z < 0) or 1 - d = 0 (z > 0; every 3PL item) P or Q is zero or
    // subnormal, the hardware log2 and rcp answer -inf and +inf, and P log P, w lambda^2 above are 0 x inf.  The logarithm takes
    // its limit log(d - c) - |z| there: P log P -> 0, lambda and nu stay finite, and the odds of an answer on the vanished side
    // come back as +inf below.  A branch of its own, which the compiler has to keep (the empty asm is not speculated): where P
    // and Q are normal floats the results are what they were.
    if (!(P >= GF_FLT_MIN) || !(Q >= GF_FLT_MIN)) {
        float lim = fast_log(a.dmc) - fabsf(z);
        asm volatile("" : "+v"(lim));
        const float lp2 = P >= GF_FLT_MIN ? lp : lim, lq2 = Q >= GF_FLT_MIN ? lq : lim;
        const float lam2 = lp2 - lq2;
        o.l = one ? lp2 : lq2;
        o.eps = fmaf(P, lp2, Q * lq2);
        o.nu = o.w * (lam2 * lam2);
    }
    const float num = one ? Q : P, den = one ? P : Q;
    o.r2 = num * num;
    o.z2 = num * fast_rcp(den);
    return o;
}

// One butterfly over the 32 item lanes of a lane half: 8 values a lane in, the sum over the lanes of value (l31 >> 2) out (the four
// lanes of a quad hold the same).  At each of the first three steps a lane keeps the half of its values its partner does not and
// hands over the other.
__device__ __forceinline__ float gf_fold8(float (&v)[8], int l31) {
    const bool b4 = (l31 & 16) != 0, b3 = (l31 & 8) != 0, b2 = (l31 & 4) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float keep = b4 ? v[i + 4] : v[i], send = b4 ? v[i] : v[i + 4];
        v[i] = keep + __shfl_xor(send, 16);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b3 ? v[i + 2] : v[i], send = b3 ? v[i] : v[i + 2];
        v[i] = keep + __shfl_xor(send, 8);
    }
    const float keep = b2 ? v[1] : v[0], send = b2 ? v[0] : v[1];
    float s = keep + __shfl_xor(send, 4);
    s += __shfl_xor(s, 2);
    return s + __shfl_xor(s, 1);
}

// LDS of both kernels: the unit's rows, the waves' person sums, the item sums of the workgroup
struct GfShared {
    int64_t rowbuf[32];
    float psum[4][GF_PERSON][32];
    float isum[2][GF_ITEM][GP_MAXJ];
};

__device__ __forceinline__ void gf_clear_items(GfShared& sh, int JT) {
    for (int i = threadIdx.x; i < 2 * GF_ITEM * GP_MAXJ; i += 256)
        if ((i & (GP_MAXJ - 1)) < JT * 32) (&sh.isum[0][0][0])[i] = 0.f;
}

// a lane's cell: into the person accumulators of its slot and the item accumulators of the tile
#define GF_ADD(i, ob, cell)                                                                         \
    do {                                                                                            \
        const float m_ = (ob) ? 1.0f : 0.f;                                                         \
        const float r2_ = (ob) ? (cell).r2 : 0.f, w_ = (ob) ? (cell).w : 0.f, z2_ = (ob) ? (cell).z2 : 0.f; \
        acc[0][i] += m_;                                                                            \
        acc[1][i] += (ob) ? (cell).l : 0.f;                                                         \
        acc[2][i] += (ob) ? (cell).eps : 0.f;                                                       \
        acc[3][i] += (ob) ? (cell).nu : 0.f;                                                        \
        acc[4][i] += r2_;                                                                           \
        acc[5][i] += w_;                                                                            \
        acc[6][i] += z2_;                                                                           \
        it[0] += m_; it[1] += r2_; it[2] += w_; it[3] += z2_;                                       \
    } while (0)

// the end of an s: the butterfly; the wave's sums of persons 16 s + 8 half + 0 .. 7 into LDS
__device__ __forceinline__ void gf_fold_out(GfShared& sh, float (&acc)[GF_PERSON][8], int s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int k = 0; k < GF_PERSON; ++k) {
        const float t = gf_fold8(acc[k], l31);
        if ((l31 & 3) == 0) sh.psum[wave][k][16 * s + 8 * half + (l31 >> 2)] = t;
    }
}

// the end of a unit: the four waves in ascending order, the unit's seven rows of `person`
__device__ __forceinline__ void gf_unit_out(GfShared& sh, int64_t unit, int64_t nb, float* __restrict__ person) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < GF_PERSON * 32) {
        const int k = tid >> 5, q = tid & 31;
        const int64_t pid = unit * 32 + q;
        const float s = ((sh.psum[0][k][q] + sh.psum[1][k][q]) + sh.psum[2][k][q]) + sh.psum[3][k][q];
        if (pid < nb) person[(int64_t)k * nb + pid] = s;
    }
    __syncthreads();                                                // the next unit rewrites the LDS
}

// the end of a workgroup: the two lane halves of every item sum, low half first, into the workgroup's partial [4][J]
__device__ __forceinline__ void gf_items_out(const GfShared& sh, int J, float* __restrict__ part) {
    float* dst = part + (int64_t)blockIdx.x * GF_ITEM * J;
    for (int i = threadIdx.x; i < GF_ITEM * J; i += 256) {
        const int k = i / J, j = i - k * J;
        dst[i] = sh.isum[0][k][j] + sh.isum[1][k][j];
    }
}

// item[k][j] = the workgroups' partials added in ascending order, in double, rounded once: a float chain over a thousand partials
// would leave its own rounding in the sum.  i runs over [4][J].
__global__ __launch_bounds__(256) void k_fit_items(const float* __restrict__ part, int64_t n_blocks, int len, float* __restrict__ item) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double s = 0.0;
#pragma unroll 8
    for (int64_t b = 0; b < n_blocks; ++b) s += (double)part[b * len + i];
    item[i] = (float)s;
}

// IRT: z as k_grid_table_irt forms it (b first, then the dimensions; 1PL: a = 1)
template <int MODEL>
__global__ __launch_bounds__(256, 2) void k_fit_irt(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                    int D, int J, float Dc, const float* __restrict__ theta_hat,
                                                    const float* __restrict__ a, const float* __restrict__ b,
                                                    const float* __restrict__ c_un, const float* __restrict__ d_un,
                                                    float* __restrict__ person, float* __restrict__ part, int64_t n_units,
                                                    int64_t units_per_block) {
    __shared__ GfShared sh;
    __shared__ float th[32 * GF_MAXD];
    __shared__ GfAsym asym[MODEL >= 3 ? GP_MAXJ : 1];               // once a workgroup: the double arithmetic is not per unit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int JT = pp_jt(J);
    gf_clear_items(sh, JT);
    if (MODEL >= 3)
        for (int j = tid; j < J; j += 256) asym[j] = gf_asymptotes<MODEL>(c_un[j], MODEL == 4 ? d_un[j] : 0.f);
    const int64_t u0 = (int64_t)blockIdx.x * units_per_block;
    const int64_t u1 = u0 + units_per_block < n_units ? u0 + units_per_block : n_units;
    for (int64_t unit = u0; unit < u1; ++unit) {
        if (tid < 32) {
            const int64_t pid = unit * 32 + tid;
            const bool valid = pid < nb;
            sh.rowbuf[tid] = valid ? (rows ? rows[pid] : pid) : (int64_t)-1;
#pragma unroll
            for (int d = 0; d < GF_MAXD; ++d) th[tid * GF_MAXD + d] = (valid && d < D) ? theta_hat[pid * D + d] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            float acc[GF_PERSON][8];
#pragma unroll
            for (int k = 0; k < GF_PERSON; ++k)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[k][i] = 0.f;
            for (int jt = wave; jt < JT; jt += 4) {
                const int j = jt * 32 + l31;
                const bool have = j < J;
                const float bj = have ? b[j] : 0.f;
                float aj[GF_MAXD];
#pragma unroll
                for (int d = 0; d < GF_MAXD; ++d) aj[d] = (MODEL >= 2 && have && d < D) ? a[(int64_t)d * J + j] : 0.f;
                GfAsym asy = {0.25f, 0.f, 0.5f, 0.f, 0.25f, 0.f};
                if (MODEL >= 3 && have) asy = asym[j];
                float it[GF_ITEM] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int p = 16 * s + 8 * half + e;
                    const int64_t rr = sh.rowbuf[p];
                    const unsigned yy = (have && rr >= 0) ? (unsigned)y[rr * J + j] : 254u;
                    float sz = bj;
                    if (MODEL == 1) {
                        sz = fmaf(th[p * GF_MAXD], 1.f, sz);
                    } else {
#pragma unroll
                        for (int d = 0; d < GF_MAXD; ++d)
                            if (d < D) sz = fmaf(th[p * GF_MAXD + d], aj[d], sz);
                    }
                    const float z = Dc * sz;
                    const bool ob = yy < 2u, one = yy == 1u;
                    const GfCell cell = (MODEL <= 2) ? gf_pick(gf_logistic(z), one) : gf_asymptote_cell(z, asy, one);
                    GF_ADD(e, ob, cell);
                }
                if (have) {
#pragma unroll
                    for (int k = 0; k < GF_ITEM; ++k) sh.isum[half][k][j] += it[k];
                }
            }
            gf_fold_out(sh, acc, s);
        }
        gf_unit_out(sh, unit, nb, person);
    }
    __syncthreads();
    gf_items_out(sh, J, part);
}

// DINA / DINO: eta as the tables have it (gp_cdm_eta / gp_cdm_qpat); the cell is the logistic cell at g_un or at -s_un
__global__ __launch_bounds__(256, 2) void k_fit_cdm(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                    int K, int J, int dino, const float* __restrict__ q,
                                                    const int32_t* __restrict__ pattern, const float* __restrict__ g_un,
                                                    const float* __restrict__ s_un, float* __restrict__ person,
                                                    float* __restrict__ part, int64_t n_units, int64_t units_per_block) {
    __shared__ GfShared sh;
    __shared__ int pat[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int JT = pp_jt(J);
    gf_clear_items(sh, JT);
    const int64_t u0 = (int64_t)blockIdx.x * units_per_block;
    const int64_t u1 = u0 + units_per_block < n_units ? u0 + units_per_block : n_units;
    for (int64_t unit = u0; unit < u1; ++unit) {
        if (tid < 32) {
            const int64_t pid = unit * 32 + tid;
            const bool valid = pid < nb;
            sh.rowbuf[tid] = valid ? (rows ? rows[pid] : pid) : (int64_t)-1;
            pat[tid] = valid ? pattern[pid] : 0;
        }
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            float acc[GF_PERSON][8];
#pragma unroll
            for (int k = 0; k < GF_PERSON; ++k)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[k][i] = 0.f;
            for (int jt = wave; jt < JT; jt += 4) {
                const int j = jt * 32 + l31;
                const bool have = j < J;
                const int qpat = have ? gp_cdm_qpat(q, K, J, j) : 0;
                const GfTerms t0 = gf_logistic_item(have ? g_un[j] : 0.f);      // eta = 0: P = g
                const GfTerms t1 = gf_logistic_item(have ? -s_un[j] : 0.f);     // eta = 1: P = 1 - s
                float it[GF_ITEM] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int p = 16 * s + 8 * half + e;
                    const int64_t rr = sh.rowbuf[p];
                    const unsigned yy = (have && rr >= 0) ? (unsigned)y[rr * J + j] : 254u;
                    const bool ob = yy < 2u, one = yy == 1u;
                    const GfCell cell = gp_cdm_eta(dino, qpat, pat[p]) ? gf_pick(t1, one) : gf_pick(t0, one);
                    GF_ADD(e, ob, cell);
                }
                if (have) {
#pragma unroll
                    for (int k = 0; k < GF_ITEM; ++k) sh.isum[half][k][j] += it[k];
                }
            }
            gf_fold_out(sh, acc, s);
        }
        gf_unit_out(sh, unit, nb, person);
    }
    __syncthreads();
    gf_items_out(sh, J, part);
}
