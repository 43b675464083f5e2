// Point estimates of the persons: the ML, MAP and Warm's weighted-likelihood (WLE) estimate of theta by Fisher scoring, from a
// caller-given start (the host passes the grid EAP), over the observed cells of a person's own row (y < 2; 254 / 255 add nothing)
// under the item parameters as they stand.  1PL to 4PL, D <= 3.
//
//     z_j = Dc (theta . a_j + b_j)  (b first, then the dimensions, as k_grid_table_irt / k_fit_irt form it; 1PL: a = 1)
//     P_j = c_j + (d_j - c_j) sigmoid(z_j)    Q_j = (1 - d_j) + (d_j - c_j) sigmoid(-z_j)    P_z = (d - c) sigmoid(z) sigmoid(-z)
//     g_d  = Dc   sum_j a_jd (y_j ? Q_j : -P_j) P_z / (P_j Q_j)        the score of the likelihood
//     I_de = Dc^2 sum_j a_jd a_je P_z^2 / (P_j Q_j)                    the expected information
//     J    = Dc^3 sum_j a_j^3 (P_z^2 / (P_j Q_j)) (sigmoid(-z_j) - sigmoid(z_j))     = sum P' P'' / (P Q), D = 1 (Warm 1989)
//
// ml: g, M = I.  map: g - theta, M = I + 1 (the N(0, I) prior of score()).  wle (D = 1): g + J / (2 I), M = I.
// Nothing is formed by cancellation: both sigmoids from e = exp(-|z|) (gf_exp_neg_abs), Q never as 1 - P, the asymptotes as float
// pairs made in double once a workgroup (gf_asymptotes); for 1PL / 2PL the cell's score is y ? sigmoid(-z) : -sigmoid(z), no
// division; for 3PL / 4PL it is y ? P_z / P : -P_z / Q, and the information is the product of the two quotients.
//
// An evaluation at theta gives delta = M^-1 g by Cholesky in registers (3 x 3 at the most; the dimensions a model has not are
// a unit diagonal).  A person stops, at the point of the evaluation -- theta_hat is ALWAYS the last point evaluated, and `info`
// the I of that evaluation --
//     converged (0)  max |delta| <= tol, before the cap; the step is not taken
//     at_bound  (1)  on two consecutive evaluations a coordinate sits on +-bound and delta points outward
//     max_iter  (2)  the max_iter-th evaluation did neither
//     singular  (3)  a pivot of the Cholesky factor (or the step) is not positive and finite
//     empty     (4)  no observed cell: theta_hat = NaN, info = 0, iters = 0
// and otherwise goes to clamp(theta + delta min(1, step_cap / max |delta|), -bound, bound).  iters counts the evaluations.
//
// k_point_irt<MODEL, DD, WLE>: a workgroup takes a contiguous chunk of units of 32 persons (gf_plan: the grid is a function of nb
// alone) and stages the item parameters in LDS once; a WAVE owns persons 8 w .. 8 w + 7 of the unit over ALL item tiles, a lane
// item 64 t + lane of every tile t.  The wave gathers its eight rows once, through `rows`, as eight bytes an item: a lane packs
// and keeps the bytes of its own items in LDS and nobody else reads them -- y is read from memory once a person, and there is
// no barrier anywhere behind the staging of the parameters.  An evaluation: every lane forms the cells of its items for the
// persons still live (a wave-uniform skip), K sums a person in registers (2: g, I; 3 with J for wle; 9 = 3 + 6 for DD = 3), one
// butterfly over the 64 lanes that halves what a lane carries at its first three steps (gf_fold8, then the two lane halves).
// Behind it the eight lanes 4 e .. 4 e + 3, 32 + 4 e .. hold the sums of person e and keep that person's state (theta, status,
// the evaluation count) in registers, all eight alike; the next evaluation fetches the eight thetas by lane reads.  The loop runs
// while the wave's ballot has a live person.  A stopped person's state is written by nobody: later evaluations, run for its
// neighbours, do not touch its bits, and its sums do not depend on who shares the wave.  Every sum has a fixed order; no atomics.
#pragma once
#include "k_grid_fit.hip"

#define GPT_ML 0
#define GPT_MAP 1
#define GPT_WLE 2
#define GPT_CONVERGED 0
#define GPT_AT_BOUND 1
#define GPT_MAX_ITER 2
#define GPT_SINGULAR 3
#define GPT_EMPTY 4
#define GPT_MAX_ITERS 255

// what a cell adds: t = the score of z (y ? Q : -P) P_z / (P Q), it = P_z^2 / (P Q), df = sigmoid(-z) - sigmoid(z)
template <int MODEL>
__device__ __forceinline__ void gpt_cell(float z, const GfAsym& as, bool one, float& t, float& it, float& df) {
    const bool pos = z >= 0.f;
    const float e = gf_exp_neg_abs(z);
    const float r = fast_rcp(1.0f + e);
    const float er = e * r;
    const float sg = pos ? r : er, sn = pos ? er : r;
    df = sn - sg;
    if (MODEL <= 2) {
        t = one ? sn : -sg;
        it = er * r;
    } else {
        const float P = fmaf(as.dmc, sg, as.c) + fmaf(as.dmcl, sg, as.cl), Q = fmaf(as.dmc, sn, as.omd) + fmaf(as.dmcl, sn, as.omdl);
        const float pz = as.dmc * (er * r);
        float u1 = pz * fast_rcp(P), u0 = pz * fast_rcp(Q);
        // P or Q zero or subnormal -- beyond |z| = 87 with c = 0 or 1 - d = 0, see gf_asymptote_cell: P_z / P -> sigmoid(-z) and
        // P_z / Q -> sigmoid(z), not 0 x inf.  A branch of its own that the compiler keeps (as in gf_asymptote_cell): where both
        // are normal floats the line above is what it was.
        if (!(P >= GF_FLT_MIN) || !(Q >= GF_FLT_MIN)) {
            float l1 = sn, l0 = sg;
            asm volatile("" : "+v"(l1), "+v"(l0));
            u1 = P >= GF_FLT_MIN ? u1 : l1;
            u0 = Q >= GF_FLT_MIN ? u0 : l0;
        }
        t = one ? u1 : -u0;
        it = u1 * u0;
    }
}

// gf_fold8 over all 64 lanes: the sum over the wave of value (l31 >> 2), the same bits in the eight lanes that hold it
__device__ __forceinline__ float gpt_fold(float (&v)[8], int l31) {
    const float s = gf_fold8(v, l31);
    return s + __shfl_xor(s, 32);
}

template <int MODEL, int DD, bool WLE>
__global__ __launch_bounds__(256, 2) void k_point_irt(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                      int D, int J, float Dc, const float* __restrict__ theta0,
                                                      const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ c_un, const float* __restrict__ d_un, int map,
                                                      int max_iter, float tol, float bound, float step_cap,
                                                      float* __restrict__ theta_hat, float* __restrict__ info,
                                                      int32_t* __restrict__ status, int32_t* __restrict__ iters, int64_t n_units,
                                                      int64_t units_per_block) {
    constexpr int K = DD == 1 ? (WLE ? 3 : 2) : 9;                 // g[DD], then the triangle of I row by row (, J)
    constexpr int TT = DD * (DD + 1) / 2;
    __shared__ uint2 ysh[4][GP_MAXJ];                               // [wave][item]: the bytes of the wave's eight persons
    __shared__ float ash[MODEL >= 2 ? DD : 1][GP_MAXJ];
    __shared__ float bsh[GP_MAXJ];
    __shared__ GfAsym asym[MODEL >= 3 ? GP_MAXJ : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, mine = l31 >> 2;
    const int JT = (J + 63) >> 6;
    for (int j = tid; j < J; j += 256) {
        bsh[j] = b[j];
        if (MODEL >= 2) {
#pragma unroll
            for (int d = 0; d < DD; ++d) ash[d][j] = d < D ? a[(int64_t)d * J + j] : 0.f;
        }
        if (MODEL >= 3) asym[j] = gf_asymptotes<MODEL>(c_un[j], MODEL == 4 ? d_un[j] : 0.f);
    }
    __syncthreads();                                                // the only barrier: the parameters are read-only from here
    const float Dc2 = Dc * Dc, Dc3 = Dc2 * Dc;
    const int64_t u0 = (int64_t)blockIdx.x * units_per_block;
    const int64_t u1 = u0 + units_per_block < n_units ? u0 + units_per_block : n_units;
    for (int64_t unit = u0; unit < u1; ++unit) {
        const int64_t p0 = unit * 32 + 8 * wave;                    // the wave's persons p0 .. p0 + 7
        if (p0 >= nb) continue;
        // the gather: a lane's items, eight persons' bytes each, and the persons' answered cells
        int64_t rr[8];
        int nob[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t pid = p0 + e;
            rr[e] = pid < nb ? (rows ? rows[pid] : pid) : (int64_t)-1;
            nob[e] = 0;
        }
        for (int jt = 0; jt < JT; ++jt) {
            const int j = jt * 64 + lane;
            const bool have = j < J;
            unsigned lo = 0u, hi = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned yy = (have && rr[e] >= 0) ? (unsigned)y[rr[e] * J + j] : 254u;
                nob[e] += __popcll(__ballot(yy < 2u));
                if (e < 4) lo |= yy << (8 * e); else hi |= yy << (8 * (e - 4));
            }
            if (have) ysh[wave][j] = make_uint2(lo, hi);
        }
        // the state of person `mine`, alike in its eight lanes
        const int64_t pid = p0 + mine;
        int my_n = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) my_n = mine == e ? nob[e] : my_n;
        float th[DD], fin[TT];
#pragma unroll
        for (int d = 0; d < DD; ++d) th[d] = (pid < nb && d < D) ? fminf(fmaxf(theta0[pid * D + d], -bound), bound) : 0.f;
#pragma unroll
        for (int k = 0; k < TT; ++k) fin[k] = 0.f;
        int st = GPT_EMPTY, ni = 0;
        bool live = pid < nb && my_n > 0, out_before = false;
        int it = 0;
        unsigned long long bal = __ballot(live);
        while (bal != 0ull) {
            ++it;
            float the[8][DD];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int d = 0; d < DD; ++d) the[e][d] = __shfl(th[d], 4 * e);
            float acc[K][8];
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
            for (int jt = 0; jt < JT; ++jt) {
                const int j = jt * 64 + lane;
                const bool have = j < J;
                const int js = have ? j : 0;
                const uint2 yb = have ? ysh[wave][js] : make_uint2(0xfefefefeu, 0xfefefefeu);
                const float bj = bsh[js];
                float aj[DD], aa[TT];
#pragma unroll
                for (int d = 0; d < DD; ++d) aj[d] = MODEL >= 2 ? ash[d][js] : 1.0f;
                {
                    int k = 0;
#pragma unroll
                    for (int d = 0; d < DD; ++d)
#pragma unroll
                        for (int f = d; f < DD; ++f) aa[k++] = aj[d] * aj[f];
                }
                const float a3 = aa[0] * aj[0];
                GfAsym asy = {0.25f, 0.f, 0.5f, 0.f, 0.25f, 0.f};
                if (MODEL >= 3) asy = asym[js];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (((bal >> (4 * e)) & 1ull) == 0ull) continue;        // wave-uniform: a stopped person costs nothing
                    const unsigned yy = ((e < 4 ? yb.x : yb.y) >> (8 * (e & 3))) & 255u;
                    const bool ob = yy < 2u, one = yy == 1u;
                    float sz = bj;
                    if (MODEL == 1) {
                        sz = fmaf(the[e][0], 1.f, sz);
                    } else {
#pragma unroll
                        for (int d = 0; d < DD; ++d)
                            if (d < D) sz = fmaf(the[e][d], aj[d], sz);
                    }
                    float t, w, df;
                    gpt_cell<MODEL>(Dc * sz, asy, one, t, w, df);
                    t = ob ? t : 0.f;
                    w = ob ? w : 0.f;
                    if (DD == 1) {
                        acc[0][e] += MODEL == 1 ? t : aj[0] * t;
                        acc[1][e] += MODEL == 1 ? w : aa[0] * w;
                        if (WLE) acc[2][e] += (MODEL == 1 ? w : a3 * w) * df;
                    } else {
#pragma unroll
                        for (int d = 0; d < DD; ++d) acc[d][e] += aj[d] * t;
#pragma unroll
                        for (int k = 0; k < TT; ++k) acc[DD + k][e] += aa[k] * w;
                    }
                }
            }
            float s[K];
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = gpt_fold(acc[k], l31);
            if (live) {
                ni = it;
                float g[DD], M[TT], dl[DD];
#pragma unroll
                for (int d = 0; d < DD; ++d) g[d] = Dc * s[d];
#pragma unroll
                for (int k = 0; k < TT; ++k) fin[k] = M[k] = Dc2 * s[DD + k];
                bool ok;
                if (DD == 1) {
                    if (map) { g[0] -= th[0]; M[0] += 1.0f; }
                    ok = M[0] > 0.f && M[0] < INFINITY;
                    if (WLE) g[0] += (Dc3 * s[2]) / (2.0f * M[0]);  // (wle comes without the prior: M = I)
                    dl[0] = g[0] / M[0];
                } else {
                    // the dimensions the model has not: a unit diagonal, a zero score
                    if (map) {
#pragma unroll
                        for (int d = 0; d < DD; ++d) g[d] -= th[d];
                        M[0] += 1.0f; M[3] += 1.0f; M[5] += 1.0f;
                    }
                    if (D < 2) M[3] = 1.0f;
                    if (D < 3) M[5] = 1.0f;
                    const float q0 = M[0];
                    const float l00 = sqrtf(q0), i00 = 1.0f / l00;
                    const float l10 = M[1] * i00, l20 = M[2] * i00;
                    const float q1 = M[3] - l10 * l10;
                    const float l11 = sqrtf(q1), i11 = 1.0f / l11;
                    const float l21 = (M[4] - l20 * l10) * i11;
                    const float q2 = M[5] - l20 * l20 - l21 * l21;
                    const float l22 = sqrtf(q2), i22 = 1.0f / l22;
                    ok = q0 > 0.f && q0 < INFINITY && q1 > 0.f && q1 < INFINITY && q2 > 0.f && q2 < INFINITY;
                    const float y0 = g[0] * i00;
                    const float y1 = (g[1] - l10 * y0) * i11;
                    const float y2 = (g[2] - l20 * y0 - l21 * y1) * i22;
                    dl[2] = y2 * i22;
                    dl[1] = (y1 - l21 * dl[2]) * i11;
                    dl[0] = (y0 - l10 * dl[1] - l20 * dl[2]) * i00;
                }
                float m = 0.f;
#pragma unroll
                for (int d = 0; d < DD; ++d) m = fmaxf(m, fabsf(dl[d]));
#pragma unroll
                for (int d = 0; d < DD; ++d) ok = ok && dl[d] == dl[d];
                ok = ok && m < INFINITY;
                if (!ok) {
                    st = GPT_SINGULAR;
                    live = false;
                } else if (m <= tol) {
                    st = GPT_CONVERGED;
                    live = false;
                } else {
                    bool outward = false;
#pragma unroll
                    for (int d = 0; d < DD; ++d) outward = outward || (th[d] >= bound && dl[d] > 0.f) || (th[d] <= -bound && dl[d] < 0.f);
                    if (outward && out_before) {
                        st = GPT_AT_BOUND;
                        live = false;
                    } else if (it >= max_iter) {
                        st = GPT_MAX_ITER;
                        live = false;
                    } else {
                        const float sc = m > step_cap ? step_cap / m : 1.0f;
#pragma unroll
                        for (int d = 0; d < DD; ++d)
                            if (d < D) th[d] = fminf(fmaxf(th[d] + dl[d] * sc, -bound), bound);
                        out_before = outward;
                    }
                }
            }
            bal = __ballot(live);
        }
        if ((lane & 35) == 0 && pid < nb) {                         // one of the person's eight lanes writes
            const bool empty = st == GPT_EMPTY;
#pragma unroll
            for (int d = 0; d < DD; ++d)
                if (d < D) theta_hat[pid * D + d] = empty ? NAN : th[d];
            int k = 0;
#pragma unroll
            for (int d = 0; d < DD; ++d)
#pragma unroll
                for (int f = d; f < DD; ++f) {
                    if (f < D) info[(int64_t)(DD == 1 ? 0 : (d * (2 * D - d - 1)) / 2 + f) * nb + pid] = fin[k];
                    ++k;
                }
            status[pid] = st;
            iters[pid] = ni;
        }
    }
}
