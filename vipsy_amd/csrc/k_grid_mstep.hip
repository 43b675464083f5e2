// The M-step of the Bock-Aitkin EM on the expected-count tables of k_grid_counts.hip: given n1[j][g], n0[j][g] (the posterior mass
// at node g of the persons who answered item j correctly / wrongly) every item is a small weighted logistic regression of its
// own -- or, for DINA / DINO, two ratios of sums.  2 J G floats are read once; nothing here is large.
//
// IRT (k_grid_mstep_irt): item j maximises
//
//     Q_j(a_j, b_j) = sum_g n1[j][g] log P_j(g) + n0[j][g] log(1 - P_j(g)),      z = Dc (theta_g . a_j + b_j)
//
// with the clamp of the tables' cell (irt_cell<2>: z clamped to +-logit(1 - eps32); a node where the clamp is active adds its
// clamped term to Q and nothing to the gradient or the curvature) in a cell of its own, gm_cell, which keeps the digits of log P
// and 1 - P where P is near 1.  Newton steps, which for the logistic link are Fisher
// scoring: with u_g = (1, theta_g), r = n1 (1 - p) - n0 p and w = (n1 + n0) p (1 - p),
//
//     gradient = Dc sum_g r u_g        -Hessian = Dc^2 sum_g w u_g u_g^T        (positive semi-definite always).
//
// Mapping: ONE WAVE AN ITEM, four items a workgroup.  An item's row of each table is at most 1 024 floats = 16 a lane, read once
// (coalesced: lane l holds nodes l, l + 64, ...) and kept in registers over all Newton steps of the launch; theta [G][D] is
// staged once a workgroup in LDS (<= 12 KB) and shared by its four items.  One evaluation gives Q, the D + 1 gradient terms and
// the (D + 1)(D + 2) / 2 curvature terms: each lane adds its nodes in ascending order, the lanes meet in the DPP tree of
// wave_sum_dpp -- a fixed order, no atomics, no LDS traffic, no barrier after the staging: the same call gives the same bits.
// A workgroup an item would put the cross-wave step (LDS + barrier) into every one of up to 64 x 9 evaluations for rows that
// fill a quarter of one wave's registers; a lane an item would read the tables with a stride of G floats.
//
// The system of at most 4 x 4 is solved by Cholesky in registers, redundantly in every lane (its inputs are wave-uniform).
// A loading with a_free = 0 is a unit row of the system with a zero right-hand side -- exact: it changes no other entry of the
// factor -- and is never written.  Step control: a step is accepted when Q does not fall by more than 1e-6 |Q| (the float32
// rounding of a sum of at most 1 024 terms), else halved, at most 8 times, else the item stops where it is.  A step whose
// largest component exceeds GM_STEP_CAP = 4 is scaled down to that length: an item whose observed answers are all equal has its
// maximum at infinity, and on the way there the system loses rank as node after node reaches the clamp -- the last solvable
// system can ask for a step of any size.  With the cap such an item moves at most 4 a step until every node is clamped, the
// curvature is exactly zero, the pivot test fails and the item stops: finite, at most 4 x newton from where it started.
// An item nobody answered (sum n = 0), a non-positive or non-finite pivot: the values keep their bits.
//
// DINA / DINO (k_grid_mstep_cdm): closed form.  With eta as k_grid_table_cdm has it (gp_cdm_eta), R0 / W0 = sum over the
// patterns with eta = 0 of n1 / n0, R1 / W1 the same over eta = 1:
//     g_un = log R0 - log W0        s_un = log W1 - log R1        (logits from positive sums, no 1 - x), clamped to +-logit(1 - eps32).
// A class without mass (R + W = 0; for DINO every single-attribute item's eta = 1 class) leaves its parameter untouched.
#pragma once
#include "vx_common.h"
#include "k_grid_post.hip"

#define GM_THREADS 256
#define GM_WAVES (GM_THREADS / 64)       // items a workgroup
#define GM_NK (GP_MAXG / 64)             // nodes a lane holds at most
#define GM_MAXD 3
#define GM_NP (GM_MAXD + 1)              // unknowns of an item: b, a_0 .. a_{D-1}
#define GM_MAX_NEWTON 64
#define GM_HALVINGS 8
#define GM_STEP_CAP 4.0f
#define GM_QTOL 1e-6f
#define GM_ZL 15.942384719848633f        // logit(1 - eps32), the clamp of irt_cell<2>

// Q, the gradient and the curvature of one item at the unknowns p = (b, a_0, a_1, a_2); h holds the upper triangle row by row
struct GmSums {
    float q;
    float g[GM_NP];
    float h[GM_NP * (GM_NP + 1) / 2];
};

// One node: log P, log(1 - P) at z clamped to +-GM_ZL, and 1 - P, P (0 where the clamp is active), every one from positive terms.
// irt_cell<2> has log P = y z - softplus(z) and 1 - P = 1 - sigmoid(z): at z = 10 differences of numbers near 10 and near 1 that
// leave 5e-5 -- good for a likelihood, but Q of an item nearly everybody answers alike is then rounded at 1e-4 of its size, a
// hundred times what the acceptance rule allows for: near the maximiser every trial looked like a fall and the item stopped on
// its halvings up to 1.5e-2 short.  Here log P = min(z, 0) - log1p(e), log(1 - P) = min(-z, 0) - log1p(e) with e = exp(-|z|), and
// log1p(e) = log(t) e / (t - 1) for t = 1 + e rounded: t - 1 is exact, and the quotient takes back what the rounding of t took.
__device__ __forceinline__ void gm_cell(float z, float& lp1, float& lp0, float& om, float& pr) {
    const float zc = __builtin_amdgcn_fmed3f(z, -GM_ZL, GM_ZL);
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(zc));   // exp(-|zc|) in (1e-7, 1]
    const float t = 1.0f + e;                                                   // in (1, 2]
    const float tm1 = t - 1.0f;
    const float lse = tm1 > 0.f ? 0.6931471805599453f * __builtin_amdgcn_logf(t) * (e * fast_rcp(tm1)) : e;
    const float big = fast_rcp(t), small = e * big;                             // sigmoid(|zc|), sigmoid(-|zc|)
    const bool pos = zc >= 0.f, inside = zc == z;
    lp1 = fminf(zc, 0.f) - lse;
    lp0 = fminf(-zc, 0.f) - lse;
    om = inside ? (pos ? small : big) : 0.f;
    pr = inside ? (pos ? big : small) : 0.f;
}

__device__ __forceinline__ void gm_eval(const float* __restrict__ th, int D, int G, int NK, int lane, float Dc,
                                        const float (&r1)[GM_NK], const float (&r0)[GM_NK], const float (&p)[GM_NP], GmSums& s) {
    float q = 0.f, g[GM_NP], h[GM_NP * (GM_NP + 1) / 2];
#pragma unroll
    for (int i = 0; i < GM_NP; ++i) g[i] = 0.f;
#pragma unroll
    for (int i = 0; i < GM_NP * (GM_NP + 1) / 2; ++i) h[i] = 0.f;
#pragma unroll
    for (int k = 0; k < GM_NK; ++k) {
        if (k < NK) {                                               // (wave-uniform)
            const int gi = lane + 64 * k;
            const int gs = gi < G ? gi : 0;                         // past the grid: node 0 with zero counts
            float u[GM_NP];
            u[0] = 1.f;
#pragma unroll
            for (int d = 0; d < GM_MAXD; ++d) u[1 + d] = d < D ? th[gs * D + d] : 0.f;
            float sz = p[0];                                        // the order of k_grid_table_irt: b, then the dimensions
#pragma unroll
            for (int d = 0; d < GM_MAXD; ++d)
                if (d < D) sz = fmaf(u[1 + d], p[1 + d], sz);
            const float z = Dc * sz;
            float lp1, lp0, om, pr;
            gm_cell(z, lp1, lp0, om, pr);                           // om = 1 - P, pr = P; both 0 where the clamp is active
            const float c1 = r1[k], c0 = r0[k];
            q = fmaf(c1, lp1, fmaf(c0, lp0, q));
            const float r = fmaf(c1, om, -(c0 * pr));
            const float w = (c1 + c0) * (om * pr);
            int t = 0;
#pragma unroll
            for (int i = 0; i < GM_NP; ++i) {
                g[i] = fmaf(r, u[i], g[i]);
                const float wu = w * u[i];
#pragma unroll
                for (int l = i; l < GM_NP; ++l, ++t) h[t] = fmaf(wu, u[l], h[t]);
            }
        }
    }
    s.q = wave_sum_dpp(q);
#pragma unroll
    for (int i = 0; i < GM_NP; ++i) s.g[i] = i <= D ? Dc * wave_sum_dpp(g[i]) : 0.f;
    int t = 0;
#pragma unroll
    for (int i = 0; i < GM_NP; ++i)
#pragma unroll
        for (int l = i; l < GM_NP; ++l, ++t) s.h[t] = l <= D ? Dc * Dc * wave_sum_dpp(h[t]) : 0.f;
}

// delta = H^-1 g for the free unknowns (a unit row and a zero for the others) by Cholesky; false on a pivot that is not positive
__device__ __forceinline__ bool gm_solve(const GmSums& s, const bool (&fr)[GM_NP], float (&delta)[GM_NP]) {
    float A[GM_NP][GM_NP], L[GM_NP][GM_NP], y[GM_NP];
    int t = 0;
#pragma unroll
    for (int i = 0; i < GM_NP; ++i)
#pragma unroll
        for (int l = i; l < GM_NP; ++l, ++t) {
            const float v = (fr[i] && fr[l]) ? s.h[t] : (i == l ? 1.f : 0.f);
            A[i][l] = v; A[l][i] = v;
        }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < GM_NP; ++i) {
#pragma unroll
        for (int l = 0; l <= i; ++l) {
            float v = A[i][l];
#pragma unroll
            for (int k = 0; k < l; ++k) v = fmaf(-L[i][k], L[l][k], v);
            if (l == i) {
                ok = ok && (v > 0.f) && (v < 3.0e38f);
                L[i][i] = sqrtf(ok ? v : 1.f);
            } else {
                L[i][l] = v / L[l][l];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < GM_NP; ++i) {                               // L y = g
        float v = fr[i] ? s.g[i] : 0.f;
#pragma unroll
        for (int k = 0; k < i; ++k) v = fmaf(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = GM_NP - 1; i >= 0; --i) {                          // L^T delta = y
        float v = y[i];
#pragma unroll
        for (int k = i + 1; k < GM_NP; ++k) v = fmaf(-L[k][i], delta[k], v);
        delta[i] = v / L[i][i];
    }
    return ok;
}

template <int MODEL>
__global__ __launch_bounds__(GM_THREADS) void k_grid_mstep_irt(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                               const float* __restrict__ n1, const float* __restrict__ n0,
                                                               const float* __restrict__ a_free, float* __restrict__ a,
                                                               float* __restrict__ b, int newton) {
    __shared__ float th[GP_MAXG * GM_MAXD];
    for (int i = threadIdx.x; i < G * D; i += GM_THREADS) th[i] = theta[i];
    __syncthreads();                                                // the only barrier: what follows is a wave's own business
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * GM_WAVES + (threadIdx.x >> 6);
    if (j >= J) return;
    const int NK = (G + 63) >> 6;
    float r1[GM_NK], r0[GM_NK], ntot = 0.f;
#pragma unroll
    for (int k = 0; k < GM_NK; ++k) {
        const int gi = lane + 64 * k;
        const bool in = k < NK && gi < G;
        r1[k] = in ? n1[(int64_t)j * G + gi] : 0.f;
        r0[k] = in ? n0[(int64_t)j * G + gi] : 0.f;
        ntot += r1[k] + r0[k];
    }
    ntot = wave_sum_dpp(ntot);
    if (!(ntot > 0.f)) return;                                      // nobody answered the item

    float p[GM_NP];
    bool fr[GM_NP];
    p[0] = b[j]; fr[0] = true;
#pragma unroll
    for (int d = 0; d < GM_MAXD; ++d) {
        if (MODEL == 1) {
            p[1 + d] = 1.f; fr[1 + d] = false;                      // 1PL: z = Dc (theta + b)
        } else {
            p[1 + d] = d < D ? a[(int64_t)d * J + j] : 0.f;
            fr[1 + d] = d < D && (a_free == nullptr || a_free[(int64_t)d * J + j] != 0.f);
        }
    }
    GmSums cur;
    gm_eval(th, D, G, NK, lane, Dc, r1, r0, p, cur);
    for (int it = 0; it < newton; ++it) {
        float delta[GM_NP];
        if (!gm_solve(cur, fr, delta)) break;
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < GM_NP; ++i) m = fmaxf(m, fabsf(delta[i]));
        if (!(m < 3.0e38f)) break;
        float t = m > GM_STEP_CAP ? GM_STEP_CAP / m : 1.f;
        bool moved = false;
        for (int hv = 0; hv <= GM_HALVINGS && !moved; ++hv) {
            float pt[GM_NP];
#pragma unroll
            for (int i = 0; i < GM_NP; ++i) pt[i] = fr[i] ? fmaf(t, delta[i], p[i]) : p[i];
            GmSums tr;
            gm_eval(th, D, G, NK, lane, Dc, r1, r0, pt, tr);
            if (tr.q >= cur.q - GM_QTOL * fabsf(cur.q)) {
#pragma unroll
                for (int i = 0; i < GM_NP; ++i) p[i] = pt[i];
                cur = tr;
                moved = true;
            }
            t *= 0.5f;
        }
        if (!moved) break;                                          // (every later step would ask for the same move)
    }
    if (lane == 0) {
        b[j] = p[0];
#pragma unroll
        for (int d = 0; d < GM_MAXD; ++d)
            if (fr[1 + d]) a[(int64_t)d * J + j] = p[1 + d];
    }
}

__global__ __launch_bounds__(GM_THREADS) void k_grid_mstep_cdm(int K, int J, int dino, const float* __restrict__ q,
                                                               const float* __restrict__ n1, const float* __restrict__ n0,
                                                               float* __restrict__ g_un, float* __restrict__ s_un) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * GM_WAVES + (threadIdx.x >> 6);
    if (j >= J) return;
    const int G = 1 << K;
    const int qpat = gp_cdm_qpat(q, K, J, j);
    float R0 = 0.f, W0 = 0.f, R1 = 0.f, W1 = 0.f;
    for (int gi = lane; gi < G; gi += 64) {                         // a lane's patterns in ascending order
        const float c1 = n1[(int64_t)j * G + gi], c0 = n0[(int64_t)j * G + gi];
        if (gp_cdm_eta(dino, qpat, gi)) { R1 += c1; W1 += c0; } else { R0 += c1; W0 += c0; }
    }
    R0 = wave_sum_dpp(R0); W0 = wave_sum_dpp(W0); R1 = wave_sum_dpp(R1); W1 = wave_sum_dpp(W1);
    if (lane == 0) {
        if (R0 + W0 > 0.f) g_un[j] = __builtin_amdgcn_fmed3f(logf(R0) - logf(W0), -GM_ZL, GM_ZL);
        if (R1 + W1 > 0.f) s_un[j] = __builtin_amdgcn_fmed3f(logf(W1) - logf(R1), -GM_ZL, GM_ZL);
    }
}
