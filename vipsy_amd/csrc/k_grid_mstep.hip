// The M-step of the Bock-Aitkin EM on the expected-count tables of k_grid_counts.hip: given n1[j][g], n0[j][g] (the posterior mass
// at node g of the persons who answered item j correctly / wrongly) every item is a small weighted logistic regression of its
// own -- or, for DINA / DINO, two ratios of sums.  2 J G floats are read once; nothing here is large.
//
// IRT (k_grid_mstep_irt<MODEL, PRIOR>): ONE kernel for the plain fit (PRIOR = false: 1PL / 2PL, vx_grid_mstep_irt) and the
// penalised one (PRIOR = true: 1PL .. 4PL, vx_grid_mstep_irt_map).  Item j maximises over its free unknowns
//
//     Q_j(p) = sum_g n1[j][g] log P_g + n0[j][g] log Q_g,      p = (b, a_0, a_1, a_2, c_un, d_un),   z = Dc (b + theta_g . a)
//
// b always, a_d where d < D and a_free is not 0 (2PL up), c_un (3PL up), d_un (4PL): at most 6 unknowns, 21 curvature terms.
//
// The method is Fisher scoring.  With dP the gradient of P and Q = 1 - P,
//     gradient = sum_g (n1 Q - n0 P) / (P Q) dP        matrix = sum_g (n1 + n0) / (P Q) dP dP^T       (positive semi-definite always).
// 1PL / 2PL: P = s(z), dP = P Q Dc (1, theta_g), so with u_g = (1, theta_g), r = n1 (1 - P) - n0 P and w = (n1 + n0) P (1 - P) these
// are Dc sum_g r u_g and Dc^2 sum_g w u_g u_g^T -- Newton's step; Dc is put on after the sums.  The cell is gm_cell: z clamped to
// +-logit(1 - eps32) as the tables' cell clamps it (irt_cell<2>); a node where the clamp is active adds its clamped term to Q_j and
// nothing to the gradient or the matrix; log P and 1 - P keep their digits where P is near 1.
//
// Mapping: ONE WAVE AN ITEM, four items a workgroup.  An item's row of each table is at most 1 024 floats = 16 a lane, read once
// (coalesced: lane l holds nodes l, l + 64, ...) and kept in registers over all steps of the launch; theta [G][D] is staged once a
// workgroup in LDS (<= 12 KB) and shared by its four items.  One evaluation gives Q_j, the gradient and the matrix: each lane adds
// its nodes in ascending order, the lanes meet in the DPP tree of wave_sum_dpp -- a fixed order, no atomics, no LDS traffic, no
// barrier after the staging: the same call gives the same bits, and an item's bits do not depend on the other items of the launch.
// A workgroup an item would put the cross-wave step (LDS + barrier) into every one of up to 64 x 9 evaluations for rows that
// fill a quarter of one wave's registers; a lane an item would read the tables with a stride of G floats.
//
// The system of at most 6 x 6 is solved by Cholesky in registers, redundantly in every lane (its inputs are wave-uniform).
// A loading with a_free = 0 is a unit row of the system with a zero right-hand side -- exact: it changes no other entry of the
// factor.  Step control: a step is accepted when Q_j does not fall by more than 1e-6 |Q_j| (the float32 rounding of a sum of at
// most 1 024 terms), else halved, at most 8 times, else the item stops where it is.  A step whose largest component exceeds
// GM_STEP_CAP = 4 is scaled down to that length: an item whose observed answers are all equal has its maximum at infinity, and on
// the way there the system loses rank as node after node reaches the clamp -- the last solvable system can ask for a step of any
// size.  With the cap such an item moves at most 4 a step until every node is clamped, the curvature is exactly zero, the pivot
// test fails and the item stops: finite, at most 4 x newton from where it started.
//
// Keeps its bits: a loading with a_free = 0 is never written (nor its prior row read); c_un / d_un outside the model are no unknowns
// at all and may be NULL; an item nobody answered (sum n = 0) keeps its values; on a pivot that is not positive or not finite the
// item stops where it is.
//
// What a prior adds (PRIOR = true; Bayes-modal EM, as BILOG, mirt and TAM have it): a normal prior on every free unknown,
//     Q_j -= 1/2 sum_k prec_k (p_k - mean_k)^2        gradient_k -= prec_k (p_k - mean_k)        matrix_kk += prec_k,
// and the step control above runs on the PENALISED Q_j.  PRIOR is a compile-time flag, not a null test: without it no penalty
// term is formed at all, so which roundings happen does not hang on what the compiler contracts around a `- 0.f`.
// prior: float [2][GM_ROWS][J] -- prior[k][j] the mean and prior[GM_ROWS + k][j] the precision (1 / sd^2) of unknown k of item j,
// k = 0: b, 1 .. 3: a_0 .. a_2, 4: c_un, 5: d_un, always six rows each; rows the model or D does not have are not read.
// Precision 0: no prior on that unknown (the mean must still be finite).  Precisions are >= 0 and finite: the caller's duty
// (vipsy_amd/grid.py: em_prior refuses anything else; the gate cannot look into device memory).
// lprior (optional, [J]; PRIOR only): -1/2 sum_k prec_k (p_k - mean_k)^2 over the item's free unknowns AT THE PARAMETERS THE CALL
// STARTED FROM, constants dropped; an item nobody answered reports its term too.
//
// The 3PL / 4PL cell (penalised only: with a guessing or slipping asymptote the likelihood part is not concave and, unpenalised,
// walks the asymptote logits to the clamp; the prior is what makes the problem well posed).  The arithmetic of irt_cell<3 / 4>
// (vx_common.h),
//     P = c + (d - c) s(z),   Q = (1 - d) + (d - c) s(-z),   z in k_grid_table_irt's order,
// c = min(s(c_un), 1 - eps32), d = min(s(d_un), 1 - eps32) and 1 - d = max(s(-d_un), eps32) formed on its own as the tables form
// them (3PL: d = 1, 1 - d = 0): Q is never 1 - P.  P and Q are clamped to [eps32, 1 - eps32]; a node that is not `inside`
// (P < eps32 or Q < eps32) adds its clamped log term to Q_j and nothing to the gradient or the matrix.  The log of the larger of
// the two is taken as log1p(-the smaller) (gm_log1m): the same number, with the digits a P near 1 no longer has.
//     dP/dz = (d - c) s(z) s(-z), grad z = Dc (1, theta_g);   dP/dc_un = s(-z) c (1 - c);   dP/dd_un = s(z) d (1 - d).
// d <= c is NOT excluded by a constraint: both asymptotes are free logits, and it is the prior that keeps them apart (the host
// side refuses a 3PL / 4PL call without a finite prior on c_un, and on d_un for 4PL).  With d < c the curve falls, P and Q stay
// probabilities and nothing here breaks; the item is then simply a bad item under a bad prior.
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
#define GM_NZ (GM_MAXD + 1)              // unknowns inside z: b, a_0 .. a_{D-1}
#define GM_ROWS 6                        // rows of means, and of precisions, in `prior`
#define GM_MAX_NEWTON 64
#define GM_HALVINGS 8
#define GM_STEP_CAP 4.0f
#define GM_QTOL 1e-6f
#define GM_ZL 15.942384719848633f        // logit(1 - eps32), the clamp of irt_cell<2>

// unknowns of an item: b, a_0 .. a_2, then c_un (3PL up) and d_un (4PL)
template <int MODEL>
struct GmDims {
    static constexpr int NP = MODEL <= 2 ? GM_NZ : (MODEL == 3 ? GM_NZ + 1 : GM_NZ + 2);
};

// Q_j, its gradient and the matrix (upper triangle row by row) of one item
template <int NP>
struct GmSums {
    float q;
    float g[NP];
    float h[NP * (NP + 1) / 2];
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

// 1/2 sum prec (p - mean)^2 over the free unknowns, in ascending order
template <int NP>
__device__ __forceinline__ float gm_penalty(const float (&p)[NP], const bool (&fr)[NP], const float (&pm)[NP], const float (&pp)[NP]) {
    float pen = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const float dv = p[i] - pm[i];
        if (fr[i]) pen = fmaf(0.5f * pp[i], dv * dv, pen);
    }
    return pen;
}

// log(1 - x) for x in [eps32, 1/2], to the relative accuracy of the hardware log2: with t = 1 - x rounded, t - 1 is exact and
// log(t) x / (1 - t) takes back what the rounding of t took (gm_cell's log1p).  The log of whichever of P and Q is the larger
// is formed so, from the smaller: log(P) of a P near 1 that was rounded at eps32 / 2 is off by 6e-8 A COUNT, and Q_j of an item
// nearly everybody answers alike (|log P| of 1e-3) is then rounded at 3e-5 of its size, thirty times what the acceptance rule
// allows for -- near its maximum every trial looks like a fall and the item stops on its halvings, short of it.
__device__ __forceinline__ float gm_log1m(float x) {
    const float t = 1.0f - x;
    return fast_log(t) * (x * fast_rcp(1.0f - t));
}

// One evaluation at the unknowns p; fr, pm (means) and pp (precisions) are read with PRIOR only
template <int MODEL, bool PRIOR>
__device__ __forceinline__ void gm_eval(const float* __restrict__ th, int D, int G, int NK, int lane, float Dc,
                                        const float (&r1)[GM_NK], const float (&r0)[GM_NK],
                                        const float (&p)[GmDims<MODEL>::NP], const bool (&fr)[GmDims<MODEL>::NP],
                                        const float (&pm)[GmDims<MODEL>::NP], const float (&pp)[GmDims<MODEL>::NP],
                                        GmSums<GmDims<MODEL>::NP>& s) {
    constexpr int NP = GmDims<MODEL>::NP, NH = NP * (NP + 1) / 2;
    float q = 0.f, g[NP], h[NH];
#pragma unroll
    for (int i = 0; i < NP; ++i) g[i] = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i) h[i] = 0.f;
    // the asymptotes as k_grid_table_irt caps them (wave-uniform)
    float c = 0.f, dd = 1.f, omd = 0.f, cc1 = 0.f, dd1 = 0.f;
    if constexpr (MODEL >= 3) {
        c = fminf(sigmoidf_(p[GM_NZ]), 1.0f - VX_EPS32);
        cc1 = c * (1.0f - c);
    }
    if constexpr (MODEL == 4) {
        dd = fminf(sigmoidf_(p[GM_NZ + 1]), 1.0f - VX_EPS32);
        omd = fmaxf(sigmoidf_(-p[GM_NZ + 1]), VX_EPS32);
        dd1 = dd * omd;
    }
    const float dmc = dd - c;
#pragma unroll
    for (int k = 0; k < GM_NK; ++k) {
        if (k < NK) {                                               // (wave-uniform)
            const int gi = lane + 64 * k;
            const int gs = gi < G ? gi : 0;                         // past the grid: node 0 with zero counts
            float u[GM_NZ];
            u[0] = 1.f;
#pragma unroll
            for (int d = 0; d < GM_MAXD; ++d) u[1 + d] = d < D ? th[gs * D + d] : 0.f;
            float sz = p[0];                                        // the order of k_grid_table_irt: b, then the dimensions
#pragma unroll
            for (int d = 0; d < GM_MAXD; ++d)
                if (d < D) sz = fmaf(u[1 + d], p[1 + d], sz);
            const float z = Dc * sz;
            const float c1 = r1[k], c0 = r0[k];
            float lp1, lp0, rr, ww, v[NP];                          // log P, log Q, the weights of dP and dP dP^T, dP
            if constexpr (MODEL <= 2) {
                float om, pr;
                gm_cell(z, lp1, lp0, om, pr);                       // om = 1 - P, pr = P; both 0 where the clamp is active
                rr = fmaf(c1, om, -(c0 * pr));
                ww = (c1 + c0) * (om * pr);
#pragma unroll
                for (int i = 0; i < GM_NZ; ++i) v[i] = u[i];        // (Dc is put on after the sums)
            } else {
                const float e = __expf(-fabsf(z));
                const float r = fast_rcp(1.0f + e);
                const float sg = (z >= 0.f) ? r : e * r;            // sigmoid(z)
                const float sn = (z >= 0.f) ? e * r : r;            // sigmoid(-z), no cancellation
                const float P = c + dmc * sg;
                const float Q = omd + dmc * sn;
                const bool inside = (P >= VX_EPS32) && (Q >= VX_EPS32);
                const float Pc = fminf(fmaxf(P, VX_EPS32), 1.0f - VX_EPS32);
                const float Qc = fminf(fmaxf(Q, VX_EPS32), 1.0f - VX_EPS32);
                const float sm = fminf(Pc, Qc);                     // <= 1/2: P + Q = 1 but for the caps
                const float ls = fast_log(sm), lb = gm_log1m(sm);
                lp1 = Pc >= Qc ? lb : ls;
                lp0 = Pc >= Qc ? ls : lb;
                const float inv = inside ? fast_rcp(Pc * Qc) : 0.f;
                rr = fmaf(c1, Qc, -(c0 * Pc)) * inv;
                ww = (c1 + c0) * inv;
                const float pz = dmc * sg * sn;
#pragma unroll
                for (int i = 0; i < GM_NZ; ++i) v[i] = pz * u[i];
                v[GM_NZ] = sn * cc1;
                if constexpr (MODEL == 4) v[NP - 1] = sg * dd1;
            }
            q = fmaf(c1, lp1, fmaf(c0, lp0, q));
            int t = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                g[i] = fmaf(rr, v[i], g[i]);
                const float wv = ww * v[i];
#pragma unroll
                for (int l = i; l < NP; ++l, ++t) h[t] = fmaf(wv, v[l], h[t]);
            }
        }
    }
    // unknown i takes part when it is b, a dimension of the model, or an asymptote; the unknowns inside z carry Dc
    if constexpr (PRIOR) s.q = wave_sum_dpp(q) - gm_penalty<NP>(p, fr, pm, pp);
    else s.q = wave_sum_dpp(q);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool on = i >= GM_NZ || i <= D;
        const float sc = i < GM_NZ ? Dc : 1.f;
        if constexpr (PRIOR) s.g[i] = on ? sc * wave_sum_dpp(g[i]) - (fr[i] ? pp[i] * (p[i] - pm[i]) : 0.f) : 0.f;
        else s.g[i] = on ? sc * wave_sum_dpp(g[i]) : 0.f;
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int l = i; l < NP; ++l, ++t) {
            const bool on = (i >= GM_NZ || i <= D) && (l >= GM_NZ || l <= D);
            const float sc = (i < GM_NZ ? Dc : 1.f) * (l < GM_NZ ? Dc : 1.f);
            if constexpr (PRIOR) s.h[t] = on ? sc * wave_sum_dpp(h[t]) + ((i == l && fr[i]) ? pp[i] : 0.f) : 0.f;
            else s.h[t] = on ? sc * wave_sum_dpp(h[t]) : 0.f;
        }
}

// delta = H^-1 g for the free unknowns (a unit row and a zero for the others) by Cholesky; false on a pivot that is not positive
template <int NP>
__device__ __forceinline__ bool gm_solve(const GmSums<NP>& s, const bool (&fr)[NP], float (&delta)[NP]) {
    float A[NP][NP], L[NP][NP], y[NP];
    int t = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int l = i; l < NP; ++l, ++t) {
            const float v = (fr[i] && fr[l]) ? s.h[t] : (i == l ? 1.f : 0.f);
            A[i][l] = v; A[l][i] = v;
        }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
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
    for (int i = 0; i < NP; ++i) {                                  // L y = g
        float v = fr[i] ? s.g[i] : 0.f;
#pragma unroll
        for (int k = 0; k < i; ++k) v = fmaf(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {                             // L^T delta = y
        float v = y[i];
#pragma unroll
        for (int k = i + 1; k < NP; ++k) v = fmaf(-L[k][i], delta[k], v);
        delta[i] = v / L[i][i];
    }
    return ok;
}

// c_un / d_un are read and written from MODEL 3 / 4 up, prior and lprior with PRIOR only
template <int MODEL, bool PRIOR>
__global__ __launch_bounds__(GM_THREADS) void k_grid_mstep_irt(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                               const float* __restrict__ n1, const float* __restrict__ n0,
                                                               const float* __restrict__ a_free, float* __restrict__ a,
                                                               float* __restrict__ b, float* __restrict__ c_un,
                                                               float* __restrict__ d_un, const float* __restrict__ prior,
                                                               float* __restrict__ lprior, int newton) {
    constexpr int NP = GmDims<MODEL>::NP;
    __shared__ float th[GP_MAXG * GM_MAXD];
    for (int i = threadIdx.x; i < G * D; i += GM_THREADS) th[i] = theta[i];
    __syncthreads();                                                // the only barrier: what follows is a wave's own business
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * GM_WAVES + (threadIdx.x >> 6);
    if (j >= J) return;

    float p[NP], pm[NP], pp[NP];
    bool fr[NP];
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
    if constexpr (MODEL >= 3) { p[GM_NZ] = c_un[j]; fr[GM_NZ] = true; }
    if constexpr (MODEL == 4) { p[NP - 1] = d_un[j]; fr[NP - 1] = true; }
#pragma unroll
    for (int i = 0; i < NP; ++i) {                                  // (row i of `prior` is unknown i in every model)
        pm[i] = PRIOR && fr[i] ? prior[(int64_t)i * J + j] : 0.f;
        pp[i] = PRIOR && fr[i] ? prior[(int64_t)(GM_ROWS + i) * J + j] : 0.f;
    }
    if constexpr (PRIOR)
        if (lprior != nullptr && lane == 0) lprior[j] = -gm_penalty<NP>(p, fr, pm, pp);

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

    GmSums<NP> cur;
    gm_eval<MODEL, PRIOR>(th, D, G, NK, lane, Dc, r1, r0, p, fr, pm, pp, cur);
    for (int it = 0; it < newton; ++it) {
        float delta[NP];
        if (!gm_solve<NP>(cur, fr, delta)) break;
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i) m = fmaxf(m, fabsf(delta[i]));
        if (!(m < 3.0e38f)) break;
        float t = m > GM_STEP_CAP ? GM_STEP_CAP / m : 1.f;
        bool moved = false;
        for (int hv = 0; hv <= GM_HALVINGS && !moved; ++hv) {
            float pt[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) pt[i] = fr[i] ? fmaf(t, delta[i], p[i]) : p[i];
            GmSums<NP> tr;
            gm_eval<MODEL, PRIOR>(th, D, G, NK, lane, Dc, r1, r0, pt, fr, pm, pp, tr);
            if (tr.q >= cur.q - GM_QTOL * fabsf(cur.q)) {
#pragma unroll
                for (int i = 0; i < NP; ++i) p[i] = pt[i];
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
        if constexpr (MODEL >= 3) c_un[j] = p[GM_NZ];
        if constexpr (MODEL == 4) d_un[j] = p[NP - 1];
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
