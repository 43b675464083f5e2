// The penalised M-step of the Bock-Aitkin EM (Bayes-modal EM, as BILOG, mirt and TAM have it): k_grid_mstep.hip's item-wise
// maximisation with a normal prior on every unknown, for all four IRT models.  On the tables n1[j][g], n0[j][g] of
// k_grid_counts.hip item j maximises
//
//     Q_j(p) = sum_g n1 log P_g + n0 log Q_g - 1/2 sum_k prec_k (p_k - mean_k)^2,      p = (b, a_0, a_1, a_2, c_un, d_un)
//
// over its free unknowns: b always, a_d where d < D and a_free is not 0 (2PL up), c_un (3PL up), d_un (4PL) -- at most 6, so
// at most 21 curvature terms.  With a guessing or slipping asymptote the likelihood part is not concave and, unpenalised, walks
// the asymptote logits to the clamp; the prior is what makes the problem well posed.
//
// The cell.  1PL / 2PL: gm_cell of k_grid_mstep.hip as it stands (z clamped to +-logit(1 - eps32), a clamped node adds its
// clamped term to Q_j and nothing else).  3PL / 4PL: the arithmetic of irt_cell<3 / 4> (vx_common.h),
//     P = c + (d - c) s(z),   Q = (1 - d) + (d - c) s(-z),   z = Dc (b + theta_g . a) in k_grid_table_irt's order,
// c = min(s(c_un), 1 - eps32), d = min(s(d_un), 1 - eps32) and 1 - d = max(s(-d_un), eps32) formed on its own as the tables form
// them (3PL: d = 1, 1 - d = 0): Q is never 1 - P.  P and Q are clamped to [eps32, 1 - eps32]; a node that is not `inside`
// (P < eps32 or Q < eps32) adds its clamped log term to Q_j and nothing to the gradient or the curvature.  The log of the
// larger of the two is taken as log1p(-the smaller) (gmm_log1m): the same number, with the digits a P near 1 no longer has.
//
// The method is Fisher scoring.  With dP the gradient of P,
//     dP/dz = (d - c) s(z) s(-z), grad z = Dc (1, theta_g);   dP/dc_un = s(-z) c (1 - c);   dP/dd_un = s(z) d (1 - d),
//     gradient = sum_g (n1 Q - n0 P) / (P Q) dP - prec (p - mean)
//     matrix   = sum_g (n1 + n0) / (P Q) dP dP^T + diag(prec)          (positive semi-definite always),
// which for 1PL / 2PL is k_grid_mstep_irt's Newton: (n1 Q - n0 P) / (P Q) dP/dz = n1 (1 - P) - n0 P.
//
// d <= c is NOT excluded by a constraint: both asymptotes are free logits, and it is the prior that keeps them apart (the host
// side refuses a 3PL / 4PL call without a finite prior on c_un, and on d_un for 4PL).  With d < c the curve falls, P and Q stay
// probabilities and nothing here breaks; the item is then simply a bad item under a bad prior.
//
// Mapping, as k_grid_mstep.hip: ONE WAVE AN ITEM, four items a workgroup; the two table rows (at most 16 floats a lane each) stay
// in registers over all steps; theta is staged once in LDS behind the launch's only barrier; each lane adds its nodes in
// ascending order and every sum goes through wave_sum_dpp -- a fixed order, no atomics: the same call gives the same bits, and an
// item's bits do not depend on the other items of the launch.  The Cholesky of at most 6 x 6 runs redundantly in every lane.
// Step control is k_grid_mstep_irt's on the PENALISED Q_j: accept when it does not fall by more than 1e-6 |Q_j|, else halve, at
// most 8 times, else the item stops; the step's largest component is capped at 4.
//
// Fixed and untouched: a loading with a_free = 0 is a unit row of the system and is never written (its prior row is not read);
// c_un / d_un outside the model are no unknowns at all and may be NULL; an item nobody answered keeps its bits; on a pivot that
// is not positive or not finite the item stops where it is.
//
// prior: float [2][GMM_ROWS][J] -- prior[k][j] the mean and prior[GMM_ROWS + k][j] the precision (1 / sd^2) of unknown k of item
// j, k = 0: b, 1 .. 3: a_0 .. a_2, 4: c_un, 5: d_un, always six rows each; rows the model or D does not have are not read.
// Precision 0: no prior on that unknown (the mean must still be finite).  Precisions are >= 0 and finite: the caller's duty
// (vipsy_amd/grid.py: em_prior refuses anything else; the gate cannot look into device memory).
// lprior (optional, [J]): -1/2 sum_k prec_k (p_k - mean_k)^2 over the item's free unknowns AT THE PARAMETERS THE CALL STARTED
// FROM, constants dropped; an item nobody answered reports its term too.
#pragma once
#include "k_grid_mstep.hip"

#define GMM_ROWS 6                               // rows of means, and of precisions, in `prior`
#define GMM_NZ (GM_MAXD + 1)                     // unknowns inside z: b, a_0 .. a_{D-1}

template <int MODEL>
struct GmmDims {
    static constexpr int NP = MODEL <= 2 ? GMM_NZ : (MODEL == 3 ? GMM_NZ + 1 : GMM_NZ + 2);
    static constexpr int NH = NP * (NP + 1) / 2;
};

// the penalised Q, its gradient and the Fisher matrix (upper triangle row by row) of one item
template <int NP>
struct GmmSums {
    float q;
    float g[NP];
    float h[NP * (NP + 1) / 2];
};

// 1/2 sum prec (p - mean)^2 over the free unknowns, in ascending order
template <int NP>
__device__ __forceinline__ float gmm_penalty(const float (&p)[NP], const bool (&fr)[NP], const float (&pm)[NP], const float (&pp)[NP]) {
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
__device__ __forceinline__ float gmm_log1m(float x) {
    const float t = 1.0f - x;
    return fast_log(t) * (x * fast_rcp(1.0f - t));
}

template <int MODEL>
__device__ __forceinline__ void gmm_eval(const float* __restrict__ th, int D, int G, int NK, int lane, float Dc,
                                         const float (&r1)[GM_NK], const float (&r0)[GM_NK],
                                         const float (&p)[GmmDims<MODEL>::NP], const bool (&fr)[GmmDims<MODEL>::NP],
                                         const float (&pm)[GmmDims<MODEL>::NP], const float (&pp)[GmmDims<MODEL>::NP],
                                         GmmSums<GmmDims<MODEL>::NP>& s) {
    constexpr int NP = GmmDims<MODEL>::NP, NH = GmmDims<MODEL>::NH;
    float q = 0.f, g[NP], h[NH];
#pragma unroll
    for (int i = 0; i < NP; ++i) g[i] = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i) h[i] = 0.f;
    // the asymptotes as k_grid_table_irt caps them (wave-uniform)
    float c = 0.f, dd = 1.f, omd = 0.f, cc1 = 0.f, dd1 = 0.f;
    if constexpr (MODEL >= 3) {
        c = fminf(sigmoidf_(p[GMM_NZ]), 1.0f - VX_EPS32);
        cc1 = c * (1.0f - c);
    }
    if constexpr (MODEL == 4) {
        dd = fminf(sigmoidf_(p[GMM_NZ + 1]), 1.0f - VX_EPS32);
        omd = fmaxf(sigmoidf_(-p[GMM_NZ + 1]), VX_EPS32);
        dd1 = dd * omd;
    }
    const float dmc = dd - c;
#pragma unroll
    for (int k = 0; k < GM_NK; ++k) {
        if (k < NK) {                                               // (wave-uniform)
            const int gi = lane + 64 * k;
            const int gs = gi < G ? gi : 0;                         // past the grid: node 0 with zero counts
            float u[GMM_NZ];
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
                for (int i = 0; i < GMM_NZ; ++i) v[i] = u[i];       // (Dc is put on after the sums, as k_grid_mstep_irt does)
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
                const float ls = fast_log(sm), lb = gmm_log1m(sm);
                lp1 = Pc >= Qc ? lb : ls;
                lp0 = Pc >= Qc ? ls : lb;
                const float inv = inside ? fast_rcp(Pc * Qc) : 0.f;
                rr = fmaf(c1, Qc, -(c0 * Pc)) * inv;
                ww = (c1 + c0) * inv;
                const float pz = dmc * sg * sn;
#pragma unroll
                for (int i = 0; i < GMM_NZ; ++i) v[i] = pz * u[i];
                v[GMM_NZ] = sn * cc1;
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
    s.q = wave_sum_dpp(q) - gmm_penalty<NP>(p, fr, pm, pp);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool on = i >= GMM_NZ || i <= D;
        const float sc = i < GMM_NZ ? Dc : 1.f;
        s.g[i] = on ? sc * wave_sum_dpp(g[i]) - (fr[i] ? pp[i] * (p[i] - pm[i]) : 0.f) : 0.f;
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int l = i; l < NP; ++l, ++t) {
            const bool on = (i >= GMM_NZ || i <= D) && (l >= GMM_NZ || l <= D);
            const float sc = (i < GMM_NZ ? Dc : 1.f) * (l < GMM_NZ ? Dc : 1.f);
            s.h[t] = on ? sc * wave_sum_dpp(h[t]) + ((i == l && fr[i]) ? pp[i] : 0.f) : 0.f;
        }
}

// delta = H^-1 g for the free unknowns (a unit row and a zero for the others) by Cholesky; false on a pivot that is not positive
// (gm_solve of k_grid_mstep.hip for NP unknowns)
template <int NP>
__device__ __forceinline__ bool gmm_solve(const GmmSums<NP>& s, const bool (&fr)[NP], float (&delta)[NP]) {
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

template <int MODEL>
__global__ __launch_bounds__(GM_THREADS) void k_grid_mstep_irt_map(int D, int J, int G, float Dc, const float* __restrict__ theta,
                                                                   const float* __restrict__ n1, const float* __restrict__ n0,
                                                                   const float* __restrict__ a_free, float* __restrict__ a,
                                                                   float* __restrict__ b, float* __restrict__ c_un,
                                                                   float* __restrict__ d_un, const float* __restrict__ prior,
                                                                   float* __restrict__ lprior, int newton) {
    constexpr int NP = GmmDims<MODEL>::NP;
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
    if constexpr (MODEL >= 3) { p[GMM_NZ] = c_un[j]; fr[GMM_NZ] = true; }
    if constexpr (MODEL == 4) { p[NP - 1] = d_un[j]; fr[NP - 1] = true; }
#pragma unroll
    for (int i = 0; i < NP; ++i) {                                  // (row i of `prior` is unknown i in every model)
        pm[i] = fr[i] ? prior[(int64_t)i * J + j] : 0.f;
        pp[i] = fr[i] ? prior[(int64_t)(GMM_ROWS + i) * J + j] : 0.f;
    }
    if (lprior != nullptr && lane == 0) lprior[j] = -gmm_penalty<NP>(p, fr, pm, pp);

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

    GmmSums<NP> cur;
    gmm_eval<MODEL>(th, D, G, NK, lane, Dc, r1, r0, p, fr, pm, pp, cur);
    for (int it = 0; it < newton; ++it) {
        float delta[NP];
        if (!gmm_solve<NP>(cur, fr, delta)) break;
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
            GmmSums<NP> tr;
            gmm_eval<MODEL>(th, D, G, NK, lane, Dc, r1, r0, pt, fr, pm, pp, tr);
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
        if constexpr (MODEL >= 3) c_un[j] = p[GMM_NZ];
        if constexpr (MODEL == 4) d_un[j] = p[NP - 1];
    }
}
