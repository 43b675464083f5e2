// Summed-score tables (Lord-Wingersky) for S-X2 item fit and the score -> latent conversion table.
//
// Over a sorted list of Js items and G nodes, with p1[j][g] = P(y_j = 1 | g), p0[j][g] = P(y_j = 0 | g) (both given: p0 is never
// formed as 1 - p1) and w_g = exp(logw[g]):  S(s | g) is the probability of the summed score s at node g, S_-j the same without
// item j, by the recursion  S = delta_0;  for every item k in ascending order:  S'[s] = p0 S[s] + p1 S[s - 1].  No term is
// negative, nothing cancels.  The model tables, float32 [Js][Js + 1]:
//     e1[j][s] = sum_g w_g p1[j][g] S_-j(s - 1 | g)   (e1[j][0] = 0 exactly)
//     e0[j][s] = sum_g w_g p0[j][g] S_-j(s | g)       (e0[j][Js] = 0 exactly)
// and dist[g][s] = S(s | g) over all Js items, float32 [G][Js + 1].
//
// k_sumscore<R, LEAVE>: one wave per (left-out item j, chunk of nodes); LEAVE = false: nothing left out, one wave per chunk, and
// the vector of every node is written to dist.  The score vector is blocked across the wave: lane l holds the scores R l .. R l +
// R - 1 in registers (R = 1 / 2 / 4 / 8 / 16 for Js + 1 <= 64 .. 1024), so a recursion step is R multiply-adds a lane and ONE
// cross-lane move: the lane's top register shifted up by one lane (a DPP wave shift, lane 0 receives 0).  The item probabilities
// of a node come 64 items at a time, one item a lane, and reach the step as scalars (v_readlane): no load sits in the chain of
// dependent steps.  Item j and the items past Js are the identity step (p1 = 0, p0 = 1), which leaves every register as it is,
// bit for bit.  Scores above the number of items folded in stay exact zeros.  Registers that hold only such zeros are NOT
// skipped: with the blocked layout they are the upper LANES, which a wave cannot switch off to any gain.
// A wave walks its nodes in ascending order and adds w p1 S(s - 1) and w p0 S(s) to 2 R accumulators; it writes them to its
// chunk's slab, and the slabs are added in ascending order by vx_reduce_slabs.  The chunking (ss_plan) is a function of Js and G
// alone; there is no atomic: the same call gives the same bits on every device.
//
// k_sumscore_persons: the summed score of every person over the listed items, -1 for a person with a cell that is not 0 or 1 among
// them.  A wave takes a person, a lane every 64th listed item; the ones are counted by ballots.
// k_sumscore_observed: o1[j][s] = the persons of score s with y_j = 1, over persons sorted by score.  A workgroup takes a chunk of
// persons, a thread owns the items t, t + 256, ..: it counts in registers while the score stays, and adds the count to o1 with an
// integer atomic when the score changes and at the end of the chunk (integer sums are the same in any order).
#pragma once
#include "k_util.hip"
#include "grid_plan.h"                  // the launch of vx_sumscore_model: SsPlan, ss_plan, ss_ws_floats

#define SS_MAXJ 1023                    // items of a call: the score vector has Js + 1 <= 1024 entries, 16 registers a lane
#define SS_MAXG 1024                    // nodes (GP_MAXG)
#define SS_MAXJ_ALL 4096                // columns of y
#define SS_WAVES 4                      // waves a workgroup
#define SS_OBS_THREADS 256
#define SS_OBS_TILES 4                  // items a thread of k_sumscore_observed owns at the most: 4 x 256 >= 1023
#define SS_OBS_MAX_BLOCKS 2048

// the value of lane - 1; lane 0 receives 0
__device__ __forceinline__ float ss_shift_up(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

template <int R, bool LEAVE>
__global__ __launch_bounds__(64 * SS_WAVES) void k_sumscore(const float* __restrict__ p1, const float* __restrict__ p0,
                                                            const float* __restrict__ logw, int Js, int G, int chunk, int n_chunks,
                                                            float* __restrict__ out1, float* __restrict__ out0) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SS_WAVES + (threadIdx.x >> 6)));
    if (wave >= (LEAVE ? Js * n_chunks : n_chunks)) return;
    const int j = LEAVE ? wave / n_chunks : -1;
    const int c = LEAVE ? wave - j * n_chunks : wave;
    const int g0 = c * chunk, g1 = g0 + chunk < G ? g0 + chunk : G;
    float a1[R], a0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a1[r] = a0[r] = 0.f;
    for (int g = g0; g < g1; ++g) {
        float S[R];
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = 0.f;
        if (lane == 0) S[0] = 1.0f;
        for (int k0 = 0; k0 < Js; k0 += 64) {
            const int k = k0 + lane;
            const bool fold = k < Js && k != j;
            const float pv = fold ? p1[(int64_t)k * G + g] : 0.f;
            const float qv = fold ? p0[(int64_t)k * G + g] : 1.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (k0 + 16 * t >= Js) break;
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const float p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pv), 16 * t + u));
                    const float q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), 16 * t + u));
                    const float carry = ss_shift_up(S[R - 1]);
#pragma unroll
                    for (int r = R - 1; r > 0; --r) S[r] = fmaf(p, S[r - 1], q * S[r]);
                    S[0] = fmaf(p, carry, q * S[0]);
                }
            }
        }
        if (LEAVE) {
            const float w = expf(logw[g]);
            const float wp = w * p1[(int64_t)j * G + g], wq = w * p0[(int64_t)j * G + g];
            const float carry = ss_shift_up(S[R - 1]);
#pragma unroll
            for (int r = R - 1; r > 0; --r) a1[r] = fmaf(wp, S[r - 1], a1[r]);
            a1[0] = fmaf(wp, carry, a1[0]);
#pragma unroll
            for (int r = 0; r < R; ++r) a0[r] = fmaf(wq, S[r], a0[r]);
        } else {
            float* d = out1 + (int64_t)g * (Js + 1);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (R * lane + r <= Js) d[R * lane + r] = S[r];
        }
    }
    if (LEAVE) {
        const int64_t at = ((int64_t)c * Js + j) * (Js + 1);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (R * lane + r <= Js) {
                out1[at + R * lane + r] = a1[r];
                out0[at + R * lane + r] = a0[r];
            }
    }
}

// score[i] = the number of 1s of person rows[i] (or i) over the listed items (items[k], or k), -1 unless every listed cell is 0 / 1
__global__ __launch_bounds__(256) void k_sumscore_persons(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                         int J, const int32_t* __restrict__ items, int Js,
                                                         int32_t* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nb; i += n_waves) {
        const uint8_t* row = y + (rows ? rows[i] : i) * J;
        int ones = 0;
        bool bad = false;
        for (int k0 = 0; k0 < Js; k0 += 64) {
            const int k = k0 + lane;
            uint32_t v = 0;
            if (k < Js) {
                const int col = items ? items[k] : k;
                v = (col >= 0 && col < J) ? row[col] : 255u;         // an item outside y: nobody is complete
            }
            ones += __popcll(__ballot(v == 1u));
            bad = bad || __any(v > 1u);
        }
        if (lane == 0) score[i] = bad ? -1 : ones;
    }
}

// o1[k][s] += the persons i of the chunk with score[i] = s and y[rows[i]][items[k]] = 1; score ascending (any order is counted
// right, a sorted one with few atomics).  A score outside 0 .. Js or an item outside y counts nothing.
__global__ __launch_bounds__(SS_OBS_THREADS) void k_sumscore_observed(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows,
                                                                     int64_t nb, int J, const int32_t* __restrict__ items, int Js,
                                                                     const int32_t* __restrict__ score, int32_t* __restrict__ o1,
                                                                     int64_t per_block) {
    const int64_t i0 = (int64_t)blockIdx.x * per_block;
    const int64_t i1 = i0 + per_block < nb ? i0 + per_block : nb;
    int col[SS_OBS_TILES], cnt[SS_OBS_TILES];
#pragma unroll
    for (int m = 0; m < SS_OBS_TILES; ++m) {
        const int k = (int)threadIdx.x + SS_OBS_THREADS * m;
        const int cc = k < Js ? (items ? items[k] : k) : -1;
        col[m] = (cc >= 0 && cc < J) ? cc : -1;
        cnt[m] = 0;
    }
    int cur = -1;
    for (int64_t i = i0; i < i1; ++i) {
        const int s = score[i];
        if (s != cur) {
            if (cur >= 0 && cur <= Js) {
#pragma unroll
                for (int m = 0; m < SS_OBS_TILES; ++m)
                    if (cnt[m]) atomicAdd(o1 + (int64_t)((int)threadIdx.x + SS_OBS_THREADS * m) * (Js + 1) + cur, cnt[m]);
            }
#pragma unroll
            for (int m = 0; m < SS_OBS_TILES; ++m) cnt[m] = 0;
            cur = s;
        }
        if (s < 0 || s > Js) continue;
        const uint8_t* row = y + rows[i] * J;
#pragma unroll
        for (int m = 0; m < SS_OBS_TILES; ++m)
            if (col[m] >= 0) cnt[m] += row[col[m]] == 1 ? 1 : 0;
    }
    if (cur >= 0 && cur <= Js) {
#pragma unroll
        for (int m = 0; m < SS_OBS_TILES; ++m)
            if (cnt[m]) atomicAdd(o1 + (int64_t)((int)threadIdx.x + SS_OBS_THREADS * m) * (Js + 1) + cur, cnt[m]);
    }
}
