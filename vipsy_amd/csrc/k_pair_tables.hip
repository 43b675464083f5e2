// Pairwise 2 x 2 tables of the responses: the observed side of Chen & Thissen's LD X2 (and of any later limited-information
// statistic).  With u_ij = [y_ij == 1], z_ij = [y_ij == 0] (every byte >= 2 is not observed, 254 / 255 among them, as k_grid_pairs
// reads them) and I_jk the persons with both cells observed, four tables int32 [J][J]:
//
//     n11 = u^T u      n10 = u^T z      n01 = z^T u      n00 = z^T z          n_ab[j][k] = |{i in I_jk : y_ij = a, y_ik = b}|
//
// The kernel accumulates (u^T u, u^T m, m^T u, m^T m) with m = u + z = [y < 2] on v_mfma_i32_32x32x32_i8 -- 0 / 1 bytes, int32
// accumulators, four MFMAs a tile pair and k-step of 32 persons -- and takes the differences when it leaves: n10 = u^T m - u^T u,
// n01 = m^T u - u^T u, n00 = m^T m - u^T m - m^T u + u^T u.  m costs one zero-byte test on a packed dword and u = y & m one AND;
// z would cost a second test.  Integers: exact up to 2^31 - 1 persons, the same bits in any summation order.
//
//   tiles     The items come in groups of 128 (a panel).  Tile f of group g holds the items 128 g + 4 i + f, i = 0 .. 31: the FOUR
//             tiles of a group interleave, so that one dword of a person's row -- items 4 i .. 4 i + 3 -- holds one byte of each.
//             A tile is any 32 items; the epilogue knows which.
//   staging   workgroup = (pair ga <= gb of item groups, chunk of person stages), 512 threads.  A stage is 128 persons: their
//             rows, gathered through `rows`, are read coalesced along the items (a dword a lane where J and y allow, bytes where
//             not), one stage ahead into registers, and stored person-major in LDS, 128 B a person and panel (32 KB for the two
//             panels; ds_read_b32 is banked by half-wave, and a half-wave reads 32 consecutive dwords: no padding is needed).
//   transpose in registers: lane (i = lane & 31, h = lane >> 5) reads the dword of items 4 i .. 4 i + 3 of the persons 16 h + e,
//             e = 0 .. 15, of the k-step -- sixteen ds_read_b32, which serve every tile of the group -- and picks byte f of four
//             persons into one dword with three v_perm_b32 (the selector is a register: f is the wave's).  Four such dwords are
//             the fragment: item 4 i + f, persons 16 h .. 16 h + 15, the operand layout of the 32x32x32 i8 MFMA, A and B alike.
//   products  wave w holds row tile w & 3 of group ga against the column tiles 2 (w >> 2), 2 (w >> 2) + 1 of group gb: eight
//             accumulators (128 registers), eight MFMAs a k-step against three fragments built.  A diagonal group pair computes
//             all its 16 tile pairs, both triangles: nothing is mirrored there.
//   sums      the chunk's differences are added to the tables with integer atomics (the call zeroes the tables first, on the
//             same stream; k_sumscore_observed is the precedent).  Zeros are not sent.  The blocks below the diagonal of item
//             groups are filled behind the launch from their transpose partners (k_pair_tables_mirror: n11 and n00 mirrored,
//             n10[k][j] = n01[j][k]): transposed atomics, a cache line a lane, cost more than all the products.
// Persons past nb, items past J and bytes >= 2 add exact zeros.
#pragma once
#include "k_util.hip"
#include "grid_plan.h"                  // PT_GROUP, PT_STAGE, PT_MAXJ, pt_plan

#define PT_THREADS 512
#define PT_PANEL_DWORDS (PT_STAGE * (PT_GROUP / 4))
#define PT_FETCH 8                      // dwords of a panel a thread stages: 128 persons x 32 dwords / 512 threads

typedef int pt_i32x4 __attribute__((ext_vector_type(4)));
typedef int pt_i32x16 __attribute__((ext_vector_type(16)));

// the four bytes of the items item0 .. item0 + 3 of the row at byte offset `base` (negative: a person past nb); 255 (not
// observed) for such a person and for an item past J.  Branch-free: a cell that is not there is read at offset 0, which every
// call owns, and replaced behind the load, so that a stage's loads are all in flight together.  DWORDS: J % 4 == 0 and y aligned
// to 4 bytes, so the dword of four items lies inside the row or past it as a whole.
template <bool DWORDS>
__device__ __forceinline__ uint32_t pt_load(const uint8_t* __restrict__ y, int64_t base, int J, int item0) {
    if (DWORDS) {
        const bool ok = base >= 0 && item0 < J;
        const uint32_t v = *(const uint32_t*)(y + (ok ? base + item0 : 0));
        return ok ? v : 0xffffffffu;
    }
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const bool ok = base >= 0 && item0 + b < J;
        const uint32_t byte = y[ok ? base + item0 + b : 0];
        v |= (ok ? byte : 255u) << (8 * b);
    }
    return v;
}

// a stage's share of a thread: dword tid & 31 of the persons (tid >> 5) + 16 t, t = 0 .. 7, of one panel or of both
template <bool DWORDS>
__device__ __forceinline__ void pt_fetch(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb, int J,
                                         int64_t stage, int ga, int gb, uint32_t (&ra)[PT_FETCH], uint32_t (&rb)[PT_FETCH]) {
    const int q = threadIdx.x & 31, p0 = threadIdx.x >> 5;
    const bool two = ga != gb;
#pragma unroll
    for (int t = 0; t < PT_FETCH; ++t) {
        const int64_t pid = stage * PT_STAGE + p0 + 16 * t;
        const int64_t row = rows ? rows[pid < nb ? pid : nb - 1] : pid;
        const int64_t base = pid < nb ? row * J : (int64_t)-1;
        ra[t] = pt_load<DWORDS>(y, base, J, ga * PT_GROUP + 4 * q);
        rb[t] = two ? pt_load<DWORDS>(y, base, J, gb * PT_GROUP + 4 * q) : 0u;
    }
}

// NF fragments of one k-step out of a staged panel: src = the lane's dword of the k-step's person 16 h; f[n] = the tile.
// u = [y == 1] and m = [y < 2] as 0 / 1 bytes, 16 persons of one item a lane.
template <int NF>
__device__ __forceinline__ void pt_fragments(const uint32_t* __restrict__ src, const int (&f)[NF], pt_i32x4 (&u)[NF],
                                             pt_i32x4 (&m)[NF]) {
    uint32_t sel[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) sel[n] = (uint32_t)f[n] | ((uint32_t)(4 + f[n]) << 8) | 0x0c0c0000u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t d0 = src[(4 * g + 0) * (PT_GROUP / 4)], d1 = src[(4 * g + 1) * (PT_GROUP / 4)];
        const uint32_t d2 = src[(4 * g + 2) * (PT_GROUP / 4)], d3 = src[(4 * g + 3) * (PT_GROUP / 4)];
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const uint32_t t01 = __builtin_amdgcn_perm(d1, d0, sel[n]);             // byte f of person 4 g, of person 4 g + 1
            const uint32_t t23 = __builtin_amdgcn_perm(d3, d2, sel[n]);
            const uint32_t raw = __builtin_amdgcn_perm(t23, t01, 0x05040100u);      // item 4 i + f of the persons 4 g .. 4 g + 3
            // a byte is < 2 iff its upper seven bits are zero: (y >> 1) + 0x7f carries into bit 7 iff they are not
            const uint32_t nz = ((((raw >> 1) & 0x7f7f7f7fu) + 0x7f7f7f7fu) >> 7) & 0x01010101u;
            const uint32_t mm = nz ^ 0x01010101u;
            m[n][g] = (int)mm;
            u[n][g] = (int)(raw & mm);
        }
    }
}

__device__ __forceinline__ pt_i32x16 pt_mfma(pt_i32x4 a, pt_i32x4 b, pt_i32x16 c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
}

template <bool DWORDS>
__global__ __launch_bounds__(PT_THREADS) void k_pair_tables(const uint8_t* __restrict__ y, const int64_t* __restrict__ rows, int64_t nb,
                                                            int J, int groups, int64_t n_stages, int64_t stages_per_chunk,
                                                            int32_t* __restrict__ n11, int32_t* __restrict__ n10,
                                                            int32_t* __restrict__ n01, int32_t* __restrict__ n00) {
    __shared__ uint32_t panel[2][PT_PANEL_DWORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5, rt = wave & 3, ch = wave >> 2;
    const int64_t n_bp = (int64_t)groups * (groups + 1) / 2;
    const int64_t chunk = blockIdx.x / n_bp;
    int rem = (int)(blockIdx.x % n_bp), ga = 0;
    while (rem >= groups - ga) { rem -= groups - ga; ++ga; }
    const int gb = ga + rem;
    const bool two = ga != gb;
    const int64_t s0 = chunk * stages_per_chunk;
    const int64_t s1 = s0 + stages_per_chunk < n_stages ? s0 + stages_per_chunk : n_stages;

    pt_i32x16 acc[2][4];                                            // [column tile][u^T u, u^T m, m^T u, m^T m]
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][t][r] = 0;

    uint32_t ra[PT_FETCH], rb[PT_FETCH];
    if (s0 < s1) pt_fetch<DWORDS>(y, rows, nb, J, s0, ga, gb, ra, rb);
    const uint32_t* pa = panel[0];
    const uint32_t* pb = two ? panel[1] : panel[0];
    const int fa[1] = {rt}, fb[2] = {2 * ch, 2 * ch + 1};
    for (int64_t s = s0; s < s1; ++s) {
        __syncthreads();                                            // the last stage has been read
#pragma unroll
        for (int t = 0; t < PT_FETCH; ++t) {
            const int at = ((tid >> 5) + 16 * t) * (PT_GROUP / 4) + (tid & 31);
            panel[0][at] = ra[t];
            if (two) panel[1][at] = rb[t];
        }
        __syncthreads();
        if (s + 1 < s1) pt_fetch<DWORDS>(y, rows, nb, J, s + 1, ga, gb, ra, rb);       // in flight under the products
#pragma unroll
        for (int ks = 0; ks < PT_STAGE / 32; ++ks) {
            const int at = (32 * ks + 16 * h) * (PT_GROUP / 4) + i;
            pt_i32x4 au[1], am[1], bu[2], bm[2];
            pt_fragments<1>(pa + at, fa, au, am);
            pt_fragments<2>(pb + at, fb, bu, bm);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                acc[c][0] = pt_mfma(au[0], bu[c], acc[c][0]);
                acc[c][1] = pt_mfma(au[0], bm[c], acc[c][1]);
                acc[c][2] = pt_mfma(am[0], bu[c], acc[c][2]);
                acc[c][3] = pt_mfma(am[0], bm[c], acc[c][3]);
            }
        }
    }

    // register r of a lane is element (row (r & 3) + 8 (r >> 2) + 4 h, column i) of the tile
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int k = gb * PT_GROUP + 4 * i + fb[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = ga * PT_GROUP + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + rt;
            if (j >= J || k >= J) continue;
            const int uu = acc[c][0][r], um = acc[c][1][r], mu = acc[c][2][r], mm = acc[c][3][r];
            const int v10 = um - uu, v01 = mu - uu, v00 = mm - um - mu + uu;
            const int64_t jk = (int64_t)j * J + k;
            if (uu) atomicAdd(n11 + jk, uu);
            if (v10) atomicAdd(n10 + jk, v10);
            if (v01) atomicAdd(n01 + jk, v01);
            if (v00) atomicAdd(n00 + jk, v00);
        }
    }
}

// the blocks below the diagonal of item groups, which no workgroup computes, from their transpose partners: n11 and n00
// mirrored, n10[j][k] = n01[k][j] and n01[j][k] = n10[k][j] (the writes run along a row and coalesce)
__global__ __launch_bounds__(256) void k_pair_tables_mirror(int J, int32_t* __restrict__ n11, int32_t* __restrict__ n10,
                                                            int32_t* __restrict__ n01, int32_t* __restrict__ n00) {
    const int64_t total = (int64_t)J * J;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx / J), k = (int)(idx - (int64_t)j * J);
        if (j / PT_GROUP <= k / PT_GROUP) continue;
        const int64_t kj = (int64_t)k * J + j;
        n11[idx] = n11[kj];
        n00[idx] = n00[kj];
        n10[idx] = n01[kj];
        n01[idx] = n10[kj];
    }
}
