// The launch and workspace plans of the grid family (vx_grid_*, vx_sumscore_*): plain int64 arithmetic, no HIP header, so that
// the host entries (vx_abi.hip), the kernels that share a helper, and a CPU-only program (tests/helpers/grid_plans.cpp,
// tests/test_grid_plans_host.py) read the SAME lines.  The plans decide the order of every sum the family promises to repeat bit
// for bit, and none of them looks at the device: the same call gives the same plan everywhere.  The constants here are the ones a
// plan needs; what only pins a kernel's own geometry stays in its k_*.hip.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VX_PLAN_HD __host__ __device__
#else
#define VX_PLAN_HD
#endif

// ---- tiles: 32 x 32, as v_mfma_f32_32x32x16_f16 accumulates them ---------------------------------------------------------
#define GI_TILE 1024                    // floats of a 32 x 32 tile
#define GRID_SLAB 256                   // a slab's persons are a multiple of this (8 units of 32)

VX_PLAN_HD inline int gp_nt(int G) { return (G + 31) / 32; }                      // node tiles
VX_PLAN_HD inline int gi_pt(int P) { return (P + 32) / 32; }                      // tiles of P + 1 columns (k_grid_info.hip)
VX_PLAN_HD inline int pp_jt(int J) { return (J + 31) / 32; }                      // item tiles (k_grid_pairs.hip)
// the upper triangle of T x T tiles, row by row
VX_PLAN_HD inline int64_t gi_pairs(int T) { return (int64_t)T * (T + 1) / 2; }
VX_PLAN_HD inline int64_t gi_pair_index(int T, int a, int b) { return (int64_t)a * T - (int64_t)a * (a - 1) / 2 + (b - a); }

// ---- SlabPlan ------------------------------------------------------------------------------------------------------------
// A call that sums cross products over persons takes them in slabs of a multiple of 256.  A fragment kernel leaves a slab's
// operands in the workspace, `unit_floats` a unit of 32 persons; a cross-product kernel (workgroup = a block of block_tiles x
// block_tiles tiles of the upper triangle x a chunk of units) leaves `pair_floats` a tile pair and chunk; the chunks are added in
// ascending order, then the slabs in person order.  The workspace: [fragments of a slab | chunk partials | their sum | running sum].
struct SlabPlan {
    int tiles, nbb;                     // tiles a side; workgroup blocks a side
    int64_t n_pairs, n_bp;              // tile pairs; workgroup blocks of the upper triangle
    int64_t slab_persons, n_chunks, units_per_chunk;
    int64_t tiles_len;                  // floats of one set of partial tiles: n_pairs * pair_floats
    int64_t off_part, off_red, off_acc, total;
};
inline int64_t slab_chunks_for(int64_t m256, int64_t n_bp, int64_t max_blocks) {
    const int64_t cap = max_blocks / n_bp > 1 ? max_blocks / n_bp : 1;
    return m256 < cap ? m256 : cap;
}
// floats for slabs of m256 * 256 persons in `chunks` chunks; the smallest workspace is one 256-person slab in one chunk
inline int64_t slab_need(int tiles, int64_t unit_floats, int64_t pair_floats, int64_t m256, int64_t chunks) {
    return m256 * 8 * unit_floats + (chunks + 2) * gi_pairs(tiles) * pair_floats;
}
inline int64_t slab_min_floats(int tiles, int64_t unit_floats, int64_t pair_floats) {
    return slab_need(tiles, unit_floats, pair_floats, 1, 1);
}
// ws_floats < 0: the preferred size (everything in one slab, as far as 512 MB go); otherwise at least slab_min_floats
inline SlabPlan slab_plan(int64_t nb, int tiles, int block_tiles, int64_t unit_floats, int64_t pair_floats, int64_t max_blocks,
                          int64_t ws_floats) {
    SlabPlan p;
    p.tiles = tiles;
    p.nbb = (tiles + block_tiles - 1) / block_tiles;
    p.n_pairs = gi_pairs(tiles);
    p.n_bp = (int64_t)p.nbb * (p.nbb + 1) / 2;
    p.tiles_len = p.n_pairs * pair_floats;
    int64_t m = (nb + GRID_SLAB - 1) / GRID_SLAB;
    if (ws_floats < 0) {
        const int64_t least = slab_min_floats(tiles, unit_floats, pair_floats);
        ws_floats = (int64_t)128 << 20;
        if (ws_floats < least) ws_floats = least;
    }
    const int64_t m_cap = (ws_floats - 3 * p.tiles_len) / (8 * unit_floats);      // with one chunk
    if (m > m_cap) m = m_cap;
    while (m > 1 && slab_need(tiles, unit_floats, pair_floats, m, slab_chunks_for(m, p.n_bp, max_blocks)) > ws_floats) --m;
    if (m < 1) m = 1;
    const int64_t chunks = slab_chunks_for(m, p.n_bp, max_blocks);
    const int64_t units = m * 8;
    p.slab_persons = m * GRID_SLAB;
    p.units_per_chunk = (units + chunks - 1) / chunks;
    p.n_chunks = (units + p.units_per_chunk - 1) / p.units_per_chunk;
    p.off_part = units * unit_floats;
    p.off_red = p.off_part + p.n_chunks * p.tiles_len;
    p.off_acc = p.off_red + p.tiles_len;
    p.total = p.off_acc + p.tiles_len;
    return p;
}

// vx_grid_info (k_grid_info.hip): P + 1 columns; a unit is a fragment pair a parameter tile, a tile pair one tile
#define GI_BT 4                         // parameter tiles a side of a workgroup's block in k_grid_xprod (one row a wave)
#define GI_MAX_BLOCKS 1024              // workgroups of a k_grid_xprod launch, about
inline SlabPlan gi_slab_plan(int64_t nb, int P, int64_t ws_floats) {
    return slab_plan(nb, gi_pt(P), GI_BT, (int64_t)gi_pt(P) * GI_TILE, GI_TILE, GI_MAX_BLOCKS, ws_floats);
}
inline int64_t gi_slab_min_floats(int P) { return slab_min_floats(gi_pt(P), (int64_t)gi_pt(P) * GI_TILE, GI_TILE); }

// vx_grid_pairs_* (k_grid_pairs.hip): J items; a unit is five fragments a k-step and item tile, a tile pair six tiles
#define PP_BT 2                         // item tiles a side of a workgroup's block in k_pair_xprod
#define PP_OPS 5                        // fragments a k-step: r head, r low, r^2 head, r^2 low, m
#define PP_ACC 6                        // accumulator tiles a tile pair: sp, n, s row, ss row, s column, ss column
#define PP_MAX_BLOCKS 2048              // workgroups of a k_pair_xprod launch, about
#define PP_UNIT_FLOATS(JT) ((int64_t)(JT) * 2 * PP_OPS * 64 * 4)      // floats of a unit's fragments
inline SlabPlan pp_slab_plan(int64_t nb, int J, int64_t ws_floats) {
    return slab_plan(nb, pp_jt(J), PP_BT, PP_UNIT_FLOATS(pp_jt(J)), (int64_t)PP_ACC * GI_TILE, PP_MAX_BLOCKS, ws_floats);
}
inline int64_t pp_slab_min_floats(int J) { return slab_min_floats(pp_jt(J), PP_UNIT_FLOATS(pp_jt(J)), (int64_t)PP_ACC * GI_TILE); }

// ---- GcPlan: vx_grid_counts (k_grid_counts.hip) --------------------------------------------------------------------------
#define GC_THREADS 512
#define GC_WAVES (GC_THREADS / 64)
#define GC_ROUND (32 * GC_WAVES)        // persons a workgroup takes at a time
#define GC_MAX_BLOCKS 256               // workgroups of a launch, about (the plan is the same on every device)
#define GC_MIN_ROUNDS 4                 // rounds a chunk has before the persons are split further

// The launch for (nb, J, G): template instance, grid and slab layout.
struct GcPlan {
    int it, ntg;                        // item tiles a wave (1, 2, 4), node tiles a workgroup (2; 1 beyond 512 items)
    int n_groups;                       // node groups
    int64_t rounds_per_chunk, n_chunks; // persons: chunks of rounds_per_chunk * GC_ROUND
    int64_t slab_len;                   // 2 J G + G
};
inline GcPlan gc_plan(int64_t nb, int J, int G) {
    GcPlan p;
    const int nit = (J + 31) / 32;
    p.it = nit <= GC_WAVES ? 1 : (nit <= 2 * GC_WAVES ? 2 : 4);
    p.ntg = p.it == 4 ? 1 : 2;
    p.n_groups = (gp_nt(G) + p.ntg - 1) / p.ntg;
    const int64_t rounds = (nb + GC_ROUND - 1) / GC_ROUND;
    int64_t chunks = (rounds + GC_MIN_ROUNDS - 1) / GC_MIN_ROUNDS;
    const int64_t cap = GC_MAX_BLOCKS / p.n_groups > 1 ? GC_MAX_BLOCKS / p.n_groups : 1;
    if (chunks > cap) chunks = cap;
    p.rounds_per_chunk = (rounds + chunks - 1) / chunks;
    p.n_chunks = (rounds + p.rounds_per_chunk - 1) / p.rounds_per_chunk;
    p.slab_len = 2 * (int64_t)J * G + G;
    return p;
}

// ---- GccPlan: vx_grid_counts_cond (k_grid_counts_cond.hip) ---------------------------------------------------------------
// The launch for (nb, n_seg, J, G): gc_plan(nb, J, G) for the template instance, the node groups and rounds_per_chunk.
// max_chunks bounds the chunks of ANY cut of nb persons into n_seg segments: a cut adds at most one round, and the rounding up
// of every segment's rounds to chunks at most one chunk a segment -- n_chunks(nb) + 2 (n_seg - 1), n_chunks(nb) for one segment.
struct GccPlan {
    GcPlan gc;
    int64_t max_chunks;
    int64_t tab_floats;                 // the table at the head of the workspace, in floats, padded to 16 bytes
};
inline GccPlan gcc_plan(int64_t nb, int n_seg, int J, int G) {
    GccPlan p;
    p.gc = gc_plan(nb, J, G);
    p.max_chunks = p.gc.n_chunks + 2 * (int64_t)(n_seg - 1);
    p.tab_floats = ((2 * ((int64_t)n_seg + 1) * 2 + 3) / 4) * 4;
    return p;
}
// chunks of a segment of `len` persons at `rounds_per_chunk` rounds a chunk at most
inline int64_t gcc_chunks(int64_t len, int64_t rounds_per_chunk) {
    const int64_t rounds = (len + GC_ROUND - 1) / GC_ROUND;
    return (rounds + rounds_per_chunk - 1) / rounds_per_chunk;
}
inline int64_t gcc_total_chunks(const int64_t* seg_start, int n_seg, int64_t rounds_per_chunk) {
    int64_t c = 0;
    for (int s = 0; s < n_seg; ++s) c += gcc_chunks(seg_start[s + 1] - seg_start[s], rounds_per_chunk);
    return c;
}
// The rounds a chunk may have in this cut: gc_plan's, raised (bisection: the total falls as it rises) until the chunks of all
// segments are no more than gc_plan's cap of workgroups -- many short segments would otherwise leave more workgroups than the
// chip holds at once, each with a short tail chunk.  One segment: gc_plan's value, its chunks being within the cap already.
inline int64_t gcc_rounds_per_chunk(const int64_t* seg_start, int n_seg, const GcPlan& gc) {
    const int64_t cap = GC_MAX_BLOCKS / gc.n_groups > 1 ? GC_MAX_BLOCKS / gc.n_groups : 1;
    int64_t lo = gc.rounds_per_chunk, hi = lo;
    if (gcc_total_chunks(seg_start, n_seg, lo) <= cap) return lo;
    for (int s = 0; s < n_seg; ++s) {
        const int64_t r = (seg_start[s + 1] - seg_start[s] + GC_ROUND - 1) / GC_ROUND;
        if (r > hi) hi = r;
    }
    while (hi - lo > 1) {                                                         // total(lo) > cap; hi: within it, or the most there is
        const int64_t mid = lo + (hi - lo) / 2;
        if (gcc_total_chunks(seg_start, n_seg, mid) <= cap) hi = mid; else lo = mid;
    }
    return hi;
}

// ---- GfPlan: vx_grid_fit_*, vx_grid_point_irt (k_grid_fit.hip, k_grid_point.hip) -----------------------------------------
#define GF_MAX_BLOCKS 1024              // workgroups of a launch at the most: 32 768 persons before a workgroup takes a second unit
#define GF_ITEM 4                       // item sums of vx_grid_fit_*: n, sr2, sw, sz2

// units of 32 persons in contiguous chunks, one chunk a workgroup
struct GfPlan { int64_t n_units, units_per_block, n_blocks; };
inline GfPlan gf_plan(int64_t nb) {
    GfPlan p;
    p.n_units = (nb + 31) / 32;
    const int64_t cap = p.n_units < GF_MAX_BLOCKS ? p.n_units : GF_MAX_BLOCKS;
    p.units_per_block = (p.n_units + cap - 1) / cap;
    p.n_blocks = (p.n_units + p.units_per_block - 1) / p.units_per_block;
    return p;
}
// the item partials of the workgroups: [n_blocks][GF_ITEM][J]
inline int64_t gf_ws_floats(int64_t nb, int J) { return gf_plan(nb).n_blocks * GF_ITEM * (int64_t)J; }

// ---- GbPlan: vx_grid_bifactor* (k_grid_bifactor.hip) ---------------------------------------------------------------------
#define GB_MAXGG 256                    // general nodes
#define GB_MAXGH 32                     // specific nodes: the rows of one tile
#define GB_MAXKC 1024                   // chunks of the testlet layout (1 024 items, were every one a testlet of its own)
#define GB_MAXD 4096                    // dimensions of the model the tables are built from
#define GB_MAX_IMAGE ((int64_t)512 << 20)       // bytes of the operand image

// [Gg][KC][4][64 lanes][8 fp16]
VX_PLAN_HD inline int64_t gb_image_bytes(int64_t Gg, int64_t KC) { return Gg * KC * 4 * 64 * 16; }
// what a call may be asked for, from its scalars alone (int64: no product of two of them can overflow)
inline bool gb_shape_ok(int64_t Gg, int64_t Gh, int64_t KC, int64_t n_tl, int64_t nb, int64_t max_persons) {
    return Gg >= 2 && Gg <= GB_MAXGG && Gh >= 1 && Gh <= GB_MAXGH && KC >= 1 && KC <= GB_MAXKC && n_tl >= 1 && n_tl <= KC &&
           nb >= 1 && nb <= max_persons && gb_image_bytes(Gg, KC) <= GB_MAX_IMAGE;
}
// the chunk starts of the testlets: 0 = tl_start[0] < tl_start[1] < .. < tl_start[n_tl] = KC (no empty testlet)
inline bool gb_testlets_ok(const int32_t* tl_start, int n_tl, int KC) {
    if (!tl_start || tl_start[0] != 0 || tl_start[n_tl] != KC) return false;
    for (int t = 0; t < n_tl; ++t)
        if (tl_start[t + 1] <= tl_start[t]) return false;
    return true;
}
// the workspace of specific = true: F, one float a person and general node, [units of 64 persons][Gg][64]
inline int64_t gb_ws_floats(int64_t nb, int64_t Gg) { return ((nb + 63) / 64) * Gg * 64; }

// ---- GbcPlan: vx_grid_bifactor_counts (k_grid_bifactor_counts.hip) -------------------------------------------------------
#define GBC_CG 2                        // chunks of a testlet a workgroup keeps accumulators for
#define GBC_NG 2                        // general nodes a workgroup (GB_NG)
#define GBC_WAVES 4                     // waves a workgroup (GP_WAVES), one unit of 64 persons each at a time
#define GBC_ROUND (64 * GBC_WAVES)      // persons a workgroup takes at a time
#define GBC_MIN_ROUNDS 2                // rounds a chunk has before the persons are split further
#define GBC_MAX_BLOCKS 256              // (node pairs x person chunks) of a launch, about; times the chunk groups = workgroups
#define GBC_MIN_CHUNKS 4                // person chunks the many node pairs of a fine general axis still leave

// The launch for (nb, KC, Gg, n_tl).  The cut of the persons looks at (nb, Gg) ALONE: a testlet's tables then do not depend on
// which other testlets the layout holds.  The slab: [n1 | n0: [16 KC][Gg][32] | mass_s: [n_tl][Gg][32] | mass: [Gg]].
struct GbcPlan {
    int n_gpairs;                       // pairs of general nodes
    int64_t n_units, units_per_chunk, n_chunks;      // units of 64 persons, in contiguous chunks of whole rounds
    int64_t off_ms, off_mass, slab_len;
};
inline GbcPlan gbc_plan(int64_t nb, int KC, int Gg, int n_tl) {
    GbcPlan p;
    p.n_gpairs = (Gg + GBC_NG - 1) / GBC_NG;
    p.n_units = (nb + 63) / 64;
    const int64_t rounds = (p.n_units + GBC_WAVES - 1) / GBC_WAVES;
    int64_t chunks = (rounds + GBC_MIN_ROUNDS - 1) / GBC_MIN_ROUNDS;
    const int64_t cap = GBC_MAX_BLOCKS / p.n_gpairs > GBC_MIN_CHUNKS ? GBC_MAX_BLOCKS / p.n_gpairs : GBC_MIN_CHUNKS;
    if (chunks > cap) chunks = cap;
    const int64_t rounds_per_chunk = (rounds + chunks - 1) / chunks;
    p.units_per_chunk = rounds_per_chunk * GBC_WAVES;
    p.n_chunks = (rounds + rounds_per_chunk - 1) / rounds_per_chunk;
    p.off_ms = (int64_t)2 * 16 * KC * Gg * 32;
    p.off_mass = p.off_ms + (int64_t)n_tl * Gg * 32;
    p.slab_len = p.off_mass + Gg;
    return p;
}
// chunk groups of a layout: every testlet in groups of GBC_CG chunks, the last one short
inline int gbc_groups(const int32_t* tl_start, int n_tl) {
    int n = 0;
    for (int t = 0; t < n_tl; ++t) n += (tl_start[t + 1] - tl_start[t] + GBC_CG - 1) / GBC_CG;
    return n;
}

// ---- SsPlan: vx_sumscore_model (k_sumscore.hip) --------------------------------------------------------------------------
#define SS_TARGET_WAVES 8192            // waves of the leave-one-out launch where the nodes allow: 8 a SIMD on 256 CUs

// registers a lane, and the nodes in contiguous chunks
struct SsPlan { int R, chunk, n_chunks; };
inline SsPlan ss_plan(int Js, int G) {
    SsPlan p;
    p.R = 1;
    while (64 * p.R < Js + 1) p.R *= 2;
    int want = (SS_TARGET_WAVES + Js - 1) / Js;
    if (want > G) want = G;
    p.chunk = (G + want - 1) / want;
    p.n_chunks = (G + p.chunk - 1) / p.chunk;
    return p;
}
// [e1 slabs: n_chunks x Js (Js + 1) | e0 slabs: the same]
inline int64_t ss_ws_floats(int Js, int G) { return 2 * (int64_t)ss_plan(Js, G).n_chunks * Js * (Js + 1); }

// ---- PtPlan: vx_pair_tables (k_pair_tables.hip) --------------------------------------------------------------------------
#define PT_GROUP 128                    // items of a panel: four tiles of 32, tile f of group g = the items 128 g + 4 i + f
#define PT_STAGE 128                    // persons staged between two barriers: four k-steps of 32
#define PT_MAXJ 1024
#define PT_TARGET_BLOCKS 256            // workgroups of a launch at the most: one of 512 threads a CU on 256 CUs, one round

// workgroup = (pair ga <= gb of item groups, chunk of stages); the chunks' integer sums meet in the tables by atomic adds, so
// the plan decides the launch only, never a bit of the result
struct PtPlan { int groups; int64_t n_bp, n_stages, stages_per_chunk, n_chunks; };
inline PtPlan pt_plan(int64_t nb, int J) {
    PtPlan p;
    p.groups = (J + PT_GROUP - 1) / PT_GROUP;
    p.n_bp = (int64_t)p.groups * (p.groups + 1) / 2;
    p.n_stages = (nb + PT_STAGE - 1) / PT_STAGE;
    int64_t chunks = PT_TARGET_BLOCKS / p.n_bp > 1 ? PT_TARGET_BLOCKS / p.n_bp : 1;
    if (chunks > p.n_stages) chunks = p.n_stages;
    p.stages_per_chunk = (p.n_stages + chunks - 1) / chunks;
    p.n_chunks = (p.n_stages + p.stages_per_chunk - 1) / p.stages_per_chunk;
    return p;
}
