// Prints every field of every plan of vipsy_amd/csrc/grid_plan.h over a fixed sweep as one JSON document
// (tests/test_grid_plans_host.py compares it with tests/golden/grid_plans.json).  Host only: the one include is the header.
// Rows carry no inputs where the sweep lists give them: the nesting is the order of the lists under "sweep".
#include "grid_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static const int64_t NBS[] = {1, 255, 256, 257, 549, 4096, 33024, 1000000, (int64_t)1 << 24};
static const int INFO_P[] = {1, 31, 32, 74, 1000, 4096};
static const int PAIRS_J[] = {1, 32, 33, 37, 500, 1024};
static const int GC_J[] = {1, 37, 256, 257, 512, 513, 1024};
static const int GC_G[] = {1, 32, 61, 512, 1024};
static const int GC_SEG[] = {1, 2, 7, 4096};
static const int64_t GF_NBS[] = {1, 255, 256, 257, 549, 4096, 33024, 1000000, (int64_t)1 << 24, 32 * 1024, 32 * 1024 + 1};
static const int SS_JS[] = {1, 2, 37, 1023};
static const int SS_G[] = {1, 61, 1024};

template <typename T, size_t N>
static void list(const char* name, const T (&v)[N], const char* end) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < N; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]%s", end);
}

// one shape of a slab plan: [shape, tiles, nbb, n_pairs, n_bp, tiles_len, min_floats, two, [rows: nb x ws_floats]], `two` the exact
// need at two 256-person granules; a row is [slab_persons, n_chunks, units_per_chunk, off_part, off_red, off_acc, total] and its
// ws_floats is, in this order: -1, min_floats, min_floats + 1, two, halfway between min_floats and the preferred size, the preferred
// size (the total that -1 gives)
template <typename Plan, typename Min>
static void slab_shape(int shape, int64_t max_blocks, Plan plan, Min min_floats, bool first) {
    const int64_t least = min_floats(shape);
    const SlabPlan s = plan(1, shape, least);
    const int64_t cap = max_blocks / s.n_bp > 1 ? max_blocks / s.n_bp : 1;
    const int64_t two = 2 * s.off_part + ((cap < 2 ? cap : 2) + 2) * s.tiles_len;
    printf("%s[%d,%d,%d,%lld,%lld,%lld,%lld,%lld,[", first ? "" : ",", shape, s.tiles, s.nbb, (long long)s.n_pairs, (long long)s.n_bp,
           (long long)s.tiles_len, (long long)least, (long long)two);
    bool first_row = true;
    for (int64_t nb : NBS) {
        const int64_t pref = plan(nb, shape, -1).total;
        const int64_t wss[] = {-1, least, least + 1, two, least + (pref - least) / 2, pref};
        for (int64_t ws : wss) {
            const SlabPlan p = plan(nb, shape, ws);
            printf("%s[%lld,%lld,%lld,%lld,%lld,%lld,%lld]", first_row ? "" : ",", (long long)p.slab_persons, (long long)p.n_chunks,
                   (long long)p.units_per_chunk, (long long)p.off_part, (long long)p.off_red, (long long)p.off_acc, (long long)p.total);
            first_row = false;
            if (p.tiles != s.tiles || p.nbb != s.nbb || p.n_pairs != s.n_pairs || p.n_bp != s.n_bp || p.tiles_len != s.tiles_len) {
                fprintf(stderr, "the tile fields of a slab plan depend on nb or ws\n");
                exit(1);
            }
        }
    }
    printf("]]");
}

// the three cuts of nb persons into n_seg segments: all in the first; equal; 1-person segments beside one long one
static void cut(int kind, int64_t nb, int n_seg, std::vector<int64_t>& st) {
    st.assign((size_t)n_seg + 1, nb);
    st[0] = 0;
    if (kind == 1)
        for (int s = 1; s < n_seg; ++s) st[s] = nb * s / n_seg;
    if (kind == 2) {
        const int64_t ones = n_seg - 1 < nb - 1 ? n_seg - 1 : nb - 1;
        for (int s = 1; s < n_seg; ++s) st[s] = s <= ones ? s : nb;
    }
}

int main() {
    printf("{\"sweep\":{");
    list("nb", NBS, ",");
    list("info_P", INFO_P, ",");
    list("pairs_J", PAIRS_J, ",");
    list("gc_J", GC_J, ",");
    list("gc_G", GC_G, ",");
    list("gcc_n_seg", GC_SEG, ",");
    list("gf_nb", GF_NBS, ",");
    list("ss_Js", SS_JS, ",");
    list("ss_G", SS_G, "},\n");

    printf("\"slab_info\":[");
    for (size_t i = 0; i < sizeof(INFO_P) / sizeof(int); ++i)
        slab_shape(INFO_P[i], GI_MAX_BLOCKS, gi_slab_plan, gi_slab_min_floats, i == 0);
    printf("],\n\"slab_pairs\":[");
    for (size_t i = 0; i < sizeof(PAIRS_J) / sizeof(int); ++i)
        slab_shape(PAIRS_J[i], PP_MAX_BLOCKS, pp_slab_plan, pp_slab_min_floats, i == 0);

    // gcc_tab_floats[n_seg]: GccPlan::tab_floats, which the loop below holds to depend on n_seg alone
    printf("],\n\"gcc_tab_floats\":[");
    for (size_t k = 0; k < sizeof(GC_SEG) / sizeof(int); ++k) printf("%s%lld", k ? "," : "", (long long)gcc_plan(1, GC_SEG[k], 1, 1).tab_floats);

    // gc[J][G][nb] = [it, ntg, n_groups, rounds_per_chunk, n_chunks, slab_len, [per n_seg: max_chunks, then gcc_rounds_per_chunk and
    //                 gcc_total_chunks of each of the three cuts (of the one cut there is where n_seg = 1)]]
    printf("],\n\"gc\":[");
    std::vector<int64_t> st;
    for (size_t j = 0; j < sizeof(GC_J) / sizeof(int); ++j)
        for (size_t g = 0; g < sizeof(GC_G) / sizeof(int); ++g)
            for (size_t n = 0; n < sizeof(NBS) / sizeof(int64_t); ++n) {
                const int J = GC_J[j], G = GC_G[g];
                const int64_t nb = NBS[n];
                const GcPlan p = gc_plan(nb, J, G);
                printf("%s[%d,%d,%d,%lld,%lld,%lld,[", j + g + n ? "," : "", p.it, p.ntg, p.n_groups, (long long)p.rounds_per_chunk,
                       (long long)p.n_chunks, (long long)p.slab_len);
                for (size_t k = 0; k < sizeof(GC_SEG) / sizeof(int); ++k) {
                    const int n_seg = GC_SEG[k];
                    const GccPlan c = gcc_plan(nb, n_seg, J, G);
                    if (c.gc.it != p.it || c.gc.ntg != p.ntg || c.gc.n_groups != p.n_groups || c.gc.rounds_per_chunk != p.rounds_per_chunk ||
                        c.gc.n_chunks != p.n_chunks || c.gc.slab_len != p.slab_len || c.tab_floats != gcc_plan(1, n_seg, 1, 1).tab_floats) {
                        fprintf(stderr, "gcc_plan's gc is not gc_plan, or tab_floats depends on more than n_seg\n");
                        return 1;
                    }
                    printf("%s%lld", k ? "," : "", (long long)c.max_chunks);
                    for (int kind = 0; kind < (n_seg == 1 ? 1 : 3); ++kind) {
                        cut(kind, nb, n_seg, st);
                        const int64_t rpc = gcc_rounds_per_chunk(st.data(), n_seg, c.gc);
                        printf(",%lld,%lld", (long long)rpc, (long long)gcc_total_chunks(st.data(), n_seg, rpc));
                    }
                }
                printf("]]");
            }

    // gf[nb] = [n_units, units_per_block, n_blocks, gf_ws_floats(nb, 37)]
    printf("],\n\"gf\":[");
    for (size_t n = 0; n < sizeof(GF_NBS) / sizeof(int64_t); ++n) {
        const GfPlan p = gf_plan(GF_NBS[n]);
        printf("%s[%lld,%lld,%lld,%lld]", n ? "," : "", (long long)p.n_units, (long long)p.units_per_block, (long long)p.n_blocks,
               (long long)gf_ws_floats(GF_NBS[n], 37));
    }

    // ss[Js][G] = [R, chunk, n_chunks, ss_ws_floats]
    printf("],\n\"ss\":[");
    for (size_t j = 0; j < sizeof(SS_JS) / sizeof(int); ++j)
        for (size_t g = 0; g < sizeof(SS_G) / sizeof(int); ++g) {
            const SsPlan p = ss_plan(SS_JS[j], SS_G[g]);
            printf("%s[%d,%d,%d,%lld]", j + g ? "," : "", p.R, p.chunk, p.n_chunks, (long long)ss_ws_floats(SS_JS[j], SS_G[g]));
        }
    printf("]}\n");
    return 0;
}
