// Prints GbcPlan (vipsy_amd/csrc/grid_plan.h), the launch plan of vx_grid_bifactor_counts, over a fixed sweep as one JSON document:
// {"sweep": {...}, "plans": [[nb, KC, Gg, n_tl, n_gpairs, n_units, units_per_chunk, n_chunks, off_ms, off_mass, slab_len], ...],
// "groups": [[chunks of the testlets ..., -> groups], ...]}.  Host only: the one include is the header
// (tests/test_bifactor_em_host.py compiles it under AddressSanitizer + UBSan and holds it to the plan said again in Python).
#include "grid_plan.h"

#include <cstdio>
#include <cstdlib>

static const int64_t NBS[] = {1, 63, 64, 65, 255, 256, 257, 512, 513, 1100, 4096, 167680, 262144, (int64_t)1 << 40};
static const int GGS[] = {2, 3, 21, 41, 61, 128, 255, 256};
static const int KCS[][2] = {{1, 1}, {3, 2}, {5, 3}, {100, 100}, {64, 3}, {1024, 1024}, {512, 1}};      // (KC, n_tl)

int main() {
    printf("{\"plans\":[");
    bool first = true;
    for (int64_t nb : NBS)
        for (int Gg : GGS)
            for (const auto& k : KCS) {
                const GbcPlan p = gbc_plan(nb, k[0], Gg, k[1]);
                const GbcPlan q = gbc_plan(nb, 1, Gg, 1);
                if (p.n_units != q.n_units || p.units_per_chunk != q.units_per_chunk || p.n_chunks != q.n_chunks) {
                    fprintf(stderr, "the cut of the persons depends on the layout\n");
                    return 1;
                }
                if (p.n_chunks < 1 || p.units_per_chunk % GBC_WAVES || (p.n_chunks - 1) * p.units_per_chunk >= p.n_units ||
                    p.n_chunks * p.units_per_chunk < p.n_units) {
                    fprintf(stderr, "a person chunk is empty, or units are left over\n");
                    return 1;
                }
                printf("%s[%lld,%d,%d,%d,%d,%lld,%lld,%lld,%lld,%lld,%lld]", first ? "" : ",", (long long)nb, k[0], Gg, k[1], p.n_gpairs,
                       (long long)p.n_units, (long long)p.units_per_chunk, (long long)p.n_chunks, (long long)p.off_ms,
                       (long long)p.off_mass, (long long)p.slab_len);
                first = false;
            }
    printf("],\"groups\":[");
    const int32_t layouts[][6] = {{0, 1, -1}, {0, 1, 3, -1}, {0, 2, 3, 4, 5, -1}, {0, 5, 10, 11, -1}, {0, 1024, -1}};
    first = true;
    for (const auto& tl : layouts) {
        int n = 0;
        while (tl[n + 1] >= 0) ++n;
        printf("%s[", first ? "" : ",");
        for (int t = 0; t <= n; ++t) printf("%d,", tl[t]);
        printf("%d]", gbc_groups(tl, n));
        first = false;
    }
    printf("]}\n");
    return 0;
}
