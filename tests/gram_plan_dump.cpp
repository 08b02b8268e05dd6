// gram_plan_dump -- csrc/gram_plan.h on a CPU (tests/test_pca_host.py builds this with the host compiler).
// stdin, one request per line:
//   "G side n p elem_size cus"  ->  "d tiles pairs K nsplit split_len partial_bytes g_ld"
//   "P tiles"                   ->  "ti:tj" for every pair index 0 .. gram_pairs(tiles) - 1, space separated
#include <cstdio>

#include "gram_plan.h"

int main()
{
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'G') {
            int side, es, cus;
            long n, p;
            if (std::scanf("%d %ld %ld %d %d", &side, &n, &p, &es, &cus) != 5) return 1;
            const aa::GramPlan g = aa::gram_plan(side, n, p, es, cus);
            std::printf("%ld %ld %ld %ld %ld %ld %ld %ld\n", g.d, g.tiles, g.pairs, g.K, g.nsplit, g.split_len,
                        g.partial_bytes, g.g_ld);
        } else if (kind == 'P') {
            long tiles;
            if (std::scanf("%ld", &tiles) != 1) return 1;
            for (long idx = 0; idx < aa::gram_pairs(tiles); ++idx) {
                long ti, tj;
                aa::gram_pair_tile(idx, tiles, &ti, &tj);
                std::printf("%ld:%ld ", ti, tj);
            }
            std::printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
