// Prints what group_plan (csrc/group_plan.h) decides for the cases read from stdin (test_calendar_host.py).  A case
// is "G C n" followed by n labels in [-1, G); its output is five lines of integers:
//   first-bad-label(lowest -1) first-bad-label(lowest 0) counted chunks
//   start[0 .. G]
//   rows[0 .. counted)
//   chunk_first[0 .. G]
//   slot begin len   of every chunk, in order
// (a case with a label outside [-1, G) prints its first line with "0 0" and four empty lines: it is not planned).
// A stand-alone program, so the test builds it with the address and undefined-behaviour sanitizers where the host
// compiler links them.
#include <cstdio>
#include <vector>

#include "group_plan.h"

static void line(const std::vector<int> &v)
{
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %d" : "%d", v[i]);
    std::printf("\n");
}

int main()
{
    for (;;) {
        int G = 0, C = 0;
        long n = 0;
        if (std::scanf("%d", &G) != 1) return 0;
        if (std::scanf("%d %ld", &C, &n) != 2) return 1;
        std::vector<int> label((size_t)n);
        for (long r = 0; r < n; ++r)
            if (std::scanf("%d", &label[(size_t)r]) != 1) return 1;
        const long bad = aa::group_plan_first_bad_label(label.data(), n, G, -1);
        if (bad >= 0) {                                 // what the entry points refuse is not planned
            std::printf("%ld %ld 0 0\n\n\n\n\n", bad, aa::group_plan_first_bad_label(label.data(), n, G, 0));
            continue;
        }
        const aa::GroupPlan pl = aa::group_plan(label.data(), n, G, C);
        std::printf("%ld %ld %ld %ld\n", bad, aa::group_plan_first_bad_label(label.data(), n, G, 0), pl.counted,
                    pl.chunks());
        line(pl.start);
        line(pl.rows);
        line(pl.chunk_first);
        std::vector<int> flat;
        for (long c = 0; c < pl.chunks(); ++c) {
            flat.push_back(pl.chunk_slot[(size_t)c]);
            flat.push_back(pl.chunk_begin[(size_t)c]);
            flat.push_back(pl.chunk_len[(size_t)c]);
        }
        line(flat);
    }
}
