// group_plan.h -- how the slot-major kernels (kernels_slots.hip: k_slot_sums, k_slot_rows) cut their work, decided
// apart from launching it: a pure function of the row labels.  Plain C++17, no HIP and no Ctx: a host compiler
// builds it alone (tests/group_plan_dump.cpp sweeps it on a CPU at the chunk edges).
//
// A "slot" is an integer label 0 .. G - 1 per row (day of year, six-hourly step of the year, pentad); -1 marks a
// row that is not counted.  A counting sort gives the row list by slot in CSR form -- rows[start[g] .. start[g + 1])
// are the rows of slot g in ascending row index -- and every slot's member list is cut, in order, into chunks of at
// most `chunk_rows` members: chunk c holds rows[chunk_begin[c] .. chunk_begin[c] + chunk_len[c]) of slot
// chunk_slot[c], and the chunks of slot g are chunk_first[g] .. chunk_first[g + 1] - 1, in ascending member order.
// A slot without counted rows has no chunk.  One chunk and one column tile are one work item of the kernels.
#pragma once

#include <vector>

namespace aa {

struct GroupPlan {
    int G = 0;
    long counted = 0;                   // rows with a label >= 0: rows.size()
    std::vector<int> start;             // G + 1
    std::vector<int> rows;              // counted
    std::vector<int> chunk_first;       // G + 1
    std::vector<int> chunk_slot, chunk_begin, chunk_len;   // one entry per chunk
    long chunks() const { return (long)chunk_slot.size(); }
};

// The first row whose label is outside [lowest, G), or -1: what the entry points refuse before they plan.
inline long group_plan_first_bad_label(const int *label, long n, int G, int lowest)
{
    for (long r = 0; r < n; ++r)
        if (label[r] < lowest || label[r] >= G) return r;
    return -1;
}

// label: n entries in [-1, G) (checked by the caller), n < 2^31, G >= 1, chunk_rows >= 1
inline GroupPlan group_plan(const int *label, long n, int G, int chunk_rows)
{
    GroupPlan pl;
    pl.G = G;
    pl.start.assign((size_t)G + 1, 0);
    for (long r = 0; r < n; ++r)
        if (label[r] >= 0) ++pl.start[(size_t)label[r] + 1];
    for (int g = 0; g < G; ++g) pl.start[(size_t)g + 1] += pl.start[(size_t)g];
    pl.counted = pl.start[(size_t)G];
    pl.rows.resize((size_t)pl.counted);
    std::vector<int> next(pl.start.begin(), pl.start.end() - 1);
    for (long r = 0; r < n; ++r)                       // ascending r: ascending row index inside a slot
        if (label[r] >= 0) pl.rows[(size_t)next[(size_t)label[r]]++] = (int)r;
    pl.chunk_first.assign((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) {
        const int b = pl.start[(size_t)g], e = pl.start[(size_t)g + 1];
        for (int at = b; at < e; at += chunk_rows) {
            pl.chunk_slot.push_back(g);
            pl.chunk_begin.push_back(at);
            pl.chunk_len.push_back(e - at < chunk_rows ? e - at : chunk_rows);
        }
        pl.chunk_first[(size_t)g + 1] = (int)pl.chunk_slot.size();
    }
    return pl;
}

}  // namespace aa
