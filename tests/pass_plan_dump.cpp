// Prints what pass_slabs, reduce_rows_plan and row_local_plan (csrc/pass_plan.h) decide, one line per case read
// from stdin (test_pass_plan_host.py).  A case is 12 integers:
//   row_local_variant row_local_acc64 row_local_split f64_mfma reduce_sparse reduce_sparse_max
//   f32 n_pad p_pad KP flag_buf time_gemm
// and its line the 24 integer fields named in FIELDS of the test, in that order, then the two names (which must fit
// the 48 bytes aa_pass_kernels keeps for each: exit status 2 if one does not).
#include <cstdio>

#include "pass_plan.h"

int main()
{
    long v[12];
    for (;;) {
        for (int i = 0; i < 12; ++i)
            if (std::scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        const aa::PassKnobs o{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5]};
        const bool f32 = v[6] != 0;
        const long n_pad = v[7], p_pad = v[8];
        const int KP = (int)v[9];
        const aa::PassSlabs s = aa::pass_slabs(f32, n_pad, p_pad);
        const aa::ReduceRowsPlan rr =
            aa::reduce_rows_plan(o, aa::ReduceRowsIn{f32, KP, p_pad, s.nslab, s.rows_per_slab, v[10] != 0, v[11] != 0});
        const aa::RowLocalPlan rl = aa::row_local_plan(o, f32, KP, n_pad, p_pad);
        char name[2][48];                               // the size of Ctx::pass_names
        const int len0 = aa::pass_name(rr, name[0], sizeof(name[0]));
        const int len1 = aa::pass_name(rl, name[1], sizeof(name[1]));
        if (len0 <= 0 || len1 <= 0 || len0 >= (int)sizeof(name[0]) || len1 >= (int)sizeof(name[1])) return 2;
        std::printf("%ld %ld %ld %d %d %d %ld %ld %ld %d %d %d %d %d %d %d %ld %ld %d %zu %d %d %d %zu %s %s\n",
                    s.colgroups, s.nslab, s.rows_per_slab, (int)rr.family, rr.targ, (int)rr.flagged, rr.grid_x,
                    rr.grid_y, rr.gather_limit, (int)rl.family, rl.targ, rl.tile, (int)rl.dbuf, (int)rl.acc64,
                    rl.variant, rl.W, rl.grid_x, rl.grid_y, rl.block, rl.lds, (int)rl.raise_lds, rl.nsplit, rl.chunk,
                    rl.partial_bytes, name[0], name[1]);
    }
}
