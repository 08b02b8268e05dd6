// Prints what qp_plan (csrc/qp_plan.h) decides, one line per case read from stdin (test_qp_plan_host.py).
// A case is 18 integers:
//   mode pass_cap quad_cap live quad_lazy fused_order wave_lazy overlap_tail sort
//   n k memory max_iterations resident own_iters iters_valid perm_ready defer
// and its line the 17 fields named in FIELDS of the test, in that order.
#include <cstdio>

#include "qp_plan.h"

int main()
{
    long v[18];
    for (;;) {
        for (int i = 0; i < 18; ++i)
            if (std::scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        const aa::QpKnobs o{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8]};
        aa::QpPlanIn in{};
        in.n = v[9];
        in.k = (int)v[10];
        in.memory = (int)v[11];
        in.max_iterations = (int)v[12];
        in.host_hessian = !v[13];
        in.own_iters = v[14] != 0;
        in.iters_valid = v[15] != 0;
        in.perm_ready = v[16] != 0;
        in.defer_possible = v[17] != 0;
        in.live_stream = true;
        const aa::QpPlan p = aa::qp_plan(o, in);
        std::printf("%d %d %d %d %d %d %d %d %ld %ld %d %d %d %d %d %d %d\n", (int)p.mapping, p.KQ, p.KW, p.sel,
                    (int)p.mem1, (int)p.full, (int)p.quad_lazy, p.cap, p.grid, p.max_trips,
                    (int)p.order, (int)p.sort_hist, p.setup_order, (int)p.tail, (int)p.tail_ord, p.order_blocks,
                    p.park_at);
    }
}
