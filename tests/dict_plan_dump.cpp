// Prints what dict_plan (csrc/dict_plan.h) decides, one line per case read from stdin (test_dict_plan_host.py).
// A case is 11 integers:
//   fuse_finalize setup_in_grad grad_side spg_tail pack_comm proj_mode proj_res_side
//   form max_iterations max_feval facts
// with facts the boolean members of DictPlanIn in the order of FACTS of the test, the first in bit 0; and its
// line 4 integers: start, line_search, tail, and the boolean fields of the plan in the order of BITS of the test.
#include <cstdio>

#include "dict_plan.h"

int main()
{
    long v[11];
    for (;;) {
        for (int i = 0; i < 11; ++i)
            if (std::scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        const aa::DictKnobs o{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6]};
        const long f = v[10];
        int b = 0;
        aa::DictPlanIn in{};
        in.form = (aa::DictForm)v[7];
        in.max_iterations = (int)v[8];
        in.max_feval = (int)v[9];
        in.slots_aa = (f >> b++) & 1;
        in.slots_mixed = (f >> b++) & 1;
        in.multi = (f >> b++) & 1;
        in.x_feasible = (f >> b++) & 1;
        in.products_valid = (f >> b++) & 1;
        in.grams_valid = (f >> b++) & 1;
        in.ckz_valid = (f >> b++) & 1;
        in.dict_inputs_overridden = (f >> b++) & 1;
        in.stats = (f >> b++) & 1;
        in.cost_dst = (f >> b++) & 1;
        in.alpha0_negative = (f >> b++) & 1;
        in.weights_follow = (f >> b++) & 1;
        in.loop_update = (f >> b++) & 1;
        in.loop_judged = (f >> b++) & 1;
        in.max_iter_seen = (f >> b++) & 1;
        in.side_resources = (f >> b++) & 1;
        in.flags_operand = (f >> b++) & 1;
        const aa::DictPlan p = aa::dict_plan(o, in);
        const bool bits[] = {p.data, p.implicit, p.project_start, p.save_restore_P, p.warm_slots_setup, p.scale_by_n,
                             p.alpha_first, p.record_cost, p.ride_dir, p.ride_grad, p.ride_res, p.ckct_done,
                             p.tail_skipped(), p.read_back(0), p.read_back(p.max_iterations - 1),
                             aa::dict_side_available(o, in.side_resources, in.multi)};
        int out = 0;
        for (unsigned i = 0; i < sizeof(bits) / sizeof(bits[0]); ++i) out |= (int)bits[i] << i;
        std::printf("%d %d %d %d\n", (int)p.start, (int)p.line_search, (int)p.tail, out);
    }
}
