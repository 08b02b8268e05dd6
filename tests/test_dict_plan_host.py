"""dict_plan (csrc/dict_plan.h), the decision of dictionary_update, on a CPU over the cross product of its facts.

The header is plain C++: tests/dict_plan_dump.cpp includes it alone, is built here with the host compiler, reads
cases from stdin and prints the plan's fields.  The plan is held against two readings that are not the header:

* path_model (tests/test_spg_step_host.py, imported unchanged): the first aa_spg_path entry and the line-search
  entries it gives have to be what the plan's start and line_search fields say, in every case path_model has a
  word for -- forms data / linear / kernel (the implicit kernel is the kernel form), options fuse_finalize,
  setup_in_grad and pq_mfma (no knob of the plan: both values give the plan's fields), set-ups cold (the products
  of the previous update are not there), second (they and the Gram state are) and second_inputs (the same behind
  aa_set_dictionary_inputs), single fits (the restart slots record no path).
* a restatement of every other field, written from dictionary_update and spg_tail_needed (csrc/solver.hip) and
  side_available / launch_proj_side (csrc/kernels_tall.hip) as they stood before the plan existed, at commit
  aaf70f9; "solver.hip:N" and "kernels_tall.hip:N" below are lines of those files at that commit.

Cases: the cross product of the facts of DictPlanIn -- the four forms, max_iterations in 1, 2, 5, max_feval in
201, 202 and sixteen of its seventeen booleans -- less what the update's own checks exclude (neither valid Grams
nor overridden inputs) and mixed slots without slots, at the default knobs and at each single-knob deviation:
8 x 884 736 cases.  The fact cut from the product is alpha0_negative: the restatement shows alpha_first to be that
fact alone (solver.hip:444) and no other field to read it; it alternates with the case number instead, so both
values meet every value of every other fact.

Planted defect, run once against this file in a scratch copy of the header: max_feval < 202 moved to <= 202 fails
test_tail_and_rides on 1 792 cases (profiles/dict_plan_refactor.txt, section 3).
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_spg_step_host import path_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-factorization-case-studies_amd", "csrc")

KNOB_ORDER = ("fuse_finalize", "setup_in_grad", "grad_side", "spg_tail", "pack_comm", "proj_mode", "proj_res_side")
KNOB_DEFAULTS = dict(fuse_finalize=1, setup_in_grad=1, grad_side=1, spg_tail=0, pack_comm=1, proj_mode=0,
                     proj_res_side=1)
KNOBS = [dict()] + [{name: 1 - KNOB_DEFAULTS[name]} for name in KNOB_ORDER]
DATA, DATA_AS_KERNEL, KERNEL_MATRIX, IMPLICIT_KERNEL = range(4)               # DictForm
FORM_WORD = ("data", "linear", "kernel", "kernel")                            # ... as path_model calls them
MAX_ITERATIONS = (1, 2, 5)
MAX_FEVAL = (201, 202)
# the boolean facts, in the bit order of dict_plan_dump.cpp
FACTS = ("slots_aa", "slots_mixed", "multi", "x_feasible", "products_valid", "grams_valid", "ckz_valid",
         "dict_inputs_overridden", "stats", "cost_dst", "alpha0_negative", "weights_follow", "loop_update",
         "loop_judged", "max_iter_seen", "side_resources", "flags_operand")
CROSSED = tuple(name for name in FACTS if name != "alpha0_negative")
COLD, WARM, FAST_SETUP, FAST_IN_GRAD = range(4)                               # DictStart
START_WORD = ("cold", "warm", "fast:k_dict_setup", "fast:in_grad")
FUSED, WIDE_X2, TALL_X3 = range(3)                                            # DictLineSearch
SKIP_FLAGGED, SKIP_DENSE, MAIN, SIDE_WHOLE, SIDE_PROJ = range(5)              # DictTail
# the boolean fields of the plan, in the bit order of dict_plan_dump.cpp
BITS = ("data", "implicit", "project_start", "save_restore_P", "warm_slots_setup", "scale_by_n", "alpha_first",
        "record_cost", "ride_dir", "ride_grad", "ride_res", "ckct_done", "tail_skipped", "read_back_first",
        "read_back_last", "side_available")
N_FACTS = 884736


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(the knobs of every case as a dict of columns, its facts likewise, the plan's fields likewise)"""
    cxx = shutil.which("g++") or (os.path.exists("/opt/rocm/llvm/bin/clang++") and "/opt/rocm/llvm/bin/clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("dict_plan") / "dict_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "dict_plan_dump.cpp"), "-o", exe], check=True)
    grid = np.array(list(itertools.product(range(4), MAX_ITERATIONS, MAX_FEVAL, *[(0, 1)] * len(CROSSED))),
                    dtype=np.int64)
    f = {"form": grid[:, 0], "max_iterations": grid[:, 1], "max_feval": grid[:, 2]}
    f.update({name: grid[:, 3 + i] for i, name in enumerate(CROSSED)})
    # AA_REQUIRE of dictionary_update (solver.hip:363); slots_mixed() asks slots_aa itself (solver.hip:313)
    keep = ((f["grams_valid"] | f["dict_inputs_overridden"]) != 0) & (f["slots_mixed"] <= f["slots_aa"])
    f = {name: col[keep] for name, col in f.items()}
    assert len(f["form"]) == N_FACTS
    f["alpha0_negative"] = np.arange(N_FACTS) % 2
    mask = sum(f[name] << i for i, name in enumerate(FACTS))
    body = ["%d %d %d %d" % row for row in zip(f["form"].tolist(), f["max_iterations"].tolist(),
                                                f["max_feval"].tolist(), mask.tolist())]
    heads = [" ".join(str(dict(KNOB_DEFAULTS, **knobs)[name]) for name in KNOB_ORDER) + " " for knobs in KNOBS]
    text = "\n".join(head + line for head in heads for line in body)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    plans = np.fromstring(out, dtype=np.int64, sep=" ").reshape(len(KNOBS) * N_FACTS, 4)
    p = {"start": plans[:, 0], "line_search": plans[:, 1], "tail": plans[:, 2]}
    p.update({name: (plans[:, 3] >> i) & 1 for i, name in enumerate(BITS)})
    o = {name: np.repeat([dict(KNOB_DEFAULTS, **knobs)[name] for knobs in KNOBS], N_FACTS) for name in KNOB_ORDER}
    f = {name: np.tile(col, len(KNOBS)) != 0 if name in FACTS else np.tile(col, len(KNOBS)) for name, col in f.items()}
    return {name: col != 0 for name, col in o.items()}, f, p


def test_start_and_line_search_are_path_models(table):
    """The first path entry and the line-search entries, wherever path_model has a word for the case."""
    o, f, p = table
    warm = f["x_feasible"] & f["products_valid"]
    second = warm & f["grams_valid"] & f["ckz_valid"] & ~f["dict_inputs_overridden"]
    setup_of = {"cold": ~warm, "second": second, "second_inputs": warm & f["dict_inputs_overridden"]}
    compared = 0
    for form, fuse, in_grad, pq, (setup, at) in itertools.product(range(4), (0, 1), (0, 1), (0, 1), setup_of.items()):
        at = at & ~f["slots_aa"] & (f["form"] == form) & (o["fuse_finalize"] == fuse) & (o["setup_in_grad"] == in_grad)
        if not at.any():
            assert fuse + in_grad == 0           # no two knobs deviate at once
            continue
        path = path_model(FORM_WORD[form], 129, 33, 3, dict(fuse_finalize=fuse, setup_in_grad=in_grad, pq_mfma=pq),
                          setup, iterations=2)
        ls = path[2:-1][:len(path[2:-1]) // 2]
        assert path[2:-1] == ls + [path[1]] + ls and len(ls) == 2
        want = (FUSED if ls[1] == "k_linesearch_fin" else
                {"k_gram_wide<32>x2": WIDE_X2, "k_gram_tall<32>x3": TALL_X3}[ls[0]])
        assert ls[1] == ("k_linesearch_fin" if want == FUSED else "k_scalar_stage")
        assert (p["start"][at] == START_WORD.index(path[0])).all(), (form, fuse, in_grad, setup)
        assert (p["line_search"][at] == want).all(), (form, fuse, in_grad, setup)
        compared += int(at.sum()) if pq else 0
    # what path_model has no word for: the slots, and products without the C K Z of the Gram state
    rest = f["slots_aa"] | (warm & ~second & ~f["dict_inputs_overridden"])
    assert compared == int((~rest).sum()) == 2260992
    assert set(p["start"].tolist()) == {COLD, WARM, FAST_SETUP, FAST_IN_GRAD}
    assert set(p["line_search"].tolist()) == {FUSED, WIDE_X2, TALL_X3}


def _restated_tail_needed(o, f):
    """spg_tail_needed, solver.hip:347-354, clause by clause."""
    needed = o["spg_tail"] | f["stats"] | (f["max_iterations"] > 1)                               # :349
    needed |= (f["form"] >= KERNEL_MATRIX) | f["slots_aa"] | f["multi"]                            # :350
    needed |= ~f["loop_update"] | f["dict_inputs_overridden"]                                      # :351
    needed |= f["loop_judged"] & ((f["max_feval"] < 202) | ~f["max_iter_seen"])                    # :352
    return needed


def test_tail_and_rides(table):
    """Tail placement and the three rides against the update as it was written before the plan."""
    o, f, p = table
    data = f["form"] <= DATA_AS_KERNEL                                       # c->form == AA_FORM_DATA, solver.hip:369
    single_quiet = (f["max_iterations"] == 1) & ~f["stats"]
    # side_available, kernels_tall.hip:2598-2602
    side_available = (o["proj_res_side"] & f["side_resources"] & ~f["multi"] & ~o["proj_mode"] & o["fuse_finalize"])
    assert np.array_equal(p["side_available"] != 0, side_available)
    needed = _restated_tail_needed(o, f)
    skipped = data & ~needed                                                 # solver.hip:481,485
    grad_on_side = data & needed & o["grad_side"] & single_quiet & side_available          # solver.hip:511
    # solver.hip:529-536: the whole tail; else launch_proj_side, which asks side_available itself
    # (kernels_tall.hip:2634); else the main stream
    proj_side = ~skipped & ~grad_on_side & single_quiet & data & side_available
    want = np.select([skipped & f["flags_operand"], skipped, grad_on_side, proj_side],      # solver.hip:491-495
                     [SKIP_FLAGGED, SKIP_DENSE, SIDE_WHOLE, SIDE_PROJ], MAIN)
    bad = np.flatnonzero(p["tail"] != want)
    assert not len(bad), "%d cases disagree, the first at row %d" % (len(bad), bad[0])
    assert np.array_equal(p["tail_skipped"] != 0, skipped)
    assert set(want.tolist()) == {SKIP_FLAGGED, SKIP_DENSE, MAIN, SIDE_WHOLE, SIDE_PROJ}
    # the facts the issue of the plan names, each by itself: any of these keeps the tail ...
    for keeps in (f["stats"], f["max_iterations"] > 1, f["form"] >= KERNEL_MATRIX, f["slots_aa"], f["multi"],
                  o["spg_tail"], ~f["loop_update"], f["dict_inputs_overridden"]):
        assert keeps.any() and not p["tail_skipped"][keeps].any()
    # ... a judged update keeps it until MAX_ITER was seen, and always when max_feval < 202 ...
    judged = f["loop_judged"]
    assert not p["tail_skipped"][judged & (~f["max_iter_seen"] | (f["max_feval"] < 202))].any()
    quiet = ~(o["spg_tail"] | f["stats"] | (f["max_iterations"] > 1) | ~data | f["slots_aa"] | f["multi"] |
              ~f["loop_update"] | f["dict_inputs_overridden"])
    assert p["tail_skipped"][quiet & judged & f["max_iter_seen"] & (f["max_feval"] >= 202)].all()
    assert p["tail_skipped"][quiet & ~judged].all()
    # ... and a data matrix standing in for a kernel is the data form to this rule (c->form == AA_FORM_DATA)
    assert p["tail_skipped"][quiet & ~judged & (f["form"] == DATA_AS_KERNEL)].all()
    # the whole tail on the side stream only with grad_side, one iteration, no stats, an available side stream
    whole = p["tail"] == SIDE_WHOLE
    assert (o["grad_side"] & single_quiet & side_available)[whole].all()
    alone = p["tail"] == SIDE_PROJ
    assert (~o["grad_side"] & single_quiet & side_available)[alone].all()
    # rides, multi-rank: solver.hip:450, :514 (inside the data form's branch, :481), :525-527
    pack = f["multi"] & o["pack_comm"] & data & ~f["slots_aa"]
    assert np.array_equal(p["ride_dir"] != 0, pack)
    assert np.array_equal(p["ride_grad"] != 0, pack & ~o["proj_mode"] & o["fuse_finalize"])
    assert np.array_equal(p["ride_res"] != 0, pack & f["weights_follow"] & single_quiet & o["fuse_finalize"])
    assert p["ride_dir"].any() and p["ride_grad"].any() and p["ride_res"].any()
    assert not (p["tail_skipped"] & (p["ride_grad"] | p["ride_res"])).any()       # a skipped tail owes no ride


def test_remaining_fields(table):
    """Start-point projection, the slots' P, gradient scale, step length, cost, read-back and ckct_done."""
    o, f, p = table
    data = f["form"] <= DATA_AS_KERNEL
    warm = f["x_feasible"] & f["products_valid"]                                                   # solver.hip:388
    fused = data & o["fuse_finalize"]                                                              # :392
    fast = fused & warm & f["grams_valid"] & f["ckz_valid"] & ~f["dict_inputs_overridden"]         # :393
    in_grad = fast & o["setup_in_grad"] & ~f["slots_aa"]                                           # :395
    want_start = np.select([in_grad, fast, warm], [FAST_IN_GRAD, FAST_SETUP, WARM], COLD)         # :398-401
    assert np.array_equal(p["start"], want_start)      # (also where path_model has no word: slots, no C K Z)
    assert np.array_equal(p["data"] != 0, data)
    assert np.array_equal(p["implicit"] != 0, f["form"] == IMPLICIT_KERNEL)                        # c->kernel.kind, :417
    assert np.array_equal(p["project_start"] != 0, ~fast & ~f["x_feasible"])                       # :402,408
    assert np.array_equal(p["save_restore_P"] != 0, ~fast & ~warm & data & f["slots_mixed"])       # :409-414
    assert np.array_equal(p["warm_slots_setup"] != 0, ~fast & f["slots_mixed"])                    # :431
    assert np.array_equal(p["scale_by_n"] != 0, f["form"] == DATA)                                 # :378
    assert np.array_equal(p["alpha_first"] != 0, f["alpha0_negative"])                             # :444
    assert np.array_equal(p["line_search"], np.select([fused, data], [FUSED, WIDE_X2], TALL_X3))   # :452,455,467
    assert np.array_equal(p["record_cost"] != 0, fused & f["cost_dst"] & (f["max_iterations"] == 1))  # :455,458
    assert np.array_equal(p["read_back_first"] != 0, f["stats"] | (f["max_iterations"] > 1))       # :540, it = 0
    assert np.array_equal(p["read_back_last"] != 0, f["stats"])                                    # :540, the last
    assert np.array_equal(p["ckct_done"] != 0, fused)                                              # :559
    for name in BITS:
        assert p[name].any() and not p[name].all(), name
