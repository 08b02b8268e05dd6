"""qp_plan (csrc/qp_plan.h), the decision of launch_qp, against launch_model on a CPU at every edge of the dispatch.

The header is plain C++: tests/qp_plan_dump.cpp includes it alone, is built here with the host compiler, reads
cases from stdin and prints the plan's fields.  Two readings of the launcher then have to agree case by case, with
no GPU: launch_model (tests/test_gpu_qp_kernels.py, imported unchanged), which gives the string launch_qp records,
and the plan, from whose fields the same string is put together here -- the mapping and its template arguments, the
cap, whether a continuation follows, whether it is k_qp_wave_ord, whether it parks at 96 with a second one behind.

Cases: the full cross product of the edge values N x K x MEMORY x MAX_ITERATIONS x (resident, order_list, defer)
at the default knobs, each qp_mode, each single-knob deviation and three cap pairs; qp_live = 0 throughout
(launch_model does not model it).  What launch_model has no word for -- the sample order, the grids, the watchdog
trip count, the set-up kernel's order argument -- is held against formulas written here from the launcher as it
was before the plan existed.  The cases with the context's own pass-count list run in all four states of (list
valid, permutation prefetched), which must not change the string.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_qp_kernels import DEFAULTS, QP_TAIL_CAP, launch_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-factorization-case-studies_amd", "csrc")

N = (1, 16, 4096, 4097, 65535, 65536, 262144, 262145)
K = (1, 4, 5, 16, 17, 32, 33, 64)
MEMORY = (1, 2, 8, 9, 16, 17, 32)
MAX_ITERATIONS = (0, 1, 2, 3, 4, 5, 24, 25, 32, 33, 96, 97, 1000)
CONTEXT = [(r, o, d) for r, o in ((0, 0), (1, 0), (1, 1)) for d in (0, 1)]      # (resident, order_list, defer)
KNOBS = ([dict()] + [dict(qp_mode=m) for m in range(5)] +
         [dict(qp_quad_lazy=1), dict(qp_wave_lazy=0), dict(qp_fused_order=0), dict(qp_sort=0), dict(qp_overlap_tail=1)] +
         [dict(qp_pass_cap=c, qp_quad_cap=c) for c in (1, 5, 200)])
N_CASES = len(KNOBS) * len(N) * len(K) * len(MEMORY) * len(MAX_ITERATIONS) * len(CONTEXT)
# a case as qp_plan_dump.cpp reads it: the knobs in this order, then n, k, memory, max_iterations, resident,
# order_list, list valid, permutation prefetched, defer; and the line it prints
KNOB_ORDER = ("qp_mode", "qp_pass_cap", "qp_quad_cap", "qp_live", "qp_quad_lazy", "qp_fused_order", "qp_wave_lazy",
              "qp_overlap_tail", "qp_sort")
FIELDS = ("mapping", "KQ", "KW", "sel", "mem1", "full", "quad_lazy", "cap", "grid", "max_trips", "order",
          "sort_hist", "setup_order", "tail", "tail_ord", "order_blocks", "park_at")
PROJECT, ROW, QUAD, WAVE_ONLY, LANE = range(5)                    # QpMap
NO_ORDER, SORT_NOW, PREFETCHED, FORMS_NEXT = range(4)             # QpSampleOrder
NO_TAIL, MAIN, DEFERRED, TWO_STAGE, LIVE = range(5)               # QpTail


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(knob index of each case, the cases [.][18], the plans as a dict of int64 columns, and for each case the
    index of the case that differs from it at most in (valid, ready) and has both set)"""
    cxx = shutil.which("g++") or (os.path.exists("/opt/rocm/llvm/bin/clang++") and "/opt/rocm/llvm/bin/clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("qp_plan") / "qp_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "qp_plan_dump.cpp"), "-o", exe], check=True)
    rows, knob_of, base_of = [], [], []
    for ki, knobs in enumerate(KNOBS):
        o = dict(DEFAULTS, qp_live=0, **knobs)
        head = tuple(o[name] for name in KNOB_ORDER)
        for n, k, memory, it, (res, own, defer) in itertools.product(N, K, MEMORY, MAX_ITERATIONS, CONTEXT):
            base = len(rows)
            for valid, ready in ((1, 1), (0, 0), (1, 0), (0, 1)) if own else ((1, 1),):
                rows.append(head + (n, k, memory, it, res, own, valid, ready, defer))
                knob_of.append(ki)
                base_of.append(base)
    text = "\n".join(" ".join(map(str, c)) for c in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    plans = np.fromstring(out, dtype=np.int64, sep=" ").reshape(len(rows), len(FIELDS))
    return knob_of, rows, {name: plans[:, i] for i, name in enumerate(FIELDS)}, np.array(base_of)


def _name(p, i, lazy):
    """The string launch_qp records, from row i of the plan's fields; lazy: the qp_wave_lazy knob, which
    launch_wave_tail reads itself."""
    wave = "k_qp_wave<32,1,%d>" % lazy
    mapping, tail = p["mapping"][i], p["tail"][i]
    if mapping == PROJECT:
        return "k_qp_project_only<%d>" % p["KQ"][i]
    if mapping == ROW:
        return "k_qp_row<%d>" % p["sel"][i]
    if mapping == WAVE_ONLY:
        return "k_qp_wave<%d,%d,1>" % (p["KW"][i], p["mem1"][i])
    if mapping == LANE:
        assert tail in (NO_TAIL, MAIN, DEFERRED) and not p["tail_ord"][i]
        return "k_qp<%d,%d>:cap=%d" % (p["KQ"][i], p["full"][i], p["cap"][i]) + (";" + wave if tail != NO_TAIL else "")
    assert mapping == QUAD and tail != LIVE
    first = "k_qp_quad_w3<%d,%d,%d>:cap=%d" % (p["sel"][i], p["mem1"][i], p["quad_lazy"][i], p["cap"][i])
    cont = "k_qp_wave_ord<%d>" % lazy if p["tail_ord"][i] else wave
    if tail == NO_TAIL:
        assert not p["tail_ord"][i]
        return first
    if tail == TWO_STAGE:
        return "%s;%s:park=%d;%s" % (first, cont, p["park_at"][i], wave)
    assert p["park_at"][i] == 1 << 30
    return first + ";" + cont


def test_plan_agrees_with_launch_model(table):
    """Every case of the cross product, in every state of the context's list: the plan's string is launch_model's."""
    knob_of, rows, p, base_of = table
    # (valid, ready) change none of the fields the string is made of: one comparison for the four states
    for name in ("mapping", "KQ", "KW", "sel", "mem1", "full", "quad_lazy", "cap", "tail", "tail_ord", "park_at"):
        assert np.array_equal(p[name], p[name][base_of]), name
    p = {name: col.tolist() for name, col in p.items()}
    bad, compared = [], 0
    for i in np.flatnonzero(base_of == np.arange(len(rows))).tolist():
        ki, (n, k, memory, it, res, own, _, _, defer) = knob_of[i], rows[i][9:]
        want = launch_model(KNOBS[ki], n, k, max_iterations=it, memory=memory, resident=bool(res),
                            order_list=bool(own), defer=bool(defer))
        got = _name(p, i, rows[i][6])
        compared += 1
        if got != want:
            bad.append((KNOBS[ki], rows[i][9:], got, want))
    assert not bad, "%d cases disagree, the first: %r" % (len(bad), bad[:5])
    assert compared == N_CASES == 489216 and len(rows) == N_CASES * 2
    # a two-stage tail parks at QP_TAIL_CAP and nowhere else
    assert {p["park_at"][i] for i in range(len(rows)) if p["tail"][i] == TWO_STAGE} == {QP_TAIL_CAP}


def test_fields_launch_model_has_no_word_for(table):
    """Sample order, set-up argument, grids and the watchdog against formulas from the launcher before the plan."""
    _, rows, p, _ = table
    c = np.array(rows, dtype=np.int64)
    (mode, _, _, live, _, fused_knob, _, overlap, sort, n, k, memory, it, res, own, valid, ready, defer) = c.T
    assert not live.any()
    KQ = np.select([k <= 4, k <= 8, k <= 16, k <= 32], [4, 8, 16, 32], 64)
    big_mem = memory > 8
    row = (KQ <= 32) & (mode == 3) & (memory <= 16)
    quad = ~big_mem & (KQ <= 32) & ((mode == 4) | ((mode == 0) & (it > 4)))
    wave_only = ~row & ~quad & (big_mem | (KQ > 32) | (mode == 1) | (mode == 3))
    mapping = np.select([it <= 0, row, quad, wave_only], [PROJECT, ROW, QUAD, WAVE_ONLY], LANE)
    assert np.array_equal(p["mapping"], mapping)
    cap = p["cap"]                                       # (held against launch_model above)
    defer_ok = (defer != 0) & (overlap != 0) & (KQ <= 32)
    two_stage = defer_ok & (QP_TAIL_CAP > cap) & (QP_TAIL_CAP < it)
    fused = ((fused_knob != 0) & (sort != 0) & (mapping == QUAD) & (res != 0) & (memory <= 1) & (~defer_ok | two_stage) &
             (cap < it) & (it > 2) & (n > 4096) & (n <= 256 * 1024) & (own != 0))
    will_sort = (sort != 0) & (it > 2) & (n > 4096) & ~wave_only & (own != 0) & (valid != 0)
    sort_now = will_sort & ~((mapping == QUAD) & fused)
    prefetched = fused & (ready != 0)
    assert np.array_equal(p["order"] == SORT_NOW, sort_now)
    assert np.array_equal(p["order"] == PREFETCHED, prefetched)
    assert np.array_equal(p["order"] == FORMS_NEXT, fused & ~prefetched)
    assert np.array_equal(p["tail_ord"] != 0, fused)
    assert np.array_equal(p["sort_hist"] != 0, (res != 0) & (will_sort | fused))
    order_blocks = (n + 1023) // 1024
    assert np.array_equal(p["order_blocks"], order_blocks)
    assert np.array_equal(p["setup_order"], np.where(fused, np.where(ready != 0, order_blocks, 0), -1))
    for m, per_block, most in ((QUAD, 16, 8192), (LANE, 64, 1024), (ROW, 4, 2048), (WAVE_ONLY, 4, 2048)):
        at = mapping == m
        assert at.any() and np.array_equal(p["grid"][at], np.minimum((n[at] + per_block - 1) // per_block, most))
    at = mapping == QUAD
    waves = np.minimum((n[at] + 15) // 16, 8192)
    rounds = (n[at] + 16 * waves - 1) // (16 * waves)
    assert np.array_equal(p["max_trips"][at], 16 * rounds * (cap[at] + 2) + 16)
    # every state of the order occurs, and both values of the set-up argument beside -1
    assert set(p["order"].tolist()) == {NO_ORDER, SORT_NOW, PREFETCHED, FORMS_NEXT}
    assert {-1, 0, 5, 256} <= set(p["setup_order"].tolist())
