"""pass_slabs, reduce_rows_plan and row_local_plan (csrc/pass_plan.h), the decisions of ensure_problem's slab
decomposition, launch_reduce_rows and launch_row_local, on a CPU at every edge of the dispatch.

The header is plain C++: tests/pass_plan_dump.cpp includes it alone, is built here with the host compiler, reads
cases from stdin and prints the plans' fields and the two names of aa_pass_kernels.  Two readings of the launchers
then have to agree case by case, with no GPU: launch_model (tests/test_gpu_pass_kernels.py, imported unchanged) gives
both names, the slabs, the column chunk and the waves per block.  What launch_model has no word for -- the grids,
the block size, the dynamic LDS bytes, the bytes of the split's partials, the template arguments, whether a call is
flagged and the gather limit -- is held against `before_the_plan` below: the launchers as they were before the plan
existed, branch by branch, written from them and not from the header.

Cases: the full cross product N x P x K x (every float32 knob set: row_local_variant -1..9 x row_local_acc64 0..2 x
row_local_split 0/1; every float64 one: f64_mfma 0..3 x row_local_split) with the reduce-over-rows knobs at their
defaults and a flag buffer given; then N x P x K x (float32, float64 at f64_mfma 0..3) at the default row-local
knobs x reduce_sparse x aa_gemm_timing x flag buffer x reduce_sparse_max in {-1, 0, 1, huge}.
"""
import itertools
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from test_gpu_pass_kernels import launch_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-factorization-case-studies_amd", "csrc")

# n: 1; both sides of the 128-row pad; of the 32 768-row threshold of the streaming kernels; the launch geometries of
# the pass-kernel tables (40 000 .. 135 000; 82 000 / 115 000 for float64); both sides of the first step of W
# (8 -> 9 behind 2048 row tiles) and of the step onto each cap: 10, 12, 14, 16 behind 2304, 2816, 3328, 3840 tiles
N = (1, 127, 128, 129, 32640, 32641, 40000, 65536, 65537, 70000, 73728, 73729, 82000, 90112, 90113, 100000, 106496,
     106497, 115000, 122880, 122881, 135000)
P = (1, 128, 129, 512, 513, 1300, 4096, 8192, 131072, 261700)
K = (1, 32, 33, 64)
HUGE = 2 ** 31 - 1                                             # reduce_sparse_max's upper end (INT_MAX)
F32_KNOBS = [dict(row_local_variant=v, row_local_acc64=a, row_local_split=s)
             for v in range(-1, 10) for a in range(3) for s in range(2)]
F64_KNOBS = [dict(f64_mfma=m, row_local_split=s) for m in range(4) for s in range(2)]
REDUCE_KNOBS = [dict(reduce_sparse=r, reduce_sparse_max=mx, time_gemm=t, flag_buf=f)
                for r in range(2) for mx in (-1, 0, 1, HUGE) for t in range(2) for f in range(2)]
DEFAULTS = dict(row_local_variant=-1, row_local_acc64=1, row_local_split=1, f64_mfma=1, reduce_sparse=1,
                reduce_sparse_max=-1, time_gemm=0, flag_buf=1)
KNOB_ORDER = ("row_local_variant", "row_local_acc64", "row_local_split", "f64_mfma", "reduce_sparse",
              "reduce_sparse_max")
MODEL_KNOBS = ("row_local_variant", "row_local_acc64", "row_local_split", "f64_mfma")      # launch_model's
N_SHAPES = len(N) * len(P) * len(K)
N_CASES = N_SHAPES * (len(F32_KNOBS) + len(F64_KNOBS) + 5 * len(REDUCE_KNOBS))
FIELDS = ("colgroups", "nslab", "rows_per_slab", "rr_family", "rr_targ", "flagged", "rr_grid_x", "rr_grid_y",
          "gather_limit", "rl_family", "rl_targ", "tile", "dbuf", "acc64", "variant", "W", "rl_grid_x", "rl_grid_y",
          "block", "lds", "raise_lds", "nsplit", "chunk", "partial_bytes")
RR_F32, RR_F64_MFMA, RR_F64_VALU = range(3)                                                # ReduceRowsFamily
F32_GLOBAL, F32_LDS, F32_BLK, F32_WS, F32_DMA, F64_WS, F64_MFMA, F64_VALU = range(8)       # RowLocalFamily
GRANULE = {F32_BLK: 128, F64_MFMA: 32}


def _cases():
    """(dtype, knobs incl. time_gemm and flag_buf, n, p, k) of every case"""
    for n, p, k in itertools.product(N, P, K):
        for knobs in F32_KNOBS:
            yield "float32", dict(DEFAULTS, **knobs), n, p, k
        for knobs in F64_KNOBS:
            yield "float64", dict(DEFAULTS, **knobs), n, p, k
        for knobs in REDUCE_KNOBS:
            yield "float32", dict(DEFAULTS, **knobs), n, p, k
            for m in range(4):
                yield "float64", dict(DEFAULTS, f64_mfma=m, **knobs), n, p, k


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(the cases, launch_model of each, the plans' integer fields as int64 columns, the two names of each)"""
    cxx = shutil.which("g++") or (os.path.exists("/opt/rocm/llvm/bin/clang++") and "/opt/rocm/llvm/bin/clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pass_plan") / "pass_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "pass_plan_dump.cpp"), "-o", exe], check=True)
    t0 = time.time()
    cases, models, lines = list(_cases()), [], []
    for dtype, o, n, p, k in cases:
        m = launch_model(dtype, {name: o[name] for name in MODEL_KNOBS}, n, p, k)
        models.append(m)
        lines.append("%s %d %d %d %d %d %d" % (" ".join(str(o[name]) for name in KNOB_ORDER), dtype == "float32",
                                               m["n_pad"], m["p_pad"], m["KP"], o["flag_buf"], o["time_gemm"]))
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    assert len(rows) == len(cases) and all(len(r) == len(FIELDS) + 2 for r in rows)
    ints = np.array([r[:len(FIELDS)] for r in rows], dtype=np.int64)
    print("pass plan: %d cases, models and plans in %.1f s" % (len(cases), time.time() - t0))
    return cases, models, {name: ints[:, i] for i, name in enumerate(FIELDS)}, [(r[-2], r[-1]) for r in rows]


def test_plan_agrees_with_launch_model(table):
    """Both names, nslab, rows_per_slab, chunk and W of every case are launch_model's."""
    cases, models, p, names = table
    p = {name: p[name].tolist() for name in ("nslab", "rows_per_slab", "chunk", "W")}
    bad = []
    for i, (case, m) in enumerate(zip(cases, models)):
        got = names[i] + (p["nslab"][i], p["rows_per_slab"][i], p["chunk"][i], p["W"][i])
        want = (m["rr"], m["rl"], m["nslab"], m["rows_per_slab"], m["chunk"], m["W"])
        if got != want:
            bad.append((case, got, want))
    assert not bad, "%d cases disagree, the first: %r" % (len(bad), bad[:5])
    assert len(cases) == N_CASES == 205920


def _ceil_div(a, b):
    return (a + b - 1) // b


def _round_up(a, b):
    return _ceil_div(a, b) * b


def before_the_plan(f32, o, n_pad, p_pad, KP, nslab, rps):
    """launch_reduce_rows (with launch_reduce_rows_flagged) and launch_row_local as they were before pass_plan.h,
    branch by branch: the fields of FIELDS that launch_model has no word for.  nslab, rps: Ctx::nslab and
    Ctx::rows_per_slab (held against launch_model above)."""
    e = {}
    # ---- launch_reduce_rows
    e["flagged"] = bool(o["flag_buf"] and o["reduce_sparse"] and not o["time_gemm"] and (f32 or o["f64_mfma"]))
    e["rr_grid_x"], e["rr_grid_y"] = (p_pad + 511) // 512 if f32 else (p_pad + 255) // 256, nslab
    if f32:
        e["rr_family"], e["rr_targ"] = RR_F32, 1 if KP == 32 else 2
    elif o["f64_mfma"]:
        e["rr_family"], e["rr_targ"] = RR_F64_MFMA, 2 if KP == 32 else 4
    else:
        e["rr_family"], e["rr_targ"] = RR_F64_VALU, KP
    gps = rps // 4
    limit = gps // (4 if f32 else 2) if o["reduce_sparse_max"] < 0 else o["reduce_sparse_max"]
    e["gather_limit"] = min(limit, gps)
    # ---- launch_row_local
    tiles = n_pad // 32
    e.update(tile=0, dbuf=0, acc64=0, variant=-1, W=0, rl_grid_y=1, block=256, lds=0, raise_lds=0, nsplit=1,
             chunk=p_pad, partial_bytes=0)

    def streaming(wmax, lds_elems, elem):
        W = min(max((tiles + 255) // 256, 8), wmax)
        e.update(W=W, rl_grid_x=(tiles + W - 1) // W, block=64 * W, lds=lds_elems(W) * elem, raise_lds=1)

    def split(rows, below, target, min_chunk, granule):
        rblocks = n_pad // rows
        nsplit, chunk = 1, p_pad
        if rblocks < below and o["row_local_split"]:
            nsplit = max(min((target + rblocks - 1) // rblocks, p_pad // min_chunk), 1)
        if nsplit > 1:
            chunk = _round_up((p_pad + nsplit - 1) // nsplit, granule)
            nsplit = (p_pad + chunk - 1) // chunk
        e.update(rl_grid_x=rblocks, rl_grid_y=nsplit, nsplit=nsplit, chunk=chunk,
                 partial_bytes=nsplit * n_pad * KP * 8 if nsplit > 1 else 0)

    if f32:
        v, a = o["row_local_variant"], o["row_local_acc64"]
        if v < 0:
            v = 4 if tiles < 8 * 128 else (9 if KP == 32 and a >= 1 else 8)
        e["variant"], e["rl_targ"] = v, KP // 32
        if v == 9 and KP == 32:
            e["rl_family"], e["acc64"] = F32_DMA, 1
            streaming(16, lambda W: 2 * 32 * 64 + W * 8 * 256, 4)
        elif v == 8:
            a64 = a >= 2
            e["rl_family"], e["acc64"] = F32_WS, int(a64)
            streaming(((16 if KP == 32 else 12) if not a64 else (12 if KP == 32 else 8)),
                      lambda W: 2 * KP * 128 + W * 32 * 64, 4)
        elif v >= 2:
            e["rl_family"], e["acc64"] = F32_BLK, int(a != 0)
            if KP == 32:
                e["tile"], e["dbuf"] = {3: (64, 1), 4: (128, 0), 5: (32, 1), 6: (128, 1), 7: (32, 0)}.get(v, (64, 0))
            else:
                e["tile"], e["dbuf"] = 64, int(v in (3, 5, 6))
            split(128, 384, 768, 512, 128)
        elif v == 1:
            e["rl_family"], e["rl_grid_x"] = F32_LDS, n_pad // 128
        else:
            RT = 2 if KP == 32 else 1
            e["rl_family"], e["rl_grid_x"] = F32_GLOBAL, (n_pad + 128 * RT - 1) // (128 * RT)
    else:
        m = o["f64_mfma"]
        if m == 2 or (m == 1 and tiles >= 8 * 128):
            e["rl_family"], e["rl_targ"] = F64_WS, KP // 16
            streaming(14 if KP == 32 else 10, lambda W: 2 * KP * 66 + W * 32 * 34, 8)
        elif m:
            e["rl_family"], e["rl_targ"] = F64_MFMA, 2 if KP == 32 else 4
            split(64, 192, 512, 256, 32)
        else:
            e["rl_family"], e["rl_targ"], e["rl_grid_x"] = F64_VALU, KP, n_pad // 64
    return e


def test_fields_launch_model_has_no_word_for(table):
    """Families, template arguments, grids, block size, LDS bytes, the split's partial bytes, `flagged` and the gather
    limit against the launchers as they were before the plan."""
    cases, models, p, _ = table
    cols = {name: col.tolist() for name, col in p.items()}
    bad, flagged_seen, limits_seen = [], set(), set()
    for i, ((dtype, o, n, pp, k), m) in enumerate(zip(cases, models)):
        f32 = dtype == "float32"
        want = before_the_plan(f32, o, m["n_pad"], m["p_pad"], m["KP"], m["nslab"], m["rows_per_slab"])
        got = {name: cols[name][i] for name in want}
        if got != want:
            bad.append(((dtype, o, n, pp, k), sorted((name, got[name], want[name]) for name in want
                                                     if got[name] != want[name])))
        flagged_seen.add((f32, o["f64_mfma"] != 0, o["reduce_sparse"], o["time_gemm"], o["flag_buf"], want["flagged"]))
        limits_seen.add((o["reduce_sparse_max"], want["gather_limit"] == m["rows_per_slab"] // 4))
    assert not bad, "%d cases disagree, the first: %r" % (len(bad), bad[:5])
    # flagged occurs, and fails for each of its reasons alone; the limit is capped at a slab's groups and is not
    assert (True, True, 1, 0, 1, True) in flagged_seen and (False, True, 1, 0, 1, True) in flagged_seen
    for alone in ((False, False, 1, 0, 1), (True, True, 0, 0, 1), (True, True, 1, 1, 1), (True, True, 1, 0, 0)):
        assert alone + (False,) in flagged_seen and alone + (True,) not in flagged_seen
    assert {(HUGE, True), (1, False), (0, False), (-1, False)} <= limits_seen
    assert set(cols["rl_family"]) == set(range(8)) and set(cols["rr_family"]) == set(range(3))


def test_invariants(table):
    """What every launch has to respect, whatever the knobs: the LDS a CU has, the block size, a column split that
    covers p_pad with no empty chunk in whole granules, at most 256 slabs that cover n_pad."""
    cases, models, p, _ = table
    n_pad = np.array([m["n_pad"] for m in models])
    p_pad = np.array([m["p_pad"] for m in models])
    assert (p["lds"] <= 160 * 1024).all() and (p["lds"] >= 0).all() and p["lds"].max() == 160 * 1024
    assert ((p["lds"] > 0) == (p["raise_lds"] != 0)).all()
    assert (p["block"] <= 1024).all() and (p["block"] % 64 == 0).all() and p["block"].max() == 1024
    assert (p["nsplit"] >= 1).all()
    assert (p["nsplit"] * p["chunk"] >= p_pad).all() and (p_pad > (p["nsplit"] - 1) * p["chunk"]).all()
    for family, granule in GRANULE.items():
        at = p["rl_family"] == family
        assert at.any() and (p["chunk"][at] % granule == 0).all() and (p["nsplit"][at] > 1).any()
    assert (p["nsplit"][~np.isin(p["rl_family"], list(GRANULE))] == 1).all()
    assert ((p["partial_bytes"] > 0) == (p["nsplit"] > 1)).all()
    assert (p["nslab"] >= 1).all() and (p["nslab"] <= 256).all() and p["nslab"].max() == 256
    assert (p["nslab"] * p["rows_per_slab"] >= n_pad).all() and (p["rows_per_slab"] % 32 == 0).all()
    assert ((p["nslab"] - 1) * p["rows_per_slab"] < n_pad).all()                # no empty slab
    for name in ("rr_grid_x", "rr_grid_y", "rl_grid_x", "rl_grid_y"):
        assert (p[name] >= 1).all() and (p[name] < 2 ** 31).all(), name
    assert (p["rl_grid_y"] <= 65535).all() and (p["rr_grid_y"] <= 65535).all()
