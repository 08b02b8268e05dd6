"""The device FurthestSum chain (csrc/kernels_tall.hip: launch_furthest_sum with k_fs_init, k_fs_distance, k_fs_step)
and the distance columns of the two explicit forms (k_distance_data, k_distance_kernel), pick by pick: the case
table, the reference rule restated, the device's search and lane arithmetic restated, the bound of a column entry
and the host-only tests that hold them.  Nothing here needs a GPU; tests/test_gpu_furthest_sum.py imports all of it.

THE RULE (``reference_replay``).  The reference keeps a list of [index, running sum], sorts it stably by sum before
every pick and pops the last element; a point that leaves is pushed back at the end with the sum of its distances to
the other selected points, in the order of ``selected`` (furthest_sum.py:17-20, :103-125 of the reference).  The
replay is driven by distance columns the way the product's host path reads them: ``col(j)[i]`` is D[i, j] for
adding and for removing j, and the back-sum of a leaving point l reads D[l, other] = ``col(other)[l]``.  After every
pick and every re-entry it records the index, the alive set and the running sums (a point that is no candidate keeps
the sum it was popped with); a pick at which the largest live sum occurs more than once is reported as shared.

THE DEVICE (``device_chain``, ``device_search``).  launch_furthest_sum's sequence of (distance column of st->cur,
step) pairs on arrays, with k_fs_step's search: thread t of 1024 scans i = t, t + 1024, ... keeping (best, first
arg, count), then the tree 512 ... 1 with its three branches (b > a: take b; b == a: add the counts and take b's
index if a has none; else keep a).  The flag goes up when the final count is not 1, when nothing is left, or when a
live sum is NaN.  ``fault`` plants one mistake.  The third branch's hand-over (``si[t] < 0``) cannot act: an index
>= 0 implies a value above -inf, so two equal values either both carry an index or both are -inf without one.  The
planted fault that drops it therefore changes nothing on any input, which test_handover_is_unreachable pins; every
other planted fault makes at least one table case fail.

THE LANES (``lane_column_data``, ``lane_column_kernel``).  Data form: lane l takes the columns l, l + 64, ... of the
zero-padded width p_pad = roundup(p, 128), three fma chains (a a, a b, b b), the butterfly 32 ... 1, then
sqrt(max(sii - 2 sij + sjj, 0)).  NumPy has no fma; a fused step is formed in long double and rounded once to
float64 (the 64-bit product carries an error of 2^-11 u, far below what the bound leaves spare).  The butterfly is
tests/rbf_restatement.py's.  Kernel form: sqrt(max((kd - 2 kj) + jj, 0)) per row.

THE BOUND of a column entry against np.longdouble on the stored values, u = 2^-53.
* Data form.  Each of the three dot products is a chain of m = p_pad / 64 fused multiply-adds per lane and six
  butterfly additions: at most (m + 6) u times the sum of the absolute values of its terms.  sii - 2 sij + sjj
  rounds twice more on operands no larger than that sum.  So the squared distance is off by at most
  e_s = (m + 8) u (sum a^2 + 2 sum |a b| + sum b^2).  The clamp at 0 only moves a value towards the true one.
* With d the computed and d* the true distance, |d - d*| = |d^2 - d*^2| / (d + d*) <= e_s / (d + d*), and never
  more than sqrt(e_s) (|d - d*|^2 <= |d^2 - d*^2|); the square root rounds once more: u d.
* Kernel form.  kd - 2 kj rounds once whether or not the compiler contracts it into an fma (2 kj is exact), adding
  jj rounds once: e_s = 2 u (|kd| + 2 |kj| + |jj|), the root as above.  Entries are compared within the bound.
The tests allow BOUND_MULTIPLE = 2 times this bound, as the standardisation suite does: the factor covers the terms
of second order in u, the long-double reference's own rounding (2^-11 u per operation) and, on the host, the
emulated fma.  Exact facts are asserted as such: d[j] == 0.0, and identical stored rows give identical bits.

MARGINS.  The cases marked ``oracle`` are also compared with the oracle's furthest_sum on the matrix NumPy forms by
the reference's formula (archetypal_analysis.py:96-100 of the reference), whose entries differ from the device's in
their last bits.  That comparison is only meaningful when no pick hangs on those bits: ``assert_margins`` replays
the case in long double and requires every pick to lead the runner-up by at least 1000 times the bounds accumulated
in the two sums (the column bounds of everything added and subtracted, and u per addition).  It is a condition on
the inputs, checked here on the CPU; the inputs (a tight cluster and extreme points at distinct radii) are chosen
so that it holds.  The other cases are compared with the replay on the device's own columns, which needs no margin.
"""
import zlib

import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
BOUND_MULTIPLE = 2.0
MARGIN_FACTOR = 1000.0
THREADS = 1024                   # k_fs_step's single block
FAULTS = ("count_dropped", "tree_ge", "back_transposed", "back_reversed", "leaving_stays_dead", "dead_updated",
          "waves_stop_16")


def round_up(a, b):
    return -(-a // b) * b


# ------------------------------------------------------------------ the case table
# name -> dict(form, dtype, n, p, k, start, exclude, extra, twins, nonsym, oracle, flag, edges).  p of a kernel-form
# case is the width of the data its kernel matrix is formed from.  ``twins``: None or (kind, a, b) -- rows a and b are
# identical; kind "far": an outlier, "near": next to the centroid.  ``flag``: the device's tie flag after the whole
# chain.  ``edges``: what the row is there for (test_table_covers_every_edge recomputes it).
CASES = {}


def _case(edges, form, dtype, n, p, k, start, exclude, extra, twins=None, nonsym=False, oracle=False, flag=False):
    name = "%s_%s_n%d_p%d_k%d_s%d_x%d_e%d%s%s" % (form, "f32" if dtype == "float32" else "f64", n, p, k, start,
                                                  len(exclude), extra,
                                                  "" if twins is None else "_%s_%d_%d" % twins,
                                                  "_nonsym" if nonsym else "")
    assert name not in CASES, name
    CASES[name] = dict(name=name, form=form, dtype=dtype, n=n, p=p, k=k, start=start, exclude=list(exclude),
                       extra=extra, twins=twins, nonsym=nonsym, oracle=oracle, flag=flag, edges=edges.split())


F32, F64 = "float32", "float64"
# the four rows per block of the data-form column, p around the 64 lanes and the padding step
_case("n=1 k=1 e=2k+3 rows4_partial start_0 start_last p_lt_64", "data", F64, 1, 1, 1, 0, [], 5)
_case("n=1 k=1 e=k+1", "data", F32, 1, 1, 1, 0, [], 2)
_case("n=1 k=1 e=3", "data", F64, 1, 1, 1, 0, [], 3)
_case("n=3 rows4_partial p_lt_64 k=2 e=k-1 start_last data_f32", "data", F32, 3, 63, 2, 2, [], 1, oracle=True)
_case("n=4 rows4_full p_eq_64 k=2 e=k start_0 data_f64", "data", F64, 4, 64, 2, 0, [], 2, oracle=True)
_case("n=5 rows4_partial p_gt_64 k=2 e=k+1 ex_one start_last", "data", F64, 5, 65, 2, 4, [2], 3, oracle=True)
# the 256 rows per block of k_fs_init and of the kernel-form column; k around the 16 waves of op 2
_case("n=255 blocks256_below p_pad_256 k=15 e=0 ex_none", "data", F32, 255, 130, 15, 7, [], 0, oracle=True)
_case("n=256 blocks256_at k=16 e=k-1 start_0 op2_rounds=1", "data", F64, 256, 5, 16, 0, [], 15, oracle=True)
_case("n=257 blocks256_past k=17 e=2k+3 ex_ends op2_rounds=2 wrap", "data", F64, 257, 20, 17, 5, [0, 100, 256], 37,
      oracle=True)
_case("k=33 e=2k+3 op2_rounds=3 wrap", "data", F32, 257, 20, 33, 9, [], 69, oracle=True)
_case("k=64 e=2k+3 op2_rounds=4 wrap", "data", F64, 257, 7, 64, 256, [3], 131, oracle=True)
_case("k=64 e=k-1 op2_rounds=4 data_f32", "data", F32, 300, 7, 64, 11, [], 63)
_case("k=1 e=0", "data", F64, 40, 5, 1, 17, [], 0, oracle=True)
_case("pool_empties k=17 e=2k+3 ex_ends", "data", F64, 20, 5, 17, 3, [0, 19, 7], 37, oracle=True)
# the 1024 threads of the step
_case("n=1023 step_partial_round k=2 e=2k+3", "data", F32, 1023, 5, 2, 1022, [], 7, oracle=True)
_case("n=1024 step_full_round k=15 e=k+1", "data", F64, 1024, 5, 15, 0, [], 16, oracle=True)
_case("n=1025 step_second_round_one k=16 e=k ex_ends", "data", F64, 1025, 5, 16, 1, [0, 1024, 512], 16, oracle=True)
_case("n=2047 step_second_round_short k=17 e=k start_last", "data", F64, 2047, 5, 17, 2046, [], 17, oracle=True)
_case("n=2049 step_third_round k=33 e=k+1", "data", F32, 2049, 5, 33, 100, [], 34, oracle=True)
_case("e=1 k=2", "data", F64, 70, 5, 2, 3, [], 1, oracle=True)
# the kernel form, both storage types, n up to 1100, a matrix that is not symmetric in its last bits
_case("kernel_f64 n=255 blocks256_below", "kernel", F64, 255, 7, 4, 0, [], 5, oracle=True)
_case("kernel_f32 n=256 blocks256_at k=15", "kernel", F32, 256, 7, 15, 255, [], 1, oracle=True)
_case("kernel_f64 n=257 blocks256_past nonsym k=17 op2_rounds=2", "kernel", F64, 257, 7, 17, 4, [0, 256], 18,
      nonsym=True)
_case("kernel_f32 n=1025 step_second_round_one", "kernel", F32, 1025, 7, 2, 9, [], 3, oracle=True)
_case("kernel_f64 n=1100 k=16", "kernel", F64, 1100, 7, 16, 1099, [5], 0, oracle=True)
_case("kernel_f64 nonsym n=5", "kernel", F64, 5, 3, 3, 1, [], 7, nonsym=True)
_case("kernel_f32 nonsym", "kernel", F32, 40, 5, 5, 2, [], 11, nonsym=True)
# shared maxima from identical stored rows: a far outlier twice -- in one thread's stride, merged at the first and
# at the last tree level, in different waves -- and the three placements that must NOT raise the flag
_case("tie_in_thread", "data", F64, 2049, 5, 3, 0, [], 2, twins=("far", 7, 1031), flag=True)
_case("tie_level_512", "data", F64, 1100, 5, 3, 0, [], 2, twins=("far", 10, 522), flag=True)
_case("tie_level_1", "data", F32, 300, 5, 3, 0, [], 2, twins=("far", 10, 11), flag=True)
_case("tie_level_2 tie_other_wave", "data", F64, 300, 5, 3, 0, [], 2, twins=("far", 10, 200), flag=True)
_case("tie_kernel_form", "kernel", F64, 64, 5, 3, 0, [], 2, twins=("far", 3, 40), flag=True)
# k = 1: the single point leaves and every running sum drops to exactly 0, a shared maximum by construction
_case("k=1 e=2 all_zero", "data", F64, 40, 5, 1, 17, [], 2, flag=True)
_case("twin_excluded", "data", F64, 2049, 5, 3, 0, [1031], 2, twins=("far", 7, 1031))
_case("twin_is_start", "data", F64, 2049, 5, 3, 7, [], 0, twins=("far", 7, 1031))
_case("twins_not_max", "data", F64, 2049, 5, 3, 0, [], 4, twins=("near", 7, 1031))

REQUIRED_EDGES = set("""n=1 n=3 n=4 n=5 n=255 n=256 n=257 n=1023 n=1024 n=1025 n=2047 n=2049 rows4_full rows4_partial
blocks256_below blocks256_at blocks256_past step_partial_round step_full_round step_second_round_one
step_second_round_short step_third_round p_lt_64 p_eq_64 p_gt_64 p_pad_256 data_f32 data_f64 kernel_f32 kernel_f64
k=1 k=2 k=15 k=16 k=17 k=33 k=64 e=0 e=1 e=k-1 e=k e=k+1 e=2k+3 e=3 op2_rounds=1 op2_rounds=2 op2_rounds=3
op2_rounds=4 wrap ex_none ex_one ex_ends pool_empties start_0 start_last nonsym tie_in_thread tie_level_512
tie_level_1 tie_other_wave tie_kernel_form all_zero twin_excluded twin_is_start twins_not_max""".split())


def edges_of(case):
    """The edges a case reaches, from its numbers alone and the launch rules: (n + 3) / 4 blocks of four waves (data-
    form column), (n + 255) / 256 blocks of 256 threads (k_fs_init, kernel-form column), one block of 1024 threads
    striding over n (k_fs_step), p_pad = roundup(p, 128) in lanes of 64, one wave per selected point in rounds of
    16 (op 2), slot = s % k."""
    n, p, k, e, ex = case["n"], case["p"], case["k"], case["extra"], case["exclude"]
    out = {"n=%d" % n, "k=%d" % k, "%s_%s" % (case["form"], "f32" if case["dtype"] == F32 else "f64")}
    out.add("rows4_full" if n % 4 == 0 else "rows4_partial")
    if n >= 255:
        out.add({255: "blocks256_below", 0: "blocks256_at", 1: "blocks256_past"}.get(n % 256, "blocks256_inside"))
    rounds, last = -(-n // THREADS), n % THREADS
    if rounds == 1 and n == THREADS - 1:
        out.add("step_partial_round")
    if n == THREADS:
        out.add("step_full_round")
    if rounds == 2:
        out.add("step_second_round_one" if last == 1 else "step_second_round_short")
    if rounds == 3:
        out.add("step_third_round")
    if case["form"] == "data":
        out.add("p_lt_64" if p < 64 else ("p_eq_64" if p == 64 else "p_gt_64"))
        if round_up(p, 128) > 128:
            out.add("p_pad_256")
    out.add("e=%d" % e)
    for label, value in (("e=k-1", k - 1), ("e=k", k), ("e=k+1", k + 1), ("e=2k+3", 2 * k + 3)):
        if e == value:
            out.add(label)
    if e > 0:
        out.add("op2_rounds=%d" % -(-k // 16))
    if e > k and k > 1:
        out.add("wrap")
    out.add("ex_none" if not ex else ("ex_one" if len(ex) == 1 else "ex_several"))
    if len(ex) > 1 and 0 in ex and n - 1 in ex:
        out.add("ex_ends")
    if k == n - len(ex) and e > 0 and n > 1:
        out.add("pool_empties")
    if k == 1 and e > 0 and n - len(ex) > 2:
        out.add("all_zero")
    if case["start"] == 0:
        out.add("start_0")
    if case["start"] == n - 1:
        out.add("start_last")
    if case["nonsym"]:
        out.add("nonsym")
    if case["twins"] is not None:
        kind, a, b = case["twins"]
        ta, tb = a % THREADS, b % THREADS
        if kind == "near":
            out.add("twins_not_max")
        elif b in ex or a in ex:
            out.add("twin_excluded")
        elif case["start"] in (a, b):
            out.add("twin_is_start")
        elif case["form"] == "kernel":
            out.add("tie_kernel_form")
        elif ta == tb:
            out.add("tie_in_thread")
        else:
            o = 512
            while ta % o != tb % o:          # after the tree's step o, thread x's value sits at x % o
                o >>= 1
            out.add("tie_level_%d" % o)
            if ta // 64 != tb // 64:
                out.add("tie_other_wave")
    return out


# ------------------------------------------------------------------ the inputs of a case
def problem(case):
    """The matrix handed to set_data (``A``: X, or K in the kernel form) and the values the context stores of it as
    float64 (``S``): a tight cluster around the origin and extreme points at distinct radii."""
    rng = np.random.RandomState(zlib.crc32(case["name"].encode()) & 0x7FFFFFFF)
    n, p = case["n"], case["p"]
    X = 0.2 * rng.standard_normal((n, p))
    n_far = min(n, 2 * case["k"] + 8)
    far = rng.choice(n, n_far, replace=False)
    direction = rng.standard_normal((n_far, p))
    direction /= np.sqrt((direction * direction).sum(axis=1))[:, None]
    X[far] = direction * (3.0 + 0.37 * np.arange(n_far) + 0.1 * rng.uniform(size=n_far))[:, None]
    if case["twins"] is not None:
        kind, a, b = case["twins"]
        X[a] = (12.0 if kind == "far" else 0.01) * rng.standard_normal(p)
        X[b] = X[a]
    if case["form"] == "data":
        A = X
    else:
        A = X.dot(X.T)
        A = 0.5 * (A + A.T)
        if case["twins"] is not None:          # identical rows AND columns, whatever the BLAS did
            _, a, b = case["twins"]
            A[b, :] = A[a, :]
            A[:, b] = A[:, a]
            A[a, b] = A[b, a] = A[b, b] = A[a, a]
    A = A.astype(case["dtype"])
    if case["nonsym"]:                          # a few ulps above the diagonal: D[l, o] and D[o, l] differ
        upper = np.triu(np.ones((n, n), dtype=bool), 1)
        A = np.where(upper, A * (1 + 3 * np.finfo(A.dtype).eps), A).astype(case["dtype"])
    return dict(case=case, A=A, S=A.astype(np.float64))


def host_column(pb, j):
    """Column j in float64 by a formula whose result depends on the row's values alone, so that identical rows give
    identical bits (a BLAS product need not): what the host tests drive the replays with."""
    S = pb["S"]
    if pb["case"]["form"] == "data":
        df = S - S[j]
        return np.sqrt((df * df).sum(axis=1))
    dg = np.diag(S)
    return np.sqrt(np.maximum((dg - 2.0 * S[:, j]) + dg[j], 0.0))


def columns_of(pb, column=host_column):
    cache = {}

    def col(j):
        j = int(j)
        if j not in cache:
            cache[j] = column(pb, j)
        return cache[j]
    return col


def reference_matrix(pb):
    """The dissimilarity matrix as the reference forms it (archetypal_analysis.py:96-100) from the stored values."""
    S = pb["S"]
    K = S.dot(S.T) if pb["case"]["form"] == "data" else S
    dg = np.diag(K)
    with np.errstate(invalid="ignore"):
        return np.sqrt(dg[np.newaxis, :] - 2 * K + dg[:, np.newaxis])


# ------------------------------------------------------------------ the long-double column and its bound
def exact_column(pb, j):
    """(d*, T): column j in long double on the stored values, and the sum of the absolute values of everything added
    on the way to the squared distance."""
    S = pb["S"].astype(LD)
    if pb["case"]["form"] == "data":
        df = S - S[j]
        d = np.sqrt((df * df).sum(axis=1))
        T = (S * S).sum(axis=1) + 2 * np.abs(S).dot(np.abs(S[j])) + (S[j] * S[j]).sum()
    else:
        dg = np.diag(S)
        d = np.sqrt(np.maximum(dg - 2 * S[:, j] + dg[j], 0))
        T = np.abs(dg) + 2 * np.abs(S[:, j]) + np.abs(dg[j])
    return d, T


def column_bound(pb, d_exact, T, d_got):
    """min(e_s / (d + d*), sqrt(e_s)) + u d* (module docstring), long double, before BOUND_MULTIPLE."""
    case = pb["case"]
    chain = round_up(case["p"], 128) // 64 + 8 if case["form"] == "data" else 2
    e_s = chain * LD(U) * T
    both = d_exact + np.asarray(d_got, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        through = np.where(both > 0, e_s / np.where(both > 0, both, 1), 0)
    return np.minimum(through, np.sqrt(e_s)) + LD(U) * d_exact


def column_ratio(pb, j, got):
    """The largest |got - d*| / (BOUND_MULTIPLE x bound) over column j (0 where both are exactly 0)."""
    d, T = exact_column(pb, j)
    bound = BOUND_MULTIPLE * column_bound(pb, d, T, got)
    err = np.abs(np.asarray(got, dtype=LD) - d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / np.where(bound > 0, bound, 1), 0)
    assert np.all((bound > 0) | (err == 0)), j
    return float(r.max())


def probe_columns(case):
    """The columns part A looks at: both ends, one inside, the twins."""
    n = case["n"]
    js = {0, n - 1, n // 2, (5 * n) // 7}
    if case["twins"] is not None:
        js |= set(case["twins"][1:])
    return sorted(js)


# ------------------------------------------------------------------ the lanes, restated
def _fma(a, b, c):
    return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


def _butterfly(lanes):
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return lanes[:, 0]


def lane_column_data(S, j):
    """k_distance_data / k_fs_distance on stored values S (n x p, float64)."""
    n, p = S.shape
    Sp = np.zeros((n, round_up(p, 128)))
    Sp[:, :p] = S
    sii, sij, sjj = np.zeros((n, 64)), np.zeros((n, 64)), np.zeros((n, 64))
    for c0 in range(0, Sp.shape[1], 64):                 # lane l: column c0 + l
        a, b = Sp[:, c0:c0 + 64], Sp[j, c0:c0 + 64][None, :]
        sii, sij, sjj = _fma(a, a, sii), _fma(a, b, sij), _fma(b, b, sjj)
    sii, sij, sjj = _butterfly(sii), _butterfly(sij), _butterfly(sjj)
    return np.sqrt(np.maximum((sii - 2.0 * sij) + sjj, 0.0))


def lane_column_kernel(S, j):
    """k_distance_kernel / the kernel branch of k_fs_distance on a stored kernel matrix S (float64)."""
    dg = np.diag(S)
    return np.sqrt(np.maximum((dg - 2.0 * S[:, j]) + dg[j], 0.0))


def lane_column(pb, j):
    return (lane_column_data if pb["case"]["form"] == "data" else lane_column_kernel)(pb["S"], j)


# ------------------------------------------------------------------ the rule, restated
class Trajectory(object):
    """events: (kind, index, alive, sums, known) after every pick ("pick") and re-entry ("back"); ``known`` marks the
    points that have been candidates (the sums of the others mean nothing).  after[e]: the number of events once e
    extra steps are done; shared[i]: event i is a pick that met a shared maximum."""

    def __init__(self):
        self.events, self.after, self.shared, self.selected_after = [], [], [], []
        self.ends = []               # device_chain: (alive, sums, known) once e extra steps are done

    def record(self, kind, index, alive, sums, known, shared=False):
        self.events.append((kind, int(index), alive.copy(), sums.copy(), known.copy()))
        self.shared.append(bool(shared))

    def close_step(self, selected):
        self.after.append(len(self.events))
        self.selected_after.append([int(s) for s in selected])

    def first_shared(self):
        return self.shared.index(True) if True in self.shared else None

    def flag_after(self, e):
        return any(self.shared[:self.after[e]])


def reference_replay(col, n, k, start, exclude, extra):
    selected = [start] * k
    q = [[i, col(start)[i]] for i in range(n) if i != start and i not in exclude]
    last = np.zeros(n)                                   # the sum a point was popped with
    known = np.zeros(n, dtype=bool)
    known[[qi[0] for qi in q]] = True
    tr = Trajectory()

    def snapshot(kind, index, shared=False):
        alive, sums = np.zeros(n, dtype=bool), last.copy()
        for i, s in q:
            alive[i], sums[i] = True, s
        tr.record(kind, index, alive, sums, known, shared)

    def take():
        q.sort(key=lambda x: x[1])                       # stable
        shared = sum(1 for x in q if x[1] == q[-1][1]) > 1
        index, s = q.pop(-1)
        last[index] = s
        return index, shared

    def add(new):
        c = col(new)
        for qi in q:
            qi[1] += c[qi[0]]

    for slot in range(1, k):
        selected[slot], shared = take()
        snapshot("pick", selected[slot], shared)
        add(selected[slot])
    tr.close_step(selected)
    for step in range(extra):
        slot = step % k
        leaving = selected[slot]
        c = col(leaving)
        for qi in q:
            qi[1] -= c[qi[0]]
        back = 0
        for other in selected:
            if other != leaving:
                back += col(other)[leaving]
        q.append([leaving, back])
        known[leaving] = True
        snapshot("back", leaving)
        selected[slot], shared = take()
        snapshot("pick", selected[slot], shared)
        add(selected[slot])
        tr.close_step(selected)
    # the sums as they stand at the end (after the last add)
    snapshot("end", selected[(extra - 1) % k] if extra > 0 else selected[k - 1])
    return tr


# ------------------------------------------------------------------ the device, restated
def device_search(sums, alive, fault=None):
    """k_fs_step's pick: (index or -1, flag)."""
    n = sums.shape[0]
    t = np.arange(THREADS)
    sv, si, sc = np.full(THREADS, -np.inf), np.full(THREADS, -1, dtype=np.int64), np.zeros(THREADS, dtype=np.int64)
    nan = False
    for r in range(-(-n // THREADS)):                    # for (i = t; i < n; i += 1024), every thread at once
        i = t + r * THREADS
        inside = i < n
        ii = np.where(inside, i, 0)
        live = inside & alive[ii]
        v = sums[ii]
        gt = live & (v > sv)
        eq = live & ~gt & (v == sv)
        nan = nan or bool(np.any(live & np.isnan(v)))
        si = np.where(gt, i, si)
        sc = np.where(gt, 1, sc)
        if fault != "count_dropped":
            sc = sc + eq
        sv = np.where(gt, v, sv)
    o = THREADS // 2
    while o:
        a, b = sv[:o].copy(), sv[o:2 * o]
        gt = (b >= a) if fault == "tree_ge" else (b > a)
        eq = ~gt & (b == a)
        hand = eq & (si[:o] < 0) if fault != "handover_dropped" else np.zeros(o, dtype=bool)
        sv[:o] = np.where(gt, b, a)
        si[:o] = np.where(gt | hand, si[o:2 * o], si[:o])
        sc[:o] = np.where(gt, sc[o:2 * o], np.where(eq, sc[:o] + sc[o:2 * o], sc[:o]))
        o >>= 1
    return int(si[0]), bool(sc[0] != 1 or si[0] < 0 or nan)


def device_chain(col, n, k, start, exclude, extra, fault=None):
    """launch_furthest_sum: k_fs_init, then (k_fs_distance of st->cur, k_fs_step) pairs."""
    alive = np.ones(n, dtype=bool)
    alive[start] = False
    alive[np.asarray(exclude, dtype=np.int64)] = False
    known = alive.copy()
    sums = np.zeros(n)
    st = dict(cur=start, selected=[start] * k)
    tr = Trajectory()

    def step(op, slot, pick, pick_slot, set_cur_slot):
        c = col(st["cur"])                                # the distance launch in front of every step
        touch = np.ones(n, dtype=bool) if fault == "dead_updated" else alive
        leaving = st["selected"][slot] if op == 2 else -1
        if op == 0:
            sums[touch] = c[touch]
        elif op == 1:
            sums[touch] = sums[touch] + c[touch]
        else:
            sums[touch] = sums[touch] - c[touch]
            dback = np.zeros(k)
            for wave in range(16):
                for q in range(wave, k, 16):
                    if fault == "waves_stop_16" and q >= 16:
                        break
                    other = st["selected"][q]
                    if other != leaving:
                        dback[q] = col(leaving)[other] if fault == "back_transposed" else col(other)[leaving]
            back = 0.0
            for q in (range(k - 1, -1, -1) if fault == "back_reversed" else range(k)):
                if st["selected"][q] != leaving:
                    back += dback[q]
            if fault != "leaving_stays_dead":
                alive[leaving] = True
            known[leaving] = True
            sums[leaving] = back
            tr.record("back", leaving, alive, sums, known)
        if pick:
            a, flag = device_search(sums, alive, fault)
            a = max(a, 0)
            st["selected"][pick_slot] = a
            alive[a] = False
            st["cur"] = a
            tr.record("pick", a, alive, sums, known, flag)
        elif set_cur_slot >= 0:
            st["cur"] = st["selected"][set_cur_slot]

    first_leaving = 0 if extra > 0 else -1

    def close():                                          # the arrays as a chain with this many extra steps ends
        tr.close_step(st["selected"])
        tr.ends.append((alive.copy(), sums.copy(), known.copy()))

    if k > 1:
        step(0, 0, 1, 1, -1)
    else:
        step(0, 0, 0, 0, first_leaving)
    for slot in range(1, k):
        if slot + 1 < k:
            step(1, 0, 1, slot + 1, -1)
        else:
            step(1, 0, 0, 0, first_leaving)
    close()
    for s in range(extra):
        slot = s % k
        step(2, slot, 1, slot, -1)
        step(1, 0, 0, 0, (s + 1) % k if s + 1 < extra else -1)
        close()
    last = tr.selected_after[-1][(extra - 1) % k] if extra > 0 else tr.selected_after[-1][k - 1]
    tr.record("end", last, alive, sums, known)
    return tr


def compare(dev, ref):
    """The device's trajectory against the rule's, event by event up to and including the first shared maximum
    (beyond it the rule's winner depends on the list's history and the two part ways): the same picks, alive sets
    and sums bit for bit, and the flag exactly where the maximum is shared."""
    stop = ref.first_shared()
    upto = len(ref.events) if stop is None else stop + 1
    assert len(dev.events) == len(ref.events)
    for i in range(upto):
        kd, jd, ad, sd, nd = dev.events[i]
        kr, jr, ar, sr, nr = ref.events[i]
        shared_only = i == stop                          # at the shared pick itself the winners may differ
        assert kd == kr and np.array_equal(nd, nr), i
        assert dev.shared[i] == ref.shared[i], (i, kd, jd, jr)
        if shared_only:
            continue
        assert jd == jr, (i, kd, jd, jr)
        assert np.array_equal(ad, ar), (i, kd)
        assert np.array_equal(sd[nd], sr[nr]), (i, kd, np.flatnonzero(sd[nd] != sr[nr])[:5])


def chain_args(case):
    return case["n"], case["k"], case["start"], case["exclude"], case["extra"]


def prefixes(case):
    """The extra_steps the GPU test runs a case with: every prefix, thinned where the chain is long."""
    k, E = case["k"], case["extra"]
    if E <= 40:
        return list(range(E + 1))
    return sorted(set(e for e in (0, 1, 2, k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, E - 1, E) if 0 <= e <= E))


# ------------------------------------------------------------------ margins
def assert_margins(pb):
    """Long-double replay of an ``oracle`` case: every pick leads the runner-up by MARGIN_FACTOR times the bounds
    accumulated in the running sums, and the reference's own matrix is finite.  Returns (picks after the whole
    chain, the smallest margin / bound)."""
    case = pb["case"]
    n, k, start, exclude, extra = chain_args(case)
    assert np.all(np.isfinite(reference_matrix(pb))), case["name"]
    cache = {}

    def col(j):
        if j not in cache:
            d, T = exact_column(pb, j)
            cache[j] = (d, column_bound(pb, d, T, d))
        return cache[j]

    alive = np.ones(n, dtype=bool)
    alive[[start] + list(exclude)] = False
    S, B = col(start)[0].copy(), col(start)[1].copy()
    selected, worst = [start] * k, [np.inf]

    def take():
        live = np.flatnonzero(alive)
        order = live[np.argsort(S[live], kind="stable")]
        best = order[-1]
        if order.size > 1:
            lead, room = S[best] - S[order[-2]], 2 * B[live].max()
            assert lead >= MARGIN_FACTOR * room, (case["name"], int(best), float(lead), float(room))
            worst[0] = min(worst[0], float(lead / room))
        alive[best] = False
        return int(best)

    def shift(j, sign):
        d, b = col(j)
        S[alive] += sign * d[alive]
        B[alive] += b[alive] + LD(U) * np.abs(S[alive])

    for slot in range(1, k):
        selected[slot] = take()
        shift(selected[slot], 1)
    for step in range(extra):
        slot = step % k
        leaving = selected[slot]
        shift(leaving, -1)
        others = [o for o in selected if o != leaving]
        S[leaving] = sum((col(o)[0][leaving] for o in others), LD(0))
        B[leaving] = sum((col(o)[1][leaving] for o in others), LD(0)) + len(others) * LD(U) * S[leaving]
        alive[leaving] = True
        selected[slot] = take()
        shift(selected[slot], 1)
    return selected, worst[0]


# ------------------------------------------------------------------ the host-only tests
@pytest.fixture(scope="module")
def problems():
    return {name: problem(case) for name, case in CASES.items()}


@pytest.fixture(scope="module")
def references(problems):
    """name -> the rule's trajectory on the host columns, computed once."""
    return {name: reference_replay(columns_of(pb), *chain_args(pb["case"])) for name, pb in problems.items()}


def test_table_covers_every_edge():
    reached = set()
    for case in CASES.values():
        got = edges_of(case)
        missing = [e for e in case["edges"] if e not in got]
        assert not missing, (case["name"], missing)
        reached |= got
    assert not REQUIRED_EDGES - reached, sorted(REQUIRED_EDGES - reached)
    for case in CASES.values():                          # what the entry point would refuse is not in the table
        n, k, start, exclude, extra = chain_args(case)
        assert 1 <= k <= 64 and 0 <= start < n and start not in exclude and k <= n - len(exclude)
        assert all(0 <= e < n for e in exclude) and len(set(exclude)) == len(exclude)
        assert prefixes(case)[0] == 0 and prefixes(case)[-1] == extra


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_search_and_chain_follow_the_rule(problems, references, name):
    """The restated device chain against the restated rule on every table case: the same index at every pick
    without a tie, the same alive sets and sums bit for bit, the flag exactly where the maximum is shared -- and
    at the end exactly where the table says."""
    pb = problems[name]
    dev = device_chain(columns_of(pb), *chain_args(pb["case"]))
    compare(dev, references[name])
    assert any(dev.shared) == pb["case"]["flag"]
    assert any(references[name].shared) == pb["case"]["flag"]


def test_the_rule_is_the_products_host_path(problems, references):
    """The restated rule and convex_dim_red's host selection (its _Pool, tie rule included) pick the same points."""
    from convex_dim_red.furthest_sum import furthest_sum_from_columns
    for name, pb in problems.items():
        col = columns_of(pb)
        n, k, start, exclude, extra = chain_args(pb["case"])
        got = furthest_sum_from_columns(lambda j, sense: col(j), lambda i, j: col(j)[int(i)], n, k, start,
                                        exclude=exclude, extra_steps=extra)
        assert list(got) == references[name].selected_after[-1], name


def _fails(pb, ref, fault):
    try:
        compare(device_chain(columns_of(pb), *chain_args(pb["case"]), fault=fault), ref)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_noticed(problems, references, fault):
    caught = [name for name in sorted(CASES) if _fails(problems[name], references[name], fault)]
    print("furthest-sum-faults %s: noticed by %d of %d cases (%s ...)" % (fault, len(caught), len(CASES),
                                                                         ", ".join(caught[:3])))
    assert caught, fault


def test_handover_is_unreachable(problems, references):
    """Dropping the tree's ``si[t] < 0`` hand-over changes no pick, count or flag: on every table case, and on
    sums with -inf, +inf and NaN among the live ones (module docstring: the branch cannot act)."""
    for name in sorted(CASES):
        assert not _fails(problems[name], references[name], "handover_dropped"), name
    rng = np.random.RandomState(3)
    for trial in range(200):
        n = int(rng.choice([1, 2, 5, 700, 1024, 1500, 2100]))
        sums = rng.choice([-np.inf, np.inf, np.nan, 0.0, 1.5, 2.5], size=n, p=[0.3, 0.02, 0.02, 0.3, 0.3, 0.06])
        alive = rng.uniform(size=n) < rng.choice([0.01, 0.5, 1.0])
        assert device_search(sums, alive) == device_search(sums, alive, "handover_dropped"), trial


def test_search_on_plain_vectors():
    """device_search against max / count on vectors with planted ties at every distance the tree merges."""
    rng = np.random.RandomState(4)
    for n in (1, 2, 1023, 1024, 1025, 2049):
        for gap in (None, 1, 2, 64, 512, 1024):
            sums = rng.uniform(size=n)
            alive = np.ones(n, dtype=bool)
            alive[rng.randint(n)] = n == 1
            top = int(np.argmax(np.where(alive, sums, -1)))
            twin = None if gap is None or top + gap >= n else top + gap
            if twin is not None:
                sums[twin], alive[twin] = sums[top], True
            index, flag = device_search(sums, alive)
            if not alive.any():
                assert (index, flag) == (-1, True)
            else:
                assert flag == (twin is not None) and (flag or index == top), (n, gap)
                assert sums[index] == sums[top]


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_restatements_stay_inside_the_bound(problems, name):
    pb = problems[name]
    case = pb["case"]
    worst = 0.0
    for j in probe_columns(case):
        d = lane_column(pb, j)
        worst = max(worst, column_ratio(pb, j, d), column_ratio(pb, j, host_column(pb, j)))
        assert d[j] == 0.0
        if case["twins"] is not None:
            _, a, b = case["twins"]
            assert d[a] == d[b] and np.array_equal(lane_column(pb, a), lane_column(pb, b))
    print("furthest-sum-errors host %s: max |d - d*| / (%g x bound) %.3f" % (name, BOUND_MULTIPLE, worst))
    assert worst <= 1.0


def test_bound_notices_a_wrong_column(problems):
    """A column that leaves out the last 64 columns of the padded width, or forgets the factor 2, is outside."""
    pb = problems[[n for n in sorted(CASES) if "p130" in n][0]]
    S, j = pb["S"], 3
    assert column_ratio(pb, j, lane_column_data(S[:, :128], j)) > 1.0
    d = lane_column_data(S, j)
    assert column_ratio(pb, j, d * (1 + 1e-14)) > 1.0


def test_margins_of_the_oracle_cases(problems, references):
    """assert_margins on exactly the cases that are compared with the oracle's selection; its long-double picks and
    the oracle's own on the reference's matrix are those of the rule on the host columns."""
    from oracle import aa_oracle as orc
    for name, pb in sorted(problems.items()):
        case = pb["case"]
        if not case["oracle"]:
            continue
        assert case["twins"] is None and not case["nonsym"]
        picks, worst = assert_margins(pb)
        print("furthest-sum-margins %s: smallest lead / accumulated bound %.3g" % (name, worst))
        assert picks == references[name].selected_after[-1], name
        n, k, start, exclude, extra = chain_args(case)
        want = orc.furthest_sum(reference_matrix(pb), k, start, exclude, extra)
        assert list(want) == picks, name


def test_margins_notice_a_tie(problems):
    pb = problems[[n for n in sorted(CASES) if "far_10_11" in n][0]]
    with pytest.raises(AssertionError):
        assert_margins(pb)


# ------------------------------------------------------------------ the host rule on a non-finite dissimilarity
def test_host_rule_names_a_non_finite_dissimilarity():
    """A running sum that is NaN (inf - inf behind an infinite dissimilarity) is refused by name, not by an
    IndexError from an empty arg-max."""
    import convex_dim_red as cdr
    D = np.array([[0.0, np.inf], [np.inf, 0.0]])
    with pytest.raises(ValueError, match="[Nn]on-finite dissimilarity"):
        cdr.furthest_sum(D, 1, 0, extra_steps=1)
    X = np.random.RandomState(0).standard_normal((6, 3))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    D[1, 4] = D[4, 1] = np.nan
    with pytest.raises(ValueError, match="[Nn]on-finite dissimilarity"):
        cdr.furthest_sum(D, 2, 1, extra_steps=2)
    assert len(cdr.furthest_sum(np.where(np.isnan(D), 0.0, D), 2, 1, extra_steps=2)) == 2
