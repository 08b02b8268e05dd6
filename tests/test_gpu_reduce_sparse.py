"""The flagged reduce-over-rows pass (option reduce_sparse): same bits as the dense pass.

The dictionary update multiplies X by its search direction D, which is zero in all but a few hundred
rows.  launch_reduce_rows(..., flag_buf) flags the aligned groups of 4 rows of the tall operand that
hold an entry != 0.0 (k_group_flags), lets k_reduce_rows_gather_f32 / _f64_mfma issue the dense
kernel's MFMA steps for the flagged groups only -- per slab, if the slab has at most
reduce_sparse_max of them -- and runs the gated dense kernel on the other slabs.  For finite X the
result has to equal the dense pass bit for bit: every test below compares with np.array_equal
against aa_pass_reduce_rows on the same context, never with a tolerance, and checks the split the
device reports (aa_reduce_sparse_counts) against the split worked out here from the operand.

Shapes: p = 640 (float32: two column groups, the second with one active wave of four; float64:
three, the last with two), n = 250 (n_pad 256: 8 slabs of 32 rows, the XCD-aware block map) and
n = 300 (n_pad 384: 12 slabs, the natural map), k = 5 and 32 (KP = 32) and k = 40 (KP = 64).  A
slab has 8 groups, so the gather kernels' batches of four groups and their one-group remainder
loop both run (5 to 8 flagged groups in a slab).  One larger float32 case (8400 x 65 536) has
528 groups per slab: the second round of 512 flag bytes, which no smaller matrix reaches
(rows_per_slab > 2048 needs n p > 2^29 under the 512-block target of ensure_problem).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pass_kernels import _relative, f32_bound, launch_model, random_operands  # noqa: E402

pytestmark = pytest.mark.gpu

P = 640
SHAPES = [(250, 5), (250, 32), (250, 40), (300, 5), (300, 32), (300, 40)]
DEFAULT_OPTIONS = dict(reduce_sparse=1, reduce_sparse_max=-1, use_graph=0)


def _restore():
    from convex_dim_red import _backend
    for name, value in DEFAULT_OPTIONS.items():
        _backend.set_option(name, value)


def expected_split(A, m, limit):
    """(gathered, dense) slab counts for the tall operand A under the geometry m: what k_group_flags and
    the gather kernel's per-slab decision must arrive at."""
    n_pad, rps = m["n_pad"], m["rows_per_slab"]
    full = np.zeros((n_pad, A.shape[1]))
    full[:A.shape[0]] = A
    flagged = (full != 0.0).any(axis=1).reshape(-1, 4).any(axis=1)          # NaN != 0 is True, -0.0 != 0 False
    gathered = dense = 0
    for s in range(m["nslab"]):
        cnt = int(flagged[s * rps // 4:min((s + 1) * rps, n_pad) // 4].sum())
        if cnt <= limit:
            gathered += 1
        else:
            dense += 1
    return gathered, dense


def operands(n, k, m, seed):
    """name -> (tall operand, reduce_sparse_max).  8 groups per slab: a limit of 8 lets the gather kernel take
    every slab."""
    rng = np.random.RandomState(seed)
    rps = m["rows_per_slab"]
    assert rps == 32 and m["nslab"] >= 2

    def rows(*idx):
        A = np.zeros((n, k))
        A[list(idx)] = rng.standard_normal((len(idx), k))
        return A

    out = {}
    out["all zero"] = (np.zeros((n, k)), 8)
    A = np.zeros((n, k))
    A[0, k - 1] = 0.75
    out["one entry in row 0"] = (A, 8)
    A = np.zeros((n, k))
    A[n - 1, 0] = -1.25
    out["one entry in row n - 1"] = (A, 8)
    out["both sides of a slab boundary"] = (rows(rps - 1, rps, 3 * rps - 1, 3 * rps), 8)
    # groups 2, 3, 4, 5 of slab 1 with their only non-zero row in position 0, 1, 2, 3; then two rows of one
    # group (positions 1 and 2: one in each row pair of the float32 kernel)
    out["each position of a group"] = (rows(rps + 8, rps + 13, rps + 18, rps + 23, 2 * rps + 5, 2 * rps + 6), 8)
    A = rows(7, rps + 2)
    A[A == 0] = -0.0
    A[40:60] = -0.0
    assert np.signbit(A).sum() > 20 * k
    out["-0.0 entries"] = (A, 8)
    A = np.zeros((n, k))
    A[rps + 17, 0] = 5e-324                                   # the smallest float64 subnormal: flagged, and
    A[rps + 3] = rng.standard_normal(k)                       # (float32 kernel) converted to a zero operand
    out["a subnormal entry"] = (A, 8)
    # slab 0: 3 flagged groups = reduce_sparse_max; slab 1: 4 -> dense; slab 2: 5, slab 3: 8 -> dense; others empty
    A = rows(0, 9, 30, rps + 1, rps + 4, rps + 8, rps + 12, *[2 * rps + 4 * g + g % 4 for g in (0, 2, 3, 5, 7)])
    if m["nslab"] > 3:
        A[3 * rps:min(4 * rps, n)] = rng.standard_normal((min(4 * rps, n) - 3 * rps, k))
    out["limit and limit + 1"] = (A, 3)
    # 5, 6, 7 and 8 flagged groups in slabs 0..3, all gathered: a batch of four groups plus 1, 2, 3 and 4 more
    A = np.zeros((n, k))
    for s, cnt in enumerate((5, 6, 7, 8)):
        for g in range(cnt):
            A[s * rps + 4 * g + (g + s) % 4] = rng.standard_normal(k)
    out["batches and remainders"] = (A, 8)
    dense = rng.uniform(size=(n, k))
    out["fully dense, default limit"] = (dense, -1)           # 8 groups > 8 // 4 (float64: 8 // 2): the dense kernel
    out["fully dense, gathered"] = (dense, 8)                 # every MFMA step of the pass through the gather kernel
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n,k", SHAPES, ids=["n%d-k%d" % s for s in SHAPES])
def test_flagged_pass_equals_dense_pass_bit_for_bit(dtype, n, k):
    from convex_dim_red import _backend
    m = launch_model(dtype, {}, n, P, k)
    assert m["nslab"] == (8 if n == 250 else 12)
    Xr, _, _ = random_operands(n, P, k, 21)
    X = Xr.astype(dtype)
    try:
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(X)
            for name, (A, limit) in operands(n, k, m, 5).items():
                _backend.set_option("reduce_sparse_max", limit)
                want = ctx.pass_reduce_rows(A)
                got = ctx.pass_reduce_rows_flagged(A)
                counts = ctx.reduce_sparse_counts()
                eff = limit if limit >= 0 else m["rows_per_slab"] // 4 // (4 if dtype == "float32" else 2)
                split = expected_split(A, m, eff)
                print("%s n=%d k=%d %-32s gathered/dense slabs %s (expected %s), %d elements differ" % (
                    dtype, n, k, name, counts, split, int((got != want).sum())))
                assert counts == split, (name, counts, split)
                assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:8].tolist())
                if name == "all zero":
                    assert not got.any() and not np.signbit(got).any()
            # reduce_sparse = 0: the flagged entry point IS the dense pass, and the counters stay where they were
            _backend.set_option("reduce_sparse", 0)
            before = ctx.reduce_sparse_counts()
            A = operands(n, k, m, 5)["batches and remainders"][0]
            assert np.array_equal(ctx.pass_reduce_rows_flagged(A), ctx.pass_reduce_rows(A))
            assert ctx.reduce_sparse_counts() == before
    finally:
        _restore()


def test_second_round_of_flag_bytes():
    """528 groups per slab (float32, 8400 x 65 536: 4 slabs of 2112 rows): flagged groups on both sides of
    group 512 of a slab go through the gather kernel's second round of flag bytes."""
    from convex_dim_red import _backend
    n, p, k = 8400, 65536, 3
    m = launch_model("float32", {}, n, p, k)
    assert m["nslab"] == 4 and m["rows_per_slab"] == 2112
    r = np.arange(n, dtype=np.float32)[:, None]
    c = np.arange(p, dtype=np.float32)[None, :]
    X = (1.0 + (r % 13.0)) * np.float32(0.37) + ((c % 29.0) - 14.0) * np.float32(0.11) * (1.0 + (r % 3.0))
    assert X.dtype == np.float32
    rng = np.random.RandomState(3)
    A = np.zeros((n, k))
    picks = [0, 5, 4 * 511 + 3, 4 * 512, 4 * 527 + 1,                       # slab 0: groups 0, 1, 511, 512, 527
             2112 + 4 * 100, 2112 + 4 * 512 + 2, 2112 + 4 * 513,             # slab 1
             3 * 2112 + 4 * 515, n - 1]                                      # slab 3 (short: 2064 rows)
    A[picks] = rng.standard_normal((len(picks), k))
    try:
        _backend.set_option("reduce_sparse_max", 528)
        with _backend.Context(dtype="float32") as ctx:
            ctx.set_data(X)
            want = ctx.pass_reduce_rows(A)
            got = ctx.pass_reduce_rows_flagged(A)
            assert ctx.reduce_sparse_counts() == (4, 0)
        assert np.array_equal(got, want), int((got != want).sum())
        assert np.abs(want).max() > 0
    finally:
        _restore()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_flagged_pass_against_float64_numpy(dtype):
    """One case against NumPy with the bound tests/test_gpu_pass_kernels.py holds the dense kernel to: n_pad
    2^-53 of sum |a||x| in float64, 4 x the emulated one-chain float32 error in float32."""
    from convex_dim_red import _backend
    n, k = 300, 5
    m = launch_model(dtype, {}, n, P, k)
    Xr, _, A = random_operands(n, P, k, 7)
    keep = np.zeros(n, bool)
    keep[[0, 1, 2, 3, 31, 32, 40, 97, 98, 130, 131, 132, 133, 200, 299]] = True
    A[~keep] = 0.0
    if dtype == "float32":
        X = Xr.astype(np.float32)
        Xd = X.astype(np.float64)
        A = A.astype(np.float32).astype(np.float64)
    else:
        X = Xd = Xr
    try:
        _backend.set_option("reduce_sparse_max", 8)
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(X)
            got = ctx.pass_reduce_rows_flagged(A)
            assert ctx.reduce_sparse_counts() == (m["nslab"], 0)
    finally:
        _restore()
    err = _relative(got, A.T.dot(Xd), np.abs(A).T.dot(np.abs(Xd)))
    bound = m["n_pad"] * 2.0 ** -53 if dtype == "float64" else f32_bound(Xd.T, A.T, None)[0]
    print("%s flagged pass against NumPy: %.3e of sum|a||x|, bound %.3e" % (dtype, err, bound))
    assert err <= bound


def _small_fit(shape, dtype, sparse, graph, limit):
    import bench
    from convex_dim_red import _backend
    n, p, k = shape
    X = bench.synthetic_rows(0, n, n, p, k).astype(dtype)
    C0, Z0 = bench.start_factors(n, k)
    _backend.set_option("reduce_sparse", sparse)
    _backend.set_option("reduce_sparse_max", limit)
    _backend.set_option("use_graph", graph)
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(X)
        ctx.set_state(C0, Z0, np.ones(k))
        ctx.prepare()
        costs = np.asarray(ctx.outer_iterations(8, dict(max_iterations=1), {}))
        counts = ctx.reduce_sparse_counts()
        C, Z, _ = ctx.get_state()
    return costs, C, Z, counts


def _with_and_without(shape, dtype, graph, limit):
    try:
        on = _small_fit(shape, dtype, 1, graph, limit)
        off = _small_fit(shape, dtype, 0, graph, limit)
    finally:
        _restore()
    print("%s %s graph=%d reduce_sparse_max=%d: slabs of the last D'X pass gathered/dense %s; last cost %.17g" % (
        shape, dtype, graph, limit, on[3], on[0][-1]))
    assert np.array_equal(on[0], off[0])
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    assert off[3] == (0, 0)
    return on[3]


@pytest.mark.parametrize("dtype,graph", [("float32", 0), ("float64", 0), ("float32", 1)],
                         ids=["float32", "float64", "float32-graph"])
def test_small_fit_is_identical_with_and_without(dtype, graph):
    """2000 rows of the benchmark's data, p = 256, k = 5, random start, 8 outer iterations: the costs and the
    factors do not depend on reduce_sparse, and the last D'X pass had a slab served by the gather kernel.

    At this shape the direction never turns sparse: in the CPU oracle's iterate_aa (spg.py:148 restated as the
    device path has it, no re-projection of its own dictionary) the line search shortens every step, C keeps
    all its 10 000 entries non-zero and D all its 2000 rows through 1500 outer iterations (the same at 1900
    and 2100 rows through 300), so no iteration count reaches a sparse direction here.  What the gather kernel
    serves in this fit is the 64th slab, the padding rows 2016..2047, and in float64 (limit: half a slab) also
    the 63rd, half padding (counts (1, 63) and (2, 62) on the device); the fit checks that dense slabs and
    gathered slabs in one call reproduce the dense pass over eight updates.
    The sparse phase is the business of test_sparse_phase_fit_is_identical_with_and_without."""
    counts = _with_and_without((2000, 256, 5), dtype, graph, -1)
    assert counts[0] > 0 and sum(counts) == 64


@pytest.mark.parametrize("dtype,graph,limit", [("float32", 0, 0), ("float64", 0, 0), ("float32", 1, 0),
                                               ("float32", 0, 1), ("float64", 0, 1)],
                         ids=["float32", "float64", "float32-graph", "float32-all-gathered", "float64-all-gathered"])
def test_sparse_phase_fit_is_identical_with_and_without(dtype, graph, limit):
    """1500 rows of the benchmark's data at the benchmark's p = 4096 and k = 32, random start, 8 outer
    iterations.  Here the CPU oracle's direction is dense in outer iterations 0 and 1 and has 157 to 169
    non-zero rows (135 to 143 of the 375 groups) in iterations 2 to 7, like the headline run.  48 slabs of 8
    groups (float64: 24 of 16): with the default limit, a quarter (float64: half) of a slab's groups, some slabs are gathered
    and some dense in the sparse iterations (both kernels serve one call); with `limit` = all of a slab's
    groups the gather kernel serves every slab of every iteration, the two dense ones included."""
    m = launch_model(dtype, {}, 1500, 4096, 32)
    assert (m["nslab"], m["rows_per_slab"]) == ((48, 32) if dtype == "float32" else (24, 64))
    counts = _with_and_without((1500, 4096, 32), dtype, graph, m["rows_per_slab"] // 4 if limit else -1)
    assert sum(counts) == m["nslab"] and counts[0] > 0
    if limit:
        assert counts == (m["nslab"], 0)
