"""The device FurthestSum chain on the MI355X, pick by pick at its edges (aa_furthest_sum: k_fs_init, k_fs_distance,
k_fs_step) and the distance columns of the two explicit forms (k_distance_data, k_distance_kernel).  Everything the
tests are judged by -- the case table, the reference rule and the device's search restated, the bound of a column
entry, the margins -- lives in tests/test_furthest_sum_host.py, which also holds it to planted faults on the CPU.

A. columns: Context.distance_column against long double on the stored values within BOUND_MULTIPLE x the bound,
   d[j] == 0.0, identical rows bit-identical, and the chain's own last column (furthest_sum_state) bit for bit
   that of aa_distance_column.
B. the chain: furthest_sum(k, start, exclude, e) for the prefixes e = 0 ... E, the state read back after each
   (aa_get_furthest_sum_state) and held exactly to the restated chain driven by the device's own columns: selected,
   cur, the alive flags, the running sums bit for bit, the tie flag exactly where the rule reports a shared maximum.
C. the margin cases against the oracle's selection on the reference's own dissimilarity matrix.
D. identities: a repeated call, a call after a larger and after a smaller install (scratch reuse), the state error.
E. the float32 kernel matrix whose implied squared distance rounds below zero, and a non-finite kernel matrix: the
   device chain and the host-driven selection end the same way.

Every test prints ``furthest-sum-errors`` lines; the MI355X run is in profiles/furthest_sum_errors.txt."""
import numpy as np
import pytest

import test_furthest_sum_host as fh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from convex_dim_red import _backend
    _backend.require_gpu()
    return _backend


@pytest.fixture(scope="module")
def problems():
    return {name: fh.problem(case) for name, case in fh.CASES.items()}


def _install(backend, ctx, pb):
    ctx.set_data(pb["A"], form=backend.FORM_DATA if pb["case"]["form"] == "data" else backend.FORM_KERNEL)


def _device_columns(ctx, pb):
    return fh.columns_of(pb, lambda _, j: ctx.distance_column(j))


def _last_pick(selected, k, e):
    return selected[(e - 1) % k] if e > 0 else selected[k - 1]


def _host_selection(ctx, n, k, start, extra, exclude):
    from convex_dim_red import archetypal_analysis as aa
    aa._FURTHEST_SUM_ON_DEVICE = False
    try:
        return aa._furthest_sum_on_device(ctx, n, k, start, extra, np.asarray(exclude, dtype="i8"))
    finally:
        aa._FURTHEST_SUM_ON_DEVICE = True


def _dispatched(ctx, n, k, start, extra, exclude):
    from convex_dim_red import archetypal_analysis as aa
    assert aa._FURTHEST_SUM_ON_DEVICE
    return aa._furthest_sum_on_device(ctx, n, k, start, extra, np.asarray(exclude, dtype="i8"))


def _known_equal(a, b, known):
    return np.array_equal(a[known], b[known])


# ---------------------------------------------------------------- A. columns
@pytest.mark.parametrize("name", sorted(fh.CASES))
def test_columns(backend, problems, name):
    pb = problems[name]
    case = pb["case"]
    n, k, start, exclude, extra = fh.chain_args(case)
    worst = 0.0
    with backend.Context(dtype=case["dtype"]) as ctx:
        _install(backend, ctx, pb)
        for j in fh.probe_columns(case):
            d = ctx.distance_column(j)
            assert d.shape == (n,) and d[j] == 0.0, j
            worst = max(worst, fh.column_ratio(pb, j, d))
        if case["twins"] is not None:
            _, a, b = case["twins"]
            da, db = ctx.distance_column(a), ctx.distance_column(b)
            assert np.array_equal(da, db) and da[a] == 0.0 and da[b] == 0.0
            for j in fh.probe_columns(case):
                d = ctx.distance_column(j)
                assert d[a] == d[b], j
        for e in sorted({0, extra}):                      # the chain's own column: the arithmetic of aa_distance_column
            ctx.furthest_sum(k, start, exclude, e)
            st = ctx.furthest_sum_state()
            assert np.array_equal(st["column"], ctx.distance_column(st["cur"])), e
            worst = max(worst, fh.column_ratio(pb, st["cur"], st["column"]))
    print("furthest-sum-errors columns %s: max |d - d*| / (%g x bound) %.3f" % (name, fh.BOUND_MULTIPLE, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- B. the chain, step by step
@pytest.mark.parametrize("name", sorted(fh.CASES))
def test_chain_step_by_step(backend, problems, name):
    pb = problems[name]
    case = pb["case"]
    n, k, start, exclude, extra = fh.chain_args(case)
    with backend.Context(dtype=case["dtype"]) as ctx:
        _install(backend, ctx, pb)
        col = _device_columns(ctx, pb)
        model = fh.device_chain(col, n, k, start, exclude, extra)
        rule = fh.reference_replay(col, n, k, start, exclude, extra)
        fh.compare(model, rule)                           # on the device's own columns
        states = 0
        for e in fh.prefixes(case):
            got = ctx.furthest_sum(k, start, exclude, e)
            st = ctx.furthest_sum_state()
            alive, sums, known = model.ends[e]
            want = model.selected_after[e]
            assert list(st["selected"]) == want, (e, list(st["selected"]), want)
            assert st["cur"] == (_last_pick(want, k, e) if (k > 1 or e > 0) else start), e
            assert np.array_equal(st["alive"], alive), (e, np.flatnonzero(st["alive"] != alive)[:5])
            assert _known_equal(st["sums"], sums, known), (e, np.flatnonzero((st["sums"] != sums) & known)[:5])
            assert np.array_equal(st["column"], col(st["cur"])), e
            flag = model.flag_after(e)
            assert flag == rule.flag_after(e), e           # exactly where the rule reports a shared maximum
            assert bool(st["tie"]) == flag, (e, st["tie"])
            if flag:
                assert got is None, e
            else:
                assert got is not None and list(got) == rule.selected_after[e], (e, got)
            states += 1
        assert model.flag_after(extra) == case["flag"]
        # the dispatcher ends at the host's answer, which is the rule's
        want = _host_selection(ctx, n, k, start, extra, exclude)
        assert list(want) == rule.selected_after[-1]
        assert np.array_equal(_dispatched(ctx, n, k, start, extra, exclude), want)
        worst = fh.column_ratio(pb, st["cur"], st["column"])
    print("furthest-sum-errors chain %s: %d states (%d events) exact, flag %s; last column max |d - d*| / (%g x bound) "
          "%.3f" % (name, states, len(model.events), case["flag"], fh.BOUND_MULTIPLE, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- C. against the oracle's selection
@pytest.mark.parametrize("name", sorted(n for n, c in fh.CASES.items() if c["oracle"]))
def test_against_the_oracle(backend, problems, name):
    """The margin cases (test_furthest_sum_host.test_margins_of_the_oracle_cases): same indices in the same order as
    the oracle's furthest_sum on the matrix NumPy forms by the reference's formula."""
    from oracle import aa_oracle as orc
    pb = problems[name]
    case = pb["case"]
    n, k, start, exclude, extra = fh.chain_args(case)
    D = fh.reference_matrix(pb)
    with backend.Context(dtype=case["dtype"]) as ctx:
        _install(backend, ctx, pb)
        worst = 0.0
        for e in sorted({0, min(1, extra), extra}):
            want = orc.furthest_sum(D, k, start, exclude, e)
            got = ctx.furthest_sum(k, start, exclude, e)
            assert got is not None and list(got) == [int(w) for w in want], (e, got, want)
        st = ctx.furthest_sum_state()
        worst = fh.column_ratio(pb, st["cur"], st["column"])
    print("furthest-sum-errors oracle %s: picks equal; last column max |d - d*| / (%g x bound) %.3f"
          % (name, fh.BOUND_MULTIPLE, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- D. identities
def _state_bits(ctx, args):
    got = ctx.furthest_sum(*args)
    st = ctx.furthest_sum_state()
    return got, st


def _same_state(a, b, known):
    return (np.array_equal(a["selected"], b["selected"]) and a["cur"] == b["cur"] and a["tie"] == b["tie"]
            and np.array_equal(a["alive"], b["alive"]) and np.array_equal(a["column"], b["column"])
            and _known_equal(a["sums"], b["sums"], known))


def test_identities(backend, problems):
    """A repeated call gives the same bits; a call after a larger and after a smaller install gives the bits of a
    fresh context (the scratch buffer is reused, not cleared); the state is refused before any selection and after
    every install."""
    small = problems["data_f64_n257_p20_k17_s5_x3_e37"]
    large = problems["data_f64_n2047_p5_k17_s2046_x0_e17"]
    tiny = problems["data_f64_n5_p65_k2_s4_x1_e3"]

    def args(pb):
        n, k, start, exclude, extra = fh.chain_args(pb["case"])
        return k, start, exclude, extra

    def known(pb):
        n, k, start, exclude, extra = fh.chain_args(pb["case"])
        mask = np.ones(n, dtype=bool)
        mask[exclude] = False
        mask[start] = extra > 0
        return mask

    with backend.Context(dtype="float64") as fresh:
        _install(backend, fresh, small)
        with pytest.raises(RuntimeError, match="no selection"):
            fresh.furthest_sum_state()
        want_picks, want = _state_bits(fresh, args(small))
        again_picks, again = _state_bits(fresh, args(small))
        assert np.array_equal(want_picks, again_picks) and _same_state(want, again, known(small))
    with backend.Context(dtype="float64") as ctx:
        for first in (large, tiny):
            _install(backend, ctx, first)
            with pytest.raises(RuntimeError, match="no selection"):
                ctx.furthest_sum_state()
            _state_bits(ctx, args(first))
            _install(backend, ctx, small)
            with pytest.raises(RuntimeError, match="no selection"):      # a selection belongs to its rows
                ctx.furthest_sum_state()
            picks, st = _state_bits(ctx, args(small))
            assert np.array_equal(picks, want_picks) and _same_state(st, want, known(small))
    print("furthest-sum-errors identities: repeated call and calls after a larger / smaller install: same bits "
          "(error / bound 0.000)")


# ---------------------------------------------------------------- E. the clamp of the kernel form; non-finite entries
def _near_duplicate_kernel():
    rng = np.random.RandomState(2)
    X = rng.randn(12, 5) + 3
    X[7] = X[3] + 1e-5 * rng.randn(5)
    return X.dot(X.T).astype(np.float32)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("start", [3, 7])
def test_float32_kernel_matrix_whose_squared_distance_rounds_below_zero(backend, dtype, start):
    """K = float32(X X') with rows 3 and 7 of X nearly equal: K_33 - 2 K_37 + K_77 is negative, the reference has NaN
    there and no selection.  Clamped like the other three forms, the entry is 0 and the device chain and the
    host-driven selection return the same picks; everywhere else the columns stay within the bound."""
    K = _near_duplicate_kernel()
    K64 = K.astype(np.float64)
    assert (K64[3, 3] - 2 * K64[3, 7]) + K64[7, 7] < 0 and (K64[7, 7] - 2 * K64[7, 3]) + K64[3, 3] < 0
    pb = dict(case=dict(form="kernel", p=5, n=12, twins=None), A=K, S=K64)
    with backend.Context(dtype=dtype) as ctx:
        ctx.set_data(K, form=backend.FORM_KERNEL)
        assert ctx.distance_column(7)[3] == 0.0 and ctx.distance_column(3)[7] == 0.0
        worst = max(fh.column_ratio(pb, j, ctx.distance_column(j)) for j in range(12))
        for k, extra, exclude in ((3, 10, []), (2, 1, [0]), (5, 13, [11])):
            want = _host_selection(ctx, 12, k, start, extra, exclude)
            got = _dispatched(ctx, 12, k, start, extra, exclude)
            assert np.array_equal(got, want), (k, extra, got, want)
            direct = ctx.furthest_sum(k, start, exclude, extra)
            assert direct is None or np.array_equal(direct, want)
            st = ctx.furthest_sum_state()
            assert np.all(np.isfinite(st["sums"][st["alive"]])) and np.all(np.isfinite(st["column"]))
    print("furthest-sum-errors clamp %s start %d: both paths agree; max |d - d*| / (%g x bound) %.3f"
          % (dtype, start, fh.BOUND_MULTIPLE, worst))
    assert worst <= 1.0


def test_non_finite_kernel_matrix_ends_in_the_host_rule(backend):
    """The install keeps a non-finite entry.  K_01 = -inf makes d(0, 1) infinite; with k = 1 the start point leaves, the
    sum of candidate 1 becomes inf - inf and candidate 0 alone holds the largest comparable sum: no shared maximum, yet
    the chain raises its flag because a live sum is NaN, and both paths end in the host rule's ValueError."""
    K = np.array([[1.0, -np.inf], [-np.inf, 1.0]])
    with backend.Context(dtype="float64") as ctx:
        ctx.set_data(K, form=backend.FORM_KERNEL)
        assert np.array_equal(ctx.distance_column(0), [0.0, np.inf])
        assert ctx.furthest_sum(1, 0, [], 1) is None
        st = ctx.furthest_sum_state()
        assert st["tie"] == 1 and np.isnan(st["sums"][1]) and st["sums"][0] == 0.0
        for select in (_host_selection, _dispatched):
            with pytest.raises(ValueError, match="[Nn]on-finite dissimilarity"):
                select(ctx, 2, 1, 0, 1, [])
        assert list(ctx.furthest_sum(1, 0, [], 0)) == [0]             # nothing leaves: nothing is subtracted
    print("furthest-sum-errors non-finite K: flag raised on a NaN sum, ValueError on both paths (error / bound 0.000)")
