"""The SPG tail of a one-iteration dictionary update (option spg_tail; csrc/dict_plan.h: dict_tail_needed).

With one SPG iteration per update, g_new, <d, g_new>, the BB step and the residual projection with its
CONVERGED / MAX_FEVAL flags have no reader in aa_outer_iterations, and in aa_iterate none once the status record
carries MAX_ITER (the judge masks CONVERGED out and the record is sticky).  Such updates run x += lambda d alone,
on the row groups the D'X pass flagged in d, or densely where it flagged none (reduce_sparse = 0).  Everything a
fit returns has to be the same bits with the tail (spg_tail = 1) and without: every comparison below is
np.array_equal or ==, never a tolerance.

Which form ran is read from Context.spg_path(): an iteration with its tail ends with the gradient launch of
g_new ("k_grad<..>"), one without ends with "tail:skip".  aa_iterate reports the last update only, so the batch
at which a fit starts to skip is counted from Context.proj_counts(): a tail is one projection (the residual's)
of an update's three, and the forced run makes exactly one more projection per skipped update.

Shapes: n = 2000, p = 256 and n = 1501, p = 130 (rows no multiple of 4, padding columns), k = 5 (KP = 32) and
k = 40 (KP = 64), both dtypes, 8 outer iterations from the benchmark's random start; at these shapes the direction
stays dense (tests/test_gpu_reduce_sparse.py), so every group is flagged, and one float32 case at 1500 x 4096,
k = 32 covers the sparse direction, where the flagged step skips most groups.  All n <= 8192: the projections
are the one-kernel form; the tail's kernels themselves are the business of tests/test_gpu_spg_step.py.

Planted defects, each run once against this file in a scratch build:
* x += lambda d left out of the skipped form: test_outer_iterations_identical (all 11 cases),
  test_iterate_identical_and_flips_after_first_batch (the five cases with more than one batch) and
  test_iterate_stopped_by_the_tolerance fail.
* a host decision that skips from the second batch on whatever the status record shows:
  test_converging_fit_keeps_the_tail fails (spg_flags 8 against 0 in the forced run).
(profiles/spg_tail_ab.txt, section 6.)
"""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F_CONV, F_ITER = 1, 8


@pytest.fixture(scope="module")
def be():
    from convex_dim_red import _backend
    _backend.require_gpu()
    assert (_backend.SPG_FLAG_CONVERGED, _backend.SPG_FLAG_MAX_ITER) == (F_CONV, F_ITER)
    return _backend


class _options(object):
    """Library options for a block, the defaults put back behind it."""
    DEFAULTS = dict(spg_tail=0, reduce_sparse=1, use_graph=0)

    def __init__(self, be, **opts):
        self.be, self.opts = be, opts

    def __enter__(self):
        for name, value in self.opts.items():
            self.be.set_option(name, value)

    def __exit__(self, *exc):
        for name in self.opts:
            self.be.set_option(name, self.DEFAULTS[name])


def _ran_tail(path):
    """True: the latest update ran its tail; False: it skipped it."""
    assert path and path[-1].startswith(("k_grad<", "tail:skip")), path
    assert "tail:skip" not in path[:-1], path
    return path[-1] != "tail:skip"


_PROBLEMS = {}


def _problem(n, p, k, dtype):
    """The benchmark's rows and random start at a small shape; built once per shape and left unchanged."""
    import bench
    key = (n, p, k)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (bench.synthetic_rows(0, n, n, p, k),) + bench.start_factors(n, k)
    X, C0, Z0 = _PROBLEMS[key]
    return X.astype(dtype), C0, Z0


def _open(be, n, p, k, dtype):
    X, C0, Z0 = _problem(n, p, k, dtype)
    ctx = be.Context(dtype=dtype)
    ctx.set_data(X)
    ctx.set_state(C0, Z0, np.ones(k))
    return ctx


def _n_proj(ctx):
    """Column projections the context has launched so far, whatever the strategy."""
    return sum(ctx.proj_counts().values())


def _assert_same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "item %d differs" % i


# ------------------------------------------------------------------ 1. aa_outer_iterations
def _outer(be, shape, dtype, tail, n_outer=8, spg_kw=None, **opts):
    with _options(be, spg_tail=tail, **opts):
        with _open(be, *shape, dtype=dtype) as ctx:
            ctx.prepare()
            costs = ctx.outer_iterations(n_outer, dict(dict(max_iterations=1), **(spg_kw or {})), {})
            path = ctx.spg_path()
            n_proj = _n_proj(ctx)
            C, Z, _ = ctx.get_state()
    return (costs, C, Z), path, n_proj


OUTER_CASES = [((n, p, k), dtype, {}) for (n, p) in ((2000, 256), (1501, 130)) for k in (5, 40)
               for dtype in ("float32", "float64")]
OUTER_CASES += [((2000, 256, 5), "float32", dict(reduce_sparse=0)),      # the dense step
                ((1501, 130, 40), "float64", dict(use_graph=1)),         # the captured pair of iterations
                ((1500, 4096, 32), "float32", {})]                       # the sparse direction


@pytest.mark.parametrize("shape,dtype,opts", OUTER_CASES,
                         ids=["%dx%d-k%d-%s%s" % (s + (d, "".join("-%s%d" % kv for kv in sorted(o.items()))))
                              for s, d, o in OUTER_CASES])
def test_outer_iterations_identical(be, shape, dtype, opts):
    """8 outer iterations: the costs after every update, C and Z do not depend on spg_tail; the default skips the
    tail (one projection less per update), the forced run does not."""
    skip, path_skip, n_skip = _outer(be, shape, dtype, 0, **opts)
    full, path_full, n_full = _outer(be, shape, dtype, 1, **opts)
    assert not _ran_tail(path_skip) and _ran_tail(path_full)
    # (host-side counters: with use_graph two updates run eagerly and the captured pair is counted once)
    assert n_full - n_skip == (4 if opts.get("use_graph") else 8)
    assert np.isfinite(skip[0]).all() and skip[0][-1] < skip[0][0]
    _assert_same(skip, full)


# ------------------------------------------------------------------ 2. aa_iterate
def _iterate(be, shape, dtype, tail, max_outer, check_every, tol):
    with _options(be, spg_tail=tail):
        with _open(be, *shape, dtype=dtype) as ctx:
            cost0 = ctx.prepare()
            costs, st = ctx.iterate(cost0, max_outer, tol, "abs_delta_f", False, True, True, dict(max_iterations=1), {},
                                    check_every=check_every)
            path = ctx.spg_path()
            n_proj = _n_proj(ctx)
            C, Z, _ = ctx.get_state()
    record = (st.n_iter, st.converged, st.error_stage, st.spg_flags, st.reserved, st.cost)
    return (np.concatenate([[cost0], costs]), C, Z), record, path, n_proj


@pytest.mark.parametrize("max_outer", [1, 7, 20])
@pytest.mark.parametrize("check_every", [1, 3, 8])
def test_iterate_identical_and_flips_after_first_batch(be, check_every, max_outer):
    """The judged loop, default against forced: iteration count, costs, flags, verdict and factors.  The first
    batch of a fit runs every tail (its status record is still empty on the host); the batch shows MAX_ITER, so
    every update behind it skips: the forced run makes one projection more per update beyond the first batch."""
    shape, dtype = (1501, 130, 5), "float32"
    got, rec, path, n_proj = _iterate(be, shape, dtype, 0, max_outer, check_every, 0.0)
    want, rec_full, path_full, n_proj_full = _iterate(be, shape, dtype, 1, max_outer, check_every, 0.0)
    assert rec == rec_full and rec[0] == max_outer - 1 and rec[4] == max_outer
    assert rec[3] & F_ITER
    _assert_same(got, want)
    assert _ran_tail(path_full)
    assert _ran_tail(path) == (max_outer <= check_every)
    assert n_proj_full - n_proj == max(0, max_outer - check_every)


def test_iterate_stopped_by_the_tolerance(be):
    """A tolerance the fit meets in the middle of a batch: iterations behind the stopping one have run (some of
    them without a tail) and the kept factors are restored; record and factors as in the forced run."""
    shape, dtype = (1501, 130, 5), "float64"
    every = 4
    probe, _, _, _ = _iterate(be, shape, dtype, 1, 16, 16, 0.0)
    steps = np.abs(probe[0][2::2] - probe[0][:-1:2])                         # |cost after iteration i - cost before it|
    # the stopping iteration: the first from the second batch on whose step is smaller than every step before it and
    # which is not the last of its batch (so that iterations behind it have run)
    stop = next(i for i in range(every + 1, 16) if 0 < steps[i] < steps[:i].min() and (i + 1) % every)
    tol = float(0.5 * (steps[stop] + steps[:stop].min()))
    enqueued = -(-(stop + 1) // every) * every
    got, rec, path, n_proj = _iterate(be, shape, dtype, 0, 40, every, tol)
    want, rec_full, _, n_proj_full = _iterate(be, shape, dtype, 1, 40, every, tol)
    assert rec == rec_full and rec[:3] == (stop, 1, 0) and rec[4] == enqueued
    _assert_same(got, want)
    assert np.array_equal(got[0][:2 * stop + 3], probe[0][:2 * stop + 3])
    assert not _ran_tail(path)
    assert n_proj_full - n_proj == enqueued - every


# ------------------------------------------------------------------ 3. a fit whose SPG converges every time
def _fixed_point():
    """n = k = 8 rows, orthogonal, with entries that are powers of two: with C = Z = I the reconstruction is exact
    and every product of the update is too -- gradient, direction and residual are exactly zero."""
    X = np.zeros((8, 16))
    for i in range(8):
        X[i, 2 * i] = 2.0 ** (i % 3)
        X[i, 2 * i + 1] = -(2.0 ** ((i + 1) % 3))
    return X, np.eye(8), np.eye(8)


def test_converging_fit_keeps_the_tail(be):
    """The status record never shows MAX_ITER, so no batch may skip: flags, costs and projection counts as in the
    forced run, the last update with its tail."""
    from oracle import aa_oracle as orc
    X, C0, Z0 = _fixed_point()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                       # spg.py:278-281 warns unless converged
        x, _, n_iter, _ = orc.update_aa_dictionary(X, C0, np.ones(8), np.trace(X.dot(X.T)), X.dot(X.T).dot(Z0),
                                                   Z0.T.dot(Z0), max_iterations=1)
    assert n_iter == 0 and np.array_equal(x, C0)

    def run(tail, dtype):
        with _options(be, spg_tail=tail):
            with be.Context(dtype=dtype) as ctx:
                ctx.set_data(X.astype(dtype))
                ctx.set_state(C0, Z0, np.ones(8))
                cost0 = ctx.prepare()
                costs, st = ctx.iterate(cost0, 9, -1.0, "abs_delta_f", False, True, True, dict(max_iterations=1), {},
                                        check_every=2)
                return costs, st.n_iter, st.spg_flags, ctx.spg_path(), _n_proj(ctx), ctx.get_state()[0]

    for dtype in ("float64", "float32"):
        costs, n_iter, flags, path, n_proj, C = run(0, dtype)
        costs_f, n_iter_f, flags_f, path_f, n_proj_f, C_f = run(1, dtype)
        assert n_iter == n_iter_f == 8 and flags == flags_f and not flags & F_ITER
        assert _ran_tail(path) and _ran_tail(path_f) and n_proj == n_proj_f
        assert np.array_equal(costs, costs_f) and np.array_equal(C, C_f) and np.array_equal(C, C0)


# ------------------------------------------------------------------ 4. paths that keep the tail
def test_two_spg_iterations_keep_the_tail(be):
    shape, dtype = (1501, 130, 5), "float32"
    a, path_a, n_a = _outer(be, shape, dtype, 0, n_outer=4, spg_kw=dict(max_iterations=2))
    b, path_b, n_b = _outer(be, shape, dtype, 1, n_outer=4, spg_kw=dict(max_iterations=2))
    assert _ran_tail(path_a) and _ran_tail(path_b) and path_a == path_b and n_a == n_b
    _assert_same(a, b)


def test_updates_with_stats_keep_the_tail(be):
    """aa_dictionary_update / aa_weights_update called one by one, with a stats record: ||res||, the evaluation
    count and the flags are the tail's."""
    def run(tail):
        out = []
        with _options(be, spg_tail=tail):
            with _open(be, 1501, 130, 5, "float64") as ctx:
                ctx.prepare()
                for _ in range(4):
                    st = ctx.dictionary_update(max_iterations=1)
                    assert _ran_tail(ctx.spg_path())
                    out += [st.res_norm, st.n_feval, st.flags, st.f, ctx.spg_scalars()["dgn"]]
                    ctx.weights_update()
                C, Z, _ = ctx.get_state()
                return out + [C, Z], _n_proj(ctx)
    a, n_a = run(0)
    b, n_b = run(1)
    assert n_a == n_b and a[0] > 0 and a[2] & F_ITER
    _assert_same(a, b)


def test_restart_slots_keep_the_tail(be):
    """Two restarts side by side (aa_slots_*): their updates are outside the skipped form."""
    from oracle import aa_oracle as orc
    n, p, k, R, iters = 300, 40, 4, 2, 6
    rng = np.random.RandomState(3)
    X = orc.right_stochastic_matrix((n, k), rng).dot(rng.standard_normal((k, p))) + 0.1 * rng.standard_normal((n, p))
    starts = [(orc.right_stochastic_matrix((k, n), rng), orc.right_stochastic_matrix((n, k), rng)) for _ in range(R)]

    def run(tail):
        out = []
        with _options(be, spg_tail=tail):
            with be.Context(dtype="float64") as ctx:
                ctx.set_data(X)
                ctx.aa_slots_begin(R, k, iters, 0.0, "abs_delta_f", False, dict(max_iterations=1), {})
                for r, (C0, Z0) in enumerate(starts):
                    ctx.aa_slots_load(r, C0, Z0)
                for r, st in enumerate(ctx.aa_slots_run(iters)):
                    assert st.stop and not st.error_stage
                    out += [st.stop_iter, st.flags] + list(ctx.aa_slots_fetch(r, st.stop_iter, True))
                assert "tail:skip" not in ctx.spg_path()
                n_proj = _n_proj(ctx)
                ctx.aa_slots_end()
        return out, n_proj
    a, n_a = run(0)
    b, n_b = run(1)
    assert n_a == n_b
    _assert_same(a, b)


def test_forced_communicator_keeps_the_tail(be):
    """The multi-rank code path on one rank (AA_FORCE_RCCL=1): its tail carries riding collectives and stays."""
    def run(tail):
        os.environ["AA_FORCE_RCCL"] = "1"
        try:
            with _options(be, spg_tail=tail):
                X, C0, Z0 = _problem(1501, 130, 5, "float32")
                with be.Context(dtype="float32") as ctx:
                    ctx.comm_init(be.comm_unique_id(), 0, 1)
                    ctx.set_data(X)
                    ctx.set_state(C0, Z0, np.ones(5))
                    ctx.prepare()
                    costs = ctx.outer_iterations(4, dict(max_iterations=1), {})
                    assert _ran_tail(ctx.spg_path())
                    C, Z, _ = ctx.get_state()
                    return (costs, C, Z), _n_proj(ctx)
        finally:
            os.environ.pop("AA_FORCE_RCCL", None)
    a, n_a = run(0)
    b, n_b = run(1)
    assert n_a == n_b
    _assert_same(a, b)
