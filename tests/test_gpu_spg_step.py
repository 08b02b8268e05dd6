"""The dictionary SPG step on the device, kernel by kernel, past its projection.

Tables, reference, bounds and the checker live in test_spg_step_host.py (its docstring derives every bound);
this file runs them on the MI355X.  Every case first asserts what Context.spg_path() reports against
path_model, the restatement of the dispatch rules, and only then looks at numbers.

A  one dictionary_update(max_iterations=1) with a stats struct per row of CASES; every array of the update is
   read back (Context.spg_array) and held against the array before it in np.longdouble (check_step): the two
   gradients element-wise, M bit for bit, the set-up's s1 / a0 / f, the sums of the direction, the Gram traces,
   lambda, f_new and the BB step through the line search's formulas, C1 = fl(C0 + lambda d), the Gram of the
   accepted point as the weights QP reads it, n_feval / flags / backtracks / branches exactly.  The cost that
   k_linesearch_fin records is held to aa_cost_from_scalars of those scalars (test_recorded_cost).
   float32 data: the passes round d to float32 on its way into D'X, so P and Q carry float32-sized errors that
   belong to the pass suite; that context is held to everything that does not read P from the host.
B  parameter families over a few iterations against orc.update_aa_dictionary / update_kernel_aa_dictionary
   with the same keywords and the same host inputs: (n_iter, n_feval, flags) equal, f and the dictionary within
   max(floor, 20 x conftest.oracle_twins), floor 1e-11 for one iteration and 1e-9 beyond.
C  identities that hold by construction, bit for bit: fuse_finalize 0 / 1 with the LDS / VALU Grams,
   setup_in_grad 0 / 1, a repeated call on a fresh context, the call without a stats struct (side stream).

Every test prints a `spg-step-errors` line; the MI355X run is in profiles/spg_step_errors.txt.
"""
import ctypes

import numpy as np
import pytest

import conftest
from test_spg_step_host import (B_SHAPES, CASES, FAMILIES, F_CONV, F_ITER, LAST_BOUNDS, LD, OPT_DEFAULTS, U,
                                assert_margins, b_problem, case_id, check_history, check_step, family_kwargs, oracle_update, path_model, problem,
                                replay, report)

pytestmark = pytest.mark.gpu

ARRAYS = ("g", "g_prev", "d", "Gr", "Gr_prev", "H", "M", "f_mem")


@pytest.fixture(scope="module")
def be():
    from convex_dim_red import _backend
    _backend.require_gpu()
    return _backend


class _options(object):
    def __init__(self, be, opts):
        self.be, self.opts = be, opts

    def __enter__(self):
        for name, value in self.opts.items():
            self.be.set_option(name, value)

    def __exit__(self, *exc):
        for name in self.opts:
            self.be.set_option(name, OPT_DEFAULTS[name])


def _open(be, pb, dtype):
    ctx = be.Context(dtype=dtype)
    ctx.set_data(pb.A, form=be.FORM_KERNEL if pb.form == "kernel" else be.FORM_DATA)
    if pb.form == "linear":
        ctx.set_linear_kernel(True)
    ctx.set_state(np.ascontiguousarray(pb.x0.T), pb.Z, pb.alpha)
    ctx.prepare()
    return ctx


def _update(be, ctx, stats, **kw):
    if stats:
        st = ctx.dictionary_update(**kw)
        return st.n_feval, st.flags, st.n_iter
    p = be.spg_params(**kw)
    be._check(ctx.lib.aa_dictionary_update(ctx.h, ctypes.byref(p), None))
    return None, None, None


def _host_flags(device_flags):
    """What dictionary_update reports for a run that ended at its last allowed iteration (here: the only one):
    the device's flags, and the iteration cap unless the run converged (spg.py:278-281)."""
    return device_flags | (0 if device_flags & F_CONV else F_ITER)


def _collect(ctx, pb, start, counts):
    out = {name: ctx.spg_array(name) for name in ARRAYS}
    out["Q"] = ctx.spg_array("Q") if pb.form != "kernel" else None
    out["sc"] = ctx.spg_scalars()
    out["C0"] = start
    out["C"] = np.ascontiguousarray(ctx.get_state()[0].T)
    out["path"] = ctx.spg_path()
    out["gram"] = ctx.grams()[1]
    out["n_feval"], out["flags"], out["n_iter"] = counts
    if counts[0] is None:          # no stats struct: the scalars hold the counts
        out["n_feval"], out["flags"] = int(out["sc"]["n_feval"]), _host_flags(int(out["sc"]["flags"]))
    return out


def _host_inputs(pb, Z):
    A = pb.A
    H = A.T.dot(Z) if pb.form == "kernel" else A.dot(A.T.dot(Z))
    return H, Z.T.dot(Z)


def _run(be, name, stats=True):
    """The update of a case on a fresh context: (the inputs it saw, its record)."""
    c, pb = CASES[name], problem(name)
    with _options(be, c["opts"]):
        with _open(be, pb, c["dtype"]) as ctx:
            start, seen, device_inputs = pb.x0, pb, False
            if c["setup"] != "cold":
                ctx.dictionary_update(max_iterations=1)
                ctx.weights_update()
                Cm, Zm, _ = ctx.get_state()
                start = np.ascontiguousarray(Cm.T)
            if c["setup"] == "second_inputs":
                H, ZtZ = _host_inputs(pb, Zm)
                ctx.set_dictionary_inputs(H, ZtZ, pb.trace)
                seen = pb.replace(x0=start, H=H, ZtZ=ZtZ, Z=Zm)
            elif c["setup"] == "cold" and c["inputs"]:
                ctx.set_dictionary_inputs(pb.H, pb.ZtZ, pb.trace)
            else:
                device_inputs = True
                ZtZ, _, _, trace = ctx.grams()
            counts = _update(be, ctx, stats, **dict(c["sp"], max_iterations=1))
            out = _collect(ctx, pb, start, counts)
            if device_inputs:
                seen = pb.replace(x0=start, H=out["H"], ZtZ=ZtZ, trace=trace)
    return seen, out


_DEVICE = {}


def _device(be, name):
    if name not in _DEVICE:
        seen, out = _run(be, name)
        _DEVICE[name] = (seen, out, replay(seen, **CASES[name]["sp"]))
    return _DEVICE[name]


def _same_bits(a, b, gram=True):
    for key in ARRAYS + ("Q", "C") + (("gram",) if gram else ()):
        assert (a[key] is None and b[key] is None) or np.array_equal(a[key], b[key]), key
    for key in a["sc"]:
        assert a["sc"][key] == b["sc"][key], key
    assert (a["n_feval"], a["flags"]) == (b["n_feval"], b["flags"])
    assert a["flags"] == _host_flags(int(a["sc"]["flags"]))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("name", sorted(CASES), ids=case_id)
def test_step_array_by_array(be, name):
    c = CASES[name]
    seen, out, ref = _device(be, name)
    assert out["path"] == path_model(c["form"], c["n"], c["p"], c["k"], c["opts"], c["setup"]), out["path"]
    # the exact counts below rest on the reference's margins: the host-only file asserts them for host inputs, and
    # here they hold for what the device handed this update too (a prepared context, a second update)
    assert_margins(seen, ref)
    ratios = check_step(seen, out, ref, c["sp"], second=c["setup"] != "cold", f32=c["dtype"] == "float32")
    report("A", name, ratios)
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("name", ["data_n129_p33_k3_second_se1", "data_n129_p33_k33_second_se1"], ids=case_id)
def test_setups_describe_the_same_point(be, name):
    """Fast (one block, from the Gram state), warm (one kernel per step, products carried) and cold (factors
    projected, products recomputed) set-ups of the same point and inputs: each within the bounds of the
    reference, and pairwise within twice those bounds."""
    c = CASES[name]
    seen, fast, ref = _device(be, name)
    runs = {"fast:in_grad": fast}
    for setup in ("warm", "cold"):
        with _open(be, seen if setup == "cold" else problem(name), "float64") as ctx:
            if setup == "warm":
                ctx.dictionary_update(max_iterations=1)
                ctx.weights_update()
                assert np.array_equal(ctx.get_state()[0].T, seen.x0)
            ctx.set_dictionary_inputs(seen.H, seen.ZtZ, seen.trace)
            counts = _update(be, ctx, True, max_iterations=1)
            runs[setup] = _collect(ctx, seen, seen.x0, counts)
    worst = {}
    for setup, out in runs.items():
        assert out["path"][0] == setup, out["path"]
        # (cold: PROJ_FEAS runs on a start that is feasible to rounding; its threshold (sum_supp - 1) / m is at most
        # the column sum's distance from 1, and an entry moves by that and one rounding)
        moved = np.abs(seen.x0.astype(LD).sum(axis=0) - 1).max() + U if setup == "cold" else 0
        ratios = check_step(seen, out, ref, c["sp"], second=True, start_moved=moved)
        assert max(ratios.values()) <= 1.0, (setup, ratios)
        worst.update({setup + ":" + key: val for key, val in ratios.items()})
    for what, key in (("f_start", None), ("s1_after", "s1"), ("a0_after", "a0"), ("lambda", "lambda"), ("f_new", "f_new")):
        vals = [LD(out["f_mem"][0] if key is None else out["sc"][key]) for out in runs.values()]
        assert max(vals) - min(vals) <= 2 * LAST_BOUNDS[what], what
    report("setups", name, worst)


@pytest.mark.parametrize("name", ["data_n129_p33_k3_cold", "data_n65_p2176_k33_cold", "data_n65_p16385_k3_cold_pq0",
                                  "data_n65537_p8_k3_cold", "linear_n129_p33_k3_cold"], ids=case_id)
def test_recorded_cost(be, name):
    """The cost k_linesearch_fin records (one outer iteration with one SPG iteration) is aa_cost_from_scalars
    of the scalars that test_step_array_by_array holds to long double: the same SPG scalars bit for bit, and
    0.5 (tr - 2 s1 + a0) / n of them within 4 u of its operands."""
    c, pb = CASES[name], problem(name)
    _, out, _ = _device(be, name)
    with _options(be, c["opts"]):
        with _open(be, pb, c["dtype"]) as ctx:
            ctx.set_dictionary_inputs(pb.H, pb.ZtZ, pb.trace)
            costs = ctx.outer_iterations(1, dict(c["sp"], max_iterations=1), {})
            sc = ctx.spg_scalars()
            assert ctx.spg_path() == out["path"]
    for key in ("s1", "a0", "lambda", "f_new", "a1", "a2", "delta", "dgn", "alpha"):
        assert sc[key] == out["sc"][key], key
    tr, s1, a0 = LD(pb.trace), LD(sc["s1"]), LD(sc["a0"])
    want = (tr - 2 * s1 + a0) / 2 / pb.n
    bound = 4 * U * (abs(tr) + 2 * abs(s1) + abs(a0)) / 2 / pb.n
    assert abs(LD(costs[0]) - want) <= bound, (costs[0], float(want))
    report("cost", name, {"cost": float(abs(LD(costs[0]) - want) / bound)})


@pytest.mark.parametrize("name", ["data_n129_p33_k3_cold", "kernel_n129_p129_k17_cold"], ids=case_id)
def test_history_over_three_iterations(be, name):
    """memory = 3: f_mem after three iterations is the reference's, entry by entry, and the counts are exact."""
    c, pb = CASES[name], problem(name)
    ref = replay(pb, memory=3, max_iterations=3)
    with _open(be, pb, "float64") as ctx:
        ctx.set_dictionary_inputs(pb.H, pb.ZtZ, pb.trace)
        st = ctx.dictionary_update(memory=3, max_iterations=3)
        out = dict(f_mem=ctx.spg_array("f_mem"), x_start=pb.x0)
        assert ctx.spg_path() == path_model(c["form"], c["n"], c["p"], c["k"], {}, "cold", iterations=3)
    assert (st.n_iter, st.n_feval, st.flags) == (ref["n_iter"], ref["n_feval"], ref["flags"])
    report("history", name, check_history(pb, out, ref, 3))


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("k", [17, 33])
def test_unfused_sequence_gives_the_bits_of_the_fused_one(be, k):
    """fuse_finalize 0 against 1 with the LDS / VALU Grams: the same Grams block for block, the same order of
    the partials, the same trace routine, the same line search.  (The Gram state is not part of it: the fused
    sequence forms the accepted Gram in closed form, the unfused one from the updated P; both are held to
    (C1 X)(C1 X)' in part A.)"""
    fused, unfused = ("data_n129_p129_k%d_cold_%s" % (k, tag) for tag in ("pq0", "fu0"))
    _same_bits(_device(be, fused)[1], _device(be, unfused)[1], gram=False)


@pytest.mark.parametrize("shape", ["n129_p33_k3", "n129_p33_k33", "n65537_p8_k3"])
def test_setup_in_grad_does_not_change_a_bit(be, shape):
    a, b = (_device(be, "data_%s_second_se%d" % (shape, v))[1] for v in (0, 1))
    assert a["path"][0] == "fast:k_dict_setup" and b["path"][0] == "fast:in_grad"
    _same_bits(a, b)


C_CASES = ["data_n129_p33_k3_cold", "data_n65601_p8_k33_cold", "data_n65_p2176_k33_cold_pq0",
           "data_n129_p33_k3_second_se1", "data_n129_p129_k17_cold_fu0", "kernel_n257_p257_k33_cold"]


@pytest.mark.parametrize("name", C_CASES, ids=case_id)
def test_fresh_context_repeats_the_bits(be, name):
    again = _run(be, name)[1]
    assert again["path"] == _device(be, name)[1]["path"]
    _same_bits(_device(be, name)[1], again)


@pytest.mark.parametrize("name", C_CASES, ids=case_id)
def test_call_without_stats_gives_the_same_bits(be, name):
    """No stats struct: the tail of the iteration (g_new, x <- x + lambda d, the BB stage, the residual
    projection) goes to the side stream; the same kernels on the same numbers."""
    side = _run(be, name, stats=False)[1]
    assert side["path"] == _device(be, name)[1]["path"]
    _same_bits(_device(be, name)[1], side)


# ------------------------------------------------------------------ B
def _family_cases():
    return [(form, shape, family) for form in ("data", "kernel") for shape in B_SHAPES for family in sorted(FAMILIES)]


_ORACLE = {}


def _oracle(form, shape, family):
    """The oracle's run and its three one-ulp twins, once per (form, shape, family)."""
    from oracle import aa_oracle as orc
    key = (form, shape, family)
    if key not in _ORACLE:
        pr, kw = b_problem(form, shape), family_kwargs(family, form, shape)

        def run(X):
            return oracle_update(form, X, pr["Z"], pr["C"], pr["alpha"], **kw)
        _ORACLE[key] = (run(pr["X"]), conftest.oracle_twins(orc, run, pr["X"], "float64"))
    return _ORACLE[key]


@pytest.mark.parametrize("form,shape,family", _family_cases(),
                         ids=lambda v: v if isinstance(v, str) else "n%d_p%d_k%d" % v)
def test_parameter_families_against_the_oracle(be, form, shape, family):
    pr, kw = b_problem(form, shape), family_kwargs(family, form, shape)
    X, Z = pr["X"], pr["Z"]
    A = X if form == "data" else X.dot(X.T)
    H = X.dot(X.T.dot(Z)) if form == "data" else A.dot(Z)
    trace = float((X * X).sum()) if form == "data" else float(np.trace(A))
    with be.Context(dtype="float64") as ctx:
        ctx.set_data(A, form=be.FORM_DATA if form == "data" else be.FORM_KERNEL)
        ctx.set_state(pr["C"], Z, pr["alpha"])
        ctx.prepare()
        ctx.set_dictionary_inputs(H, Z.T.dot(Z), trace)
        st = ctx.dictionary_update(**kw)
        C = ctx.get_state()[0]
        path = ctx.spg_path()
    # (the string holds 511 characters: a long run's later entries, which repeat the first iteration's, are dropped)
    want = path_model(form, shape[0], shape[1] if form == "data" else shape[0], shape[2], {}, "cold", st.n_iter + 1)
    assert path == want[:len(path)] and len(path) >= min(len(want), 14), path
    (x, f, n_iter, n_feval, flags), twins = _oracle(form, shape, family)
    assert (st.n_iter, st.n_feval, st.flags) == (n_iter, n_feval, flags)
    floor = 1e-11 if kw["max_iterations"] == 1 else 1e-9
    tol_f = max(floor * max(1.0, abs(f)), 20 * max(abs(t[1] - f) for t in twins))
    tol_x = max(floor, 20 * max(np.abs(t[0] - x).max() for t in twins))
    err_f, err_x = abs(st.f - f), np.abs(C - x).max()
    report("B", "%s n%d_p%d_k%d %s" % ((form,) + shape + (family,)), {"f": err_f / tol_f, "dictionary": err_x / tol_x})
    assert err_f <= tol_f and err_x <= tol_x, (err_f, tol_f, err_x, tol_x)


def test_memory_17_is_refused(be):
    pr = b_problem("data", B_SHAPES[0])
    with be.Context(dtype="float64") as ctx:
        ctx.set_data(pr["X"])
        ctx.set_state(pr["C"], pr["Z"], pr["alpha"])
        ctx.prepare()
        with pytest.raises(RuntimeError, match="memory"):
            ctx.dictionary_update(memory=17, max_iterations=8)
        assert ctx.dictionary_update(memory=16, max_iterations=1).n_iter == 0
