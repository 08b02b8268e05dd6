"""Reconstruction scores, row blocks of resident data and the drivers' cross-validation loop on the
MI355X (aa_gpnh_residual_scores, aa_set_data_rows, convex_dim_red.validation).

The tolerance of every comparison of sums of squares is DERIVED from the inputs (``_reference``): with
u = 2^-53 every entry of R = X - Z W' carries at most (k + 2) u (|x| + sum_j |z_j| |w_j|) of rounding in
either evaluation (the k-term product, the subtraction), so a sum S = sum r^2 over N terms may differ by
at most ``2 sum |r| (k + 2) u (|x| + |z|.|w|) + N u S``; the tests allow 4 x that (two evaluations, and
slack for the order of the summation tree)."""
import itertools
import warnings
from copy import deepcopy

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _reference(Xd, Z, Wt):
    """float64 NumPy sums of squares of R = Xd - Z Wt (Wt: k x p) and their rounding bounds:
    ``(col, row, sse), (col_bound, row_bound, sse_bound)``."""
    n, p = Xd.shape
    k = Z.shape[1]
    R = Xd - Z.dot(Wt)
    E = (k + 2) * U * (np.abs(Xd) + np.abs(Z).dot(np.abs(Wt)))
    T = 2.0 * np.abs(R) * E
    R2 = R * R
    col, row, sse = R2.sum(axis=0), R2.sum(axis=1), R2.sum()
    bounds = (T.sum(axis=0) + n * U * col, T.sum(axis=1) + p * U * row, T.sum() + n * p * U * sse)
    return (col, row, sse), bounds


def _simplex_rows(rng, n, k):
    Z = rng.uniform(size=(n, k)) ** 3
    return Z / Z.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 257, 1610])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_scores_against_float64_numpy(dtype, n):
    rng = np.random.RandomState(100 + n)
    combos = list(itertools.product((False, True), repeat=3))
    worst = 0.0
    with _backend.Context(dtype=dtype) as ctx:
        for p in (1, 127, 128, 129, 1000):
            X = rng.standard_normal((n, p)) * rng.uniform(0.1, 5.0, size=p) + rng.uniform(-2.0, 2.0, size=p)
            ctx.set_data(X)
            Xd = ctx.get_data()
            if dtype == "float64":
                assert np.array_equal(Xd, X)
            for k in (1, 3, 5, 10, 32, 33, 64):
                Z = _simplex_rows(rng, n, k)
                W = rng.standard_normal((p, k))
                ctx.gpnh_set_factors(k, W=W, Z=Z)
                (col_w, row_w, sse_w), (col_b, row_b, sse_b) = _reference(Xd, Z, np.ascontiguousarray(W.T))
                col, row, sse = ctx.gpnh_residual_scores()
                msg = "dtype=%s n=%d p=%d k=%d" % (dtype, n, p, k)
                assert col.shape == (p,) and row.shape == (n,)
                ratio = max((np.abs(col - col_w) / col_b).max(), (np.abs(row - row_w) / row_b).max(),
                            abs(sse - sse_w) / sse_b)
                worst = max(worst, ratio)
                assert np.all(np.abs(col - col_w) <= 4 * col_b), msg
                assert np.all(np.abs(row - row_w) <= 4 * row_b), msg
                assert abs(sse - sse_w) <= 4 * sse_b, msg
                # what exists: the residual cost of the same context
                cost = ctx.gpnh_residual_cost()
                assert abs(sse / (2 * n) - cost) <= 4 * sse_b / (2 * n), msg
                # nullable outputs, every combination; identical bits on every call
                for want_col, want_row, want_tot in combos:
                    c2, r2, t2 = ctx.gpnh_residual_scores(columns=want_col, samples=want_row, total=want_tot)
                    assert (c2 is None) == (not want_col) and (r2 is None) == (not want_row)
                    assert (t2 is None) == (not want_tot)
                    assert c2 is None or np.array_equal(c2, col), msg
                    assert r2 is None or np.array_equal(r2, row), msg
                    assert t2 is None or t2 == sse, msg
    print("largest error / bound over the cases of n=%d, %s: %.3f (allowed 4)" % (n, dtype, worst))


def test_scores_entry_point_refusals():
    rng = np.random.RandomState(0)
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(rng.standard_normal((20, 6)))
        with pytest.raises(RuntimeError, match="-3"):                 # AA_ERR_STATE: no factors yet
            ctx.gpnh_residual_scores()
        ctx.gpnh_set_factors(2, Z=_simplex_rows(rng, 20, 2))
        with pytest.raises(RuntimeError, match="-3"):                 # weights but no dictionary
            ctx.gpnh_residual_scores()
    K = rng.standard_normal((12, 12))
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(K.dot(K.T), form=_backend.FORM_KERNEL)
        with pytest.raises(RuntimeError, match="-3"):                 # kernel form
            ctx.gpnh_residual_scores()
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_rbf_features(rng.standard_normal((12, 3)), 0.5)
        with pytest.raises(RuntimeError, match="-3"):                 # implicit kernel
            ctx.gpnh_residual_scores()


def _problem(n=300, p=40, k=4, seed=0):
    rng = np.random.RandomState(seed)
    basis = rng.uniform(size=(k, p))
    X = _simplex_rows(rng, n, k).dot(basis) + 0.01 * rng.standard_normal((n, p))
    Y = _simplex_rows(rng, 90, k).dot(basis) + 0.01 * rng.standard_normal((90, p))
    return X, Y


AA_KW = dict(tolerance=1e-6, max_iterations=60, dictionary_solver_kwargs=dict(max_iterations=1))


def _cost_bound(Xd, weights, components):
    (_, _, sse), (_, _, sse_b) = _reference(Xd, weights, components)
    m = Xd.shape[0]
    return sse / (2 * m), 4 * sse_b / (2 * m)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_score_agrees_with_transform_cost(dtype):
    X, Y = _problem()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.ArchetypalAnalysis(4, init="furthest_sum", random_state=0, dtype=dtype, **AA_KW)
        model.fit_transform(X)
        kmodel = cdr.KernelAA(4, init="furthest_sum", random_state=0, dtype=dtype, **AA_KW)
        kmodel.fit_transform(X, features=True)
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(Y)
        dd = cdr.DeviceData(ctx, Y.shape, None, Y.shape[1:])
        Yd = dd.to_host()
        # host array (float64: a float64 context, as transform uses) and DeviceData (the context's dtype)
        for data, resident in ((Y, Y), (dd, Yd)):
            weights, cost = model.transform(data)
            s = model.score(data)
            want, bound = _cost_bound(resident, weights, model.archetypes)
            print("AA %s %s: score %.17g transform %.17g numpy %.17g bound %.3g"
                  % (dtype, type(data).__name__, s.cost, cost, want, bound))
            assert abs(s.cost - cost) <= bound
            assert abs(s.cost - want) <= bound
            recon = model.inverse_transform(weights)
            rmse = np.sqrt(((resident - recon) ** 2).mean(axis=0)).mean()
            assert abs(s.rmse - rmse) <= _rmse_bound(resident, model, weights)
            pooled = np.sqrt(((resident - recon) ** 2).mean())
            assert abs(s.rmse_pooled - pooled) <= bound / (2 * want) * pooled + 8 * U * pooled
            assert s.column_sse.shape == (Y.shape[1],) and s.sample_sse.shape == (Y.shape[0],)
            # explicit weights, and no draws
            state = model.random_state.get_state()[1].copy()
            s2 = model.score(data, weights=weights)
            assert s2.cost == s.cost and np.array_equal(s2.column_sse, s.column_sse)
            assert np.array_equal(model.random_state.get_state()[1], state)
        weights, cost = kmodel.transform(Y)
        for data, resident in ((Y, Y), (dd, Yd)):
            s = kmodel.score(data)
            want, bound = _cost_bound(resident, weights, kmodel._transform_state["archetypes"])
            print("KernelAA %s %s: score %.17g transform %.17g numpy %.17g bound %.3g"
                  % (dtype, type(data).__name__, s.cost, cost, want, bound))
            assert abs(s.cost - want) <= bound
            if data is Y:
                assert abs(s.cost - cost) <= bound           # transform ran on the same float64 upload


@pytest.mark.parametrize("lambda_W", [0, 1])
def test_gpnh_score_is_the_data_term(lambda_W):
    X, Y = _problem(seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.GPNHConvexCoding(4, lambda_W=lambda_W, init="random", random_state=0, tolerance=1e-6,
                                     max_iterations=40)
        model.fit_transform(X)
        with _backend.Context(dtype="float64") as ctx:
            ctx.set_data(Y)
            dd = cdr.DeviceData(ctx, Y.shape, None, Y.shape[1:])
            for data in (Y, dd):
                weights, _ = model.transform(data)
                s = model.score(data)
                want, bound = _cost_bound(Y, weights, np.ascontiguousarray(model.dictionary.T))
                direct = 0.5 * np.linalg.norm(Y - weights.dot(model.dictionary.T)) ** 2 / Y.shape[0]
                print("GPNH lambda_W=%g %s: score %.17g numpy %.17g bound %.3g"
                      % (lambda_W, type(data).__name__, s.cost, direct, bound))
                assert abs(s.cost - want) <= bound and abs(s.cost - direct) <= bound
                recon = model.inverse_transform(weights)
                rmse = np.sqrt(((Y - recon) ** 2).mean(axis=0)).mean()
                assert abs(s.rmse - rmse) <= _rmse_bound(Y, model, weights)


def _field(dtype):
    rng = np.random.RandomState(7)
    n_time, n_lat, n_lon = 120, 6, 8
    lat = np.linspace(-75.0, 75.0, n_lat)
    field = rng.standard_normal((n_time, n_lat, n_lon))
    field[:, rng.uniform(size=(n_lat, n_lon)) < 0.2] = np.nan          # always missing
    field[rng.randint(n_time), 2, 3] = np.nan                          # missing once: dropped as well
    weights = (np.cos(np.deg2rad(lat)).clip(0.0, 1.0) ** 0.5)[:, np.newaxis]
    return (field.astype(np.float32) if dtype == "float32" else field), weights


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_row_blocks_of_resident_data(dtype):
    raw, weights = _field(dtype)
    dd = cdr.weight_and_flatten_on_device(raw, weights, dtype=dtype)
    full = dd.to_host()
    n, p = dd.shape
    assert p < raw.shape[1] * raw.shape[2] and full.shape == (n, p)
    for a, b in ((0, n), (0, 1), (n - 1, n), (17, 93), (0, 64), (64, 120)):
        with dd.rows(a, b) as block:
            assert block.shape == (b - a, p) and block.dtype == dd.dtype
            assert block.valid is dd.valid and block.original_shape == dd.original_shape
            assert np.array_equal(block.to_host(), full[a:b])
    with dd.rows(slice(10, 100)) as block, block.rows(slice(5, None)) as inner, inner.rows(0, 30) as third:
        assert np.array_equal(inner.to_host(), full[15:100])
        assert np.array_equal(third.to_host(), full[15:45])
    with pytest.raises(ValueError):
        dd.rows(5, n + 1)
    t = 97
    train = dd.rows(0, t)
    host = full[:t]                  # float64 holding the resident values: uploaded into a context of `dtype`
    dd.close()                                                          # the block owns its memory
    with pytest.raises(RuntimeError):
        dd.rows(0, 5)
    assert np.array_equal(train.to_host(), full[:t])
    k = 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for init in ("random", "furthest_sum"):
            kw = dict(init=init, tolerance=1e-6, max_iterations=40, dtype=dtype,
                      dictionary_solver_kwargs=dict(max_iterations=1))
            a = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
            Wa = a.fit_transform(train)
            b = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
            Wb = b.fit_transform(host)
            assert np.array_equal(Wa, Wb) and np.array_equal(a.dictionary, b.dictionary)
            assert a.cost == b.cost and a.n_iter == b.n_iter and list(a.cost_deltas) == list(b.cost_deltas)
            assert np.array_equal(a.archetypes, b.archetypes)
            gkw = dict(lambda_W=0.5, init=init, tolerance=1e-6, max_iterations=30, dtype=dtype)
            g = cdr.GPNHConvexCoding(k, random_state=0, **gkw)
            Zg = g.fit_transform(train)
            g2 = cdr.GPNHConvexCoding(k, random_state=0, **gkw)
            Zh = g2.fit_transform(host)
            assert np.array_equal(Zg, Zh) and np.array_equal(g.dictionary, g2.dictionary)
            assert g.cost == g2.cost and g.n_iter == g2.n_iter and list(g.cost_deltas) == list(g2.cost_deltas)
    train.close()


def _drivers_loop(make_model, X, n_folds, n_init):
    """bin/run_hadisst_aa.py:215-244 with fit_aa_model (:149-174), written out with the public API on
    host slices."""
    out = dict(training_cost=[], training_rmse=[], test_cost=[], test_rmse=[], n_iter=[], weights=[],
               test_weights=[], bounds=[])
    for train_stop, test_start, test_stop in cdr.time_series_folds(X.shape[0], n_folds):
        train, test = X[:train_stop], X[test_start:test_stop]
        best = None
        for _ in range(n_init):
            model = make_model()
            model.fit_transform(train)
            if best is None or model.cost < best.cost:
                best = deepcopy(model)
        recon = best.inverse_transform(best.weights)
        out["training_cost"].append(best.cost)
        out["n_iter"].append(best.n_iter)
        out["weights"].append(best.weights.copy())
        out["training_rmse"].append(np.sqrt(((train - recon) ** 2).mean(axis=0)).mean())
        b_train = _rmse_bound(train, best, best.weights)
        test_weights, test_cost = best.transform(test)
        recon = best.inverse_transform(test_weights)
        out["test_cost"].append(test_cost)
        out["test_weights"].append(test_weights.copy())
        out["test_rmse"].append(np.sqrt(((test - recon) ** 2).mean(axis=0)).mean())
        out["bounds"].append((b_train, _rmse_bound(test, best, test_weights)))
    return out


def _rmse_bound(X, model, weights):
    """What 4 x the bound on the column sums of squares allows the mean column RMSE to move:
    d sqrt(S / m) = dS / (2 sqrt(S m))."""
    comps = model.archetypes if hasattr(model, "archetypes") else np.ascontiguousarray(model.dictionary.T)
    (col, _, _), (col_b, _, _) = _reference(X, weights, comps)
    m = X.shape[0]
    return (4 * col_b / (2 * np.sqrt(col * m))).mean() + 8 * U * np.sqrt(col / m).mean()


def _cv_problem(which):
    if which == "aa":                                                   # the C1 recipe
        rng = np.random.RandomState(0)
        basis = rng.uniform(size=(3, 50))
        Z = cdr.right_stochastic_matrix((200, 3), random_state=rng)
        return Z.dot(basis) + 0.01 * rng.randn(200, 50)
    rng = np.random.RandomState(2)
    return _simplex_rows(rng, 600, 4).dot(rng.standard_normal((4, 40))) + 0.05 * rng.standard_normal((600, 40))


@pytest.mark.parametrize("init", ["random", "furthest_sum"])
@pytest.mark.parametrize("n_init", [1, 3])
@pytest.mark.parametrize("which", ["aa", "gpnh"])
def test_cross_validation_is_the_drivers_loop(which, n_init, init):
    X = _cv_problem(which)
    n_folds = 4

    def factory(rng):
        if which == "aa":                                               # the drivers' settings (fit_aa_model)
            return lambda: cdr.ArchetypalAnalysis(n_components=3, delta=0, init=init, tolerance=1e-6,
                                                  max_iterations=1000, random_state=rng,
                                                  dictionary_solver_kwargs=dict(max_iterations=1))
        return lambda: cdr.GPNHConvexCoding(n_components=4, lambda_W=0.1, init=init, tolerance=1e-6,
                                            max_iterations=1000, random_state=rng)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rng_want = np.random.RandomState(11)
        want = _drivers_loop(factory(rng_want), X, n_folds, n_init)
        rng_host = np.random.RandomState(11)
        got_host = cdr.time_series_cross_validate(factory(rng_host), X, n_folds=n_folds, n_init=n_init)
        rng_dev = np.random.RandomState(11)
        with _backend.Context(dtype="float64") as ctx:
            ctx.set_data(X)
            dd = cdr.DeviceData(ctx, X.shape, None, X.shape[1:])
            got_dev = cdr.time_series_cross_validate(factory(rng_dev), dd, n_folds=n_folds, n_init=n_init)
    for got, rng in ((got_host, rng_host), (got_dev, rng_dev)):
        assert got["folds"] == cdr.time_series_folds(X.shape[0], n_folds)
        assert got["training_cost"] == want["training_cost"]            # bit-identical, fold by fold
        assert got["test_cost"] == want["test_cost"]
        assert got["n_iter"] == want["n_iter"]
        assert len(got["models"]) == n_folds
        for f in range(n_folds):
            assert np.array_equal(got["training_weights"][f], want["weights"][f])
            assert np.array_equal(got["test_weights"][f], want["test_weights"][f])
            assert np.array_equal(got["models"][f].weights, want["test_weights"][f])
            b_train, b_test = want["bounds"][f]
            assert abs(got["training_rmse"][f] - want["training_rmse"][f]) <= b_train
            assert abs(got["test_rmse"][f] - want["test_rmse"][f]) <= b_test
        state, ref = rng.get_state(), rng_want.get_state()
        assert state[0] == ref[0] and np.array_equal(state[1], ref[1]) and state[2:] == ref[2:]
    for key in ("training_cost", "training_rmse", "test_cost", "test_rmse", "n_iter"):
        assert got_host[key] == got_dev[key], key                       # host-array and DeviceData input
