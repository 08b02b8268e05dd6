"""KernelAA on resident data on the MI355X: the row gather ``DeviceData.take``, the fit on an implicit RBF or
polynomial kernel whose features are read from a resident block, ``transform`` of a resident block, the
per-sample kernel-form residuals ``kernel_scores``, and time-series cross-validation of a kernel model.

Whatever only moves data (take, the feature build, borrowing or widening a block) is held to the bits of the
host-array route.  Whatever computes is held to NumPy float64 within bounds built from absolute values, each
with its derivation: derived, not tuned.  Data as in tests/test_gpu_kernel_poly.py: clusters scaled so that
gamma |x|^2 <= 1 for every row, so that no kernel value cancels (polynomial values in [0, 8], RBF arguments in
[0, 4])."""
import copy
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def cdr():
    import convex_dim_red
    from convex_dim_red import _backend
    _backend.require_gpu()
    return convex_dim_red


def _clusters(rng, n, p, k, gamma):
    """The clustered data of tests/test_gpu_kernel_poly.py: gamma |x|^2 <= 1 for every row."""
    centers = rng.standard_normal((k, p)) * 2.0
    X = centers[rng.randint(k, size=n)] + 0.4 * rng.standard_normal((n, p))
    X = X / np.sqrt(gamma * (X * X).sum(axis=1).max())
    return X * (1.0 - 1e-12)


def _block(X, dtype):
    """``X`` uploaded as a resident block of ``dtype`` (what time_series_cross_validate does with a host array)."""
    from convex_dim_red import _backend
    from convex_dim_red.preprocessing import DeviceData
    ctx = _backend.Context(dtype=dtype)
    ctx.set_data(np.asarray(X, dtype=dtype), form=_backend.FORM_DATA)
    return DeviceData(ctx, X.shape, None, X.shape[1:])


def _stored(X, dtype):
    """The float64 values a block of ``dtype`` holds for ``X``."""
    return np.asarray(np.asarray(X, dtype=dtype), dtype=np.float64)


def _poly(Y, X, gamma, coef0, degree):
    b = gamma * Y.dot(X.T) + coef0
    v = b.copy()
    for _ in range(degree - 1):
        v = v * b
    return v


def _poly_diag(X, gamma, coef0, degree):
    b = gamma * (X * X).sum(axis=1) + coef0
    v = b.copy()
    for _ in range(degree - 1):
        v = v * b
    return v


def _rbf(Y, X, gamma):
    """exp(-gamma ||y - x||^2) from the differences (no cancellation)."""
    return np.exp(-gamma * ((Y[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))


def _quiet_fit(model, data, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit_transform(data, **kw)
    return model


KERNELS = {"rbf": dict(kernel="rbf"), "poly2": dict(kernel="poly", degree=2, coef0=1),
           "poly3": dict(kernel="poly", degree=3, coef0=1)}


# ---------------------------------------------------------------- take
TAKE_N, TAKE_P = 300, 37                                 # n_pad = 384; p no multiple of any padding


def _index_sets():
    rng = np.random.RandomState(12)
    mixed = np.concatenate([[5, 5, -1, -300, 299, 0, -7, 293], rng.randint(-TAKE_N, TAKE_N, size=142)])
    return {"single": np.array([17]), "129": rng.choice(TAKE_N, size=129, replace=False),
            "reversed": np.arange(TAKE_N - 1, -1, -1), "duplicates_negatives": mixed}


@pytest.fixture(scope="module")
def take_data():
    return np.random.RandomState(3).standard_normal((TAKE_N, TAKE_P)) * 3.0 + 0.5


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("which", ["single", "129", "reversed", "duplicates_negatives"])
def test_take_is_the_numpy_gather_and_pads_with_zeros(cdr, take_data, which, dtype):
    """take(idx).to_host() is owner.to_host()[idx] bit for bit (negative entries from the end); a float32 block
    widened to float64 holds exactly its float32 values; and the copy is padded like an upload: the column
    statistics of the taken block -- and, where the set has more rows than components (all but the single row),
    an ArchetypalAnalysis fit on it -- have the bits they have on a fresh upload of X[idx], which a non-zero
    padding row or column would change (the moments and every pass read whole padded tiles)."""
    idx = _index_sets()[which]
    with _block(take_data, dtype) as owner:
        want = owner.to_host()[idx]
        assert np.array_equal(want, _stored(take_data, dtype)[idx])
        with owner.take(idx) as got:
            assert got.shape == (len(idx), TAKE_P) and got.dtype == np.dtype(dtype)
            assert np.array_equal(got.to_host(), want)
            with _block(want, dtype) as fresh:
                a, b = got.column_stats(), fresh.column_stats()
                assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std) and a.n_samples == len(idx)
                if len(idx) > 3:
                    kw = dict(init="furthest_sum", random_state=2, max_iterations=6, tolerance=0, dtype=dtype,
                              require_monotonic_cost_decrease=False, dictionary_solver_kwargs=dict(max_iterations=1))
                    ma = _quiet_fit(cdr.ArchetypalAnalysis(3, **kw), got)
                    mb = _quiet_fit(cdr.ArchetypalAnalysis(3, **kw), fresh)
                    assert ma.cost == mb.cost and ma.n_iter == mb.n_iter
                    assert np.array_equal(ma.weights, mb.weights) and np.array_equal(ma.dictionary, mb.dictionary)
                    assert np.array_equal(ma.archetypes, mb.archetypes)
        if dtype == "float32":
            with owner.take(idx, dtype=np.float64) as wide:
                assert wide.dtype == np.float64
                assert np.array_equal(wide.to_host(), want)
                with _block(want, "float64") as fresh:
                    a, b = wide.column_stats(), fresh.column_stats()
                    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std)
        with owner.take(None) as whole:
            assert np.array_equal(whole.to_host(), owner.to_host())


@pytest.mark.parametrize("bad,first", [([0, TAKE_N], 1), ([-1, 3], 0), ([2, 2 ** 40, -5], 1)])
def test_an_out_of_range_index_never_reaches_the_gather(cdr, take_data, bad, first):
    """Straight to Context.set_data_take, past DeviceData's own check: error -1 (AA_ERR_ARG) that names the
    first bad index, nothing launched, and the target context still serves the data it held."""
    from convex_dim_red import _backend
    small = np.arange(12.0).reshape(4, 3)
    with _block(take_data, "float64") as owner, _backend.Context(dtype="float64") as ctx:
        ctx.set_data(small)
        with pytest.raises(RuntimeError, match=r"error -1: .*idx\[%d\] = %d " % (first, bad[first])):
            ctx.set_data_take(owner._ctx, np.array(bad))
        assert (ctx.n, ctx.p) == (4, 3)
        assert np.array_equal(ctx.get_data(), small)
        ctx.set_data_take(owner._ctx, np.array([299, 0]))             # and it still takes a good set
        assert np.array_equal(ctx.get_data(), take_data[[299, 0]])


# ---------------------------------------------------------------- fit on a resident block
FIT_N = 200


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("init", ["furthest_sum", "random"])
@pytest.mark.parametrize("kernel", ["rbf", "poly2", "poly3"])
@pytest.mark.parametrize("k", [3, 40])                   # KP = 32 / 64
@pytest.mark.parametrize("p", [1, 32, 37])               # feat_ld rounds 1 up to 2 / 32; an exact chunk; a row crossing one
def test_fit_on_a_resident_block_has_the_bits_of_the_host_fit(cdr, monkeypatch, p, k, kernel, init, dtype):
    """fit_transform(block, features=True, ...) against fit_transform(block.to_host(), ...) with equal seeds: the
    feature buffer built on the device holds the host route's bits, so every result does -- and the resident fit
    runs with the block's to_host and its context's get_data patched to raise: the training block is never
    downloaded (the support rows come back through a gathered block of their own)."""
    rng = np.random.RandomState(7 * p + k)
    gamma = 1.0 / p
    X = _clusters(rng, FIT_N, p, 5, gamma)
    host = _stored(X, dtype)
    kw = dict(features=True, gamma=gamma, **KERNELS[kernel])
    make = lambda: cdr.KernelAA(k, init=init, random_state=5, max_iterations=8, tolerance=0,     # noqa: E731
                                require_monotonic_cost_decrease=False, dictionary_solver_kwargs=dict(max_iterations=1))
    want = _quiet_fit(make(), host, **kw)

    def refuse(*args, **kwargs):
        raise AssertionError("the training block was downloaded")
    with _block(X, dtype) as block:
        monkeypatch.setattr(block, "to_host", refuse)
        monkeypatch.setattr(block._ctx, "get_data", refuse)
        got = _quiet_fit(make(), block, **kw)
    assert got.cost == want.cost and got.n_iter == want.n_iter
    assert np.array_equal(got.cost_deltas, want.cost_deltas)
    for name in ("weights", "dictionary", "alpha"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert sorted(got._transform_state) == sorted(want._transform_state)
    for key, value in want._transform_state.items():
        assert np.array_equal(np.asarray(got._transform_state[key]), np.asarray(value)), key
    copy.deepcopy(got)                                   # host arrays only


# ---------------------------------------------------------------- transform of a resident block
MODEL_P = 37


def _fitted(cdr, form, k, seed=11):
    """A model fitted on host rows (n = 200, p = 37), the training rows, 257 further rows and the kernel."""
    rng = np.random.RandomState(seed + k)
    gamma = 1.0 / MODEL_P
    XY = _clusters(rng, FIT_N + 257, MODEL_P, 5, gamma)
    X, Y = XY[:FIT_N], XY[FIT_N:]
    model = cdr.KernelAA(k, random_state=4, max_iterations=8, tolerance=0, require_monotonic_cost_decrease=False,
                         dictionary_solver_kwargs=dict(max_iterations=1))
    if form == "linear":
        _quiet_fit(model, X, features=True)
    elif form == "explicit":
        _quiet_fit(model, _poly(X, X, gamma, 1.0, 2))
    else:
        _quiet_fit(model, X, features=True, gamma=gamma, **KERNELS[form])
    model.max_iterations = 40
    return model, X, Y, gamma


@pytest.fixture(scope="module")
def fitted(cdr):
    cache = {}

    def get(form, k):
        if (form, k) not in cache:
            cache[form, k] = _fitted(cdr, form, k)
        model, X, Y, gamma = cache[form, k]
        return copy.deepcopy(model), X, Y, gamma
    return get


def _poly_diag_bound(Y, gamma, degree):
    """|d_t(device) - d_t(host)| <= 4 (p + 2 degree) 2^-53 kappa(|y_t|, |y_t|): a sum of p squares in another order
    and degree multiplications on either side, every term non-negative."""
    return 4.0 * (Y.shape[1] + 2 * degree) * U * _poly_diag(np.abs(Y), gamma, 1.0, degree)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", ["linear", "rbf", "poly3"])
@pytest.mark.parametrize("m", [70, 257])
def test_transform_of_a_resident_block(cdr, fitted, m, form, dtype):
    """transform(block) against transform(block.to_host()) from equal random states: a float64 block is borrowed,
    a float32 one widened exactly, the calls and the draws are the same -- the weights are bit-identical, and so is
    the cost for the linear and the RBF kernel.  The polynomial cost takes kappa(y, y) from row norms summed on
    the device where the host route sums on the host, the only place where the two differ: within
    0.5 mean_t |delta d_t|."""
    a, _, Y, gamma = fitted(form, 3)
    b = copy.deepcopy(a)
    Y = Y[:m]
    with _block(Y, dtype) as block:
        Wa, ca = a.transform(block)
        Wb, cb = b.transform(_stored(Y, dtype))
    assert Wa.shape == (m, 3)
    assert np.array_equal(Wa, Wb)
    assert a.random_state.randint(1 << 30) == b.random_state.randint(1 << 30)
    if form == "poly3":
        bound = 0.5 * _poly_diag_bound(_stored(Y, dtype), gamma, 3).mean()
        print("transform m %d %s %s: |cost - cost(host)| %.3e, bound %.3e" % (m, form, dtype, abs(ca - cb), bound))
        assert abs(ca - cb) <= bound
    else:
        assert ca == cb


# ---------------------------------------------------------------- kernel_scores
def _reference_residuals(model, X, Yh, W, gamma, form):
    """NumPy float64 on the explicit kernel, with the model's own A: r = d - 2 w.(kappa(Y, X) D') + w' A w, its
    magnitude |d| + 2 sum_j w_j (|kappa| |D'|)_tj + sum_ij w_i |A_ij| w_j, d, and the length of the longest
    chain of roundings behind an element."""
    state = model._transform_state
    A = state["A"]
    D = np.asarray(model.alpha)[:, None] * model.dictionary
    p, k = Yh.shape[1], model.n_components
    if form == "linear":
        cross, d, degree, s = Yh.dot(X.T), (Yh * Yh).sum(axis=1), 0, X.shape[0]
    elif form == "rbf":
        cross, d, degree, s = _rbf(Yh, X, gamma), np.ones(len(Yh)), 0, len(state["support"])
    else:
        degree = state["degree"]
        cross, d, s = _poly(Yh, X, gamma, 1.0, degree), _poly_diag(Yh, gamma, 1.0, degree), len(state["support"])
    XW = cross.dot(D.T)
    r = d - 2.0 * (W * XW).sum(axis=1) + np.einsum("ti,ij,tj->t", W, A, W)
    mag = np.abs(d) + 2.0 * (W * np.abs(cross).dot(np.abs(D.T))).sum(axis=1) + np.einsum("ti,ij,tj->t", W, np.abs(A), W)
    length = p + 2 * degree + s + k * k + 4
    if form == "rbf":
        # the device forms the argument as gamma (|y|^2 + |x|^2 - 2 y.x): three sums of p terms whose absolute
        # values add up to at most gamma (|y| + |x|)^2 <= 4, so the argument is off by at most 4 (p + 4) 2^-53
        # absolutely, which is the relative error it leaves in exp(-argument)
        length += 4 * (p + 4)
    return r, d, mag, length


@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("form", ["linear", "rbf", "poly2", "poly3"])
def test_kernel_scores_against_numpy(cdr, fitted, form, k):
    """m = 257 (two blocks of 256 samples, the second holding one), from a host array, a float64 block and a
    float32 block: sample_sse and diagonal element-wise against NumPy, within 4 L 2^-53 |terms| in the manner of
    _product_bound -- L = p + 2 degree + s + k^2 + 4: a dot product of p terms and the power behind every kernel
    value, a sum over the s support rows, the k^2 terms of w' A w, and the four operations that combine them
    (for RBF plus the argument's error, see _reference_residuals); cost, rmse and explained from the returned
    vectors by the documented formulas (the device sums in another order: m 2^-53 sum |.|); the cost against
    transform's; the same bits from a second call."""
    model, X, Y, gamma = fitted(form, k)
    W, cost = model.transform(Y)
    m = len(Y)
    for dtype in (None, "float64", "float32"):
        Yh = Y if dtype is None else _stored(Y, dtype)
        if dtype is None:
            s, again = model.kernel_scores(Y), model.kernel_scores(Y, weights=W)
        else:
            with _block(Y, dtype) as block:
                s, again = model.kernel_scores(block, weights=W), model.kernel_scores(block)
        assert isinstance(s, cdr.KernelScores) and s.sample_sse.shape == (m,) and s.diagonal.shape == (m,)
        for name in ("cost", "rmse", "explained"):
            assert getattr(s, name) == getattr(again, name), name
        assert np.array_equal(s.sample_sse, again.sample_sse) and np.array_equal(s.diagonal, again.diagonal)
        r, d, mag, length = _reference_residuals(model, X, Yh, W, gamma, form)
        bound = 4.0 * length * U * mag
        print("kernel_scores %s k %d %s: max |r - want| / bound %.3f, min r %.3e"
              % (form, k, dtype, (np.abs(s.sample_sse - r) / bound).max(), s.sample_sse.min()))
        assert np.all(np.abs(s.sample_sse - r) <= bound)
        if form == "rbf":
            assert np.array_equal(s.diagonal, d)
        else:
            degree = model._transform_state.get("degree", 0)
            assert np.all(np.abs(s.diagonal - d) <= 4.0 * (Yh.shape[1] + 2 * degree) * U * np.abs(d))
        sum_r, sum_d = s.sample_sse.sum(), s.diagonal.sum()
        tol_r, tol_d = m * U * np.abs(s.sample_sse).sum(), m * U * sum_d
        assert abs(s.cost - 0.5 * sum_r / m) <= 0.5 * tol_r / m
        assert abs(s.rmse ** 2 * m - max(sum_r, 0.0)) <= tol_r + 4 * U * abs(sum_r)
        assert abs(s.explained - (1.0 - sum_r / sum_d)) <= (tol_r + abs(sum_r) / sum_d * tol_d) / sum_d + 2 * U
        if dtype is None:
            print("    cost %.17g, transform's %.17g, |diff| / (2^-53 sum |terms|) %.3f"
                  % (s.cost, cost, abs(s.cost - cost) / (U * mag.sum())))
            assert abs(s.cost - cost) <= m * U * mag.sum() / m


def test_kernel_scores_of_a_linear_model_against_score(cdr, fitted):
    """A cross-check without cancellation: for a linear-features model r_t is the data-space residual
    |y_t - w_t D X|^2 that score() sums directly.  Within the bound of the kernel form (score's own error is a
    sum of p non-negative squares, far inside it)."""
    model, X, Y, gamma = fitted("linear", 3)
    W, _ = model.transform(Y)
    _, _, mag, length = _reference_residuals(model, X, Y, W, gamma, "linear")
    got, want = model.kernel_scores(Y).sample_sse, model.score(Y).sample_sse
    print("linear: max |kernel_scores - score| / bound %.3f" % (np.abs(got - want) / (4.0 * length * U * mag)).max())
    assert np.all(np.abs(got - want) <= 4.0 * length * U * mag)
    with _block(Y, "float64") as block:
        assert np.array_equal(model.kernel_scores(block).sample_sse, got)


@pytest.mark.parametrize("k", [3, 40])
def test_kernel_scores_of_an_explicit_kernel_model(cdr, fitted, k):
    """A model fitted on an explicit kernel matrix: the cross kernel and the diagonal come from the caller; against
    NumPy with a sum over all n training columns in the place of the support."""
    model, X, Y, gamma = fitted("explicit", k)
    cross, diag = _poly(Y, X, gamma, 1.0, 2), _poly_diag(Y, gamma, 1.0, 2)
    W, cost = model.transform(cross, diagonal=diag)
    s = model.kernel_scores(cross, diagonal=diag)
    A = model._transform_state["A"]
    D = np.asarray(model.alpha)[:, None] * model.dictionary
    r = diag - 2.0 * (W * cross.dot(D.T)).sum(axis=1) + np.einsum("ti,ij,tj->t", W, A, W)
    mag = diag + 2.0 * (W * cross.dot(D.T)).sum(axis=1) + np.einsum("ti,ij,tj->t", W, np.abs(A), W)
    bound = 4.0 * (X.shape[0] + k * k + 4) * U * mag
    print("explicit k %d: max |r - want| / bound %.3f" % (k, (np.abs(s.sample_sse - r) / bound).max()))
    assert np.all(np.abs(s.sample_sse - r) <= bound)
    assert np.array_equal(s.diagonal, diag)
    assert abs(s.cost - cost) <= len(Y) * U * mag.sum() / len(Y)


# ---------------------------------------------------------------- cross-validation
CV = dict(n=120, p=7, folds=3, n_init=2, k=3)


def _cv_data():
    return _clusters(np.random.RandomState(8), CV["n"], CV["p"], 4, 0.25)


@pytest.mark.parametrize("kernel", ["rbf", "poly2"])
def test_cross_validation_of_a_kernel_model(cdr, kernel):
    """time_series_cross_validate with a KernelAA factory against the drivers' loop written on host slices with
    the same shared RandomState: fit_transform(X[:stop], features=True, ...) n_init times keeping the first
    lowest cost, kernel_scores of the prefix, transform(X[test]), kernel_scores of the test block.  Bit-identical
    per fold: training_cost, n_iter, both weights, the RMSEs and the explained fractions; test_cost bit-identical
    for RBF and within the polynomial diagonal's bound for poly."""
    X = _cv_data()
    fit_kwargs = dict(features=True, gamma=0.25, **KERNELS[kernel])

    def factory(rs):
        return lambda: cdr.KernelAA(CV["k"], init="furthest_sum", random_state=rs, max_iterations=30, tolerance=1e-6,
                                    dictionary_solver_kwargs=dict(max_iterations=1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rs_got, rs_want = np.random.RandomState(9), np.random.RandomState(9)
        got = cdr.time_series_cross_validate(factory(rs_got), X, n_folds=CV["folds"],
                                             n_init=CV["n_init"], dtype="float64", fit_kwargs=fit_kwargs)
        make = factory(rs_want)
        for i, (stop, lo, hi) in enumerate(cdr.time_series_folds(CV["n"], CV["folds"])):
            best = None
            for _ in range(CV["n_init"]):
                model = make()
                model.fit_transform(X[:stop], **fit_kwargs)
                if best is None or model.cost < best.cost:
                    best = copy.deepcopy(model)
            assert got["training_cost"][i] == best.cost and got["n_iter"][i] == best.n_iter
            assert np.array_equal(got["training_weights"][i], best.weights)
            train = best.kernel_scores(X[:stop])
            assert got["training_rmse"][i] == train.rmse and got["training_explained"][i] == train.explained
            W, cost = best.transform(X[lo:hi])
            assert np.array_equal(got["test_weights"][i], W)
            if kernel == "rbf":
                assert got["test_cost"][i] == cost
            else:
                bound = 0.5 * _poly_diag_bound(X[lo:hi], 0.25, 2).mean()
                print("fold %d: |test_cost - host| %.3e, bound %.3e" % (i, abs(got["test_cost"][i] - cost), bound))
                assert abs(got["test_cost"][i] - cost) <= bound
            test = best.kernel_scores(X[lo:hi])
            assert got["test_rmse"][i] == test.rmse and got["test_explained"][i] == test.explained
            assert 0.0 < test.rmse and test.explained <= 1.0
    assert len(got["models"]) == CV["folds"]
    assert rs_got.randint(1 << 30) == rs_want.randint(1 << 30)         # the same draws were made


def test_cross_validation_without_fit_kwargs_is_unchanged(cdr):
    """fit_kwargs=None: an ArchetypalAnalysis factory gets what the explicit loop gives (the comparison of
    tests/test_gpu_validation.py), and no feature-space keys appear."""
    X = _cv_data()

    def factory(rs):
        return lambda: cdr.ArchetypalAnalysis(CV["k"], init="furthest_sum", random_state=rs, max_iterations=30,
                                              tolerance=1e-6, dtype="float64",
                                              dictionary_solver_kwargs=dict(max_iterations=1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = cdr.time_series_cross_validate(factory(np.random.RandomState(9)), X, n_folds=CV["folds"],
                                             n_init=CV["n_init"], dtype="float64")
        make = factory(np.random.RandomState(9))
        for i, (stop, lo, hi) in enumerate(cdr.time_series_folds(CV["n"], CV["folds"])):
            best = None
            for _ in range(CV["n_init"]):
                model = make()
                model.fit_transform(X[:stop])
                if best is None or model.cost < best.cost:
                    best = copy.deepcopy(model)
            assert got["training_cost"][i] == best.cost and got["n_iter"][i] == best.n_iter
            assert np.array_equal(got["training_weights"][i], best.weights)
            assert got["training_rmse"][i] == best.score(X[:stop]).rmse
            W, cost = best.transform(X[lo:hi])
            assert np.array_equal(got["test_weights"][i], W) and got["test_cost"][i] == cost
            assert got["test_rmse"][i] == best.score(X[lo:hi]).rmse
    assert "training_explained" not in got and "test_explained" not in got
