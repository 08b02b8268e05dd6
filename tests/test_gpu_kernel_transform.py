"""KernelAA.transform on the MI355X: weights and cost of new samples for a fitted kernel model, in each of
the three forms a KernelAA can be fitted in (explicit kernel matrix, linear features, RBF features), against
the oracle's per-sample QPs (qp_batch with A = D K D', B = D kappa(X, Y), D = diag(alpha) C); the cross RBF
product on its own against NumPy; state and errors."""
import copy
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cdr():
    import convex_dim_red
    from convex_dim_red import _backend
    _backend.require_gpu()
    return convex_dim_red


@pytest.fixture(scope="module")
def orc():
    from oracle import aa_oracle
    return aa_oracle


def _rbf(Y, X, gamma):
    """exp(-gamma ||y - x||^2) from the differences (no cancellation), in row blocks of Y."""
    step = max(1, 4000000 // (X.shape[0] * X.shape[1]))
    out = np.empty((Y.shape[0], X.shape[0]))
    for i in range(0, Y.shape[0], step):
        out[i:i + step] = np.exp(-gamma * ((Y[i:i + step, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    return out


def _clusters(rng, n, p, k=4, spread=0.5):
    centers = 2.0 * rng.standard_normal((k, p))
    return centers[rng.randint(k, size=n)] + spread * rng.standard_normal((n, p))


def _oracle_transform(orc, model, K, cross, diag, rs, max_iterations, wkw=None):
    """What KernelAA.transform computes, in the oracle: K the training kernel, cross = kappa(X, Y) (n x m),
    diag = kappa(y, y), rs a copy of the model's generator."""
    D = model.alpha[:, None] * model.dictionary
    A = D.dot(K).dot(D.T)
    B = D.dot(cross)                                    # k x m, b_y = -B[:, y]
    m = cross.shape[1]
    Z0 = orc.right_stochastic_matrix((m, model.n_components), rs)
    kw = dict(wkw or {})
    kw["max_iterations"] = max_iterations
    W = orc.qp_batch(A, B, Z0, "kn", **kw)
    cost = 0.5 * (diag.sum() - 2 * np.sum(W * B.T) + np.einsum("ti,ij,tj->", W, A, W)) / m
    return W, cost


@pytest.mark.parametrize("delta", [0.0, 0.1])
def test_explicit_kernel_against_the_oracle(cdr, orc, delta):
    rng = np.random.RandomState(3)
    n, m, p, k, gamma = 150, 60, 4, 4, 0.3
    X = _clusters(rng, n, p)
    Y = _clusters(rng, m, p)
    K = _rbf(X, X, gamma)
    cross = _rbf(Y, X, gamma)                           # kappa(Y, X), m x n
    diag = np.ones(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.KernelAA(k, delta=delta, random_state=1, max_iterations=40, tolerance=1e-9)
        model.fit_transform(K)
    D = model.alpha[:, None] * model.dictionary
    assert np.abs(model._transform_state["A"] - D.dot(K).dot(D.T)).max() < 1e-13
    # a fixed, small pass count: rounding level
    fixed = copy.deepcopy(model)
    fixed.max_iterations = 5
    rs = copy.deepcopy(fixed.random_state)
    W, cost = fixed.transform(cross, diagonal=diag)
    wW, wcost = _oracle_transform(orc, model, K, cross.T, diag, rs, 5)
    assert np.abs(W - wW).max() <= 1e-10
    assert abs(cost - wcost) <= 1e-12 * abs(wcost)
    # the defaults (max_iterations passes at most): the bounds of the known-answer transform leg
    rs = copy.deepcopy(model.random_state)
    W, cost = model.transform(cross, diagonal=diag)
    wW, wcost = _oracle_transform(orc, model, K, cross.T, diag, rs, model.max_iterations)
    assert np.abs(W - wW).max() < 1e-5
    assert abs(cost - wcost) < 1e-8
    assert np.all(W >= 0) and np.abs(W.sum(axis=1) - 1).max() < 1e-12


def test_linear_features_match_the_explicit_path_and_the_residual(cdr):
    rng = np.random.RandomState(4)
    n, m, p, k = 200, 50, 7, 5
    X = _clusters(rng, n, p, k=5)
    Y = _clusters(rng, m, p, k=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.KernelAA(k, delta=0.05, random_state=2, max_iterations=30)
        model.fit_transform(X, features=True)
    D = model.alpha[:, None] * model.dictionary
    DX = D.dot(X)
    assert np.abs(model._transform_state["archetypes"] - DX).max() < 1e-12 * np.abs(DX).max()
    for passes in (5, None):
        lin = copy.deepcopy(model)
        if passes:
            lin.max_iterations = passes
        exp = copy.deepcopy(lin)                        # same factors, same draws, explicit form
        exp._transform_state = dict(form="kernel", n_samples=n, A=lin._transform_state["A"])
        W, cost = lin.transform(Y)
        We, coste = exp.transform(Y.dot(X.T), diagonal=(Y * Y).sum(axis=1))
        host = 0.5 * np.linalg.norm(Y - W.dot(DX)) ** 2 / m
        assert abs(cost - host) <= 1e-10 * host
        if passes:
            assert np.abs(W - We).max() <= 1e-10
            assert abs(cost - coste) <= 1e-10 * host
        else:
            assert np.abs(W - We).max() < 1e-5 and abs(cost - coste) < 1e-8


def _rbf_model(cdr, X, k, gamma, sparse_support=None, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.KernelAA(k, random_state=seed, max_iterations=3, tolerance=0,
                             require_monotonic_cost_decrease=False)
        if sparse_support is None:
            model.fit_transform(X, features=True, kernel="rbf", gamma=gamma)
        else:                                           # a dictionary on a few training rows only, kept
            n = X.shape[0]
            C = np.zeros((k, n))
            rs = np.random.RandomState(seed)
            for i in range(k):
                C[i, rs.choice(sparse_support, size=min(3, len(sparse_support)), replace=False)] = rs.uniform(0.1, 1, 1)[0]
            C /= C.sum(axis=1, keepdims=True)
            model.fit_transform(X, features=True, kernel="rbf", gamma=gamma, dictionary=C, update_dictionary=False)
    return model


@pytest.mark.parametrize("k", [1, 3, 32, 33, 64])
@pytest.mark.parametrize("p", [1, 5, 100])
def test_rbf_features_against_the_oracle(cdr, orc, k, p):
    rng = np.random.RandomState(10 * k + p)
    n = 160
    gamma = 0.5 / p
    X = _clusters(rng, n, p)
    K = _rbf(X, X, gamma)
    model = _rbf_model(cdr, X, k, gamma)
    D = model.alpha[:, None] * model.dictionary
    assert model._transform_state["support_rows"].shape[0] == np.count_nonzero(np.any(D != 0, axis=0))
    model.max_iterations = 5
    for m in (1, 17, 1000):
        Y = _clusters(rng, m, p)
        rs = copy.deepcopy(model.random_state)
        W, cost = model.transform(Y)
        wW, wcost = _oracle_transform(orc, model, K, _rbf(X, Y, gamma), np.ones(m), rs, 5)
        assert W.shape == (m, k)
        assert np.abs(W - wW).max() <= 1e-9, (m, np.abs(W - wW).max())
        assert abs(cost - wcost) <= 1e-11 * abs(wcost), (m, cost, wcost)


@pytest.mark.parametrize("support", ["whole", "few"])
def test_rbf_support_whole_and_small(cdr, orc, support):
    rng = np.random.RandomState(7)
    n, p, k, gamma = 500, 6, 5, 0.2
    X = _clusters(rng, n, p)
    K = _rbf(X, X, gamma)
    if support == "whole":
        model = _rbf_model(cdr, X, k, gamma)
        D = model.alpha[:, None] * model.dictionary
        if not np.all(np.any(D != 0, axis=0)):          # make the support the whole training set
            model.dictionary = 0.5 * model.dictionary + 0.5 / n
            model._transform_state = None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model.fit_transform(X, features=True, kernel="rbf", gamma=gamma,
                                    dictionary=model.dictionary, update_dictionary=False)
        assert len(model._transform_state["support"]) == n
    else:
        model = _rbf_model(cdr, X, k, gamma, sparse_support=np.arange(0, n, 50))
        assert len(model._transform_state["support"]) <= 10
    model.max_iterations = 5
    Y = np.vstack([_clusters(rng, 300, p), X[:20]])      # rows of the training set among the new ones
    rs = copy.deepcopy(model.random_state)
    W, cost = model.transform(Y)
    wW, wcost = _oracle_transform(orc, model, K, _rbf(X, Y, gamma), np.ones(len(Y)), rs, 5)
    assert np.abs(W - wW).max() <= 1e-9
    assert abs(cost - wcost) <= 1e-11 * abs(wcost)


@pytest.mark.parametrize("m,s,p,k", [(1, 1, 1, 1), (17, 65, 5, 3), (1000, 129, 100, 33),
                                     (3001, 2049, 37, 64), (2500, 3000, 130, 32)])
def test_cross_product_against_numpy(cdr, m, s, p, k):
    from convex_dim_red import _backend
    rng = np.random.RandomState(m + s + p + k)
    XS = rng.standard_normal((s, p))
    Y = rng.standard_normal((m, p))
    Y[: min(m, s) // 2] = XS[: min(m, s) // 2]          # distances of about 0
    V = rng.uniform(size=(s, k))
    gamma = 1.0 / p
    want = _rbf(Y, XS, gamma).dot(V)
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(Y)
        ctx.set_rbf_reference(XS, V, gamma)
        got = ctx.rbf_cross(fetch=True)
        again = ctx.rbf_cross(fetch=True)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got, again)


def test_state_copies_and_errors(cdr):
    rng = np.random.RandomState(11)
    n, m, p, k, gamma = 120, 40, 3, 3, 0.4
    X = _clusters(rng, n, p)
    Y = _clusters(rng, m, p)
    for kind in ("kernel", "linear", "rbf"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = cdr.KernelAA(k, random_state=5, max_iterations=20)
            if kind == "kernel":
                model.fit_transform(_rbf(X, X, gamma))
                args, kw = (_rbf(Y, X, gamma),), dict(diagonal=np.ones(m))
            elif kind == "linear":
                model.fit_transform(X, features=True)
                args, kw = (Y,), {}
            else:
                model.fit_transform(X, features=True, kernel="rbf", gamma=gamma)
                args, kw = (Y,), {}
        before = copy.deepcopy(model)
        twin = copy.deepcopy(model)
        W, cost = model.transform(*args, **kw)
        W2, cost2 = twin.transform(*args, **kw)
        assert np.array_equal(W, W2) and cost == cost2, kind
        assert np.array_equal(model.weights, W)
        for name, value in vars(before).items():
            if name in ("weights", "random_state"):
                continue
            now = getattr(model, name)
            if name == "_transform_state":
                assert sorted(now) == sorted(value)
                for key in value:
                    assert np.array_equal(np.asarray(now[key]), np.asarray(value[key])), (kind, key)
            elif isinstance(value, np.ndarray) or isinstance(value, list):
                assert np.array_equal(np.asarray(now), np.asarray(value)), (kind, name)
            else:
                assert now == value, (kind, name)
        width = n if kind == "kernel" else p
        with pytest.raises(ValueError):
            model.transform(np.ones((m, width + 1)), **kw)
        if kind == "kernel":
            with pytest.raises(ValueError, match="diagonal"):
                model.transform(*args)
