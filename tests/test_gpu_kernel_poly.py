"""KernelAA on the implicit polynomial kernel (gamma x.y + coef0)^degree on the MI355X: the K V product on the
f64 matrix cores element-wise against NumPy, the trace, the distance column and FurthestSum, fixed
iterations against the oracle's kernel form on the explicit matrix, the estimator run to its stopping rule,
and transform against the explicit path and NumPy.

Inputs everywhere: clustered data scaled so that max |gamma x.y| <= 1, coef0 = 1, degree 2 or 3.  The
entries of K then lie in [0, 8] and no power cancels.  The explicit K is NumPy float64 with the device's
multiplication order (b = gamma s + coef0, v = b, v = v * b)."""
import copy
import warnings

import numpy as np
import pytest

from conftest import oracle_twins

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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


def _poly(Y, X, gamma, coef0, degree):
    b = gamma * Y.dot(X.T) + coef0
    v = b.copy()
    for _ in range(degree - 1):
        v = v * b
    return v


def _clusters(rng, n, p, k, gamma):
    """The clustered data of test_kernel_aa_on_the_implicit_rbf_kernel, scaled so that gamma |x|^2 <= 1 for
    every row (hence |gamma x.y| <= 1 for every pair)."""
    centers = rng.standard_normal((k, p)) * 2.0
    X = centers[rng.randint(k, size=n)] + 0.4 * rng.standard_normal((n, p))
    X = X / np.sqrt(gamma * (X * X).sum(axis=1).max())
    return X * (1.0 - 1e-12)                             # the largest gamma |x|^2 is 1 up to rounding: keep it below


def _assert_simplex(M, atol):
    assert np.all(M >= 0)
    assert np.allclose(M.sum(axis=1), 1, rtol=0, atol=atol)


def _product_bound(p, degree, n, magnitude):
    """|got - want| <= 4 (p + 2 d + n) 2^-53 (|K| |V|), element-wise: a dot product of length p, d
    multiplications (and as many in the reference), a sum over n terms; derived, not tuned."""
    return 4.0 * (p + 2 * degree + n) * U * magnitude


# n = 130: one partial 64-row tile and padding columns; 4200 with the launcher's split arithmetic
# (launch_kernel_product's): 66 row tiles, 14 splits of 5 column tiles, the last one a single tile; p = 7 (no
# multiple of 4), 33 (crosses a 32-feature chunk), 64 (exact chunks); k = 3 (KP = 32), 40 (KP = 64)
@pytest.mark.parametrize("n,p,k,degree", [(130, 7, 3, 2), (130, 33, 40, 3), (130, 64, 3, 3), (900, 64, 40, 2),
                                          (900, 33, 3, 3), (4200, 7, 3, 3), (4200, 33, 40, 2)])
def test_one_product_against_numpy(cdr, orc, n, p, k, degree):
    """K V through set_state / prepare / grams.  Twice: with random factors (C K C' and C K Z, judged with
    the magnitude |C| |K| |V|), and with one-hot rows in C, which makes C K Z the selected rows of the tall
    product K Z itself and C K C' single entries of K (a sum of exact zeros and one term), at the tile and
    split edges.  Then the trace: the NumPy sum to n 2^-52 relative, the same bits from two calls."""
    from convex_dim_red import _backend
    rng = np.random.RandomState(1000 * degree + n + p + k)
    gamma = 1.0 / p
    X = _clusters(rng, n, p, 5, gamma)
    K = _poly(X, X, gamma, 1.0, degree)
    assert K.min() >= 0.0 and K.max() <= 8.0
    C0 = orc.right_stochastic_matrix((k, n), rng)
    Z0 = orc.right_stochastic_matrix((n, k), rng)
    edges = [0, 1, 15, 16, 62, 63, 64, 65, 127, 128, n - 66, n - 65, n - 64, n - 2, n - 1, 319, 320, 321]
    rows = [r for r in edges if 0 <= r < n]
    rows = np.array(sorted(set(rows)) + list(rng.choice(n, size=40, replace=False)))
    traces = []
    with _backend.Context(dtype="float64") as ctx:
        for rep in range(2):
            ctx.set_poly_features(X, gamma, 1.0, degree)
            ctx.set_state(C0, Z0, np.ones(k))
            ctx.prepare()
            ZtZ, CKCt, CKZ, tr = ctx.grams()
            traces.append(tr)
        for got, V in ((CKCt, C0.T), (CKZ, Z0)):
            want = C0.dot(K).dot(V)
            bound = _product_bound(p, degree, n, C0.dot(np.abs(K)).dot(V))
            print("n %d p %d k %d d %d: random factors, max |got - want| / bound %.3f"
                  % (n, p, k, degree, (np.abs(got - want) / bound).max()))
            assert np.all(np.abs(got - want) <= bound)
        for i0 in range(0, len(rows), k):
            sel = rows[i0:i0 + k]
            sel = np.concatenate([sel, rows[:k - len(sel)]])
            C1 = np.zeros((k, n))
            C1[np.arange(k), sel] = 1.0
            ctx.set_state(C1, Z0, np.ones(k))
            ctx.prepare()
            _, CKCt, CKZ, _ = ctx.grams()
            want = K[sel].dot(Z0)
            assert np.all(np.abs(CKZ - want) <= _product_bound(p, degree, n, np.abs(K[sel]).dot(Z0))), sel
            want = K[np.ix_(sel, sel)]
            assert np.all(np.abs(CKCt - want) <= _product_bound(p, degree, n, np.abs(want))), sel
    want_tr = _poly_diag(X, gamma, 1.0, degree).sum()
    assert abs(traces[0] - want_tr) <= n * 2.0 ** -52 * want_tr
    assert traces[0] == traces[1]


def _poly_diag(X, gamma, coef0, degree):
    b = gamma * (X * X).sum(axis=1) + coef0
    v = b.copy()
    for _ in range(degree - 1):
        v = v * b
    return v


@pytest.mark.parametrize("degree", [2, 3])
def test_distance_column_and_furthest_sum(cdr, degree):
    """d_i = sqrt(max(K_ii - 2 K_ij + K_jj, 0)) to 1e-7 absolute, the RBF test's bound: near zero the square
    root amplifies the rounding of K (an error of 1e-15 in the difference is 3e-8 in d), away from zero the
    agreement is at rounding level; d_j is exactly 0.  The device FurthestSum then equals the reference
    selection rule on the dissimilarities the context serves."""
    from convex_dim_red import _backend
    from convex_dim_red import archetypal_analysis as aa
    rng = np.random.RandomState(21)
    n, p, k = 900, 12, 5
    gamma = 1.0 / p
    X = _clusters(rng, n, p, k, gamma)
    K = _poly(X, X, gamma, 1.0, degree)
    kd = np.diag(K)
    want = np.sqrt(np.maximum(kd[:, None] - 2 * K + kd[None, :], 0.0))
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_poly_features(X, gamma, 1.0, degree)
        D = np.stack([ctx.distance_column(j) for j in range(n)], axis=1)
        print("degree %d: distance columns, max |got - want| %.2e" % (degree, np.abs(D - want).max()))
        assert np.abs(D - want).max() < 1e-7
        assert np.all(np.diag(D) == 0.0)
        for start, extra_steps in ((0, 10), (123, 3)):
            picks = aa._furthest_sum_on_device(ctx, n, k, start, extra_steps, np.array([], dtype="i8"))
            assert np.array_equal(picks, cdr.furthest_sum(D, k, start, extra_steps=extra_steps)), (start, picks)


# ---------------------------------------------------------------- fixed iterations, and the fits transform shares
FIT = dict(n=900, p=12, k=5, degree=3, seed=4)


def _fit_problem(orc):
    rng = np.random.RandomState(FIT["seed"])
    n, p, k = FIT["n"], FIT["p"], FIT["k"]
    gamma = 1.0 / p
    XY = _clusters(rng, n + 200, p, k, gamma)            # training rows and new rows, scaled together
    X, Y = XY[:n], XY[n:]
    K = _poly(X, X, gamma, 1.0, FIT["degree"])
    C0 = orc.right_stochastic_matrix((k, n), rng)
    Z0 = orc.right_stochastic_matrix((n, k), rng)
    return X, Y, K, C0, Z0, gamma


def _fixed_run(cdr, orc, iters):
    """The oracle's kernel form on the explicit K from a custom start, its twins (K moved by one ulp), and the
    product's explicit-kernel and implicit fits from the same start."""
    X, Y, K, C0, Z0, gamma = _fit_problem(orc)
    k = FIT["k"]
    kw = dict(tolerance=0, max_iterations=iters, dictionary_solver_kwargs=dict(max_iterations=1),
              require_monotonic_cost_decrease=False)

    def run(Kin):
        return orc.iterate_kernel_aa(Kin, Z0.copy(), C0.copy(), np.ones(k), **kw)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = run(K)
        twins = oracle_twins(orc, run, K, "float64")
        fits = []
        for data, extra in ((K, {}), (X, dict(features=True, kernel="poly", gamma=gamma, coef0=1, degree=FIT["degree"]))):
            m = cdr.KernelAA(k, init="custom", random_state=7, **kw)
            m.fit_transform(data, dictionary=C0, weights=Z0, alpha=np.ones(k), **extra)
            fits.append(m)
    return dict(X=X, Y=Y, K=K, gamma=gamma, base=base, twins=twins, explicit=fits[0], implicit=fits[1])


@pytest.fixture(scope="module")
def run25(cdr, orc):
    return _fixed_run(cdr, orc, 25)


def _judge_against_the_oracle(run, iters):
    base, twins = run["base"], run["twins"]
    for t in twins:                                      # the twins end in the optimum of the base run
        assert np.array_equal(t[1].argmax(axis=1), base[1].argmax(axis=1))
    t_cost = max(abs(t[3] - base[3]) for t in twins) / abs(base[3])
    t_C = max(np.abs(t[1] - base[1]).max() for t in twins)
    for name in ("explicit", "implicit"):
        m = run[name]
        print("polynomial kernel, %d iterations, %s: cost rel diff from the oracle %.2e (bound %.2e), dictionary "
              "%.2e (bound %.2e)" % (iters, name, abs(m.cost - base[3]) / abs(base[3]), max(1e-10, 20 * t_cost),
                                     np.abs(m.dictionary - base[1]).max(), max(1e-9, 20 * t_C)))
    for name in ("explicit", "implicit"):
        m = run[name]
        assert abs(m.cost - base[3]) <= max(1e-10, 20 * t_cost) * abs(base[3])
        assert np.abs(m.dictionary - base[1]).max() <= max(1e-9, 20 * t_C)
        assert np.array_equal(m.dictionary.argmax(axis=1), base[1].argmax(axis=1))
        _assert_simplex(m.weights, 1e-12)
        _assert_simplex(m.dictionary, 1e-12)


def test_four_iterations_against_the_oracle(cdr, orc):
    """n = 900, p = 12, k = 5, degree 3, custom start: the implicit fit and the product's explicit-kernel fit
    against orc.iterate_kernel_aa on the explicit K, both judged by the oracle's own response to a one-ulp
    change of K: cost within max(1e-10, 20 x twin), dictionary within max(1e-9, 20 x twin), equal arg-max
    per dictionary row."""
    _judge_against_the_oracle(_fixed_run(cdr, orc, 4), 4)


def test_twenty_five_iterations_against_the_oracle(run25):
    """The same after 25 iterations."""
    _judge_against_the_oracle(run25, 25)


@pytest.mark.parametrize("init", ["furthest_sum", "random"])
def test_estimator_runs_to_its_stopping_rule(cdr, orc, init):
    X, _, _, _, _, gamma = _fit_problem(orc)
    n, k = FIT["n"], FIT["k"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = cdr.KernelAA(k, init=init, random_state=3, tolerance=1e-5, max_iterations=40,
                             dictionary_solver_kwargs=dict(max_iterations=1))
        W = model.fit_transform(X, features=True, kernel="poly", gamma=gamma, degree=2)
    assert model.cost_deltas[0] < 0 and model.cost > 0
    assert W.shape == (n, k) and model.dictionary.shape == (k, n) and model.alpha.shape == (k,)
    assert 1 <= model.n_iter <= 40
    _assert_simplex(W, 1e-12)
    _assert_simplex(model.dictionary, 1e-12)
    state = model._transform_state
    assert state["form"] == "poly" and state["degree"] == 2 and state["coef0"] == 1.0 and state["gamma"] == gamma


# ---------------------------------------------------------------- transform
def _oracle_transform(orc, Z, C, alpha, K, cross, diag, rs, max_iterations):
    """KernelAA.transform in the oracle (tests/test_gpu_kernel_transform.py): cross = kappa(X, Y), n x m."""
    D = alpha[:, None] * C
    A = D.dot(K).dot(D.T)
    B = D.dot(cross)
    m = cross.shape[1]
    Z0 = orc.right_stochastic_matrix((m, C.shape[0]), rs)
    W = orc.qp_batch(A, B, Z0, "kn", max_iterations=max_iterations)
    cost = 0.5 * (diag.sum() - 2 * np.sum(W * B.T) + np.einsum("ti,ij,tj->", W, A, W)) / m
    return W, cost


@pytest.mark.parametrize("m", [70, 200])
def test_transform_against_the_explicit_path(cdr, orc, run25, m):
    """Weights and cost of m new rows: the implicit model (device cross product, m x n kernel never formed)
    against the explicit path -- transform(kappa(Y, X), diagonal=kappa(y, y)) on the model fitted on the
    explicit K from the same start, same draws.  The two models' dictionaries differ within the twin
    yardstick of the 25-iteration fit they share, so the yardstick here is the oracle's transform on its
    twins' factors against the one on its base run's: weights within max(1e-9, 20 x twin), cost within
    max(1e-10, 20 x twin) relative."""
    Y = run25["Y"][:m]
    X, K, gamma = run25["X"], run25["K"], run25["gamma"]
    cross = _poly(Y, X, gamma, 1.0, FIT["degree"])      # m x n
    diag = _poly_diag(Y, gamma, 1.0, FIT["degree"])
    implicit, explicit = copy.deepcopy(run25["implicit"]), copy.deepcopy(run25["explicit"])
    rs = copy.deepcopy(implicit.random_state)
    Wi, ci = implicit.transform(Y)
    We, ce = explicit.transform(cross, diagonal=diag)
    outs = [_oracle_transform(orc, r[0], r[1], r[2], K, cross.T, diag, copy.deepcopy(rs), implicit.max_iterations)
            for r in [run25["base"]] + list(run25["twins"])]
    t_W = max(np.abs(o[0] - outs[0][0]).max() for o in outs[1:])
    t_cost = max(abs(o[1] - outs[0][1]) for o in outs[1:]) / abs(outs[0][1])
    print("transform, m = %d: weights implicit - explicit %.2e (bound %.2e), cost rel %.2e (bound %.2e); implicit "
          "against the oracle: weights %.2e, cost rel %.2e"
          % (m, np.abs(Wi - We).max(), max(1e-9, 20 * t_W), abs(ci - ce) / abs(ce), max(1e-10, 20 * t_cost),
             np.abs(Wi - outs[0][0]).max(), abs(ci - outs[0][1]) / abs(outs[0][1])))
    assert Wi.shape == (m, FIT["k"])
    _assert_simplex(Wi, 1e-12)
    assert np.abs(Wi - We).max() <= max(1e-9, 20 * t_W)
    assert abs(ci - ce) <= max(1e-10, 20 * t_cost) * abs(ce)
    assert np.abs(Wi - outs[0][0]).max() <= max(1e-9, 20 * t_W)
    assert abs(ci - outs[0][1]) <= max(1e-10, 20 * t_cost) * abs(outs[0][1])


@pytest.mark.parametrize("m,s,p,k,degree", [(70, 40, 12, 5, 3), (200, 150, 12, 5, 2), (70, 150, 33, 40, 3),
                                            (200, 40, 7, 3, 2)])
def test_cross_product_against_numpy(cdr, m, s, p, k, degree):
    """kappa(Y, X_S) V on the device against NumPy within the bound of the fit's product with the support
    size s in the place of n: supports below and above one 64-column tile; the same bits from two calls."""
    from convex_dim_red import _backend
    rng = np.random.RandomState(m + s + p + k)
    gamma = 1.0 / p
    XY = _clusters(rng, s + m, p, 5, gamma)
    XS, Y = XY[:s], XY[s:]
    V = rng.uniform(size=(s, k))
    Kc = _poly(Y, XS, gamma, 1.0, degree)
    want = Kc.dot(V)
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(Y)
        ctx.set_poly_reference(XS, V, gamma, 1.0, degree)
        got = ctx.poly_cross(fetch=True)
        again = ctx.poly_cross(fetch=True)
    bound = _product_bound(p, degree, s, np.abs(Kc).dot(V))
    print("cross product m %d s %d p %d k %d d %d: max |got - want| / bound %.3f"
          % (m, s, p, k, degree, (np.abs(got - want) / bound).max()))
    assert got.shape == (m, k)
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got, again)


def test_entry_points_refuse_bad_parameters(cdr):
    """AA_ERR_ARG for degree < 1, gamma <= 0, coef0 < 0 and non-finite values, from both set-up calls."""
    from convex_dim_red import _backend
    X = np.linspace(-1.0, 1.0, 60).reshape(12, 5)
    bad = [(0.0, 1.0, 2), (-1.0, 1.0, 2), (0.2, -0.5, 2), (0.2, 1.0, 0), (float("nan"), 1.0, 2),
           (0.2, float("nan"), 2), (float("inf"), 1.0, 2), (0.2, float("inf"), 2)]
    with _backend.Context(dtype="float64") as ctx:
        for gamma, coef0, degree in bad:
            with pytest.raises(RuntimeError, match="polynomial kernel needs"):
                ctx.set_poly_features(X, gamma, coef0, degree)
        ctx.set_data(X)
        for gamma, coef0, degree in bad:
            with pytest.raises(RuntimeError, match="polynomial kernel needs"):
                ctx.set_poly_reference(X[:4], np.ones((4, 2)), gamma, coef0, degree)
        with pytest.raises(RuntimeError):
            ctx.poly_cross()                                     # no reference set
