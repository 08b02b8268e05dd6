"""Column statistics and standardisation of resident data on the MI355X (aa_data_column_moments,
aa_set_data_rows_affine, DeviceData.column_stats / standardized / unscale,
weight_and_flatten_on_device(standardize=True)).

The bound of the moments is DERIVED from the inputs.  With u = 2^-53 and n rows, a float64 sum of n terms in
any order is within (n - 1) u sum|x| of the exact one, so a computed mean is within
``b_mean = n u mean|x_j|`` of the exact mean (the division adds one more u).  For the variance, an inexact mean
m + e changes sum (x - m)^2 by -2 e sum (x - m) + n e^2 = n e^2, because sum (x - m) = 0: the first-order effect
cancels and e^2 <= b_mean^2 remains; the subtraction, the square, the n-term sum and the division add
(n + 4) u var_j.  So ``b_var = (n + 4) u var_j + b_mean^2``.  NumPy and the device are each within that bound
of the exact value; the tests allow a difference of 2 x the bound.  (A one-sweep E[x^2] - E[x]^2 loses
n u mean(x^2), which on the columns whose offset is 10^4 times their spread is 10^5 .. 10^8 times b_var.)

The scaled copy is compared exactly: a float64 subtraction, a float64 division and one rounding to the stored
type are what NumPy does too."""
import warnings

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# 2500 is above the largest number of row slabs the moments launcher chooses (2048)
ROWS = [1, 2, 127, 128, 129, 1000, 2500]
COLS = [1, 127, 128, 129, 167, 257, 1000]


def _columns(rng, n, p):
    """standard_normal * uniform(0.1, 5) + offset; even columns: offset 1e4 * uniform(-1, 1), odd columns: 0."""
    offset = 1e4 * rng.uniform(-1.0, 1.0, size=p)
    offset[1::2] = 0.0
    return rng.standard_normal((n, p)) * rng.uniform(0.1, 5.0, size=p) + offset


def _moment_bounds(Xd):
    n = Xd.shape[0]
    b_mean = n * U * np.abs(Xd).mean(axis=0)
    return b_mean, (n + 4) * U * Xd.var(axis=0) + b_mean ** 2


def _device_data(ctx, X):
    ctx.set_data(X)
    return cdr.DeviceData(ctx, X.shape, None, X.shape[1:])


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_moments_against_float64_numpy(dtype, n):
    rng = np.random.RandomState(200 + n)
    worst_mean = worst_var = 0.0
    with _backend.Context(dtype=dtype) as ctx:
        for p in COLS:
            X = _columns(rng, n, p)
            ctx.set_data(X)
            Xd = ctx.get_data()                     # the stored values: what a float32 context is judged on
            if dtype == "float64":
                assert np.array_equal(Xd, X)
            mean, var = ctx.data_column_moments()
            msg = "dtype=%s n=%d p=%d" % (dtype, n, p)
            assert mean.shape == (p,) and var.shape == (p,) and mean.dtype == np.float64 and var.dtype == np.float64
            if n == 1:
                assert np.array_equal(mean, Xd[0]), msg
                assert np.array_equal(var, np.zeros(p)), msg
            else:
                b_mean, b_var = _moment_bounds(Xd)
                e_mean, e_var = np.abs(mean - Xd.mean(axis=0)), np.abs(var - Xd.var(axis=0))
                worst_mean = max(worst_mean, (e_mean / b_mean).max())
                worst_var = max(worst_var, (e_var / b_var).max())
                assert np.all(e_mean <= 2 * b_mean), msg
                assert np.all(e_var <= 2 * b_var), msg
            # identical bits on every call; NULL outputs honoured
            m2, v2 = ctx.data_column_moments()
            assert np.array_equal(m2, mean) and np.array_equal(v2, var), msg
            m3, none = ctx.data_column_moments(var=False)
            assert none is None and np.array_equal(m3, mean), msg
            none, v3 = ctx.data_column_moments(mean=False)
            assert none is None and np.array_equal(v3, var), msg
            assert ctx.data_column_moments(mean=False, var=False) == (None, None)
            # the Python surface: std = sqrt(var) on the host, cached
            dd = cdr.DeviceData(ctx, X.shape, None, X.shape[1:])
            stats = dd.column_stats()
            assert isinstance(stats, cdr.ColumnStats) and stats.n_samples == n
            assert np.array_equal(stats.mean, mean) and np.array_equal(stats.std, np.sqrt(var)), msg
            assert dd.column_stats() is stats and dd.scaling is None
    print("largest error / bound over the cases of n=%d, %s: mean %.3f, var %.3f (allowed 2)"
          % (n, dtype, worst_mean, worst_var))


def _stored(A, dtype):
    return A.astype(np.float32).astype(np.float64) if dtype == "float32" else A


@pytest.mark.parametrize("n", ROWS[1:])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_scaled_copy_is_exact(dtype, n):
    rng = np.random.RandomState(300 + n)
    with _backend.Context(dtype=dtype) as ctx, _backend.Context(dtype=dtype) as block:
        for p in COLS:
            D = _device_data(ctx, _columns(rng, n, p))
            Xd = D.to_host()
            own = D.column_stats()
            foreign = cdr.ColumnStats(rng.standard_normal(p) * 3.0, rng.uniform(0.5, 2.0, size=p), 7)
            for center in (False, True):
                for stats in (None, foreign):
                    msg = "dtype=%s n=%d p=%d center=%s %s stats" % (dtype, n, p, center,
                                                                      "own" if stats is None else "foreign")
                    used = own if stats is None else stats
                    shift = used.mean if center else np.zeros(p)
                    with D.standardized(center=center, stats=stats) as Y:
                        assert Y.shape == D.shape and Y.dtype == D.dtype
                        assert Y.scaling.center is center and Y.scaling.stats is used
                        assert np.array_equal(Y.to_host(), _stored((Xd - shift) / used.std, dtype)), msg
            # the row-block form of the entry point, through the binding
            for row0, nb in ((0, n), (n - 1, 1), (n // 3, n - n // 3), (1, max(1, n // 2))):
                if row0 + nb > n:
                    continue
                for shift, scale in ((foreign.mean, foreign.std), (None, foreign.std), (foreign.mean, None),
                                     (None, None))[:4 if row0 == 0 else 1]:
                    block.set_data_rows_affine(ctx, row0, nb, shift, scale)
                    want = (Xd[row0:row0 + nb] - (0.0 if shift is None else shift)) / (1.0 if scale is None else scale)
                    assert (block.n, block.p) == (nb, p)
                    assert np.array_equal(block.get_data(), _stored(want, dtype)), (dtype, n, p, row0, nb)


@pytest.mark.parametrize("p", [129, 167])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_padding_stays_zero_seen_through_the_solvers(dtype, p):
    """A non-zero padding column or row of the scaled copy would enter the Gram products of the pass kernels:
    fits on the resident block and on a fresh upload of its values must agree bit for bit."""
    rng = np.random.RandomState(400 + p)
    n, k = 129, 3
    basis = rng.uniform(size=(k, p)) * rng.uniform(0.5, 4.0, size=p) + rng.uniform(-3.0, 3.0, size=p)
    Z = rng.uniform(size=(n, k)) ** 3
    X = (Z / Z.sum(axis=1, keepdims=True)).dot(basis) + 0.05 * rng.standard_normal((n, p))
    with _backend.Context(dtype=dtype) as ctx:
        Y = _device_data(ctx, X).standardized(center=True)
    host = Y.to_host()
    assert host.shape == (n, p) and np.all(np.isfinite(host))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for init in ("random", "furthest_sum"):
            kw = dict(init=init, tolerance=1e-6, max_iterations=5, dtype=dtype,
                      dictionary_solver_kwargs=dict(max_iterations=1))
            a = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
            Wa = a.fit_transform(Y)
            b = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
            Wb = b.fit_transform(host)
            assert np.array_equal(Wa, Wb) and np.array_equal(a.dictionary, b.dictionary)
            assert a.cost == b.cost and a.n_iter == b.n_iter and list(a.cost_deltas) == list(b.cost_deltas)
            gkw = dict(lambda_W=0.5, init=init, tolerance=1e-6, max_iterations=5, dtype=dtype)
            g = cdr.GPNHConvexCoding(k, random_state=0, **gkw)
            Zg = g.fit_transform(Y)
            g2 = cdr.GPNHConvexCoding(k, random_state=0, **gkw)
            Zh = g2.fit_transform(host)
            assert np.array_equal(Zg, Zh) and np.array_equal(g.dictionary, g2.dictionary)
            assert g.cost == g2.cost and g.n_iter == g2.n_iter and list(g.cost_deltas) == list(g2.cost_deltas)
    Y.close()


def _field():
    rng = np.random.RandomState(11)
    n_time, n_lat, n_lon = 150, 7, 9
    lat = np.linspace(-75.0, 75.0, n_lat)
    field = rng.standard_normal((n_time, n_lat, n_lon)) * rng.uniform(0.2, 6.0, size=(n_lat, n_lon)) + 280.0
    field[:, rng.uniform(size=(n_lat, n_lon)) < 0.2] = np.nan          # always missing
    field[rng.randint(n_time), 2, 3] = np.nan                          # missing once: dropped as well
    weights = (np.cos(np.deg2rad(lat)).clip(0.0, 1.0) ** 0.5)[:, np.newaxis]
    return field, weights


def test_driver_standardize_in_one_call():
    """bin/run_jra55_pca_aa.py:157-166: weights * da, flatten, NaN mask, / np.std(axis=0)."""
    raw, weights = _field()
    flat = (raw * weights).reshape(raw.shape[0], -1)
    valid = ~np.isnan(flat).any(axis=0)
    valid_data = flat[:, valid]
    with cdr.weight_and_flatten_on_device(raw, weights, dtype="float64") as B, \
            cdr.weight_and_flatten_on_device(raw, weights, dtype="float64", standardize=True) as S:
        assert B.scaling is None and np.array_equal(B.to_host(), valid_data)
        assert B.unscale(valid_data) is valid_data
        assert np.array_equal(S.valid, valid) and np.array_equal(S.valid, B.valid)
        assert S.shape == B.shape and S.original_shape == B.original_shape and S.dtype == B.dtype
        stats, center = S.scaling
        assert center is False and stats.n_samples == raw.shape[0]
        assert np.array_equal(stats.std, B.column_stats().std) and np.array_equal(stats.mean, B.column_stats().mean)
        # exactly the driver's sequence, divided by the std the device reports
        assert np.array_equal(S.to_host(), valid_data / stats.std)
        # and that std is np.std's within the bound of the moments: s1 - s2 = (v1 - v2) / (s1 + s2), each
        # square root adds one rounding
        want = np.std(valid_data, axis=0)
        _, b_var = _moment_bounds(valid_data)
        tol = 2 * b_var / (stats.std + want) + 2 * U * want
        print("largest std error / tolerance: %.3f" % (np.abs(stats.std - want) / tol).max())
        assert np.all(np.abs(stats.std - want) <= tol)
        # x / s * s: two roundings
        back = S.unscale(S.to_host())
        assert np.all(np.abs(back - valid_data) <= 2 * np.spacing(np.abs(valid_data)))
        with S.rows(10, 60) as part:
            assert part.scaling is S.scaling
            assert np.array_equal(part.to_host(), S.to_host()[10:60])
        # centred: (x - m) / s * s + m; three roundings on x - m and one on the sum (derivation in DESIGN 5.3)
        with B.standardized(center=True) as C:
            assert C.scaling.center is True
            dev = np.abs(valid_data - stats.mean)
            assert np.all(np.abs(C.unscale(C.to_host()) - valid_data) <= 4 * U * (dev + np.abs(valid_data)))
            arche = C.to_host()[:3]
            assert np.array_equal(C.unscale(arche[np.newaxis]), (arche * stats.std + stats.mean)[np.newaxis])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_constant_columns_are_refused_and_the_source_survives(dtype):
    rng = np.random.RandomState(5)
    for n in (1, 129, 2500):
        X = _columns(rng, n, 9)
        X[:, 3] = 0.0
        X[:, 5] = -2.0
        with _backend.Context(dtype=dtype) as ctx:
            D = _device_data(ctx, X)
            Xd = D.to_host()
            stats = D.column_stats()
            assert stats.mean[3] == 0.0 and stats.std[3] == 0.0
            assert stats.mean[5] == -2.0 and stats.std[5] == 0.0
            if n > 1:
                assert np.all(stats.std[[0, 1, 2, 4, 6, 7, 8]] > 0)
                for center in (False, True):
                    with pytest.raises(ValueError, match=r"2 column\(s\).*column 3"):
                        D.standardized(center=center)
            else:
                with pytest.raises(ValueError, match=r"9 column\(s\).*column 0"):
                    D.standardized()
            good = cdr.ColumnStats(np.zeros(9), np.full(9, 2.0), n)
            with D.standardized(center=True, stats=good) as Y, D.rows(0, 1) as first:
                assert np.array_equal(Y.to_host(), _stored(Xd / 2.0, dtype))
                assert np.array_equal(first.to_host(), Xd[:1])
            D.close()
            with pytest.raises(RuntimeError, match="closed"):
                D.standardized(stats=good)


def test_entry_point_refusals():
    rng = np.random.RandomState(0)
    A = rng.standard_normal((20, 6))
    ones = np.ones(6)
    with _backend.Context(dtype="float64") as owner, _backend.Context(dtype="float64") as target:
        with pytest.raises(RuntimeError, match="error -3:"):                 # AA_ERR_STATE: no data yet
            owner.data_column_moments()
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_affine(owner, 0, 1)
        owner.set_data(A)
        B = rng.standard_normal((7, 4))
        target.set_data(B)
        for row0, nb in ((-1, 5), (0, 0), (0, 21), (20, 1), (5, 16), (0, -3)):
            with pytest.raises(RuntimeError, match="error -1:"):             # AA_ERR_ARG: bad row block
                target.set_data_rows_affine(owner, row0, nb, None, ones)
        with pytest.raises(RuntimeError, match="error -1:"):                 # ctx == owner
            owner.set_data_rows_affine(owner, 0, 5, None, ones)
        with _backend.Context(dtype="float32") as other:
            with pytest.raises(RuntimeError, match="error -1:"):             # dtype mismatch
                other.set_data_rows_affine(owner, 0, 5, None, ones)
        # a divisor that is zero or not finite, a shift that is not finite: refused, the target keeps its data
        for shift, scale in ((None, [1, 1, 0.0, 1, 1, 1]), (None, [1, 1, 1, 1, 1, np.inf]),
                             (None, [np.nan, 1, 1, 1, 1, 1]), (None, [1, -0.0, 1, 1, 1, 1]),
                             ([0, 0, 0, np.inf, 0, 0], ones), ([0, np.nan, 0, 0, 0, 0], None)):
            with pytest.raises(RuntimeError, match="error -1:"):
                target.set_data_rows_affine(owner, 0, 10, shift, scale)
            assert (target.n, target.p) == (7, 4)
            assert np.array_equal(target.get_data(), B)
            mean, var = target.data_column_moments()
            assert np.all(np.abs(mean - B.mean(axis=0)) <= 2 * _moment_bounds(B)[0])
        with pytest.raises(ValueError):                               # the binding checks the lengths
            target.set_data_rows_affine(owner, 0, 10, None, np.ones(5))
        target.set_data_rows_affine(owner, 2, 10, None, -ones)        # a negative divisor is a divisor
        assert np.array_equal(target.get_data(), -A[2:12])
    K = rng.standard_normal((12, 12))
    with _backend.Context(dtype="float64") as ctx, _backend.Context(dtype="float64") as target:
        ctx.set_data(K.dot(K.T), form=_backend.FORM_KERNEL)
        with pytest.raises(RuntimeError, match="error -3:"):                 # kernel form
            ctx.data_column_moments()
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_affine(ctx, 0, 5, None, None)
    with _backend.Context(dtype="float64") as ctx, _backend.Context(dtype="float64") as target:
        ctx.set_rbf_features(rng.standard_normal((12, 3)), 0.5)
        with pytest.raises(RuntimeError, match="error -3:"):                 # implicit kernel
            ctx.data_column_moments()
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_affine(ctx, 0, 5, None, None)
