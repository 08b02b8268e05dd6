"""Seasonal anomalies and per-group standardisation of resident data on the MI355X (aa_data_weighted_column_sums,
aa_data_grouped_sqdev, aa_set_data_rows_model, DeviceData.seasonal_anomalies / grouped_column_stats /
standardized_by_group).

The bounds of the sums are DERIVED from the inputs.  With u = 2^-53, a float64 sum of n products in any order, fused
or not, is within (n + 1) u sum|a||x| of the exact one, so the device and NumPy's ``A @ Xd`` differ by at most
``2 (n + 2) u (|A| @ |Xd|)``; the squared deviations add one subtraction and one square per term:
``2 (n + 4) u (A @ (Xd - centre)^2)`` for A >= 0.  Both are taken on the STORED values (what a float32 block holds).
The per-group statistics use DESIGN 5.3's ``b_mean`` / ``b_var`` with the group's own rows and count (the weight
1 / count is one rounding, the one the mean's division makes).  The anomaly model is judged by the bound that
tests/anomaly_restatement.py derives, twice over (the device and the restatement are each within it).  Every copy is
compared exactly: the kernel makes the float64 roundings of the NumPy expression and one rounding to the stored type."""
import warnings

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend

import anomaly_restatement as ar

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# 2500 is above the largest number of row slabs the launcher chooses (2048)
ROWS = [1, 2, 127, 128, 129, 1000, 2500]
COLS = [1, 127, 128, 129, 167, 257]


def _columns(rng, n, p):
    """standard_normal * uniform(0.1, 5) + offset; even columns: offset 1e4 * uniform(-1, 1), odd columns: 0."""
    offset = 1e4 * rng.uniform(-1.0, 1.0, size=p)
    offset[1::2] = 0.0
    return rng.standard_normal((n, p)) * rng.uniform(0.1, 5.0, size=p) + offset


def _stored(A, dtype):
    return A.astype(np.float32).astype(np.float64) if dtype == "float32" else A


def _device_data(ctx, X):
    ctx.set_data(X)
    return cdr.DeviceData(ctx, X.shape, None, X.shape[1:])


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err > 0, err / bound, 0.0).max())


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_sums_against_float64_numpy(dtype, n):
    rng = np.random.RandomState(500 + n)
    worst = worst_sq = 0.0
    with _backend.Context(dtype=dtype) as ctx:
        for p in COLS:
            ctx.set_data(_columns(rng, n, p))
            Xd = ctx.get_data()
            for G in (1, 14, 16):
                msg = "dtype=%s n=%d p=%d G=%d" % (dtype, n, p, G)
                A = rng.standard_normal((G, n)) * rng.uniform(0.01, 10.0, size=(G, 1))
                A[:, rng.uniform(size=n) < 0.3] = 0.0                       # rows of X that do not count
                if G > 1:
                    A[G // 2] = 0.0                                          # a coefficient row of zeros
                out = ctx.data_weighted_column_sums(A)
                assert out.shape == (G, p) and out.dtype == np.float64, msg
                err, bound = np.abs(out - A.dot(Xd)), 2 * (n + 2) * U * np.abs(A).dot(np.abs(Xd))
                worst = max(worst, _ratio(err, bound))
                assert np.all(err <= bound), msg
                if G > 1:
                    assert np.array_equal(out[G // 2], np.zeros(p)), msg
                assert np.array_equal(ctx.data_weighted_column_sums(A), out), msg     # the same bits on every call
                # squared deviations from a per-group table; label -1: the row is not counted
                Gc = (1, 12, 16)[(1, 14, 16).index(G)]
                grp = rng.randint(-1, Gc, size=n)
                centre = _columns(rng, Gc, p)
                W = np.abs(A)
                sq = ctx.data_weighted_column_sums(W, groups=grp, centre=centre)
                dev2 = np.where((grp >= 0)[:, None], (Xd - centre[np.maximum(grp, 0)]) ** 2, 0.0)
                want = W.dot(dev2)
                err, bound = np.abs(sq - want), 2 * (n + 4) * U * want
                worst_sq = max(worst_sq, _ratio(err, bound))
                assert sq.shape == (G, p) and np.all(err <= bound), msg
                assert np.array_equal(ctx.data_weighted_column_sums(W, groups=grp, centre=centre), sq), msg
    print("largest error / bound over the cases of n=%d, %s: sums %.3f, squared deviations %.3f (allowed 1)"
          % (n, dtype, worst, worst_sq))


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_model_copy_is_exact(dtype, n):
    """Each combination of present and absent parts, whole blocks and sub-blocks, G = 1, 12, 16."""
    rng = np.random.RandomState(600 + n)
    with _backend.Context(dtype=dtype) as ctx, _backend.Context(dtype=dtype) as block:
        for p, G in zip(COLS, (1, 12, 16, 12, 16, 1)):
            ctx.set_data(_columns(rng, n, p))
            Xd = ctx.get_data()
            shift, scale = _columns(rng, G, p), rng.uniform(0.5, 2.0, size=(G, p)) * rng.choice([-1.0, 1.0], size=(G, p))
            icpt, slope = rng.standard_normal(p) * 100.0, rng.standard_normal(p) * 0.1
            for row0, nb in ((0, n), (n - 1, 1), (n // 3, n - n // 3), (1, n // 2)):
                if nb < 1 or row0 + nb > n:
                    continue
                grp = rng.randint(0, G, size=nb)
                t = np.arange(row0, row0 + nb, dtype=np.float64) * rng.choice([1.0, 1.0 / 3.0])
                for parts in range(8):
                    use_shift, use_trend, use_scale = parts & 1, parts & 2, parts & 4
                    want = Xd[row0:row0 + nb]
                    if use_shift:
                        want = want - shift[grp]
                    if use_trend:
                        want = want - (icpt + slope * t[:, None])
                    if use_scale:
                        want = want / scale[grp]
                    block.set_data_rows_model(ctx, row0, nb, groups=grp if (use_shift or use_scale) else None,
                                              shift=shift if use_shift else None,
                                              intercept=icpt if use_trend else None,
                                              slope=slope if use_trend else None, t=t if use_trend else None,
                                              scale=scale if use_scale else None)
                    assert (block.n, block.p) == (nb, p)
                    assert np.array_equal(block.get_data(), _stored(want, dtype)), (dtype, n, p, G, row0, nb, parts)
                if G == 1:                                                   # one group needs no labels
                    block.set_data_rows_model(ctx, row0, nb, shift=shift, scale=scale)
                    assert np.array_equal(block.get_data(), _stored((Xd[row0:row0 + nb] - shift[0]) / scale[0], dtype))


ANOMALY_CASES = [(25, 12, None, 1), (129, 5, None, 1), (1000, 12, (240, 720), 1), (2500, 12, None, 1),
                 (129, 5, (3, 100), 0), (64, 1, None, 1)]


@pytest.fixture(scope="module")
def anomaly_inputs():
    """The columns of every end-to-end case with the restatement's model and bound on the STORED values, per dtype:
    computed once, read by the tests."""
    out = {}
    for n, period, base, order in ANOMALY_CASES:
        X = ar.columns(np.random.RandomState(700 + n + period), n, 167, period)
        for dtype in ("float64", "float32"):
            Xd = _stored(X, dtype)
            out[n, period, base, order, dtype] = (X, Xd, ar.restate(Xd, period, base, order),
                                                  ar.model_bound(Xd, period, base, order))
    return out


@pytest.mark.parametrize("n,period,base,order", ANOMALY_CASES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_seasonal_anomalies_end_to_end(anomaly_inputs, dtype, n, period, base, order):
    X, Xd, (cycle, slope, icpt), bound = anomaly_inputs[n, period, base, order, dtype]
    p = X.shape[1]
    with _backend.Context(dtype=dtype) as ctx:
        D = _device_data(ctx, X)
        assert D.anomaly is None and np.array_equal(D.to_host(), Xd)
        with D.seasonal_anomalies(period=period, base_rows=base, trend_order=order) as Y:
            rec = Y.anomaly
            assert isinstance(rec, cdr.SeasonalAnomalies) and rec.period == period
            assert rec.base_rows == ((0, n) if base is None else base)
            assert Y.shape == D.shape and Y.dtype == D.dtype and Y.scaling is None and Y.group_scaling is None
            # the sums: within twice the host test's bound of the restatement
            assert rec.seasonal_cycle.shape == (period, p)
            r_cycle = _ratio(np.abs(rec.seasonal_cycle - cycle), bound[:period])
            assert np.all(np.abs(rec.seasonal_cycle - cycle) <= 2 * bound[:period])
            phase, t = np.arange(n) % period, np.arange(n, dtype=np.float64)
            want = Xd - rec.seasonal_cycle[phase]
            if order:
                r_slope = _ratio(np.abs(rec.slope - slope), bound[period])
                r_icpt = _ratio(np.abs(rec.intercept - icpt), bound[period + 1])
                assert np.all(np.abs(rec.slope - slope) <= 2 * bound[period])
                assert np.all(np.abs(rec.intercept - icpt) <= 2 * bound[period + 1])
                want = want - (rec.intercept + rec.slope * t[:, None])
                print("n=%d P=%d %s: largest error / bound: cycle %.4f, slope %.4f, intercept %.4f (allowed 2)"
                      % (n, period, dtype, r_cycle, r_slope, r_icpt))
            else:
                assert rec.slope is None and rec.intercept is None
                print("n=%d P=%d %s: largest error / bound: cycle %.4f (allowed 2)" % (n, period, dtype, r_cycle))
            if period == 1:
                assert np.array_equal(rec.seasonal_cycle, np.zeros((1, p)))
            # the copy: exact given the record's own tables
            assert np.array_equal(Y.to_host(), _stored(want, dtype))
            # the model belongs to the row index: blocks cut from this one carry no record
            with Y.rows(0, min(n, 7)) as head, Y.take([n - 1, 0]) as picked:
                assert head.anomaly is None and picked.anomaly is None
                assert np.array_equal(picked.to_host(), Y.to_host()[[n - 1, 0]])
        # the source is left as it was
        assert np.array_equal(ctx.get_data(), Xd)


@pytest.mark.parametrize("n", [25, 129, 2500])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_grouped_stats_and_standardisation(dtype, n):
    rng = np.random.RandomState(800 + n)
    worst_mean = worst_var = 0.0
    with _backend.Context(dtype=dtype) as ctx, _backend.Context(dtype=dtype) as other:
        for p, G in ((129, 12), (167, 16), (1, 1)):
            D = _device_data(ctx, _columns(rng, n, p))
            Xd = D.to_host()
            groups = np.arange(n) % G if G != 16 else np.concatenate([np.arange(G), rng.randint(0, G, size=n - G)])
            for rows in (None, (n // 5, n)):
                msg = "dtype=%s n=%d p=%d G=%d rows=%r" % (dtype, n, p, G, rows)
                lo, hi = (0, n) if rows is None else rows
                if np.bincount(groups[lo:hi], minlength=G).min() == 0:
                    with pytest.raises(ValueError, match="no counted row"):
                        D.grouped_column_stats(groups, rows=rows)
                    continue
                stats = D.grouped_column_stats(groups, rows=rows)
                assert isinstance(stats, cdr.GroupedColumnStats)
                assert stats.mean.shape == (G, p) and stats.std.shape == (G, p), msg
                assert np.array_equal(stats.counts, np.bincount(groups[lo:hi], minlength=G)), msg
                for g in range(G):
                    sel = Xd[lo:hi][groups[lo:hi] == g]
                    cnt = sel.shape[0]
                    b_mean = cnt * U * np.abs(sel).mean(axis=0)
                    b_var = (cnt + 4) * U * sel.var(axis=0) + b_mean ** 2
                    e_mean = np.abs(stats.mean[g] - sel.mean(axis=0))
                    e_var = np.abs(stats.std[g] ** 2 - sel.var(axis=0))
                    worst_mean = max(worst_mean, _ratio(e_mean, b_mean))
                    assert np.all(e_mean <= 2 * b_mean), (msg, g)
                    if cnt == 1:
                        assert np.array_equal(stats.std[g], np.zeros(p)), (msg, g)
                    else:
                        # std^2 is var up to the two roundings of sqrt and the square: 3 u var
                        worst_var = max(worst_var, _ratio(e_var, b_var + 3 * U * sel.var(axis=0)))
                        assert np.all(e_var <= 2 * b_var + 3 * U * sel.var(axis=0)), (msg, g)
            # the copy is exact given the statistics: own, a base period's, another block's
            own = D.grouped_column_stats(groups) if n >= 2 * G else None
            foreign = cdr.GroupedColumnStats(_columns(rng, G, p), rng.uniform(0.5, 2.0, size=(G, p)), None)
            E = _device_data(other, _columns(rng, 2 * G + 3, p))
            theirs = E.grouped_column_stats(np.arange(2 * G + 3) % G)
            for stats in (own, foreign, theirs):
                if stats is None or np.any(stats.std == 0):
                    continue
                for center in (True, False):
                    with D.standardized_by_group(groups, stats=stats, center=center) as Y:
                        want = (Xd - stats.mean[groups] if center else Xd) / stats.std[groups]
                        assert np.array_equal(Y.to_host(), _stored(want, dtype)), (dtype, n, p, G, center)
                        assert Y.group_scaling.stats is stats and Y.group_scaling.center is center
                        assert np.array_equal(Y.group_scaling.groups, groups)
                        assert Y.anomaly is None and Y.shape == D.shape and Y.dtype == D.dtype
            if own is not None and not np.any(own.std == 0):
                with D.standardized_by_group(groups) as Y:                  # stats=None: the block's own
                    assert np.array_equal(Y.group_scaling.stats.mean, own.mean)
                    assert np.array_equal(Y.to_host(), _stored((Xd - own.mean[groups]) / own.std[groups], dtype))
            # a group of zero rows has mean 0 and std 0 exactly: refused before anything is copied
            if G > 1 and n >= 2 * G:
                flat = Xd.copy()
                flat[groups == 1] = 0.0
                F = _device_data(other, flat)
                with pytest.raises(ValueError, match="group 1, column 0"):
                    F.standardized_by_group(groups)
    print("largest error / bound over the cases of n=%d, %s: mean %.3f, var %.3f (allowed 2)"
          % (n, dtype, worst_mean, worst_var))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_padding_stays_zero_seen_through_the_solvers(dtype):
    """A non-zero padding column or row of the anomalies block would enter the Gram products of the pass kernels:
    fits on the resident block and on a fresh upload of its values must agree bit for bit."""
    rng = np.random.RandomState(900)
    n, p, k = 129, 167, 3
    X = ar.columns(rng, n, p, 12)
    with _backend.Context(dtype=dtype) as ctx:
        D = _device_data(ctx, X)
        A = D.seasonal_anomalies(period=12)
        Y = A.standardized_by_group(np.arange(n) % 12, stats=A.grouped_column_stats(np.arange(n) % 12, rows=(12, 108)))
        A.close()
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
    Y.close()


def test_entry_point_refusals():
    rng = np.random.RandomState(0)
    A = rng.standard_normal((20, 6))
    B = rng.standard_normal((7, 4))
    ones, coef = np.ones((2, 6)), rng.standard_normal((3, 20))
    labels = np.arange(20) % 2
    with _backend.Context(dtype="float64") as owner, _backend.Context(dtype="float64") as target:
        with pytest.raises(RuntimeError, match="error -3:"):                 # AA_ERR_STATE: no data yet
            owner.data_weighted_column_sums(np.ones((1, 0)))
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_model(owner, 0, 1)
        owner.set_data(A)
        target.set_data(B)
        with pytest.raises(RuntimeError, match="error -1:"):                 # more than 16 coefficient rows
            owner.data_weighted_column_sums(np.ones((17, 20)))
        for bad in (-2, 2, 16):                                              # a label outside [-1, Gc)
            grp = labels.copy()
            grp[5] = bad
            with pytest.raises(RuntimeError, match="error -1:"):
                owner.data_weighted_column_sums(np.abs(coef), groups=grp, centre=ones)
        with pytest.raises(ValueError):                                      # the binding checks the shapes
            owner.data_weighted_column_sums(np.ones((3, 19)))
        with pytest.raises(ValueError):
            owner.data_weighted_column_sums(np.abs(coef), groups=labels, centre=np.ones((2, 5)))
        for row0, nb in ((-1, 5), (0, 0), (0, 21), (20, 1), (5, 16)):
            with pytest.raises(RuntimeError, match="error -1:"):             # AA_ERR_ARG: bad row block
                target.set_data_rows_model(owner, row0, nb)
        with pytest.raises(RuntimeError, match="error -1:"):                 # ctx == owner
            owner.set_data_rows_model(owner, 0, 5)
        with _backend.Context(dtype="float32") as other:
            with pytest.raises(RuntimeError, match="error -1:"):             # dtype mismatch
                other.set_data_rows_model(owner, 0, 5)
        # refused, and the target keeps its data: too many groups, a label without a table row, a zero or non-finite
        # divisor, a non-finite shift, slope, intercept or time
        def table(value, at=(1, 3)):
            out = np.ones((2, 6))
            out[at] = value
            return out
        t10, lab10 = np.arange(10.0), labels[:10]
        for kw in (dict(groups=np.zeros(10, dtype=int), scale=np.ones((17, 6))),
                   dict(groups=np.where(np.arange(10) == 4, 2, lab10), scale=ones),
                   dict(groups=np.where(np.arange(10) == 4, -1, lab10), shift=ones),
                   dict(scale=ones),                                          # two groups, no labels
                   dict(groups=lab10, scale=table(0.0)), dict(groups=lab10, scale=table(-0.0)),
                   dict(groups=lab10, scale=table(np.inf)), dict(groups=lab10, scale=table(np.nan)),
                   dict(groups=lab10, shift=table(np.inf)), dict(groups=lab10, shift=table(np.nan), scale=ones),
                   dict(intercept=np.zeros(6), slope=table(np.nan)[1], t=t10),
                   dict(intercept=table(np.inf)[1], slope=np.zeros(6), t=t10),
                   dict(intercept=np.zeros(6), slope=np.zeros(6), t=np.where(t10 == 3, np.nan, t10))):
            with pytest.raises(RuntimeError, match="error -1:"):
                target.set_data_rows_model(owner, 0, 10, **kw)
            assert (target.n, target.p) == (7, 4)
            assert np.array_equal(target.get_data(), B)
        with pytest.raises(ValueError):                                      # the trend's parts come together
            target.set_data_rows_model(owner, 0, 10, slope=np.zeros(6))
        with pytest.raises(ValueError):
            target.set_data_rows_model(owner, 0, 10, groups=lab10, scale=np.ones((2, 5)))
        target.set_data_rows_model(owner, 2, 10, groups=lab10, scale=-ones)   # a negative divisor is a divisor
        assert np.array_equal(target.get_data(), -A[2:12])
    K = rng.standard_normal((12, 12))
    with _backend.Context(dtype="float64") as ctx, _backend.Context(dtype="float64") as target:
        ctx.set_data(K.dot(K.T), form=_backend.FORM_KERNEL)
        with pytest.raises(RuntimeError, match="error -3:"):                 # kernel form
            ctx.data_weighted_column_sums(np.ones((1, 12)))
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_model(ctx, 0, 5)
