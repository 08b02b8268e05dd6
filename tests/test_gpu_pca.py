"""PCA of resident data on the MI355X: aa_data_gram, aa_set_data_projected, DeviceData.pca and ResidentPCA.

Every bound is DERIVED from the inputs (tests/pca_restatement.py): the Gram matrix and the projection element-wise
against float64 NumPy on the STORED values, within the rounding bound of two evaluations of the same sums; the
end-to-end model against ``sklearn.decomposition.PCA(svd_solver='full')`` within twice the larger of the
restatement's own deviation from scikit-learn and the perturbation bound of the Gram rounding error (Weyl for the
eigenvalues, Davis-Kahan for the components) -- the device and the yardstick each commit that error once; the
scores at the tolerance tests/test_gpu_validation.py holds the same pass to.
"""
import warnings

import numpy as np
import pytest
from sklearn.decomposition import PCA

import convex_dim_red as cdr
from convex_dim_red import _backend

import pca_restatement as pr
from test_gpu_anomalies import _columns, _ratio, _stored
from test_gpu_validation import _reference

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GRAM_ROWS = [1, 2, 63, 64, 65, 129, 200]
GRAM_COLS = [1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 167, 257]
# read off csrc/gram_plan.h: several splits, the last one short (test_gram_plan_splits_the_gpu_test_shapes pins it)
SPLIT_SHAPES = pr.SPLIT_SHAPES


def _gram_case(ctx, Xd, side, centre, msg):
    shift = Xd.mean(axis=0) if centre else None
    G = ctx.data_gram(side, shift)
    d = Xd.shape[0] if side == "rows" else Xd.shape[1]
    assert G.shape == (d, d) and G.dtype == np.float64, msg
    err, bound = np.abs(G - pr.gram(Xd, shift, side)), pr.gram_bound(Xd, shift, side)
    assert np.all(err <= bound), (msg, _ratio(err, bound))
    assert np.array_equal(G, G.T), msg
    assert np.array_equal(ctx.data_gram(side, shift), G), msg               # the same bits on every call
    return _ratio(err, bound)


@pytest.mark.parametrize("side", ["rows", "cols"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gram_against_float64_numpy(dtype, side):
    """Even columns are offset by up to 1e4: a centred padding row or column would show as an error of order 1e8."""
    worst = 0.0
    with _backend.Context(dtype=dtype) as ctx:
        for n, p in [(n, p) for n in GRAM_ROWS for p in GRAM_COLS] + SPLIT_SHAPES[side]:
            ctx.set_data(_columns(np.random.RandomState(900 + n + p), n, p))
            Xd = ctx.get_data()
            for centre in (True, False):
                msg = "dtype=%s side=%s n=%d p=%d centre=%s" % (dtype, side, n, p, centre)
                worst = max(worst, _gram_case(ctx, Xd, side, centre, msg))
    print("largest error / bound over the Gram cases, %s by %s: %.3f (allowed 1)" % (dtype, side, worst))


def test_gram_entry_point_refusals():
    lib = _backend.load_library()
    out = np.empty((4, 4))
    ptr = out.ctypes.data_as(_backend._dp)
    with _backend.Context(dtype="float64") as ctx:
        assert lib.aa_data_gram(ctx.h, 0, None, ptr, 4) == -3                # no data
        rng = np.random.RandomState(0)
        G = rng.standard_normal((4, 4))
        ctx.set_data(G.dot(G.T), form=_backend.FORM_KERNEL)
        assert lib.aa_data_gram(ctx.h, 0, None, ptr, 4) == -3                # a kernel matrix
        ctx.set_rbf_features(rng.standard_normal((4, 3)), 0.5)
        assert lib.aa_data_gram(ctx.h, 0, None, ptr, 4) == -3                # an implicit kernel
        ctx.set_data(rng.standard_normal((4, 3)))
        assert lib.aa_data_gram(ctx.h, 2, None, ptr, 4) == -1                # no such side
        assert lib.aa_data_gram(ctx.h, 0, None, ptr, 3) == -1                # ldo < d
        assert lib.aa_data_gram(ctx.h, 0, None, None, 4) == -1
        assert lib.aa_data_gram(ctx.h, 0, None, ptr, 4) == 0
        ctx.set_data(np.zeros((3, 8193), dtype=np.float32))
        assert lib.aa_data_gram(ctx.h, 1, None, ptr, 8193) == -1             # d above the cap, before anything is written
        assert b"8192" in lib.aa_last_error()
        assert ctx.data_gram("rows").shape == (3, 3)                         # the other side of the same block is fine


PROJ_P = [1, 5, 127, 128, 129, 257]
PROJ_Q = [1, 15, 16, 17, 64, 167, 256]
FIT_Q = (1, 17, 167, 256)                 # where the fit on the block is compared with the fit on its download


def _gpnh(dtype, k):
    return cdr.GPNHConvexCoding(k, lambda_W=0.5, init="random", random_state=0, tolerance=1e-6, max_iterations=5,
                                dtype=dtype, weights_solver_kwargs=dict(max_iterations=1))


@pytest.mark.parametrize("m", [1, 15, 16, 17, 129, 1000])
@pytest.mark.parametrize("src,dst", [("float64", "float64"), ("float32", "float64"), ("float32", "float32")])
def test_projection_against_float64_numpy(src, dst, m):
    rng = np.random.RandomState(1000 + m)
    worst = 0.0
    with _backend.Context(dtype=src) as owner, _backend.Context(dtype=dst) as block:
        for p in PROJ_P:
            owner.set_data(_columns(rng, m, p))
            Xd = owner.get_data()
            for q in PROJ_Q:
                V = rng.standard_normal((q, p)) * rng.uniform(0.1, 3.0, size=(q, 1))
                if q > 1:
                    V[q // 2] = 0.0                                          # a direction of zeros
                shift = Xd.mean(axis=0) if q % 2 else None                   # centred and not
                for row0, nb in ((0, m), (m - 1, 1), (m // 3, m - m // 3), (1, m // 2)):
                    if nb < 1 or row0 + nb > m:
                        continue
                    msg = "%s->%s m=%d p=%d q=%d rows [%d, %d)" % (src, dst, m, p, q, row0, row0 + nb)
                    block.set_data_projected(owner, row0, nb, V, shift)
                    assert (block.n, block.p) == (nb, q), msg
                    Y = block.get_data()
                    rows = Xd[row0:row0 + nb]
                    err, bound = np.abs(Y - pr.project(rows, shift, V)), pr.project_bound(rows, shift, V, dst)
                    worst = max(worst, _ratio(err, bound))
                    assert np.all(err <= bound), (msg, _ratio(err, bound))
                    if q > 1:
                        assert np.array_equal(Y[:, q // 2], np.zeros(nb)), msg
                    if dst == "float32":
                        assert np.array_equal(Y, Y.astype(np.float32).astype(np.float64)), msg
                    if p == 129 and q in FIT_Q and row0 == 0 and nb == m:
                        # the block obeys the layout of an upload: a fit on it is the fit on its values, bit for bit
                        dd = cdr.DeviceData(block, (nb, q), None, (q,))
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            a, b = _gpnh(dst, min(3, q, nb)), _gpnh(dst, min(3, q, nb))
                            Za = a.fit_transform(dd)
                            Zb = b.fit_transform(Y.astype(np.float32) if dst == "float32" else Y)
                        assert a.cost == b.cost and a.n_iter == b.n_iter and np.array_equal(Za, Zb), msg
                        assert np.array_equal(a.dictionary, b.dictionary), msg
    print("largest error / bound over the projections of m=%d, %s -> %s: %.3f (allowed 1)" % (m, src, dst, worst))


def test_projection_entry_point_refusals():
    rng = np.random.RandomState(2)
    A, B = rng.standard_normal((20, 6)), rng.standard_normal((7, 4))
    V = rng.standard_normal((3, 6))
    with _backend.Context(dtype="float64") as owner, _backend.Context(dtype="float64") as block, \
            _backend.Context(dtype="float32") as single:
        owner.set_data(A)
        block.set_data(B)
        single.set_data(B)

        def refused(target, *args):
            with pytest.raises(RuntimeError, match="error -1"):
                target.set_data_projected(owner, *args)
            assert (target.n, target.p) == B.shape and np.array_equal(target.get_data(), _stored(B, "float32")
                                                                      if target is single else B)
        refused(block, 0, 21, V)                                             # more rows than the owner holds
        refused(block, 19, 2, V)
        refused(block, -1, 2, V)
        refused(block, 0, 0, V)
        refused(block, 0, 20, rng.standard_normal((257, 6)))                 # more than 256 directions
        for bad in (np.nan, np.inf):
            Vb, sb = V.copy(), np.zeros(6)
            Vb[2, 5], sb[3] = bad, bad
            refused(block, 0, 20, Vb)
            refused(block, 0, 20, V, sb)
        refused(single, 0, 20, V)                                            # float64 rows are not narrowed
        with pytest.raises(ValueError):
            block.set_data_projected(owner, 0, 20, V[:, :5])
        block.set_data_projected(owner, 0, 20, V)
        assert (block.n, block.p) == (20, 3)


# ------------------------------------------------------------------ end to end
E2E = [(40, 300, 8), (300, 40, 8), (129, 257, 12), (1000, 167, 12), (17, 16, 5)]


@pytest.fixture(scope="module")
def yardsticks():
    """Per (shape, dtype, side): the stored input, scikit-learn's full PCA with its PCs, the restatement and its
    deviation from scikit-learn -- computed once, read by the tests."""
    out = {}
    for n, p, q in E2E:
        for dtype in ("float64", "float32"):
            Xd = pr.stored(pr.low_rank(n, p, q), dtype)
            sk = PCA(n_components=q, svd_solver="full").fit(Xd)
            sk_pcs = sk.transform(Xd)
            for side in ("rows", "cols"):
                m = pr.fit(Xd, q, side=side)
                own = dict(lam=np.abs(m.eigenvalues_[:q] - sk.singular_values_ ** 2).max(),
                           sin=pr.sines(m.components_, sk.components_).max(),
                           pcs=np.abs(pr.project(Xd, m.mean_, m.components_) - sk_pcs).max())
                out[n, p, q, dtype, side] = (Xd, sk, sk_pcs, m, own)
    return out


@pytest.mark.parametrize("side", ["rows", "cols"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,p,q", E2E)
def test_pca_against_sklearn_full(yardsticks, n, p, q, dtype, side):
    Xd, sk, sk_pcs, rest, own = yardsticks[n, p, q, dtype, side]
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(Xd)
        block = cdr.DeviceData(ctx, Xd.shape, None, Xd.shape[1:])
        assert np.array_equal(block.to_host(), Xd)
        model = block.pca(q, side=side)
        with model.transform(block) as projected:
            pcs = projected.to_host()
            assert projected.shape == (n, q) and projected.dtype == np.float64
        if (n, p) == (129, 257):
            for k in (1, 5, 12):
                cut, direct = model.truncate(k), block.pca(k, side=side)
                for name in ("components_", "explained_variance_", "explained_variance_ratio_", "singular_values_",
                             "noise_variance_", "eigenvalues_", "mean_"):
                    assert np.array_equal(getattr(cut, name), getattr(direct, name)), (k, name)
    assert model.side_ == side and model.n_components_ == q and model.components_.shape == (q, p)
    assert (model.n_samples_, model.n_features_in_) == (n, p)
    lam_sk = sk.singular_values_ ** 2
    weyl, dk = pr.perturbation_bounds(Xd, rest.mean_, side, rest.eigenvalues_, q)
    # the mean: two float64 evaluations of a mean of n values
    assert np.all(np.abs(model.mean_ - sk.mean_) <= 2 * (n + 2) * U * np.abs(Xd).mean(axis=0))
    d_lam = np.abs(model.eigenvalues_[:q] - lam_sk).max()
    sin = pr.sines(model.components_, sk.components_)
    row_norm = np.linalg.norm(pr.centred(Xd, rest.mean_), axis=1)
    pcs_bound = np.outer(row_norm, np.sqrt(2.0) * dk) + pr.project_bound(Xd, rest.mean_, rest.components_)
    # components, and with them the PCs, are compared after aligning signs by their dot product
    d_pcs = np.abs(pcs * np.sign(np.sum(model.components_ * sk.components_, axis=1)) - sk_pcs)
    print("%dx%d q=%d %s by %s, device / allowed: eigenvalues %.3g / %.3g (restatement %.3g, Weyl %.3g); max sin "
          "%.3g / %.3g (restatement %.3g, Davis-Kahan %.3g); PCs %.3g / %.3g (restatement %.3g)"
          % (n, p, q, dtype, side, d_lam, 2 * max(own["lam"], weyl), own["lam"], weyl, sin.max(),
             2 * max(own["sin"], dk.max()), own["sin"], dk.max(), d_pcs.max(), 2 * max(own["pcs"], pcs_bound.max()),
             own["pcs"]))
    assert d_lam <= 2 * max(own["lam"], weyl)
    assert np.all(sin <= 2 * np.maximum(own["sin"], dk))
    assert np.all(d_pcs <= 2 * np.maximum(own["pcs"], pcs_bound))
    # the signs themselves, wherever the two largest magnitudes of a component differ by more than its entries can move
    top = np.sort(np.abs(sk.components_), axis=1)[:, -2:]
    decided = top[:, 1] - top[:, 0] > 2 * np.sqrt(2.0) * 2 * np.maximum(own["sin"], dk)
    assert decided.any()
    assert np.all(np.sum(model.components_ * sk.components_, axis=1)[decided] > 0)
    pick = np.argmax(np.abs(model.components_), axis=1)
    assert np.all(model.components_[np.arange(q), pick] > 0)
    # the derived attributes are the stated functions of the eigenvalues
    lam = model.eigenvalues_
    assert lam.shape == ((n if side == "rows" else p),) and np.all(lam[:-1] >= lam[1:]) and lam[-1] >= 0
    assert np.array_equal(model.explained_variance_, lam[:q] / (n - 1))
    assert np.array_equal(model.explained_variance_ratio_, lam[:q] / lam.sum())
    assert np.array_equal(model.singular_values_, np.sqrt(lam[:q]))
    assert model.noise_variance_ == lam[q:min(n, p)].mean() / (n - 1)
    assert abs(model.noise_variance_ - sk.noise_variance_) <= (2 * max(own["lam"], weyl) / (n - 1)
                                                               + 1e-12 * sk.noise_variance_)


def test_pca_auto_side_and_uncentred():
    for (n, p), want in (((40, 300), "rows"), ((300, 40), "cols"), ((64, 64), "rows")):
        Xd = pr.low_rank(n, p, 4)
        with _backend.Context(dtype="float64") as ctx:
            ctx.set_data(Xd)
            block = cdr.DeviceData(ctx, Xd.shape, None, Xd.shape[1:])
            model = block.pca(4)
            plain = block.pca(4, center=False)
        assert model.side_ == want and plain.side_ == want
        assert np.array_equal(plain.mean_, np.zeros(p)) and not plain.centered_
        rest = pr.fit(Xd, 4, center=False)
        weyl, dk = pr.perturbation_bounds(Xd, None, want, rest.eigenvalues_, 4)
        assert np.abs(plain.eigenvalues_[:4] - rest.eigenvalues_[:4]).max() <= 2 * weyl
        assert np.all(pr.sines(plain.components_, rest.components_) <= 2 * dk)


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("q", [1, 12, 63])
def test_score_against_float64_numpy(dtype, q):
    n, p, m = 300, 129, 77
    X = pr.low_rank(n + m, p, 70)
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(X)
        whole = cdr.DeviceData(ctx, X.shape, None, X.shape[1:])
        with whole.rows(0, n) as train, whole.rows(n, n + m) as test:
            model = train.pca(q)
            for block in (train, test):                                      # a validation block takes the training model
                Xd = block.to_host()
                with model.transform(block) as projected:
                    pcs = projected.to_host()
                s = model.score(block, pcs=pcs)
                Z = np.hstack([pcs, np.ones((Xd.shape[0], 1))])
                Wt = np.vstack([model.components_, model.mean_])
                (col_w, row_w, sse_w), (col_b, row_b, sse_b) = _reference(Xd, Z, Wt)
                direct = Xd - (pcs.dot(model.components_) + model.mean_)
                assert np.abs((direct * direct).sum(axis=0) - col_w).max() <= col_b.max()
                print("q=%d %s %d rows: largest error / bound %.3f (allowed 4), rmse %.6g"
                      % (q, dtype, Xd.shape[0], max(_ratio(np.abs(s.column_sse - col_w), col_b),
                                                    _ratio(np.abs(s.sample_sse - row_w), row_b)), s.rmse))
                assert np.all(np.abs(s.column_sse - col_w) <= 4 * col_b)
                assert np.all(np.abs(s.sample_sse - row_w) <= 4 * row_b)
                assert abs(s.cost - 0.5 * sse_w / Xd.shape[0]) <= 4 * sse_b / (2 * Xd.shape[0])
                assert s.rmse == np.sqrt(s.column_sse / Xd.shape[0]).mean()
                # pcs left out: the model's own transform of the block, the same bits
                again = model.score(block)
                assert np.array_equal(again.column_sse, s.column_sse) and again.cost == s.cost
                assert np.array_equal(model.score(block, pcs=projected).sample_sse, s.sample_sse)
            if q == 63:
                wide = train.pca(64)
                with pytest.raises(ValueError, match="64 components"):
                    wide.score(train)
                assert wide.truncate(63).score(train).cost > 0


# ------------------------------------------------------------------ the C3 pipeline
def test_pipeline_from_the_raw_field_to_a_gpnh_fit():
    """weight_and_flatten_on_device -> seasonal_anomalies -> pca(12) -> transform -> GPNHConvexCoding.fit_transform:
    nothing but the raw field goes up, nothing but models and weights comes down."""
    rng = np.random.RandomState(7)
    n_time, n_lat, n_lon, q, k = 240, 9, 14, 12, 3
    t = np.arange(n_time)
    modes = rng.standard_normal((q + 2, n_lat * n_lon))
    series = rng.standard_normal((n_time, q + 2)) * (3.0 * 0.8 ** np.arange(q + 2))
    field = (series.dot(modes) + 2.0 * np.sin(2 * np.pi * t / 12.0)[:, None] + 0.01 * t[:, None]
             + 0.01 * rng.standard_normal((n_time, n_lat * n_lon)) + 280.0).reshape(n_time, n_lat, n_lon)
    field[:, 2, 3:6] = np.nan
    weights = np.sqrt(np.cos(np.deg2rad(np.linspace(-60, 60, n_lat))))[:, None]
    with cdr.weight_and_flatten_on_device(field, weights, dtype="float64") as raw, raw.seasonal_anomalies() as anom:
        model = anom.pca(q)
        with model.transform(anom) as pcs:
            assert pcs.shape == (n_time, q)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                a, b = _gpnh("float64", k), _gpnh("float64", k)
                Za = a.fit_transform(pcs)
                Zb = b.fit_transform(pcs.to_host())
            scores = model.score(anom, pcs=pcs)
        host = anom.to_host()
    assert Za.shape == (n_time, k) and np.isfinite(a.cost)
    assert a.cost == b.cost and np.array_equal(Za, Zb)
    sk = PCA(n_components=q, svd_solver="full").fit(host)
    assert np.allclose(model.explained_variance_, sk.explained_variance_, rtol=1e-9, atol=0)
    assert np.all(np.abs(np.sum(model.components_ * sk.components_, axis=1)) > 1 - 1e-9)
    resid = host - sk.inverse_transform(sk.transform(host))
    assert abs(scores.rmse - np.sqrt((resid ** 2).mean(axis=0)).mean()) <= 1e-9 * scores.rmse
