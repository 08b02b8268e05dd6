"""Reconstruction scores and time-series cross-validation, host side (no GPU needed): the fold
arithmetic against scikit-learn, the derived scores against NumPy / scikit-learn, refusals that must
happen before any device call, and the two new entry points in header, library and binding."""
import ctypes
import os
import re

import numpy as np
import pytest
from sklearn.model_selection import TimeSeriesSplit

import convex_dim_red as cdr
from convex_dim_red import _backend, validation
from convex_dim_red.preprocessing import DeviceData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


def test_time_series_folds_are_scikit_learns():
    accepted = refused = 0
    for n in range(2, 61):
        for f in range(2, 11):
            try:
                want = [(int(tr[-1]) + 1, int(te[0]), int(te[-1]) + 1)
                        for tr, te in TimeSeriesSplit(n_splits=f).split(np.arange(n))]
            except ValueError:
                with pytest.raises(ValueError):
                    cdr.time_series_folds(n, f)
                refused += 1
                continue
            got = cdr.time_series_folds(n, f)
            assert got == want, (n, f)
            assert all(isinstance(v, int) for fold in got for v in fold)
            accepted += 1
    assert accepted > 400 and refused > 0
    for bad in (1, 0, -3, 2.5, None):
        with pytest.raises(ValueError):
            cdr.time_series_folds(30, bad)


def test_scores_from_sums_against_numpy_and_scikit_learn():
    rng = np.random.RandomState(3)
    m, p = 57, 13
    X = rng.standard_normal((m, p)) * rng.uniform(0.1, 10.0, size=p)
    R = X + 0.3 * rng.standard_normal((m, p))              # "reconstruction"
    res = X - R
    s = validation._scores_from_sums((res ** 2).sum(axis=0), (res ** 2).sum(axis=1))
    try:
        from sklearn.metrics import root_mean_squared_error
        rmse = root_mean_squared_error(X, R)
    except ImportError:
        rmse = np.sqrt(((X - R) ** 2).mean(axis=0)).mean()
    assert abs(s.rmse - rmse) <= 1e-15 * rmse
    pooled = np.sqrt(((X - R) ** 2).mean())
    assert abs(s.rmse_pooled - pooled) <= 1e-15 * pooled
    cost = 0.5 * ((X - R) ** 2).sum() / m
    assert abs(s.cost - cost) <= 1e-15 * cost
    assert s.column_sse.shape == (p,) and s.sample_sse.shape == (m,)
    assert isinstance(s, cdr.Scores)


def _fitted_aa(k=2, p=3, m=5):
    model = cdr.ArchetypalAnalysis(k, random_state=0)
    model.archetypes = np.ones((k, p))
    model.weights = np.full((m, k), 1.0 / k)
    return model


def _fitted_gpnh(k=2, p=3, m=5):
    model = cdr.GPNHConvexCoding(k, random_state=0)
    model.dictionary = np.ones((p, k))
    model.weights = np.full((m, k), 1.0 / k)
    return model


def _fitted_kernel(form, k=2, p=3, n=12, m=5):
    model = cdr.KernelAA(k, random_state=0)
    model.dictionary = np.full((k, n), 1.0 / n)
    model.alpha = np.ones(k)
    model.weights = np.full((m, k), 1.0 / k)
    state = dict(form=form, n_samples=n, A=np.eye(k))
    if form != "kernel":
        state["n_features"] = p
    if form == "linear":
        state["archetypes"] = np.ones((k, p))
    model._transform_state = state
    return model


def test_score_refusals_happen_before_any_device_call(no_device):
    for model in (cdr.ArchetypalAnalysis(2, random_state=0), cdr.GPNHConvexCoding(2, random_state=0),
                  cdr.KernelAA(2, random_state=0)):
        with pytest.raises(ValueError, match="not fitted"):
            model.score(np.ones((5, 3)))
    for model in (_fitted_aa(), _fitted_gpnh(), _fitted_kernel("linear")):
        before = model.random_state.get_state()[1].copy()
        with pytest.raises(ValueError, match="3"):
            model.score(np.ones((5, 4)))                              # wrong width
        with pytest.raises(ValueError):
            model.score(np.ones(3))
        with pytest.raises(ValueError):
            model.score(np.ones((0, 3)))
        with pytest.raises(ValueError, match="weights"):
            model.score(np.ones((5, 3)), weights=np.ones((4, 2)))     # one row per row of data
        with pytest.raises(ValueError, match="weights"):
            model.score(np.ones((5, 3)), weights=np.ones((5, 3)))
        with pytest.raises(ValueError, match="weights"):
            model.score(np.ones((6, 3)))                              # the model's own weights: 5 rows
        model.weights = None
        with pytest.raises(ValueError, match="weights"):
            model.score(np.ones((5, 3)))
        assert np.array_equal(model.random_state.get_state()[1], before)   # no draws
    for form in ("kernel", "rbf"):
        with pytest.raises(ValueError, match="data-space"):
            _fitted_kernel(form).score(np.ones((5, 3)))


class _FakeContext(object):
    """Stands in for an open context: ``rows`` must decide everything it refuses without touching it."""
    h = 1
    dtype_code = _backend.AA_F64
    device = 0

    def close(self):
        self.h = None


def test_row_block_refusals_happen_before_any_device_call(no_device):
    dd = DeviceData(_FakeContext(), (10, 4), np.ones(4, dtype=bool), (4,))
    for args in ((3, 3), (5, 2), (-1, 4), (0, 11), (10, 12), (10,), (slice(4, 4),), (slice(7, 3),),
                 (slice(0, 10, 2),), (slice(None, None, -1),), (slice(0, 11),), (slice(-2, 5),), (1.5, 4),
                 (slice(0, 5), 7)):
        with pytest.raises(ValueError):
            dd.rows(*args)
    with pytest.raises(AssertionError, match="device call"):        # a good block gets as far as the device
        dd.rows(2, 6)
    dd.close()
    with pytest.raises(RuntimeError, match="closed"):
        dd.rows(2, 6)
    with pytest.raises(RuntimeError, match="closed"):
        dd.rows(slice(0, 10))
    with pytest.raises(ValueError):                                   # the range is still checked first
        dd.rows(0, 11)


def test_cross_validation_arguments_are_checked_before_any_device_call(no_device):
    def never():
        raise AssertionError("a model was made")
    with pytest.raises(ValueError):
        cdr.time_series_cross_validate(never, np.ones((5, 3)), n_folds=5)       # too few samples
    with pytest.raises(ValueError):
        cdr.time_series_cross_validate(never, np.ones(5), n_folds=2)
    with pytest.raises(ValueError):
        cdr.time_series_cross_validate(never, np.ones((50, 3)), n_folds=2, n_init=0)


def test_new_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "aa_hip.h")) as fh:
        header = fh.read()
    names = ("aa_gpnh_residual_scores", "aa_set_data_rows")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    if not os.path.exists(_backend.library_path()):
        pytest.fail("libaa_hip.so has not been built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_backend.library_path())
    for name in names:
        assert hasattr(lib, name), name
    assert cdr.Scores is validation.Scores
    for name in ("Scores", "time_series_folds", "time_series_cross_validate"):
        assert name in cdr.__all__
