"""Seasonal anomalies and per-group standardisation of resident data, host side (no GPU needed): the coefficient
matrix of ``seasonal_coefficients`` against a step-by-step NumPy restatement of the reference notebook
``hadisst_sst_anom.ipynb`` (tests/anomaly_restatement.py, which also derives the bound), the refusals that are
decided before any device call, and the new names in header, library, binding and package."""
import ctypes
import os
import re

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend, preprocessing
from convex_dim_red.preprocessing import DeviceData, GroupedColumnStats

import anomaly_restatement as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


class _FakeContext(object):
    """Stands in for an open context: what the new methods refuse they must refuse without touching it."""
    h = 1
    dtype_code = _backend.AA_F64
    device = 0

    def close(self):
        self.h = None

    def data_weighted_column_sums(self, *args, **kwargs):
        raise AssertionError("a device call was made")

    def set_data_rows_model(self, *args, **kwargs):
        raise AssertionError("a device call was made")


def _block(n=40, p=4):
    return DeviceData(_FakeContext(), (n, p), np.ones(p, dtype=bool), (p,))


@pytest.mark.parametrize("n,period,base", ar.CASES)
def test_coefficients_reproduce_the_restatement(n, period, base):
    """``seasonal_coefficients(...)[0] @ X`` against the notebook's steps with ``linregress`` per column, within
    ``C n u (A_parts @ |X|)``, C = 11 as derived in tests/anomaly_restatement.py."""
    rng = np.random.RandomState(n + period)
    X = ar.columns(rng, n, 10, period)
    A, parts = cdr.seasonal_coefficients(n, period, base)
    assert A.shape == parts.shape == (period + 2, n) and A.dtype == np.float64
    got = A.dot(X)
    cycle, slope, icpt = ar.restate(X, period, base)
    bound = ar.model_bound(X, period, base)
    err = np.abs(got - np.vstack([cycle, slope, icpt]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    print("n=%d P=%d: largest error / bound: cycle %.4f, slope %.4f, intercept %.4f (allowed 1)"
          % (n, period, ratio[:period].max(), ratio[period].max(), ratio[period + 1].max()))
    assert np.all(err <= bound)
    # the cycle has no mean over the phases, and without a trend the cycle rows are the same
    assert np.all(np.abs(got[:period].sum(axis=0)) <= bound[:period].sum(axis=0))
    A0, parts0 = cdr.seasonal_coefficients(n, period, base, trend_order=0)
    assert np.array_equal(A0, A[:period]) and np.array_equal(parts0, parts[:period])
    if base is None:
        assert np.array_equal(cdr.seasonal_coefficients(n, period, (0, n))[0], A)


def test_model_refusals_happen_before_any_device_call(no_device):
    dd = _block(40, 4)
    for call in (lambda **kw: cdr.seasonal_coefficients(40, **kw), lambda **kw: dd.seasonal_anomalies(**kw)):
        for period in (0, 15, -3, 2.0, None, True):
            with pytest.raises(ValueError, match="period"):
                call(period=period)
        for order in (2, -1, 1.0, None):
            with pytest.raises(ValueError, match="trend_order"):
                call(period=12, trend_order=order)
        for base in ((5, 5), (7, 3), (-1, 20), (0, 41), (40, 41), (0.0, 20), 7, (1, 2, 3)):   # empty, outside, malformed
            with pytest.raises(ValueError, match="base_rows"):
                call(period=12, base_rows=base)
        for base in ((6, 17), (0, 12), (30, 40), (34, 40)):             # a phase without a full-window base row
            with pytest.raises(ValueError, match="phase"):
                call(period=12, base_rows=base)
    for n, period in ((12, 12), (4, 5), (13, 14)):                      # n < 2 h + 1
        with pytest.raises(ValueError, match="window"):
            cdr.seasonal_coefficients(n, period)
        with pytest.raises(ValueError, match="window"):
            _block(n, 3).seasonal_anomalies(period=period)
    with pytest.raises(ValueError, match="2 rows"):
        cdr.seasonal_coefficients(1, 1)
    for n in (0, -4, 2.5):
        with pytest.raises(ValueError, match="positive integer"):
            cdr.seasonal_coefficients(n, 1)
    assert cdr.seasonal_coefficients(1, 1, trend_order=0)[0].shape == (1, 1)
    with pytest.raises(ValueError, match="phase 0"):                    # one full window serves phase 6 only
        cdr.seasonal_coefficients(13, 12)
    assert cdr.seasonal_coefficients(24, 12)[0].shape == (14, 24)       # t = 6 .. 17: every phase once
    # what is in order gets as far as the device
    with pytest.raises(AssertionError, match="device call"):
        dd.seasonal_anomalies()
    with pytest.raises(AssertionError, match="device call"):
        dd.seasonal_anomalies(period=5, base_rows=(3, 33), trend_order=0)
    dd.close()
    with pytest.raises(RuntimeError, match="closed"):
        dd.seasonal_anomalies()
    with pytest.raises(ValueError, match="period"):                     # the arguments are still checked first
        dd.seasonal_anomalies(period=15)


def test_group_refusals_happen_before_any_device_call(no_device):
    n, p = 24, 4
    dd = _block(n, p)
    months = np.arange(n) % 12
    good = GroupedColumnStats(np.zeros((12, p)), np.ones((12, p)), np.full(12, 2))
    for call in (dd.grouped_column_stats, lambda g: dd.standardized_by_group(g, stats=good)):
        for labels in (months[:-1], np.arange(n + 1) % 12, months.reshape(2, 12), 3):           # length / shape
            with pytest.raises(ValueError, match="one group label per row"):
                call(labels)
        for labels in (months.astype(float), months > 5, ["a"] * n):                              # dtype
            with pytest.raises(ValueError, match="integer group labels"):
                call(labels)
        bad = months.copy()
        bad[3] = -1
        with pytest.raises(ValueError, match="start at 0"):                                      # range
            call(bad)
        with pytest.raises(ValueError, match="more than 16 groups"):
            call(np.arange(n) % 17)
    assert preprocessing.MAX_GROUPS == 16
    with pytest.raises(ValueError, match="group 12 has no counted row"):    # label 12 is named, rows [0, 12) lack it
        dd.grouped_column_stats(np.arange(n) % 13, rows=(0, 12))
    with pytest.raises(ValueError, match="group 3 has no counted row"):
        dd.grouped_column_stats(np.where(months == 3, 4, months))
    for rows in ((5, 5), (-1, 4), (0, n + 1), (2.0, 8), 4):
        with pytest.raises(ValueError, match="rows"):
            dd.grouped_column_stats(months, rows=rows)
    # statistics: shape, zero / non-finite std, mean
    for std in (np.ones(p), np.ones((12, p + 1)), np.ones((11, p)), np.ones((17, p)), None):
        with pytest.raises(ValueError, match="stats.std"):
            dd.standardized_by_group(months, stats=GroupedColumnStats(np.zeros((12, p)), std, None))
    for value, count in ((0.0, 1), (-0.0, 1), (np.inf, 1), (np.nan, 1)):
        std = np.ones((12, p))
        std[7, 2] = value
        for center in (False, True):
            with pytest.raises(ValueError, match=r"%d entries.*group 7, column 2" % count):
                dd.standardized_by_group(months, stats=GroupedColumnStats(np.zeros((12, p)), std, None), center=center)
    with pytest.raises(ValueError, match="needs stats with a mean"):
        dd.standardized_by_group(months, stats=GroupedColumnStats(None, np.ones((12, p)), None))
    with pytest.raises(ValueError, match="shape of stats.std"):
        dd.standardized_by_group(months, stats=GroupedColumnStats(np.zeros((11, p)), np.ones((12, p)), None))
    with pytest.raises(ValueError, match="non-finite"):
        dd.standardized_by_group(months, stats=GroupedColumnStats(np.full((12, p), np.nan), np.ones((12, p)), None))
    # what is in order gets as far as the device
    for call in (lambda: dd.grouped_column_stats(months), lambda: dd.grouped_column_stats(months, rows=(6, 18)),
                 lambda: dd.standardized_by_group(months), lambda: dd.standardized_by_group(months, stats=good),
                 lambda: dd.standardized_by_group(months, center=False,
                                                  stats=GroupedColumnStats(None, np.ones((12, p)), None))):
        with pytest.raises(AssertionError, match="device call"):
            call()
    dd.close()
    for call in (lambda: dd.grouped_column_stats(months), lambda: dd.standardized_by_group(months),
                 lambda: dd.standardized_by_group(months, stats=good)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    with pytest.raises(ValueError):                                         # the labels are still checked first
        dd.grouped_column_stats(months[:-1])


def test_constructor_keeps_its_positional_arguments(no_device):
    import inspect
    spec = inspect.getfullargspec(DeviceData.__init__)
    assert spec.args[:6] == ["self", "ctx", "shape", "valid", "original_shape", "scaling"]
    assert spec.defaults == (None,) * (len(spec.args) - 5)
    plain = _block()
    assert plain.anomaly is None and plain.group_scaling is None and plain.scaling is None
    scaling = cdr.ColumnScaling(cdr.ColumnStats(np.zeros(4), np.ones(4), 3), False)
    assert DeviceData(_FakeContext(), (3, 4), None, (4,), scaling).scaling is scaling
    spec = inspect.getfullargspec(DeviceData.seasonal_anomalies)
    assert spec.args == ["self", "period", "base_rows", "trend_order"] and spec.defaults == (12, None, 1)


def test_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "aa_hip.h")) as fh:
        header = fh.read()
    names = ("aa_data_weighted_column_sums", "aa_data_grouped_sqdev", "aa_set_data_rows_model")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    if not os.path.exists(_backend.library_path()):
        pytest.fail("libaa_hip.so has not been built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_backend.library_path())
    for name in names:
        assert hasattr(lib, name), name
    for name in ("seasonal_coefficients", "SeasonalAnomalies", "GroupedColumnStats", "GroupScaling"):
        assert name in cdr.__all__ and getattr(cdr, name) is getattr(preprocessing, name)
    assert cdr.SeasonalAnomalies._fields == ("period", "base_rows", "seasonal_cycle", "slope", "intercept")
    assert cdr.GroupedColumnStats._fields == ("mean", "std", "counts")
    assert cdr.GroupScaling._fields == ("stats", "center", "groups")
    for method in ("seasonal_anomalies", "grouped_column_stats", "standardized_by_group"):
        assert callable(getattr(DeviceData, method))
    for method in ("data_weighted_column_sums", "set_data_rows_model"):
        assert callable(getattr(_backend.Context, method))
