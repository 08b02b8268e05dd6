"""Column statistics and standardisation of resident data, host side (no GPU needed): the refusals that are
decided from passed-in statistics before any device call, the arithmetic of ``unscale``, and the new names in
header, library, binding and package."""
import ctypes
import os
import re

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend, preprocessing
from convex_dim_red.preprocessing import ColumnScaling, ColumnStats, DeviceData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


class _FakeContext(object):
    """Stands in for an open context: what ``standardized`` refuses it must refuse without touching it."""
    h = 1
    dtype_code = _backend.AA_F64
    device = 0

    def close(self):
        self.h = None

    def data_column_moments(self):
        raise AssertionError("a device call was made")

    def set_data_rows_affine(self, *args):
        raise AssertionError("a device call was made")


def _block(n=10, p=4, scaling=None):
    return DeviceData(_FakeContext(), (n, p), np.ones(p, dtype=bool), (p,), scaling)


def test_standardize_refusals_happen_before_any_device_call(no_device):
    dd = _block()
    good = ColumnStats(np.zeros(4), np.ones(4), 10)
    for std in (np.ones(3), np.ones(5), np.ones((4, 1)), 1.0, None):          # one value per feature
        for center in (False, True):
            with pytest.raises(ValueError, match="one value per feature"):
                dd.standardized(center=center, stats=ColumnStats(np.zeros(4), std, 10))
    with pytest.raises(ValueError, match="needs stats with a mean"):
        dd.standardized(center=True, stats=ColumnStats(None, np.ones(4), 10))
    with pytest.raises(ValueError, match="one value per feature"):
        dd.standardized(center=True, stats=ColumnStats(np.zeros(5), np.ones(4), 10))
    with pytest.raises(ValueError, match="non-finite"):
        dd.standardized(center=True, stats=ColumnStats(np.array([0, np.nan, 0, 0]), np.ones(4), 10))
    for std, count, first in (([1, 0.0, 1, 1], 1, 1), ([1, 1, 1, np.inf], 1, 3), ([np.nan, 1, -0.0, 1], 2, 0),
                              ([0.0, 0.0, 0.0, 0.0], 4, 0), ([2, 1, -np.inf, np.nan], 2, 2)):
        for center in (False, True):
            with pytest.raises(ValueError, match=r"%d column\(s\).*column %d\)" % (count, first)):
                dd.standardized(center=center, stats=ColumnStats(np.zeros(4), np.array(std), 10))
    # without a mean the uncentred form is fine: it gets as far as the device
    for stats in (good, ColumnStats(None, np.ones(4), 10), ColumnStats(np.full(4, np.nan), [1, 2, 3, 4], 3)):
        with pytest.raises(AssertionError, match="device call"):
            dd.standardized(stats=stats)
    with pytest.raises(AssertionError, match="device call"):
        dd.standardized(center=True, stats=good)
    with pytest.raises(AssertionError, match="device call"):              # own statistics: the device computes them
        dd.standardized()
    dd.close()
    with pytest.raises(RuntimeError, match="closed"):
        dd.standardized(stats=good)
    with pytest.raises(RuntimeError, match="closed"):
        dd.standardized()
    with pytest.raises(RuntimeError, match="closed"):
        dd.column_stats()
    with pytest.raises(ValueError):                                         # the statistics are still checked first
        dd.standardized(stats=ColumnStats(None, np.zeros(4), 10))


def test_unscale_arithmetic_and_identity(no_device):
    rng = np.random.RandomState(0)
    p = 5
    mean, std = rng.standard_normal(p) * 10.0, rng.uniform(0.1, 3.0, size=p)
    stats = ColumnStats(mean, std, 12)
    plain = _block(12, p)
    assert plain.scaling is None
    for a in (rng.standard_normal((3, p)), rng.standard_normal(p), [[1.0, 2, 3, 4, 5]], "anything"):
        assert plain.unscale(a) is a                                        # not standardised: the identity
    scaled = _block(12, p, ColumnScaling(stats, False))
    centred = _block(12, p, ColumnScaling(stats, True))
    for shape in ((p,), (3, p), (2, 3, p), (0, p)):
        a = rng.standard_normal(shape)
        keep = a.copy()
        assert np.array_equal(scaled.unscale(a), a * std)
        assert np.array_equal(centred.unscale(a), a * std + mean)
        assert np.array_equal(a, keep)                                      # the argument is left alone
        assert centred.unscale(a).shape == shape
    assert np.array_equal(centred.unscale([[1, 2, 3, 4, 5]]), np.array([[1.0, 2, 3, 4, 5]]) * std + mean)
    out = centred.unscale(np.ones((2, p), dtype=np.float32))
    assert out.dtype == np.float64
    for bad in (np.ones((3, p + 1)), np.ones(p - 1), np.float64(2.0)):
        with pytest.raises(ValueError, match="last axis"):
            centred.unscale(bad)
    # x -> (x - m) / s -> unscale: back to within the roundings of the four operations
    x = rng.standard_normal((7, p)) * std + mean
    back = centred.unscale((x - mean) / std)
    assert np.all(np.abs(back - x) <= 4 * 2.0 ** -53 * (np.abs(x - mean) + np.abs(x)))
    assert np.all(np.abs(scaled.unscale(x / std) - x) <= 2 * np.spacing(np.abs(x)))
    # a row block of a standardised block is in the same units
    assert DeviceData(_FakeContext(), (3, p), None, (p,), centred.scaling).scaling is centred.scaling


def test_standardize_keyword_leaves_the_default_alone(no_device):
    import inspect
    spec = inspect.getfullargspec(cdr.weight_and_flatten_on_device)
    assert spec.args == ["values", "weights", "rows", "dtype", "device", "standardize"]
    assert spec.defaults == (None, None, None, None, False)
    with pytest.raises(ValueError):                                         # argument checks come first, as before
        cdr.weight_and_flatten_on_device(np.ones(5), standardize=True)
    with pytest.raises(AssertionError, match="device call"):
        cdr.weight_and_flatten_on_device(np.ones((5, 3)), standardize=True)
    spec = inspect.getfullargspec(DeviceData.standardized)
    assert spec.args == ["self", "center", "stats"] and spec.defaults == (False, None)


def test_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "aa_hip.h")) as fh:
        header = fh.read()
    names = ("aa_data_column_moments", "aa_set_data_rows_affine")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    if not os.path.exists(_backend.library_path()):
        pytest.fail("libaa_hip.so has not been built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_backend.library_path())
    for name in names:
        assert hasattr(lib, name), name
    assert cdr.ColumnStats is preprocessing.ColumnStats and cdr.ColumnScaling is preprocessing.ColumnScaling
    for name in ("ColumnStats", "ColumnScaling", "DeviceData", "weight_and_flatten_on_device"):
        assert name in cdr.__all__
    assert ColumnStats._fields == ("mean", "std", "n_samples")
    assert ColumnScaling._fields == ("stats", "center")
    for method in ("column_stats", "standardized", "unscale"):
        assert callable(getattr(DeviceData, method))
    for method in ("data_column_moments", "set_data_rows_affine"):
        assert callable(getattr(_backend.Context, method))
