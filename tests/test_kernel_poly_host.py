"""KernelAA on the implicit polynomial kernel, host side (no GPU needed): every refusal is raised before any
device call, the defaults are scikit-learn's (degree 3, gamma = 1 / n_features, coef0 1), the state a fit
leaves behind is deep-copyable, and the three entry points are declared in the header and bound."""
import copy
import os
import re

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend
from convex_dim_red import archetypal_analysis as aa

NEW_SYMBOLS = ("aa_set_poly_features", "aa_set_poly_reference", "aa_poly_cross")


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


class _FakeContext(object):
    """Stands in for _backend.Context in a fit: records how the kernel was set."""
    calls = []

    def __init__(self, dtype=None):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_kernel_features(self, spec, X):
        assert spec["form"] == "poly"
        type(self).calls.append((X.shape, spec["gamma"], spec["coef0"], spec["degree"]))

    def grams(self):
        k = 2
        return np.eye(k), 2.0 * np.eye(k), np.eye(k), 1.0


@pytest.fixture
def stub_device(monkeypatch):
    """The device loop replaced by one that returns its starting factors: the host flow of a fit runs."""
    def iterate(ctx, label, weights, dictionary, alpha, *args, **kwargs):
        return weights, dictionary, alpha, 1.0, 1, 0.0, [-1.0]
    _FakeContext.calls = []
    monkeypatch.setattr(_backend, "Context", _FakeContext)
    monkeypatch.setattr(aa, "_iterate_on_device", iterate)
    return _FakeContext


X = np.linspace(-1.0, 1.0, 60).reshape(12, 5)


@pytest.mark.parametrize("kwargs,match", [
    (dict(kernel="poly"), "features=True"),                                   # needs the features
    (dict(kernel="poly", features=True, degree=2.5), "degree"),
    (dict(kernel="poly", features=True, degree=2.0), "degree"),               # an integer type, not a whole float
    (dict(kernel="poly", features=True, degree=0), "degree"),
    (dict(kernel="poly", features=True, degree=-3), "degree"),
    (dict(kernel="poly", features=True, degree=True), "degree"),
    (dict(kernel="poly", features=True, gamma=0.0), "gamma"),
    (dict(kernel="poly", features=True, gamma=-1.0), "gamma"),
    (dict(kernel="poly", features=True, gamma=float("nan")), "gamma"),
    (dict(kernel="poly", features=True, coef0=-0.5), "coef0"),
    (dict(kernel="poly", features=True, coef0=float("inf")), "coef0"),
    (dict(kernel="rbf", features=True, degree=2), "degree"),                  # belong to the polynomial kernel
    (dict(kernel="rbf", features=True, coef0=1.0), "coef0"),
    (dict(features=True, degree=2), "degree"),
    (dict(features=True, coef0=0.0), "coef0"),
    (dict(degree=3), "degree"),
    (dict(kernel="sigmoid", features=True), "kernel"),
])
def test_refusals_are_raised_before_any_device_call(no_device, kwargs, match):
    data = X if kwargs.get("features") else X.dot(X.T)
    model = cdr.KernelAA(2, random_state=0)
    with pytest.raises(ValueError, match=match):
        model.fit_transform(data, **kwargs)
    assert getattr(model, "_transform_state", None) is None


def test_defaults_are_scikit_learns(stub_device):
    model = cdr.KernelAA(2, random_state=0, init="random")
    model.fit_transform(X, features=True, kernel="poly")
    assert stub_device.calls == [((12, 5), 1.0 / 5, 1.0, 3)]
    state = model._transform_state
    assert state["form"] == "poly" and state["gamma"] == 0.2 and state["coef0"] == 1.0 and state["degree"] == 3
    assert isinstance(state["degree"], int)
    model.fit_transform(X, features=True, kernel="poly", degree=np.int64(2), gamma=0.5, coef0=0)
    assert stub_device.calls[-1] == ((12, 5), 0.5, 0.0, 2)


def test_fitted_state_is_deep_copyable(stub_device):
    model = cdr.KernelAA(2, random_state=0, init="random")
    model.fit_transform(X, features=True, kernel="poly", degree=2)
    state = model._transform_state
    D = model.alpha[:, None] * model.dictionary
    assert np.array_equal(state["support_rows"], X[state["support"]])
    assert np.array_equal(state["support_dictionary"], D[:, state["support"]])
    assert np.array_equal(state["A"], 2.0 * np.eye(2))
    twin = copy.deepcopy(model)
    assert sorted(twin._transform_state) == sorted(state)
    for key, value in state.items():
        assert np.array_equal(np.asarray(twin._transform_state[key]), np.asarray(value)), key
        if isinstance(value, np.ndarray):
            assert twin._transform_state[key] is not value
    with pytest.raises(ValueError, match="polynomial"):
        twin.score(X)
    with pytest.raises(ValueError, match="diagonal"):                  # follows from the features
        twin.transform(X[:4], diagonal=np.ones(4))
    with pytest.raises(ValueError, match="5"):
        twin.transform(np.ones((4, 6)))


def test_kernel_values_multiply_in_a_fixed_order():
    s = np.array([-0.75, 0.0, 0.3, 1.0])
    b = 0.5 * s + 1.0
    assert np.array_equal(aa._poly_kernel_values(s, 0.5, 1.0, 1), b)
    assert np.array_equal(aa._poly_kernel_values(s, 0.5, 1.0, 3), (b * b) * b)


def test_new_symbols_are_declared_and_bound():
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "aa_hip.h")
    with open(header) as fh:
        text = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(aa_ctx \*ctx" % name, text, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS, name
