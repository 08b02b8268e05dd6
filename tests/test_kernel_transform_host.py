"""KernelAA.transform, host side (no GPU needed): an unfitted model, a data width that does not match
the fitted form and a missing or short ``diagonal`` are refused before any device call."""
import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


def _pretend_fitted(form, n=12, p=3, k=2):
    """A KernelAA with the host state a fit of ``form`` leaves behind (the fit itself needs a GPU)."""
    m = cdr.KernelAA(k, random_state=0)
    m.dictionary = np.full((k, n), 1.0 / n)
    m.alpha = np.ones(k)
    state = dict(form=form, n_samples=n, A=np.eye(k))
    if form != "kernel":
        state["n_features"] = p
    m._transform_state = state
    return m


def test_transform_of_an_unfitted_model_is_refused_before_any_device_call(no_device):
    m = cdr.KernelAA(3, random_state=0)
    with pytest.raises(ValueError, match="not fitted"):
        m.transform(np.ones((4, 5)), diagonal=np.ones(4))
    with pytest.raises(ValueError, match="not fitted"):
        m.transform(np.ones((4, 5)))
    assert m.weights is None


def test_transform_arguments_are_checked_before_any_device_call(no_device):
    rs_before = _pretend_fitted("kernel").random_state.get_state()[1].copy()
    m = _pretend_fitted("kernel")
    with pytest.raises(ValueError, match="12"):
        m.transform(np.ones((4, 11)), diagonal=np.ones(4))          # one column per training sample
    with pytest.raises(ValueError, match="diagonal"):
        m.transform(np.ones((4, 12)))
    with pytest.raises(ValueError, match="diagonal"):
        m.transform(np.ones((4, 12)), diagonal=np.ones(3))
    with pytest.raises(ValueError):
        m.transform(np.ones(12), diagonal=np.ones(1))
    assert np.array_equal(m.random_state.get_state()[1], rs_before)   # no draws were taken
    for form in ("linear", "rbf"):
        m = _pretend_fitted(form)
        with pytest.raises(ValueError, match="3"):
            m.transform(np.ones((4, 12)))                             # n_features, not n_samples
        with pytest.raises(ValueError, match="diagonal"):
            m.transform(np.ones((4, 3)), diagonal=np.ones(4))         # implied by the features
        with pytest.raises(ValueError):
            m.transform(np.ones((0, 3)))
