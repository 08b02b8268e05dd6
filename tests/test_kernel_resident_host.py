"""KernelAA on resident data, host side (no GPU needed): every refusal of ``DeviceData.take``,
``KernelAA.kernel_scores`` / ``transform`` and ``time_series_cross_validate`` happens with the device patched
out and without a draw from ``random_state``; ``KernelAA.score`` still refuses models without a data-space
residual; the four new entry points are declared, exported and bound; the arithmetic of ``KernelScores``."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from sklearn.exceptions import NotFittedError

import convex_dim_red as cdr
from convex_dim_red import _backend, validation
from convex_dim_red.preprocessing import DeviceData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aa_set_data_take", "aa_set_rbf_features_resident", "aa_set_poly_features_resident",
               "aa_kernel_sample_residuals")


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


class _Handle(object):
    """Stands in for an open context behind a DeviceData."""
    h = 1
    device = 0

    def __init__(self, code=_backend.AA_F64):
        self.dtype_code = code

    def close(self):
        self.h = 0


def _resident(shape=(10, 4), code=_backend.AA_F64):
    return DeviceData(_Handle(code), shape, None, shape[1:])


def _same_state(rs, ref):
    a, b = rs.get_state(), ref.get_state()
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _model(form, k=2, n=6, p=4, seed=3):
    """A KernelAA that looks fitted in ``form`` (host arrays only: nothing here reaches the device)."""
    rs = np.random.RandomState(seed)
    model = cdr.KernelAA(k, random_state=rs)
    model.dictionary = np.full((k, n), 1.0 / n)
    model.alpha = np.ones(k)
    model.weights = np.full((n, k), 1.0 / k)
    state = dict(form=form, n_samples=n, A=np.eye(k))
    if form != "kernel":
        state.update(n_features=p)
    if form == "linear":
        state.update(archetypes=np.ones((k, p)))
    if form in ("rbf", "poly"):
        state.update(gamma=0.5, support=np.arange(n), support_rows=np.ones((n, p)),
                     support_dictionary=model.dictionary.copy())
    if form == "poly":
        state.update(coef0=1.0, degree=2)
    model._transform_state = state
    return model, rs


def test_take_refuses_on_the_host(no_device):
    dd = _resident()
    for bad in ([], np.zeros((2, 2), dtype=int), [0.0, 1.0], [True, False], np.array([True] * 10), [0, 10], [-11],
                ["a"], 3, [[1, 2]], np.array([], dtype=np.int64)):
        with pytest.raises(ValueError):
            dd.take(bad)
    with pytest.raises(ValueError, match="narrowed"):
        dd.take([0, 1], dtype=np.float32)
    with pytest.raises(ValueError):
        dd.take([0, 1], dtype=np.int32)
    with pytest.raises(ValueError, match="index 10 .position 2."):
        dd.take([9, -10, 10, 11])
    for good in ([0, 9, -1, -10, 3, 3], np.array([5], dtype=np.uint8), (1, 2)):
        with pytest.raises(AssertionError, match="device call"):    # a good set gets as far as the device
            dd.take(good)
    with pytest.raises(AssertionError, match="device call"):
        _resident(code=_backend.AA_F32).take([1], dtype=np.float64)
    with pytest.raises(AssertionError, match="device call"):
        _resident(code=_backend.AA_F32).take([1], dtype="float32")
    dd.close()
    with pytest.raises(RuntimeError, match="closed"):
        dd.take([1])
    with pytest.raises(ValueError):                                   # the indices are still checked first
        dd.take([10])
    spec = inspect.getfullargspec(DeviceData.take)
    assert spec.args == ["self", "indices", "dtype"] and spec.defaults == (None,)


@pytest.mark.parametrize("method", ["transform", "kernel_scores"])
def test_kernel_methods_refuse_before_any_device_call_or_draw(no_device, method):
    unfitted = cdr.KernelAA(2, random_state=0)
    with pytest.raises(NotFittedError):
        getattr(unfitted, method)(np.ones((3, 4)))
    for form in ("kernel", "linear", "rbf", "poly"):
        model, rs = _model(form)
        ref = np.random.RandomState(3)
        call = getattr(model, method)
        width = 6 if form == "kernel" else 4
        kw = dict(diagonal=np.ones(5)) if form == "kernel" else {}
        for bad in (np.ones((5, width + 1)), np.ones(width), np.ones((0, width))):
            with pytest.raises(ValueError, match="KernelAA.%s: expected" % method):
                call(bad, **kw)
        with pytest.raises(ValueError, match="expected"):
            call(_resident((5, width + 1)), **kw) if form != "kernel" else call(np.ones((5, width + 2)), **kw)
        if form == "kernel":
            with pytest.raises(TypeError, match="host array, not DeviceData"):
                call(_resident((5, 6)), diagonal=np.ones(5))
            with pytest.raises(ValueError, match="`diagonal` .* is required"):
                call(np.ones((5, 6)))
            with pytest.raises(ValueError, match="must hold 5 values"):
                call(np.ones((5, 6)), diagonal=np.ones(4))
        else:
            with pytest.raises(ValueError, match="`diagonal` is only taken"):
                call(np.ones((5, 4)), diagonal=np.ones(5))
            with pytest.raises(ValueError, match="`diagonal` is only taken"):
                call(_resident((5, 4)), diagonal=np.ones(5))
        if method == "kernel_scores":
            for bad in (np.ones((5, 3)), np.ones((4, 2)), np.ones(5)):
                with pytest.raises(ValueError, match="`weights` must be"):
                    call(np.ones((5, width)), weights=bad, **kw)
            with pytest.raises(ValueError, match="`weights` must be"):   # the model's own belong to 6 rows
                call(np.ones((5, width)), **kw)
            model.weights = None
            with pytest.raises(ValueError, match="holds no weights"):
                call(np.ones((5, width)), **kw)
        assert _same_state(rs, ref), (method, form)


def test_score_still_refuses_models_without_a_data_space_residual(no_device):
    for form, what in (("kernel", "an explicit kernel matrix"), ("rbf", "the RBF kernel"),
                       ("poly", "the polynomial kernel")):
        model, _ = _model(form)
        with pytest.raises(ValueError, match="has no data-space residual"):
            model.score(np.ones((6, 4)))
        with pytest.raises(ValueError, match=what):
            model.score(_resident((6, 4)))


def test_cross_validation_refuses_an_explicit_kernel_model_before_the_upload(no_device):
    rs, ref = np.random.RandomState(5), np.random.RandomState(5)
    made = []

    def make():
        made.append(cdr.KernelAA(3, random_state=rs))
        return made[-1]
    X = np.ones((40, 3))
    for fit_kwargs in (None, {}, dict(kernel="rbf"), dict(features=False, kernel="poly")):
        with pytest.raises(ValueError, match="explicit kernel matrix has no row blocks"):
            cdr.time_series_cross_validate(make, X, n_folds=3, fit_kwargs=fit_kwargs)
    assert len(made) == 4 and _same_state(rs, ref)
    with pytest.raises(AssertionError, match="device call"):        # a feature model gets as far as the upload
        cdr.time_series_cross_validate(make, X, n_folds=3, fit_kwargs=dict(features=True, kernel="rbf"))
    with pytest.raises(AssertionError, match="device call"):
        cdr.time_series_cross_validate(lambda: cdr.ArchetypalAnalysis(3, random_state=rs), X, n_folds=3)
    assert _same_state(rs, ref)
    spec = inspect.getfullargspec(cdr.time_series_cross_validate)
    assert spec.args == ["make_model", "data", "n_folds", "n_init", "dtype", "fit_kwargs"]
    assert spec.defaults == (10, 1, None, None)


def test_new_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "aa_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(aa_ctx \*ctx" % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    for i, kind in enumerate(("GIVEN", "ONES", "POLY", "LINEAR")):
        assert re.search(r"^#define AA_DIAG_%s\s+%d$" % (kind, i), header, re.M), kind
        assert _backend.DIAG_KINDS[i] == kind.lower()
    if not os.path.exists(_backend.library_path()):
        pytest.fail("libaa_hip.so has not been built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_backend.library_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("set_data_take", "set_rbf_features_resident", "set_poly_features_resident",
                 "kernel_sample_residuals"):
        assert callable(getattr(_backend.Context, name)), name
    assert cdr.KernelScores is validation.KernelScores and "KernelScores" in cdr.__all__
    assert cdr.KernelScores._fields == ("cost", "rmse", "explained", "sample_sse", "diagonal")


def test_kernel_scores_arithmetic():
    r = np.array([0.25, 0.0, 1.5, 0.75])
    d = np.array([1.0, 2.0, 3.0, 4.0])
    s = validation._kernel_scores_from_sums(r, d, r.sum(), d.sum())
    assert isinstance(s, cdr.KernelScores)
    assert s.cost == 0.5 * 2.5 / 4 and s.rmse == np.sqrt(2.5 / 4) and s.explained == 1.0 - 2.5 / 10.0
    assert np.array_equal(s.sample_sse, r) and np.array_equal(s.diagonal, d)
    # a perfect reconstruction whose residuals come out slightly negative: nothing is clamped but the root
    r = np.array([-3e-17, 1e-17, -2e-17])
    s = validation._kernel_scores_from_sums(r, np.ones(3), r.sum(), 3.0)
    assert s.cost == 0.5 * r.sum() / 3 and s.cost < 0
    assert s.rmse == 0.0
    assert s.explained == 1.0 - r.sum() / 3.0 and s.explained >= 1.0
    assert np.array_equal(s.sample_sse, r) and s.sample_sse.min() < 0
    # the sums are taken as given (the device's fixed-order sums), not recomputed from the vectors
    s = validation._kernel_scores_from_sums(np.array([1.0, 2.0]), np.array([4.0, 4.0]), 3.5, 8.5)
    assert s.cost == 0.5 * 3.5 / 2 and s.explained == 1.0 - 3.5 / 8.5
