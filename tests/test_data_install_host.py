"""What `_backend.Context` records about an install (`Context._adopt`), without a device: the setters run
against a stand-in library whose entry points succeed.  After any two installs in a row the binding's view of
the context is what the second one alone leaves on a fresh object."""
import itertools

import numpy as np
import pytest

from convex_dim_red import _backend

P_VALID = 3            # columns the stand-in aa_set_data_weighted reports as kept


class _Lib(object):
    """Every entry point returns AA_OK; aa_set_data_weighted also fills *p_valid."""

    def __getattr__(self, name):
        def call(*args):
            if name == "aa_set_data_weighted":
                args[-1]._obj.value = P_VALID
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(_backend, "require_gpu", lambda: None)
    monkeypatch.setattr(_backend, "load_library", lambda: _Lib())


def _context():
    return _backend.Context(dtype="float64", device=0)


def _owner(n, p, row_lo=0, n_global=None):
    o = _context()
    o.set_data(np.zeros((n, p)), n_global=n_global, row_offset=row_lo)
    return o


# name -> (setter, what it leaves: n, p, row_lo, n_global, implicit, and whether it keeps an owner)
def _setters():
    shard = _owner(11, 4, row_lo=5, n_global=40)       # share_data takes the owner's shard over
    whole = _owner(9, 6)
    return {
        "set_data": (lambda c: c.set_data(np.zeros((7, 2)), n_global=30, row_offset=4), (7, 2, 4, 30, False, False)),
        "share_data": (lambda c: c.share_data(shard), (11, 4, 5, 40, False, True)),
        "set_data_rows": (lambda c: c.set_data_rows(whole, 2, 5), (5, 6, 0, 5, False, False)),
        "set_data_rows_affine": (lambda c: c.set_data_rows_affine(whole, 1, 4, scale=np.ones(6)),
                                 (4, 6, 0, 4, False, False)),
        "set_data_take": (lambda c: c.set_data_take(whole, [8, 0, 0]), (3, 6, 0, 3, False, False)),
        "set_data_weighted": (lambda c: c.set_data_weighted(np.zeros((12, 5)), row0=2, n=8),
                              (8, P_VALID, 0, 8, False, False)),
        "set_rbf_features": (lambda c: c.set_rbf_features(np.zeros((10, 3)), 0.5), (10, 10, 0, 10, True, False)),
        "set_poly_features": (lambda c: c.set_poly_features(np.zeros((13, 3)), 0.5, 1.0, 2), (13, 13, 0, 13, True, False)),
        "set_rbf_features_resident": (lambda c: c.set_rbf_features_resident(whole, 0.5), (9, 9, 0, 9, True, False)),
        "set_poly_features_resident": (lambda c: c.set_poly_features_resident(whole, 0.5, 1.0, 2),
                                       (9, 9, 0, 9, True, False)),
    }


def _view(c):
    return (c.n, c.p, c.row_lo, c.n_global, c.implicit, c._data_owner is not None)


def test_every_setter_alone(stub):
    for name, (install, want) in _setters().items():
        c = _context()
        assert _view(c) == (0, 0, 0, 0, False, False)
        install(c)
        assert _view(c) == want, name
        assert all(type(v) is int for v in _view(c)[:4]), name


def test_the_second_install_decides(stub):
    setters = _setters()
    for first, second in itertools.product(setters, repeat=2):
        c, fresh = _context(), _context()
        setters[first][0](c)
        setters[second][0](c)
        setters[second][0](fresh)
        assert _view(c) == _view(fresh) == setters[second][1], (first, second)


def test_context_has_no_form(stub):
    c = _context()
    for install, _ in _setters().values():
        install(c)
        assert not hasattr(c, "form")
