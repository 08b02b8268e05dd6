"""The implicit kernels' descriptor (csrc/aa_internal.h: KernelSpec) as the ABI shows it, for both kinds: a
context names a kernel -- Ctx::kernel for the fit, Ctx::cross for a transform's reference set -- only through a
call that succeeded, and a refused call leaves what it named before fully usable.

n = 70 rows of p = 5 features, k = 3, s = 65 reference rows (one full column tile plus one row).  Every
comparison is bit for bit between two runs of the same device code; no tolerance is involved."""
import numpy as np
import pytest

from convex_dim_red import _backend

pytestmark = pytest.mark.gpu

N, P, K, S = 70, 5, 3, 65
ARG, STATE = -1, -3
KINDS = ("rbf", "poly")
PARAMS = {"rbf": (0.3,), "poly": (0.3, 1.0, 2)}
# parameters kernel_spec_check turns down, with the words it uses
BAD = {"rbf": [(0.0,)], "poly": [(0.0, 1.0, 2), (0.3, 1.0, 0), (0.3, -0.5, 2)]}
WORDS = {"rbf": "gamma must be positive", "poly": "the polynomial kernel needs gamma > 0, coef0 >= 0 and degree >= 1"}

rng = np.random.RandomState(2024)
X = rng.standard_normal((N, P))
XS = rng.standard_normal((S, P))
V = rng.uniform(size=(S, K))
C0 = rng.uniform(size=(K, N))
C0 /= C0.sum(axis=1, keepdims=True)
Z0 = rng.uniform(size=(N, K))
Z0 /= Z0.sum(axis=1, keepdims=True)


def _error(lib):
    return lib.aa_last_error().decode()


def _features(lib, ctx, kind, params, owner=None):
    """The kind's features entry point, host or resident form, called through the library: its return code."""
    if owner is None:
        return getattr(lib, "aa_set_%s_features" % kind)(ctx.h, _backend._ptr(X), N, P, P, *params)
    return getattr(lib, "aa_set_%s_features_resident" % kind)(ctx.h, owner.h, *params)


def _reference(lib, ctx, kind, params):
    return getattr(lib, "aa_set_%s_reference" % kind)(ctx.h, K, _backend._ptr(XS), S, P, P, _backend._ptr(V), K, *params)


def _set(ctx, kind, what, *args):
    getattr(ctx, "set_%s_%s" % (kind, what))(*(args + PARAMS[kind]))


def _grams(ctx):
    ctx.set_state(C0, Z0, np.ones(K))              # K Z and C K are computed again, from what the context names
    ctx.prepare()
    return ctx.grams()                             # Z'Z, C K C', C K Z, tr K


def _same(a, b):
    return all(np.array_equal(x, y) and np.all(np.isfinite(x)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_kind_cross_is_refused(kind):
    other = KINDS[1 - KINDS.index(kind)]
    lib = _backend.load_library()
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(X)
        _set(ctx, kind, "reference", XS, V)
        before = getattr(ctx, "%s_cross" % kind)(fetch=True)
        assert getattr(lib, "aa_%s_cross" % other)(ctx.h, None) == STATE
        assert "aa_set_%s_reference first" % other in _error(lib)
        after = getattr(ctx, "%s_cross" % kind)(fetch=True)
        assert ctx.kernel_cross(fetch=True).tobytes() == after.tobytes()
    assert np.all(np.isfinite(before)) and np.any(before != 0) and np.array_equal(before, after)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_features_install_leaves_the_kernel_usable(kind):
    lib = _backend.load_library()
    with _backend.Context(dtype="float64") as ctx, _backend.Context(dtype="float64") as owner:
        owner.set_data(X)
        _set(ctx, kind, "features", X)
        before = _grams(ctx)
        for asked in KINDS:
            for params in BAD[asked]:
                for own in (None, owner):
                    assert _features(lib, ctx, asked, params, own) == ARG, (asked, params)
                    assert WORDS[asked] in _error(lib)
        assert (ctx.n, ctx.p) == (N, N)
        assert _same(before, _grams(ctx))
        assert _features(lib, ctx, kind, PARAMS[kind]) == 0             # the good call goes through, same bits
        assert _same(before, _grams(ctx))


@pytest.mark.parametrize("kind", KINDS)
def test_refused_reference_set_leaves_the_reference_usable(kind):
    lib = _backend.load_library()
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(X)
        _set(ctx, kind, "reference", XS, V)
        before = ctx.kernel_cross(fetch=True)
        for asked in KINDS:
            for params in BAD[asked]:
                assert _reference(lib, ctx, asked, params) == ARG, (asked, params)
                assert WORDS[asked] in _error(lib)
        after = ctx.kernel_cross(fetch=True)
    assert np.all(np.isfinite(before)) and np.array_equal(before, after)


@pytest.mark.parametrize("kind", KINDS)
def test_float32_context_is_refused_by_the_library(kind):
    lib = _backend.load_library()
    kept = X.astype(np.float32)
    with _backend.Context(dtype="float32") as ctx, _backend.Context(dtype="float64") as owner:
        owner.set_data(X)
        ctx.set_data(kept)
        for own in (None, owner):
            assert _features(lib, ctx, kind, PARAMS[kind], own) == STATE
            assert "float64 context" in _error(lib)
            assert (ctx.n, ctx.p) == (N, P) and np.array_equal(ctx.get_data(), kept.astype(np.float64))


@pytest.mark.parametrize("kind", KINDS)
def test_time_kernel_runs_the_products_of_either_kind(kind):
    with _backend.Context(dtype="float64") as fit, _backend.Context(dtype="float64") as new:
        _set(fit, kind, "features", X)
        fit.set_state(C0, Z0, np.ones(K))
        assert fit.time_kernel(8, 1) >= 0.0
        new.set_data(X)
        with pytest.raises(RuntimeError, match="error -3: aa_time_kernel 9"):    # no reference set yet
            new.time_kernel(9, 1)
        _set(new, kind, "reference", XS, V)
        assert new.time_kernel(9, 1) >= 0.0
        assert np.array_equal(new.kernel_cross(fetch=True), getattr(new, "%s_cross" % kind)(fetch=True))
