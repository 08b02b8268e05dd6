"""Installing data (include/aa_hip.h, "installing data"): what a context is after one of the ten entry points
that give it a matrix (six store one, four set up an implicit kernel) depends on that call alone.

* History: for every ordered pair (first, second) of installers, a context that ran first -- and a short fit on
  it, so that factors, scratch and the QP's records of the first matrix exist -- and then second cannot be told
  from a fresh context that ran second alone: same sizes, same stored bits (or the same refusal to hand out a
  matrix that an implicit kernel never stores), same trace bits, and the same bits after two outer iterations
  from one fixed start.  The two matrices differ in both sizes (130 x 129, two rows and one column past the
  128-element pads, and 61 x 5), installed in either order, so that a size kept from the first install shows.
* Refusals: a call that the shared owner check turns down returns the code its entry point has always returned,
  names the entry point, and leaves the target's matrix as it was.
* The QP's pass counts and sample order belong to the rows they were recorded for.

Everything is compared bit for bit between two runs of the same device code; no tolerance is involved."""
import warnings

import numpy as np
import pytest

from convex_dim_red import _backend

pytestmark = pytest.mark.gpu

K = 3
SHAPES = {"large": (130, 129), "small": (61, 5)}
SPG_KW = dict(max_iterations=3)
QP_KW = dict(max_iterations=40)
GAMMA, COEF0, DEGREE = 0.01, 1.0, 2
STORED = ("set_data", "share_data", "set_data_rows", "set_data_rows_affine", "set_data_take", "set_data_weighted")
FEATURES = ("set_rbf_features", "set_rbf_features_resident", "set_poly_features", "set_poly_features_resident")
INSTALLERS = {"float64": STORED + FEATURES, "float32": STORED}         # the feature installers are float64-only


class _Inputs(object):
    """The arguments of every installer for one shape and dtype; the owners are contexts of their own."""

    def __init__(self, dtype, n, p):
        rng = np.random.RandomState(1000 * n + p)
        self.n, self.p = n, p
        self.M = rng.uniform(0.5, 1.5, size=(n, p))
        self.tall = rng.uniform(0.5, 1.5, size=(n + 7, p))             # rows / rows_affine / take read from it
        self.shift, self.scale = rng.uniform(-1.0, 1.0, size=p), rng.uniform(0.5, 2.0, size=p)
        self.idx = rng.randint(0, n + 7, size=n)                        # any order, duplicates
        self.raw = rng.uniform(0.5, 1.5, size=(n + 4, p + 2))           # two columns drop out
        self.raw[1, 0] = self.raw[n + 3, p // 2 + 1] = np.nan
        self.weights = rng.uniform(0.5, 1.0, size=p + 2)
        self.exact, self.rows = _backend.Context(dtype=dtype), _backend.Context(dtype=dtype)
        self.exact.set_data(self.M)
        self.rows.set_data(self.tall)

    def close(self):
        self.exact.close()
        self.rows.close()

    def install(self, ctx, name):
        if name == "set_data":
            ctx.set_data(self.M)
        elif name == "share_data":
            ctx.share_data(self.exact)
        elif name == "set_data_rows":
            ctx.set_data_rows(self.rows, 3, self.n)
        elif name == "set_data_rows_affine":
            ctx.set_data_rows_affine(self.rows, 4, self.n, self.shift, self.scale)
        elif name == "set_data_take":
            ctx.set_data_take(self.rows, self.idx)
        elif name == "set_data_weighted":
            assert ctx.set_data_weighted(self.raw, self.weights, row0=2, n=self.n).sum() == self.p
        elif name == "set_rbf_features":
            ctx.set_rbf_features(self.M, GAMMA)
        elif name == "set_rbf_features_resident":
            ctx.set_rbf_features_resident(self.exact, GAMMA)
        elif name == "set_poly_features":
            ctx.set_poly_features(self.M, GAMMA, COEF0, DEGREE)
        elif name == "set_poly_features_resident":
            ctx.set_poly_features_resident(self.exact, GAMMA, COEF0, DEGREE)
        else:
            raise KeyError(name)


@pytest.fixture(scope="module")
def inputs():
    made = {}

    def get(dtype, shape):
        if (dtype, shape) not in made:
            made[dtype, shape] = _Inputs(dtype, *SHAPES[shape])
        return made[dtype, shape]
    yield get
    for item in made.values():
        item.close()


def _fit(ctx, k, n_outer):
    """`n_outer` outer iterations from a start that depends on (n, k) only."""
    rng = np.random.RandomState(7 * ctx.n + k)
    C0 = rng.uniform(size=(k, ctx.n))
    Z0 = rng.uniform(size=(ctx.n, k))
    ctx.set_state(C0 / C0.sum(axis=1, keepdims=True), Z0 / Z0.sum(axis=1, keepdims=True), np.ones(k))
    cost0 = ctx.prepare()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, st = ctx.iterate(cost0, n_outer, 0.0, "abs_delta_f", False, True, True, SPG_KW, QP_KW, check_every=1)
    assert not st.error_stage and st.n_iter == n_outer - 1
    C, Z, _ = ctx.get_state()
    return cost0, costs, C, Z


def _observe(ctx, stored):
    """Everything the ABI shows of a context after an install."""
    seen = {"shape": (ctx.n, ctx.p)}
    if stored:
        seen["data"] = ctx.get_data()
    else:
        with pytest.raises(RuntimeError, match="error -3:"):             # nothing stands in for an implicit kernel
            ctx.get_data()
    seen["trace"] = np.float64(ctx.data_trace())
    seen["cost0"], seen["costs"], seen["C"], seen["Z"] = _fit(ctx, K, 2)
    return seen


def _differences(a, b):
    out = [] if a["shape"] == b["shape"] else ["shape %r != %r" % (a["shape"], b["shape"])]
    for key in sorted(set(a) - {"shape"}):
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape or not np.array_equal(x, y) or np.isnan(x).any():
            out.append(key)
    return out


@pytest.mark.parametrize("direction", ["grow", "shrink"])
@pytest.mark.parametrize("dtype,second", [(d, s) for d in ("float64", "float32") for s in INSTALLERS[d]])
def test_history_does_not_matter(inputs, dtype, second, direction):
    before, after = ("small", "large") if direction == "grow" else ("large", "small")
    old, new = inputs(dtype, before), inputs(dtype, after)
    stored = second in STORED
    with _backend.Context(dtype=dtype) as fresh:
        new.install(fresh, second)
        want = _observe(fresh, stored)
    assert want["shape"] == ((new.n, new.p) if stored else (new.n, new.n))
    assert want["trace"] > 0 and np.all(np.isfinite(want["costs"]))
    failed = []
    for first in INSTALLERS[dtype]:
        with _backend.Context(dtype=dtype) as ctx:
            old.install(ctx, first)
            _fit(ctx, K + 1, 1)                    # factors, scratch and QP records of the first matrix
            new.install(ctx, second)
            try:
                diff = _differences(want, _observe(ctx, stored))
            except (RuntimeError, AssertionError, pytest.fail.Exception) as e:
                diff = ["%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")]
        print("%s %s -> %s (%s): %s" % (dtype, first, second, direction, diff or "same"))
        if diff:
            failed.append((first, diff))
    assert not failed, failed


# ------------------------------------------------------------------ refusals
OWNER_TAKING = {
    "aa_share_data": lambda lib, t, o: lib.aa_share_data(t.h, o.h),
    "aa_set_data_rows": lambda lib, t, o: lib.aa_set_data_rows(t.h, o.h, 0, 1),
    "aa_set_data_rows_affine": lambda lib, t, o: lib.aa_set_data_rows_affine(t.h, o.h, 0, 1, None, None),
    "aa_set_data_take": lambda lib, t, o: lib.aa_set_data_take(t.h, o.h, None, 1),
    "aa_set_rbf_features_resident": lambda lib, t, o: lib.aa_set_rbf_features_resident(t.h, o.h, GAMMA),
    "aa_set_poly_features_resident": lambda lib, t, o: lib.aa_set_poly_features_resident(t.h, o.h, GAMMA, COEF0, DEGREE),
}
ARG, STATE = -1, -3


@pytest.mark.parametrize("entry", sorted(OWNER_TAKING))
def test_refused_installs_leave_the_context_as_it_was(entry):
    call = OWNER_TAKING[entry]
    lib = _backend.load_library()
    features = "features" in entry
    rng = np.random.RandomState(3)
    B, A = rng.standard_normal((7, 4)), rng.standard_normal((20, 6))
    G = rng.standard_normal((12, 12))
    G = G.dot(G.T)

    def refused(target, owner, code, kept):
        assert call(lib, target, owner) == code
        assert entry in lib.aa_last_error().decode()
        assert (target.n, target.p) == kept.shape and np.array_equal(target.get_data(), kept)

    with _backend.Context(dtype="float64") as target, _backend.Context(dtype="float64") as owner:
        target.set_data(B)
        refused(target, target, ARG, B)                                  # the same context twice
        refused(target, owner, STATE, B)                                 # an owner without data
        owner.set_data(G, form=_backend.FORM_KERNEL)
        if entry == "aa_share_data":                                     # the one that takes a stored kernel matrix
            with _backend.Context(dtype="float64") as other:
                other.share_data(owner)
                assert np.array_equal(other.get_data(), G)
        else:
            refused(target, owner, STATE, B)                             # a kernel-form owner
        owner.set_rbf_features(A, GAMMA)
        refused(target, owner, STATE, B)                                 # an implicit kernel behind the owner
        owner.set_data(A)
        with _backend.Context(dtype="float32") as single:                # the other dtype: no narrowing, and the
            B32 = B.astype(np.float32)                                   # implicit kernels want a float64 context
            single.set_data(B32)
            refused(single, owner, STATE if features else ARG, B32.astype(np.float64))
        assert call(lib, target, owner) == 0                             # and the good call goes through


# ------------------------------------------------------------------ the QP's records of the previous rows
def test_new_rows_forget_the_qp_records():
    """set_data and a fit, then fewer rows of another matrix and one GPNH weights update: the weights and the
    kernels launched are those of a fresh context."""
    rng = np.random.RandomState(11)
    n, p, m = 130, 5, 61
    A, T = rng.uniform(size=(n, p)), rng.uniform(size=(n, p))
    W, Z0 = rng.uniform(size=(p, K)), np.full((m, K), 1.0 / K)
    with _backend.Context(dtype="float64") as owner, _backend.Context(dtype="float64") as ctx, \
            _backend.Context(dtype="float64") as fresh:
        owner.set_data(T)
        ctx.set_data(A)
        _fit(ctx, K, 2)
        out = []
        for c in (ctx, fresh):
            c.set_data_rows(owner, 9, m)
            c.gpnh_set_factors(K, W, Z0)
            c.gpnh_weights_update(W.T.dot(W), **QP_KW)
            out.append((c.gpnh_get_weights(), c.qp_kernels()))
    assert out[0][1] == out[1][1] and out[0][1]
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_new_rows_forget_the_sample_order(dtype):
    """The four-lane QP kernel leaves the sample order of the NEXT weights update behind, for more than 4096
    samples, and takes it up when the row count matches.  4300 rows of another matrix are not the next update
    of the first: same kernels, same bits as on a fresh context."""
    rng = np.random.RandomState(12)
    n, p = 4300, 5
    A, T = rng.uniform(size=(n, p)), rng.uniform(size=(n + 5, p))
    with _backend.Context(dtype=dtype) as owner, _backend.Context(dtype=dtype) as ctx, \
            _backend.Context(dtype=dtype) as fresh:
        owner.set_data(T)
        ctx.set_data(A)
        ctx.set_state(*_start(n))
        cost0 = ctx.prepare()
        ctx.iterate(cost0, 3, 0.0, "abs_delta_f", False, True, True, SPG_KW, {}, check_every=1)
        out = []
        for c in (ctx, fresh):
            c.set_data_rows(owner, 5, n)
            c.set_state(*_start(n))
            cost0 = c.prepare()
            costs, _ = c.iterate(cost0, 1, 0.0, "abs_delta_f", False, False, True, SPG_KW, {}, check_every=1)
            out.append((c.qp_kernels(), cost0, costs, c.get_state()[1]))
    print("%s: %s | %s" % (dtype, out[0][0], out[1][0]))
    assert out[0][0] == out[1][0] and out[0][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


def _start(n):
    rng = np.random.RandomState(n)
    C0, Z0 = rng.uniform(size=(K, n)), rng.uniform(size=(n, K))
    return C0 / C0.sum(axis=1, keepdims=True), Z0 / Z0.sum(axis=1, keepdims=True), np.ones(K)
