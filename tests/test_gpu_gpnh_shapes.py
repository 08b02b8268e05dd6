"""The GPNH device loop (aa_gpnh_iterate, aa_gpnh_slots_* and the kernels behind them in
csrc/kernels_tall.hip) at every solve size and on every cost path.

The shape table below walks the launchers' dispatch edges: the three instantiations of the
dictionary solve (KM = 16 / 32 / 64), one to three solve blocks (with the guarded and the
zero-filled columns of the last one), both component paddings (KP = 32 / 64), the in-kernel Gram
of the cost kernel with four, two and one thread(s) per output, and the wide-Gram path
(k_gram_wide<32> / <64> + k_gram_finalize) after a dictionary update.  Every row carries what it
is expected to hit as data; `test_table_covers_every_dispatch_value` recomputes that from k and p
with the launchers' rules restated and fails when a value is no longer reached.

Legs
  1  the dictionary solve alone against an extended-precision solve of the same normal equations,
     entry by entry, within a derived first-order error bound (`_solve_reference`);
  2  the cost kernel before and after the update (wide Gram / in-kernel Gram) against the
     extended-precision cost of the factors the device holds;
  3  the whole device path (two outer iterations, lane-per-sample and four-lane / wave-per-sample
     weights QPs) against the oracle;
  4  the pivot test of the Cholesky factorisation: duplicate, rescued and nearly duplicate columns;
  5  restart slots beyond k = 16 through the C ABI, and k = 16 through fit_restarts, bit for bit
     against the single fit.

The host-only tests at the end keep the bound honest without a GPU: a float64 NumPy Cholesky
solve of every system stays within it.  Figures of the MI355X run: profiles/gpnh_shape_errors.txt
(every GPU test prints a `gpnh-shapes` line with its largest error / bound ratio)."""
import warnings

import numpy as np
import pytest

from conftest import oracle_twins
from test_gpu_parity import _trace_noise

LD = np.longdouble
U = LD(2.0) ** -53                       # unit roundoff of float64

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def cdr():
    import convex_dim_red
    from convex_dim_red import _backend
    _backend.require_gpu()
    return convex_dim_red


@pytest.fixture(scope="module")
def orc():
    from oracle import aa_oracle
    return aa_oracle


def _assert_simplex(M, atol=1e-12):
    assert np.all(M >= 0)
    assert np.allclose(M.sum(axis=1), 1, rtol=0, atol=atol)


# ---------------------------------------------------------------- the shape table
# (n, p, k), lambdas, KM of the solve, KP, solve blocks, Gram path of the cost after the update
# ("in4" / "in2" / "in1": inside k_gpnh_cost with that many threads per output; "wide32" / "wide64":
# k_gram_wide<KP> + k_gram_finalize), legs
TABLE = [
    ((64, 128, 1), (0.0, 1.0), 16, 32, 1, "in4", (1, 2, 3)),      # pref = 0, 1 x 1 system; p = p_pad
    ((65, 129, 2), (0.0, 1.0), 16, 32, 1, "in4", (1, 2, 3)),      # ragged p (p_pad 256)
    ((2, 5, 2), (1.0,), 16, 32, 1, "in4", (1, 2, 3)),             # fewer rows than a wave
    ((1, 1, 1), (0.0, 1.0), 16, 32, 1, "in4", (3,)),              # whole-path leg only
    ((1000, 5, 3), (0.0, 1.0), 16, 32, 1, "in4", (1, 2, 3)),      # p_pad almost all padding
    ((130, 127, 5), (0.0, 1.0), 16, 32, 1, "in4", (1, 2, 3)),     # data in the last of the four column spans
    ((200, 90, 8), (0.0, 1.0), 16, 32, 1, "in4", (1, 2, 3)),      # parts 4 -> 2 edge (k^2 = 64)
    ((200, 90, 9), (0.0, 1.0), 16, 32, 1, "in2", (1, 2, 3)),      #                   (k^2 = 81)
    ((200, 90, 11), (0.0, 1.0), 16, 32, 1, "in2", (1, 2, 3)),     # parts 2 -> 1 edge (121)
    ((400, 200, 12), (0.0, 1.0), 16, 32, 1, "in1", (1, 2, 3)),    #                   (144)
    ((333, 256, 16), (0.0, 1.0), 16, 32, 1, "in1", (1, 2, 3)),    # k^2 = 256, k p_pad = 4096 exactly
    ((333, 257, 16), (0.0, 1.0), 16, 32, 2, "wide32", (1, 2, 3)),   # p_pad 384: second block half empty
    ((500, 513, 10), (0.0, 1.0), 16, 32, 3, "wide32", (1, 2, 3)),   # k p_pad > 4096 at small k
    ((150, 300, 17), (0.0, 1.0), 32, 32, 2, "wide32", (1, 2, 3)),   # KM = 32 lower edge
    ((300, 260, 32), (0.0, 1.0), 32, 32, 2, "wide32", (1, 2, 3)),   # KM = 32 / KP = 32 upper edge
    ((200, 40, 33), (0.0, 1.0), 64, 64, 1, "wide64", (1, 2, 3)),    # KM = KP = 64 lower edge; p < k
    ((300, 700, 64), (0.0, 1.0), 64, 64, 3, "wide64", (1, 2, 3)),   # k = 64; six 128-column chunks
]
F32_SOLVE_SHAPES = [(333, 257, 16), (150, 300, 17), (300, 700, 64)]


def _sid(shape):
    return "n%d_p%d_k%d" % shape


def _cases(leg):
    return [pytest.param(row[0], lam, id="%s_lam%g" % (_sid(row[0]), lam))
            for row in TABLE if leg in row[6] for lam in row[1]]


def _p_pad(p):
    return 128 * ((p + 127) // 128)


def _dispatch(p, k):
    """The launchers' rules restated (launch_gpnh_solve, ensure_problem, gpnh_cost_can_gram,
    gpnh_cost_body)."""
    pp = _p_pad(p)
    km = 16 if k <= 16 else (32 if k <= 32 else 64)
    kp = 32 if k <= 32 else 64
    blocks = (pp + 255) // 256
    if k * k <= 256 and k * pp <= 4096:
        parts = 4 if 256 // (k * k) >= 4 else (2 if 256 // (k * k) >= 2 else 1)
        gram = "in%d" % parts
    else:
        gram = "wide%d" % kp
    return km, kp, blocks, gram


# ---------------------------------------------------------------- problems
_PROBLEMS = {}


def _problem(shape):
    """X = Zt W0' + 0.1 noise with right-stochastic weights, a Gaussian start dictionary and
    right-stochastic start weights, as the other GPNH tests draw them."""
    if shape not in _PROBLEMS:
        n, p, k = shape
        rng = np.random.RandomState(1000 + n + p + k)
        W0 = rng.standard_normal((p, k))
        Zt = rng.uniform(size=(n, k))
        Zt /= Zt.sum(axis=1, keepdims=True)
        X = Zt.dot(W0.T) + 0.1 * rng.standard_normal((n, p))
        Wi = 0.5 * rng.standard_normal((p, k))
        Zi = rng.uniform(size=(n, k))
        Zi /= Zi.sum(axis=1, keepdims=True)
        for a in (X, Wi, Zi):
            a.setflags(write=False)
        _PROBLEMS[shape] = (X, Wi, Zi)
    return _PROBLEMS[shape]


def _pivot_problem(kind, shape):
    """Leg 4: the table's kind of problem with the start weights made (nearly) rank deficient."""
    key = (kind,) + shape
    if key not in _PROBLEMS:
        X, Wi, Zi = _problem(shape)
        Z = np.array(Zi)
        if kind == "duplicate":
            Z[:, 1] = Z[:, 0]
            Z /= Z.sum(axis=1, keepdims=True)
        elif kind == "zero":
            Z[:, 2] = 0.0
            Z /= Z.sum(axis=1, keepdims=True)
        elif kind == "near":
            g = np.random.RandomState(77).standard_normal(shape[0])
            Z[:, 1] = Z[:, 0] * (1.0 + 1e-3 * g)
        Z.setflags(write=False)
        _PROBLEMS[key] = (X, Wi, Z)
    return _PROBLEMS[key]


# leg 4 systems that stay on the device: (kind, shape, lambda)
PIVOT_ON_DEVICE = [("zero", (200, 90, 5), 1.0), ("near", (300, 260, 12), 0.0), ("near", (200, 130, 33), 0.0)]
PIVOT_DUPLICATE = [(200, 90, 4), (200, 130, 33)]


# ---------------------------------------------------------------- extended-precision reference
def _gamma(j):
    j = LD(j)
    return j * U / (1 - j * U)


def _ld_cholesky(A):
    """Lower Cholesky factor in np.longdouble, row by row."""
    k = A.shape[0]
    L = np.zeros((k, k), dtype=LD)
    for j in range(k):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0, "the reference system is not positive definite"
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _ld_solve(L, B):
    """L L' Y = B by two substitutions in np.longdouble (B: k x m)."""
    k = L.shape[0]
    Y = np.array(B, dtype=LD)
    for i in range(k):
        if i:
            Y[i] -= L[i, :i].dot(Y[:i])
        Y[i] /= L[i, i]
    for i in range(k - 1, -1, -1):
        if i + 1 < k:
            Y[i] -= L[i + 1:, i].dot(Y[i + 1:])
        Y[i] /= L[i, i]
    return Y


def _gw(p, k):
    if k == 1:
        return np.zeros((1, 1), dtype=LD)
    return (LD(4) / (LD(p) * k * (k - 1))) * (k * np.eye(k, dtype=LD) - 1)


_REFERENCES = {}


def _solve_reference(key, X, Z, lam, rhs=None):
    """W' of (Z'Z/n + lambda GW) W' = Z'X/n in np.longdouble and the component-wise first-order bound
    on what a float64 Cholesky solve of the float64-formed system may differ from it:

        |dW'| <= |A^-1| (dB + dA |W'|) + gamma_2 |W'|
        dB = gamma_m |Z|'|X| / n                        (rhs given: it is exact, dB = gamma_1 |b|)
        dA = gamma_m |Z|'|Z| / n + gamma_4 |A| + gamma_(3k+2) |L||L'|
        gamma_j = j u / (1 - j u), u = 2^-53, m = n + 256 (covers any row padding of the kernels)

    dA: the Gram's accumulation, the division by n and the penalty's two operations, and the
    backward error of a Cholesky solve (Higham, Accuracy and Stability, theorem 10.4); the last term:
    the division of the right-hand side by n and the final rounding.  Everything is evaluated from
    the reference's own A, L and W'.  Returns (W' [k x p] as float64-exact longdouble, bound)."""
    ck = (key, float(lam), None if rhs is None else rhs.tobytes())
    if ck in _REFERENCES:
        return _REFERENCES[ck]
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 on this platform"
    n, k = Z.shape
    p = X.shape[1]
    Zl = np.asarray(Z, dtype=LD)
    absZtZ = np.abs(Zl).T.dot(np.abs(Zl))
    A = Zl.T.dot(Zl) / n + LD(lam) * _gw(p, k)
    m = n + 256
    if rhs is None:
        Xl = np.asarray(X, dtype=LD)
        B = Zl.T.dot(Xl) / n
        dB = _gamma(m) * np.abs(Zl).T.dot(np.abs(Xl)) / n
    else:
        B = np.asarray(rhs, dtype=LD) / n
        dB = _gamma(1) * np.abs(B)
    L = _ld_cholesky(A)
    Wt = _ld_solve(L, B)
    Ainv = _ld_solve(L, np.eye(k, dtype=LD))
    dA = _gamma(m) * absZtZ / n + _gamma(4) * np.abs(A) + _gamma(3 * k + 2) * np.abs(L).dot(np.abs(L).T)
    bound = np.abs(Ainv).dot(dB + dA.dot(np.abs(Wt))) + _gamma(2) * np.abs(Wt)
    _REFERENCES[ck] = (Wt, bound)
    return Wt, bound


def _solve_ratio(W, Wt_ref, bound):
    """Largest |error| / bound over the entries of the p x k dictionary W."""
    err = np.abs(np.asarray(W, dtype=LD).T - Wt_ref)
    assert np.all(bound > 0)
    return float((err / bound).max())


def _cost_reference(X, Z, W, lam):
    """0.5 (tr X'X - 2 <Z'X, W'> + <Z'Z, W'W>) / n + lambda penalty in np.longdouble, and gamma_m times the
    sum of the absolute values of every term that enters (m = n + p_pad + k^2 + 256)."""
    n, k = Z.shape
    p = X.shape[1]
    Xl, Zl, Wl = (np.asarray(a, dtype=LD) for a in (X, Z, W))
    tr = (Xl * Xl).sum()
    ZtX = Zl.T.dot(Xl)
    ZtZ = Zl.T.dot(Zl)
    G = Wl.T.dot(Wl)
    cost = LD(0.5) * (tr - 2 * (ZtX * Wl.T).sum() + (ZtZ * G).sum()) / n
    mag = LD(0.5) * (tr + 2 * (np.abs(ZtX) * np.abs(Wl.T)).sum() + (np.abs(ZtZ) * np.abs(G)).sum()) / n
    if lam != 0 and k > 1:
        pref = LD(lam) * LD(2) / (LD(k) * p * (k - 1))
        d = np.diag(G)
        iu = np.triu_indices(k, 1)
        cost += pref * (d[:, None] + d[None, :] - 2 * G)[iu].sum()
        mag += pref * (d[:, None] + d[None, :] + 2 * np.abs(G))[iu].sum()
    return cost, _gamma(n + _p_pad(p) + k * k + 256) * mag


# ---------------------------------------------------------------- legs 1 and 2: one device call per case
_DEVICE = {}


def _device_update(key, X, Wi, Z, lam, dtype):
    """One aa_gpnh_iterate with the dictionary update only: (error_stage, cost0, costs, W after the
    call, Z'X as the float32 pass kernel leaves it or None, the data as the device holds them)."""
    ck = (key, float(lam), dtype)
    if ck not in _DEVICE:
        from convex_dim_red import _backend
        k = Z.shape[1]
        Xh = X.astype(np.float32) if dtype == "float32" else X
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(Xh)
            ctx.gpnh_set_factors(k, W=Wi, Z=Z)
            ztx = ctx.gpnh_reduce(want_ztx=True, want_trace=False)[0] if dtype == "float32" else None
            cost0, costs, st = ctx.gpnh_iterate(lam, 1, 0.0, "rel_delta_f", False, True, False, {}, check_every=1)
            W = np.array(ctx.gpnh_get_dictionary())
        _DEVICE[ck] = (int(st.error_stage), cost0, np.array(costs), W, ztx, np.asarray(Xh, dtype=np.float64))
    return _DEVICE[ck]


def _check_solve(tag, key, X, Wi, Z, lam, dtype):
    stage, _, _, W, ztx, _ = _device_update(key, X, Wi, Z, lam, dtype)
    assert stage == 0, "the device left for the host loop (error_stage %d)" % stage
    assert W.shape == Wi.shape and np.all(np.isfinite(W))
    Wt_ref, bound = _solve_reference(key, X, Z, lam, rhs=ztx)
    ratio = _solve_ratio(W, Wt_ref, bound)
    print("gpnh-shapes %s %s lam %g %s: max |dW| / bound %.3e" % (tag, "_".join(map(str, key)), lam, dtype, ratio))
    assert ratio <= 1.0, (key, lam, dtype, ratio)


@gpu
@pytest.mark.parametrize("shape,lam", _cases(1))
def test_dictionary_solve_within_the_derived_bound(cdr, shape, lam):
    """Leg 1, float64 context: every entry of the solved dictionary within the first-order bound of
    `_solve_reference` (a float64 Cholesky on the CPU stays at 0.003 to 0.02 of it; an indexing or
    predicate error moves a whole row by orders of magnitude more)."""
    X, Wi, Zi = _problem(shape)
    _check_solve("leg1", shape, X, Wi, Zi, lam, "float64")


@gpu
@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("shape", F32_SOLVE_SHAPES, ids=_sid)
def test_dictionary_solve_float32_context(cdr, shape, lam):
    """Leg 1, float32 context: the right-hand side is what the float32 pass kernel produced (its
    accuracy is the business of tests/test_gpu_pass_kernels.py), fetched from the same context and
    taken as exact; Z'Z and the solve are float64 in both modes."""
    X, Wi, Zi = _problem(shape)
    _check_solve("leg1", shape, X, Wi, Zi, lam, "float32")


def _check_costs(tag, key, X, Wi, Z, lam, dtype):
    stage, cost0, costs, W, _, Xd = _device_update(key, X, Wi, Z, lam, dtype)
    assert stage == 0 and len(costs) == 2
    noise = _trace_noise(Xd, dtype)
    for name, got, Wd in (("cost0", cost0, Wi), ("costs[0]", costs[0], W)):
        want, bound = _cost_reference(Xd, Z, Wd, lam)
        bound = float(bound) + noise
        err = abs(float(LD(got) - want))
        print("gpnh-shapes %s %s lam %g %s %s: |dcost| / bound %.3e" % (tag, "_".join(map(str, key)), lam, dtype,
                                                                        name, err / bound))
        assert err <= bound, (key, lam, dtype, name, got, float(want), err, bound)
    assert costs[1] == costs[0]                     # no weights update: the cost is carried


@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,lam", _cases(2))
def test_cost_on_both_gram_paths(cdr, shape, lam, dtype):
    """Leg 2: the initial cost (W'W from the wide Gram kernels) and the cost after the dictionary
    update (W'W formed inside the cost kernel or by the wide kernels, as the table says) against the
    extended-precision cost of the factors the device holds."""
    X, Wi, Zi = _problem(shape)
    _check_costs("leg2", shape, X, Wi, Zi, lam, dtype)


# ---------------------------------------------------------------- leg 3: the whole device path
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("row", [r for r in TABLE if 3 in r[6]], ids=lambda r: _sid(r[0]))
def test_whole_path_vs_oracle(cdr, orc, row, dtype):
    """Leg 3: two outer iterations of _iterate_gpnh_convex_coding against the oracle, with the
    production weights solver (one SPG pass: lane-per-sample QP) and with six passes (four-lane QP
    at k <= 32, wave-per-sample above).  float64: cost 1e-10, W 1e-8 of max |W|, Z 1e-8; float32: the
    larger of 2e-4 on the cost and 20 x what the oracle's own twins do.  The cost is measured against
    max(|cost|, 1e-3 tr(XX')/n): tiny n reconstructs exactly.  Every row stays on the device, the
    one-sample and two-sample problems included."""
    from convex_dim_red import gpnh_convex_coding as gp
    shape, lams = row[0], row[1]
    n, p, k = shape
    X, Wi, Zi = _problem(shape)
    Xh = X.astype(np.float32) if dtype == "float32" else X
    Xd = np.asarray(Xh, dtype=np.float64)
    worst = dict(cost=0.0, W=0.0, Z=0.0)
    for lam in lams:
        for qp_kw in (dict(max_iterations=1), dict(max_iterations=6)):
            kw = dict(lambda_W=lam, tolerance=0, max_iterations=2, require_monotonic_cost_decrease=False,
                      weights_solver_kwargs=qp_kw)

            def oracle(Xin):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    return orc.iterate_gpnh(Xin, np.array(Zi), np.array(Wi), **kw)

            want = oracle(Xd)
            host_calls = []
            host_loop = gp._host_loop
            gp._host_loop = lambda *a, **kwa: host_calls.append(1) or host_loop(*a, **kwa)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    Z, W, cost, n_iter, _, deltas = gp._iterate_gpnh_convex_coding(Xh, np.array(Zi), np.array(Wi),
                                                                                   dtype=dtype, **kw)
            finally:
                gp._host_loop = host_loop
            assert not host_calls, "the device loop left for the host loop"      # (1, 1, 1) and (2, 5, 2) included
            assert n_iter == 1 and len(deltas) == 2
            assert W.shape == (p, k) and Z.shape == (n, k)
            _assert_simplex(Z)
            scale = max(abs(want[2]), 1e-3 * (Xd * Xd).sum() / n)
            if dtype == "float64":
                tol = 1e-10 * scale
            else:
                base = oracle(X)[2]
                twins = oracle_twins(orc, lambda Xin: oracle(Xin)[2], X, dtype)
                tol = max(2e-4 * scale, 20 * max(abs(t - base) for t in twins))
            dc = abs(cost - want[2])
            worst["cost"] = max(worst["cost"], dc / tol)
            assert dc <= tol, (shape, lam, qp_kw, cost, want[2], tol)
            if dtype == "float64":
                dW = np.abs(W - want[1]).max() / np.abs(want[1]).max()
                dZ = np.abs(Z - want[0]).max()
                worst["W"], worst["Z"] = max(worst["W"], dW / 1e-8), max(worst["Z"], dZ / 1e-8)
                assert dW < 1e-8, (shape, lam, qp_kw, dW)
                assert dZ < 1e-8, (shape, lam, qp_kw, dZ)
    print("gpnh-shapes leg3 %s %s: deviation / tolerance: cost %.3e, W %.3e, Z %.3e"
          % (_sid(shape), dtype, worst["cost"], worst["W"], worst["Z"]))


# ---------------------------------------------------------------- leg 4: the pivot test
@gpu
@pytest.mark.parametrize("shape", PIVOT_DUPLICATE, ids=_sid)
def test_duplicate_columns_leave_for_the_host_loop(cdr, orc, shape):
    """Two identical columns of the weights and lambda_W = 0: a pivot is rounding noise, below
    1e-13 of the largest diagonal entry.  aa_gpnh_iterate reports error_stage 3 and has written no
    row of the dictionary; the driver returns the oracle's lstsq result (tolerances of
    test_gpu_parity.py::test_gpnh_unused_component_falls_back_to_lstsq)."""
    from convex_dim_red import _backend
    from convex_dim_red import gpnh_convex_coding as gp
    X, Wi, Z = _pivot_problem("duplicate", shape)
    k = shape[2]
    with _backend.Context(dtype="float64") as ctx:
        ctx.set_data(X)
        ctx.gpnh_set_factors(k, W=Wi, Z=Z)
        _, costs, st = ctx.gpnh_iterate(0.0, 1, 0.0, "rel_delta_f", False, True, False, {}, check_every=1)
        assert st.error_stage == 3 and st.n_iter == -1 and len(costs) == 0
        assert np.array_equal(ctx.gpnh_get_dictionary(), Wi)           # bit for bit
    kw = dict(lambda_W=0.0, tolerance=0, max_iterations=1, update_weights=False,
              require_monotonic_cost_decrease=False)
    want = orc.iterate_gpnh(X, np.array(Z), np.array(Wi), **kw)
    Zf, W, cost, n_iter, _, _ = gp._iterate_gpnh_convex_coding(X, np.array(Z), np.array(Wi), **kw)
    assert np.array_equal(Zf, Z) and n_iter == 0
    assert abs(cost - want[2]) < 1e-10 * want[2]
    assert np.abs(W - want[1]).max() < 1e-9 * max(1.0, np.abs(want[1]).max())


@gpu
@pytest.mark.parametrize("kind,shape,lam", PIVOT_ON_DEVICE, ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_definite_systems_stay_on_the_device(cdr, kind, shape, lam):
    """A zero column rescued by lambda_W > 0 (GW makes the system definite), and nearly duplicate
    columns (smallest pivot about 1e-6 of the largest diagonal entry, far above 1e-13): the call stays
    on the device and the solve passes leg 1's bound; the cost passes leg 2's."""
    X, Wi, Z = _pivot_problem(kind, shape)
    _check_solve("leg4", (kind,) + shape, X, Wi, Z, lam, "float64")
    _check_costs("leg4", (kind,) + shape, X, Wi, Z, lam, "float64")


# ---------------------------------------------------------------- leg 5: restart slots beyond k = 16
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("R,n,p,k", [(3, 600, 300, 17), (2, 600, 260, 32)], ids=["3x17", "2x32"])
def test_slots_beyond_16_components_match_the_single_fit(cdr, R, n, p, k, dtype):
    """aa_gpnh_slots_begin accepts k <= 32 (include/aa_hip.h): every restart's weights, dictionary,
    cost record and initial cost are, bit for bit, what aa_gpnh_iterate gives the same start alone
    on a fresh context (k_gpnh_solve_slots<32>, the KP = 64 arrays of the stacked factors)."""
    from convex_dim_red import _backend
    rng = np.random.RandomState(500 + k)
    Zt = rng.uniform(size=(n, k))
    Zt /= Zt.sum(axis=1, keepdims=True)
    X = Zt.dot(rng.standard_normal((k, p))) + 0.1 * rng.standard_normal((n, p))
    Xh = X.astype(np.float32) if dtype == "float32" else X
    starts = []
    for _ in range(R):
        Z0 = rng.uniform(size=(n, k))
        starts.append((0.5 * rng.standard_normal((p, k)), Z0 / Z0.sum(axis=1, keepdims=True)))
    lam, iters, qp_kw = 0.5, 5, dict(max_iterations=1)
    alone = []
    for W0, Z0 in starts:
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(Xh)
            mono = 8 * 6e-8 * ctx.data_trace() / n if dtype == "float32" else 0.0
            ctx.gpnh_set_factors(k, W=W0, Z=Z0)
            cost0, costs, st = ctx.gpnh_iterate(lam, iters, 0.0, "rel_delta_f", False, True, True, qp_kw,
                                                check_every=8, mono_tolerance=mono)
            assert st.error_stage == 0 and st.n_iter == iters - 1
            alone.append((ctx.gpnh_get_weights(), np.array(ctx.gpnh_get_dictionary()), cost0, np.array(costs)))
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(Xh)
        ctx.gpnh_slots_begin(R, k, lam, iters, 0.0, "rel_delta_f", False, qp_kw, mono_tolerance=mono)
        for r, (W0, Z0) in enumerate(starts):
            ctx.gpnh_slots_load(r, W0, Z0)
        status = ctx.gpnh_slots_run(iters)
        for r, st in enumerate(status):
            assert st.stop and st.stop_iter == iters - 1 and not st.flags and not st.error_stage
            Z, W, cost0, costs = ctx.gpnh_slots_fetch(r, st.stop_iter)
            wZ, wW, wcost0, wcosts = alone[r]
            assert cost0 == wcost0, (r, cost0, wcost0)
            assert np.array_equal(costs, wcosts), (r, costs, wcosts)
            assert np.array_equal(W, wW), (r, np.abs(W - wW).max())
            assert np.array_equal(Z, wZ), (r, np.abs(Z - wZ).max())
        ctx.aa_slots_end()


@gpu
@pytest.mark.parametrize("p", [256, 257], ids=["in-kernel-gram", "wide-gram"])
def test_restarts_of_16_components_side_by_side(cdr, orc, p):
    """fit_restarts at the upper edge of what restarts._slots_eligible sends to the slots, k = 16 in
    four slots, with W'W of every slot formed inside the cost kernel (p = 256) and by the wide Gram
    kernels (p = 257): restart by restart the sequential loop's result, bit for bit."""
    from convex_dim_red import restarts
    n, k, n_init = 400, 16, 5
    rng = np.random.RandomState(16 + p)
    X = orc.right_stochastic_matrix((n, k), rng).dot(rng.standard_normal((k, p))) + 0.1 * rng.standard_normal((n, p))
    kw = dict(lambda_W=0.5, init="random", tolerance=0, max_iterations=6, stopping_criterion="rel_delta_f",
              require_monotonic_cost_decrease=False, weights_solver_kwargs=dict(max_iterations=1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        shared = np.random.RandomState(3)
        seq = []
        for _ in range(n_init):
            m = cdr.GPNHConvexCoding(k, random_state=shared, **kw)
            m.fit_transform(X)
            seq.append(m)
        shared = np.random.RandomState(3)
        restarts.slots_profile.clear()
        models, best = cdr.fit_restarts(lambda: cdr.GPNHConvexCoding(k, random_state=shared, **kw), X, n_init,
                                        n_slots=4)
    assert restarts.slots_profile["slots"] == 4
    for a, b in zip(seq, models):
        assert a.cost == b.cost and a.n_iter == b.n_iter
        assert list(a.cost_deltas) == list(b.cost_deltas)
        assert np.array_equal(a.weights, b.weights) and np.array_equal(a.dictionary, b.dictionary)
    assert best == int(np.argmin([m.cost for m in seq]))


# ---------------------------------------------------------------- host-only tests
def test_table_covers_every_dispatch_value():
    """Every row's expected KM, KP, number of solve blocks and Gram path follow from k and p by the
    launchers' rules, and every value of each is reached by a row that runs legs 1 and 2."""
    seen = dict(km=set(), kp=set(), blocks=set(), gram=set())
    for shape, _, km, kp, blocks, gram, legs in TABLE:
        assert _dispatch(shape[1], shape[2]) == (km, kp, blocks, gram), shape
        if 1 in legs and 2 in legs and 3 in legs:
            seen["km"].add(km)
            seen["kp"].add(kp)
            seen["blocks"].add(blocks)
            seen["gram"].add(gram)
    assert seen["km"] == {16, 32, 64}
    assert seen["kp"] == {32, 64}
    assert seen["blocks"] == {1, 2, 3}
    assert seen["gram"] == {"in4", "in2", "in1", "wide32", "wide64"}
    ks = {row[0][2] for row in TABLE}
    assert {1, 2, 8, 9, 11, 12, 16, 17, 32, 33, 64} <= ks          # both sides of every k threshold
    assert (333, 256, 16) in [row[0] for row in TABLE]              # k^2 = 256 and k p_pad = 4096 with equality
    assert all(shape in [row[0] for row in TABLE] for shape in F32_SOLVE_SHAPES)


def test_longdouble_solve_agrees_with_numpy():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 on this platform"
    rng = np.random.RandomState(0)
    M = rng.standard_normal((5, 5))
    A = M.dot(M.T) + 5 * np.eye(5)
    B = rng.standard_normal((5, 3))
    got = _ld_solve(_ld_cholesky(np.asarray(A, dtype=LD)), B)
    want = np.linalg.solve(A, B)
    assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-13 * np.abs(want).max()


def _numpy_cholesky_ratio(key, X, Z, lam):
    n, k = Z.shape
    p = X.shape[1]
    A = Z.T.dot(Z) / n + lam * np.asarray(_gw(p, k), dtype=np.float64)
    L = np.linalg.cholesky(A)
    W = np.linalg.solve(L.T, np.linalg.solve(L, Z.T.dot(X) / n)).T
    Wt_ref, bound = _solve_reference(key, X, Z, lam)
    return _solve_ratio(W, Wt_ref, bound)


@pytest.mark.parametrize("shape,lam", _cases(1))
def test_numpy_cholesky_stays_within_the_bound(shape, lam):
    """Keeps leg 1's bound honest without a GPU: a float64 NumPy Cholesky solve of the float64-formed
    system is within it, with room (0.003 to 0.02 of it on the table's shapes)."""
    X, _, Zi = _problem(shape)
    ratio = _numpy_cholesky_ratio(shape, X, Zi, lam)
    assert ratio <= 1.0, (shape, lam, ratio)


@pytest.mark.parametrize("kind,shape,lam", PIVOT_ON_DEVICE, ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_numpy_cholesky_stays_within_the_bound_on_the_pivot_systems(kind, shape, lam):
    X, _, Z = _pivot_problem(kind, shape)
    ratio = _numpy_cholesky_ratio((kind,) + shape, X, Z, lam)
    assert ratio <= 1.0, (kind, shape, lam, ratio)
