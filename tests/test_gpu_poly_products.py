"""The implicit polynomial kernel's products on the MI355X, element by element at their dispatch edges: K V of
k_poly_kv_mfma through set_poly_features / set_state / prepare / grams, poly(Y, X_S) V of the same kernel in its
cross launch, the distance column of k_distance_poly, the trace of k_poly_trace, the AA_DIAG_POLY diagonal of
k_kernel_sample_residuals and the features taken from a resident owner -- each against the long-double reference
of tests/poly_restatement.py (the power by ``**``, not the device's multiplication chain) within the bound derived
there in A = sum|y||x| and b, not in |K|: degrees 1, 2, 3, 5 and 8, coef0 = 0 on centred data, planted pairs with
gamma y.x + coef0 = 0 to rounding, data far from the origin.  On the integer lattice (family e) every product and
the trace equal the integer result bit for bit.

Every test prints ``poly-errors`` lines with the largest |got - want| / bound; the MI355X run is in
profiles/poly_product_errors.txt.  The cases and what each is there for: poly_restatement.FIT_CASES, CROSS_CASES,
DISTANCE_CASES, RESIDENT_CASES; tests/test_poly_products_host.py holds the same bound against an emulation of the
kernels and shows that it notices planted faults."""
import numpy as np
import pytest

import poly_restatement as pr
from test_gpu_rbf_products import _one_hot_groups

pytestmark = pytest.mark.gpu

LD = pr.LD


@pytest.fixture(scope="module")
def backend():
    from convex_dim_red import _backend
    _backend.require_gpu()
    return _backend


def _spec(pb):
    return pb["gamma"], pb["coef0"], pb["degree"]


def _judge_products(ctx, what, pb, ref):
    """The random-factor run (all rows referenced, n <= 900) and the one-hot runs on a context whose kernel is
    set, the trace with each; returns the Grams of the random-factor run (None above 900 rows).  On the lattice
    everything is compared with ``np.array_equal`` as well.  Prints the largest ratios."""
    n, k, C0, Z0 = pb["n"], pb["k"], pb["C0"], pb["Z0"]
    Zl = Z0.astype(LD)
    exact = ref.exact
    want_tr, tr_bound = pr.trace_reference(pb["X"], *_spec(pb))
    dense = None
    ratios = {}
    if n <= pr.RANDOM_FACTORS_UP_TO:
        ctx.set_state(C0, Z0, np.ones(k))
        ctx.prepare()
        dense = ctx.grams()
        Cl = C0.astype(LD)
        for name, got, V in (("C K C'", dense[1], Cl.T), ("C K Z", dense[2], Zl)):
            ratios["random " + name] = pr.ratio(got, Cl.dot(ref.K).dot(V), Cl.dot(ref.en).dot(V))
        if exact is not None:
            assert np.array_equal(dense[1], exact["CKCt"]) and np.array_equal(dense[2], exact["CKV"])
    r_rows = r_entries = r_trace = 0.0
    for sel in _one_hot_groups(pb["rows"], k, pb["zeros"] + pb["near"]):
        C1 = np.zeros((k, n))
        C1[np.arange(k), sel] = 1.0
        ctx.set_state(C1, Z0, np.ones(k))
        ctx.prepare()
        _, CKCt, CKZ, tr = ctx.grams()
        i = ref.take(sel)
        r_rows = max(r_rows, pr.ratio(CKZ, ref.K[i].dot(Zl), ref.en[i].dot(Zl)))          # rows of K Z0
        r_entries = max(r_entries, pr.ratio(CKCt, ref.K[i][:, sel], ref.e[i][:, sel]))     # entries of K
        r_trace = max(r_trace, float(abs(LD(tr) - want_tr) / tr_bound))
        if exact is not None:
            assert np.array_equal(CKZ, exact["KV"][i]), sel
            assert np.array_equal(CKCt, exact["K"][i][:, sel]), sel
            assert tr == float(want_tr)
    ratios["one-hot rows of K Z"], ratios["entries of K"], ratios["trace"] = r_rows, r_entries, r_trace
    print("poly-errors %s: max |got - want| / bound: %s%s"
          % (what, ", ".join("%s %.3f" % (name, r) for name, r in sorted(ratios.items())),
             "; lattice: every product and the trace equal the integer result" if exact is not None else ""))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    return dense


def _planted_rows(pb):
    return [r for pair in pb["zeros"] + pb["near"] for r in pair]


@pytest.mark.parametrize("case", pr.FIT_CASES, ids=str)
def test_fit_through_grams(backend, case):
    """K V of k_poly_kv_mfma<32|64> in the fit's launch (Y = X_S = the features, ld = p rounded up to 32, columns
    padded to 128: whole column tiles of padding) at the tile, k-step, chunk and split edges
    (poly_restatement.FIT_CASES).  With random stochastic factors (n <= 900) C K C' and C K Z are held to
    |C| (e + 2 n u |K|) |V|; with one-hot rows of C -- prepare's kernel-form branch forms C K Z = C (K Z) and
    C K C' = (K C')' C' with the Gram kernel, a sum of exact zeros and one term -- C K Z is the selected rows of
    K Z0 and C K C' single entries of K, held to the entry bound e; family (c)'s planted pairs sit in one
    selection each.  The trace within its bound.  The lattice: all of these bit for bit.  Setting the features
    again gives the same bits."""
    pb = pr.fit_problem(case)
    ref = pr.FitReference(pb, _planted_rows(pb))
    with backend.Context(dtype="float64") as ctx:
        ctx.set_poly_features(pb["X"], *_spec(pb))
        dense = _judge_products(ctx, "K V n %d p %d k %d degree %d family %s" % case, pb, ref)
        first = ctx.grams()                                 # of the last one-hot selection
        ctx.set_poly_features(pb["X"], *_spec(pb))
        if dense is not None:
            ctx.set_state(pb["C0"], pb["Z0"], np.ones(pb["k"]))
            ctx.prepare()
            assert all(np.array_equal(a, b) for a, b in zip(dense, ctx.grams()))
        else:
            sel = _one_hot_groups(pb["rows"], pb["k"], [])[-1]
            C1 = np.zeros((pb["k"], pb["n"]))
            C1[np.arange(pb["k"]), sel] = 1.0
            ctx.set_state(C1, pb["Z0"], np.ones(pb["k"]))
            ctx.prepare()
            assert all(np.array_equal(a, b) for a, b in zip(first, ctx.grams()))


@pytest.mark.parametrize("case", pr.CROSS_CASES, ids=str)
def test_cross_product(backend, case):
    """poly(Y, X_S) V of k_poly_kv_mfma<32|64> in the cross launch (ld = p_pad, columns padded to 64) element by
    element within (e + 2 s u |K|) |V|; the lattice bit for bit in every row; duplicated rows of Y give equal
    rows; a second call the same bits.  The last two cases have 30 column splits of 2 tiles."""
    pb = pr.cross_problem(case)
    rows = np.arange(pb["m"]) if pb["rows"] is None else pb["rows"]
    K, b, A = pr.reference(pb["Y"], pb["XS"], pb["gamma"], pb["coef0"], pb["degree"], rows)
    e = pr.entry_bound(b, A, pb["gamma"], pb["degree"], pr.round_up(pb["p"], 4))
    V = pb["V"].astype(LD)
    with backend.Context(dtype="float64") as ctx:
        ctx.set_data(pb["Y"])
        ctx.set_poly_reference(pb["XS"], pb["V"], *_spec(pb))
        got = ctx.poly_cross(fetch=True)
        again = ctx.poly_cross(fetch=True)
    assert got.shape == (pb["m"], pb["k"])
    r = pr.ratio(got[rows], K.dot(V), pr.term_bound(e, K, pb["s"]).dot(V))
    lattice = pb["name"] == "e"
    if lattice:
        assert np.array_equal(got, pr.lattice_exact(pb["Y"], pb["XS"], pb["coef0"], pb["degree"], pb["V"])["KV"])
    print("poly-errors cross m %d s %d p %d k %d degree %d family %s: max |got - want| / bound %.3f%s"
          % (case + (r, "; lattice: equal to the integer result" if lattice else "")))
    assert r <= 1.0
    for a, c in pb["twins"]:
        assert np.array_equal(got[a], got[c]), (a, c)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("case", pr.DISTANCE_CASES, ids=str)
def test_distance_column(backend, case):
    """k_distance_poly at the ends of its lane loop and of its four rows per block, on families (b), (c) and (e):
    the squares against D2 = K_ii - 2 K_ij + K_jj from three long-double values within
    e_ii + 2 e_ij + e_jj + 4 u (T + D2); where D2 is below its bound, d^2 <= 2 x bound; exactly 0 for row j and for
    its copy."""
    n, p, columns, degree, name = case
    worst, below = 0.0, 0
    with backend.Context(dtype="float64") as ctx:
        for j in columns:
            pb = pr.distance_problem(case, j)
            ctx.set_poly_features(pb["X"], pb["gamma"], pb["coef0"], degree)
            d = ctx.distance_column(j)
            D2, bound = pr.distance_reference(pb["X"], j, pb["gamma"], pb["coef0"], degree)
            d2 = d.astype(LD) ** 2
            worst = max(worst, pr.ratio(d2, D2, bound))
            small = np.asarray(D2 < bound)
            below += int(small.sum())
            assert np.all(d2[small] <= 2 * bound[small])
            assert d.shape == (n,) and d[j] == 0.0 and d[(j + 1) % n] == 0.0
    print("poly-errors distance column n %d p %d degree %d family %s: max |d^2 - D2| / bound %.3f (%d squares below "
          "their bound)" % (n, p, degree, name, worst, below))
    assert worst <= 1.0


@pytest.mark.parametrize("case", pr.TRACE_CASES, ids=str)
def test_trace(backend, case):
    """k_poly_trace on families (b) to (d) -- norms of every scale, coef0 = 0 among them -- within
    sum e_ii + n u sum|K_ii|; the same bits from two calls."""
    pb = pr.fit_problem(case)
    want, bound = pr.trace_reference(pb["X"], *_spec(pb))
    k = pb["k"]
    traces = []
    with backend.Context(dtype="float64") as ctx:
        for _ in range(2):
            ctx.set_poly_features(pb["X"], *_spec(pb))
            ctx.set_state(pb["C0"], pb["Z0"], np.ones(k))
            ctx.prepare()
            traces.append(ctx.grams()[3])
    r = float(abs(LD(traces[0]) - want) / bound)
    print("poly-errors trace n %d p %d k %d degree %d family %s: |got - want| / bound %.3f" % (case + (r,)))
    assert r <= 1.0 and traces[0] == traces[1]


@pytest.mark.parametrize("case", pr.DIAGONAL_CASES, ids=str)
def test_sample_residuals_diagonal(backend, case):
    """kernel_sample_residuals(kind='poly') behind a cross product on family (c): the diagonal it writes,
    poly_kappa of k_rbf_norms' |y_t|^2, against the long-double diagonal within the entry bound, and its sum
    (sums[1]) within the trace bound."""
    pb = pr.cross_problem(case)
    m, k = pb["m"], pb["k"]
    rng = np.random.RandomState(m + k)
    K, e = pr.diagonal_reference(pb["Y"], *_spec(pb))
    want, bound = pr.trace_reference(pb["Y"], *_spec(pb))
    with backend.Context(dtype="float64") as ctx:
        ctx.set_data(pb["Y"])
        ctx.set_poly_reference(pb["XS"], pb["V"], *_spec(pb))
        ctx.poly_cross()
        ctx.gpnh_set_factors(k, Z=pr.stochastic(rng, (m, k)))
        _, diag, _, sum_d = ctx.kernel_sample_residuals(np.eye(k), "poly")
    r_diag = pr.ratio(diag, K, e)
    r_sum = float(abs(LD(sum_d) - want) / bound)
    print("poly-errors residual diagonal m %d s %d p %d k %d degree %d family %s: max |got - want| / bound: "
          "diagonal %.3f, its sum %.3f" % (case + (r_diag, r_sum)))
    assert diag.shape == (m,) and r_diag <= 1.0 and r_sum <= 1.0


@pytest.mark.parametrize("case", pr.RESIDENT_CASES, ids=str)
def test_resident_features(backend, case):
    """set_poly_features_resident from a float32 and a float64 owner (p = 1, 127, 129: p_pad 128, 128, 256) on
    family (b): the products meet the bound against the reference built from the values the owner stores, and have
    the bits of set_poly_features on those values."""
    pb = pr.resident_problem(case)
    ref = pr.FitReference(pb)
    grams = []
    with backend.Context(dtype=case[0]) as owner, backend.Context(dtype="float64") as ctx:
        owner.set_data(pb["owner_X"])
        for resident in (True, False):
            if resident:
                ctx.set_poly_features_resident(owner, *_spec(pb))
            else:
                ctx.set_poly_features(pb["X"], *_spec(pb))
            dense = _judge_products(ctx, "resident %s p %d (%s)" % (case + ("owner" if resident else "host copy",)),
                                    pb, ref)
            grams.append(dense + ctx.grams())               # the random factors' and the last selection's
    assert all(np.array_equal(a, b) for a, b in zip(*grams))
