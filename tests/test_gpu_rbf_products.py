"""The implicit RBF kernel's products on the MI355X, element by element at their dispatch edges: K V of k_rbf_kv
through set_state / prepare / grams, rbf(Y, X_S) V of k_rbf_cross_mfma, the distance column of k_distance_rbf and
the features taken from a resident owner -- each against the long-double reference of tests/rbf_restatement.py
(squared differences, not the norm expansion the kernels use) within the bound derived there, plus the exact
facts: K is 1.0 between duplicated rows and never above 1.0, the identity on lattice points with gamma = 800,
the trace is n, a second call gives the same bits.

Every test prints ``rbf-errors`` lines with the largest |got - want| / bound; the MI355X run is in
profiles/rbf_product_errors.txt.  The cases and what each is there for: rbf_restatement.KV_CASES, CROSS_CASES,
DISTANCE_CASES, RESIDENT_CASES; tests/test_rbf_products_host.py holds the same bound against an emulation of the
kernels and shows that it notices planted faults."""
import numpy as np
import pytest

import rbf_restatement as rr

pytestmark = pytest.mark.gpu

LD = rr.LD


@pytest.fixture(scope="module")
def backend():
    from convex_dim_red import _backend
    _backend.require_gpu()
    return _backend


def _one_hot_groups(rows, k, pairs):
    """Selections of k rows for the one-hot C: each pair first (both rows in one selection), then ``rows`` k at
    a time; a short selection is filled from the head of ``rows``."""
    groups = [list(pair)[:k] for pair in pairs] + [list(rows[i:i + k]) for i in range(0, len(rows), k)]
    return [np.array((g + list(rows) * k)[:k]) for g in groups]


class _Reference(object):
    """K, its entry bound and the bound of a term of an n-term product, for the rows asked for (all rows up to
    n = 900), indexed by row number."""

    def __init__(self, X, gamma, rows):
        n = X.shape[0]
        self.rows = np.arange(n) if n <= rr.KV_RANDOM_FACTORS_UP_TO else np.unique(rows)
        self.at = np.full(n, -1)
        self.at[self.rows] = np.arange(len(self.rows))
        self.K, s = rr.reference(X, X, gamma, self.rows)
        E = rr.entry_E(X, X, gamma, s, self.rows)
        self.B0, self.Bn = rr.entry_bound(self.K, E), rr.entry_bound(self.K, E, n)

    def take(self, sel):
        assert np.all(self.at[sel] >= 0)
        return self.at[sel]


def _judge_products(ctx, what, pb, ref, twins=(), near=(), identity=False):
    """The random-factor run (all rows referenced) and the one-hot runs on a context whose kernel is set; returns
    the Grams of the random-factor run (None above 900 rows).  Prints the largest ratios."""
    n, k, C0, Z0 = pb["n"], pb["k"], pb["C0"], pb["Z0"]
    Zl = Z0.astype(LD)
    dense = None
    ratios = {}
    if n <= rr.KV_RANDOM_FACTORS_UP_TO:
        ctx.set_state(C0, Z0, np.ones(k))
        ctx.prepare()
        dense = ctx.grams()
        Cl = C0.astype(LD)
        for name, got, V in (("C K C'", dense[1], Cl.T), ("C K Z", dense[2], Zl)):
            ratios["random " + name] = rr.ratio(got, Cl.dot(ref.K).dot(V), Cl.dot(ref.Bn).dot(V))
        assert dense[3] == float(n)
    r_rows = r_entries = 0.0
    for sel in _one_hot_groups(pb["rows"], k, list(twins) + list(near)):
        C1 = np.zeros((k, n))
        C1[np.arange(k), sel] = 1.0
        ctx.set_state(C1, Z0, np.ones(k))
        ctx.prepare()
        _, CKCt, CKZ, tr = ctx.grams()
        i = ref.take(sel)
        r_rows = max(r_rows, rr.ratio(CKZ, ref.K[i].dot(Zl), ref.Bn[i].dot(Zl)))          # rows of K Z0
        r_entries = max(r_entries, rr.ratio(CKCt, ref.K[i][:, sel], ref.B0[i][:, sel]))    # entries of K
        assert CKCt.max() <= 1.0, sel                       # the clamp
        assert np.all(CKCt[sel[:, None] == sel[None, :]] == 1.0), sel       # the diagonal shortcut
        if identity:
            assert np.array_equal(CKZ, Z0[sel]), sel
            assert np.array_equal(CKCt, (sel[:, None] == sel[None, :]).astype(np.float64)), sel
        if len(sel) > 1 and (sel[0], sel[1]) in [tuple(t) for t in twins]:
            assert CKCt[0, 1] == 1.0 and CKCt[1, 0] == 1.0, sel             # d2 exactly 0 between duplicated rows
        assert tr == float(n)
    ratios["one-hot rows of K Z"], ratios["entries of K"] = r_rows, r_entries
    print("rbf-errors %s: max |got - want| / bound: %s"
          % (what, ", ".join("%s %.3f" % (name, r) for name, r in sorted(ratios.items()))))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    return dense


@pytest.mark.parametrize("case", rr.KV_CASES, ids=str)
def test_kv_through_grams(backend, case):
    """K V of k_rbf_kv<32|64> at the tile, chunk and split edges (rbf_restatement.KV_CASES).  With random stochastic
    factors (n <= 900) C K C' and C K Z are held to |C| (2 u (E + n) o K) |V|; with one-hot rows of C -- prepare's
    kernel-form branch forms C K Z = C (K Z) and C K C' = (K C')' C' with the Gram kernel, a sum of exact zeros
    and one term -- C K Z is the selected rows of K Z0 and C K C' single entries of K, held to the entry bound.
    Family (c): exactly 1.0 between duplicated rows; every family: no entry above 1.0, the diagonal 1.0, the
    trace n; family (d): the identity bit for bit.  Setting the features again gives the same bits."""
    pb = rr.kv_problem(case)
    pairs = pb["twins"] + pb["near"]
    ref = _Reference(pb["X"], pb["gamma"], np.concatenate([pb["rows"]] + [np.array(t) for t in pairs]))
    with backend.Context(dtype="float64") as ctx:
        ctx.set_rbf_features(pb["X"], pb["gamma"])
        dense = _judge_products(ctx, "K V n %d p %d k %d family %s" % case, pb, ref, pb["twins"], pb["near"],
                                identity=pb["name"] == "d")
        first = ctx.grams()                                 # of the last one-hot selection
        ctx.set_rbf_features(pb["X"], pb["gamma"])
        if dense is not None:
            ctx.set_state(pb["C0"], pb["Z0"], np.ones(pb["k"]))
            ctx.prepare()
            again = ctx.grams()
            assert all(np.array_equal(a, b) for a, b in zip(dense, again))
        else:
            sel = _one_hot_groups(pb["rows"], pb["k"], [])[-1]
            C1 = np.zeros((pb["k"], pb["n"]))
            C1[np.arange(pb["k"]), sel] = 1.0
            ctx.set_state(C1, pb["Z0"], np.ones(pb["k"]))
            ctx.prepare()
            assert all(np.array_equal(a, b) for a, b in zip(first, ctx.grams()))


@pytest.mark.parametrize("case", rr.CROSS_CASES, ids=str)
def test_cross_product(backend, case):
    """rbf(Y, X_S) V of k_rbf_cross_mfma<32|64> element by element: Y holds copies of reference rows, rows whose
    every kernel value is thirty and more orders of magnitude below those (free to be wrong under a bound
    relative to the largest entry) and fresh rows.  The norms are k_rbf_norms' (p fma's each), as the bound
    counts them; no diagonal term.  The last case has three column splits of 2, 2 and 1 tiles."""
    pb = rr.cross_problem(case)
    rows = np.arange(pb["m"]) if pb["rows"] is None else pb["rows"]
    K, s = rr.reference(pb["Y"], pb["XS"], pb["gamma"], rows)
    E = rr.entry_E(pb["Y"], pb["XS"], pb["gamma"], s, rows)
    V = pb["V"].astype(LD)
    with backend.Context(dtype="float64") as ctx:
        ctx.set_data(pb["Y"])
        ctx.set_rbf_reference(pb["XS"], pb["V"], pb["gamma"])
        got = ctx.rbf_cross(fetch=True)
        again = ctx.rbf_cross(fetch=True)
    assert got.shape == (pb["m"], pb["k"])
    r = rr.ratio(got[rows], K.dot(V), rr.entry_bound(K, E, pb["s"]).dot(V))
    kind = pb["kind"][rows]
    far = float(np.abs(got[rows][kind == 1]).max()) if np.any(kind == 1) else 0.0
    print("rbf-errors cross m %d s %d p %d k %d: max |got - want| / bound %.3f (largest entry of a far row %.1e)"
          % (case + (r, far)))
    assert r <= 1.0
    assert np.array_equal(got, again)


@pytest.mark.parametrize("case", rr.DISTANCE_CASES, ids=str)
def test_distance_column(backend, case):
    """k_distance_rbf at the ends of its lane loop and of its four rows per block: the squares against
    t = -2 expm1(-gamma s) within 4 u (gamma s (p + 4) e + 2 e + 2 + t); exactly 0 for row j and for its copy."""
    n, p, columns = case
    worst = 0.0
    with backend.Context(dtype="float64") as ctx:
        for j in columns:
            X, gamma = rr.distance_problem(case, j)
            ctx.set_rbf_features(X, gamma)
            d = ctx.distance_column(j)
            t, bound = rr.distance_reference(X, gamma, j)
            worst = max(worst, rr.ratio(d.astype(LD) ** 2, t, bound))
            assert d.shape == (n,) and d[j] == 0.0 and d[(j + 1) % n] == 0.0
    print("rbf-errors distance column n %d p %d: max |d^2 - t| / bound %.3f" % (n, p, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("case", rr.RESIDENT_CASES, ids=str)
def test_resident_features(backend, case):
    """set_rbf_features_resident from a float32 and a float64 owner (p = 1, 127, 129: p_pad 128, 128, 256): the
    products meet the bound against the reference built from the values the owner stores, and have the bits of
    set_rbf_features on those values."""
    pb = rr.resident_problem(case)
    ref = _Reference(pb["Xs"], pb["gamma"], pb["rows"])
    grams = []
    with backend.Context(dtype=case[0]) as owner, backend.Context(dtype="float64") as ctx:
        owner.set_data(pb["X"])
        for resident in (True, False):
            if resident:
                ctx.set_rbf_features_resident(owner, pb["gamma"])
            else:
                ctx.set_rbf_features(pb["Xs"], pb["gamma"])
            dense = _judge_products(ctx, "resident %s p %d (%s)" % (case + ("owner" if resident else "host copy",)),
                                    pb, ref)
            grams.append(dense + ctx.grams())               # the random factors' and the last selection's
    assert all(np.array_equal(a, b) for a, b in zip(*grams))
