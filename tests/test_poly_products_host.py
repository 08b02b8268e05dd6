"""The polynomial product tests' own machinery, checked on the host (tests/poly_restatement.py): the NumPy emulation
of k_poly_kv_mfma (fit and cross launch), k_distance_poly, k_poly_trace and the AA_DIAG_POLY diagonal meets the
derived bound against the long-double reference on every case of tests/test_gpu_poly_products.py and equals the
integer result bit for bit on the lattice; every planted fault is noticed by a case of the table it belongs to;
the bound of tests/test_gpu_kernel_poly.py, relative to |K|, is exceeded by the correct emulation where b cancels;
and the tables reach every shape, degree and split they are there for."""
import numpy as np
import pytest

import poly_restatement as pr
from test_gpu_kernel_poly import _product_bound

LD = pr.LD


def _planted_rows(pb):
    return [r for pair in pb["zeros"] + pb["near"] for r in pair]


def _judge_fit(pb, ref, entries, out, padding_row):
    """What the GPU test can see of a fit, on the emulation's K[rows], (K Z0)[rows] and -- for the random factors,
    n <= 900 -- C0 (K Z0): the largest ratios to the entry bound and the product bounds, and the exact facts as a
    list of the ones broken (the lattice bit for bit; the padding row, which only the emulation shows)."""
    Zl = pb["Z0"].astype(LD)
    r_entry = pr.ratio(entries, ref.K, ref.e)
    r_prod = pr.ratio(out, ref.K.dot(Zl), ref.en.dot(Zl))
    broken = []
    if pb["n"] <= pr.RANDOM_FACTORS_UP_TO:
        Cl = pb["C0"].astype(LD)
        r_prod = max(r_prod, pr.ratio(pb["C0"].dot(out), Cl.dot(ref.K).dot(Zl), Cl.dot(ref.en).dot(Zl)))
        if ref.exact is not None and not np.array_equal(pb["C0"].dot(out), ref.exact["CKV"]):
            broken.append("lattice C K Z")
    if ref.exact is not None:
        if not np.array_equal(entries, ref.exact["K"]):
            broken.append("lattice K")
        if not np.array_equal(out, ref.exact["KV"]):
            broken.append("lattice K Z")
    if np.any(padding_row != 0.0):
        broken.append("padding row")
    return r_entry, r_prod, broken


def _emulate_fit(pb, ref, fault=None):
    return pr.emulate_product(pb["X"], pb["X"], pb["gamma"], pb["coef0"], pb["degree"], pb["Z0"], ref.rows,
                              fault=fault)


_worst = {}


def _note(table, r):
    _worst[table] = max(_worst.get(table, 0.0), r)
    print("largest ratio of table %s so far: %.3f" % (table, _worst[table]))


@pytest.mark.parametrize("case", pr.FIT_CASES, ids=str)
def test_emulated_fit_meets_the_bound(case):
    pb = pr.fit_problem(case)
    ref = pr.FitReference(pb, _planted_rows(pb))
    r_entry, r_prod, broken = _judge_fit(pb, ref, *_emulate_fit(pb, ref))
    print("emulated fit %s: max |got - want| / bound: entries %.3f, product %.3f%s"
          % (case, r_entry, r_prod, "; lattice: equal, bits %s" % ref.exact["bits"] if ref.exact else ""))
    _note("fit", max(r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0 and not broken, (r_entry, r_prod, broken)
    if pb["zeros"]:                                         # the planted pairs are what they are said to be
        for a, b in pb["zeros"]:
            i = ref.take(np.array([a]))[0]
            assert abs(ref.K[i, b]) <= ref.e[i, b] and ref.e[i, b] < 1e-12 * abs(ref.K[i, a])


def _judge_cross(pb, entries, out, padding_row):
    rows = np.arange(pb["m"]) if pb["rows"] is None else pb["rows"]
    broken = []
    if pb["name"] == "e":
        exact = pr.lattice_exact(pb["Y"], pb["XS"], pb["coef0"], pb["degree"], pb["V"], rows=rows)
        if not np.array_equal(entries, exact["K"]):
            broken.append("lattice K")
        if not np.array_equal(out, exact["KV"]):
            broken.append("lattice K V")
    K, b, A = pr.reference(pb["Y"], pb["XS"], pb["gamma"], pb["coef0"], pb["degree"], rows)
    e = pr.entry_bound(b, A, pb["gamma"], pb["degree"], pr.round_up(pb["p"], 4))
    V = pb["V"].astype(LD)
    where = {int(r): i for i, r in enumerate(rows)}
    for a, c in pb["twins"]:
        if a in where and c in where and not np.array_equal(out[where[a]], out[where[c]]):
            broken.append("twins %d %d" % (a, c))
    if np.any(padding_row != 0.0):
        broken.append("padding row")
    return pr.ratio(entries, K, e), pr.ratio(out, K.dot(V), pr.term_bound(e, K, pb["s"]).dot(V)), broken


def _emulate_cross(pb, fault=None):
    return pr.emulate_product(pb["Y"], pb["XS"], pb["gamma"], pb["coef0"], pb["degree"], pb["V"], pb["rows"],
                              same_set=False, fault=fault)


@pytest.mark.parametrize("case", pr.CROSS_CASES, ids=str)
def test_emulated_cross_meets_the_bound(case):
    pb = pr.cross_problem(case)
    r_entry, r_prod, broken = _judge_cross(pb, *_emulate_cross(pb))
    print("emulated cross %s: max |got - want| / bound: entries %.3f, product %.3f" % (case, r_entry, r_prod))
    _note("cross", max(r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0 and not broken, (r_entry, r_prod, broken)


@pytest.mark.parametrize("case", pr.DISTANCE_CASES, ids=str)
def test_emulated_distance_meets_the_bound(case):
    n = case[0]
    for j in case[2]:
        pb = pr.distance_problem(case, j)
        spec = (pb["gamma"], pb["coef0"], case[3])
        d = pr.emulate_distance(pb["X"], j, *spec)
        D2, bound = pr.distance_reference(pb["X"], j, *spec)
        r = pr.ratio(d * d, D2, bound)
        small = np.asarray(D2 < bound)
        print("emulated distance column %s j %d: max |d^2 - D2| / bound %.3f, %d of %d below their bound"
              % (case[:2] + case[3:], j, r, small.sum(), n))
        _note("distance", r)
        assert r <= 1.0 and d[j] == 0.0 and d[(j + 1) % n] == 0.0
        assert np.all((d * d)[small] <= 2 * bound[small])
        if case[4] == "e":                                  # the lattice: the square is an integer, held exactly
            assert np.array_equal(np.sqrt(D2.astype(np.float64)), d)


@pytest.mark.parametrize("case", pr.RESIDENT_CASES, ids=str)
def test_emulated_resident_meets_the_bound(case):
    pb = pr.resident_problem(case)
    ref = pr.FitReference(pb)
    r_entry, r_prod, broken = _judge_fit(pb, ref, *_emulate_fit(pb, ref))
    print("emulated resident %s: max |got - want| / bound: entries %.3f, product %.3f" % (case, r_entry, r_prod))
    _note("resident", max(r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0 and not broken


@pytest.mark.parametrize("case", pr.TRACE_CASES + pr.DIAGONAL_CASES, ids=str)
def test_emulated_trace_and_diagonal_meet_the_bound(case):
    """k_poly_trace on the features of a fit case; the AA_DIAG_POLY diagonal and its sum on the new rows of a cross
    case (six fields)."""
    pb = pr.fit_problem(case) if len(case) == 5 else pr.cross_problem(case)
    X = pb["X"] if len(case) == 5 else pb["Y"]
    spec = (pb["gamma"], pb["coef0"], pb["degree"])
    K, e = pr.diagonal_reference(X, *spec)
    want, bound = pr.trace_reference(X, *spec)
    r_diag = pr.ratio(pr.emulate_diagonal(X, *spec), K, e)
    r_trace = float(abs(LD(pr.emulate_trace(X, *spec)) - want) / bound)
    print("emulated trace %s: max |got - want| / bound: diagonal %.3f, trace %.3f" % (case, r_diag, r_trace))
    _note("trace", max(r_diag, r_trace))
    assert r_diag <= 1.0 and r_trace <= 1.0


@pytest.mark.parametrize("case", [c for c in pr.FIT_CASES if c[4] == "e"], ids=str)
def test_lattice_is_exactly_representable(case):
    """lattice_exact's Python-integer assertion holds with the bits the issue worked out (about 25 per entry at
    p = 65, degree 3), and the lattice trace is an integer far below 2^53."""
    pb = pr.fit_problem(case)
    ref = pr.FitReference(pb)
    bits = ref.exact["bits"]
    print("lattice %s: bits needed %s of %d allowed" % (case, bits, pr.LATTICE_BITS))
    assert max(bits.values()) <= pr.LATTICE_BITS < 53
    diag = pr.emulate_diagonal(pb["X"], pb["gamma"], pb["coef0"], pb["degree"])
    assert np.array_equal(diag, np.rint(diag)) and diag.sum() < 2.0 ** pr.LATTICE_BITS
    assert pr.emulate_trace(pb["X"], pb["gamma"], pb["coef0"], pb["degree"]) == diag.sum()


# fault -> (table, the case whose inputs notice it, how: "bound" (a ratio above 1) or the exact fact that breaks)
PLANTED = {"drop_last_kstep": ("fit", (65, 5, 32, 5, "b"), "bound"),
           "padding_column_counted": ("fit", (65, 31, 64, 2, "d"), "bound"),
           "skip_last_tile": ("fit", (3500, 33, 33, 5, "b"), "bound"),
           "sum_leaves_out_split": ("fit", (900, 5, 17, 8, "c"), "bound"),
           "degree_off_by_one": ("fit", (128, 33, 33, 1, "b"), "bound"),
           "coef0_after_power": ("fit", (64, 4, 17, 2, "c"), "bound"),
           "gamma_on_coef0": ("fit", (130, 31, 16, 5, "d"), "bound"),
           "component_tile_to_neighbour": ("fit", (129, 1, 17, 3, "c"), "bound"),
           "rows_not_zeroed": ("fit", (65, 31, 64, 2, "d"), "padding row")}
# the same faults on the lattice and in the cross launch: a differing bit
PLANTED_EXACT = {"drop_last_kstep": ("fit", (64, 65, 32, 3, "e"), "lattice K"),
                 "padding_column_counted": ("cross", (200, 63, 33, 32, 3, "e"), "lattice K V"),
                 "skip_last_tile": ("fit", (2100, 65, 17, 3, "e"), "lattice K Z"),
                 "sum_leaves_out_split": ("cross", (1100, 3800, 5, 33, 3, "e"), "lattice K V"),
                 "degree_off_by_one": ("fit", (130, 3, 33, 3, "e"), "lattice K"),
                 "coef0_after_power": ("fit", (129, 64, 64, 2, "e"), "lattice K"),
                 "component_tile_to_neighbour": ("cross", (200, 63, 129, 64, 2, "e"), "lattice K V"),
                 "rows_not_zeroed": ("cross", (200, 63, 33, 32, 3, "e"), "padding row")}


def test_every_fault_is_planted():
    assert sorted(PLANTED) == sorted(pr.FAULTS)
    for table, case, _ in list(PLANTED.values()) + list(PLANTED_EXACT.values()):
        assert case in (pr.FIT_CASES if table == "fit" else pr.CROSS_CASES)


def _run_planted(table, case, fault):
    if table == "fit":
        pb = pr.fit_problem(case)
        ref = pr.FitReference(pb, _planted_rows(pb))
        return _judge_fit(pb, ref, *_emulate_fit(pb, ref, fault))
    pb = pr.cross_problem(case)
    return _judge_cross(pb, *_emulate_cross(pb, fault))


@pytest.mark.parametrize("fault,planted", [(f, PLANTED[f]) for f in sorted(PLANTED)]
                         + [(f, PLANTED_EXACT[f]) for f in sorted(PLANTED_EXACT)], ids=str)
def test_planted_faults_are_caught(fault, planted):
    """gamma applied to coef0 cannot show on the lattice (gamma = 1): only a bound case notices it.  Rows past m
    left as computed show in no entry point -- every consumer multiplies them by zero rows, the downloads stop at
    m -- so only the emulation's padding row notices them; the GPU file cannot."""
    table, case, how = planted
    r_entry, r_prod, broken = _run_planted(table, case, fault)
    print("planted %s on %s %s: ratios %.3g (entries) %.3g (product), exact facts broken: %s"
          % (fault, table, case, r_entry, r_prod, broken))
    if how == "bound":
        assert max(r_entry, r_prod) > 1.0
    else:
        assert how in broken


def test_a_bound_relative_to_K_fails_where_b_cancels():
    """The gap this file closes, kept as evidence: at a planted pair of family (c) the correct emulation is off by
    more than tests/test_gpu_kernel_poly.py's ``_product_bound`` -- 4 (p + 2 d + n) u |K| -- allows for a single
    entry of K (a one-hot C K C'), although it is well inside the bound in A and b: that bound can only be run on
    data where nothing cancels."""
    case = (64, 4, 17, 2, "c")
    pb = pr.fit_problem(case)
    ref = pr.FitReference(pb, _planted_rows(pb))
    entries, _, _ = _emulate_fit(pb, ref)
    a, b = pb["zeros"][0]
    err = abs(LD(entries[a, b]) - ref.K[a, b])
    old = _product_bound(pb["p"], pb["degree"], pb["n"], max(abs(float(ref.K[a, b])), abs(entries[a, b])))
    print("entry (%d, %d) of %s: K %.3e, emulation %.3e, |difference| %.3e; bound relative to |K| %.3e, bound in A "
          "and b %.3e" % (a, b, case, float(ref.K[a, b]), entries[a, b], float(err), old, float(ref.e[a, b])))
    assert err > old and err <= ref.e[a, b]


def test_tables_cover_every_value():
    """Every n, p, k and degree the tables promise, both KP with more than one split, more than one tile per split
    in both launch shapes, every family, and the splits the cases are named for."""
    ns, ps, ks, ds, fams = (set(c[i] for c in pr.FIT_CASES) for i in range(5))
    assert {1, 63, 64, 65, 128, 129, 130, 900} <= ns and ns & {2100, 3500}
    assert ps == {1, 3, 4, 5, 31, 32, 33, 64, 65} and ks == {1, 16, 17, 32, 33, 64}
    assert ds == set(pr.DEGREES) and fams == set("abcde")
    assert pr.kv_splits(2100) == (17, 2) and pr.kv_splits(3500) == (19, 3) and 56 - 18 * 3 == 2
    assert [pr.kv_splits(n) for n in (1, 63, 64, 65, 128, 129, 130, 900)] == [(2, 1)] * 5 + [(4, 1)] * 2 + [(16, 1)]
    for kp in (32, 64):                                     # several splits, and several tiles per split, at both KP
        mine = [c for c in pr.FIT_CASES if (32 if c[2] <= 32 else 64) == kp]
        assert any(pr.kv_splits(c[0])[0] > 2 for c in mine) and any(pr.kv_splits(c[0])[1] > 1 for c in mine)
    assert all(c[0] > pr.RANDOM_FACTORS_UP_TO or c[3] <= 3 for c in pr.FIT_CASES if c[4] == "e")
    assert any(c[3] == 2 and c[4] == "e" and c[0] <= pr.RANDOM_FACTORS_UP_TO for c in pr.FIT_CASES)
    assert {(1, 1), (63, 64), (64, 65), (65, 129), (200, 63)} <= set(c[:2] for c in pr.CROSS_CASES)
    assert set(c[2] for c in pr.CROSS_CASES) == {1, 3, 4, 5, 33, 129}
    assert set(c[3] for c in pr.CROSS_CASES) == {1, 32, 33, 64}
    assert pr.cross_splits(1100, 3800) == (30, 2) and pr.cross_splits(65, 129) == (3, 1)
    assert any(pr.cross_splits(c[0], c[1])[1] > 1 for c in pr.CROSS_CASES)
    assert set(c[4] for c in pr.DISTANCE_CASES) == set("bce")
    assert set(c[3] for c in pr.FIT_CASES + pr.DISTANCE_CASES) | set(c[4] for c in pr.CROSS_CASES) == set(pr.DEGREES)
    assert pr.TRACE_CASES and set(c[4] for c in pr.TRACE_CASES) == set("bcd") and pr.DIAGONAL_CASES
