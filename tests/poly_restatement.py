"""The implicit polynomial kernel K_rc = (gamma y_r.x_c + coef0)^degree restated for the polynomial product tests
(host and GPU): a long-double reference, the rounding bound both are judged by, a NumPy emulation of the device
arithmetic (host test only), the input families, and the tables of cases.  The launchers' split arithmetic, the
clusters, the stochastic factors, the edge rows and ``ratio`` are rbf_restatement's.  Not a test module.

THE REFERENCE.  ``reference`` sums the dot product feature by feature in ``np.longdouble``, forms
``b = gamma s + coef0`` there and takes the power with ``**``.  The device (poly_kappa) takes it by degree - 1
multiplications, so the two do not share a formula for the power.  Beside K it returns b and
``A_rc = sum_q |y_rq| |x_cq|``, the sum of the absolute values of everything added up on the way to the dot
product, before anything cancels.

THE BOUND is written in A and b, not in |K|: where ``gamma s + coef0`` cancels (coef0 = 0 on centred data, or a
pair with ``gamma y.x = -coef0``) an entry of K carries an error unrelated to its own size.  ``u = 2^-53``; a sum
of t fma's in any order is within ``t u sum|a||b|`` of the exact one (higher orders of u dropped).

* The dot product is t fma's -- the tile body runs p rounded up to 4 of them (the zero padding adds exact zeros),
  in whatever order the matrix cores take the four of a k-step: ``|s_dev - s| <= t u A``.
* ``b = fma(gamma, s_dev, coef0)`` rounds once, relative to the computed value, which is at most
  ``|b| + gamma t u A``: ``|b_dev - b| <= gamma t u A + u |b| + (second order)``.  With ``gamma A >= |gamma s|``
  one more ``gamma u A`` swallows that second-order term outright: ``delta = u (gamma (t + 1) A + |b|)``.
* With ``B = |b| + delta`` both b and b_dev lie in [-B, B], so ``|b_dev^d - b^d| <= d B^(d-1) delta`` (mean
  value), and the d - 1 multiplications round d - 1 times, each relative to a result of at most B^d:
  ``|K_dev - K| <= d B^(d-1) delta + (d - 1) u B^d``.  Degree 1: delta alone.

Per entry ``e_rc = 2 (d B^(d-1) delta + (d - 1) u B^d)``.  The factor 2 covers the terms of second order in u,
the reference's own long-double rounding (2^-64 relative on each of the same operations, a 2000th of u) and the
emulation's lack of fma -- NumPy rounds a product before it adds it, twice the roundings counted in the sums;
derived, not tuned against any output.  For data far from the origin A grows with the squared offset while b need
not: the bound says how many digits are lost (family d).

PRODUCTS.  ``out = K V`` adds an n-term sum of fma's (padding columns add ``coef0^d x 0``, exact zeros; the
grid.y splits and k_sum_chunks are one more way of ordering the same sum): a term of it is off by
``e + 2 n u |K|``, so ``|got - want| <= (e + 2 n u |K|) |V|`` element by element.  With factors on both sides
(``C K V`` through the Gram kernel) the second sum over n adds ``n u |C| |K| |V|``; to first order the total is
``|C| (e / 2 + 2 n u |K|) |V|``, and the spare ``e / 2`` keeps its meaning: the bound is
``|C| (e + 2 n u |K|) |V|``.  A one-hot row of C makes both sums a sum of exact zeros and one term: ``C K Z`` is
then the selected rows of ``K Z``, and an entry of ``C K C'`` a single entry of K, held to ``e`` alone.

THE DISTANCE COLUMN (k_distance_poly) sums x_i.x_i, x_i.x_j and x_j.x_j with lane l taking the features l,
l + 64, ... and a butterfly over the 64 lanes: ``t = ceil(p / 64) + 6`` roundings on any path to the sum, the
term count of the three entry bounds.  Squares are compared so that the square root near 0 does not dictate the
tolerance: with ``D2 = K_ii - 2 K_ij + K_jj`` from three reference values and
``T = |K_ii| + 2 |K_ij| + |K_jj|``, the two additions round a result of at most T each (2 u T) and squaring
the rounded root adds 2 u D2; doubled like the entries:
``|d_got^2 - D2| <= e_ii + 2 e_ij + e_jj + 4 u (T + D2)``.  The clamp at 0 moves a computed value towards the
true one (coef0 >= 0: K is positive semi-definite, D2 >= 0).  Where D2 is below its bound this says
``d_got^2 <= 2 x bound``, asserted in those words too.  For i = j, and for a copy of row j, the three sums are the
same fma's on the same numbers in the same order, so ``k - 2 k + k`` is exactly 0.

TRACE AND DIAGONAL.  k_rbf_norms sums ``|x_i|^2`` with p fma's, k_poly_trace and the AA_DIAG_POLY branch of
k_kernel_sample_residuals put it through poly_kappa: the entry bound with ``A = |x_i|^2`` and t = p; the sum of n
such values adds ``n u sum|K_ii|`` (its second order sits in the entries' factor 2).

THE LATTICE (family e) needs no bound: small-integer features, gamma = 1, integer coef0, factors whose entries
are multiples of 2^-6.  Every dot product, every power and every partial sum of a product, in any order, is
then an integer multiple of 2^-6 (2^-12 with factors on both sides) that float64 holds exactly -- ``lattice_exact``
asserts so with Python integers, three bits to spare below 2^53 -- and the device result equals the integer
result bit for bit.  That pins every index, tile, split and k_sum_chunks with no tolerance at all.

THE EMULATION (``emulate_product``; host test only) follows the device's order in float64: the dot product in
32-feature chunks of 4-feature k-steps up to p rounded up to 4, poly_kappa's multiplication order, the 64-column
tiles in their grid.y splits -- every tile, the ones that lie wholly in the padding too: the tile body has no
``break`` like k_rbf_kv's --, the columns of a tile in ascending order (k-step (mt, q) contracts the columns
16 mt + 4 q + 0..3), k_sum_chunks' order.  ``fault`` plants one mistake (FAULTS)."""
import numpy as np

from rbf_restatement import (LD, U, clusters, cross_splits, edge_rows, kv_splits, ratio, round_up,  # noqa: F401
                             split_arithmetic, stochastic)

DEGREES = (1, 2, 3, 5, 8)
RANDOM_FACTORS_UP_TO = 900
LATTICE_BITS = 50                       # what lattice_exact allows the largest sum of absolute values, of 53


# ---------------------------------------------------------------- the reference and the bound
def reference(Y, X, gamma, coef0, degree, rows=None):
    """(K, b, A) in long double for the rows ``rows`` of Y (None: all) against every row of X."""
    Yl = np.asarray(Y, dtype=LD)
    Yl = Yl if rows is None else Yl[np.asarray(rows)]
    Xl = np.asarray(X, dtype=LD)
    s = np.zeros((Yl.shape[0], Xl.shape[0]), dtype=LD)
    A = np.zeros_like(s)
    for q in range(Xl.shape[1]):
        t = Yl[:, q][:, None] * Xl[:, q][None, :]
        s += t
        A += np.abs(t)
    b = LD(gamma) * s + LD(coef0)
    return b ** int(degree), b, A


def entry_bound(b, A, gamma, degree, terms):
    """e = 2 (d B^(d-1) delta + (d - 1) u B^d), delta = u (gamma (terms + 1) A + |b|), B = |b| + delta."""
    u = LD(U)
    delta = u * (LD(gamma) * (terms + 1) * A + np.abs(b))
    B = np.abs(b) + delta
    e = 2 * (degree * B ** (degree - 1) * delta + (degree - 1) * u * B ** degree)
    assert np.all(e > 0), "an all-zero pair with coef0 = 0: nothing to round, no bound to divide by"
    return e


def term_bound(e, K, n_terms):
    """e + 2 n u |K|: a term of an n-term product."""
    return e + 2 * n_terms * LD(U) * np.abs(K)


def diagonal_reference(X, gamma, coef0, degree):
    """(K_ii, e_ii) from the long-double squared norms, t = p (k_rbf_norms)."""
    Xl = np.asarray(X, dtype=LD)
    s = (Xl * Xl).sum(axis=1)
    b = LD(gamma) * s + LD(coef0)
    return b ** int(degree), entry_bound(b, s, gamma, degree, Xl.shape[1])


def trace_reference(X, gamma, coef0, degree):
    """(trace, bound): the sum of the diagonal and sum e_ii + n u sum|K_ii|."""
    K, e = diagonal_reference(X, gamma, coef0, degree)
    return K.sum(), e.sum() + K.shape[0] * LD(U) * np.abs(K).sum()


def distance_reference(X, j, gamma, coef0, degree):
    """(D2, bound) of the squared distance column of row j (module docstring)."""
    Xl = np.asarray(X, dtype=LD)
    terms = -(-Xl.shape[1] // 64) + 6
    Kij, bij, Aij = reference(X, X[j:j + 1], gamma, coef0, degree)
    Kij, bij, Aij = Kij[:, 0], bij[:, 0], Aij[:, 0]
    sii = (Xl * Xl).sum(axis=1)
    bii = LD(gamma) * sii + LD(coef0)
    Kii = bii ** int(degree)
    eii = entry_bound(bii, sii, gamma, degree, terms)
    D2 = Kii - 2 * Kij + Kii[j]
    T = np.abs(Kii) + 2 * np.abs(Kij) + np.abs(Kii[j])
    return D2, eii + 2 * entry_bound(bij, Aij, gamma, degree, terms) + eii[j] + 4 * LD(U) * (T + np.abs(D2))


# ---------------------------------------------------------------- the input families
def family(name, rng, n, p, degree):
    """dict(name, X, gamma, coef0):
      a  the benign clusters of tests/test_gpu_kernel_poly.py: gamma = 1 / p, gamma |x|^2 <= 1, coef0 = 1;
      b  centred clusters, gamma = 0.25 / p, coef0 = 0, odd degree: K of both signs, b cancels freely;
      c  centred clusters, gamma = 0.5 / p, coef0 one of 0.25, 0.5, 1; ``plant`` adds the pairs;
      d  centred clusters moved by 30 per feature, every other row negated, gamma = 1 / (900 p), coef0 = 1:
         between a row and a negated one gamma y.x is about -1 and b what is left of 1 - 1, gamma A about 1;
      e  the lattice: integer features in [-3, 3], gamma = 1, coef0 = 2."""
    out = dict(name=name, coef0=1.0)
    if name == "e":
        out.update(X=rng.randint(-3, 4, size=(n, p)).astype(np.float64), gamma=1.0, coef0=2.0)
        return out
    X = clusters(rng, n, p)
    if name == "a":
        gamma = 1.0 / p
        X = X / np.sqrt(gamma * (X * X).sum(axis=1).max()) * (1.0 - 1e-12)
    else:
        assert n > 1
        X = X - X.mean(axis=0)
        if name == "b":
            assert degree % 2 == 1
            gamma = 0.25 / p
            out["coef0"] = 0.0
        elif name == "c":
            gamma = 0.5 / p
            out["coef0"] = float(rng.choice([0.25, 0.5, 1.0]))
        else:
            assert name == "d"
            X = X + 30.0
            X[1::2] *= -1.0
            gamma = 1.0 / (900.0 * p)
    out.update(X=X, gamma=gamma)
    return out


def plant(X, gamma, coef0, zeros, near):
    """In place: for (a, b) in ``zeros`` row b becomes ``-x_a coef0 / (gamma |x_a|^2)``, so that
    gamma x_a.x_b + coef0 is 0 to rounding; for (a, b) in ``near`` row b becomes x_a moved up by one ulp."""
    for a, b in zeros:
        X[b] = -X[a] * (coef0 / (gamma * (X[a] * X[a]).sum()))
    for a, b in near:
        X[b] = np.nextafter(X[a], np.inf)


def usable_pairs(candidates, n, used=()):
    """The candidates (source, target) inside n rows that touch no row an earlier pair (or ``used``) touched."""
    used, out = set(used), []
    for a, b in candidates:
        if 0 <= a < n and 0 <= b < n and a != b and a not in used and b not in used:
            out.append((a, b))
            used.update((a, b))
    return out


def from_end(pairs, n):
    """Negative row numbers count from the last row."""
    return [(a, b if b >= 0 else n + b) for a, b in pairs]


def lattice_factor(rng, shape):
    """Rows of multiples of 2^-6 that sum to 1."""
    return rng.multinomial(64, np.ones(shape[1]) / shape[1], size=shape[0]) / 64.0


def lattice_exact(Y, X, coef0, degree, V, C=None, rows=None):
    """The integer results on the lattice (gamma = 1), as float64: dict(K, KV[, CKV]) for the rows ``rows`` of Y.
    Asserts with Python integers that every partial sum of the dot products, of the powers, of K V in units of
    2^-6 and of C K V in units of 2^-12, in any order, stays below 2^LATTICE_BITS: the sums of the absolute values
    do.  Returns the bits needed beside the results."""
    Y = np.asarray(Y)[np.arange(len(Y)) if rows is None else np.asarray(rows)]
    Yi, Xi = np.rint(Y).astype(np.int64), np.rint(X).astype(np.int64)
    assert np.array_equal(Yi, Y) and np.array_equal(Xi, X) and float(coef0) == int(coef0)
    Vn = np.rint(np.asarray(V) * 64.0).astype(np.int64)
    assert np.array_equal(Vn / 64.0, V)
    dot_bits = int((np.abs(Yi).dot(np.abs(Xi).T)).max() + int(coef0)).bit_length()
    b = Yi.dot(Xi.T) + int(coef0)
    entry_bits = (int(np.abs(b).max()) ** int(degree)).bit_length()
    assert dot_bits <= LATTICE_BITS and entry_bits <= LATTICE_BITS, (dot_bits, entry_bits)
    K = b ** int(degree)                                   # int64, exact: below 2^50 by the line above
    # int64 sums of at most n terms below 2^50 x 2^6 could wrap: a float64 estimate rules that out first
    assert np.abs(K).astype(np.float64).dot(np.abs(Vn).astype(np.float64)).max() < 2.0 ** 60
    product_bits = int(np.abs(K).dot(np.abs(Vn)).max()).bit_length()
    assert product_bits <= LATTICE_BITS, product_bits
    out = dict(K=K.astype(np.float64), KV=K.dot(Vn) / 64.0, bits=dict(entry=entry_bits, product=product_bits))
    if C is not None:
        Cn = np.rint(np.asarray(C) * 64.0).astype(np.int64)
        assert np.array_equal(Cn / 64.0, C) and rows is None
        two_bits = int(np.abs(Cn).dot(np.abs(K).dot(np.abs(Vn))).max()).bit_length()
        assert two_bits <= LATTICE_BITS, two_bits
        out.update(CKV=Cn.dot(K.dot(Vn)) / 4096.0)
        out["bits"]["two_sided"] = two_bits
    return out


# ---------------------------------------------------------------- the cases of the GPU file
# The fit, K V through set_poly_features / set_state / prepare / grams: (n, p, k, degree, family), what each is for.
# kv_splits: n <= 128 two splits of one tile (n <= 64: the second one wholly padding), 129 / 130 four (the last
# wholly padding), 900 sixteen of one tile, 2100 seventeen of 2 tiles, 3500 nineteen of 3 tiles, the last of 2.
FIT_CASES = [
    (1, 1, 1, 1, "a"),          # one sample, one feature (pk = 4 > p), one component; the loop of poly_kappa never runs
    (63, 3, 16, 3, "b"),        # a partial row tile and a padding tile; p < one k-step; a full 16-component tile
    (63, 64, 33, 8, "a"),       # two exact 32-feature chunks; KP = 64; seven multiplications
    (64, 4, 17, 2, "c"),        # one exact tile beside a tile of padding only; p = one k-step; b = 0 planted
    (64, 65, 32, 3, "e"),       # lattice; a third chunk of one feature (feat_ld = 96); KP = 32 full
    (65, 5, 32, 5, "b"),        # one row past the tile: both splits hold data; p one past a k-step
    (65, 31, 64, 2, "d"),       # p one short of the chunk (feat_ld = 32); KP = 64 full; digits lost to the offset
    (128, 32, 1, 8, "c"),       # n = n_pad, no padding at all; p = the chunk = feat_ld; one component
    (128, 33, 33, 1, "b"),      # one feature into the second chunk; KP = 64 by one; degree 1, K = gamma x.y
    (129, 1, 17, 3, "c"),       # one row into the third tile, a fourth tile of padding; p = 1 with b = 0 planted
    (129, 64, 64, 2, "e"),      # lattice with factors on both sides (degree 2), KP = 64 full
    (130, 31, 16, 5, "d"),      # the existing tests' smallest n, at p = 31
    (130, 3, 33, 3, "e"),       # lattice at p = 3, KP = 64
    (900, 65, 64, 2, "e"),      # lattice, 16 splits of one tile, factors on both sides
    (900, 5, 17, 8, "c"),       # 16 splits at KP = 32, degree 8 with b = 0 planted
    (900, 32, 32, 1, "d"),      # degree 1 on the offset data
    (2100, 65, 17, 3, "e"),     # lattice, 17 splits of 2 tiles at KP = 32 (one-hot rows only)
    (3500, 33, 33, 5, "b"),     # 19 splits of 3 tiles, the last of 2, at KP = 64 (one-hot rows only)
]
FIT_ZEROS = [(0, -1), (5, 70), (63, 64), (127, 128)]        # -1: the last row
FIT_NEAR = [(1, -2), (62, 65), (15, 16)]


def fit_problem(case):
    """dict(X, gamma, coef0, degree, n, p, k, C0, Z0, rows, zeros, near): family (c) carries the planted pairs that
    exist at this n, across tile edges; the lattice carries lattice factors."""
    n, p, k, degree, name = case
    rng = np.random.RandomState(500000 + 1000 * p + 10 * n + k)
    pb = family(name, rng, n, p, degree)
    pb.update(n=n, p=p, k=k, degree=degree, zeros=[], near=[])
    if name == "c":
        pb["zeros"] = usable_pairs(from_end(FIT_ZEROS, n), n)
        pb["near"] = usable_pairs(from_end(FIT_NEAR, n), n, [r for pair in pb["zeros"] for r in pair])
        plant(pb["X"], pb["gamma"], pb["coef0"], pb["zeros"], pb["near"])
    factor = lattice_factor if name == "e" else stochastic
    pb.update(C0=factor(rng, (k, n)), Z0=factor(rng, (n, k)), rows=edge_rows(rng, n))
    return pb


class FitReference(object):
    """K, its entry bound e and the bound of a term of an n-term product for the rows asked for (all rows up to
    n = 900), indexed by row number; on the lattice ``exact`` holds the integer results of the same rows."""

    def __init__(self, pb, extra_rows=()):
        n, X = pb["n"], pb["X"]
        rows = np.concatenate([pb["rows"], np.asarray(extra_rows, dtype=np.int64).ravel()])
        self.rows = np.arange(n) if n <= RANDOM_FACTORS_UP_TO else np.unique(rows)
        self.at = np.full(n, -1)
        self.at[self.rows] = np.arange(len(self.rows))
        self.K, b, A = reference(X, X, pb["gamma"], pb["coef0"], pb["degree"], self.rows)
        self.e = entry_bound(b, A, pb["gamma"], pb["degree"], round_up(pb["p"], 4))
        self.en = term_bound(self.e, self.K, n)
        self.exact = None
        if pb["name"] == "e":
            dense = n <= RANDOM_FACTORS_UP_TO
            self.exact = lattice_exact(X, X, pb["coef0"], pb["degree"], pb["Z0"], pb["C0"] if dense else None,
                                       None if dense else self.rows)
            if dense:
                self.exact["CKCt"] = lattice_exact(X, X, pb["coef0"], pb["degree"], pb["C0"].T, pb["C0"])["CKV"]

    def take(self, sel):
        assert np.all(self.at[sel] >= 0)
        return self.at[sel]


# The cross product, set_poly_reference / poly_cross: (m, s, p, k, degree, family).  cross_splits: one tile per
# split up to s = 129; (1100, 3800): 18 row tiles, 60 column tiles, 30 splits of 2 tiles.
CROSS_CASES = [
    (1, 1, 1, 1, 2, "a"),           # one row against one reference row
    (63, 64, 3, 32, 3, "b"),        # s = one exact tile, no padding column at all; p < one k-step
    (64, 65, 4, 33, 8, "c"),        # one reference row into the second tile (two splits); b = 0 planted
    (65, 129, 5, 64, 5, "d"),       # three splits of one tile, KP = 64 full
    (200, 63, 33, 32, 3, "e"),      # lattice; four row tiles, the last partial; one padding column
    (65, 129, 129, 33, 1, "b"),     # p_pad = 256, five chunks, the last of one feature
    (200, 63, 129, 64, 2, "e"),     # lattice at p = 129
    (1100, 3800, 5, 33, 3, "e"),    # lattice, 30 splits of 2 tiles, every row compared
    (1100, 3800, 4, 1, 5, "c"),     # the same launch within the bound, b = 0 planted, one component
]
CROSS_TWINS = [(1, -2), (5, 70), (62, 65)]                  # rows of Y that are copies: (source, copy)


def cross_problem(case):
    """Reference rows XS and new rows Y of one family; family (c): Y rows 0, m - 1 (and 64) are the zero partners
    of reference rows 0, s - 1 (and 63).  ``twins``: duplicated rows of Y.  V uniform, on the lattice multiples of
    2^-6.  ``rows``: the rows referenced (None: all)."""
    m, s, p, k, degree, name = case
    rng = np.random.RandomState(600000 + 1000 * p + 10 * s + m + k)
    pb = family(name, rng, s + m, p, degree)
    XY = pb.pop("X")
    pb.update(m=m, s=s, p=p, k=k, degree=degree, zeros=[])
    if name == "c":
        pb["zeros"] = usable_pairs([(0, s), (s - 1, s + m - 1), (63, s + 64)], s + m)
        plant(XY, pb["gamma"], pb["coef0"], pb["zeros"], [])
    XS, Y = XY[:s].copy(), XY[s:].copy()
    pb["twins"] = usable_pairs(from_end(CROSS_TWINS, m), m, [b - s for _, b in pb["zeros"]])
    for a, b in pb["twins"]:
        Y[b] = Y[a]
    V = rng.randint(0, 65, size=(s, k)) / 64.0 if name == "e" else rng.uniform(size=(s, k))
    rows = None
    if m > 200 and name != "e":
        rows = np.unique(np.concatenate([edge_rows(rng, m), rng.choice(m, 200, replace=False),
                                         np.arange(m - 130, m)]))
    pb.update(XS=XS, Y=Y, V=V, rows=rows)
    return pb


# aa_distance_column: (n, p, columns j, degree, family), the shapes of rbf_restatement.DISTANCE_CASES: p below, at
# and past the 64 lanes and past two rounds of them; n below, at and past the four rows of a block.  Row
# (j + 1) mod n is a copy of row j wherever n > 1; family (c): row j + 2 is j's zero partner and row j + 3 one
# ulp from j where n has them.
DISTANCE_CASES = [(1, 1, (0,), 2, "e"), (3, 63, (0, 1, 2), 3, "b"), (4, 64, (0, 2, 3), 2, "c"),
                  (5, 65, (0, 3, 4), 3, "e"), (130, 130, (0, 77, 129), 5, "b"), (130, 1, (0, 64, 129), 8, "c"),
                  (5, 130, (0, 2, 4), 1, "c"), (4, 1, (0, 1, 3), 1, "b")]


def distance_problem(case, j):
    n, p, _, degree, name = case
    rng = np.random.RandomState(700000 + 1000 * p + 10 * n + j)
    pb = family(name, rng, n, p, degree)
    X = pb["X"]
    if name == "c":
        plant(X, pb["gamma"], pb["coef0"], [(j, (j + 2) % n)] if n >= 3 else [], [(j, (j + 3) % n)] if n >= 4 else [])
    if n > 1:
        X[(j + 1) % n] = X[j]
    return pb


# resident features: the owner's dtype and p (p_pad = 128, 128, 256), n = 130, k = 3, family (b), degree 3
RESIDENT_CASES = [(dtype, p) for dtype in ("float32", "float64") for p in (1, 127, 129)]
RESIDENT_N, RESIDENT_K, RESIDENT_DEGREE = 130, 3, 3


def resident_problem(case):
    """A fit problem whose X holds the values the owner stores (rounded to float32 for a float32 owner), as
    float64; ``owner_X`` is the array in the owner's dtype."""
    dtype, p = case
    n, k, degree = RESIDENT_N, RESIDENT_K, RESIDENT_DEGREE
    rng = np.random.RandomState(800000 + p + (dtype == "float32"))
    pb = family("b", rng, n, p, degree)
    owner_X = pb["X"].astype(dtype)
    pb.update(X=owner_X.astype(np.float64), owner_X=owner_X, n=n, p=p, k=k, degree=degree, zeros=[], near=[],
              C0=stochastic(rng, (k, n)), Z0=stochastic(rng, (n, k)), rows=edge_rows(rng, n))
    return pb


# the trace and the AA_DIAG_POLY diagonal: the fit cases of families (b) to (d), and the cross cases of family (c)
TRACE_CASES = [case for case in FIT_CASES if case[4] in "bcd"]
DIAGONAL_CASES = [case for case in CROSS_CASES if case[5] == "c"]


# ---------------------------------------------------------------- the emulation (host test only)
FAULTS = ("drop_last_kstep", "padding_column_counted", "skip_last_tile", "sum_leaves_out_split",
          "degree_off_by_one", "coef0_after_power", "gamma_on_coef0", "component_tile_to_neighbour",
          "rows_not_zeroed")


def kappa(S, gamma, coef0, degree, fault=None):
    """poly_kappa in float64: b = gamma s + coef0 (two roundings where the device's fma has one), v = b, then
    degree - 1 times v = v * b."""
    if fault == "gamma_on_coef0":
        b = gamma * (S + coef0)
    elif fault == "coef0_after_power":
        b = gamma * S
    else:
        b = gamma * S + coef0
    v = b.copy()
    for _ in range(degree - (0 if fault == "degree_off_by_one" else 1)):
        v = v * b
    return v + coef0 if fault == "coef0_after_power" else v


def emulate_product(Y, X, gamma, coef0, degree, V, rows=None, same_set=True, fault=None):
    """(entries, out, padding_row): the device's K for the rows ``rows`` of Y (None: all) against the rows of X,
    its product with V, and the output row the kernel leaves for the first row past m, in the order of
    k_poly_kv_mfma as the fit launches it (``same_set``: Y is X, columns padded to 128) or as the cross product
    does (columns padded to 64).  ``fault``: one of FAULTS --
      drop_last_kstep             the last 4-feature k-step of the last chunk never runs;
      padding_column_counted      the first padding column carries the V row before it, not zeros;
      skip_last_tile              the first split leaves its loop one tile early;
      sum_leaves_out_split        k_sum_chunks starts its loop at split 2;
      degree_off_by_one           poly_kappa multiplies once too often;
      coef0_after_power           (gamma s)^degree + coef0;
      gamma_on_coef0              gamma (s + coef0);
      component_tile_to_neighbour the output components 16..31 are written where 0..15 belong, their own place
                                  left empty;
      rows_not_zeroed             rows >= m are written as computed (coef0^degree times the column sums of V)."""
    assert fault is None or fault in FAULTS
    Y, X, V = (np.asarray(a, dtype=np.float64) for a in (Y, X, V))
    ncols, p = X.shape
    m, k = Y.shape[0], V.shape[1]
    rows = np.arange(m) if rows is None else np.asarray(rows)
    col_pad = round_up(ncols, 128 if same_set else 64)
    nsplit, tps = kv_splits(ncols) if same_set else cross_splits(m, ncols)
    KP = 32 if k <= 32 else 64
    pk = round_up(p, 4)
    Xp = np.zeros((col_pad, pk))
    Xp[:ncols, :p] = X
    Vp = np.zeros((col_pad, KP))
    Vp[:ncols, :k] = V
    if fault == "padding_column_counted" and ncols < col_pad:
        Vp[ncols] = Vp[ncols - 1]
    yr = np.zeros((len(rows) + 1, pk))                      # the last one: a padding row of Y
    yr[:-1, :p] = Y[rows]
    S = np.zeros((len(rows) + 1, col_pad))
    for q0 in range(0, pk, 32):
        for step in range(8):
            if q0 + 4 * step >= pk:
                break
            if fault == "drop_last_kstep" and q0 + 4 * step == pk - 4:
                continue
            for q in range(q0 + 4 * step, q0 + 4 * step + 4):
                S = yr[:, q][:, None] * Xp[:, q][None, :] + S
    E = kappa(S, gamma, coef0, degree, fault)
    partial = np.zeros((nsplit, len(rows) + 1, KP))
    for q in range(nsplit):
        ct1 = min((q + 1) * tps, col_pad // 64)
        if fault == "skip_last_tile" and q == 0:
            ct1 -= 1
        for c in range(q * tps * 64, ct1 * 64):             # padding tiles and all
            partial[q] = E[:, c][:, None] * Vp[c][None, :] + partial[q]
    out = partial[0].copy()
    for q in range(2 if fault == "sum_leaves_out_split" else 1, nsplit):
        out += partial[q]
    if fault == "component_tile_to_neighbour":
        out[:, :16] = out[:, 16:32]
        out[:, 16:32] = 0.0
    padding_row = out[-1, :k] if fault == "rows_not_zeroed" else np.zeros(k)
    return E[:-1, :ncols], out[:-1, :k], padding_row


def sequential_norms(F):
    """k_rbf_norms: s = x_q x_q + s, q ascending."""
    s = np.zeros(F.shape[0])
    for q in range(F.shape[1]):
        s = F[:, q] * F[:, q] + s
    return s


def emulate_diagonal(X, gamma, coef0, degree):
    """poly_kappa of k_rbf_norms' squared norms: the values k_poly_trace adds and AA_DIAG_POLY writes."""
    return kappa(sequential_norms(np.asarray(X, dtype=np.float64)), gamma, coef0, degree)


def emulate_trace(X, gamma, coef0, degree):
    """k_poly_trace: thread t adds the rows t, t + 256, ..., then the tree over the 256 threads."""
    d = emulate_diagonal(X, gamma, coef0, degree)
    part = np.zeros(256)
    for r0 in range(0, len(d), 256):
        chunk = d[r0:r0 + 256]
        part[:len(chunk)] += chunk
    w = 128
    while w:
        part[:w] += part[w:2 * w]
        w >>= 1
    return part[0]


def emulate_distance(X, j, gamma, coef0, degree):
    """k_distance_poly: lane l sums the features l, l + 64, ... of the three dot products; the butterfly adds
    lanes 32, 16, ... apart."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    lanes = np.zeros((3, n, 64))
    for q in range(X.shape[1]):
        a, b = X[:, q], X[j, q]
        for i, t in enumerate((a * a, a * b, np.full(n, b * b))):
            lanes[i][:, q % 64] = t + lanes[i][:, q % 64]
    o = 32
    while o:
        lanes = lanes + lanes[:, :, np.arange(64) ^ o]
        o >>= 1
    kii, kij, kjj = (kappa(lanes[i][:, 0], gamma, coef0, degree) for i in range(3))
    return np.sqrt(np.maximum(kii - 2.0 * kij + kjj, 0.0))
