"""The implicit RBF kernel K_rc = exp(-gamma |x_r - x_c|^2) restated for the RBF product tests (host and GPU): a
long-double reference, the rounding bound both are judged by, a NumPy emulation of the device arithmetic (host
test only), the input families, the launchers' split arithmetic and the tables of cases.  Not a test module.

THE REFERENCE.  ``reference`` sums the squared differences ``(y_rq - x_cq)^2`` in ``np.longdouble`` and takes
``exp`` there.  The kernels (k_rbf_kv, k_rbf_cross_mfma) instead expand ``d2 = |y_r|^2 + |x_c|^2 - 2 y_r.x_c``: a
different formula, so a mistake in one is not repeated in the other.  The squared dissimilarity of the distance
column is ``-2 expm1(-gamma s)``.

THE BOUND.  ``u = 2^-53``; a sum of p fma's in any order is within ``p u sum|a||b|`` of the exact one (higher
orders of u dropped).  Write ``M_rc = |y_r|^2 + |x_c|^2 + 2 sum_q |y_rq||x_cq|`` for the sum of the absolute
values of everything added up on the way to d2, before anything cancels.

* The three sums (two squared norms by k_rbf_norms, one dot product) are p fma's each: ``p u M``.  The two
  additions ``(|y|^2 + |x|^2) - 2 S`` round twice, each result at most M: ``2 u M``.  The clamp at 0 moves a
  computed d2 towards the true one (which is >= 0).  So ``|d2_dev - d2| <= (p + 2) u M``.
* ``gamma * d2`` rounds once: ``u gamma d2``.  The argument of exp is therefore off by at most
  ``u (gamma (p + 2) M + gamma d2)``, and an absolute error of the argument is a relative error of exp.
* exp itself and the rounding of its result: ``2 u`` relative.

Per entry ``E_rc = gamma (p + 2) M_rc + gamma d2_rc + 2`` and ``|K_dev - K| <= 2 u E_rc K_rc``.  The factor 2
covers the second-order terms, the reference's own long-double rounding and, in a product with factors on both
sides, the second n-term sum (see below); derived, not tuned.  For data far from the origin M grows with the
squared offset while d2 does not: the bound says how many digits the expansion loses there (family b).

UNDERFLOW.  A relative bound on exp holds where the result is a normal number.  From ``gamma d2 > 745.14`` the
correctly rounded float64 result is 0 while the long-double reference still holds 1e-324 and less, so every
entry bound carries the absolute term ``TINY = 2^-1074`` (one subnormal spacing).  Between the two, for
``gamma d2`` in [700, 746], results are subnormal and neither term describes them: ``guard`` asserts that no
pair of any input lies there.  Family (d) sits wholly above (K is the identity bit for bit).

PRODUCTS.  ``out = K V`` adds an n-term sum of fma's: ``|got - want| <= (2 u (E + n) o K + TINY) |V|``, element
by element (``o``: the entry-wise product).  With factors on both sides (``C K V`` through the Gram kernel) the
second sum over n adds ``n u |C| K |V|``; to first order the total is ``(E + 2 n) u <= (2 E + 2 n) u``, and the
second-order terms ``((E + 2 n) u)^2`` stay below the spare ``E u`` while ``(E + 2 n)^2 u <= E``, which holds
for every n and E here by ten orders of magnitude: the bound is ``|C| (2 u (E + n) o K + TINY) |V|``.  A one-hot
row of C makes both sums a sum of exact zeros and one term: ``C K Z`` is then the selected rows of ``K Z``, and an
entry of ``C K C'`` a single entry of K, held to the entry bound.

THE DISTANCE COLUMN (k_distance_rbf) sums the squared differences directly, 64 lanes and a butterfly.  With s the
long-double squared distance, ``e = exp(-gamma s)`` and ``t = 2 - 2 e``, squares are compared so that the square
root near 0 does not dictate the tolerance: ``|d_got^2 - t| <= 4 u (gamma s (p + 4) e + 2 e + 2 + t)`` -- the
sum (p + 2 roundings with the differences and the butterfly) and ``gamma s`` move the argument of exp, exp and
``2 - 2 e`` round, and squaring the rounded root adds ``2 u t``.

EXACT FACTS the tests pin.  (1) In k_rbf_kv the norms and the dot product of two equal rows are the same fma's
on the same numbers in the same order (feature by feature; the zero padding of a 16-chunk adds exact zeros), so
d2 is exactly 0 and K exactly 1.0 between duplicated rows, wherever in the tiles they sit.  (2) The clamp makes
every entry of K at most 1.0.  The bound above does not need the clamp -- without it an entry between two nearly
equal rows is 1 + (rounding of d2), inside the bound -- so fact (2), not the bound, is what notices a missing
clamp; family (c) therefore carries rows one ulp apart beside its exact duplicates.  (3) The diagonal is 1.0 by
the shortcut and the trace is n.  (4) On family (d) every off-diagonal exp underflows: K is the identity.

THE EMULATION (``emulate_product``; host test only) follows the device's order of operations in float64:
sequential norms, the dot product feature by feature in chunks of 16, the clamp, the diagonal shortcut, the
column tiles of 64 in their grid.y splits with ``if (c0 >= n) break``, k_sum_chunks' order.  NumPy has no fma,
so a product is rounded before it is added: twice the roundings the bound counts in the sums, still far inside
it (the largest ratio on any case is printed by the host test).  ``fault`` plants one mistake."""
import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
LD = np.longdouble


def round_up(a, b):
    return (a + b - 1) // b * b


# ---------------------------------------------------------------- the launchers' split arithmetic
def split_arithmetic(row_tiles, col_tiles):
    """(nsplit, tiles_per_split) of launch_kernel_product (the fit and the cross product): about 1024 blocks in all."""
    nsplit = (1024 + row_tiles - 1) // row_tiles
    nsplit = max(1, min(nsplit, col_tiles))
    tps = (col_tiles + nsplit - 1) // nsplit
    return (col_tiles + tps - 1) // tps, tps


def kv_splits(n):
    """kernel_kv: rows and columns are the n samples padded to 128 (n_pad), in tiles of 64."""
    tiles = round_up(n, 128) // 64
    return split_arithmetic(tiles, tiles)


def cross_splits(m, s):
    """kernel_cross: m resident rows padded to 128, s reference rows padded to 64."""
    return split_arithmetic(round_up(m, 128) // 64, round_up(s, 64) // 64)


def tiles_done(ncols, col_tiles, nsplit, tps, stop_at_padding):
    """Column tiles each split works through; k_rbf_kv leaves its loop at the first tile past the data."""
    done = []
    for q in range(nsplit):
        tiles = range(q * tps, min((q + 1) * tps, col_tiles))
        done.append(len([t for t in tiles if not (stop_at_padding and t * 64 >= ncols)]))
    return done


# ---------------------------------------------------------------- the reference and the bound
def reference(Y, X, gamma, rows=None):
    """(K, s) in long double for the rows ``rows`` of Y (None: all) against every row of X: s the squared
    distances summed from the differences, K = exp(-gamma s)."""
    Yl = np.asarray(Y, dtype=LD)
    Yl = Yl if rows is None else Yl[np.asarray(rows)]
    Xl = np.asarray(X, dtype=LD)
    s = np.zeros((Yl.shape[0], Xl.shape[0]), dtype=LD)
    for q in range(Xl.shape[1]):
        d = Yl[:, q][:, None] - Xl[:, q][None, :]
        s += d * d
    return np.exp(-LD(gamma) * s), s


def entry_E(Y, X, gamma, s, rows=None):
    """E_rc = gamma (p + 2) M_rc + gamma d2_rc + 2 (module docstring), long double."""
    Yl = np.abs(np.asarray(Y, dtype=LD))
    Yl = Yl if rows is None else Yl[np.asarray(rows)]
    Xl = np.abs(np.asarray(X, dtype=LD))
    p = Xl.shape[1]
    M = (Yl * Yl).sum(axis=1)[:, None] + (Xl * Xl).sum(axis=1)[None, :] + 2 * Yl.dot(Xl.T)
    return LD(gamma) * (p + 2) * M + LD(gamma) * s + 2


def entry_bound(K, E, n_terms=0):
    """2 u (E + n_terms) K + TINY per entry; n_terms = 0: an entry of K itself, n: a term of an n-term product."""
    return 2 * LD(U) * (E + n_terms) * K + LD(TINY)


def ratio(got, want, bound):
    """The largest |got - want| / bound, as a float; every bound here is positive."""
    return float((np.abs(np.asarray(got, dtype=LD) - want) / bound).max())


def distance_reference(X, gamma, j):
    """(t, bound) for the squared distance column of row j: t = -2 expm1(-gamma s), the bound of the docstring."""
    p = X.shape[1]
    _, s = reference(X, X[j:j + 1], gamma)
    s = s[:, 0]
    e = np.exp(-LD(gamma) * s)
    t = -2 * np.expm1(-LD(gamma) * s)
    return t, 4 * LD(U) * (LD(gamma) * s * (p + 4) * e + 2 * e + 2 + t)


def guard(Y, X, gamma):
    """No gamma d2 of any pair in [700, 746] (subnormal results; float64 is ample for a range test)."""
    Y, X = np.asarray(Y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    sx = (X * X).sum(axis=1)
    for r0 in range(0, Y.shape[0], 1024):
        y = Y[r0:r0 + 1024]
        g = gamma * ((y * y).sum(axis=1)[:, None] + sx[None, :] - 2 * y.dot(X.T))
        assert not np.any((g >= 700.0) & (g <= 746.0)), "an input pair with gamma d2 in [700, 746]"


# ---------------------------------------------------------------- the input families
def clusters(rng, n, p, k=5):
    """The clustered data of test_kernel_aa_on_the_implicit_rbf_kernel."""
    centers = rng.standard_normal((k, p)) * 2.0
    return centers[rng.randint(k, size=n)] + 0.4 * rng.standard_normal((n, p))


def stochastic(rng, shape):
    """Dense rows on the simplex, entries spread over three orders of magnitude."""
    A = rng.uniform(0.1, 1.0, size=shape) ** 3
    return A / A.sum(axis=1, keepdims=True)


def family(name, rng, n, p):
    """dict(X, gamma, twins, near): family a (centred clusters, gamma = 0.5 / p), b (a moved by 30 per
    feature), c (a with rows duplicated across tile boundaries -- ``twins`` -- and rows one ulp apart --
    ``near``), d (distinct integer lattice points, gamma = 800: K is the identity)."""
    out = dict(name=name, gamma=0.5 / p, twins=[], near=[])
    if name == "d":
        if p == 1:
            X = rng.permutation(n).astype(np.float64)[:, None] - n // 2
        else:
            X = np.unique(rng.randint(-9, 10, size=(4 * n, p)), axis=0)
            X = X[rng.permutation(X.shape[0])[:n]].astype(np.float64)
        assert X.shape == (n, p)
        out.update(X=X, gamma=800.0)
        return out
    X = clusters(rng, n, p)
    X = X - X.mean(axis=0)
    if name == "b":
        X = X + 30.0
    if name == "c":
        assert n >= 128
        out["twins"] = [(5, 70), (63, 64), (0, n - 1)]
        out["near"] = [(1, n - 2), (62, 65), (10, 100), (15, 16), (2, 120), (61, 66)]
        for a, b in out["twins"]:
            X[b] = X[a]
        for a, b in out["near"]:
            X[b] = np.nextafter(X[a], np.inf)
    out["X"] = X
    return out


def edge_rows(rng, n):
    """The rows the one-hot runs select: tile and split edges that exist, and 40 random ones."""
    edges = [0, 1, 15, 16, 62, 63, 64, 65, 127, 128, n - 66, n - 65, n - 64, n - 2, n - 1, 319, 320, 321]
    rows = sorted(set(r for r in edges if 0 <= r < n))
    return np.array(rows + list(rng.choice(n, size=min(40, n), replace=False)))


# ---------------------------------------------------------------- the cases of the GPU file
# K V through grams(): (n, p, k, family).  n: one sample; 63 / 64 / 65 and 128 / 129 / 130 around a column tile
# and around n_pad (64: the second split leaves at once; 130: four splits, the last one empty); 900: 16 splits of
# one tile; 4200: 14 splits of 5 tiles, the last a single tile (one-hot rows only).  p: 1, and 15 / 16 / 17 / 33
# around the 16-feature chunk.  k: 3 and 32 (KP = 32), 33 and 40 (KP = 64).  Every n and every p comes with both.
KV_CASES = [(1, 1, 1, "a"),
            (63, 15, 3, "a"), (63, 16, 40, "b"),
            (64, 16, 32, "a"), (64, 17, 33, "a"),
            (65, 17, 3, "b"), (65, 1, 40, "a"),
            (128, 33, 32, "a"), (128, 15, 40, "c"),
            (129, 1, 3, "d"), (129, 33, 33, "b"),
            (130, 17, 3, "c"), (130, 16, 40, "d"),
            (900, 17, 40, "a"), (900, 33, 3, "c"),
            (4200, 17, 3, "a"), (4200, 1, 40, "d"), (4200, 33, 33, "b")]
KV_RANDOM_FACTORS_UP_TO = 900


def kv_problem(case):
    n, p, k, name = case
    rng = np.random.RandomState(100000 + 1000 * p + 10 * n + k)
    pb = family(name, rng, n, p)
    guard(pb["X"], pb["X"], pb["gamma"])
    pb.update(n=n, p=p, k=k, C0=stochastic(rng, (k, n)), Z0=stochastic(rng, (n, k)), rows=edge_rows(rng, n))
    return pb


# aa_rbf_cross: (m, s, p, k).  m around a row tile, s around a column tile (129: three splits of one tile),
# p around the 4-feature MFMA step and the 32-feature chunk, k: 1 and 32 (KP = 32), 33 and 64 (KP = 64).  The
# last one: 256 row tiles give 4 splits at most, 5 column tiles then 3 splits of 2, 2 and 1 tiles.
CROSS_CASES = [(1, 1, 1, 1), (63, 64, 3, 32), (64, 65, 4, 33), (65, 129, 5, 64), (200, 129, 31, 1),
               (200, 64, 32, 33), (63, 1, 33, 32), (64, 129, 37, 64), (65, 65, 32, 1), (200, 65, 37, 32),
               (16300, 300, 5, 3)]


def cross_problem(case):
    """Reference rows XS from the clusters (centred), gamma = 0.5 / p, V uniform.  Y by thirds: copies of
    reference rows (d2 about 0), reference rows moved away so that gamma d2 is in the hundreds for every
    reference row, and fresh rows of the same clusters."""
    m, s, p, k = case
    rng = np.random.RandomState(200000 + 1000 * p + 10 * s + m + k)
    gamma = 0.5 / p
    XY = clusters(rng, s + m, p)
    XY = XY - XY.mean(axis=0)
    XS, Y = XY[:s], XY[s:].copy()
    kind = np.arange(m) % 3
    src = rng.randint(s, size=m)
    Y[kind == 0] = XS[src[kind == 0]]
    off = rng.standard_normal((m, p))
    off *= np.sqrt(rng.uniform(250.0, 350.0, size=m) / gamma)[:, None] / np.sqrt((off * off).sum(axis=1))[:, None]
    Y[kind == 1] = XS[src[kind == 1]] + off[kind == 1]
    guard(Y, XS, gamma)
    rows = None if m <= 200 else np.unique(np.concatenate([edge_rows(rng, m), rng.choice(m, 200, replace=False),
                                                           np.arange(m - 130, m)]))
    return dict(Y=Y, XS=XS, gamma=gamma, V=rng.uniform(size=(s, k)), rows=rows, m=m, s=s, p=p, k=k, kind=kind)


# aa_distance_column: (n, p, columns j).  p below, at and past the 64 lanes and past two rounds of them; n below, at
# and past the four rows of a block.  Row (j + 1) mod n is a copy of row j wherever n > 1.
DISTANCE_CASES = [(1, 1, (0,)), (3, 63, (0, 1, 2)), (4, 64, (0, 2, 3)), (5, 65, (0, 3, 4)), (130, 130, (0, 77, 129)),
                  (130, 1, (0, 64, 129)), (5, 130, (0, 2, 4)), (4, 1, (0, 1, 3))]


def distance_problem(case, j):
    n, p, _ = case
    rng = np.random.RandomState(300000 + 1000 * p + 10 * n + j)
    X = clusters(rng, n, p)
    X = X - X.mean(axis=0)
    if n > 1:
        X[(j + 1) % n] = X[j]
    return X, 0.5 / p


# resident features: the owner's dtype and p (p_pad = 128, 128, 256), n = 130, k = 3
RESIDENT_CASES = [(dtype, p) for dtype in ("float32", "float64") for p in (1, 127, 129)]
RESIDENT_N, RESIDENT_K = 130, 3


def resident_problem(case):
    """X as the owner stores it (rounded to float32 for a float32 owner), as float64."""
    dtype, p = case
    rng = np.random.RandomState(400000 + p + (dtype == "float32"))
    X = clusters(rng, RESIDENT_N, p)
    X = (X - X.mean(axis=0)).astype(dtype)
    Xs = X.astype(np.float64)
    gamma = 0.5 / p
    guard(Xs, Xs, gamma)
    return dict(X=X, Xs=Xs, gamma=gamma, n=RESIDENT_N, p=p, k=RESIDENT_K, C0=stochastic(rng, (RESIDENT_K, RESIDENT_N)),
                Z0=stochastic(rng, (RESIDENT_N, RESIDENT_K)), rows=edge_rows(rng, RESIDENT_N))


# ---------------------------------------------------------------- the emulation (host test only)
FAULTS = ("drop_last_feature", "skip_last_tile", "padding_tile_as_data", "neighbour_norm", "no_clamp",
          "diagonal_value", "diagonal_local", "sum_leaves_out_split")


def sequential_norms(F):
    """k_rbf_norms: s = x_q x_q + s, q ascending."""
    s = np.zeros(F.shape[0])
    for q in range(F.shape[1]):
        s = F[:, q] * F[:, q] + s
    return s


def emulate_product(Y, X, gamma, V, rows=None, same_set=True, fault=None):
    """(entries, out): the device's K for the rows ``rows`` of Y (None: all) against the rows of X, and its
    product with V, in the order of k_rbf_kv (``same_set``: Y is X -- padding to 128, the diagonal shortcut,
    the loop left at the first padding tile) or of k_rbf_cross_mfma (padding to 64, neither).  ``fault``: one
    of FAULTS --
      drop_last_feature     the last feature of a partial 16-chunk never enters the dot product;
      skip_last_tile        the first split leaves its loop one tile early;
      padding_tile_as_data  a tile past the data is not skipped and reads the 64 rows before it once more
                            (features and V; the zero rows of V that padding really holds would hide it);
      neighbour_norm        |x_c|^2 is read one column to the right;
      no_clamp              d2 is not clamped at 0;
      diagonal_value        the shortcut writes the double below 1;
      diagonal_local        the shortcut compares the indices inside the tile, not the global ones;
      sum_leaves_out_split  k_sum_chunks starts its loop at split 2."""
    assert fault is None or fault in FAULTS
    Y, X, V = (np.asarray(a, dtype=np.float64) for a in (Y, X, V))
    ncols, p = X.shape
    rows = np.arange(Y.shape[0]) if rows is None else np.asarray(rows)
    col_pad = round_up(ncols, 128 if same_set else 64)
    nsplit, tps = kv_splits(ncols) if same_set else cross_splits(Y.shape[0], ncols)
    Xp = np.zeros((col_pad + 1, p))
    Xp[:ncols] = X
    Vp = np.zeros((col_pad, V.shape[1]))
    Vp[:ncols] = V
    yr = Y[rows]
    ny, nx = sequential_norms(yr), sequential_norms(Xp)
    S = np.zeros((len(rows), col_pad))
    for q0 in range(0, p, 16):
        for q in range(q0, min(q0 + 16, p)):                # past p a chunk holds zeros: fma(0, 0, s) = s
            if fault == "drop_last_feature" and q == p - 1 and p % 16:
                continue
            S = yr[:, q][:, None] * Xp[:col_pad, q][None, :] + S
    nxc = nx[1:] if fault == "neighbour_norm" else nx[:col_pad]
    d2 = ny[:, None] + nxc[None, :] - 2.0 * S
    if fault != "no_clamp":
        d2 = np.maximum(d2, 0.0)
    E = np.exp(-gamma * d2)
    if same_set:
        here = np.arange(len(rows))
        if fault == "diagonal_local":
            E[(rows[:, None] % 64) == (np.arange(col_pad)[None, :] % 64)] = 1.0
        else:
            E[here, rows] = np.nextafter(1.0, 0.0) if fault == "diagonal_value" else 1.0
    partial = np.zeros((nsplit, len(rows), V.shape[1]))
    for q in range(nsplit):
        ct1 = min((q + 1) * tps, col_pad // 64)
        if fault == "skip_last_tile" and q == 0:
            ct1 -= 1
        for ct in range(q * tps, ct1):
            c0 = ct * 64
            if same_set and c0 >= ncols:
                if fault != "padding_tile_as_data":
                    break
                c0 -= 64
            for c in range(c0, c0 + 64):
                partial[q] = E[:, c][:, None] * Vp[c][None, :] + partial[q]
    out = partial[0].copy()
    for q in range(2 if fault == "sum_leaves_out_split" else 1, nsplit):
        out += partial[q]
    return E[:, :ncols], out


def emulate_distance(X, gamma, j):
    """k_distance_rbf: lane l sums the features l, l + 64, ...; the butterfly adds lanes 32, 16, ... apart."""
    X = np.asarray(X, dtype=np.float64)
    lanes = np.zeros((X.shape[0], 64))
    for q in range(X.shape[1]):
        df = X[:, q] - X[j, q]
        lanes[:, q % 64] = df * df + lanes[:, q % 64]
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return np.sqrt(np.maximum(2.0 - 2.0 * np.exp(-gamma * lanes[:, 0]), 0.0))
