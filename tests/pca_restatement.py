"""DeviceData.pca restated in NumPy float64 on the stored values, and the bounds the device is held to.

The route is the device's (convex_dim_red/pca.py): the mean, the Gram matrix of the centred matrix over one side,
``numpy.linalg.eigh``, eigenvalues descending and clipped at 0; by columns the components are the eigenvectors,
by rows ``diag(lambda^-1/2) U' Xc`` evaluated as ``A X - (A 1) mean'``; every component oriented so that its entry
of largest magnitude is positive.  Nothing here imports the package.

Bounds, with u = 2^-53.  A float64 sum of K products in any order, fused or not, is within (K + 1) u sum|a||b| of
the exact one, and each centred operand carries the one rounding of its subtraction, so two evaluations of a Gram
entry differ by at most ``2 (K + 2) u (|Xc| |Xc|')`` (K the contraction length: p by rows, n by columns), and two
evaluations of a projection by ``2 (p + 2) u (|Xc| |V|')``, plus 2^-24 |value| (half a float32 ulp at the most) when
the result is stored in float32.  A symmetric perturbation B of the Gram matrix moves every eigenvalue by at most
||B||_F (Weyl) and the eigenvector of eigenvalue i by sin(angle) <= 2 ||B||_F / gap_i (Davis-Kahan in the form of
Yu, Wang and Samworth), gap_i the distance to the nearest other eigenvalue.
"""
import numpy as np

U = 2.0 ** -53
# Shapes at which csrc/gram_plan.h, at 256 compute units, cuts the contraction into several splits the last of
# which is short (few tile pairs over a long contraction); (n, p) per side.  tests/test_pca_host.py holds the header
# to that, tests/test_gpu_pca.py runs them:
#   rows 200 x 3001: 10 pairs, 94 chunks in 47 splits of 64 features, the last holds 57
#   rows  65 x 5000:  3 pairs, 157 chunks in 157 splits of 32 (one chunk each), the last holds 8
#   cols 5000 x 167:  6 pairs, 157 chunks in 79 splits of 64 rows, the last holds 8
#   cols 2500 x 257: 15 pairs, 79 chunks in 27 splits of 96 rows, the last holds 4
SPLIT_SHAPES = {"rows": [(200, 3001), (65, 5000)], "cols": [(5000, 167), (2500, 257)]}


class Model(object):
    """The attributes of ResidentPCA, host arrays."""


def low_rank(n, p, q):
    """The end-to-end input: rank q + 2 with singular values 10 0.8^i sqrt(n), noise 1e-2, even columns offset by
    up to 1e2, seed n + p."""
    rng = np.random.RandomState(n + p)
    r = q + 2
    left, _ = np.linalg.qr(rng.standard_normal((n, r)))
    right, _ = np.linalg.qr(rng.standard_normal((p, r)))
    X = (left * (10.0 * 0.8 ** np.arange(r) * np.sqrt(n))).dot(right.T) + 1e-2 * rng.standard_normal((n, p))
    offset = 1e2 * rng.uniform(-1.0, 1.0, size=p)
    offset[1::2] = 0.0
    return X + offset


def stored(X, dtype):
    return X.astype(np.float32).astype(np.float64) if np.dtype(dtype) == np.float32 else np.asarray(X, np.float64)


def centred(Xd, mean):
    return Xd if mean is None else Xd - mean


def gram(Xd, mean, side):
    Xc = centred(Xd, mean)
    return Xc.dot(Xc.T) if side == "rows" else Xc.T.dot(Xc)


def gram_bound(Xd, mean, side):
    A = np.abs(centred(Xd, mean))
    K = Xd.shape[1] if side == "rows" else Xd.shape[0]
    return 2 * (K + 2) * U * (A.dot(A.T) if side == "rows" else A.T.dot(A))


def project(Xd, mean, V):
    return centred(Xd, mean).dot(V.T)


def project_bound(Xd, mean, V, out_dtype=np.float64):
    value = project(Xd, mean, V)
    bound = 2 * (Xd.shape[1] + 2) * U * np.abs(centred(Xd, mean)).dot(np.abs(V).T)
    if np.dtype(out_dtype) == np.float32:
        bound = bound + 2.0 ** -24 * np.abs(value)
    return bound


def orient(components):
    components = np.array(components, dtype=np.float64)
    for row in components:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1.0
    return components


def fit(Xd, q, center=True, side="auto"):
    n, p = Xd.shape
    if side == "auto":
        side = "rows" if n <= p else "cols"
    mean = Xd.mean(axis=0) if center else None
    lam, vec = np.linalg.eigh(gram(Xd, mean, side))
    lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
    if side == "cols":
        components = vec[:, :q].T
    else:
        A = (vec[:, :q] / np.sqrt(lam[:q])).T
        components = A.dot(Xd) - (0.0 if mean is None else np.outer(A.sum(axis=1), mean))
    m = Model()
    m.components_ = orient(components)
    m.mean_ = np.zeros(p) if mean is None else mean
    m.eigenvalues_ = lam
    m.n_samples_, m.n_features_in_, m.side_ = n, p, side
    rest = lam[q:min(n, p)]
    m.explained_variance_ = lam[:q] / (n - 1)
    m.explained_variance_ratio_ = lam[:q] / lam.sum()
    m.singular_values_ = np.sqrt(lam[:q])
    m.noise_variance_ = rest.mean() / (n - 1) if rest.size else 0.0
    return m


def gaps(lam, q):
    """gap_i of the first q eigenvalues among all of ``lam`` (descending)."""
    padded = np.concatenate([[np.inf], lam, [-np.inf]])
    return np.minimum(padded[:q] - padded[1:q + 1], padded[1:q + 1] - padded[2:q + 2])


def perturbation_bounds(Xd, mean, side, lam, q):
    """(Weyl bound on the eigenvalues, Davis-Kahan bound on sin(angle) of each of the first q eigenvectors) for
    the Gram rounding error."""
    B = np.linalg.norm(gram_bound(Xd, mean, side))
    return B, 2.0 * B / gaps(lam, q)


def sines(a, b):
    """sin of the angle between the rows of ``a`` and the rows of ``b``."""
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    bn = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.linalg.norm(an - np.sum(an * bn, axis=1, keepdims=True) * bn, axis=1)

