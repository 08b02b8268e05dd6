"""Calendar-slot climatology and anomalies restated step by step in NumPy for the calendar tests (host and GPU), with
the rounding bounds they are judged by.  Not a test module.

The steps: a loop over the slots with ``X[idx].sum(0)`` over the rows ``idx`` that carry the slot's label (``-1``: not
counted); the means ``sum / count`` and the deviations ``sum (x - c)^2`` about a table ``c``; the smoothed climatology
``S @ mean`` with ``S = calendar_smoother(count > 0, H)`` and the rows of ``mean`` of empty slots set to 0; the
anomalies ``(X - clim[slot]) / scale[slot]``.

THE BOUNDS.  ``u = 2^-53``; a float64 sum of m terms in any order is within ``(m + 1) u sum|x|`` of the exact one
(higher orders of u dropped, one spare rounding).

* Sums.  The device and the restatement each add the ``m_g`` rows of slot g in an order of their own, so they differ
  by at most ``2 (m_g + 2) u sum_{t in g} |x|`` (``sum_bound``).  The squared deviations add one subtraction and one
  square, fused or not, per term: ``2 (m_g + 4) u sum (x - c)^2`` (``sqdev_bound``).  Both are taken on the STORED
  values (what a float32 block holds).  A slot without counted rows has no term: exactly 0.
* Statistics.  DESIGN 5.3: a mean over cnt rows is within ``b_mean = cnt u mean|x|`` of the exact one, and the
  variance about it within ``b_var = (cnt + 4) u var + b_mean^2`` (the first-order term of the mean's error cancels
  because the deviations from the mean add up to zero).  The device and ``np.mean`` / ``np.var`` are each within them.
* Smoothing.  ``S @ mean`` is a G-term sum per entry: the host product is within ``(G + 2) u (|S| @ |mean|)`` of the
  exact one, and an error ``e`` of the means passes through as ``|S| @ |e|``; so two evaluations with the same ``S``
  differ by at most ``|S| @ b_mean + (G + 2) u (|S| @ |mean|)`` (``smooth_bound``; empty slots: ``b_mean = 0``).
* ``calendar_smoother`` itself.  For a trigonometric polynomial m of order <= H sampled on the present slots,
  ``S m`` is m on all G slots.  ``S = B pinv(B[present])`` comes out of an SVD of a design matrix with a condition
  number of 1.41 - 1.43 at the cases tested, so its entries carry a few roundings of their own, and the product a
  G-term sum: within ``4 (G + 2) u (|S| @ |m|)`` (``SMOOTHER_FACTOR``; measured 0.002 - 0.25 of it at
  ``SMOOTHER_CASES``, 0.007 - 0.99 of ``(G + 2) u |S||m|``, the largest in the interpolating case
  ``2 H + 1 = G``).  ``S S = S`` on the present block is judged in the same measure with the magnitudes an entry
  of ``S`` is added up from, ``parts = |B| @ |pinv(B[present])| >= |S|``, in the place of ``|S|``: where an exact entry of ``S`` is 0 (the interpolating case, ``S = I``) the computed one is
  a rounding of its parts, not of itself, and ``S S - S`` is of that size: ``4 (G + 2) u (parts @ parts)``
  (``smoother_parts``).
* Standardised anomalies.  ``scale^2 = sum (x - clim)^2 / cnt`` over the slot's base rows, about the climatology that
  is subtracted (so no ``b_mean^2`` term): relative error ``(cnt + 4) u`` from the sum, the division, the root and its
  square.  A stored anomaly is ``(x - clim) / scale`` with two float64 roundings and one to the stored type ``u_T``
  (``2^-24`` for float32, ``u`` for float64), so its square is off by ``2 (u_T + 2 u)`` relative; NumPy's mean of the
  cnt squares adds ``(cnt + 2) u``.  The mean square of a used slot's anomalies over its base rows is therefore 1
  within ``rms_bound = 2 u_T + (2 cnt + 10) u``."""
import numpy as np

from convex_dim_red import calendar_smoother

U = 2.0 ** -53
SMOOTHER_FACTOR = 4.0
# (G, harmonics, missing slots): the cases of the smoother's host test
SMOOTHER_CASES = [(366, 4, 1), (1464, 3, 4), (12, 2, 0), (17, 8, 0), (5, 2, 0)]


def smoother_parts(present, harmonics):
    """``|B| @ |pinv(B[present])|`` on the present block: what the entries of ``S`` are added up from."""
    G = present.size
    theta = 2.0 * np.pi * np.arange(G) / G
    B = np.column_stack([np.ones(G)] + [f(h * theta) for h in range(1, harmonics + 1) for f in (np.cos, np.sin)])
    return np.abs(B[present]).dot(np.abs(np.linalg.pinv(B[present])))


def columns(rng, n, p):
    """``_columns`` of tests/test_gpu_anomalies.py: standard_normal * uniform(0.1, 5) + offset; even columns: offset
    1e4 * uniform(-1, 1), odd columns: 0."""
    offset = 1e4 * rng.uniform(-1.0, 1.0, size=p)
    offset[1::2] = 0.0
    return rng.standard_normal((n, p)) * rng.uniform(0.1, 5.0, size=p) + offset


def slot_sums(X, slots, G, centre=None):
    """(sums (G, p), counts (G,)): per slot the sum of its rows, or of their squared deviations from ``centre[g]``."""
    sums, counts = np.zeros((G, X.shape[1])), np.zeros(G, dtype=np.int64)
    for g in range(G):
        idx = np.flatnonzero(slots == g)
        counts[g] = idx.size
        if idx.size:
            sums[g] = X[idx].sum(0) if centre is None else ((X[idx] - centre[g]) ** 2).sum(0)
    return sums, counts


def slot_stats(X, slots, G, centre=None):
    """(mean, std, counts) per slot, NaN where a slot is empty; ``std`` about ``centre`` (None: the slot's mean)."""
    sums, counts = slot_sums(X, slots, G)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(counts[:, None] > 0, sums / counts[:, None], np.nan)
        sq, _ = slot_sums(X, slots, G, mean if centre is None else centre)
        std = np.sqrt(np.where(counts[:, None] > 0, sq / counts[:, None], np.nan))
    return mean, std, counts


def climatology(mean, counts, harmonics=None):
    """The slot means, or ``S @ mean`` with the rows of empty slots set to 0 first."""
    if harmonics is None:
        return mean
    return calendar_smoother(counts > 0, harmonics).dot(np.where(np.isnan(mean), 0.0, mean))


def anomalies(X, slots, clim, scale=None):
    out = X - clim[slots]
    return out if scale is None else out / scale[slots]


def sum_bound(X, slots, G):
    abs_sums, counts = slot_sums(np.abs(X), slots, G)
    return 2.0 * (counts[:, None] + 2) * U * abs_sums


def sqdev_bound(X, slots, G, centre):
    sq, counts = slot_sums(X, slots, G, centre)
    return 2.0 * (counts[:, None] + 4) * U * sq


def stat_bounds(X, slots, G):
    """(b_mean, b_var, var), each (G, p), zero where a slot is empty."""
    p = X.shape[1]
    b_mean, b_var, var = np.zeros((G, p)), np.zeros((G, p)), np.zeros((G, p))
    for g in range(G):
        sel = X[slots == g]
        if sel.shape[0]:
            cnt = sel.shape[0]
            var[g] = sel.var(axis=0)
            b_mean[g] = cnt * U * np.abs(sel).mean(axis=0)
            b_var[g] = (cnt + 4) * U * var[g] + b_mean[g] ** 2
    return b_mean, b_var, var


def smooth_bound(S, mean, b_mean):
    G = S.shape[0]
    return np.abs(S).dot(b_mean) + (G + 2) * U * np.abs(S).dot(np.abs(np.where(np.isnan(mean), 0.0, mean)))


def rms_bound(counts, dtype):
    u_t = 2.0 ** -24 if np.dtype(dtype) == np.float32 else U
    return 2.0 * u_t + (2.0 * counts + 10.0) * U
