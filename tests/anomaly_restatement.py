"""The monthly-anomaly calculation of the reference notebook ``hadisst_sst_anom.ipynb``, restated step by step in
NumPy for the anomaly tests (host and GPU), with the rounding bound both are judged by.  Not a test module.

The steps, per column ``x`` of ``n`` equally spaced rows: the centred moving average ``m`` (window ``[1/2, 1, ...,
1, 1/2] / P`` for an even period ``P``, ``ones(P) / P`` for an odd one; NaN where the window does not fit); the
means of ``x - m`` per phase ``t mod P`` over the base rows, NaN skipped; the cycle = those means minus their mean;
``y = x - cycle[t mod P]``; ``scipy.stats.linregress(arange(n), y)``.

THE BOUND.  ``u = 2^-53``; a sum of k products in any order is within ``k u sum|a||b|`` of the exact one (higher
orders of u dropped).  Write ``parts`` for ``seasonal_coefficients(...)[1] @ |X|``: the sum of the absolute values
of everything that is added up on the way to a value, before anything cancels.

* The restatement.  A window sum is w <= 15 products (+1: the weights are rounded quotients), ``x - m`` one
  rounding, a phase mean a sum of cnt <= n terms and a division, the mean over the phases P <= 14 terms and a
  division, its subtraction one rounding: the cycle is within ``(w + cnt + P + 5) u parts``.  ``y`` adds one
  rounding.  linregress centres (``np.cov``): ``slope = sum (t - tm)(y - ym) / sum (t - tm)^2`` with ``tm`` exact
  (half an integer), so an error of ``ym`` cancels to first order (``sum (t - tm) = 0``), and what remains is the
  rounding of ``y - ym``, of the n-term dot product, of the n-term sum of squares and of two divisions:
  ``(2 n + 5) u |s|'|y - ym|`` with ``s`` the regression weights.  ``|y - ym| <= |y| + mean|y|``, and
  ``sum|s| mean|y| <= KAPPA |s|'|y|`` holds for the columns used here with ``KAPPA = 2`` (``model_bound`` asserts
  it: the magnitude of every column is spread evenly enough over the rows), so the slope is within
  ``(1 + KAPPA)(2 n + 5) u`` of its parts plus the ``(w + cnt + P + 6) u`` it inherits through ``y``.  The intercept
  ``ym - slope tm`` has the parts ``1/n + tm |s|`` and two more roundings.
  In all: at most ``(3 (2 n + 5) + n + w + P + 8) u parts <= (7 n + 52) u parts``.
* ``A @ X``.  An entry of ``A`` is built from at most ``P + 4`` of its parts with at most 4 roundings each (window
  quotient, count quotient, the mean over the phases, the passage through the cycle rows), the product with ``X``
  is an n-term sum: ``(n + P + 8) u parts <= (n + 22) u parts``.

Together ``(8 n + 74) u parts <= C n u parts`` with ``C = 11`` for every ``n >= 25``, the smallest case tested.  (The
measured differences are a few hundredths of ``n u parts``: the bound is a worst case over n roundings of one sign.)"""
import numpy as np
from scipy.stats import linregress

from convex_dim_red import seasonal_coefficients

U = 2.0 ** -53
C = 11.0
KAPPA = 2.0
# (n, period, base_rows): the host test's shapes
CASES = [(25, 12, None), (40, 5, (3, 33)), (127, 14, (10, 120)), (1000, 12, (240, 720)), (64, 1, None)]


def columns(rng, n, p, period):
    """noise + a sinusoid of the period + a drift; every second column offset by 1e4."""
    t = np.arange(n)[:, np.newaxis]
    X = rng.standard_normal((n, p)) * rng.uniform(0.2, 2.0, size=p)
    X += np.sin(2.0 * np.pi * t / period + rng.uniform(0.0, 6.0, size=p)) * rng.uniform(1.0, 3.0, size=p)
    X += t * (0.02 * rng.standard_normal(p))
    X[:, ::2] += 1e4
    return X


def restate(X, period, base_rows=None, trend_order=1):
    """(cycle (P, p), slope (p,), intercept (p,)) of the notebook's calculation; slope / intercept None without trend."""
    n, p = X.shape
    lo, hi = (0, n) if base_rows is None else base_rows
    if period % 2 == 0:
        window = np.ones(period + 1)
        window[0] = window[-1] = 0.5
        window = window / period
    else:
        window = np.ones(period) / period
    half = (window.size - 1) // 2
    smooth = np.full(X.shape, np.nan)
    for t in range(half, n - half):
        smooth[t] = window.dot(X[t - half:t + half + 1])
    detrended = X - smooth
    phase = np.arange(n) % period
    in_base = (np.arange(n) >= lo) & (np.arange(n) < hi)
    means = np.stack([np.nanmean(detrended[in_base & (phase == g)], axis=0) for g in range(period)])
    cycle = means - means.mean(axis=0)
    if trend_order == 0:
        return cycle, None, None
    y = X - cycle[phase]
    slope, intercept = np.empty(p), np.empty(p)
    for j in range(p):
        fit = linregress(np.arange(n), y[:, j])
        slope[j], intercept[j] = fit[0], fit[1]
    return cycle, slope, intercept


def model_bound(X, period, base_rows=None, trend_order=1):
    """``C n u (A_parts @ |X|)``, (period + 2 trend_order, p), after checking the assumption KAPPA stands for."""
    n = X.shape[0]
    A, parts = seasonal_coefficients(n, period, base_rows, trend_order)
    assert parts.shape == A.shape and np.all(parts >= np.abs(A))
    if trend_order:
        y = X - restate(X, period, base_rows, 0)[0][np.arange(n) % period]
        s = np.abs(np.arange(n) - 0.5 * (n - 1))
        assert np.all(s.sum() * np.abs(y).mean(axis=0) <= KAPPA * s.dot(np.abs(y)))
    return C * n * U * parts.dot(np.abs(X))
