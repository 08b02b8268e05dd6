"""Driver-side preprocessing on the GPU.

What ``bin/run_hadisst_aa.py`` / ``bin/run_jra55_pca_gpnh.py`` do with NumPy before they fit
(reference ``run_hadisst_aa.py:112-146,196-209``): multiply the field by its latitude weights,
flatten the feature dimensions, drop every grid point (column) that is missing at any time, and
split the rows into a training and a validation block.  ``weight_and_flatten_on_device`` does the
same on the device from ONE upload of the raw field and returns a ``DeviceData`` that the
estimators accept wherever they accept a data matrix; the NetCDF / xarray I/O stays with the
driver, which passes ``da.values`` (sample dimension first) and the weights it computed.
"""
from __future__ import absolute_import, division

from collections import namedtuple

import numpy as np

from . import _backend

# Column statistics of a resident block: float64 arrays of length n_features (``std`` = sqrt of the mean squared
# deviation, ddof 0, as ``np.std``) and the number of rows they were taken over.
ColumnStats = namedtuple("ColumnStats", ("mean", "std", "n_samples"))
# What ``DeviceData.standardized`` applied: the ``ColumnStats`` it divided by (and subtracted, if ``center``).
ColumnScaling = namedtuple("ColumnScaling", ("stats", "center"))

# The anomaly model a block made by ``DeviceData.seasonal_anomalies`` was built with, as float64 host arrays:
# ``seasonal_cycle`` (period, n_features), ``slope`` / ``intercept`` (n_features,; None with trend_order 0).
SeasonalAnomalies = namedtuple("SeasonalAnomalies", ("period", "base_rows", "seasonal_cycle", "slope", "intercept"))
# Per-group column statistics: ``mean`` / ``std`` (n_groups, n_features) (``std`` with ddof 0, as xarray's
# ``.std``) and ``counts``, the rows each group's statistics were taken over.
GroupedColumnStats = namedtuple("GroupedColumnStats", ("mean", "std", "counts"))
# What ``DeviceData.standardized_by_group`` applied: the statistics, whether it centred, and the row labels.
GroupScaling = namedtuple("GroupScaling", ("stats", "center", "groups"))

# What a block made by ``DeviceData.calendar_anomalies`` had removed, as host arrays: ``climatology`` / ``scale``
# (n_slots, n_features) float64 (``scale`` None without ``standardize``; rows of slots that had no base row hold NaN
# unless ``harmonics`` filled the climatology), ``counts`` the base rows per slot, ``slots`` the block's row labels.
CalendarAnomalies = namedtuple("CalendarAnomalies", ("n_slots", "base_rows", "harmonics", "climatology", "scale",
                                                     "counts", "slots"))

MAX_SLOTS = _backend.MAX_SLOTS   # calendar slots the slot-major device path takes (AA_MAX_SLOTS: 366 x 4)
MAX_GROUPS = 16          # coefficient rows / groups one device pass takes (AA_MAX_COEF_ROWS)
MAX_PERIOD = MAX_GROUPS - 2


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _checked_row_range(rows, n, who):
    """(lo, hi) of ``rows`` (None: all n rows), or ValueError."""
    if rows is None:
        return 0, n
    try:
        lo, hi = rows
    except (TypeError, ValueError):
        raise ValueError("%s: (lo, hi) expected; got %r" % (who, rows))
    if not (_is_int(lo) and _is_int(hi)):
        raise ValueError("%s: integer bounds expected; got %r, %r" % (who, lo, hi))
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi > n or hi <= lo:
        raise ValueError("%s: [%d, %d) is empty or outside the %d rows held" % (who, lo, hi, n))
    return lo, hi


def seasonal_coefficients(n, period, base_rows=None, trend_order=1):
    """Host only: the monthly-anomaly model of the reference notebook ``hadisst_sst_anom.ipynb``
    (``calculate_monthly_anomalies``) as a coefficient matrix.  Every quantity of that model is a fixed linear
    functional of a column ``x`` of ``n`` rows, so ``A @ X`` gives, for every column at once,

    * rows ``0 .. period - 1``: the seasonal cycle -- the centred moving average ``m`` (window ``[1/2, 1, ..., 1,
      1/2] / period`` for an even period, ``ones(period) / period`` for an odd one), the means of ``x - m`` over
      the rows ``t = g (mod period)`` inside ``base_rows = (lo, hi)`` (None: all rows) that have a full window
      (``h <= t < n - h``, ``h`` half the window width), minus the mean of these ``period`` phase means;
    * row ``period``: the slope, and row ``period + 1``: the intercept, of the least-squares line through
      ``x[t] - cycle[t mod period]`` over ALL rows against ``t = 0 .. n - 1`` (``trend_order=1``;
      ``trend_order=0`` leaves both rows out; higher orders, which the notebook fits with ``curve_fit``, are
      refused).

    Returns ``(A, A_parts)``, both ``(period + 2 * trend_order, n)`` float64.  ``A_parts >= |A|`` adds the
    absolute values of the parts of ``A`` BEFORE they cancel -- indicator / count, indicator * |window| / count,
    the mean over the phases, and for the trend rows ``|s|' (I + |cycle rows|)`` with ``s`` the regression's own
    weights (intercept: ``1/n + mean(t) |s|``) -- so ``n u (A_parts @ |X|)`` bounds the rounding error of
    ``A @ X`` AND of the notebook's step-by-step evaluation.  ``period``: 1 .. 14.  A phase without a usable base
    row, where the notebook would produce NaN, is a ``ValueError``."""
    if not _is_int(n) or n < 1:
        raise ValueError("seasonal_coefficients: n must be a positive integer; got %r" % (n,))
    if not _is_int(period) or not 1 <= period <= MAX_PERIOD:
        raise ValueError("seasonal_coefficients: period must be an integer from 1 to %d; got %r" % (MAX_PERIOD, period))
    if trend_order not in (0, 1) or not _is_int(trend_order):
        raise ValueError("seasonal_coefficients: trend_order must be 0 (no trend) or 1 (linear); got %r"
                         % (trend_order,))
    n, P = int(n), int(period)
    if P % 2 == 0:
        window = np.ones(P + 1)
        window[0] = window[-1] = 0.5
        window = window / P
    else:
        window = np.ones(P) / P
    h = (window.size - 1) // 2
    if n < 2 * h + 1:
        raise ValueError("seasonal_coefficients: %d rows are fewer than one moving-average window (%d)"
                         % (n, 2 * h + 1))
    if trend_order == 1 and n < 2:
        raise ValueError("seasonal_coefficients: a linear trend needs at least 2 rows")
    lo, hi = _checked_row_range(base_rows, n, "seasonal_coefficients: base_rows")
    first, stop = max(lo, h), min(hi, n - h)
    M, M_parts = np.zeros((P, n)), np.zeros((P, n))
    for g in range(P):
        rows = np.arange(first + (g - first) % P, stop, P)
        if rows.size == 0:
            raise ValueError("seasonal_coefficients: phase %d has no row with a full window inside the base rows "
                             "[%d, %d); the notebook's cycle would be NaN there" % (g, lo, hi))
        picked = np.zeros(n)
        picked[rows] = 1.0
        # the windows of the picked rows laid over each other (the window is symmetric and of odd length)
        spread = np.convolve(picked, window, mode="same")
        M[g] = (picked - spread) / rows.size
        M_parts[g] = (picked + spread) / rows.size
    cycle = M - M.mean(axis=0)
    cycle_parts = M_parts + M_parts.mean(axis=0)
    if trend_order == 0:
        return cycle, cycle_parts
    t = np.arange(n, dtype=np.float64)
    t_mean = 0.5 * (n - 1)
    s = (t - t_mean) / np.dot(t - t_mean, t - t_mean)           # slope = s' y
    phase = np.arange(n) % P

    def through_cycle(w, w_abs):
        # w' y with y = x - cycle[t mod P]: w' (I - E cycle), E the n x P indicator of the phases
        return (w - np.bincount(phase, weights=w, minlength=P).dot(cycle),
                w_abs + np.bincount(phase, weights=w_abs, minlength=P).dot(cycle_parts))
    slope, slope_parts = through_cycle(s, np.abs(s))
    icpt, icpt_parts = through_cycle(1.0 / n - t_mean * s, 1.0 / n + t_mean * np.abs(s))   # mean(y) - slope mean(t)
    return np.vstack([cycle, slope, icpt]), np.vstack([cycle_parts, slope_parts, icpt_parts])


def calendar_smoother(present, harmonics):
    """Host only: the ``(G, G)`` float64 matrix ``S`` that smooths a per-slot table (a climatology by day or
    six-hourly step of the year) and fills its empty slots: the least-squares projection onto a constant plus the
    first ``harmonics`` annual harmonics ``cos(h theta_g), sin(h theta_g)``, ``theta_g = 2 pi g / G``, fitted over
    the slots with ``present[g]`` and evaluated on all ``G`` -- ``S = B pinv(B[present])`` written into the present
    columns, zero elsewhere, so ``S @ table`` never reads a row of an absent slot (a 29 February outside the base
    period) and fills it from the fit.  ``present``: a non-empty 1-D boolean array; ``harmonics``: an integer >= 1
    with ``2 harmonics + 1 <= present.sum()``.  Like ``seasonal_coefficients`` the model is an explicit matrix, so
    the rounding of ``S @ table`` is bounded by ``(G + 2) u (|S| @ |table|)``."""
    present = np.asarray(present)
    if present.ndim != 1 or present.size < 1 or present.dtype != np.bool_:
        raise ValueError("calendar_smoother: present must be a non-empty 1-D boolean array; got %s of shape %r"
                         % (present.dtype, present.shape))
    if not _is_int(harmonics) or harmonics < 1:
        raise ValueError("calendar_smoother: harmonics must be an integer >= 1; got %r" % (harmonics,))
    G, H, m = present.size, int(harmonics), int(present.sum())
    if 2 * H + 1 > m:
        raise ValueError("calendar_smoother: %d harmonics need %d slots with data; %d of %d have any"
                         % (H, 2 * H + 1, m, G))
    theta = 2.0 * np.pi * np.arange(G) / G
    B = np.ones((G, 2 * H + 1))
    for h in range(1, H + 1):
        B[:, 2 * h - 1] = np.cos(h * theta)
        B[:, 2 * h] = np.sin(h * theta)
    S = np.zeros((G, G))
    S[:, present] = B.dot(np.linalg.pinv(B[present]))
    return S


def _checked_slots(slots, n, n_slots, who):
    """(labels as intc, number of slots) of one calendar-slot label per row, or ValueError."""
    raw = np.asarray(slots)
    if raw.ndim != 1 or raw.shape[0] != n:
        raise ValueError("%s: one slot label per row (%d) expected; got shape %r" % (who, n, raw.shape))
    if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer):
        raise ValueError("%s: integer slot labels expected; got dtype %s" % (who, raw.dtype))
    if raw.min() < 0:
        raise ValueError("%s: slot labels start at 0; got %d" % (who, raw.min()))
    if n_slots is None:
        n_slots = int(raw.max()) + 1
    elif not _is_int(n_slots) or n_slots < 1:
        raise ValueError("%s: n_slots must be a positive integer; got %r" % (who, n_slots))
    if n_slots > MAX_SLOTS:
        raise ValueError("%s: n_slots = %d: more than %d slots" % (who, n_slots, MAX_SLOTS))
    if raw.max() >= n_slots:
        raise ValueError("%s: slot label %d with n_slots = %d" % (who, raw.max(), n_slots))
    return raw.astype(np.intc), int(n_slots)


def _checked_slot_table(table, n_slots, n_features, who):
    table = np.asarray(table, dtype=np.float64)
    if table.shape != (n_slots, n_features):
        raise ValueError("%s must be (%d, %d), one row per slot; got shape %r" % (who, n_slots, n_features, table.shape))
    return table


def _first_bad(bad_mask, used):
    """(slot, column) of the first True entry of ``bad_mask`` (n_slots, p) in a slot with ``used``, or None."""
    bad = np.argwhere(bad_mask & used[:, None])
    return None if bad.size == 0 else (int(bad[0][0]), int(bad[0][1]))


def _checked_groups(groups, n, who):
    """(labels as intc, number of groups) of one label per row, or ValueError."""
    raw = np.asarray(groups)
    if raw.ndim != 1 or raw.shape[0] != n:
        raise ValueError("%s: one group label per row (%d) expected; got shape %r" % (who, n, raw.shape))
    if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer):
        raise ValueError("%s: integer group labels expected; got dtype %s" % (who, raw.dtype))
    if raw.min() < 0:
        raise ValueError("%s: group labels start at 0; got %d" % (who, raw.min()))
    if raw.max() >= MAX_GROUPS:
        raise ValueError("%s: more than %d groups (label %d)" % (who, MAX_GROUPS, raw.max()))
    return raw.astype(np.intc), int(raw.max()) + 1


def _checked_group_stats(stats, n_groups, n_features, center):
    """(shift or None, scale) tables of a per-group standardisation, or ValueError: from ``stats`` alone."""
    who = "DeviceData.standardized_by_group"
    std = None if stats.std is None else np.asarray(stats.std, dtype=np.float64)
    if std is None or std.ndim != 2 or std.shape[1] != n_features:
        raise ValueError("%s: stats.std must be (n_groups, %d); got %s"
                         % (who, n_features, "None" if std is None else "shape %r" % (std.shape,)))
    if std.shape[0] < n_groups or std.shape[0] > MAX_GROUPS:
        raise ValueError("%s: the labels name %d groups, stats.std holds %d (at most %d)"
                         % (who, n_groups, std.shape[0], MAX_GROUPS))
    bad = np.argwhere(~np.isfinite(std) | (std == 0))
    if bad.size:
        raise ValueError("%s: %d entries of stats.std are zero or non-finite (the first is group %d, column %d); the "
                         "notebook's division would fill them with inf / NaN" % (who, bad.shape[0], bad[0][0], bad[0][1]))
    if not center:
        return None, std
    if stats.mean is None:
        raise ValueError("%s: center=True needs stats with a mean" % who)
    mean = np.asarray(stats.mean, dtype=np.float64)
    if mean.shape != std.shape:
        raise ValueError("%s: stats.mean must have the shape of stats.std %r; got %r" % (who, std.shape, mean.shape))
    if not np.all(np.isfinite(mean)):
        raise ValueError("%s: stats.mean has non-finite entries" % who)
    return mean, std


def _checked_stats(stats, n_features, center):
    """(shift or None, scale) of a standardisation, or ValueError: decided on the host, from ``stats`` alone."""
    std = None if stats.std is None else np.asarray(stats.std, dtype=np.float64)
    if std is None or std.shape != (n_features,):
        raise ValueError("DeviceData.standardized: stats.std must hold one value per feature (%d); got %s"
                         % (n_features, "None" if std is None else "shape %r" % (std.shape,)))
    bad = np.flatnonzero(~np.isfinite(std) | (std == 0))
    if bad.size:
        raise ValueError("DeviceData.standardized: %d column(s) have a zero or non-finite std (the first is column "
                         "%d); the reference's division would fill them with inf / NaN" % (bad.size, bad[0]))
    if not center:
        return None, std
    if stats.mean is None:
        raise ValueError("DeviceData.standardized: center=True needs stats with a mean")
    mean = np.asarray(stats.mean, dtype=np.float64)
    if mean.shape != (n_features,):
        raise ValueError("DeviceData.standardized: stats.mean must hold one value per feature (%d); got shape %r"
                         % (n_features, mean.shape))
    if not np.all(np.isfinite(mean)):
        raise ValueError("DeviceData.standardized: stats.mean has non-finite entries")
    return mean, std


class DeviceData(object):
    """A preprocessed data matrix resident on the GPU.

    ``shape``  -- (n_samples, n_valid_features) of the block it holds;
    ``valid``  -- boolean mask over the flattened features (True: kept), what the drivers use to
                  put archetypes back on the grid;
    ``to_host()`` -- the matrix as float64 NumPy (downloaded once, then cached);
    ``scaling``  -- None, or the ``ColumnScaling`` a block made by ``standardized()`` was scaled with;
    ``anomaly``  -- None, or the ``SeasonalAnomalies`` model a block made by ``seasonal_anomalies()`` had removed;
    ``group_scaling`` -- None, or the ``GroupScaling`` a block made by ``standardized_by_group()`` was scaled with;
    ``calendar`` -- None, or the ``CalendarAnomalies`` record a block made by ``calendar_anomalies()`` had removed.

    Pass it as ``data`` to ``ArchetypalAnalysis.fit_transform / transform`` or
    ``GPNHConvexCoding.fit_transform``; ``close()`` (or ``with``) frees the device copy."""

    def __init__(self, ctx, shape, valid, original_shape, scaling=None, anomaly=None, group_scaling=None,
                 calendar=None):
        self._ctx = ctx
        self.shape = shape
        self.valid = valid
        self.original_shape = original_shape
        self.scaling = scaling
        self.anomaly = anomaly
        self.group_scaling = group_scaling
        self.calendar = calendar
        self.ndim = 2
        self._host = None
        self._stats = None

    @property
    def dtype(self):
        return np.dtype(np.float32 if self._ctx.dtype_code == _backend.AA_F32 else np.float64)

    def borrow(self):
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        return _backend._Borrowed(self._ctx)

    def rows(self, start, stop=None):
        """Rows ``[start, stop)`` (or a ``slice`` with step 1) as a new ``DeviceData``: a device-to-device
        copy (aa_set_data_rows) with a lifetime of its own -- what the drivers' cross-validation slices
        on the host (``training_data[train_index]``, bin/run_hadisst_aa.py:217-218).  ``valid`` and
        ``original_shape`` are inherited."""
        n_total = self.shape[0]
        if isinstance(start, slice):
            if stop is not None:
                raise ValueError("DeviceData.rows: a slice or (start, stop), not both")
            if start.step not in (None, 1):
                raise ValueError("DeviceData.rows: the block must be contiguous (slice step 1)")
            lo = 0 if start.start is None else start.start
            hi = n_total if start.stop is None else start.stop
        else:
            lo, hi = start, (n_total if stop is None else stop)
        if not all(isinstance(v, (int, np.integer)) for v in (lo, hi)):
            raise ValueError("DeviceData.rows: integer bounds expected; got %r, %r" % (lo, hi))
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi > n_total or hi <= lo:
            raise ValueError("DeviceData.rows: [%d, %d) is empty or outside the %d rows held" % (lo, hi, n_total))
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        ctx = _backend.Context(dtype=self.dtype, device=self._ctx.device)
        try:
            ctx.set_data_rows(self._ctx, lo, hi - lo)
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, (hi - lo, self.shape[1]), self.valid, self.original_shape, self.scaling)

    def take(self, indices, dtype=None):
        """Rows ``indices`` as a new ``DeviceData``, ``to_host()[indices]`` without leaving the device: a gather
        (aa_set_data_take) with a lifetime of its own -- seasonal subsets, k-fold splits, bootstrap resamples, the
        few rows a kernel model keeps for ``transform``.  ``indices``: a 1-D sequence or array of integers in any
        order, duplicates allowed, negative entries counting from the end as in NumPy (None: every row in order).
        ``dtype``: None (this block's) or ``np.float64`` on a float32 block, an exact widening; narrowing is
        refused.  Every refusal is a ``ValueError`` raised before any device call.  ``valid``, ``original_shape``
        and ``scaling`` are inherited."""
        n_total = self.shape[0]
        try:
            target = None if dtype is None else np.dtype(dtype)
        except TypeError:
            target = np.dtype(object)
        if target is not None and target not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("DeviceData.take: dtype must be float32 or float64; got %r" % (dtype,))
        idx = None
        if indices is not None:
            raw = np.asarray(indices)
            if raw.ndim != 1 or raw.size == 0:
                raise ValueError("DeviceData.take: a non-empty 1-D sequence of row indices expected; got shape %r"
                                 % (raw.shape,))
            if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer):
                raise ValueError("DeviceData.take: integer row indices expected (a boolean mask goes through "
                                 "np.flatnonzero); got dtype %s" % raw.dtype)
            bad = np.flatnonzero((raw < -n_total) | (raw >= n_total))
            if bad.size:
                raise ValueError("DeviceData.take: index %d (position %d) is outside the %d rows held"
                                 % (int(raw[bad[0]]), bad[0], n_total))
            idx = raw.astype(np.int64)
            idx[idx < 0] += n_total
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        if target is None:
            target = self.dtype
        elif target != self.dtype and target != np.dtype(np.float64):
            raise ValueError("DeviceData.take: a float64 block is not narrowed to float32 (only the exact widening "
                             "float32 -> float64 is offered)")
        ctx = _backend.Context(dtype=target, device=self._ctx.device)
        try:
            ctx.set_data_take(self._ctx, idx)
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, (n_total if idx is None else idx.shape[0], self.shape[1]), self.valid,
                          self.original_shape, self.scaling)

    def column_stats(self):
        """``ColumnStats(mean, std, n_samples)`` of the block's columns, from two float64 sweeps over the
        resident matrix (aa_data_column_moments); computed once (a ``DeviceData`` never changes)."""
        if self._stats is None:
            if self._ctx is None or not self._ctx.h:
                raise RuntimeError("DeviceData has been closed")
            mean, var = self._ctx.data_column_moments()
            self._stats = ColumnStats(mean, np.sqrt(var), self.shape[0])
        return self._stats

    def standardized(self, center=False, stats=None):
        """A new ``DeviceData`` (same device and dtype, a lifetime of its own) holding ``x / std``, or
        ``(x - mean) / std`` with ``center``: the drivers' ``--standardize``
        (``valid_data / np.std(valid_data, axis=0, keepdims=True)``, bin/run_jra55_pca_aa.py:165-166) without
        leaving the device.  ``stats``: None (this block's own ``column_stats()``) or the ``ColumnStats`` of
        another block -- a validation or cross-validation test block takes its training block's.  A zero or
        non-finite std, where the reference would silently produce inf / NaN, is a ``ValueError`` raised before
        anything is copied.  ``valid`` and ``original_shape`` are inherited; ``scaling`` records what was applied."""
        if stats is not None:
            shift, scale = _checked_stats(stats, self.shape[1], center)
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        if stats is None:
            stats = self.column_stats()
            shift, scale = _checked_stats(stats, self.shape[1], center)
        ctx = _backend.Context(dtype=self.dtype, device=self._ctx.device)
        try:
            ctx.set_data_rows_affine(self._ctx, 0, self.shape[0], shift, scale)
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, self.shape, self.valid, self.original_shape, ColumnScaling(stats, bool(center)))

    def seasonal_anomalies(self, period=12, base_rows=None, trend_order=1):
        """A new ``DeviceData`` (same device and dtype, a lifetime of its own) holding the monthly anomalies of the
        reference notebook ``hadisst_sst_anom.ipynb`` (``calculate_monthly_anomalies``): ``x - cycle[t mod period]
        - (intercept + slope t)``, the rows being equally spaced times ``t = 0 .. n - 1`` -- see
        ``seasonal_coefficients`` for the model, ``base_rows = (lo, hi)`` for the notebook's base period and
        ``trend_order=0`` for no detrending.  One weighted-sums pass over the resident matrix gives the model
        (aa_data_weighted_column_sums, float64), one read-and-write pass the anomalies (aa_set_data_rows_model, the
        notebook's order ``(x - cycle) - fitted``, one rounding to the block's dtype).  Every refusal is a
        ``ValueError`` raised before any device call.  ``valid``, ``original_shape`` and ``scaling`` are inherited;
        ``anomaly`` holds the ``SeasonalAnomalies`` record.  The model is tied to the row index (row ``r`` has
        phase ``r mod period`` and time ``r``), so ``rows()`` and ``take()`` of the new block carry no record."""
        n = self.shape[0]
        A, _ = seasonal_coefficients(n, period, base_rows, trend_order)
        lo, hi = _checked_row_range(base_rows, n, "base_rows")
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        P = int(period)
        model = self._ctx.data_weighted_column_sums(A)
        cycle = model[:P].copy()
        slope, icpt = (model[P].copy(), model[P + 1].copy()) if trend_order else (None, None)
        ctx = _backend.Context(dtype=self.dtype, device=self._ctx.device)
        try:
            ctx.set_data_rows_model(self._ctx, 0, n, groups=np.arange(n) % P, shift=cycle, intercept=icpt,
                                    slope=slope, t=None if slope is None else np.arange(n, dtype=np.float64))
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, self.shape, self.valid, self.original_shape, self.scaling,
                          anomaly=SeasonalAnomalies(P, (lo, hi), cycle, slope, icpt))

    def grouped_column_stats(self, groups, rows=None):
        """``GroupedColumnStats(mean, std, counts)``: the column statistics of each group of rows, ``groups`` holding
        one integer label ``0 .. G - 1`` per row, ``G <= 16`` -- the notebook's ``groupby(time.month).mean() /
        .std()`` (ddof 0).  ``rows = (lo, hi)`` counts only those rows, the notebook's base period; every group
        needs at least one counted row.  Two float64 sweeps over the resident matrix, the second over the
        deviations from the first's means (aa_data_weighted_column_sums, aa_data_grouped_sqdev).  Refusals are
        ``ValueError``s raised before any device call."""
        n = self.shape[0]
        labels, G = _checked_groups(groups, n, "DeviceData.grouped_column_stats")
        lo, hi = _checked_row_range(rows, n, "DeviceData.grouped_column_stats: rows")
        counted = np.full(n, -1, dtype=np.intc)
        counted[lo:hi] = labels[lo:hi]
        counts = np.bincount(counted[lo:hi], minlength=G)
        if np.any(counts == 0):
            raise ValueError("DeviceData.grouped_column_stats: group %d has no counted row"
                             % np.flatnonzero(counts == 0)[0])
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        A = (counted[None, :] == np.arange(G)[:, None]) / counts[:, None].astype(np.float64)
        mean = self._ctx.data_weighted_column_sums(A)
        var = self._ctx.data_weighted_column_sums(A, groups=counted, centre=mean)
        return GroupedColumnStats(mean, np.sqrt(var), counts)

    def standardized_by_group(self, groups, stats=None, center=True):
        """A new ``DeviceData`` (same device and dtype, a lifetime of its own) holding ``(x - mean[g]) / std[g]``
        with ``g = groups[row]``, or ``x / std[g]`` without ``center``: the notebook's per-month standardisation
        ``(x - mean_month) / std_month``.  ``stats``: None (this block's own ``grouped_column_stats(groups)``) or
        the ``GroupedColumnStats`` of a base period (``grouped_column_stats(groups, rows=...)``) or of another
        block.  A zero or non-finite std is a ``ValueError`` raised before anything is copied.  ``valid``,
        ``original_shape`` and ``scaling`` are inherited; ``group_scaling`` records ``(stats, center, groups)``
        (tied to the row index: ``rows()`` and ``take()`` of the new block carry none)."""
        n = self.shape[0]
        labels, G = _checked_groups(groups, n, "DeviceData.standardized_by_group")
        if stats is not None:
            shift, scale = _checked_group_stats(stats, G, self.shape[1], center)
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        if stats is None:
            stats = self.grouped_column_stats(labels)
            shift, scale = _checked_group_stats(stats, G, self.shape[1], center)
        ctx = _backend.Context(dtype=self.dtype, device=self._ctx.device)
        try:
            ctx.set_data_rows_model(self._ctx, 0, n, groups=labels, shift=shift, scale=scale)
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, self.shape, self.valid, self.original_shape, self.scaling,
                          group_scaling=GroupScaling(stats, bool(center), labels))

    def _slot_moments(self, counted, G, centre):
        """(mean, counts) of the counted rows per slot, or with ``centre`` (root mean square about it, counts); NaN
        where a slot has no counted row."""
        sums, counts = self._ctx.data_slot_sums(counted, G, centre=centre)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(counts[:, None] > 0, sums / counts[:, None].astype(np.float64), np.nan)
        return (out if centre is None else np.sqrt(out)), counts

    def calendar_stats(self, slots, n_slots=None, rows=None, centre=None):
        """``GroupedColumnStats(mean, std, counts)`` with ``(n_slots, n_features)`` tables: the column statistics of
        each calendar slot, ``slots`` holding one integer label ``0 .. n_slots - 1`` per row (day of year, six-hourly
        step of the year, pentad: the driver's time axis decides, leap days included), ``n_slots <= 1464`` (None:
        the largest label + 1) -- ``groupby(time.dayofyear).mean() / .std()`` (ddof 0) for hundreds of groups, where
        ``grouped_column_stats`` stops at 16.  ``rows = (lo, hi)`` counts only those rows, the base period.  ``std``
        is ``sqrt(sum (x - c)^2 / count)`` about ``centre`` (an ``(n_slots, n_features)`` table), or without it about
        the slot's own mean in a second sweep.  Slots without counted rows hold NaN and count 0.  Slot-major float64
        sweeps over the resident matrix (aa_data_slot_sums).  Refusals are ``ValueError``s raised before any device
        call, except a non-finite ``centre`` entry in a slot that has counted rows, which is one raised after the
        first sweep."""
        who = "DeviceData.calendar_stats"
        n, p = self.shape
        labels, G = _checked_slots(slots, n, n_slots, who)
        lo, hi = _checked_row_range(rows, n, who + ": rows")
        if centre is not None:
            centre = _checked_slot_table(centre, G, p, who + ": centre")
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        counted = np.full(n, -1, dtype=np.intc)
        counted[lo:hi] = labels[lo:hi]
        mean, counts = self._slot_moments(counted, G, None)
        if centre is not None:
            bad = _first_bad(~np.isfinite(centre), counts > 0)
            if bad:
                raise ValueError("%s: centre[%d][%d] = %r is not finite" % ((who,) + bad + (centre[bad],)))
        std, _ = self._slot_moments(counted, G, mean if centre is None else centre)
        return GroupedColumnStats(mean, std, counts)

    def calendar_anomalies(self, slots, n_slots=None, base_rows=None, harmonics=None, standardize=False, model=None):
        """A new ``DeviceData`` (same device and dtype, a lifetime of its own) holding ``x - clim[g]`` with
        ``g = slots[row]``, or ``(x - clim[g]) / scale[g]`` with ``standardize``: the deviations from a climatology
        per calendar slot that the JRA-55 drivers read as ``.anom.`` / ``.std_anom.`` files, for up to 1464 slots
        (``slots`` / ``n_slots`` as in ``calendar_stats``).  ``clim`` is the slot means over ``base_rows = (lo, hi)``
        (None: all rows); with ``harmonics = H`` it is ``calendar_smoother(counts > 0, H) @ mean`` (empty slots
        entering as 0 and filled from the fit).  ``scale[g]`` is the root mean square of ``x - clim[g]`` over the
        slot's base rows: a second sweep, centred on the climatology that is actually subtracted.  ``model``: the
        ``calendar`` record of another block (the training block's, for a validation or test block) to apply
        instead; no statistics are taken then, and ``base_rows`` / ``harmonics`` beside it are refused.  Argument
        refusals are ``ValueError``s raised before any device call; after the sums and before anything is copied, a
        slot that a row of this block uses and whose climatology is not finite (no base row and no ``harmonics``) or
        whose scale is zero or not finite is a ``ValueError`` that names slot and column.  ``valid``,
        ``original_shape`` and ``scaling`` are inherited; ``calendar`` holds the ``CalendarAnomalies`` record (tied
        to the row index: ``rows()`` and ``take()`` of the new block carry none).  Trends are not removed."""
        who = "DeviceData.calendar_anomalies"
        n, p = self.shape
        S = None
        if model is not None:
            if not isinstance(model, CalendarAnomalies):
                raise ValueError("%s: model must be a CalendarAnomalies record; got %r" % (who, type(model).__name__))
            if base_rows is not None or harmonics is not None:
                raise ValueError("%s: base_rows / harmonics belong to the block the model was taken from; "
                                 "leave them out beside model" % who)
            if n_slots is not None and n_slots != model.n_slots:
                raise ValueError("%s: n_slots = %r, the model has %d" % (who, n_slots, model.n_slots))
            labels, G = _checked_slots(slots, n, model.n_slots, who)
            clim = _checked_slot_table(model.climatology, G, p, who + ": model.climatology")
            scale = None
            if standardize:
                if model.scale is None:
                    raise ValueError("%s: standardize needs a model with a scale (taken with standardize)" % who)
                scale = _checked_slot_table(model.scale, G, p, who + ": model.scale")
            lo, hi = model.base_rows
            harmonics, counts = model.harmonics, model.counts
        else:
            labels, G = _checked_slots(slots, n, n_slots, who)
            lo, hi = _checked_row_range(base_rows, n, who + ": base_rows")
            if harmonics is not None:
                if not _is_int(harmonics) or harmonics < 1:
                    raise ValueError("%s: harmonics must be None or an integer >= 1; got %r" % (who, harmonics))
                try:
                    S = calendar_smoother(np.bincount(labels[lo:hi], minlength=G) > 0, harmonics)
                except ValueError as e:
                    raise ValueError("%s: harmonics: %s" % (who, e))
        used = np.bincount(labels, minlength=G) > 0
        if self._ctx is None or not self._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        if model is None:
            counted = np.full(n, -1, dtype=np.intc)
            counted[lo:hi] = labels[lo:hi]
            mean, counts = self._slot_moments(counted, G, None)
            clim = mean if S is None else S.dot(np.where(np.isnan(mean), 0.0, mean))
        bad = _first_bad(~np.isfinite(clim), used)
        if bad:
            raise ValueError("%s: the climatology of slot %d, column %d is %r: a row of the block uses the slot, no "
                             "base row does and there are no harmonics to fill it" % ((who,) + bad + (clim[bad],)))
        if model is None:
            scale = self._slot_moments(counted, G, clim)[0] if standardize else None
        if scale is not None:
            bad = _first_bad(~np.isfinite(scale) | (scale == 0), used)
            if bad:
                raise ValueError("%s: the scale of slot %d, column %d is %r (zero or not finite); the division would "
                                 "fill the column with inf / NaN" % ((who,) + bad + (scale[bad],)))
        ctx = _backend.Context(dtype=self.dtype, device=self._ctx.device)
        try:
            ctx.set_data_rows_slots(self._ctx, 0, n, labels, shift=clim, scale=scale)
        except Exception:
            ctx.close()
            raise
        record = CalendarAnomalies(G, (lo, hi), None if harmonics is None else int(harmonics), clim, scale, counts,
                                   labels)
        return DeviceData(ctx, self.shape, self.valid, self.original_shape, self.scaling, calendar=record)

    def pca(self, n_components, center=True, side='auto'):
        """The ``ResidentPCA`` model of this block with ``n_components`` leading components: what
        ``sklearn.decomposition.PCA(n_components, svd_solver='full')`` fits on ``to_host()`` (``run_pca`` of the
        reference notebook ``hadisst_pca.ipynb``), without the download.  The mean is ``column_stats()``'s (zeros
        with ``center=False``); the Gram matrix of the centred block with itself (aa_data_gram, float64) over the
        smaller side -- ``side='auto'``: by rows if n <= p, else by columns; 'rows' / 'cols' force one -- goes
        through one ``numpy.linalg.eigh`` on the host.  By columns the components are the eigenvectors; by rows
        they are ``diag(lambda^-1/2) U' Xc``, one weighted-sums pass per 16 components
        (aa_data_weighted_column_sums).  Every component is oriented so that its entry of largest magnitude is
        positive.  Refusals are ``ValueError``s raised before any device call: ``n_components`` not a positive
        integer, above ``min(n - 1 if center else n, p)`` or above 256, and ``min(n, p)`` above 8192
        (``_backend.GRAM_MAX_D``); after the eigen-solve, a component that a Gram matrix does not resolve."""
        from .pca import fit_pca
        return fit_pca(self, n_components, center=center, side=side)

    def unscale(self, array):
        """Host only: a ``(..., n_features)`` array in this block's units (archetypes, a dictionary's transpose,
        a reconstruction) back in the units before ``standardized()``: ``array * std (+ mean)``.  The identity
        for a block that is not standardised."""
        if self.scaling is None:
            return array
        array = np.asarray(array, dtype=np.float64)
        stats, center = self.scaling
        if array.ndim < 1 or array.shape[-1] != self.shape[1]:
            raise ValueError("DeviceData.unscale: the last axis must hold the %d features; got shape %r"
                             % (self.shape[1], array.shape))
        out = array * np.asarray(stats.std, dtype=np.float64)
        if center:
            out += np.asarray(stats.mean, dtype=np.float64)
        return out

    def to_host(self):
        if self._host is None:
            self._host = self._ctx.get_data()
        return self._host

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __deepcopy__(self, memo):          # never copied into a model (estimators keep no data)
        return self


def weight_and_flatten_on_device(values, weights=None, rows=None, dtype=None, device=None, standardize=False):
    """``values``: array (n_samples, *feature_dims), NaN where data are missing (``da.values``
    with the sample dimension first, as ``weight_and_flatten_data`` arranges it);
    ``weights``: None or an array broadcastable to ``feature_dims`` (e.g. the latitude weights
    ``sqrt(cos(lat))[:, None]`` for (lat, lon) fields);
    ``rows``: None (all samples) or a ``slice`` / ``(start, stop)`` of the block to keep resident
    (``slice(0, n_training)`` for the training set, ``slice(n_training, None)`` for validation --
    the NaN mask is always taken over ALL samples, as the reference takes it before it splits);
    ``standardize``: divide every kept column by its standard deviation over the rows kept, as the JRA-55
    drivers' ``--standardize`` does after the mask (bin/run_jra55_pca_aa.py:157-166); the block returned is
    ``DeviceData.standardized()`` of the one described above and carries the statistics in ``scaling``.
    Returns a ``DeviceData``."""
    values = np.asarray(values)
    if values.ndim < 2:
        raise ValueError("expected an array with a sample dimension and at least one feature dimension")
    n_total = values.shape[0]
    feature_shape = values.shape[1:]
    flat = values.reshape(n_total, -1)
    col_w = None
    if weights is not None:
        col_w = np.ascontiguousarray(np.broadcast_to(np.asarray(weights, dtype=np.float64),
                                                     feature_shape)).reshape(-1)
    if rows is None:
        start, stop = 0, n_total
    elif isinstance(rows, slice):
        start, stop, step = rows.indices(n_total)
        if step != 1:
            raise ValueError("rows must be a contiguous block")
    else:
        start, stop = rows
    ctx = _backend.Context(dtype=dtype, device=device)
    try:
        valid = ctx.set_data_weighted(flat, col_w, start, stop - start)
    except Exception:
        ctx.close()
        raise
    block = DeviceData(ctx, (stop - start, int(valid.sum())), valid, feature_shape)
    if not standardize:
        return block
    with block:
        return block.standardized()
