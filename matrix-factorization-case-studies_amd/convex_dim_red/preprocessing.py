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
    ``scaling``  -- None, or the ``ColumnScaling`` a block made by ``standardized()`` was scaled with.

    Pass it as ``data`` to ``ArchetypalAnalysis.fit_transform / transform`` or
    ``GPNHConvexCoding.fit_transform``; ``close()`` (or ``with``) frees the device copy."""

    def __init__(self, ctx, shape, valid, original_shape, scaling=None):
        self._ctx = ctx
        self.shape = shape
        self.valid = valid
        self.original_shape = original_shape
        self.scaling = scaling
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
