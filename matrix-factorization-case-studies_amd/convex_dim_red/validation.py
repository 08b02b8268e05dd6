"""Reconstruction scores and time-series cross-validation on resident data.

What the reference's drivers do on the host after every fit and every ``transform``
(``bin/run_hadisst_aa.py:213-245, 285-290, 325-366``; the same in the other AA / GPNH drivers):
``inverse_transform`` and ``mean_squared_error(data, reconstruction, squared=False)``, and in the
cross-validation branch a fit on every growing prefix of the training rows (``TimeSeriesSplit``)
followed by a transform of the block behind it.  Here the scores come from one pass over the
resident matrix (aa_gpnh_residual_scores: the m x p reconstruction is never formed and the data
never leave the GPU), the folds are row blocks cut on the device (``DeviceData.rows``), and the
drivers' loop is one call.
"""
from __future__ import absolute_import, division

from collections import namedtuple
from copy import deepcopy

import numpy as np

from . import _backend
from .preprocessing import DeviceData

Scores = namedtuple("Scores", ["cost", "rmse", "rmse_pooled", "column_sse", "sample_sse"])
Scores.__doc__ = """Reconstruction scores of m samples with p features, R = data - weights . components:

``cost``        0.5 ||R||_F^2 / m in residual form (what ``ArchetypalAnalysis.transform`` returns; for
                GPNH the data term of the cost, without ``lambda_W`` x penalty);
``rmse``        mean over the columns of sqrt(column_sse / m): ``mean_squared_error(data,
                reconstruction, squared=False)`` of the drivers (uniform average over the outputs);
``rmse_pooled`` sqrt(||R||_F^2 / (m p));
``column_sse``  (p) sums of squares per feature;  ``sample_sse``  (m) per sample."""


def _scores_from_sums(column_sse, sample_sse):
    """The derived numbers from the two vectors of sums of squares (host only)."""
    column_sse = np.asarray(column_sse, dtype=np.float64)
    sample_sse = np.asarray(sample_sse, dtype=np.float64)
    m, p = sample_sse.shape[0], column_sse.shape[0]
    sse = column_sse.sum()
    return Scores(cost=0.5 * sse / m, rmse=np.sqrt(column_sse / m).mean(),
                  rmse_pooled=np.sqrt(sse / (m * p)), column_sse=column_sse, sample_sse=sample_sse)


KernelScores = namedtuple("KernelScores", ["cost", "rmse", "explained", "sample_sse", "diagonal"])
KernelScores.__doc__ = """Feature-space scores of m samples under a kernel model (``KernelAA.kernel_scores``), with
r_t = kappa(y_t, y_t) - 2 w_t.(D kappa(X, y_t)) + w_t' A w_t the squared feature-space distance of sample t from
its reconstruction and d_t = kappa(y_t, y_t):

``cost``        0.5 sum_t r_t / m (the kernel-form cost ``KernelAA.transform`` returns);
``rmse``        sqrt(max(sum_t r_t, 0) / m), a distance in feature space;
``explained``   1 - sum_t r_t / sum_t d_t;
``sample_sse``  (m) r_t, not clamped: it may be negative at rounding level;  ``diagonal``  (m) d_t."""


def _kernel_scores_from_sums(sample_sse, diagonal, sum_r, sum_d):
    """The derived numbers from the two vectors and their sums (host only)."""
    sample_sse = np.asarray(sample_sse, dtype=np.float64)
    diagonal = np.asarray(diagonal, dtype=np.float64)
    m = sample_sse.shape[0]
    sum_r, sum_d = float(sum_r), float(sum_d)
    return KernelScores(cost=0.5 * sum_r / m, rmse=float(np.sqrt(max(sum_r, 0.0) / m)),
                        explained=1.0 - sum_r / sum_d, sample_sse=sample_sse, diagonal=diagonal)


def _score_arguments(whom, data, n_features, n_components, weights, model_weights):
    """Host-side checks of ``score`` (before any device call); returns (data, weights)."""
    if not isinstance(data, DeviceData):
        data = np.asarray(data)
        if data.dtype != np.float32:
            data = np.asarray(data, dtype=np.float64)
    if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != n_features:
        raise ValueError("%s.score: expected an (m, %d) data matrix with m >= 1 (the model was fitted on %d "
                         "features); got shape %s" % (whom, n_features, n_features, tuple(data.shape)))
    if weights is None:
        weights = model_weights
        if weights is None:
            raise ValueError("%s.score: the model holds no weights; pass `weights`" % whom)
    weights = np.asarray(weights, dtype=np.float64)
    if weights.shape != (data.shape[0], n_components):
        raise ValueError("%s.score: `weights` must be (%d, %d), one row per row of data; got shape %s"
                         % (whom, data.shape[0], n_components, weights.shape))
    return data, weights


def _residual_scores(data, components, weights, dtype):
    """Scores of ``data - weights . components`` (``components``: k x p) on the device: the data's own
    context when it is a ``DeviceData``, else one upload in the arithmetic ``transform`` would use."""
    on_device = isinstance(data, DeviceData)
    if on_device:
        manager = data.borrow()
    else:
        manager = _backend.Context(dtype=np.float64 if data.dtype == np.float64 else dtype)
    with manager as ctx:
        if not on_device:
            ctx.set_data(data, form=_backend.FORM_DATA)
        ctx.gpnh_set_factors(components.shape[0], W=components.T, Z=weights)
        column_sse, sample_sse, _ = ctx.gpnh_residual_scores(total=False)
    return _scores_from_sums(column_sse, sample_sse)


def time_series_folds(n_samples, n_folds):
    """``[(train_stop, test_start, test_stop), ...]``: the splits of
    ``sklearn.model_selection.TimeSeriesSplit(n_splits=n_folds)`` on ``n_samples`` rows -- fold i trains
    on rows ``[0, train_stop)`` and tests on ``[test_start, test_stop)`` with ``test_start == train_stop``,
    test blocks of ``n_samples // (n_folds + 1)`` rows, the last one ending at ``n_samples``."""
    if not isinstance(n_folds, (int, np.integer)) or isinstance(n_folds, bool):
        raise ValueError("The number of folds must be of Integral type. %r was passed." % (n_folds,))
    n_folds, n_samples = int(n_folds), int(n_samples)
    if n_folds <= 1:
        raise ValueError("time_series_folds requires at least one train/test split by setting n_folds=2 or "
                         "more, got n_folds=%d." % n_folds)
    if n_folds + 1 > n_samples:
        raise ValueError("Cannot have number of folds=%d greater than the number of samples=%d."
                         % (n_folds + 1, n_samples))
    test_size = n_samples // (n_folds + 1)
    first = n_samples - n_folds * test_size
    return [(start, start, start + test_size) for start in range(first, n_samples, test_size)]


def _kernel_model_scores(fit_kwargs):
    """Whether the models of a cross-validation are scored in feature space (``KernelAA`` on a non-linear
    kernel: ``kernel_scores``) rather than in data space (``score``); refuses a ``KernelAA`` that would be
    fitted on an explicit kernel matrix.  Host only."""
    if not fit_kwargs.get('features', False):
        raise ValueError("time_series_cross_validate: a KernelAA is cross-validated on feature rows "
                         "(fit_kwargs=dict(features=True, kernel=...)); an explicit kernel matrix has no row "
                         "blocks: its training and test parts are sub-matrices, not runs of rows")
    return fit_kwargs.get('kernel', 'linear') != 'linear'


def time_series_cross_validate(make_model, data, n_folds=10, n_init=1, dtype=None, fit_kwargs=None):
    """The cross-validation loop of the drivers (``bin/run_hadisst_aa.py:215-244`` with ``fit_aa_model``
    ``:149-174``) on resident data.

    ``make_model()`` returns a fresh ``ArchetypalAnalysis`` or ``GPNHConvexCoding`` (the drivers build
    theirs on one shared ``RandomState``); ``data`` is the training matrix, a host array -- uploaded
    ONCE in ``dtype`` (None: the package default), then cut on the device -- or a ``DeviceData``.
    Per fold, in the drivers' order and with their draws: ``n_init`` times ``make_model()`` and
    ``fit_transform`` of the training prefix, keeping a deep copy of the first model with the lowest cost;
    ``score`` of that model on the prefix with its own weights; ``transform`` of the test block;
    ``score`` on the test block.  Restarts inside a fold run one after the other on the resident prefix.

    ``fit_kwargs`` (None: none) are passed to every ``fit_transform``.  With
    ``fit_kwargs=dict(features=True, kernel='rbf' | 'poly', ...)`` ``make_model()`` may return a ``KernelAA``:
    the same loop and draw order, the training block never leaves the device, and the two RMSEs are feature-space
    distances, ``kernel_scores(...).rmse``, joined by ``training_explained`` / ``test_explained``; on the linear
    kernel (``features=True`` alone) the scores are ``score``'s, as for the other estimators.  A ``KernelAA``
    without ``features=True`` is refused before the upload: an explicit kernel matrix has no row blocks.

    Returns a dict of per-fold lists: ``training_cost`` (the fit's cost), ``training_rmse``,
    ``test_cost`` (what ``transform`` returned), ``test_rmse``, ``n_iter``, ``training_weights``,
    ``test_weights``, ``folds`` (``time_series_folds``) and ``models`` (the kept models)."""
    if not isinstance(n_init, (int, np.integer)) or n_init < 1:
        raise ValueError("n_init must be a positive integer; got %r" % (n_init,))
    fit_kwargs = {} if fit_kwargs is None else dict(fit_kwargs)
    own = not isinstance(data, DeviceData)
    if own:
        data = np.asarray(data)
        if data.ndim != 2:
            raise ValueError("expected a data matrix (n_samples x n_features); got shape %s" % (data.shape,))
    folds = time_series_folds(data.shape[0], n_folds)
    out = dict(training_cost=[], training_rmse=[], test_cost=[], test_rmse=[], n_iter=[], training_weights=[],
               test_weights=[], folds=folds, models=[])
    # the first model is made before the upload (nothing is drawn in between), so that a kernel model that cannot
    # be cross-validated is refused before anything reaches the device
    first = make_model()
    in_feature_space = hasattr(first, 'kernel_scores') and _kernel_model_scores(fit_kwargs)
    if in_feature_space:
        out.update(training_explained=[], test_explained=[])
    if own:
        ctx = _backend.Context(dtype=dtype)
        try:
            ctx.set_data(data, form=_backend.FORM_DATA)
        except Exception:
            ctx.close()
            raise
        data = DeviceData(ctx, data.shape, None, data.shape[1:])
    try:
        for train_stop, test_start, test_stop in folds:
            with data.rows(0, train_stop) as train, data.rows(test_start, test_stop) as test:
                best = None
                for _ in range(n_init):
                    model, first = (make_model(), None) if first is None else (first, None)
                    model.fit_transform(train, **fit_kwargs)
                    if best is None or model.cost < best.cost:
                        best = deepcopy(model)
                out["training_cost"].append(best.cost)
                out["n_iter"].append(best.n_iter)
                out["training_weights"].append(best.weights)
                scores = best.kernel_scores(train) if in_feature_space else best.score(train)
                out["training_rmse"].append(scores.rmse)
                if in_feature_space:
                    out["training_explained"].append(scores.explained)
                test_weights, test_cost = best.transform(test)
                out["test_cost"].append(test_cost)
                out["test_weights"].append(test_weights)
                scores = best.kernel_scores(test) if in_feature_space else best.score(test)
                out["test_rmse"].append(scores.rmse)
                if in_feature_space:
                    out["test_explained"].append(scores.explained)
                out["models"].append(best)
    finally:
        if own:
            data.close()
    return out
