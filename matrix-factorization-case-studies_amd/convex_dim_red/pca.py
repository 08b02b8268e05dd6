"""PCA of resident data: EOFs and principal-component blocks without leaving the device.

What ``run_pca`` of the reference notebook ``hadisst_pca.ipynb`` computes with
``sklearn.decomposition.PCA(n_components=k, tol=1e-8)`` -- means, EOFs, PCs, explained variances, singular values
and the training / validation RMSE, one refit per ``k`` -- and what ``bin/run_jra55_pca_gpnh.py`` /
``bin/run_jra55_pca_aa.py`` then read back as the input of their fits.  Here the decomposition goes through the
Gram matrix of the smaller side of the centred matrix (aa_data_gram, float64 on the f64 matrix cores) and ONE
``numpy.linalg.eigh`` on the host, as the GPNH dictionary does its k x k solve on the host; the PCs of a block are
a row-local projection installed as a new ``DeviceData`` (aa_set_data_projected), ready for
``GPNHConvexCoding.fit_transform``.  The result is the exact PCA (scikit-learn's default at these sizes is a
randomised approximation), and ``ResidentPCA.truncate`` serves every ``k`` of the notebook's sweep from one
decomposition.

Going through a Gram matrix squares the condition number: a component whose eigenvalue is below
``max(n, p) d 2^-52`` of the largest (d the order of the Gram matrix) is not resolved and is refused.
"""
from __future__ import absolute_import, division

import numpy as np

from . import _backend
from .preprocessing import DeviceData, _is_int
from .validation import _residual_scores

MAX_COMPONENTS = _backend.MAX_PROJECTED      # directions one projection pass takes
MAX_SCORED_COMPONENTS = _backend.MAX_K - 1   # score(): the mean rides as one more factor of the scores pass
_COEF_ROWS = 16                              # coefficient rows of one aa_data_weighted_column_sums call


def _checked_request(shape, implicit, n_components, center, side):
    """(q, side) of a ``pca`` request on a block of ``shape``, or ValueError: host only, before any device call."""
    who = "DeviceData.pca"
    if implicit:
        raise ValueError("%s: the block holds no data matrix (data form needed)" % who)
    n, p = shape
    if not _is_int(n_components) or n_components < 1:
        raise ValueError("%s: n_components must be a positive integer; got %r" % (who, n_components))
    q = int(n_components)
    if side not in ("auto", "rows", "cols"):
        raise ValueError("%s: side must be 'auto', 'rows' or 'cols'; got %r" % (who, side))
    most = min(n - 1 if center else n, p)
    if q > most:
        raise ValueError("%s: %d components asked of a %d x %d block%s, which has at most %d"
                         % (who, q, n, p, " (centred)" if center else "", most))
    if q > MAX_COMPONENTS:
        raise ValueError("%s: %d components; at most %d are projected in one pass" % (who, q, MAX_COMPONENTS))
    if min(n, p) > _backend.GRAM_MAX_D:
        raise ValueError("%s: min(n, p) = %d is above GRAM_MAX_D = %d, the largest Gram matrix that is formed and "
                         "put through one dense eigen-solve" % (who, min(n, p), _backend.GRAM_MAX_D))
    if side == "auto":
        side = "rows" if n <= p else "cols"
    if (n if side == "rows" else p) > _backend.GRAM_MAX_D:
        raise ValueError("%s: side=%r needs a %d x %d Gram matrix, above GRAM_MAX_D = %d"
                         % (who, side, n if side == "rows" else p, n if side == "rows" else p, _backend.GRAM_MAX_D))
    return q, side


def gram_eigen(G, q, n, p):
    """Host only: ``(eigenvalues, vectors)`` of the symmetric Gram matrix ``G`` -- all d eigenvalues in descending
    order, clipped at 0, and the eigenvectors of the first ``q`` as columns -- or ValueError when component ``q``
    is not resolved: ``lambda_q <= max(n, p) d 2^-52 lambda_1``."""
    d = G.shape[0]
    lam, vec = np.linalg.eigh(G)
    lam, vec = lam[::-1], vec[:, ::-1]
    lam = np.maximum(lam, 0.0)
    floor = max(n, p) * d * 2.0 ** -52 * lam[0]
    if not lam[q - 1] > floor:
        raise ValueError("DeviceData.pca: component %d is not resolved through a Gram matrix (its eigenvalue %.3g is "
                         "not above max(n, p) d 2^-52 = %.3g of the largest, %.3g); %d components are resolved"
                         % (q, lam[q - 1], max(n, p) * d * 2.0 ** -52, lam[0], int(np.sum(lam > floor))))
    return lam, np.ascontiguousarray(vec[:, :q])


def orient(components):
    """Host only: every row of ``components`` with its entry of largest magnitude positive (the first such entry
    on ties): ``svd_flip(u_based_decision=False)`` of scikit-learn 1.7."""
    components = np.array(components, dtype=np.float64)
    pick = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), pick])
    signs[signs == 0] = 1.0
    return components * signs[:, None]


def row_side_coefficients(lam, vectors):
    """Host only: ``A = diag(lambda^-1/2) U'`` (q x n), so that the components are ``A Xc``.  C-contiguous: NumPy
    then sums every row on its own, and row i is the same bits whatever q is (``truncate`` is a direct fit)."""
    return np.ascontiguousarray((vectors / np.sqrt(lam[:vectors.shape[1]])).T)


class ResidentPCA(object):
    """The PCA model of a resident block.  Host arrays only (``copy.deepcopy``-safe), scikit-learn's names:

    ``components_`` (q, p) unit EOFs, the entry of largest magnitude of each positive;  ``mean_`` (p,) (zeros
    without centring);  ``explained_variance_`` lambda / (n - 1);  ``explained_variance_ratio_`` lambda / trace;
    ``singular_values_`` sqrt(lambda);  ``noise_variance_`` the mean of the remaining min(n, p) - q values of
    lambda / (n - 1) (0 if none);  ``n_samples_``, ``n_features_in_``, ``n_components_``;  ``eigenvalues_`` all d
    eigenvalues of the Gram matrix, descending;  ``centered_``, ``side_``."""

    def __init__(self, components, mean, eigenvalues, n_samples, centered, side):
        self.components_ = components
        self.mean_ = mean
        self.eigenvalues_ = eigenvalues
        self.n_samples_ = int(n_samples)
        self.n_features_in_ = int(components.shape[1])
        self.n_components_ = q = int(components.shape[0])
        self.centered_ = bool(centered)
        self.side_ = side
        dof = max(self.n_samples_ - 1, 1)
        rank = min(self.n_samples_, self.n_features_in_)
        self.explained_variance_ = eigenvalues[:q] / dof
        self.explained_variance_ratio_ = eigenvalues[:q] / eigenvalues.sum()
        self.singular_values_ = np.sqrt(eigenvalues[:q])
        self.noise_variance_ = float(eigenvalues[q:rank].mean() / dof) if rank > q else 0.0

    def truncate(self, k):
        """The model with the first ``k <= n_components_`` components: what a fit with ``n_components=k`` gives."""
        if not _is_int(k) or not 1 <= k <= self.n_components_:
            raise ValueError("ResidentPCA.truncate: k must be an integer from 1 to %d; got %r" % (self.n_components_, k))
        return ResidentPCA(self.components_[:int(k)].copy(), self.mean_.copy(), self.eigenvalues_.copy(),
                           self.n_samples_, self.centered_, self.side_)

    def _checked_block(self, block, who):
        if not isinstance(block, DeviceData):
            raise ValueError("ResidentPCA.%s: a DeviceData block expected; got %s" % (who, type(block).__name__))
        if block.ndim != 2 or block.shape[1] != self.n_features_in_:
            raise ValueError("ResidentPCA.%s: the model was fitted on %d features; the block has shape %r"
                             % (who, self.n_features_in_, tuple(block.shape)))

    def transform(self, block, dtype=None):
        """The principal components of ``block`` -- ``(block - mean_) @ components_.T`` -- as a new ``DeviceData``
        of shape (m, q) with a lifetime of its own (aa_set_data_projected).  ``dtype``: None -- float64; float32 is
        allowed only for a float32 block.  A row block of the training block, or a validation block, transforms
        with the training model, as in ``run_pca``."""
        self._checked_block(block, "transform")
        try:
            target = np.dtype(np.float64 if dtype is None else dtype)
        except TypeError:
            target = np.dtype(object)
        if target not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("ResidentPCA.transform: dtype must be float32 or float64; got %r" % (dtype,))
        if self.n_components_ > MAX_COMPONENTS:
            raise ValueError("ResidentPCA.transform: %d components; at most %d are projected in one pass"
                             % (self.n_components_, MAX_COMPONENTS))
        if target == np.dtype(np.float32) and block.dtype != target:
            raise ValueError("ResidentPCA.transform: float32 components are offered only for a float32 block")
        if block._ctx is None or not block._ctx.h:
            raise RuntimeError("DeviceData has been closed")
        ctx = _backend.Context(dtype=target, device=block._ctx.device)
        try:
            ctx.set_data_projected(block._ctx, 0, block.shape[0], self.components_,
                                   self.mean_ if self.centered_ else None)
        except Exception:
            ctx.close()
            raise
        return DeviceData(ctx, (block.shape[0], self.n_components_), None, (self.n_components_,))

    def inverse_transform(self, pcs):
        """Host only: ``pcs @ components_ + mean_`` for an (m, q) array or ``DeviceData`` of components."""
        pcs = pcs.to_host() if isinstance(pcs, DeviceData) else np.asarray(pcs, dtype=np.float64)
        if pcs.ndim != 2 or pcs.shape[1] != self.n_components_:
            raise ValueError("ResidentPCA.inverse_transform: an (m, %d) array of components expected; got shape %r"
                             % (self.n_components_, tuple(pcs.shape)))
        return pcs.dot(self.components_) + self.mean_

    def score(self, block, pcs=None):
        """``Scores`` of ``block - inverse_transform(pcs)`` (``pcs``: None -- ``transform(block)``): the training and
        validation RMSE and cost of ``run_pca``, from one pass over the resident block (aa_gpnh_residual_scores)
        with one augmented factor pair -- weights ``[pcs, 1]``, components ``[components_; mean_]`` -- so that no
        centred copy and no reconstruction is formed.  At most 63 components."""
        self._checked_block(block, "score")
        if self.n_components_ > MAX_SCORED_COMPONENTS:
            raise ValueError("ResidentPCA.score: %d components; the scores pass takes %d beside the mean (truncate())"
                             % (self.n_components_, MAX_SCORED_COMPONENTS))
        if pcs is not None and not isinstance(pcs, DeviceData):
            pcs = np.asarray(pcs, dtype=np.float64)
        if pcs is not None and tuple(pcs.shape) != (block.shape[0], self.n_components_):
            raise ValueError("ResidentPCA.score: pcs must be (%d, %d), one row per row of the block; got shape %r"
                             % (block.shape[0], self.n_components_, tuple(pcs.shape)))
        if pcs is None:
            with self.transform(block) as projected:
                pcs = projected.to_host()
        elif isinstance(pcs, DeviceData):
            pcs = pcs.to_host()
        weights = np.hstack([pcs, np.ones((pcs.shape[0], 1))])
        components = np.vstack([self.components_, self.mean_])
        return _residual_scores(block, components, weights, block.dtype)


def fit_pca(block, n_components, center=True, side="auto"):
    """``DeviceData.pca``: see there."""
    implicit = block._ctx is not None and getattr(block._ctx, "implicit", False)
    q, side = _checked_request(block.shape, implicit, n_components, center, side)
    if block._ctx is None or not block._ctx.h:
        raise RuntimeError("DeviceData has been closed")
    n, p = block.shape
    mean = np.array(block.column_stats().mean, dtype=np.float64) if center else np.zeros(p)
    G = block._ctx.data_gram(side, mean if center else None)
    lam, vectors = gram_eigen(G, q, n, p)
    if side == "cols":
        components = vectors.T
    else:
        A = row_side_coefficients(lam, vectors)
        AX = np.vstack([block._ctx.data_weighted_column_sums(A[g:g + _COEF_ROWS]) for g in range(0, q, _COEF_ROWS)])
        components = AX - np.outer(A.sum(axis=1), mean)          # A Xc = A X - (A 1) mean'
    return ResidentPCA(orient(components), mean, lam, n, center, side)
