"""Archetypal analysis on MI355X.

Mirrors the public classes and the test-visible private functions of reference
src/convex_dim_red/archetypal_analysis.py (same names, argument meaning, return
tuples, exceptions and warnings); every numeric step runs on the GPU through
``_backend.Context`` (csrc/solver.hip) -- the alternating loop included: the monotonicity
check, the stopping rule and the k-vector scale-factor update (``delta != 0``) run on the
device (aa_iterate), the host reads one status record per batch of iterations.  What stays
on the host is argument validation, RNG-ordered initialisation (FurthestSum's candidate
list), warnings, timing and verbose tables; the host-driven one-update-at-a-time loop is
kept as a cross-check (``_DEVICE_LOOP = False``).

Unlike the reference, ``ArchetypalAnalysis`` never forms the n x n kernel
``data.dot(data.T)`` (reference :1032), the n x n dissimilarity matrix (:95-100) or
``np.trace(X.dot(X.T))`` (:552): FurthestSum pulls distance columns from the device
and the trace is ||X||_F^2.
"""
from __future__ import absolute_import, division, print_function

import contextlib
import numbers
import time
import warnings

import numpy as np
from sklearn.exceptions import NotFittedError
from sklearn.utils import check_array, check_random_state

from . import _backend
from .furthest_sum import furthest_sum, furthest_sum_from_columns
from .preprocessing import DeviceData
from .simplex_projection import simplex_project_rows  # noqa: F401  (reference re-export)
from .spg import quad_simplex_spg, spg  # noqa: F401
from .stochastic_matrices import right_stochastic_matrix
from .validation import _kernel_scores_from_sums, _residual_scores, _score_arguments
from .validation_utils import check_array_shape, check_stochastic_matrix

INTEGER_TYPES = (numbers.Integral, np.integer)
INITIALIZATION_METHODS = (None, 'random', 'furthest_sum',)
_DEVICE_LOOP_BATCH = 8          # outer iterations between two host polls of the device loop
_DEVICE_LOOP = True


# ----------------------------------------------------------------------------
# validation / initialisation (reference :27-164) -- host side
# ----------------------------------------------------------------------------
def _check_init_weights(weights, shape, whom):
    check_stochastic_matrix(check_array(weights), shape, whom, axis=1)


def _check_init_dictionary(dictionary, shape, whom):
    check_stochastic_matrix(check_array(dictionary), shape, whom, axis=1)


def _check_init_scale_factors(alpha, delta, shape, whom):
    check_array_shape(alpha, shape, whom)
    if np.any(np.logical_or(alpha < 1 - delta, alpha > 1 + delta)):
        raise ValueError('Initial scale factors infeasible in %s' % (whom))


def _initialize_kernel_aa_scale_factors_random(n_components, delta=0, random_state=None):
    rng = check_random_state(random_state)
    if delta != 0:
        return rng.uniform(low=(1 - delta), high=(1 + delta), size=(n_components,))
    return np.ones(n_components)


def _one_hot_rows(selected, n_samples, dtype):
    dictionary = np.zeros((len(selected), n_samples), dtype=dtype)
    dictionary[np.arange(len(selected)), np.asarray(selected, dtype=np.int64)] = 1
    return dictionary


def _initialize_kernel_aa_dictionary_furthest_sum(kernel, n_components, start_index=None,
                                                  n_extra_steps=10, exclude=None,
                                                  random_state=None):
    """Reference :84-110 for a given kernel matrix (KernelAA path)."""
    rng = check_random_state(random_state)
    n_samples = kernel.shape[0]
    if start_index is None:
        start_index = rng.randint(n_samples)
    if exclude is None:
        exclude = np.array([], dtype='i8')
    diag = np.diag(kernel)
    dissimilarities = np.sqrt(diag[np.newaxis, :] - 2 * kernel + diag[:, np.newaxis])
    selected = furthest_sum(dissimilarities, n_components, start_index, exclude, n_extra_steps)
    return _one_hot_rows(selected, n_samples, kernel.dtype)


_FURTHEST_SUM_ON_DEVICE = True       # False: always the host-driven selection (one distance column per pick)


def _furthest_sum_on_device(ctx, n_samples, n_components, start_index, n_extra_steps, exclude, cache=None):
    """FurthestSum with distance columns computed from the resident data matrix (``cache``: columns
    already fetched for the same matrix -- restarts.fit_restarts shares one over its restarts)."""
    shared = cache is not None                   # restarts.fit_restarts: one cache for the draws of all restarts
    cache = {} if cache is None else cache
    # A restart loop on a matrix whose distance columns are expensive (short and wide: the
    # HadISST shape, 322 MB per column) keeps the host-driven form: its picks end at the same few
    # extreme points restart after restart, so nearly every column comes out of the shared cache.
    column_bytes = float(getattr(ctx, 'n', 0)) * float(getattr(ctx, 'p', 0)) * (4 if ctx.dtype_code == _backend.AA_F32 else 8)
    if _FURTHEST_SUM_ON_DEVICE and not (shared and column_bytes > 64e6):
        # the whole selection in one chain of device launches (aa_furthest_sum); the host's list logic
        # below takes over when a pick meets a shared maximum (the reference's tie rule lives there)
        from .furthest_sum import _validate
        ex = [] if exclude is None else [int(e) for e in exclude]
        _validate(n_samples, n_components, start_index, ex)
        picked = ctx.furthest_sum(n_components, start_index, ex, n_extra_steps) if n_components > 0 else None
        if picked is not None:
            return picked

    def column_of(j, sense):
        j = int(j)
        if j not in cache:
            cache[j] = ctx.distance_column(j)
        return cache[j]

    def row_entry(i, j):
        return column_of(j, "into")[int(i)]

    return furthest_sum_from_columns(column_of, row_entry, n_samples, n_components,
                                     start_index, exclude=exclude, extra_steps=n_extra_steps)


def _initialize_kernel_aa_dictionary(kernel, n_components, init='furthest_sum',
                                     random_state=None, **kwargs):
    if init is None:
        init = 'furthest_sum'
    if init == 'furthest_sum':
        return _initialize_kernel_aa_dictionary_furthest_sum(
            kernel, n_components, start_index=kwargs.get('start_index', None),
            n_extra_steps=kwargs.get('n_extra_steps', 10), exclude=kwargs.get('exclude', None),
            random_state=random_state)
    if init == 'random':
        rng = check_random_state(random_state)
        return right_stochastic_matrix((n_components, kernel.shape[0]), random_state=rng)
    raise ValueError('Invalid init parameter: got %r instead of one of %r'
                     % (init, INITIALIZATION_METHODS))


def _initialize_kernel_aa_weights(kernel, n_components, init='furthest_sum', random_state=None):
    if init is None:
        init = 'furthest_sum'
    if init in ('furthest_sum', 'random'):
        rng = check_random_state(random_state)
        return right_stochastic_matrix((kernel.shape[0], n_components), random_state=rng)
    raise ValueError('Invalid init parameter: got %r instead of one of %r'
                     % (init, INITIALIZATION_METHODS))


def _initialize_kernel_aa(kernel, n_components, init='furthest_sum', random_state=None, **kwargs):
    """Dictionary first, then weights, from the same generator (reference :151-164)."""
    rng = check_random_state(random_state)
    dictionary = _initialize_kernel_aa_dictionary(kernel, n_components, init=init,
                                                  random_state=rng, **kwargs)
    weights = _initialize_kernel_aa_weights(kernel, n_components, init=init, random_state=rng)
    return dictionary, weights


class _ShapeOnly(object):
    """Stands in for the n x n kernel where only ``shape[0]`` is consulted."""

    def __init__(self, n):
        self.shape = (n, n)


def _check_if_cost_increased(old, new, tolerance, stage, require_decrease=True):
    """Reference :167-174."""
    if (new > old) and (abs(new - old) > tolerance) and require_decrease:
        raise RuntimeError('factorization cost increased after {} update'.format(stage))


def _get_stopping_criteria(stopping_criterion):
    """Reference :177-197."""
    if stopping_criterion == 'abs_delta_f':
        return lambda old_cost, new_cost, tolerance: abs(new_cost - old_cost) < tolerance
    if stopping_criterion == 'rel_delta_f':
        return lambda old_cost, new_cost, tolerance: (
            abs((new_cost - old_cost) / max(abs(new_cost), abs(old_cost))) < tolerance)
    raise ValueError("unsupported stopping criterion '%s'" % stopping_criterion)


# ----------------------------------------------------------------------------
# scale factors (reference :220-258): k-vector problem, stays on the host
# ----------------------------------------------------------------------------
def _kernel_aa_scale_factors_objective(alpha, trace_K, CKZ, ZtZ, CKCt):
    n_samples = CKZ.shape[1]
    return 0.5 * (trace_K - 2 * alpha.dot(np.diag(CKZ))
                  + np.sum(np.outer(alpha, alpha) * ZtZ * CKCt)) / n_samples


def _kernel_aa_scale_factors_gradient(alpha, CKZ, ZtZ, CKCt):
    n_samples = CKZ.shape[1]
    return np.diag(ZtZ.dot(np.diag(alpha).dot(CKCt)) - CKZ) / n_samples


def _update_kernel_aa_scale_factors(alpha, trace_K, CKZ, ZtZ, CKCt, delta, **kwargs):
    lo, hi = 1.0 - delta, 1.0 + delta
    return spg(lambda a: _kernel_aa_scale_factors_objective(a, trace_K, CKZ, ZtZ, CKCt),
               lambda a: _kernel_aa_scale_factors_gradient(a, CKZ, ZtZ, CKCt),
               alpha, project=lambda a: np.fmin(np.fmax(lo, a), hi), **kwargs)[0]


# ----------------------------------------------------------------------------
# device-backed building blocks
# ----------------------------------------------------------------------------
def _warn_from_spg_flags(stats):
    """Re-issue the UserWarnings spg() raises (reference spg.py:225-229,272-281); ``stats``
    is one update's SPGStats or the device loop's IterStats (flags OR-ed over its iterations)."""
    flags = stats.flags if hasattr(stats, 'flags') else stats.spg_flags
    if flags & _backend.SPG_FLAG_LAMBDA_MIN:
        warnings.warn('step size below tolerance in SPG line search', UserWarning)
    if flags & _backend.SPG_FLAG_MAX_FEVAL:
        warnings.warn('maximum number of function evaluations exceeded in SPG', UserWarning)
    if flags & _backend.SPG_FLAG_MAX_ITER:
        warnings.warn('maximum number of iterations exceeded in SPG', UserWarning)
    if flags & _backend.SPG_FLAG_PROJ_UNCONV:
        warnings.warn('simplex projection pass cap reached on the device', RuntimeWarning)


def _scaled_cost(ctx, alpha):
    """0.5 (tr - 2 tr(D CKZ) + tr(D ZtZ D CKCt)) / n from the device Gram products."""
    ctx.set_alpha(alpha)
    return ctx.cost()


def _kernel_aa_cost(K, weights, dictionary, alpha):
    """Kernel AA cost (reference :200-217)."""
    K = np.asarray(K, dtype=np.float64)
    with _backend.Context(dtype=np.float64) as ctx:
        ctx.set_data(K, form=_backend.FORM_KERNEL)
        ctx.set_state(dictionary, weights, alpha)
        return ctx.prepare()


def _update_dictionary_on_device(matrix, form, dictionary, alpha, trace, KZ, ZtZ, dtype, **kwargs):
    with _backend.Context(dtype=dtype) as ctx:
        ctx.set_data(matrix, form=form)
        n, k = dictionary.shape[1], dictionary.shape[0]
        placeholder = np.full((n, k), 1.0 / k)
        ctx.set_state(dictionary, placeholder, alpha)
        ctx.set_dictionary_inputs(KZ, ZtZ, trace)
        stats = ctx.dictionary_update(**kwargs)
        _warn_from_spg_flags(stats)
        return ctx.get_state()[0]


def _update_kernel_aa_dictionary(K, dictionary, alpha, trace_K, KZ, ZtZ, **kwargs):
    """SPG update of the dictionary for kernel AA (reference :304-321)."""
    return _update_dictionary_on_device(np.asarray(K, dtype=np.float64), _backend.FORM_KERNEL,
                                        dictionary, alpha, trace_K, KZ, ZtZ, np.float64, **kwargs)


def _update_aa_dictionary(X, dictionary, alpha, trace_XXt, XXtZ, ZtZ, **kwargs):
    """SPG update of the dictionary for AA (reference :324-341)."""
    return _update_dictionary_on_device(np.asarray(X), _backend.FORM_DATA, dictionary, alpha,
                                        trace_XXt, XXtZ, ZtZ, None, **kwargs)


def _update_kernel_aa_weights(weights, alpha, CK, CKCt, **solver_kwargs):
    """Per-sample simplex QPs (reference :369-396)."""
    da = np.diag(alpha)
    return _backend.qp_batch(da.dot(CKCt.dot(da)), da.dot(CK), weights, "kn", **solver_kwargs)


def _gu_update_kernel_aa_weights(CKCt, CK, initial_weights, gamma, memory, sigma_one, sigma_two,
                                 lambda_min, alpha0, alpha_min, alpha_max, epsilon_one,
                                 epsilon_two, max_iterations, max_feval):
    """Positional form of the reference gufunc (:344-366)."""
    return _backend.qp_batch(CKCt, CK, initial_weights, "kn", gamma=gamma, memory=memory,
                             sigma_one=sigma_one, sigma_two=sigma_two, lambda_min=lambda_min,
                             alpha0=alpha0, alpha_min=alpha_min, alpha_max=alpha_max,
                             epsilon_one=epsilon_one, epsilon_two=epsilon_two,
                             max_iterations=max_iterations, max_feval=max_feval)


def _iterate_on_device(ctx, label, weights, dictionary, alpha, delta, update_weights,
                       update_dictionary, update_scale_factors, tolerance, max_iterations,
                       verbose, **kwargs):
    """Alternating minimisation loop shared by both forms (reference :399-531, :534-670).
    ``ctx`` already holds the data/kernel matrix."""
    n_components = weights.shape[1]
    require_monotonic = kwargs.get('require_monotonic_cost_decrease', True)
    has_converged = _get_stopping_criteria(kwargs.get('stopping_criterion', 'abs_delta_f'))
    dictionary_solver_kwargs = kwargs.get('dictionary_solver_kwargs', {})
    weights_solver_kwargs = kwargs.get('weights_solver_kwargs', {})
    scale_factors_solver_kwargs = kwargs.get('scale_factors_solver_kwargs', {})

    alpha = np.asarray(alpha, dtype=np.float64)
    ctx.set_state(dictionary, weights, alpha)
    new_cost = ctx.prepare()

    iter_times = []
    cost_deltas = []
    if verbose:
        print("*** {}: n_components = {:d} ***".format(label, n_components))
        print('{:<12s} | {:<13s} | {:<13s} | {:<12s}'.format(
            'Iteration', 'Cost', 'Cost delta', 'Time'))
        print(80 * '-')

    if _DEVICE_LOOP:
        # the loop runs on the device, monotonicity check and stopping rule included (and, for
        # delta != 0, the k-vector scale-factor SPG of reference :243-258 as one small kernel);
        # the host reads one status record per batch of iterations (aa_iterate).  verbose: one
        # batch per call so the table can be printed.
        scale_on = bool(update_scale_factors and delta != 0)
        stop_name = kwargs.get('stopping_criterion', 'abs_delta_f')
        # float32 data (this build's throughput mode): the trace-form cost cancels tr(XX')/n
        # down to the residual, so it carries ~eps_float32 * tr(XX')/n of noise per evaluation;
        # an "increase" inside that band is not one (archetypal_analysis.py:167-174 compares
        # float64 costs, where the band is below every sensible tolerance)
        mono_tol = tolerance
        if ctx.dtype_code == _backend.AA_F32:
            mono_tol = max(tolerance, 8 * 6e-8 * ctx.data_trace() / weights.shape[0])
        n_iter = -1
        done = False
        while not done and n_iter + 1 < max_iterations:
            budget = max_iterations - (n_iter + 1)
            chunk = min(budget, _DEVICE_LOOP_BATCH) if verbose else budget
            start_time = time.perf_counter()
            costs, st = ctx.iterate(new_cost, chunk, tolerance, stop_name, require_monotonic,
                                    update_dictionary, update_weights, dictionary_solver_kwargs,
                                    weights_solver_kwargs, check_every=_DEVICE_LOOP_BATCH,
                                    mono_tolerance=mono_tol, delta=delta if scale_on else 0.0,
                                    scale_kw=scale_factors_solver_kwargs if scale_on else None)
            elapsed = time.perf_counter() - start_time
            ran = max(st.reserved, 1)
            per_iter = elapsed / ran
            if update_dictionary:
                _warn_from_spg_flags(st)
            if st.error_stage:
                raise RuntimeError('factorization cost increased after {} update'.format(
                    {1: 'dictionary', 2: 'weights', 3: 'scale factors'}[st.error_stage]))
            starts = np.concatenate(([new_cost], costs[1::2][:-1]))
            finals = costs[1::2]
            for j in range(st.n_iter + 1):
                iter_times.append(per_iter)
                cost_deltas.append(finals[j] - starts[j])
                if verbose:
                    print('{:12d} | {: 12.6e} | {: 12.6e} | {: 12.6e}'.format(
                        n_iter + 2 + j, finals[j], finals[j] - starts[j], per_iter))
            n_iter += st.n_iter + 1
            new_cost = st.cost
            if st.converged:
                if verbose:
                    print('*** Converged at iteration {:d} ***'.format(n_iter + 1))
                done = True
        dictionary, weights, alpha = ctx.get_state()
        return (weights, dictionary, alpha, new_cost, n_iter, np.mean(iter_times), cost_deltas)

    # the same loop driven from the host one update at a time (scale factors with the generic
    # host spg): kept as the cross-check of the device loop (tests set _DEVICE_LOOP = False)
    n_iter = -1
    for n_iter in range(max_iterations):
        start_time = time.perf_counter()
        old_cost = new_cost

        if update_scale_factors and delta != 0:
            ZtZ, CKCt, CKZ, trace = ctx.grams()
            alpha = _update_kernel_aa_scale_factors(alpha, trace, CKZ, ZtZ, CKCt, delta,
                                                    **scale_factors_solver_kwargs)
            new_cost = _scaled_cost(ctx, alpha)
            _check_if_cost_increased(old_cost, new_cost, tolerance, 'scale factors',
                                     require_decrease=require_monotonic)

        if update_dictionary:
            stats = ctx.dictionary_update(**dictionary_solver_kwargs)
            _warn_from_spg_flags(stats)
            new_cost = ctx.cost()
            _check_if_cost_increased(old_cost, new_cost, tolerance, 'dictionary',
                                     require_decrease=require_monotonic)

        if update_weights:
            ctx.weights_update(**weights_solver_kwargs)
            new_cost = ctx.cost()
            _check_if_cost_increased(old_cost, new_cost, tolerance, 'weights',
                                     require_decrease=require_monotonic)

        end_time = time.perf_counter()
        iter_times.append(end_time - start_time)
        cost_deltas.append(new_cost - old_cost)
        if verbose:
            print('{:12d} | {: 12.6e} | {: 12.6e} | {: 12.6e}'.format(
                n_iter + 1, new_cost, new_cost - old_cost, end_time - start_time))
        if has_converged(old_cost, new_cost, tolerance):
            if verbose:
                print('*** Converged at iteration {:d} ***'.format(n_iter + 1))
            break

    dictionary, weights, _ = ctx.get_state()
    return (weights, dictionary, alpha, new_cost, n_iter, np.mean(iter_times), cost_deltas)


def _iterate_kernel_aa(K, weights, dictionary, alpha, delta=0,
                       update_weights=True, update_dictionary=True,
                       update_scale_factors=True, tolerance=1e-6,
                       max_iterations=1000, verbose=0, **kwargs):
    """Iterate kernel AA until convergence (reference :399-531); returns
    ``(weights, dictionary, alpha, cost, n_iter, mean_iter_time, cost_deltas)``."""
    with _backend.Context(dtype=np.float64) as ctx:
        ctx.set_data(np.asarray(K, dtype=np.float64), form=_backend.FORM_KERNEL)
        return _iterate_on_device(ctx, "Kernel AA", weights, dictionary, alpha, delta,
                                  update_weights, update_dictionary, update_scale_factors,
                                  tolerance, max_iterations, verbose, **kwargs)


def _iterate_aa(X, weights, dictionary, alpha, delta=0,
                update_weights=True, update_dictionary=True,
                update_scale_factors=True, tolerance=1e-6,
                max_iterations=1000, verbose=0, **kwargs):
    """Iterate AA until convergence (reference :534-670); same 7-tuple.  ``dtype`` may
    be passed in kwargs ('float64' default = reference arithmetic; 'float32' = MFMA
    throughput mode)."""
    with _backend.Context(dtype=kwargs.pop('dtype', None)) as ctx:
        ctx.set_data(X, form=_backend.FORM_DATA)
        return _iterate_on_device(ctx, "AA", weights, dictionary, alpha, delta,
                                  update_weights, update_dictionary, update_scale_factors,
                                  tolerance, max_iterations, verbose, **kwargs)


def _transform_hessian(ctx, alpha):
    """A = D K D' (k x k, D = diag(alpha) C) of KernelAA.transform, from the device's C K C' of the final
    dictionary (the Hessian of the weights QPs, archetypal_analysis.py:369-396)."""
    alpha = np.asarray(alpha, dtype=np.float64)
    return alpha[:, np.newaxis] * ctx.grams()[1] * alpha[np.newaxis, :]


def _fit_on_data_matrix(self, data, linear_kernel, label, dictionary=None, weights=None, alpha=None,
                        update_dictionary=True, update_weights=True, update_scale_factors=True,
                        **kwargs):
    """Body of ``ArchetypalAnalysis._aa`` (reference :1036-1118) and of ``KernelAA`` on the
    implicit linear kernel (``linear_kernel``: the data matrix stands in for K = X X')."""
    on_device = isinstance(data, DeviceData)      # preprocessed on the GPU (preprocessing.py)
    if not on_device:
        data = np.asarray(data)
    n_samples = data.shape[0]
    if self.n_components is None:
        self.n_components = data.shape[1]
        self._n_components_defaulted_from = 'n_features'
    self._check_hyper_parameters()
    shape_only = _ShapeOnly(n_samples)
    if (kwargs.get('_draw_only', False) and self.init == 'random' and not on_device and dictionary is None
            and weights is None and alpha is None and update_dictionary and update_weights):
        # restarts.fit_restarts: the start factors of a random start need no device (and no checksum of
        # the data matrix per restart)
        return self._resolve_factors(
            n_samples, None, None, None, True, True,
            lambda: _initialize_kernel_aa_dictionary(shape_only, self.n_components, init='random',
                                                     random_state=self.random_state),
            lambda: _initialize_kernel_aa_weights(shape_only, self.n_components, init='random',
                                                  random_state=self.random_state))

    # the data matrix stays on the device between fits of the same array (the drivers' n_init
    # restarts, bin/run_hadisst_aa.py:158-172): only the start factors travel
    # one process per GPU (torch.distributed.run) with CONVEX_DIM_RED_DISTRIBUTED=1: this rank keeps
    # its row block of the data, RCCL all-reduces the Gram products, every rank gets the full factors
    distributed = _backend.distributed_env() is not None and not on_device
    draw_ctx = kwargs.get('_draw_ctx') if kwargs.get('_draw_only', False) else None
    with (_backend.borrowed(draw_ctx) if draw_ctx is not None else      # fit_restarts: one context for all draws
          data.borrow() if on_device else
          _backend.sharded_context(data, form=_backend.FORM_DATA, dtype=self.dtype) if distributed else
          _backend.resident_context(data, form=_backend.FORM_DATA, dtype=self.dtype)) as ctx:

        def init_dictionary():
            init = 'furthest_sum' if self.init is None else self.init
            if init == 'furthest_sum':
                rng = self.random_state
                start_index = kwargs.get('start_index', None)
                if start_index is None:
                    start_index = rng.randint(n_samples)
                exclude = kwargs.get('exclude', None)
                if exclude is None:
                    exclude = np.array([], dtype='i8')
                columns = kwargs['_cache'].setdefault('distance_columns', {}) if '_cache' in kwargs else None
                selected = _furthest_sum_on_device(
                    ctx, n_samples, self.n_components, start_index,
                    kwargs.get('n_extra_steps', 10), exclude, cache=columns)
                return _one_hot_rows(selected, n_samples, np.float64)
            return _initialize_kernel_aa_dictionary(shape_only, self.n_components, init=init,
                                                    random_state=self.random_state)

        dictionary, weights, alpha = self._resolve_factors(
            n_samples, dictionary, weights, alpha, update_dictionary, update_weights,
            init_dictionary,
            lambda: _initialize_kernel_aa_weights(shape_only, self.n_components,
                                                  init=self.init,
                                                  random_state=self.random_state))
        if kwargs.get('_draw_only', False):      # restarts.fit_restarts: start factors only
            return dictionary, weights, alpha
        self.weights = weights.copy()
        self.dictionary = dictionary.copy()
        self.alpha = alpha.copy()

        ctx.set_linear_kernel(linear_kernel)         # the context may be a reused one
        result = _iterate_on_device(
            ctx, label, self.weights, self.dictionary, self.alpha, self.delta,
            update_weights, update_dictionary, update_scale_factors, self.tolerance,
            self.max_iterations, self.verbose, **self._solver_kwargs())
        out = self._finish(result)
        self._cx = ctx.archetypes()
        if linear_kernel:                        # KernelAA.transform: C K C' of the final dictionary
            self._ckct = ctx.grams()[1]
    return out


# ----------------------------------------------------------------------------
# estimators
# ----------------------------------------------------------------------------
class _BaseAA(object):
    _whom = '_kernel_aa'

    def __init__(self, n_components, delta=0, init=None,
                 tolerance=1e-6, max_iterations=1000, verbose=0,
                 random_state=None, **kwargs):
        self.n_components = n_components
        self.delta = delta
        self.init = init
        self.tolerance = tolerance
        self.max_iterations = max_iterations
        self.verbose = verbose
        self.random_state = check_random_state(random_state)
        self.require_monotonic_cost_decrease = kwargs.get('require_monotonic_cost_decrease', True)
        self.stopping_criterion = kwargs.get('stopping_criterion', 'abs_delta_f')
        self.dtype = kwargs.get('dtype', None)          # MI355X build: 'float64' | 'float32'

        self.weights = None
        self.dictionary = None
        self.alpha = None
        self.cost = 0
        self.n_iter = 0
        self.avg_time_per_iter = 0
        self.cost_deltas = None

        self.weights_solver_kwargs = kwargs.get('weights_solver_kwargs', {})
        self.dictionary_solver_kwargs = kwargs.get('dictionary_solver_kwargs', {})
        self.scale_factors_solver_kwargs = kwargs.get('scale_factors_solver_kwargs', {})

    def _check_hyper_parameters(self):
        if not isinstance(self.n_components, INTEGER_TYPES) or self.n_components <= 0:
            raise ValueError('Number of components must be a positive integer;'
                             ' got (n_components=%r)' % self.n_components)
        _backend.check_component_count(self.n_components, self._whom,
                                       getattr(self, '_n_components_defaulted_from', None))
        if not isinstance(self.max_iterations, INTEGER_TYPES) or self.max_iterations <= 0:
            raise ValueError('Maximum number of iterations must be a positive '
                             'integer; got (max_iterations=%r)' % self.max_iterations)
        if not isinstance(self.tolerance, numbers.Number) or self.tolerance < 0:
            raise ValueError('Tolerance for stopping criteria must be '
                             'positive; got (tolerance=%r)' % self.tolerance)

    def _resolve_factors(self, n_samples, dictionary, weights, alpha, update_dictionary,
                         update_weights, init_dictionary, init_weights):
        """Initialisation dispatch of the reference (:799-830, :1047-1078); the two
        callables produce a dictionary / weights from ``self.random_state``."""
        k = self.n_components
        whom = self._whom
        if self.init == 'custom':
            _check_init_weights(weights, (n_samples, k), '%s (input weights)' % whom)
            _check_init_dictionary(dictionary, (k, n_samples), '%s (input dictionary)' % whom)
            _check_init_scale_factors(alpha, self.delta, (k,), '%s (input scale factors)' % whom)
        elif not update_dictionary and update_weights:
            _check_init_dictionary(dictionary, (k, n_samples), '%s (input dictionary)' % whom)
            weights = init_weights()
        elif update_dictionary and not update_weights:
            _check_init_weights(weights, (n_samples, k), '%s (input weights)' % whom)
            dictionary = init_dictionary()
        else:
            dictionary = init_dictionary()
            weights = init_weights()
        if alpha is None:
            alpha = _initialize_kernel_aa_scale_factors_random(
                k, delta=self.delta, random_state=self.random_state)
        else:
            _check_init_scale_factors(alpha, self.delta, (k,), '%s (input scale factors)' % whom)
        return dictionary, weights, alpha

    def _solver_kwargs(self):
        return dict(require_monotonic_cost_decrease=self.require_monotonic_cost_decrease,
                    stopping_criterion=self.stopping_criterion,
                    weights_solver_kwargs=self.weights_solver_kwargs,
                    dictionary_solver_kwargs=self.dictionary_solver_kwargs,
                    scale_factors_solver_kwargs=self.scale_factors_solver_kwargs)

    def _finish(self, result):
        (self.weights, self.dictionary, self.alpha, cost, n_iter, avg_time, cost_deltas) = result
        if n_iter == self.max_iterations and self.tolerance > 0:
            warnings.warn('Maximum number of iterations %d reached.' % self.max_iterations,
                          UserWarning)
        return cost, n_iter, avg_time, cost_deltas


def _poly_kernel_values(dots, gamma, coef0, degree):
    """``(gamma dots + coef0)^degree`` by repeated multiplication, in the order of the device (poly_kappa)."""
    base = gamma * np.asarray(dots, dtype=np.float64) + coef0
    out = base.copy()
    for _ in range(degree - 1):
        out = out * base
    return out


@contextlib.contextmanager
def _float64_rows(data):
    """A float64 context whose data matrix holds the rows of ``data``, which the kernel-form entry points need:
    a host array is uploaded, a float64 ``DeviceData`` lends its own context (as ``score`` borrows it), a float32
    one is widened on the device into a copy that lives as long as the ``with`` block (``take``, exact)."""
    if not isinstance(data, DeviceData):
        with _backend.Context(dtype=np.float64) as ctx:
            ctx.set_data(data, form=_backend.FORM_DATA)
            yield ctx
    elif data.dtype == np.float64:
        with data.borrow() as ctx:
            yield ctx
    else:
        with data.take(None, dtype=np.float64) as wide:
            with wide.borrow() as ctx:
                yield ctx


def _kernel_spec(which, features, gamma, kwargs):
    """The feature-space kernel a ``KernelAA.fit_transform`` call names, checked: None for the linear kernel
    (explicit matrix or ``features=True``), else ``dict(form=, gamma=[, coef0=, degree=])`` with ``gamma``
    None for the default.  Pops ``degree`` / ``coef0`` from ``kwargs``; every refusal is a ValueError."""
    given = [name for name in ('degree', 'coef0') if name in kwargs]
    degree = kwargs.pop('degree', 3)
    coef0 = kwargs.pop('coef0', 1)
    if which not in ('linear', 'rbf', 'poly'):
        raise ValueError("kernel must be 'linear', 'rbf' or 'poly' (the last two with features=True); got %r"
                         % (which,))
    if which != 'poly' and given:
        raise ValueError("%s belong%s to kernel='poly'; got kernel=%r"
                         % (' and '.join(given), 's' if len(given) == 1 else '', which))
    if which != 'linear' and not features:
        raise ValueError("kernel=%r is computed from the features: pass them with features=True" % (which,))
    if which == 'linear':
        return None
    if which == 'rbf':
        return dict(form='rbf', gamma=gamma)
    if isinstance(degree, (bool, np.bool_)) or not isinstance(degree, (int, np.integer)) or degree < 1:
        raise ValueError("degree must be an integer >= 1; got %r" % (degree,))
    if gamma is not None and not (np.isfinite(gamma) and gamma > 0):
        raise ValueError("gamma must be positive and finite; got %r" % (gamma,))
    if not (np.isfinite(coef0) and coef0 >= 0):
        raise ValueError("coef0 must be >= 0 and finite (the polynomial kernel is then positive semi-definite); "
                         "got %r" % (coef0,))
    return dict(form='poly', gamma=None if gamma is None else float(gamma), coef0=float(coef0), degree=int(degree))


class KernelAA(_BaseAA):
    """Kernel archetypal analysis on a given kernel matrix (reference :673-910).

    Parameters and attributes are those of the reference class: ``n_components``,
    ``delta``, ``init`` (None | 'random' | 'furthest_sum' | 'custom'), ``tolerance``,
    ``max_iterations``, ``verbose``, ``random_state`` and the keyword dictionaries
    ``weights_solver_kwargs``, ``dictionary_solver_kwargs``,
    ``scale_factors_solver_kwargs``, ``require_monotonic_cost_decrease``,
    ``stopping_criterion``; after fitting: ``weights``, ``dictionary``, ``alpha``,
    ``cost``, ``n_iter``, ``avg_time_per_iter``, ``cost_deltas``.
    """
    _whom = '_kernel_aa'

    def _kernel_aa(self, kernel, dictionary=None, weights=None, alpha=None,
                   update_dictionary=True, update_weights=True,
                   update_scale_factors=True, **kwargs):
        self.__dict__.pop('_transform_state', None)      # a failed fit leaves nothing to transform with
        features = kwargs.pop('features', False)
        which = kwargs.pop('feature_kernel', 'linear')
        gamma = kwargs.pop('gamma', None)
        spec = _kernel_spec(which, features, gamma, kwargs)     # ValueErrors before any device call
        if spec is not None:
            return self._kernel_aa_implicit(kernel, spec, dictionary, weights, alpha, update_dictionary,
                                            update_weights, update_scale_factors, **kwargs)
        if features:
            # `kernel` is the n x p feature matrix X (or a DeviceData) of the linear
            # kernel K = X X', which is never formed -- n = 100 000 would be 80 GB.  Same
            # algorithm, conventions and RNG order as the explicit-kernel path below; FurthestSum
            # runs on ||x_i - x_j||^2 = K_ii - 2 K_ij + K_jj computed from X.
            if self.n_components is None:
                self.n_components = kernel.shape[0]
                self._n_components_defaulted_from = 'n_samples'
            out = _fit_on_data_matrix(self, kernel, True, "Kernel AA", dictionary, weights, alpha,
                                      update_dictionary, update_weights, update_scale_factors,
                                      **kwargs)
            cx = self.__dict__.pop('_cx')
            ckct = self.__dict__.pop('_ckct')
            alpha_ = np.asarray(self.alpha, dtype=np.float64)
            self._transform_state = dict(
                form='linear', n_samples=kernel.shape[0], n_features=kernel.shape[1],
                A=alpha_[:, np.newaxis] * ckct * alpha_[np.newaxis, :],
                archetypes=alpha_[:, np.newaxis] * cx)                  # D X, k x p
            return out
        kernel = np.asarray(kernel)
        n_samples = kernel.shape[0]
        if kernel.shape[1] != n_samples:
            raise ValueError('Expected square kernel matrix in %s. '
                             'Got shape %s' % ('kernel_aa', kernel.shape))
        if self.n_components is None:
            self.n_components = n_samples
            self._n_components_defaulted_from = 'n_samples'
        self._check_hyper_parameters()

        dictionary, weights, alpha = self._resolve_factors(
            n_samples, dictionary, weights, alpha, update_dictionary, update_weights,
            lambda: _initialize_kernel_aa_dictionary(kernel, self.n_components, init=self.init,
                                                     random_state=self.random_state, **kwargs),
            lambda: _initialize_kernel_aa_weights(kernel, self.n_components, init=self.init,
                                                  random_state=self.random_state))
        self.weights = weights.copy()
        self.dictionary = dictionary.copy()
        self.alpha = alpha.copy()

        # _iterate_kernel_aa, with the context kept open for the Hessian of transform()
        with _backend.Context(dtype=np.float64) as ctx:
            ctx.set_data(np.asarray(kernel, dtype=np.float64), form=_backend.FORM_KERNEL)
            result = _iterate_on_device(
                ctx, "Kernel AA", self.weights, self.dictionary, self.alpha, self.delta, update_weights,
                update_dictionary, update_scale_factors, self.tolerance, self.max_iterations, self.verbose,
                **self._solver_kwargs())
            state = dict(form='kernel', n_samples=n_samples, A=_transform_hessian(ctx, result[2]))
        out = self._finish(result)
        self._transform_state = state
        return out

    def _kernel_aa_implicit(self, X, spec, dictionary, weights, alpha, update_dictionary, update_weights,
                            update_scale_factors, **kwargs):
        """SURVEY 8(f4), the alternative it names: a feature-space kernel of the rows of ``X``, never formed --
        the RBF kernel ``exp(-gamma ||x_i - x_j||^2)`` or the polynomial kernel ``(gamma x_i.x_j + coef0)^degree``
        (``spec``: _kernel_spec).  The kernel form of the algorithm (reference :399-531, :673-910)
        with every product ``C K`` / ``K Z`` computed as one fused pass over the features
        (aa_set_rbf_features, aa_set_poly_features).  Same conventions, initialisers and RNG order as the
        explicit-kernel path: ``KernelAA(...).fit_transform(rbf_kernel(X, gamma=g))`` is what it reproduces
        (tests/test_gpu_parity.py::test_kernel_aa_on_the_implicit_rbf_kernel, tests/test_gpu_kernel_poly.py)."""
        # a DeviceData stays where it is: the feature buffer is filled from the resident block
        # (aa_set_*_features_resident) and only the few support rows transform() keeps come back
        on_device = isinstance(X, DeviceData)
        if not on_device:
            X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError('Expected a feature matrix (n_samples x n_features); got shape %s' % (X.shape,))
        spec = dict(spec)
        if spec['gamma'] is None:
            spec['gamma'] = 1.0 / X.shape[1]              # scikit-learn's default for both kernels
        gamma = spec['gamma']
        n_samples = X.shape[0]
        if self.n_components is None:
            self.n_components = n_samples
            self._n_components_defaulted_from = 'n_samples'
        self._check_hyper_parameters()
        shape_only = _ShapeOnly(n_samples)
        with contextlib.ExitStack() as stack:
            if on_device:
                owner = stack.enter_context(X.borrow())
                ctx = stack.enter_context(_backend.Context(dtype=np.float64, device=owner.device))
                ctx.set_kernel_features(spec, owner)
            else:
                ctx = stack.enter_context(_backend.Context(dtype=np.float64))
                ctx.set_kernel_features(spec, X)

            def init_dictionary():
                init = 'furthest_sum' if self.init is None else self.init
                if init == 'furthest_sum':
                    rng = self.random_state
                    start_index = kwargs.get('start_index', None)
                    if start_index is None:
                        start_index = rng.randint(n_samples)
                    exclude = kwargs.get('exclude', None)
                    if exclude is None:
                        exclude = np.array([], dtype='i8')
                    selected = _furthest_sum_on_device(ctx, n_samples, self.n_components, start_index,
                                                       kwargs.get('n_extra_steps', 10), exclude)
                    return _one_hot_rows(selected, n_samples, np.float64)
                return _initialize_kernel_aa_dictionary(shape_only, self.n_components, init=init,
                                                        random_state=self.random_state)

            dictionary, weights, alpha = self._resolve_factors(
                n_samples, dictionary, weights, alpha, update_dictionary, update_weights, init_dictionary,
                lambda: _initialize_kernel_aa_weights(shape_only, self.n_components, init=self.init,
                                                      random_state=self.random_state))
            self.weights = weights.copy()
            self.dictionary = dictionary.copy()
            self.alpha = alpha.copy()
            result = _iterate_on_device(
                ctx, "Kernel AA", self.weights, self.dictionary, self.alpha, self.delta, update_weights,
                update_dictionary, update_scale_factors, self.tolerance, self.max_iterations, self.verbose,
                **self._solver_kwargs())
            A = _transform_hessian(ctx, result[2])
        out = self._finish(result)
        # transform() needs the training rows in the support of D = diag(alpha) C only
        D = np.asarray(self.alpha, dtype=np.float64)[:, np.newaxis] * self.dictionary
        support = np.flatnonzero(np.any(D != 0, axis=0))
        if on_device:
            with X.take(support) as rows:                               # s x p values cross the bus, not n x p
                support_rows = np.ascontiguousarray(rows.to_host())
        else:
            support_rows = np.ascontiguousarray(X[support])
        self._transform_state = dict(form=spec['form'], n_samples=n_samples, n_features=X.shape[1], A=A,
                                     gamma=float(gamma), support=support,
                                     support_rows=support_rows,
                                     support_dictionary=np.ascontiguousarray(D[:, support]))
        if spec['form'] == 'poly':
            self._transform_state.update(coef0=spec['coef0'], degree=spec['degree'])
        return out

    def fit_transform(self, data, dictionary=None, weights=None, alpha=None, **kwargs):
        """Factorise the kernel matrix ``data`` (n x n) and return the weights.  With
        ``features=True`` (an extension of the reference's signature) ``data`` is the n x p
        feature matrix of the linear kernel ``data.dot(data.T)`` -- or, with ``kernel='rbf',
        gamma=g``, of the RBF kernel ``exp(-g ||x_i - x_j||^2)``, or, with ``kernel='poly', degree=3,
        gamma=None, coef0=1`` (scikit-learn's ``polynomial_kernel`` and its defaults, ``gamma = 1 /
        n_features``), of the polynomial kernel ``(gamma x_i.x_j + coef0)^degree`` -- which is then never
        formed."""
        if 'kernel' in kwargs:                 # (`kernel` is also the name of _kernel_aa's first argument)
            kwargs['feature_kernel'] = kwargs.pop('kernel')
        self.cost, self.n_iter, self.avg_time_per_iter, self.cost_deltas = self._kernel_aa(
            data, dictionary=dictionary, weights=weights, alpha=alpha, **kwargs)
        return self.weights

    def fit(self, kernel, **kwargs):
        self.fit_transform(kernel, **kwargs)
        return self

    def transform(self, data, diagonal=None):
        """Weights of new samples for the fitted model, and their cost: the per-sample simplex QPs of
        ``ArchetypalAnalysis.transform`` (reference :1151-1199, which writes them in kernel form) with
        ``A = D K D'`` and ``b_y = -D kappa(X, y)``, ``D = diag(alpha) C``, from fresh random starting weights
        (``self.random_state``), ``max_iterations`` SPG passes at most; the cost is
        ``0.5 sum_y (kappa(y, y) + 2 w_y.b_y + w_y' A w_y) / m`` (the kernel-form cost, reference :200-217).

        ``data`` is what the model was fitted on, for the new samples:
          * an explicit kernel matrix: the cross kernel ``kappa(Y, X)`` (m x n_samples), with ``diagonal``
            = ``kappa(y, y)`` (m values, required);
          * ``features=True``: the new feature rows Y (m x n_features) -- linear kernel: ``Y (D X)'`` as in
            ``ArchetypalAnalysis.transform`` and the cost ``0.5 ||Y - W D X||^2 / m``; ``kernel='rbf'``: the RBF
            values against the training rows in the support of D on the f64 matrix cores (aa_rbf_cross),
            the m x n cross kernel never formed; ``kernel='poly'``: the same with the polynomial kernel
            (aa_poly_cross) and ``kappa(y, y) = (gamma |y|^2 + coef0)^degree``.  The rows may be a ``DeviceData``:
            a float64 block lends its context, a float32 one is widened on the device (exact), the draws and the
            weights are those of ``transform(data.to_host())``; the polynomial diagonal then comes from row norms
            computed on the device (aa_kernel_sample_residuals), so that cost differs from the host array's at
            rounding level.
        Returns ``(weights, cost)``; ``weights`` is also stored in ``self.weights``."""
        state = getattr(self, '_transform_state', None)
        if state is None:
            raise NotFittedError('This KernelAA instance is not fitted yet: call fit or fit_transform '
                                 'before transform')
        data, diagonal = self._kernel_arguments('transform', state, data, diagonal)
        on_device = isinstance(data, DeviceData)
        form = state['form']
        m, k = data.shape[0], self.n_components
        kw = dict(self.weights_solver_kwargs)
        kw['max_iterations'] = self.max_iterations            # reference :1194
        A = state['A']
        initial_weights = right_stochastic_matrix((m, k), random_state=self.random_state)
        with _float64_rows(data) as ctx:
            self._set_linear_terms(ctx, state, initial_weights)
            ctx.gpnh_weights_update(A, **kw)
            self.weights = ctx.gpnh_get_weights()
            if form == 'linear':
                cost = ctx.gpnh_residual_cost()                             # 0.5 ||Y - W D X||^2 / m
            elif form == 'poly' and on_device:
                # kappa(y, y) from row norms computed on the device: the block is not downloaded for a diagonal
                cost = 0.5 * ctx.kernel_sample_residuals(A, 'poly', samples=False, diagonal=False)[2] / m
            else:
                if form == 'poly':
                    diagonal = _poly_kernel_values((data * data).sum(axis=1), state['gamma'], state['coef0'],
                                                   state['degree'])       # kappa(y, y)
                cost = ctx.kernel_transform_cost(A, diagonal)
        return self.weights, cost

    def _kernel_arguments(self, method, state, data, diagonal):
        """Host-side checks of ``transform`` and ``kernel_scores`` (before any device call and before anything is
        drawn): what ``data`` and ``diagonal`` have to be for the fitted form.  Returns ``(data, diagonal)``, a host
        array as float64."""
        form = state['form']
        if isinstance(data, DeviceData):
            if form == 'kernel':
                raise TypeError('KernelAA.%s takes a host array, not DeviceData' % method)
        else:
            data = np.asarray(data, dtype=np.float64)
        width, what = ((state['n_samples'], 'the cross kernel kappa(Y, X_train): one column per training sample')
                       if form == 'kernel' else
                       (state['n_features'], 'the feature rows of the new samples'))
        if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != width:
            raise ValueError('KernelAA.%s: expected %s, an (m, %d) array with m >= 1; got shape %s'
                             % (method, what, width, tuple(data.shape)))
        m = data.shape[0]
        if form == 'kernel':
            if diagonal is None:
                raise ValueError('KernelAA.%s: `diagonal` (kappa(y, y) of the %d new samples) is required '
                                 'for a model fitted on an explicit kernel matrix' % (method, m))
            diagonal = np.asarray(diagonal, dtype=np.float64)
            if diagonal.shape != (m,):
                raise ValueError('KernelAA.%s: `diagonal` must hold %d values (one per row of data); '
                                 'got shape %s' % (method, m, diagonal.shape))
        elif diagonal is not None:
            raise ValueError('KernelAA.%s: `diagonal` is only taken for a model fitted on an explicit '
                             'kernel matrix; with features=True it follows from the features' % method)
        return data, diagonal

    def _set_linear_terms(self, ctx, state, weights):
        """The linear terms ``XW = kappa(Y, X_train) D'`` of the rows resident in ``ctx`` (m x k, what the QPs
        and the kernel-form costs read) and the weights ``weights``, in the call order of ``transform``."""
        form, k = state['form'], self.n_components
        if form == 'kernel':
            D = np.asarray(self.alpha, dtype=np.float64)[:, np.newaxis] * self.dictionary
            ctx.gpnh_set_factors(k, W=D.T, Z=weights)                       # kappa(Y, X) D'
        elif form == 'linear':
            ctx.gpnh_set_factors(k, W=state['archetypes'].T, Z=weights)     # Y (D X)'
        else:                                                               # 'rbf', 'poly': the state names the kernel
            ctx.set_kernel_reference(state, state['support_rows'], state['support_dictionary'].T)
            ctx.kernel_cross()                                              # kappa(Y, X_S) D_S'
            ctx.gpnh_set_factors(k, Z=weights)

    def kernel_scores(self, data, weights=None, diagonal=None):
        """Feature-space scores of ``data`` under the fitted model, for every fitted form:
        ``validation.KernelScores`` of the per-sample residuals ``r_t = kappa(y_t, y_t) - 2 w_t.(D kappa(X, y_t)) +
        w_t' A w_t`` -- the cost ``transform`` returns, a feature-space RMSE, the explained fraction
        ``1 - sum r / sum kappa(y, y)`` and both vectors -- from one launch on the device
        (aa_kernel_sample_residuals).  ``data`` and ``diagonal`` are what ``transform`` takes: the cross kernel
        ``kappa(Y, X_train)`` as a host array with ``diagonal`` for a model fitted on an explicit kernel matrix;
        the feature rows, a host array or a ``DeviceData``, without ``diagonal`` for ``features=True``.
        ``weights`` (m x n_components) None: the model's own, as after ``fit_transform`` or ``transform`` of the
        same rows.  No random numbers are drawn."""
        state = getattr(self, '_transform_state', None)
        if state is None:
            raise NotFittedError('This KernelAA instance is not fitted yet: call fit or fit_transform '
                                 'before kernel_scores')
        data, diagonal = self._kernel_arguments('kernel_scores', state, data, diagonal)
        m, k = data.shape[0], self.n_components
        if weights is None:
            weights = self.weights
            if weights is None:
                raise ValueError('KernelAA.kernel_scores: the model holds no weights; pass `weights`')
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != (m, k):
            raise ValueError('KernelAA.kernel_scores: `weights` must be (%d, %d), one row per row of data; got '
                             'shape %s' % (m, k, weights.shape))
        kind = {'kernel': 'given', 'linear': 'linear', 'rbf': 'ones', 'poly': 'poly'}[state['form']]
        with _float64_rows(data) as ctx:
            self._set_linear_terms(ctx, state, weights)
            sample_sse, diag, sum_r, sum_d = ctx.kernel_sample_residuals(state['A'], kind, diag=diagonal)
        return _kernel_scores_from_sums(sample_sse, diag, sum_r, sum_d)

    def score(self, data, weights=None):
        """Reconstruction scores of ``data`` (m x n_features, host array or ``DeviceData``) for a model
        fitted with ``features=True`` on the linear kernel, whose archetypes ``D X`` live in data space:
        ``validation.Scores`` of ``data - weights (D X)`` (``weights`` None: the model's own, as after
        ``fit_transform`` or ``transform``).  Models fitted on an explicit kernel matrix or on the RBF or
        polynomial kernel have no data-space residual (their cost is the kernel form's, see ``transform``)."""
        state = getattr(self, '_transform_state', None)
        if state is None:
            raise NotFittedError('This KernelAA instance is not fitted yet: call fit or fit_transform '
                                 'before score')
        if state['form'] != 'linear':
            raise ValueError("KernelAA.score: a model fitted on %s has no data-space residual; only "
                             "features=True on the linear kernel has (archetypes D X)"
                             % {'kernel': 'an explicit kernel matrix', 'rbf': 'the RBF kernel',
                                'poly': 'the polynomial kernel'}[state['form']])
        data, weights = _score_arguments('KernelAA', data, state['n_features'], self.n_components, weights,
                                         self.weights)
        return _residual_scores(data, np.asarray(state['archetypes'], dtype=np.float64), weights, self.dtype)


class ArchetypalAnalysis(_BaseAA):
    """Standard archetypal analysis ``min ||X - Z C X||_F^2`` (reference :913-1215).

    Same constructor, attributes (plus ``archetypes``) and methods as the reference:
    ``fit_transform(X)``, ``transform(X) -> (weights, cost)``, ``inverse_transform``.
    As in the reference there is no ``fit`` method.  Extra keyword: ``dtype``
    ('float64' default = reference arithmetic, 'float32' = fp32-MFMA throughput mode).
    """
    _whom = '_aa'

    def __init__(self, n_components, delta=0, init=None, tolerance=1e-6, max_iterations=1000,
                 verbose=0, random_state=None, **kwargs):
        super(ArchetypalAnalysis, self).__init__(
            n_components, delta=delta, init=init, tolerance=tolerance,
            max_iterations=max_iterations, verbose=verbose, random_state=random_state, **kwargs)
        self.archetypes = None

    def _aa(self, data, dictionary=None, weights=None, alpha=None,
            update_dictionary=True, update_weights=True, update_scale_factors=True, **kwargs):
        return _fit_on_data_matrix(self, data, False, "AA", dictionary, weights, alpha,
                                   update_dictionary, update_weights, update_scale_factors, **kwargs)

    def fit_transform(self, data, dictionary=None, weights=None, alpha=None, **kwargs):
        """Factorise ``data`` (n_samples x n_features) and return the weights."""
        self.cost, n_iter_, avg_time_, cost_deltas_ = self._aa(
            data, dictionary=dictionary, weights=weights, alpha=alpha, **kwargs)
        cx = self.__dict__.pop('_cx')
        if self.delta != 0:
            self.dictionary = np.dot(np.diag(self.alpha), self.dictionary)
            cx = self.alpha[:, np.newaxis] * cx
        self.archetypes = cx                     # = dictionary.dot(data), reference :1144
        self.n_iter = n_iter_
        self.avg_time_per_iter = avg_time_
        self.cost_deltas = cost_deltas_
        return self.weights

    def transform(self, data):
        """Weights of new samples for the fitted archetypes, and their cost (reference
        :1151-1199): per-sample QPs with A = (CX)(CX)', b_t = -(CX) x_t from fresh random
        starting weights, ``max_iterations`` SPG passes at most, then 0.5 ||X - W (CX)||_F^2 / n.
        One context, one upload: X (CX)' is the row-local GEMM, the QPs and the residual norm run
        on the resident data (csrc/solver.hip: aa_gpnh_set_factors / _weights_update /
        _residual_cost, which are the "data times a k x p dictionary" entry points)."""
        on_device = isinstance(data, DeviceData)
        if not on_device:
            data = np.asarray(data)
            if data.dtype != np.float32:
                data = np.asarray(data, dtype=np.float64)
        n_samples = data.shape[0]
        kw = dict(self.weights_solver_kwargs)
        kw['max_iterations'] = self.max_iterations            # reference :1194
        archetypes = np.asarray(self.archetypes, dtype=np.float64)
        CKCt = archetypes.dot(archetypes.T)                   # k x k
        initial_weights = right_stochastic_matrix((n_samples, self.n_components),
                                                  random_state=self.random_state)
        if on_device:
            manager = data.borrow()
        else:
            manager = _backend.Context(dtype=np.float64 if data.dtype == np.float64 else self.dtype)
        with manager as ctx:
            if not on_device:
                ctx.set_data(data, form=_backend.FORM_DATA)
            ctx.gpnh_set_factors(self.n_components, W=archetypes.T, Z=initial_weights)   # X (CX)'
            ctx.gpnh_weights_update(CKCt, **kw)
            self.weights = ctx.gpnh_get_weights()
            cost = ctx.gpnh_residual_cost()
        return self.weights, cost

    def score(self, data, weights=None):
        """Reconstruction scores of ``data`` (m x n_features, host array or ``DeviceData``) under the
        fitted archetypes: ``validation.Scores`` of ``data - weights . archetypes`` -- the cost
        ``transform`` returns, the drivers' RMSE (``mean_squared_error(data, inverse_transform(weights),
        squared=False)``, bin/run_hadisst_aa.py:230-244), the pooled RMSE and the sums of squares per
        feature and per sample -- from one pass over the matrix on the device (aa_gpnh_residual_scores);
        the reconstruction is never formed.  ``weights`` (m x n_components) None: the model's own, as
        after ``fit_transform`` or ``transform`` of the same rows.  No random numbers are drawn."""
        if self.archetypes is None:
            raise NotFittedError('This ArchetypalAnalysis instance is not fitted yet: call fit_transform '
                                 'before score')
        archetypes = np.asarray(self.archetypes, dtype=np.float64)
        data, weights = _score_arguments('ArchetypalAnalysis', data, archetypes.shape[1], archetypes.shape[0],
                                         weights, self.weights)
        return _residual_scores(data, archetypes, weights, self.dtype)

    def inverse_transform(self, weights):
        return weights.dot(self.archetypes)
