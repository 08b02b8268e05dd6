"""The dictionary's column simplex projection (launch_proj and the kernels behind it in
csrc/kernels_tall.hip) in every strategy, against the exact projection.

The harness feeds the projection exactly known inputs through the existing ABI.  With
aa_set_dictionary_inputs(H, Z'Z = 0, trace) the matrix M = D Z'Z D is zero, so the gradient kernel
computes g = fl(-H fl(1/n)) -- reproduced here bit for bit -- and the gradient does not change during
the update.  With a first step length that is a power of two, w = x - a g is one rounding of an exact
value whether or not the compiler contracts it.  One dictionary_update(max_iterations=1) then returns
C1 = x0 + lambda (P(w) - x0), and the line search accepts lambda = 1 (f is linear in the step); the
tests read lambda, the flags and n_feval back and assert them.  Two scenarios per table row:

  "dir"   C0 has dyadic rows that sum to exactly 1 (PROJ_FEAS returns them bit for bit), H places one
          column class per component in w = x0 - a g, and C1 is P(w) to three roundings
          (fl(w - t), fl(. - x0), fl(x0 + .): at most 1.5 u for entries below 1);
  "feas"  C0 IS the infeasible w, H = 0: PROJ_FEAS projects it, and the update then projects the result
          once more (d = P(x) - x is rounding-sized).  The second projection moves an entry by at most
          its own threshold, |sum x - 1| / m <= the first projection's threshold error + u/2, so this
          scenario is held to twice the threshold bound + 4 u, and its off-support entries may come
          back as rounding-sized positives (a row sum of x below 1 makes the second threshold negative):
          it compares values only, "dir" compares supports too.

The bound ("rounding dust"): a column's device threshold is (s - 1) / m with s a
float64 sum of its m support entries in some order, so
    |t_dev - t*| <= u ((m + 2) sum_supp |w| / m + |t*|),   u = 2^-53,
and an entry differs from max(w - t*, 0) by at most that plus 2 u.  Entries with |w - t*| below the
bound may fall on either side of the support (at most 1 % of a column, checked on the reference alone by
a host-only test); every other entry must have the exact support.  Row sums: the m support entries move
with the threshold, sum_supp (w - t_dev) - 1 = m (t_S - t_dev), and each is rounded once (u / 2 of it),
so |sum P - 1| <= m x threshold bound + u / 2 = u ((m + 2) sum_supp |w| + m |t*| + 1/2): (m + 2) u for a
column with sum_supp |w| = 1 and t* = 0, which is not every column (tail2, m = 2, sum |w| = 1.5: a float64
NumPy projection is off by 5.1 u, more than 4 u), plus u for each of the at most eight entries where
x0 != 0 (the roundings of fl(P - x0) and fl(x0 + d)).  In "feas" the row sum is that of the SECOND
projection, whose input sums to 1 within rounding: (n + 2) u + 2 u whatever the column.

Which strategy ran is read from Context.proj_counts() after every call; whether a list column is
solved in LDS or from global memory is decided on the host from the exact w (#{w > max - 1} against
2048) and asserted for the rows that claim a path.

Two columns of the issue's list are built differently, for reasons the host-only tests pin down:
the geometric column 1 - 2^-i needs three Michelot passes from max - 1 (Michelot's map is a Newton
step), so the "chain" column is built instead so that every pass drops exactly one entry (14 passes
and more: the second batch of the iterative path); and the constant column is 0 (threshold -1/n),
because a constant c != 0 loses (c n) u / 2 to the rounding of t, far more than 2 ulp of 1/n; its
2-ulp check runs where n is a power of two (see _exact_answer).

Figures of the MI355X run: profiles/proj_errors.txt (every GPU test prints a `proj-errors` line with its
largest error / bound ratio)."""
import ctypes

import numpy as np
import pytest

LD = np.longdouble
U = LD(2.0) ** -53                       # unit roundoff of float64

gpu = pytest.mark.gpu
pytestmark = pytest.mark.gpu

LDS_CAP = 2048                           # PROJ_LDS_CAP
P_DATA = 8

DEFAULTS = {"proj_mode": 0, "proj_small": 1, "fin_in_last": 1, "fuse_finalize": 1, "proj_res_side": 1}
# strategy -> (options, counter it must increment, stats struct passed)
STRATEGIES = {
    "small32": ({}, "small32", True),
    "small32_fin0": ({"fin_in_last": 0}, "small32", True),
    "small32_side1": ({}, "small32", False),              # residual projection on the side stream
    "small32_side0": ({"proj_res_side": 0}, "small32", False),
    "small64": ({"proj_small": 2}, "small64", True),
    "list": ({"proj_small": 0}, "list", True),
    "list_default": ({}, "list", True),                   # n > 8192 with the default options
    "list_ps2": ({"proj_small": 2}, "list", True),        # n > 16384 with proj_small = 2
    "list_fin0": ({"proj_small": 0, "fin_in_last": 0}, "list", True),
    "list_nofuse": ({"proj_small": 0, "fuse_finalize": 0}, "list", True),
    "list_side1": ({"proj_small": 0}, "list", False),
    "list_side0": ({"proj_small": 0, "proj_res_side": 0}, "list", False),
    "iter": ({"proj_mode": 1}, "iterative", True),
}
# strategies that must give the bits of their base strategy
SAME_BITS = {"small32_fin0": "small32", "small32_side1": "small32", "small32_side0": "small32",
             "list_fin0": "list", "list_side1": "list", "list_side0": "list"}

CLASSES = ("dense", "c2048", "c2049", "sparse", "allneg", "tied", "const", "onehot0", "onehotN", "tail2",
           "offset", "chain")

# ---------------------------------------------------------------- the shape table
# n, k, strategy, counter, KP, tall blocks, rows per block, list path of the cold "dir" projection
# ("": not a list strategy, "lds" / "global" / "both": what its columns reach), column classes
# (None: all twelve, cycled), dtype
TABLE = []


def _rows(n, k, strategies, kp, tb, rpb, cls=None, path=None, dtype="float64"):
    for s in strategies:
        kind = STRATEGIES[s][1]
        TABLE.append((n, k, s, kind, kp, tb, rpb, (path or "") if kind == "list" else "", cls, dtype))


# every n at k = 2
_rows(1, 2, ("small32", "list", "iter"), 32, 1, 8, ("dense", "sparse"), "lds")
_rows(7, 2, ("small32", "list", "iter"), 32, 1, 8, ("dense", "tied"), "lds")
_rows(255, 2, ("small32", "list", "iter"), 32, 1, 256, ("dense", "tail2"), "lds")
_rows(256, 2, ("small32", "list", "list_fin0", "iter"), 32, 1, 256, ("dense", "onehotN"), "lds")
_rows(257, 2, tuple(s for s in STRATEGIES if s not in ("small64", "list_default", "list_ps2")), 32, 2, 136,
      ("dense", "tail2"), "lds")
_rows(2049, 2, ("small32", "list", "iter"), 32, 9, 232, ("c2048", "c2049"), "both")
_rows(8192, 2, ("small32", "list"), 32, 32, 256, ("dense", "onehotN"), "both")
_rows(8193, 2, ("list_default", "small64", "iter"), 32, 33, 256, ("dense", "tail2"), "both")
_rows(16384, 2, ("small64", "list_default"), 32, 64, 256, ("dense", "onehotN"), "both")
_rows(16385, 2, ("list_ps2",), 32, 65, 256, ("dense", "tail2"), "both")
_rows(65537, 2, ("list_default", "iter"), 32, 256, 264, ("dense", "tail2"), "both")
# every k at n = 257 and n = 8193
_rows(257, 1, ("small32", "list", "iter"), 32, 2, 136, ("chain",), "lds")
_rows(257, 31, ("small32", "list", "iter"), 32, 2, 136, None, "lds")
_rows(257, 32, ("small32", "list", "list_fin0", "iter"), 32, 2, 136, None, "lds")
_rows(257, 33, ("small32", "list", "iter"), 64, 2, 132, None, "lds")
_rows(257, 64, ("small32", "list", "list_fin0", "iter"), 64, 2, 132, None, "lds")
_rows(8193, 1, ("list_default",), 32, 33, 256, ("dense",), "global")
_rows(8193, 31, ("list_default",), 32, 33, 256, None, "both")
_rows(8193, 32, ("list_default", "small64", "iter"), 32, 33, 256, None, "both")
_rows(8193, 33, ("list_default", "small64"), 64, 33, 252, None, "both")
_rows(8193, 64, ("list_default",), 64, 33, 252, None, "both")
# the dyadic columns where 1/n is dyadic too
_rows(256, 3, ("small32", "list", "iter"), 32, 1, 256, ("const", "tied", "onehot0"), "lds")
# all twelve classes at the LDS boundary, and the largest case
_rows(2049, 32, ("small32", "list", "list_nofuse", "iter"), 32, 9, 232, None, "both")
_rows(65537, 32, ("list_default",), 32, 256, 264, None, "both")
# the data dtype does not enter: one float32 context per strategy
_rows(257, 2, ("small32", "list", "iter"), 32, 2, 136, ("dense", "tail2"), "lds", "float32")
_rows(8193, 2, ("small64",), 32, 33, 256, ("dense", "tail2"), "both", "float32")


def _rid(row):
    return "n%d_k%d_%s%s" % (row[0], row[1], row[2], "_f32" if row[9] == "float32" else "")


def _dispatch(n, k, opts):
    """launch_proj's and tall_setup's rules restated: counter, KP, tall blocks, rows per block,
    whether the last block of a pass finalizes its reduction."""
    o = dict(DEFAULTS)
    o.update(opts)
    kp = 32 if k <= 32 else 64
    tb = min(256, max(1, -(-n // 256)))
    rs = 256 // kp
    rpb = -(-(-(-n // tb)) // rs) * rs
    if o["proj_mode"] == 1:
        kind = "iterative"
    elif o["proj_small"] >= 1 and n <= 8192:
        kind = "small32"
    elif o["proj_small"] >= 2 and n <= 16384:
        kind = "small64"
    else:
        kind = "list"
    fin_in_last = bool(o["fin_in_last"] and o["fuse_finalize"] and tb > 1)
    return kind, kp, tb, rpb, fin_in_last


# ---------------------------------------------------------------- inputs
def _chain(n):
    """A column on which every Michelot pass from max - 1 drops exactly one entry: two entries 1 (threshold
    1/2), then w_{j+1} = tau_j - delta_j with tau_j the threshold of the j largest, which is dropped by the
    pass after the one that drops w_{j+2} when delta_{j+1} > delta_j j (j + 2) / (j + 1); delta grows from
    1e-13 by twice that factor.  Everything else lies below max - 1 = 0."""
    w = np.full(n, -1.0)
    vals = [1.0, 1.0]
    tau, delta, j = LD(0.5), LD(1e-13), 2
    while len(vals) < min(n, 14):
        v = tau - delta
        vals.append(float(v))
        tau = (j * tau + v) / (j + 1)
        delta = 2 * delta * j * (j + 2) / (j + 1)
        j += 1
    w[(np.arange(len(vals)) * 17) % n if n >= 17 * len(vals) else np.arange(len(vals))] = vals
    return w


def _column(cls, n, rng):
    if cls == "chain" and n >= 14:
        return _chain(n)
    if cls in ("dense", "chain"):
        return 0.05 + 0.9 * rng.uniform(size=n)
    if cls in ("c2048", "c2049"):
        cnt = 2048 if cls == "c2048" else 2049
        if n <= cnt:
            return 0.5 + 0.5 * rng.uniform(size=n)
        w = -0.5 - rng.uniform(size=n)
        idx = rng.permutation(n)[:cnt]
        w[idx] = 0.5 + 0.49 * rng.uniform(size=cnt)
        w[idx[0]] = 1.0
        return w
    if cls == "sparse":
        w = -1.0 - rng.uniform(size=n)
        idx = rng.permutation(n)[:3]
        w[idx] = np.array([0.9, 0.8, 0.7])[:len(idx)] + 0.01 * rng.uniform(size=len(idx))
        return w
    if cls == "allneg":
        return -3.0 + rng.uniform(size=n)
    if cls == "tied":
        w = np.full(n, -1.0)
        w[rng.permutation(n)[:2]] = 0.75
        return w
    if cls == "const":
        return np.zeros(n)
    if cls in ("onehot0", "onehotN"):
        w = np.zeros(n)
        w[0 if cls == "onehot0" else n - 1] = 2.0
        return w
    if cls == "tail2":
        w = -1.0 - rng.uniform(size=n)
        w[n - 1] = 0.6
        w[max(n - 2, 0)] = 0.9
        return w
    if cls == "offset":
        return 1e6 + 0.5 * rng.uniform(size=n)
    raise ValueError(cls)


def _exact_answer(cls, n, w):
    """Item 4: the known projections of the dyadic columns (None: no closed form)."""
    if cls == "tied":
        return np.where(w == 0.75, 0.5 if n > 1 else 1.0, 0.0)
    if cls == "const":
        # 1/n is dyadic for a power of two only; otherwise the second projection of "feas" sums n copies of
        # fl(1/n) with float64 rounding (28 u at n = 65537) and its threshold, that sum's error / n, is tens
        # of ulp of 1/n: those columns are held to the bound of every other column
        return np.full(n, 1.0 / n) if n & (n - 1) == 0 else None
    if cls in ("onehot0", "onehotN"):
        return np.where(w == 2.0, 1.0, 0.0)
    return None


def _dyadic_simplex(n, k, rng):
    """k columns of n entries, multiples of 2^-10 that sum to exactly 1, at most eight non-zeros."""
    x = np.zeros((n, k))
    for i in range(k):
        q = min(n, 8)
        cuts = np.sort(rng.permutation(1023)[:q - 1] + 1)
        parts = np.diff(np.concatenate(([0], cuts, [1024])))
        x[rng.permutation(n)[:q], i] = parts / 1024.0
    assert np.all(x.sum(axis=0) == 1.0)
    return x


def _gradient(H, n):
    """k_grad with M = 0 and alpha = 1: (0 - H * 1) * scale, scale = 1.0 / n."""
    return -H * (1.0 / n)


_INPUTS = {}


def _inputs(n, k, cls):
    """Everything a table row's runs share, in the tall orientation (n x k): the data X (it only feeds
    P, Q and the line search), the target columns T, the dyadic start x0, H with x0 - g(H) ~ T, and the
    exact w of the "dir" scenario as the device forms it."""
    key = (n, k, cls)
    if key not in _INPUTS:
        rng = np.random.RandomState(7 * n + k)
        names = [(cls or CLASSES)[i % len(cls or CLASSES)] for i in range(k)]
        T = np.stack([_column(c, n, rng) for c in names], axis=1)
        x0 = _dyadic_simplex(n, k, rng)
        H = (T - x0) * float(n)
        w = x0 - 1.0 * _gradient(H, n)
        X = rng.standard_normal((n, P_DATA))
        Z = rng.uniform(size=(n, k))
        Z /= Z.sum(axis=1, keepdims=True)
        for a in (T, x0, H, w, X, Z):
            a.setflags(write=False)
        _INPUTS[key] = dict(names=names, T=T, x0=x0, H=H, w=w, X=X, Z=Z)
    return _INPUTS[key]


# ---------------------------------------------------------------- extended-precision reference
class Ref(object):
    """The exact projection of every column of W (n x k) onto the simplex: thresholds by the sorted scan
    in np.longdouble (simplex_projection.py:14-26), support sizes, the threshold bound of the module
    docstring, and the dust mask under a per-entry bound."""

    def __init__(self, W):
        Wl = np.asarray(W, dtype=LD)
        n = Wl.shape[0]
        srt = -np.sort(-Wl, axis=0)
        css = np.cumsum(srt, axis=0)
        j = np.arange(1, n + 1, dtype=LD)[:, None]
        m = (srt - (css - 1) / j > 0).sum(axis=0)
        self.m = m
        self.t = (css[m - 1, np.arange(Wl.shape[1])] - 1) / m
        self.W = Wl
        self.supp = Wl > self.t
        sabs = np.where(self.supp, np.abs(Wl), 0).sum(axis=0)
        self.tbound = U * ((m + 2) * sabs / m + np.abs(self.t))
        self.P = np.maximum(Wl - self.t, 0)

    def dust(self, bound):
        return np.abs(self.W - self.t) < bound


_REFS = {}


def _ref(key, W):
    if key not in _REFS:
        _REFS[key] = Ref(W)
    return _REFS[key]


def _michelot_passes(w):
    """Passes of the iterative path from max - 1 under POST_MICHELOT's rule."""
    t, prev, shrunk, passes = w.max() - 1.0, 0, False, 0
    while passes < 400:
        S = w > t
        cnt = int(S.sum())
        passes += 1
        conv = prev > 0 and (cnt == prev or (shrunk and cnt > prev))
        if prev > 0 and cnt < prev:
            shrunk = True
        t = (w[S].sum() - 1.0) / cnt if cnt else w.max() - 1.0
        prev = cnt
        if conv:
            break
    return passes


# ---------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def be():
    from convex_dim_red import _backend
    _backend.require_gpu()
    return _backend


def _run(be, X, C0, Z, steps, strategy, dtype="float64"):
    """One context: set_state(C0), then one dictionary_update(max_iterations=1) per (H, alpha0) step.
    Returns per step the fetched dictionary (n x k), the SPG scalars and the projection counters."""
    opts, _, stats = STRATEGIES[strategy]
    n, k = C0.shape
    out = []
    for name, value in opts.items():
        be.set_option(name, value)
    try:
        with be.Context(dtype=dtype) as ctx:
            ctx.set_data(X)
            ctx.set_state(np.ascontiguousarray(C0.T), Z, np.ones(k))
            for H, alpha0 in steps:
                ctx.set_dictionary_inputs(H, np.zeros((k, k)), 0.0)
                kw = dict(max_iterations=1)
                if alpha0 is not None:
                    kw["alpha0"] = alpha0
                if stats:
                    st = ctx.dictionary_update(**kw)
                    n_feval, flags = st.n_feval, st.flags
                else:
                    p = be.spg_params(**kw)
                    be._check(ctx.lib.aa_dictionary_update(ctx.h, ctypes.byref(p), None))
                    n_feval = flags = None
                sc = ctx.spg_scalars()
                if n_feval is None:
                    n_feval, flags = int(sc["n_feval"]), int(sc["flags"]) or 8      # (the host adds the cap flag)
                C1 = np.ascontiguousarray(ctx.get_state()[0].T)
                out.append(dict(C=C1, sc=sc, counts=ctx.proj_counts(), n_feval=n_feval, flags=flags))
    finally:
        for name in opts:
            be.set_option(name, DEFAULTS[name])
    return out


def _expect_counts(kind, total):
    return {name: (total if name == kind else 0) for name in ("small32", "small64", "list", "iterative")}


def _check_preconditions(step, lam=1.0):
    """lambda = 1, one function evaluation in the line search (n_feval: start, trial point, BB stage), the
    flags `converged` (the residual of the step is small) or `iteration cap` and nothing else: no
    projection ran into its pass cap."""
    assert step["sc"]["lambda"] == lam
    assert step["n_feval"] == 3
    assert step["flags"] in (1, 8), step["flags"]


def _check_projection(C1, ref, x0, lam, feas=False, extra=0):
    """Items 1 and 2 for one projection: values within the bound, exact support outside dust ("dir"),
    non-negative, row sums.  Returns the largest error / bound ratio."""
    bound = (2 * ref.tbound + 4 * U if feas else ref.tbound + 2 * U) + extra
    want = ref.P if feas else x0 + LD(lam) * (ref.P - x0)
    err = np.abs(C1.astype(LD) - want)
    assert np.all(err <= bound), "column(s) %s off the exact projection by %s x bound" % (
        np.unique(np.nonzero(err > bound)[1]), float((err / bound).max()))
    dust = ref.dust(bound)
    assert dust.mean(axis=0).max() <= 0.01 or dust.sum(axis=0).max() == 0
    if not feas:
        assert np.array_equal((C1 > 0)[~dust], ref.supp[~dust])
    assert C1.min() >= 0
    rows = np.abs(C1.astype(LD).sum(axis=0) - 1)
    if feas:
        rbound = (C1.shape[0] + 2) * U + 2 * U
    else:
        rbound = ref.m * ref.tbound + U * (1 + (x0 != 0).sum(axis=0))
    assert np.all(rows <= rbound), float((rows / rbound).max())
    return float((err / bound).max())


def _check_scalars(step, x0, g, H, entry_bound_res):
    """Item 3: delta, dd, s1d from d = (C1 - x0) / lambda and res2, resinf from the exact projection of
    C1 - g, all in np.longdouble, within the forward bound of an n k-term float64 sum.  d is recovered from
    C1 = fl(x0 + lambda d), which adds u |C1| per entry; a residual entry carries its projection's entry
    bound."""
    sc, C1 = step["sc"], step["C"].astype(LD)
    nk = LD(C1.size)
    d = (C1 - x0) / LD(sc["lambda"])
    rec = U * np.abs(C1)
    for name, other in (("delta", g.astype(LD)), ("dd", d), ("s1d", H.astype(LD))):
        want = (d * other).sum()
        slack = nk * U * np.abs(d * other).sum() + ((2 if name == "dd" else 1) * rec * np.abs(other)).sum()
        assert abs(LD(sc[name]) - want) <= slack, (name, sc[name], float(want), float(slack))
    rref = Ref(step["C"] - g)
    res = rref.P - C1
    eb = rref.tbound + 2 * U
    slack = nk * U * (res * res).sum() + (2 * np.abs(res) * eb + eb * eb).sum() + 4 * U * (res * res).sum()
    assert abs(LD(sc["res2"]) - (res * res).sum()) <= slack, (sc["res2"], float((res * res).sum()), float(slack))
    assert abs(LD(sc["resinf"]) - np.abs(res).max()) <= 2 * eb.max(), (sc["resinf"], float(np.abs(res).max()))
    return rref


_DEVICE = {}


def _device(be, row):
    """The two scenarios of a table row on the device, run once per session."""
    n, k, strategy, kind, kp, tb, rpb, path, cls, dtype = row
    key = (n, k, strategy, cls, dtype)
    if key not in _DEVICE:
        inp = _inputs(n, k, cls)
        dirs = _run(be, inp["X"], inp["x0"], inp["Z"], [(inp["H"], 1.0)], strategy, dtype)[0]
        feas = _run(be, inp["X"], inp["T"], inp["Z"], [(np.zeros((n, k)), 1.0)], strategy, dtype)[0]
        for step in (dirs, feas):      # which strategy ran: PROJ_FEAS, PROJ_DIR, PROJ_RES, all by the claimed one
            assert step["counts"] == _expect_counts(kind, 3), (strategy, step["counts"])
        _DEVICE[key] = (dirs, feas)
    return _DEVICE[key]


def _report(strategy, what, ratio):
    print("proj-errors %-14s %-28s largest error / bound %.3f" % (strategy, what, ratio))


# ---------------------------------------------------------------- legs 1-4: every row against the exact projection
@pytest.mark.parametrize("row", TABLE, ids=_rid)
def test_projection_against_exact(be, row):
    n, k, strategy, kind, kp, tb, rpb, path, cls, dtype = row
    inp = _inputs(n, k, cls)
    dirs, feas = _device(be, row)
    _check_preconditions(dirs)
    _check_preconditions(feas)
    ref = _ref(("dir", n, k, cls), inp["w"])
    if path:
        cand = (inp["w"] > inp["w"].max(axis=0) - 1.0).sum(axis=0)
        reached = {"lds" if c <= LDS_CAP else "global" for c in cand}
        assert reached == ({"lds", "global"} if path == "both" else {path}), sorted(cand)
    r1 = _check_projection(dirs["C"], ref, inp["x0"].astype(LD), dirs["sc"]["lambda"])
    g = _gradient(inp["H"], n)
    _check_scalars(dirs, inp["x0"].astype(LD), g, inp["H"], None)
    # PROJ_FEAS on its own: d = P(x) - x is rounding-sized, <d, g> and <d, H> vanish with H
    fref = _ref(("feas", n, k, cls), inp["T"])
    r2 = _check_projection(feas["C"], fref, None, 1.0, feas=True)
    assert feas["sc"]["delta"] == 0.0 and feas["sc"]["s1d"] == 0.0
    assert feas["sc"]["dd"] <= float(((fref.tbound + 2 * U) ** 2 * n).sum())
    assert feas["sc"]["resinf"] <= float(2 * (fref.tbound + 2 * U).max())
    # item 4: the dyadic columns
    for i, name in enumerate(inp["names"]):
        exact = _exact_answer(name, n, inp["T"][:, i])
        if exact is not None:
            assert np.all(np.abs(feas["C"][:, i] - exact) <= 2 * np.spacing(exact)), (name, i)
    _report(strategy, _rid(row), max(r1, r2))


# ---------------------------------------------------------------- leg 5: strategies agree
def _groups():
    seen = {}
    for row in TABLE:
        if row[9] == "float64":
            seen.setdefault((row[0], row[1], row[8]), []).append(row)
    return [rows for rows in seen.values() if len(rows) > 1]


@pytest.mark.parametrize("rows", _groups(), ids=lambda rows: "n%d_k%d" % rows[0][:2])
def test_strategies_agree(be, rows):
    n, k, cls = rows[0][0], rows[0][1], rows[0][8]
    ref = _ref(("dir", n, k, cls), _inputs(n, k, cls)["w"])
    fref = _ref(("feas", n, k, cls), _inputs(n, k, cls)["T"])
    got = {row[2]: _device(be, row) for row in rows}
    worst = 0.0
    for a in got:
        for b in got:
            if a >= b:
                continue
            for s, r, bound in ((0, ref, ref.tbound + 2 * U), (1, fref, 2 * fref.tbound + 4 * U)):
                diff = np.abs(got[a][s]["C"].astype(LD) - got[b][s]["C"])
                assert np.all(diff <= bound), (a, b, s)
                worst = max(worst, float((diff / bound).max()))
                if s == 0:
                    dust = r.dust(bound)
                    assert np.array_equal((got[a][s]["C"] > 0)[~dust], (got[b][s]["C"] > 0)[~dust])
    for s, base in SAME_BITS.items():
        if s in got and base in got:
            for sc in (0, 1):
                assert np.array_equal(got[s][sc]["C"], got[base][sc]["C"]), (s, base)
                if STRATEGIES[s][2]:
                    assert got[s][sc]["sc"] == got[base][sc]["sc"], (s, base)
                else:      # no stats struct: the same SPG iteration, scalar for scalar
                    for name in ("lambda", "delta", "dd", "s1d", "res2", "resinf", "n_feval"):
                        assert got[s][sc]["sc"][name] == got[base][sc]["sc"][name], (s, base, name)
    _report("agree", "n%d_k%d (%d strategies)" % (n, k, len(got)), worst)


@pytest.mark.parametrize("strategy", ["small32", "list", "iter"])
def test_fresh_context_repeats_the_bits(be, strategy):
    row = next(r for r in TABLE if r[:3] == (2049, 32, strategy))
    inp = _inputs(2049, 32, None)
    first = _device(be, row)[0]
    again = _run(be, inp["X"], inp["x0"], inp["Z"], [(inp["H"], 1.0)], strategy)[0]
    assert np.array_equal(first["C"], again["C"]) and first["sc"] == again["sc"]
    assert again["counts"] == _expect_counts(row[3], 3)


@pytest.mark.parametrize("row", [r for r in TABLE if r[9] == "float32"], ids=_rid)
def test_data_dtype_does_not_enter(be, row):
    twin = next(r for r in TABLE if r[:3] == row[:3] and r[9] == "float64")
    for a, b in zip(_device(be, row), _device(be, twin)):
        assert np.array_equal(a["C"], b["C"])
        assert a["counts"] == b["counts"]


# ---------------------------------------------------------------- the first step length (PROJ_ALPHA)
@pytest.mark.parametrize("strategy,n", [("small32", 257), ("list", 257), ("iter", 257), ("small64", 8193),
                                        ("list_default", 8193)])
def test_default_first_step(be, strategy, n):
    """alpha0 left to the solver: PROJ_ALPHA projects x0 - g and the step is 1 / max|P(x0 - g) - x0|.  The
    step alpha that PROJ_DIR used is anchored on the reported ainv (the BB stage overwrites the scalar);
    it is no power of two, so w = x0 - alpha g carries one more rounding than the harness knows (fused or
    not): u (|alpha g| + |w|) per entry is added to the bound, and the support check leaves those out."""
    k = 12
    inp = _inputs(n, k, None)
    g = _gradient(inp["H"], n)
    step = _run(be, inp["X"], inp["x0"], inp["Z"], [(inp["H"], None)], strategy)[0]
    assert step["counts"] == _expect_counts(STRATEGIES[strategy][1], 4)
    _check_preconditions(step)
    aref = _ref(("dir", n, k, None), inp["w"])              # x0 - 1.0 * g
    ainv = np.abs(aref.P - inp["x0"]).max()
    assert abs(LD(step["sc"]["ainv"]) - ainv) <= 2 * (aref.tbound + 2 * U).max()
    alpha = 1.0 / step["sc"]["ainv"]
    w = inp["x0"] - alpha * g
    ref = Ref(w)
    extra = U * (np.abs(alpha * g) + np.abs(w)).astype(LD)
    extra = extra + np.broadcast_to(extra.max(axis=0), extra.shape)      # the threshold moves with its entries
    r = _check_projection(step["C"], ref, inp["x0"].astype(LD), step["sc"]["lambda"], extra=extra)
    _check_scalars(step, inp["x0"].astype(LD), g, inp["H"], None)
    _report(strategy, "default alpha0 n%d" % n, r)


# ---------------------------------------------------------------- leg 6: warm starts
def _warm_H(x, tw, n, rng, situations, a):
    """H with w = x - a g(H) per column: "above" -- every entry below the warm threshold (m = 0: the start
    falls back to max - 1); "below" -- every entry far above it (the candidate list is the whole column);
    "near" -- the previous w moved a little (the Newton step from the warm threshold is the start)."""
    T = np.empty_like(x)
    for i, s in enumerate(situations):
        if s == "above":
            T[:, i] = tw[i] - 0.25 - 0.5 * rng.uniform(size=n)
        elif s == "below":
            T[:, i] = tw[i] + 3.0 + 0.9 * rng.uniform(size=n)
        else:
            T[:, i] = x[:, i] + tw[i] + 0.01 * rng.uniform(size=n) * (x[:, i] > 0)
    return (T - x) * float(n) / a


@pytest.mark.parametrize("strategy", ["small32", "list", "iter"])
def test_warm_starts(be, strategy):
    """Three updates on one context with fresh dictionary inputs in between: the second and third
    projections of each kind start from the thresholds the previous update left (set_dictionary_inputs
    does not reset them).  Every column meets each of the three situations once, as second or third call;
    the input x of a call is the dictionary fetched after the previous one, exactly known."""
    n, k, kind = 2049, 6, STRATEGIES[strategy][1]
    inp = _inputs(n, k, ("dense", "sparse", "c2049", "dense", "tail2", "offset"))
    rng = np.random.RandomState(5)
    sits = [("above", "below", "near", "near", "above", "below"), ("below", "near", "above", "below", "near", "above")]
    # the steps depend on what the device returns: one context, three calls, driven step by step
    opts, _, _ = STRATEGIES[strategy]
    for name, value in opts.items():
        be.set_option(name, value)
    worst = 0.0
    try:
        with be.Context(dtype="float64") as ctx:
            ctx.set_data(inp["X"])
            ctx.set_state(np.ascontiguousarray(inp["x0"].T), inp["Z"], np.ones(k))
            x, H, a, ref = inp["x0"], inp["H"], 1.0, _ref(("dir", n, k, tuple(inp["names"])), inp["w"])
            for call in range(3):
                ctx.set_dictionary_inputs(H, np.zeros((k, k)), 0.0)
                st = ctx.dictionary_update(max_iterations=1, alpha0=a)
                step = dict(sc=ctx.spg_scalars(), C=np.ascontiguousarray(ctx.get_state()[0].T),
                            n_feval=st.n_feval, flags=st.flags)
                # PROJ_FEAS runs in the first call only (the dictionary is then known to be feasible)
                assert ctx.proj_counts() == _expect_counts(kind, 3 + 2 * call)
                _check_preconditions(step)
                worst = max(worst, _check_projection(step["C"], ref, x.astype(LD), step["sc"]["lambda"]))
                _check_scalars(step, x.astype(LD), _gradient(H, n), H, None)
                if call < 2:
                    x, a = step["C"], (0.5, 1.0)[call]
                    H = _warm_H(x, np.asarray(ref.t, dtype=np.float64), n, rng, sits[call], a)
                    w = x - a * _gradient(H, n)
                    tw = np.asarray(ref.t, dtype=np.float64)
                    above = (w > tw).sum(axis=0)
                    for i, s in enumerate(sits[call]):       # the situations hold for the exact w
                        assert (above[i] == 0) if s == "above" else (above[i] == n) if s == "below" else \
                            (0 < above[i] < n), (call, i, s, above[i])
                    ref = Ref(w)
    finally:
        for name in opts:
            be.set_option(name, DEFAULTS[name])
    _report(strategy, "warm starts n%d" % n, worst)


# ---------------------------------------------------------------- the LDS boundary, bit for bit
def _block_sum(s, m):
    """block_sum_sm: xor-shuffle tree inside each wave of 64, then the four wave totals in order."""
    s = s.reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return ((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0], int(m.sum())


def _list_solver_threshold(w, n, kp, tb, rpb, in_lds):
    """k_proj_collect + k_proj_solve<false> of one column from the cold lower bound max - 1, with every
    float64 addition in the device's order: thread (rsub, comp) of block b appends its rows in row order to
    segment b RS + rsub; the solver's thread t owns spt consecutive segments.  In LDS the segments are
    concatenated and thread t sums entries t, t + 256, ...; from global memory it sums its own segments
    level by level."""
    rs = 256 // kp
    th = w.max() - 1.0
    segs = []
    for b in range(tb):
        for rsub in range(rs):
            v = w[np.arange(b * rpb + rsub, min(b * rpb + rpb, n), rs)]
            segs.append(v[v > th])
    spt = -(-len(segs) // 256)
    u = np.concatenate(segs)
    prev, conv = -1, False
    for _ in range(200):
        if conv:
            break
        s, m = np.zeros(256), np.zeros(256, dtype=int)
        for t in range(256):
            if in_lds:
                mine = u[t::256]
            else:
                own = segs[t * spt:(t + 1) * spt]
                depth = max([len(x) for x in own] + [0])
                mine = np.array([x[i] for i in range(depth) for x in own if i < len(x)])
            for v in mine[mine > th]:
                s[t] += v
                m[t] += 1
        tot, cnt = _block_sum(s, m)
        if cnt == prev or (prev > 0 and cnt > prev) or cnt == 0:
            conv = True
        if cnt > 0 and cnt != prev:
            th = (tot - 1.0) / cnt
        if cnt > 0:
            prev = cnt
    return th, len(u)


def test_lds_boundary_picks_the_summation_order(be):
    """A list of exactly 2048 candidates is solved in LDS, one of 2049 from global memory.  Both orders
    give a correct threshold, so only the bits can tell which ran: the column with 2048 candidates must
    carry the threshold of the LDS order -- which differs from the global order's in the last bit for this
    column, asserted -- and the column with 2049 the global order's."""
    row = next(r for r in TABLE if r[:3] == (2049, 2, "list"))
    n, k, _, _, kp, tb, rpb, _, cls, _ = row
    inp = _inputs(n, k, cls)
    got = _device(be, row)[0]["C"]
    pred = {}
    for i, want_total in ((0, 2048), (1, 2049)):
        w, x0 = inp["w"][:, i], inp["x0"][:, i]
        for in_lds in (True, False):
            th, total = _list_solver_threshold(w, n, kp, tb, rpb, in_lds)
            assert total == want_total
            pred[i, in_lds] = x0 + (np.maximum(w - th, 0.0) - x0)
    assert not np.array_equal(pred[0, True], pred[0, False])
    assert np.array_equal(got[:, 0], pred[0, True])
    assert np.array_equal(got[:, 1], pred[1, False])


# ---------------------------------------------------------------- host-only
# (no device: these run with the GPU suite because of the module mark, and anywhere with `-m gpu -k host`)
def test_host_table_covers_every_named_edge():
    """Every row's claims are recomputed from the dispatch rules, and every edge the file is there for is
    reached by some row: losing a row fails here, without a GPU."""
    seen = set()
    for n, k, strategy, kind, kp, tb, rpb, path, cls, dtype in TABLE:
        opts = STRATEGIES[strategy][0]
        assert _dispatch(n, k, opts)[:4] == (kind, kp, tb, rpb), _rid((n, k, strategy, 0, 0, 0, 0, 0, 0, dtype))
        assert STRATEGIES[strategy][1] == kind
        fin = _dispatch(n, k, opts)[4]
        seen.add(("n", n) if k == 2 else None)
        seen.add(("k", n, k) if n in (257, 8193) else None)
        seen.add(("kind", kind))
        seen.add(("kp", kp))
        seen.add(("tb", tb))
        seen.add(("fin_in_last", kind if kind != "small64" else "small32", fin))
        seen.add(("dtype", kind, dtype))
        seen.add(("fuse_finalize", opts.get("fuse_finalize", 1)))
        if not STRATEGIES[strategy][2]:
            seen.add(("side", kind, opts.get("proj_res_side", 1)))
        if cls is None and k >= len(CLASSES):
            seen.add(("all classes", kind))
        if path:
            inp = _inputs(n, k, cls)
            for c in (inp["w"] > inp["w"].max(axis=0) - 1.0).sum(axis=0):
                seen.add(("candidates", int(c)) if c in (2048, 2049) else ("path", "lds" if c <= LDS_CAP else "global"))
    want = [("n", n) for n in (1, 7, 255, 256, 257, 2049, 8192, 8193, 16384, 16385, 65537)]
    want += [("k", n, k) for n in (257, 8193) for k in (1, 2, 31, 32, 33, 64)]
    want += [("kind", s) for s in ("small32", "small64", "list", "iterative")]
    want += [("kp", 32), ("kp", 64), ("tb", 1), ("tb", 2), ("tb", 256)]
    want += [("fin_in_last", s, f) for s in ("small32", "list") for f in (False, True)]
    want += [("dtype", s, "float32") for s in ("small32", "small64", "list", "iterative")]
    want += [("fuse_finalize", 0), ("candidates", 2048), ("candidates", 2049), ("path", "lds"), ("path", "global")]
    want += [("side", s, v) for s in ("small32", "list") for v in (0, 1)]
    want += [("all classes", s) for s in ("small32", "small64", "list", "iterative")]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    # n = 16385 with proj_small = 2 falls to the list path; 65537 rows: 256 blocks of 264 rows, seven of them
    # empty and one with 65 rows; 257 rows: 17 per collect thread (2 x 8 unrolled + 1)
    assert _dispatch(16385, 2, {"proj_small": 2})[0] == "list"
    kind, kp, tb, rpb, _ = _dispatch(65537, 2, {})
    assert (tb, rpb, tb - -(-65537 // rpb), 65537 - (-(-65537 // rpb) - 1) * rpb) == (256, 264, 7, 65)
    assert _dispatch(257, 2, {})[3] // (256 // 32) == 17


def test_host_reference_and_inputs_hold_their_claims():
    """On the reference alone: the column classes are what their names say for the exact w of every row,
    the dust share stays below 1 % of a column, a float64 Michelot iteration in NumPy stays within the
    bound, the chain column needs more passes than the iterative path's first batch of 12 (the geometric
    column 1 - 2^-i needs three), and no column comes near the cap of 200."""
    most_passes = 0
    for n, k, cls in sorted({(r[0], r[1], r[8]) for r in TABLE}, key=str):
        if n * k > 8193 * 64:
            continue                                          # (the largest rows repeat classes of smaller ones)
        inp = _inputs(n, k, cls)
        for key, W in (("dir", inp["w"]), ("feas", inp["T"])):
            ref = _ref((key, n, k, cls), W)
            bound = ref.tbound + 2 * U
            dust = ref.dust(bound)
            assert dust.sum(axis=0).max() <= max(0.01 * n, 0), (n, k, key, dust.sum(axis=0))
            for i, name in enumerate(inp["names"]):
                w = W[:, i]
                cand = int((w > w.max() - 1.0).sum())
                if name == "dense" or name == "offset":
                    assert cand == n
                if name in ("c2048", "c2049") and n > 2049:
                    assert cand == int(name[1:])
                if name == "sparse":
                    assert cand == min(n, 3)
                if name == "tail2" and n >= 2:
                    assert set(np.nonzero(ref.supp[:, i])[0]) == {n - 2, n - 1}
                passes = _michelot_passes(w)
                most_passes = max(most_passes, passes)
                if name == "chain" and n >= 14:
                    assert passes > 12, passes
                # a plain float64 Michelot iteration stays within the bound
                t = w.max() - 1.0
                for _ in range(passes + 2):
                    S = w > t
                    t = (w[S].sum() - 1.0) / S.sum()
                assert abs(LD(t) - ref.t[i]) <= ref.tbound[i], (n, k, key, name)
    assert 12 < most_passes < 100
    i = np.arange(2049)
    assert _michelot_passes(1.0 - 2.0 ** -i) == 3
