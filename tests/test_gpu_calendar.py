"""Calendar-slot climatology and anomalies of resident data on the MI355X (aa_data_slot_sums,
aa_set_data_rows_slots, DeviceData.calendar_stats / calendar_anomalies): the three slot-major kernels of
csrc/kernels_slots.hip at the edges of their work items -- C = AA_SLOT_CHUNK_ROWS rows of one slot, W =
AA_SLOT_TILE_COLS columns -- in both element types.

Every bound is DERIVED in tests/calendar_restatement.py and taken on the STORED values (what a float32 block holds):
the sums against a NumPy loop over the slots within ``2 (m_g + 2) u sum|x|`` / ``2 (m_g + 4) u sum (x - c)^2``, the
statistics within DESIGN 5.3's ``b_mean`` / ``b_var`` with the slot's rows and count, the smoothed climatology within
``|S| @ b_mean + (G + 2) u (|S| @ |mean|)``.  Every copy is compared exactly: the kernel makes the float64 roundings
of the NumPy expression and one rounding to the stored type."""
import ctypes
import warnings

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend

import calendar_restatement as cr

pytestmark = pytest.mark.gpu

U = cr.U
C, W = _backend.SLOT_CHUNK_ROWS, _backend.SLOT_TILE_COLS
COLS = sorted({1, 127, 128, 129, 167, 257, W - 1, W, W + 1})


def _labels(name):
    """(G, counting labels in [-1, G), block labels in [0, G)) of a label pattern."""
    rng = np.random.RandomState(sum(ord(ch) for ch in name))
    if name.startswith("one-"):
        lab = np.zeros(int(name[4:]), dtype=int)
        return 1, lab, lab
    if name == "mod17":
        lab = np.arange(1000) % 17
        return 17, lab, lab
    if name == "random366":                 # not in row order, 0 - 8 rows per slot
        lab = rng.randint(0, 366, size=1000)
        return 366, lab, lab
    assert name == "sparse1464"             # 30 % of the rows not counted, the last 100 slots unused
    lab = rng.randint(0, 1364, size=1500)
    return 1464, np.where(rng.uniform(size=1500) < 0.3, -1, lab), lab


PATTERNS = ["one-%d" % n for n in (1, C - 1, C, C + 1, 3 * C + 1)] + ["mod17", "random366", "sparse1464"]


def _stored(A, dtype):
    return A.astype(np.float32).astype(np.float64) if dtype == "float32" else A


def _device_data(ctx, X):
    ctx.set_data(X)
    return cdr.DeviceData(ctx, X.shape, None, X.shape[1:])


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err > 0, err / bound, 0.0).max())


def _tables(rng, G, p, used):
    """(shift, scale) with NaN in the rows of the slots that are not used: those rows must not be read."""
    shift = cr.columns(rng, G, p)
    scale = rng.uniform(0.5, 2.0, size=(G, p)) * rng.choice([-1.0, 1.0], size=(G, p))
    shift[~used] = np.nan
    scale[~used] = np.nan
    return shift, scale


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_slot_sums_against_the_restatement(dtype, pattern):
    G, lab, _ = _labels(pattern)
    n = lab.shape[0]
    rng = np.random.RandomState(1100 + n)
    worst = worst_sq = 0.0
    with _backend.Context(dtype=dtype) as ctx:
        for p in COLS:
            msg = "dtype=%s %s p=%d" % (dtype, pattern, p)
            ctx.set_data(cr.columns(rng, n, p))
            Xd = ctx.get_data()
            sums, counts = ctx.data_slot_sums(lab, G)
            want, want_counts = cr.slot_sums(Xd, lab, G)
            assert sums.shape == (G, p) and sums.dtype == np.float64 and np.array_equal(counts, want_counts), msg
            err, bound = np.abs(sums - want), cr.sum_bound(Xd, lab, G)
            worst = max(worst, _ratio(err, bound))
            assert np.all(err <= bound), msg
            empty = counts == 0
            assert np.array_equal(sums[empty], np.zeros((int(empty.sum()), p))), msg     # exactly 0, count 0
            again, counts2 = ctx.data_slot_sums(lab, G)
            assert np.array_equal(again, sums) and np.array_equal(counts2, counts), msg  # the same bits on every call
            # squared deviations about a table; the rows of empty slots hold NaN and are not read
            centre = cr.columns(rng, G, p)
            centre[empty] = np.nan
            sq, counts3 = ctx.data_slot_sums(lab, G, centre=centre)
            want, _ = cr.slot_sums(Xd, lab, G, centre)
            err, bound = np.abs(sq - want), cr.sqdev_bound(Xd, lab, G, centre)
            worst_sq = max(worst_sq, _ratio(err, bound))
            assert sq.shape == (G, p) and np.all(err <= bound) and np.array_equal(counts3, counts), msg
            assert np.array_equal(sq[empty], np.zeros((int(empty.sum()), p))), msg
            assert np.array_equal(ctx.data_slot_sums(lab, G, centre=centre)[0], sq), msg
    print("largest error / bound over the columns of %s, %s: sums %.3f, squared deviations %.3f (allowed 1)"
          % (pattern, dtype, worst, worst_sq))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_slot_sums_without_a_counted_row(dtype):
    """Every label -1: no chunk, so only the finish kernel runs; every sum is exactly 0 with count 0, and no row
    of the centre table is read."""
    rng = np.random.RandomState(1150)
    with _backend.Context(dtype=dtype) as ctx:
        for n, p, G in ((5, 1, 1), (70, 129, 3), (70, W + 1, 366)):
            ctx.set_data(cr.columns(rng, n, p))
            lab = np.full(n, -1)
            for centre in (None, np.full((G, p), np.nan)):
                sums, counts = ctx.data_slot_sums(lab, G, centre=centre)
                assert np.array_equal(sums, np.zeros((G, p))) and np.array_equal(counts, np.zeros(G, dtype=int))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_slot_copy_is_exact(dtype, pattern):
    """Shift only, scale only and both; whole blocks and sub-blocks with row0 > 0; NaN in the table rows of the
    slots that the block does not use."""
    G, _, lab = _labels(pattern)
    n = lab.shape[0]
    rng = np.random.RandomState(1200 + n)
    with _backend.Context(dtype=dtype) as ctx, _backend.Context(dtype=dtype) as block:
        for p in COLS:
            ctx.set_data(cr.columns(rng, n, p))
            Xd = ctx.get_data()
            for row0, nb in ((0, n), (n // 3, n - n // 2), (n - 1, 1)):
                if nb < 1 or row0 + nb > n:
                    continue
                mine = lab[row0:row0 + nb]
                shift, scale = _tables(rng, G, p, np.bincount(mine, minlength=G) > 0)
                for use_shift, use_scale in ((True, False), (False, True), (True, True)):
                    want = Xd[row0:row0 + nb]
                    if use_shift:
                        want = want - shift[mine]
                    if use_scale:
                        want = want / scale[mine]
                    block.set_data_rows_slots(ctx, row0, nb, mine, shift=shift if use_shift else None,
                                              scale=scale if use_scale else None)
                    assert (block.n, block.p) == (nb, p)
                    got = block.get_data()
                    assert np.array_equal(got, _stored(want, dtype)), (dtype, pattern, p, row0, nb, use_shift, use_scale)
            assert np.array_equal(ctx.get_data(), Xd)                        # the source is left as it was


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_padding_stays_zero_seen_through_a_fit(dtype):
    """A non-zero padding column or row of the new block would enter the Gram products of the pass kernels: a fit
    on the resident block and one on a fresh upload of its values agree bit for bit."""
    rng = np.random.RandomState(1300)
    n, p, k = 200, 37, 3
    lab = rng.randint(0, 40, size=n)
    with _backend.Context(dtype=dtype) as ctx:
        D = _device_data(ctx, cr.columns(rng, n, p))
        Y = D.calendar_anomalies(lab, n_slots=40, harmonics=3, standardize=True)
    host = Y.to_host()
    assert host.shape == (n, p) and np.all(np.isfinite(host))
    kw = dict(init="furthest_sum", tolerance=1e-6, max_iterations=5, dtype=dtype,
              dictionary_solver_kwargs=dict(max_iterations=1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
        Wa = a.fit_transform(Y)
        b = cdr.ArchetypalAnalysis(k, random_state=0, **kw)
        Wb = b.fit_transform(host)
    assert np.array_equal(Wa, Wb) and np.array_equal(a.dictionary, b.dictionary)
    assert a.cost == b.cost and a.n_iter == b.n_iter and list(a.cost_deltas) == list(b.cost_deltas)
    Y.close()


STAT_CASES = [("mod17", 3), ("random366", 4), ("sparse1464", 3)]


@pytest.fixture(scope="module")
def stat_inputs():
    """The columns of every statistics case with the restatement's tables and bounds on the STORED values, per
    dtype: computed once, read by the tests.  The base period is the middle 80 % of the rows; a row outside it
    whose slot has no base row takes the label of a base row, so that every slot the block uses has statistics."""
    out = {}
    for pattern, H in STAT_CASES:
        G, _, lab = _labels(pattern)
        n = lab.shape[0]
        X = cr.columns(np.random.RandomState(1400 + G), n, 167)
        base = (n // 10, n - n // 10)
        lab = lab.copy()
        outside = (np.arange(n) < base[0]) | (np.arange(n) >= base[1])
        orphan = outside & ~(np.bincount(lab[base[0]:base[1]], minlength=G) > 0)[lab]
        lab[orphan] = lab[base[0] + np.flatnonzero(orphan) % (base[1] - base[0])]
        counted = np.full(n, -1)
        counted[base[0]:base[1]] = lab[base[0]:base[1]]
        for dtype in ("float64", "float32"):
            Xd = _stored(X, dtype)
            out[pattern, dtype] = (X, Xd, lab, base, counted, cr.slot_stats(Xd, counted, G), cr.stat_bounds(Xd, counted, G))
    return out


@pytest.mark.parametrize("pattern,H", STAT_CASES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_calendar_stats_against_the_restatement(stat_inputs, dtype, pattern, H):
    X, Xd, lab, base, counted, (mean, std, counts), (b_mean, b_var, var) = stat_inputs[pattern, dtype]
    G, p = mean.shape
    with _backend.Context(dtype=dtype) as ctx:
        D = _device_data(ctx, X)
        stats = D.calendar_stats(lab, n_slots=G, rows=base)
        assert isinstance(stats, cdr.GroupedColumnStats) and stats.mean.shape == stats.std.shape == (G, p)
        assert np.array_equal(stats.counts, counts)
        empty, single = counts == 0, counts == 1
        assert empty.any() or pattern == "mod17"
        assert np.all(np.isnan(stats.mean[empty])) and np.all(np.isnan(stats.std[empty]))
        e_mean = np.abs(stats.mean[~empty] - mean[~empty])
        assert np.all(e_mean <= 2 * b_mean[~empty])
        assert np.array_equal(stats.std[single], np.zeros((int(single.sum()), p)))
        many = counts > 1
        # std^2 is var up to the roundings of the division, the root and the square: 3 u var
        e_var = np.abs(stats.std[many] ** 2 - var[many])
        assert np.all(e_var <= 2 * b_var[many] + 3 * U * var[many])
        print("%s %s: largest error / bound: mean %.3f, var %.3f (allowed 2)"
              % (pattern, dtype, _ratio(e_mean, b_mean[~empty]), _ratio(e_var, b_var[many] + 3 * U * var[many])))
        # without rows every row counts, and n_slots defaults to the largest label + 1
        whole = D.calendar_stats(lab)
        assert whole.mean.shape == (lab.max() + 1, p) and np.array_equal(whole.counts, np.bincount(lab))
        # about a given centre: the mean squared deviation from it, within the bound of the sums and the three
        # roundings (division, root, square) each side makes
        centre = np.where(np.isnan(mean), np.nan, mean + 1.0)
        about = D.calendar_stats(lab, n_slots=G, rows=base, centre=centre)
        assert np.array_equal(about.mean, stats.mean, equal_nan=True)
        want = cr.slot_stats(Xd, counted, G, centre)[1]
        bound = (cr.sqdev_bound(Xd, counted, G, centre)[~empty] / counts[~empty, None] + 6 * U * want[~empty] ** 2)
        assert np.all(np.abs(about.std[~empty] ** 2 - want[~empty] ** 2) <= bound)
        assert np.all(np.isnan(about.std[empty]))
        bad = centre.copy()
        bad[np.flatnonzero(~empty)[0], 3] = np.inf
        with pytest.raises(ValueError, match=r"centre\[%d\]\[3\]" % np.flatnonzero(~empty)[0]):
            D.calendar_stats(lab, n_slots=G, rows=base, centre=bad)


@pytest.mark.parametrize("pattern,H", STAT_CASES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_calendar_anomalies_end_to_end(stat_inputs, dtype, pattern, H):
    X, Xd, lab, base, counted, (mean, std, counts), (b_mean, b_var, var) = stat_inputs[pattern, dtype]
    G, p = mean.shape
    n = lab.shape[0]
    in_base = counted >= 0
    with _backend.Context(dtype=dtype) as ctx, _backend.Context(dtype=dtype) as second:
        D = _device_data(ctx, X)
        D.scaling = "inherited"
        # a used slot without a base row and no harmonics to fill it: refused before anything is copied
        if np.any(counts == 0):
            orphan = np.where(np.arange(n) == 0, np.flatnonzero(counts == 0)[0], lab)
            with pytest.raises(ValueError, match="climatology of slot %d, column 0" % orphan[0]):
                D.calendar_anomalies(orphan, n_slots=G, base_rows=base)
        # plain slot means over all rows: the block is the NumPy expression on the record's own tables
        with D.calendar_anomalies(lab, n_slots=G) as A:
            rec = A.calendar
            assert isinstance(rec, cdr.CalendarAnomalies) and (rec.n_slots, rec.base_rows, rec.harmonics) == (G, (0, n), None)
            assert rec.scale is None and np.array_equal(rec.slots, lab) and np.array_equal(rec.counts, np.bincount(lab, minlength=G))
            all_mean = cr.slot_stats(Xd, lab, G)[0]
            used = rec.counts > 0
            assert np.all(np.abs(rec.climatology[used] - all_mean[used]) <= 2 * cr.stat_bounds(Xd, lab, G)[0][used])
            assert np.array_equal(A.to_host(), _stored(cr.anomalies(Xd, lab, rec.climatology), dtype))
            # harmonics=None leaves the means untouched: the table subtracted is calendar_stats' own, bit for bit
            assert np.array_equal(rec.climatology, D.calendar_stats(lab, n_slots=G).mean, equal_nan=True)
            assert A.shape == D.shape and A.dtype == D.dtype and A.scaling == "inherited"
            assert A.anomaly is None and A.group_scaling is None and D.calendar is None
        # a slot of one row is its own mean: scale 0, named before anything is copied
        if np.any(np.bincount(lab, minlength=G) == 1):
            with pytest.raises(ValueError, match="scale of slot %d, column 0" % np.flatnonzero(np.bincount(lab, minlength=G) == 1)[0]):
                D.calendar_anomalies(lab, n_slots=G, standardize=True)
        # smoothed climatology over a base period, standardised
        with D.calendar_anomalies(lab, n_slots=G, base_rows=base, harmonics=H, standardize=True) as A:
            rec = A.calendar
            assert (rec.n_slots, rec.base_rows, rec.harmonics) == (G, base, H) and np.array_equal(rec.counts, counts)
            S = cdr.calendar_smoother(counts > 0, H)
            want = cr.climatology(mean, counts, H)
            err, bound = np.abs(rec.climatology - want), cr.smooth_bound(S, mean, b_mean)
            assert rec.climatology.shape == (G, p) and np.all(err <= bound)
            used = (np.bincount(lab, minlength=G) > 0) & (counts > 0)
            Y = A.to_host()
            assert np.array_equal(Y, _stored(cr.anomalies(Xd, lab, rec.climatology, rec.scale), dtype))
            worst = 0.0
            for g in np.flatnonzero(used):
                ms = (Y[in_base & (lab == g)] ** 2).mean(axis=0)
                worst = max(worst, _ratio(np.abs(ms - 1.0), cr.rms_bound(counts[g], dtype)))
                assert np.all(np.abs(ms - 1.0) <= cr.rms_bound(counts[g], dtype)), g
            print("%s %s H=%d: largest error / bound: climatology %.3f, mean square of a slot %.3f (allowed 1)"
                  % (pattern, dtype, H, _ratio(err, bound), worst))
            # the record belongs to the row index: blocks cut from this one carry none
            with A.rows(0, 7) as head, A.take([n - 1, 0]) as picked:
                assert head.calendar is None and picked.calendar is None
                assert np.array_equal(picked.to_host(), Y[[n - 1, 0]])
            # another block takes this one's record: no statistics, the same expression on the same tables
            n2 = 300
            lab2 = np.random.RandomState(7).choice(np.flatnonzero(used), size=n2)
            E = _device_data(second, cr.columns(np.random.RandomState(8), n2, p))
            for standardize in (False, True):
                with E.calendar_anomalies(lab2, model=rec, standardize=standardize) as B:
                    want = cr.anomalies(E.to_host(), lab2, rec.climatology, rec.scale if standardize else None)
                    assert np.array_equal(B.to_host(), _stored(want, dtype))
                    assert B.calendar.climatology is not None and np.array_equal(B.calendar.slots, lab2)
                    assert (B.calendar.n_slots, B.calendar.base_rows, B.calendar.harmonics) == (G, base, H)
                    assert (B.calendar.scale is None) == (not standardize)
            # ... and the anomalies go on into the PCA without a download
            model = A.pca(3)
            assert model.components_.shape == (3, p) and np.all(np.isfinite(model.components_))
        assert np.array_equal(ctx.get_data(), Xd)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_agreement_with_the_sixteen_group_path(dtype):
    """G = 12: calendar_stats (slot-major kernels) and grouped_column_stats (the MFMA pass, untouched) each obey
    b_mean / b_var, so they differ by at most the sum of the two bounds."""
    rng = np.random.RandomState(1500)
    n, G = 1000, 12
    months = np.arange(n) % G
    with _backend.Context(dtype=dtype) as ctx:
        for p in (129, 167):
            D = _device_data(ctx, cr.columns(rng, n, p))
            Xd = D.to_host()
            for rows in (None, (240, 720)):
                lo, hi = (0, n) if rows is None else rows
                counted = np.full(n, -1)
                counted[lo:hi] = months[lo:hi]
                new, old = D.calendar_stats(months, rows=rows), D.grouped_column_stats(months, rows=rows)
                b_mean, b_var, var = cr.stat_bounds(Xd, counted, G)
                assert np.array_equal(new.counts, old.counts)
                e_mean, e_var = np.abs(new.mean - old.mean), np.abs(new.std ** 2 - old.std ** 2)
                assert np.all(e_mean <= 2 * b_mean)
                assert np.all(e_var <= 2 * (b_var + 3 * U * var))
                print("p=%d rows=%r %s: largest difference / bound: mean %.3f, var %.3f (allowed 1)"
                      % (p, rows, dtype, _ratio(e_mean, 2 * b_mean), _ratio(e_var, 2 * (b_var + 3 * U * var))))


def test_entry_point_refusals():
    rng = np.random.RandomState(0)
    A = rng.standard_normal((20, 6))
    B = rng.standard_normal((7, 4))
    lab = np.arange(20) % 3
    with _backend.Context(dtype="float64") as owner, _backend.Context(dtype="float64") as target:
        with pytest.raises(RuntimeError, match="error -3:"):                 # AA_ERR_STATE: no data yet
            owner.data_slot_sums(np.zeros(0, dtype=int), 1)
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_slots(owner, 0, 1, [0], shift=np.zeros((1, 0)))
        owner.set_data(A)
        target.set_data(B)
        # the sums: G out of range, a label outside [-1, G), a non-finite centre entry of a used slot
        for G in (0, -1, 1465):
            with pytest.raises(RuntimeError, match="error -1:.*slots"):
                owner.data_slot_sums(np.zeros(20, dtype=int), G)
        for bad in (-2, 3, 1464):
            with pytest.raises(RuntimeError, match=r"error -1:.*slot\[5\] = %d" % bad):
                owner.data_slot_sums(np.where(np.arange(20) == 5, bad, lab), 3)
        for value in (np.nan, np.inf, -np.inf):
            centre = np.zeros((4, 6))
            centre[3] = np.nan                                               # slot 3 has no row: not read
            assert owner.data_slot_sums(lab, 4, centre=centre)[0].shape == (4, 6)
            centre[1, 2] = value
            with pytest.raises(RuntimeError, match=r"error -1:.*centre\[1\]\[2\]"):
                owner.data_slot_sums(lab, 4, centre=centre)
        with pytest.raises(ValueError):                                      # the binding checks the shapes
            owner.data_slot_sums(lab[:-1], 3)
        with pytest.raises(ValueError):
            owner.data_slot_sums(lab, 3, centre=np.zeros((3, 5)))
        assert np.array_equal(owner.get_data(), A)
        # the install: every refusal leaves the target what it was
        ones = np.ones((3, 6))

        def table(value, at=(1, 3), rows=3):
            out = np.ones((rows, 6))
            out[at] = value
            return out
        lab10 = lab[:10]
        cases = [dict(slots=np.zeros(10, dtype=int), scale=np.ones((1465, 6))),           # G > AA_MAX_SLOTS
                 dict(slots=np.zeros(10, dtype=int), shift=np.ones((0, 6))),              # G < 1
                 dict(slots=np.where(np.arange(10) == 4, 3, lab10), scale=ones),          # a label outside [0, G)
                 dict(slots=np.where(np.arange(10) == 4, -1, lab10), shift=ones),
                 dict(slots=lab10, scale=table(0.0)), dict(slots=lab10, scale=table(-0.0)),
                 dict(slots=lab10, scale=table(np.inf)), dict(slots=lab10, scale=table(np.nan)),
                 dict(slots=lab10, shift=table(np.inf)), dict(slots=lab10, shift=table(np.nan), scale=ones)]
        for kw in cases:
            with pytest.raises(RuntimeError, match="error -1:"):
                target.set_data_rows_slots(owner, 0, 10, **kw)
            assert (target.n, target.p) == (7, 4) and np.array_equal(target.get_data(), B)
        with pytest.raises(RuntimeError, match=r"error -1:.*scale\[1\]\[3\]"):            # the first offender is named
            target.set_data_rows_slots(owner, 0, 10, lab10, scale=table(0.0))
        with pytest.raises(RuntimeError, match=r"error -1:.*slot\[4\] = 3"):
            target.set_data_rows_slots(owner, 0, 10, np.where(np.arange(10) == 4, 3, lab10), scale=ones)
        # both tables NULL: the binding refuses it itself, so ask the library
        slots = np.ascontiguousarray(lab10, dtype=np.intc)
        rc = target.lib.aa_set_data_rows_slots(target.h, owner.h, 0, 10, 3,
                                               slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None)
        assert rc == -1 and np.array_equal(target.get_data(), B)
        with pytest.raises(ValueError):
            target.set_data_rows_slots(owner, 0, 10, lab10)
        for row0, nb in ((-1, 5), (0, 0), (0, 21), (20, 1), (5, 16)):
            with pytest.raises(RuntimeError, match="error -1:"):             # bad row block
                target.set_data_rows_slots(owner, row0, nb, np.zeros(max(nb, 0), dtype=int), shift=np.ones((1, 6)))
        with pytest.raises(RuntimeError, match="error -1:"):                 # ctx == owner
            owner.set_data_rows_slots(owner, 0, 5, lab[:5], shift=ones)
        with _backend.Context(dtype="float32") as other:
            with pytest.raises(RuntimeError, match="error -1:"):             # dtype mismatch
                other.set_data_rows_slots(owner, 0, 5, lab[:5], shift=ones)
        with pytest.raises(ValueError):                                      # the binding checks the shapes
            target.set_data_rows_slots(owner, 0, 10, lab10, scale=np.ones((3, 5)))
        assert np.array_equal(target.get_data(), B)
        # the same values in rows that no row of the block uses are not read
        unused = table(np.nan, at=(3, slice(None)), rows=4)
        unused[3, 0] = 0.0
        target.set_data_rows_slots(owner, 2, 10, lab[2:12], shift=unused - 1.0, scale=-unused)
        assert np.array_equal(target.get_data(), -A[2:12])                   # a negative divisor is a divisor
    K = rng.standard_normal((12, 12))
    with _backend.Context(dtype="float64") as ctx, _backend.Context(dtype="float64") as target:
        ctx.set_data(K.dot(K.T), form=_backend.FORM_KERNEL)
        with pytest.raises(RuntimeError, match="error -3:"):                 # kernel form
            ctx.data_slot_sums(np.zeros(12, dtype=int), 1)
        with pytest.raises(RuntimeError, match="error -3:"):
            target.set_data_rows_slots(ctx, 0, 5, np.zeros(5, dtype=int), shift=np.zeros((1, 12)))
