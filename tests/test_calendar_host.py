"""Calendar-slot climatology and anomalies of resident data, host side (no GPU needed): the work plan of the
slot-major kernels (csrc/group_plan.h) at its chunk edges, ``calendar_smoother`` against trigonometric polynomials
within the bound tests/calendar_restatement.py derives, the refusals that are decided before any device call, and
the new names in header, library, binding and package."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import convex_dim_red as cdr
from convex_dim_red import _backend, preprocessing
from convex_dim_red.preprocessing import CalendarAnomalies, DeviceData

import calendar_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-factorization-case-studies_amd", "csrc")
C = _backend.SLOT_CHUNK_ROWS
U = cr.U


# ------------------------------------------------------------------------------------------------ the plan header
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """tests/group_plan_dump.cpp built with the host compiler; with -fsanitize=address,undefined where that links
    (the program is a stand-alone executable), without where it does not.  Returns run(cases) -> parsed plans."""
    cxx = shutil.which("g++") or (os.path.exists("/opt/rocm/llvm/bin/clang++") and "/opt/rocm/llvm/bin/clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("group_plan") / "group_plan_dump")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
            os.path.join(ROOT, "tests", "group_plan_dump.cpp"), "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                               capture_output=True, text=True)
    if sanitized.returncode != 0:
        print("the host compiler does not link the sanitizers; plain build")
        subprocess.run(base, check=True)

    def run(cases):
        text = "\n".join("%d %d %d %s" % (G, chunk, len(labels), " ".join(str(v) for v in labels))
                         for G, chunk, labels in cases)
        done = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]
        lines = done.stdout.split("\n")
        assert len(lines) == 5 * len(cases) + 1 and lines[-1] == ""
        out = []
        for i in range(len(cases)):
            head, start, rows, first, flat = ([int(v) for v in line.split()] for line in lines[5 * i:5 * i + 5])
            out.append(dict(bad_counting=head[0], bad_block=head[1], counted=head[2], nchunk=head[3], start=start,
                            rows=rows, chunk_first=first, chunks=[tuple(flat[j:j + 3]) for j in range(0, len(flat), 3)]))
        return out
    return run


def _check_plan(plan, G, chunk, labels):
    labels = np.asarray(labels)
    assert plan["bad_counting"] == -1 and plan["counted"] == int((labels >= 0).sum()) == len(plan["rows"])
    assert plan["bad_block"] == (-1 if labels.min(initial=0) >= 0 else int(np.flatnonzero(labels < 0)[0]))
    start, rows = plan["start"], plan["rows"]
    assert len(start) == G + 1 and start[0] == 0 and start[-1] == plan["counted"]
    # every counted row exactly once, rows labelled -1 absent, ascending inside a slot, under its own label
    assert sorted(rows) == np.flatnonzero(labels >= 0).tolist()
    for g in range(G):
        mine = rows[start[g]:start[g + 1]]
        assert mine == np.flatnonzero(labels == g).tolist(), g
    # chunks: at most `chunk` long, in order, tiling every slot's list; a slot without rows has none
    first, chunks = plan["chunk_first"], plan["chunks"]
    assert len(first) == G + 1 and first[0] == 0 and first[-1] == plan["nchunk"] == len(chunks)
    for g in range(G):
        at = start[g]
        for slot, begin, length in chunks[first[g]:first[g + 1]]:
            assert slot == g and begin == at and 1 <= length <= chunk
            assert length == chunk or begin + length == start[g + 1]       # only a slot's last chunk is short
            at += length
        assert at == start[g + 1]
        assert first[g + 1] - first[g] == -(-(start[g + 1] - start[g]) // chunk)


def test_group_plan_at_the_chunk_edges(plan_dump):
    """Built with the address and undefined-behaviour sanitizers where the host compiler links them (the fixture
    falls back to a plain build and says so where it does not)."""
    assert _backend.SLOT_CHUNK_ROWS in (64, 128)
    rng = np.random.RandomState(0)
    cases = []
    # slots of 0, 1, C - 1, C, C + 1 and 2 C + 1 members in one plan, shuffled over the rows, some rows not counted
    sizes = [0, 1, C - 1, C, C + 1, 2 * C + 1]
    for G in (len(sizes), 17, 1464):
        members = (sizes * (G // len(sizes) + 1))[:G] if G <= 17 else [sizes[g % 6] if g < 24 else g % 3 for g in range(G)]
        labels = np.concatenate([np.full(m, g) for g, m in enumerate(members)] + [np.full(37, -1)]).astype(int)
        rng.shuffle(labels)
        cases.append((G, C, labels))
    for n in (1, C - 1, C, C + 1, 3 * C + 1):                       # one slot
        cases.append((1, C, np.zeros(n, dtype=int)))
    cases.append((1, C, np.full(5, -1)))                            # nothing counted: no chunk at all
    cases.append((17, C, np.arange(1000) % 17))
    cases.append((1464, C, np.where(rng.uniform(size=1500) < 0.3, -1, rng.randint(0, 1364, size=1500))))
    cases.append((366, 3, rng.randint(0, 366, size=1000)))         # another chunk length
    cases.append((12, C, np.arange(100000) % 12))                   # the headline's monthly labels: enough work items
    plans = plan_dump(cases)
    for plan, (G, chunk, labels) in zip(plans, cases):
        _check_plan(plan, G, chunk, labels)
    assert plans[8]["nchunk"] == 0 and plans[8]["rows"] == []
    assert plans[-1]["nchunk"] >= 1024
    # the label checks of the entry points name the first offender
    bad = plan_dump([(5, C, [0, 4, 5, -1, -2]), (5, C, [0, -1, 7])])
    assert (bad[0]["bad_counting"], bad[0]["bad_block"]) == (2, 2)
    assert (bad[1]["bad_counting"], bad[1]["bad_block"]) == (2, 1)


# ------------------------------------------------------------------------------------------------ calendar_smoother
def _trig_poly(rng, G, order):
    theta = 2.0 * np.pi * np.arange(G) / G
    m = 1e3 * rng.standard_normal() + np.zeros(G)
    for h in range(1, order + 1):
        m += rng.standard_normal() * np.cos(h * theta) + rng.standard_normal() * np.sin(h * theta)
    return m


@pytest.mark.parametrize("G,H,missing", cr.SMOOTHER_CASES)
def test_smoother_reproduces_trigonometric_polynomials(G, H, missing):
    rng = np.random.RandomState(G + H)
    present = np.ones(G, dtype=bool)
    present[rng.choice(G, size=missing, replace=False)] = False
    S = cdr.calendar_smoother(present, H)
    assert S.shape == (G, G) and S.dtype == np.float64
    assert np.array_equal(S[:, ~present], np.zeros((G, missing)))          # an absent slot is never read
    worst = 0.0
    for order in range(H + 1):
        m = _trig_poly(rng, G, order)
        seen = np.where(present, m, 0.0)
        bound = cr.SMOOTHER_FACTOR * (G + 2) * U * np.abs(S).dot(np.abs(seen))
        err = np.abs(S.dot(seen) - m)                                      # on ALL slots: the missing ones are filled
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (G, H, order)
        with_nan = np.where(present, m, np.nan)                            # what calendar_anomalies does with NaN rows
        assert np.array_equal(S.dot(np.where(np.isnan(with_nan), 0.0, with_nan)), S.dot(seen))
    # idempotent on the present block, in the same measure over the parts of S (tests/calendar_restatement.py)
    Sp, parts = S[np.ix_(present, present)], cr.smoother_parts(present, H)
    bound = cr.SMOOTHER_FACTOR * (G + 2) * U * parts.dot(parts)
    err = np.abs(Sp.dot(Sp) - Sp)
    assert np.all(err <= bound)
    print("G=%d H=%d missing=%d: largest error / bound: reproduction %.4f, idempotence %.4f (allowed 1)"
          % (G, H, missing, worst, float((err / bound).max())))


def test_smoother_refusals_and_no_harmonics():
    present = np.ones(12, dtype=bool)
    for harmonics in (0, -1, 2.0, None, True, "2"):
        with pytest.raises(ValueError, match="harmonics"):
            cdr.calendar_smoother(present, harmonics)
    with pytest.raises(ValueError, match="harmonics"):                       # 2 H + 1 > slots with data
        cdr.calendar_smoother(present, 6)
    few = np.zeros(12, dtype=bool)
    few[:4] = True
    with pytest.raises(ValueError, match="harmonics"):
        cdr.calendar_smoother(few, 2)
    assert cdr.calendar_smoother(few, 1).shape == (12, 12)
    for bad in (np.ones((3, 4), dtype=bool), np.ones(0, dtype=bool), np.ones(12), 5):
        with pytest.raises(ValueError, match="present"):
            cdr.calendar_smoother(bad, 1)


class _NumpyContext(object):
    """A context whose two slot entry points are NumPy: what ``calendar_anomalies`` does with the sums on the host
    -- means, smoothing, scale, the tables it hands to the copy -- can then be read without a device."""
    h = 1
    dtype_code = _backend.AA_F64
    device = 0

    def __init__(self, X=None, **kwargs):
        self.X, self.installed = X, None

    def close(self):
        self.h = None

    def data_slot_sums(self, slots, n_slots, centre=None):
        return cr.slot_sums(self.X, np.asarray(slots), n_slots, centre)

    def set_data_rows_slots(self, owner, row0, n, slots, shift=None, scale=None):
        self.installed = (row0, n, np.asarray(slots), shift, scale)


def test_host_arithmetic_of_calendar_anomalies(monkeypatch):
    """harmonics=None leaves the means untouched: the climatology that is subtracted IS the table of slot means
    ``calendar_stats`` returns, bit for bit; with harmonics it is ``S @ mean`` with the empty slots entering as 0."""
    monkeypatch.setattr(_backend, "Context", _NumpyContext)
    rng = np.random.RandomState(3)
    n, p, G = 90, 5, 20
    X = cr.columns(rng, n, p)
    lab = rng.randint(0, G - 2, size=n)                     # the last two slots are never used
    lab[:10] = np.arange(10)
    base = (10, 80)
    lab[80:] = lab[10:20]                                   # every slot the block uses past the base has base rows
    lab[:10] = lab[20:30]
    dd = DeviceData(_NumpyContext(X), (n, p), None, (p,))
    stats = dd.calendar_stats(lab, n_slots=G, rows=base)
    assert np.all(np.isnan(stats.mean[G - 2:])) and np.array_equal(stats.counts[G - 2:], [0, 0])
    plain = dd.calendar_anomalies(lab, n_slots=G, base_rows=base)
    assert plain.calendar.harmonics is None and plain.calendar.scale is None
    assert np.array_equal(plain.calendar.climatology, stats.mean, equal_nan=True)
    row0, nb, slots, shift, scale = plain._ctx.installed
    assert (row0, nb) == (0, n) and np.array_equal(slots, lab) and scale is None
    assert shift is plain.calendar.climatology
    smooth = dd.calendar_anomalies(lab, n_slots=G, base_rows=base, harmonics=2, standardize=True)
    S = cdr.calendar_smoother(stats.counts > 0, 2)
    assert np.array_equal(smooth.calendar.climatology, S.dot(np.where(np.isnan(stats.mean), 0.0, stats.mean)))
    assert np.all(np.isfinite(smooth.calendar.climatology))                  # the empty slots are filled
    counted = np.full(n, -1)
    counted[base[0]:base[1]] = lab[base[0]:base[1]]
    want = cr.slot_stats(X, counted, G, smooth.calendar.climatology)[1]
    assert np.array_equal(smooth.calendar.scale, want, equal_nan=True)
    assert smooth._ctx.installed[3] is smooth.calendar.climatology and smooth._ctx.installed[4] is smooth.calendar.scale


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device raises: whatever the tests below see was decided on the host."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


class _FakeContext(object):
    """Stands in for an open context: what the new methods refuse they must refuse without touching it."""
    h = 1
    dtype_code = _backend.AA_F64
    device = 0

    def close(self):
        self.h = None

    def data_slot_sums(self, *args, **kwargs):
        raise AssertionError("a device call was made")

    def set_data_rows_slots(self, *args, **kwargs):
        raise AssertionError("a device call was made")


def _block(n=40, p=4):
    return DeviceData(_FakeContext(), (n, p), np.ones(p, dtype=bool), (p,))


def test_refusals_happen_before_any_device_call(no_device):
    n, p = 40, 4
    dd = _block(n, p)
    days = np.arange(n) % 17
    good = CalendarAnomalies(17, (0, n), None, np.zeros((17, p)), np.ones((17, p)), np.full(17, 2), days)
    calls = (dd.calendar_stats, dd.calendar_anomalies, lambda s, **kw: dd.calendar_anomalies(s, model=good, **kw))
    for call in calls:
        for labels in (days[:-1], np.arange(n + 1) % 17, days.reshape(2, 20), 3):             # length / shape
            with pytest.raises(ValueError, match="one slot label per row"):
                call(labels)
        for labels in (days.astype(float), days > 5, ["a"] * n):                                # dtype
            with pytest.raises(ValueError, match="integer slot labels"):
                call(labels)
        bad = days.copy()
        bad[3] = -1
        with pytest.raises(ValueError, match="start at 0"):                                    # range
            call(bad)
        bad[3] = 17
        with pytest.raises(ValueError, match="label 17 with n_slots = 17"):
            call(bad, n_slots=17)
    for call in calls[:2]:
        with pytest.raises(ValueError, match="more than 1464 slots"):
            call(days, n_slots=1465)
        with pytest.raises(ValueError, match="more than 1464 slots"):
            call(np.where(np.arange(n) == 7, 1464, days))
        for n_slots in (0, -3, 17.0, True):
            with pytest.raises(ValueError, match="n_slots"):
                call(days, n_slots=n_slots)
    assert preprocessing.MAX_SLOTS == _backend.MAX_SLOTS == 1464
    for rows in ((5, 5), (-1, 4), (0, n + 1), (2.0, 8), 4, (1, 2, 3)):
        with pytest.raises(ValueError, match="rows"):
            dd.calendar_stats(days, rows=rows)
        with pytest.raises(ValueError, match="base_rows"):
            dd.calendar_anomalies(days, base_rows=rows)
    for centre in (np.zeros(p), np.zeros((17, p + 1)), np.zeros((16, p)), np.zeros((18, p))):  # a table of the wrong shape
        with pytest.raises(ValueError, match="centre"):
            dd.calendar_stats(days, centre=centre)
    for harmonics in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="harmonics"):
            dd.calendar_anomalies(days, harmonics=harmonics)
    with pytest.raises(ValueError, match="harmonics"):                      # 17 slots carry at most 8 harmonics
        dd.calendar_anomalies(days, harmonics=9)
    with pytest.raises(ValueError, match="harmonics"):                      # the base rows fill only 5 slots
        dd.calendar_anomalies(days, base_rows=(0, 5), harmonics=3)
    # model=: nothing of the other block's statistics may be restated beside it; its tables must fit
    for kw in (dict(base_rows=(0, 20)), dict(harmonics=2), dict(n_slots=18)):
        with pytest.raises(ValueError, match="model"):
            dd.calendar_anomalies(days, model=good, **kw)
    with pytest.raises(ValueError, match="model"):
        dd.calendar_anomalies(days, model=(17, None))
    with pytest.raises(ValueError, match="model.climatology"):
        dd.calendar_anomalies(days, model=good._replace(climatology=np.zeros((17, p + 1))))
    with pytest.raises(ValueError, match="model.scale"):
        dd.calendar_anomalies(days, model=good._replace(scale=np.ones((16, p))), standardize=True)
    with pytest.raises(ValueError, match="standardize needs"):
        dd.calendar_anomalies(days, model=good._replace(scale=None), standardize=True)
    # decided from the model's tables alone, still before anything is copied: a used slot without a climatology,
    # a zero or non-finite scale; slot and column are named.  Slot 16 + 1 = 17 is not there; unused rows may be NaN
    clim = np.zeros((17, p))
    clim[5, 2] = np.nan
    with pytest.raises(ValueError, match="slot 5, column 2"):
        dd.calendar_anomalies(days, model=good._replace(climatology=clim))
    for value in (0.0, -0.0, np.inf, np.nan):
        scale = np.ones((17, p))
        scale[7, 1] = value
        with pytest.raises(ValueError, match="scale of slot 7, column 1"):
            dd.calendar_anomalies(days, model=good._replace(scale=scale), standardize=True)
    # what is in order gets as far as the device
    unused = np.ones((18, p))
    unused[17] = np.nan                                                     # no row of the block uses slot 17
    wide = good._replace(n_slots=18, climatology=unused, scale=unused)
    for call in (lambda: dd.calendar_stats(days), lambda: dd.calendar_stats(days, n_slots=366, rows=(3, 30)),
                 lambda: dd.calendar_stats(days, centre=np.zeros((17, p))),
                 lambda: dd.calendar_anomalies(days), lambda: dd.calendar_anomalies(days, harmonics=8, standardize=True),
                 lambda: dd.calendar_anomalies(days, model=good, standardize=True),
                 lambda: dd.calendar_anomalies(days, model=wide, standardize=True)):
        with pytest.raises(AssertionError, match="device call"):
            call()
    dd.close()
    for call in (lambda: dd.calendar_stats(days), lambda: dd.calendar_anomalies(days),
                 lambda: dd.calendar_anomalies(days, model=good)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    with pytest.raises(ValueError):                                         # the labels are still checked first
        dd.calendar_stats(days[:-1])


def test_constructor_and_signatures(no_device):
    spec = inspect.getfullargspec(DeviceData.__init__)
    assert spec.args[-1] == "calendar" and spec.defaults == (None,) * (len(spec.args) - 5)
    assert _block().calendar is None
    record = CalendarAnomalies(1, (0, 3), None, np.zeros((1, 4)), None, np.array([3]), np.zeros(3, dtype=int))
    assert DeviceData(_FakeContext(), (3, 4), None, (4,), calendar=record).calendar is record
    spec = inspect.getfullargspec(DeviceData.calendar_anomalies)
    assert spec.args == ["self", "slots", "n_slots", "base_rows", "harmonics", "standardize", "model"]
    assert spec.defaults == (None, None, None, False, None)
    spec = inspect.getfullargspec(DeviceData.calendar_stats)
    assert spec.args == ["self", "slots", "n_slots", "rows", "centre"] and spec.defaults == (None, None, None)


def test_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "aa_hip.h")) as fh:
        header = fh.read()
    names = ("aa_data_slot_sums", "aa_set_data_rows_slots")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    for macro, mirror in (("AA_MAX_SLOTS", _backend.MAX_SLOTS), ("AA_SLOT_CHUNK_ROWS", _backend.SLOT_CHUNK_ROWS),
                          ("AA_SLOT_TILE_COLS", _backend.SLOT_TILE_COLS)):
        assert int(re.search(r"^#define\s+%s\s+(\d+)" % macro, header, re.M).group(1)) == mirror, macro
    with open(os.path.join(CSRC, "Makefile")) as fh:
        assert "group_plan.h" in fh.read()
    if not os.path.exists(_backend.library_path()):
        pytest.fail("libaa_hip.so has not been built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_backend.library_path())
    for name in names:
        assert hasattr(lib, name), name
    for name in ("calendar_smoother", "CalendarAnomalies"):
        assert name in cdr.__all__ and getattr(cdr, name) is getattr(preprocessing, name)
    assert cdr.CalendarAnomalies._fields == ("n_slots", "base_rows", "harmonics", "climatology", "scale", "counts",
                                             "slots")
    for method in ("calendar_stats", "calendar_anomalies"):
        assert callable(getattr(DeviceData, method))
    for method in ("data_slot_sums", "set_data_rows_slots"):
        assert callable(getattr(_backend.Context, method))
