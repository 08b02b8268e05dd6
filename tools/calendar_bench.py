"""Times the calendar-slot statistics and anomalies of a resident block (DeviceData.calendar_stats,
calendar_anomalies) against the host route (to_host, the restatement vectorised in NumPy, upload), end to end in one
process, and their kernels against the streaming read of the same matrix and against the <= 16-group pass.

    python tools/calendar_bench.py [--runs 5] [--reps 20] [--rounds 5] [--quick]

Shapes: 100 000 x 4096 float32 with 366 slots (rows labelled r mod 366) and 89 120 x 167 float64 with 1464 slots
(r mod 1464, the six-hourly C3 stand-in); base rows = the middle half, 4 harmonics, standardised.  End to end: a
host clock around calls that end in a device synchronise, median of ``--runs`` after one warm-up run (the host
route, which has nothing to warm, runs ``--runs`` times).  The host route sorts the base rows by slot once (a stable
argsort) and takes the sums with ``np.add.reduceat``.  Kernels: HIP events around ``--reps`` launches
(aa_time_kernel 21 / 22 / 23 -- rows labelled r mod 366 on both shapes --, what the <= 16-group path offers: the
16-row weighted sums 15, which take coefficients and no labels, and their squared-deviation form 16 with the rows
labelled r mod 12; and the streaming-read variants 2-5), ``--rounds`` alternating rounds after a warm-up round,
median.  Algorithmic bytes per launch: the sums read n p_pad elements and write and read back one float64 partial
row per chunk of AA_SLOT_CHUNK_ROWS rows; the copy reads and writes n p_pad elements.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization-case-studies_amd"))

import convex_dim_red as cdr  # noqa: E402
from convex_dim_red import _backend  # noqa: E402

SHAPES = (("headline width", 100000, 4096, "float32", 366), ("C3 stand-in", 89120, 167, "float64", 1464))
HARMONICS = 4
TIMED_SLOTS = 366           # the labels aa_time_kernel 21 .. 23 use


def host_route(X, slots, G, base):
    """The restatement on a float64 matrix, vectorised: returns the standardised anomalies."""
    lo, hi = base
    order = np.argsort(slots[lo:hi], kind="stable")
    lab = slots[lo:hi][order]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    present = np.zeros(G, dtype=bool)
    present[lab[starts]] = True
    counts = np.bincount(lab, minlength=G)
    Xs = X[lo:hi][order]
    mean = np.zeros((G, X.shape[1]))
    mean[present] = np.add.reduceat(Xs, starts, axis=0) / counts[present, None]
    clim = cdr.calendar_smoother(present, HARMONICS).dot(mean)
    Xs -= clim[lab]
    np.square(Xs, out=Xs)
    scale = np.full((G, X.shape[1]), np.nan)
    scale[present] = np.sqrt(np.add.reduceat(Xs, starts, axis=0) / counts[present, None])
    del Xs
    y = X - clim[slots]
    y /= scale[slots]
    return y


def _median(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="rows divided by 16 (rehearsal)")
    a = ap.parse_args()
    _backend.require_gpu()
    for name, n, p, dtype, G in SHAPES:
        if a.quick:
            n //= 16
        rng = np.random.default_rng(0)
        X = rng.standard_normal((n, p), dtype=np.float32)
        X += (2.0 * np.sin(2.0 * np.pi * np.arange(n) / G) + 1e-4 * np.arange(n))[:, None].astype(np.float32)
        X += 280.0
        base = (n // 4, n - n // 4)
        slots = np.arange(n) % G
        es = 4 if dtype == "float32" else 8
        p_pad = (p + 127) // 128 * 128
        nbytes = float(n) * p_pad * es
        members = n // TIMED_SLOTS + (np.arange(TIMED_SLOTS) < n % TIMED_SLOTS)            # rows per slot, r mod 366
        chunks = int((-(-members // _backend.SLOT_CHUNK_ROWS)).sum())
        partial_bytes = 2.0 * chunks * p_pad * 8
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(X)
            del X
            D = cdr.DeviceData(ctx, (n, p), None, (p,))
            t_stats, t_anom, t_host = [], [], []
            for run in range(a.runs + 1):
                t0 = time.perf_counter()
                D.calendar_stats(slots, n_slots=G, rows=base)
                t1 = time.perf_counter()
                A = D.calendar_anomalies(slots, n_slots=G, base_rows=base, harmonics=HARMONICS, standardize=True)
                t2 = time.perf_counter()
                if run:                                           # run 0 warms up
                    t_stats.append(t1 - t0)
                    t_anom.append(t2 - t1)
                if run < a.runs:
                    A.close()
            dev = A.to_host()
            A.close()
            for run in range(a.runs):
                D._host = None
                out = None
                t0 = time.perf_counter()
                out = host_route(D.to_host(), slots, G, base)
                with _backend.Context(dtype=dtype) as back:
                    back.set_data(out.astype(np.float32) if dtype == "float32" else out)
                t_host.append(time.perf_counter() - t0)
            D._host = None
            stored = out.astype(np.float32).astype(np.float64) if dtype == "float32" else out
            agree = float(np.abs(dev - stored).max() / np.abs(stored).max())
            del out, stored, dev
            # kernels: the streaming read needs factors of any kind behind the context
            k = 4
            ctx.gpnh_set_factors(k, W=np.ones((p, k)), Z=np.full((n, k), 1.0 / k))
            kinds = (21, 22, 23, 15, 16, 2, 3, 4, 5)
            t = dict((w, []) for w in kinds)
            for rnd in range(a.rounds + 1):
                for which in kinds:
                    ms = ctx.time_kernel(which, a.reps)
                    if rnd:
                        t[which].append(ms)
        floor = min(_median(t[w])[0] for w in (2, 3, 4, 5))
        old, old_sq = _median(t[15])[0], _median(t[16])[0]
        st, an, ho = _median(t_stats), _median(t_anom), _median(t_host)
        print("%s  %d x %d  %s  %d slots, base rows [%d, %d), %d harmonics   (runs %d; rounds %d, reps %d)"
              % (name, n, p, dtype, G, base[0], base[1], HARMONICS, a.runs, a.rounds, a.reps))
        print("  calendar_stats()                                  median %9.2f ms  [%9.2f, %9.2f]"
              % (1e3 * st[0], 1e3 * st[1], 1e3 * st[2]))
        print("  calendar_anomalies(harmonics, standardize)        median %9.2f ms  [%9.2f, %9.2f]"
              % (1e3 * an[0], 1e3 * an[1], 1e3 * an[2]))
        print("  host route (to_host, NumPy, upload)               median %9.2f ms  [%9.2f, %9.2f]   host / device = %.1f"
              % (1e3 * ho[0], 1e3 * ho[1], 1e3 * ho[2], ho[0] / an[0]))
        print("  largest |device - host route| / largest entry = %.2e" % agree)
        for which, label, b in ((21, "slot sums, 366 slots (+ finish)", nbytes + partial_bytes),
                                (22, "squared deviations, 366 slots (+ finish)", nbytes + partial_bytes),
                                (23, "slot copy, shift table (read + write)", 2 * nbytes)):
            m = _median(t[which])
            print("  %-44s median %8.4f ms  [%8.4f, %8.4f]   %6.2f TB/s   %5.2f x read floor   %5.2f x the 16-row %s"
                  % (label, m[0], m[1], m[2], b / m[0] / 1e9, m[0] / floor, m[0] / (old_sq if which == 22 else old),
                     "squared deviations" if which == 22 else "sums"))
        print("  (%d chunks: %.1f MB of partials written and read back, counted in the TB/s of the two sums)"
              % (chunks, partial_bytes / 1e6))
        print("  weighted sums, 16 coefficient rows (+ finish)  median %8.4f ms   %6.2f TB/s   %5.2f x read floor"
              % (old, nbytes / old / 1e9, old / floor))
        print("  squared deviations, 16 rows, r mod 12 (+ finish) median %8.4f ms   %6.2f TB/s   %5.2f x read floor"
              % (old_sq, nbytes / old_sq / 1e9, old_sq / floor))
        print("  streaming read                               median %8.4f ms   %6.2f TB/s   (variants 2-5: %s)"
              % (floor, nbytes / floor / 1e9, ", ".join("%.4f" % _median(t[w])[0] for w in (2, 3, 4, 5))))
        print(json.dumps(dict(shape=name, n=n, p=p, dtype=dtype, slots=G, base_rows=base, harmonics=HARMONICS, runs=a.runs,
                              stats_s=st, anomalies_s=an, host_s=ho, agree=agree, sums_ms=_median(t[21]),
                              sqdev_ms=_median(t[22]), copy_ms=_median(t[23]), sums16_ms=_median(t[15]), sqdev16_ms=_median(t[16]), chunks=chunks, stream_ms=floor,
                              bytes=nbytes, partial_bytes=partial_bytes)), flush=True)


if __name__ == "__main__":
    main()
