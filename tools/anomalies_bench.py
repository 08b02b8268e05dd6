"""Times the seasonal anomalies and the per-group standardisation of a resident block (DeviceData.seasonal_anomalies,
grouped_column_stats + standardized_by_group) against the host route (to_host, the notebook's steps in NumPy,
upload), end to end in one process, and their kernels against the streaming read of the same matrix.

    python tools/anomalies_bench.py [--runs 5] [--reps 20] [--rounds 5] [--quick] [--device-only]

Shapes: 100 000 x 4096 float32 (the headline shard's width) and 89 120 x 167 float64 (C3 stand-in), period 12,
base rows = the middle half.  End to end: a host clock around calls that end in a device synchronise, median of
``--runs`` after one warm-up run (the host route, which has nothing to warm, runs ``--runs`` times).  The host
route is vectorised over the columns (the notebook loops ``linregress`` over them and builds an xarray rolling
window: slower), so the comparison favours the host.  Kernels: HIP events
around ``--reps`` launches (aa_time_kernel 15 / 16 / 17 and the streaming-read variants 2-5), ``--rounds``
alternating rounds after a warm-up round, median.  Bounds per launch of the weighted sums: bytes = n p_pad x
element size (+ the 16 n float64 coefficients once per 512 columns), flop = 2 * 16 * n * p_pad on the f64 matrix
cores.  ``--device-only`` runs the device calls alone, twice per shape (the leg to put under a profiler).  One JSON
line per shape."""
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

SHAPES = (("headline width", 100000, 4096, "float32"), ("C3 stand-in", 89120, 167, "float64"))
PERIOD = 12


def host_route(X, base, groups):
    """The notebook's steps on a float64 matrix, vectorised over the columns; returns the standardised anomalies."""
    n = X.shape[0]
    lo, hi = base
    window = np.ones(PERIOD + 1)
    window[0] = window[-1] = 0.5
    window /= PERIOD
    h = PERIOD // 2
    smooth, term = np.zeros((n - 2 * h, X.shape[1])), np.empty((n - 2 * h, X.shape[1]))
    for k in range(2 * h + 1):
        np.multiply(X[k:n - 2 * h + k], window[k], out=term)
        smooth += term
    del term
    detrended = X[h:n - h] - smooth
    del smooth
    rows = np.arange(h, n - h)
    means = np.stack([detrended[(rows % PERIOD == g) & (rows >= lo) & (rows < hi)].mean(axis=0)
                      for g in range(PERIOD)])
    del detrended
    cycle = means - means.mean(axis=0)
    y = X.copy()
    for g in range(PERIOD):
        y[g::PERIOD] -= cycle[g]
    t = np.arange(n, dtype=np.float64)
    tc = t - t.mean()
    slope = tc.dot(y) / tc.dot(tc)                      # sum tc = 0: the mean of y drops out
    icpt = y.mean(axis=0) - slope * t.mean()
    for r0 in range(0, n, 4096):
        y[r0:r0 + 4096] -= icpt + slope * t[r0:r0 + 4096, None]
    for g in range(PERIOD):
        sel = y[lo:hi][groups[lo:hi] == g]
        y[g::PERIOD] = (y[g::PERIOD] - sel.mean(axis=0)) / sel.std(axis=0)
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
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    _backend.require_gpu()
    for name, n, p, dtype in SHAPES:
        if a.quick:
            n //= 16
        rng = np.random.default_rng(0)
        X = rng.standard_normal((n, p), dtype=np.float32)
        X += (2.0 * np.sin(2.0 * np.pi * np.arange(n) / PERIOD) + 1e-4 * np.arange(n))[:, None].astype(np.float32)
        X += 280.0
        base = (n // 4, n - n // 4)
        groups = np.arange(n) % PERIOD
        es = 4 if dtype == "float32" else 8
        p_pad = (p + 127) // 128 * 128
        nbytes, flop = float(n) * p_pad * es, 2.0 * 16 * n * p_pad
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(X)
            del X
            D = cdr.DeviceData(ctx, (n, p), None, (p,))

            def device_anomalies():
                return D.seasonal_anomalies(period=PERIOD, base_rows=base)

            def device_standardise(A):
                return A.standardized_by_group(groups, stats=A.grouped_column_stats(groups, rows=base))

            if a.device_only:
                for _ in range(2):
                    with device_anomalies() as A, device_standardise(A):
                        pass
                print("%s  %d x %d  %s: device calls only, twice" % (name, n, p, dtype), flush=True)
                continue
            t_anom, t_std, t_host = [], [], []
            for run in range(a.runs + 1):
                t0 = time.perf_counter()
                A = device_anomalies()
                t1 = time.perf_counter()
                S = device_standardise(A)
                t2 = time.perf_counter()
                if run:                                           # run 0 warms up
                    t_anom.append(t1 - t0)
                    t_std.append(t2 - t1)
                if run < a.runs:
                    S.close()
                A.close()
            dev = S.to_host()
            S.close()
            for run in range(a.runs):
                D._host = None
                out = None
                t0 = time.perf_counter()
                out = host_route(D.to_host(), base, groups)
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
            kinds = (15, 16, 17, 2, 3, 4, 5)
            t = dict((w, []) for w in kinds)
            for rnd in range(a.rounds + 1):
                for which in kinds:
                    ms = ctx.time_kernel(which, a.reps)
                    if rnd:
                        t[which].append(ms)
        floor = min(_median(t[w])[0] for w in (2, 3, 4, 5))
        an, st, ho = _median(t_anom), _median(t_std), _median(t_host)
        print("%s  %d x %d  %s  period %d, base rows [%d, %d)   (runs %d; rounds %d, reps %d)"
              % (name, n, p, dtype, PERIOD, base[0], base[1], a.runs, a.rounds, a.reps))
        print("  seasonal_anomalies()                              median %9.2f ms  [%9.2f, %9.2f]"
              % (1e3 * an[0], 1e3 * an[1], 1e3 * an[2]))
        print("  grouped_column_stats() + standardized_by_group()  median %9.2f ms  [%9.2f, %9.2f]"
              % (1e3 * st[0], 1e3 * st[1], 1e3 * st[2]))
        print("  host route (to_host, NumPy, upload)               median %9.2f ms  [%9.2f, %9.2f]   host / device = %.1f"
              % (1e3 * ho[0], 1e3 * ho[1], 1e3 * ho[2], ho[0] / (an[0] + st[0])))
        print("  largest |device - host route| / largest entry = %.2e" % agree)
        for which, label, b in ((15, "weighted sums, 16 rows (+ finish)", nbytes),
                                (16, "squared deviations, 16 rows (+ finish)", nbytes),
                                (17, "model copy, anomalies form (read + write)", 2 * nbytes)):
            m = _median(t[which])
            print("  %-44s median %8.4f ms  [%8.4f, %8.4f]   %6.2f TB/s  %s  %5.2f x read floor"
                  % (label, m[0], m[1], m[2], b / m[0] / 1e9,
                     "%6.2f TFLOP/s" % (flop / m[0] / 1e9) if which != 17 else " " * 14, m[0] / floor))
        print("  streaming read                               median %8.4f ms   %6.2f TB/s   (variants 2-5: %s)"
              % (floor, nbytes / floor / 1e9, ", ".join("%.4f" % _median(t[w])[0] for w in (2, 3, 4, 5))))
        print(json.dumps(dict(shape=name, n=n, p=p, dtype=dtype, period=PERIOD, base_rows=base, runs=a.runs,
                              anomalies_s=an, standardise_s=st, host_s=ho, agree=agree, sums_ms=_median(t[15]),
                              sqdev_ms=_median(t[16]), model_ms=_median(t[17]), stream_ms=floor, bytes=nbytes,
                              flop=flop)), flush=True)


if __name__ == "__main__":
    main()
