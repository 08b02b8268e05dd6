"""Times the reconstruction-scores pass (aa_gpnh_residual_scores: k_residual_scores, f64 matrix cores)
against the residual pass of aa_gpnh_residual_cost (k_residual, f64 VALU) and the plain streaming read
of the resident matrix, with HIP events (aa_time_kernel 10 / 11 / 2-5), and -- end to end -- the drivers'
way to their RMSE (download the data, inverse_transform, NumPy) against ``score`` on the DeviceData.

    python tools/validation_bench.py [--rounds 7] [--reps 20] [--e2e 3] [--quick]

Shapes: the headline test's (40 000 x 4096, k = 32), the C2 stand-in (1610 x 25 000, k = 5) and the C3
stand-in (22 280 x 167, k = 10), both context dtypes.  Every round times the kernels one after the other
(alternating), after a warm-up round; the table gives the median and the range over the rounds.  The
floor is the fastest of the four streaming-read variants.  Bounds per launch: bytes = n p x element size,
flop = 2 * 4 ceil(k / 4) n p.  One JSON line per shape and dtype at the end of each block."""
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

SHAPES = (("headline", 40000, 4096, 32), ("C2 stand-in", 1610, 25000, 5), ("C3 stand-in", 22280, 167, 10))


def _stats(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="shapes divided by 8 (rehearsal)")
    a = ap.parse_args()
    _backend.require_gpu()
    for name, n, p, k in SHAPES:
        if a.quick:
            n, p = max(n // 8, 64), max(p // 8, 16)
        rng = np.random.RandomState(0)
        basis = rng.uniform(size=(k, p))
        Z = rng.uniform(size=(n, k)) ** 3
        Z /= Z.sum(axis=1, keepdims=True)
        X = (Z.dot(basis) + 0.01 * rng.standard_normal((n, p))).astype(np.float32)
        for dtype in ("float64", "float32"):
            es = 8 if dtype == "float64" else 4
            nbytes, flop = float(n) * p * es, 2.0 * 4 * ((k + 3) // 4) * n * p
            with _backend.Context(dtype=dtype) as ctx:
                ctx.set_data(X)
                ctx.gpnh_set_factors(k, W=basis.T, Z=Z)
                col, row, sse = ctx.gpnh_residual_scores()
                cost = ctx.gpnh_residual_cost()
                t = {10: [], 11: [], 2: [], 3: [], 4: [], 5: []}
                for rnd in range(a.rounds + 1):
                    for which in (10, 11, 2, 3, 4, 5):
                        ms = ctx.time_kernel(which, a.reps)
                        if rnd:                                   # round 0 warms every kernel up
                            t[which].append(ms)
                dd = cdr.DeviceData(ctx, (n, p), None, (p,))
                model = cdr.ArchetypalAnalysis(k, random_state=0)
                model.archetypes, model.weights = basis, Z
                drv, dev = [], []
                for _ in range(a.e2e):
                    dd._host = None
                    t0 = time.perf_counter()
                    data = dd.to_host()
                    recon = model.inverse_transform(model.weights)
                    rmse_host = np.sqrt(((data - recon) ** 2).mean(axis=0)).mean()
                    drv.append(time.perf_counter() - t0)
                    del data, recon
                    t0 = time.perf_counter()
                    rmse_dev = model.score(dd).rmse
                    dev.append(time.perf_counter() - t0)
                dd._host = None
            floor = min(_stats(t[w])[0] for w in (2, 3, 4, 5))
            s, c = _stats(t[10]), _stats(t[11])
            print("%s  %d x %d  k = %d  %s   (rounds %d, reps %d)" % (name, n, p, k, dtype, a.rounds, a.reps))
            print("  k_residual_scores  median %8.4f ms  [%8.4f, %8.4f]   %6.2f TB/s  %6.2f TFLOP/s  %5.2f x floor"
                  % (s[0], s[1], s[2], nbytes / s[0] / 1e9, flop / s[0] / 1e9, s[0] / floor))
            print("  k_residual         median %8.4f ms  [%8.4f, %8.4f]   %6.2f TB/s                 %5.2f x floor"
                  % (c[0], c[1], c[2], nbytes / c[0] / 1e9, c[0] / floor))
            print("  streaming read     median %8.4f ms   %6.2f TB/s   (variants 2-5: %s)"
                  % (floor, nbytes / floor / 1e9, ", ".join("%.4f" % _stats(t[w])[0] for w in (2, 3, 4, 5))))
            print("  k_residual / k_residual_scores = %.2f;  sse/(2n) = %.12e, residual cost = %.12e" % (c[0] / s[0], sse / (2 * n), cost))
            d, v = _stats(drv), _stats(dev)
            print("  end to end RMSE: download + inverse_transform + NumPy  median %.4f s [%.4f, %.4f] (%.10e);"
                  "  score(DeviceData)  median %.4f s [%.4f, %.4f] (%.10e)"
                  % (d[0], d[1], d[2], rmse_host, v[0], v[1], v[2], rmse_dev))
            print(json.dumps(dict(shape=name, n=n, p=p, k=k, dtype=dtype, rounds=a.rounds, reps=a.reps,
                                  scores_ms=s, residual_ms=c, stream_ms=floor, bytes=nbytes, flop=flop,
                                  speedup=c[0] / s[0], driver_s=d, score_s=v)), flush=True)


if __name__ == "__main__":
    main()
