"""Times the fit-side K V product of the implicit polynomial kernel (k_poly_kv_mfma, f64 matrix cores) and of
the implicit RBF kernel (k_rbf_kv, f64 VALU) on the same shape in the same run, with HIP events
(aa_time_kernel 8 on a context of each kind).

    python tools/implicit_poly_bench.py [--n 20000] [--p 100] [--k 10] [--degree 3] [--reps 5]

Both kernels do n^2 (2 p + 2 KP) flop per launch (KP = 32 for k <= 32, 64 above).  Prints one line per
kernel, the share of the f64 matrix rate the polynomial product reaches (--peak, TFLOP/s) and a JSON
summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization-case-studies_amd"))

from convex_dim_red import _backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak", type=float, default=78.6, help="f64 matrix peak of the device, TFLOP/s")
    a = ap.parse_args()
    n, p, k = a.n, a.p, a.k
    kp = 32 if k <= 32 else 64
    rng = np.random.RandomState(0)
    X = rng.standard_normal((n, p))
    X /= np.sqrt((X * X).sum(axis=1).max() / p)          # gamma |x.y| <= 1
    gamma = 1.0 / p
    flop = float(n) * n * (2 * p + 2 * kp)
    C = rng.uniform(size=(k, n))
    C /= C.sum(axis=1, keepdims=True)
    Z = np.full((n, k), 1.0 / k)
    res = {}
    for name in ("k_poly_kv_mfma", "k_rbf_kv"):
        with _backend.Context(dtype="float64") as ctx:
            if name == "k_rbf_kv":
                ctx.set_rbf_features(X, gamma)
            else:
                ctx.set_poly_features(X, gamma, 1.0, a.degree)
            ctx.set_state(C, Z, np.ones(k))
            res[name] = ctx.time_kernel(8, a.reps)
    out = dict(n=n, p=p, k=k, KP=kp, degree=a.degree, reps=a.reps, flop_per_launch=flop, f64_matrix_peak_tflops=a.peak)
    for name, ms in res.items():
        tf = flop / (ms * 1e-3) / 1e12
        print("%-18s %9.3f ms  %7.2f TFLOP/s" % (name, ms, tf))
        out[name + "_ms"] = ms
        out[name + "_tflops"] = tf
    out["speedup"] = res["k_rbf_kv"] / res["k_poly_kv_mfma"]
    out["share_of_f64_matrix_peak"] = out["k_poly_kv_mfma_tflops"] / a.peak
    print("polynomial (MFMA) / RBF (VALU) throughput: %.2fx; %.0f %% of the f64 matrix rate (%.1f TFLOP/s)"
          % (out["speedup"], 100 * out["share_of_f64_matrix_peak"], a.peak))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
