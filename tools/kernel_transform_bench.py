"""Times the cross RBF product of KernelAA.transform (k_rbf_cross_mfma, f64 matrix cores) against the RBF
fit's K V product (k_rbf_kv, f64 VALU) on the same square shape, with HIP events (aa_time_kernel 9 / 8).

    python tools/kernel_transform_bench.py [--n 20000] [--p 100] [--k 10] [--reps 5]

Both kernels do n^2 (2 p + 2 KP) flop per launch (KP = 32 for k <= 32, 64 above).  Prints one line per
kernel and a JSON summary line."""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, p, k = a.n, a.p, a.k
    kp = 32 if k <= 32 else 64
    rng = np.random.RandomState(0)
    X = rng.standard_normal((n, p))
    gamma = 1.0 / p
    flop = float(n) * n * (2 * p + 2 * kp)
    res = {}
    with _backend.Context(dtype="float64") as ctx:       # the fit's product: K Z on the implicit kernel
        ctx.set_rbf_features(X, gamma)
        C = rng.uniform(size=(k, n))
        ctx.set_state(C / C.sum(axis=1, keepdims=True), np.full((n, k), 1.0 / k), np.ones(k))
        res["k_rbf_kv"] = ctx.time_kernel(8, a.reps)
    with _backend.Context(dtype="float64") as ctx:       # the transform's product: rows X against X_S = X
        ctx.set_data(X)
        ctx.set_rbf_reference(X, rng.uniform(size=(n, k)) / n, gamma)
        res["k_rbf_cross_mfma"] = ctx.time_kernel(9, a.reps)
    out = dict(n=n, m=n, s=n, p=p, k=k, KP=kp, reps=a.reps, flop_per_launch=flop)
    for name, ms in res.items():
        tf = flop / (ms * 1e-3) / 1e12
        print("%-18s %9.3f ms  %7.2f TFLOP/s" % (name, ms, tf))
        out[name + "_ms"] = ms
        out[name + "_tflops"] = tf
    out["speedup"] = res["k_rbf_kv"] / res["k_rbf_cross_mfma"]
    print("cross / kv throughput: %.2fx" % out["speedup"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
