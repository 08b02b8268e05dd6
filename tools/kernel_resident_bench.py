"""Times what keeps a KernelAA workflow on resident data against the only route there was before it -- download the
block with ``to_host()``, then the host-array call -- in the same run:

  * ``DeviceData.take`` of a random permutation of the rows (k_gather_rows),
  * the feature build of the implicit polynomial kernel from a resident block (k_features_from_data),
  * ``KernelAA.kernel_scores`` of a resident block (k_kernel_sample_residuals behind the cross product).

    python tools/kernel_resident_bench.py [--rounds 7] [--reps 50] [--quick] [--out profiles/kernel_resident.txt]

Shape of profiles/implicit_poly.txt: n = 20 000, p = 100, k = 10, degree 3 (the kernel times also at 50 times the
rows, where the matrix no longer fits the Infinity Cache).  Two kinds of numbers, named for what they are.  Kernel
times: HIP events on the context's stream around ``reps`` launches after an untimed one (aa_time_kernel 13 / 14,
and 2-5 for the plain streaming read of the same matrix, the bandwidth reference), as GB/s of the bytes the kernel
has to move (read + written).  Call times: a host clock around the whole call, which ends in
a device synchronise -- allocation, zero fill, launches and the copies included; every round times the resident
route and the download route one after the other, after a warm-up round; median and range over the rounds."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization-case-studies_amd"))

import convex_dim_red as cdr  # noqa: E402
from convex_dim_red import _backend  # noqa: E402


def _stats(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def _block(X, dtype):
    ctx = _backend.Context(dtype=dtype)
    ctx.set_data(np.asarray(X, dtype=dtype))
    return cdr.DeviceData(ctx, X.shape, None, X.shape[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="n divided by 8 (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_resident.txt"))
    a = ap.parse_args()
    _backend.require_gpu()
    n, p, k, degree = (2500 if a.quick else 20000), 100, 10, 3
    gamma = 1.0 / p
    rng = np.random.RandomState(0)
    centers = rng.standard_normal((k, p)) * 2.0
    X = centers[rng.randint(k, size=n)] + 0.4 * rng.standard_normal((n, p))
    X = X / np.sqrt(gamma * (X * X).sum(axis=1).max())
    perm = rng.permutation(n)
    lines, record = [], dict(n=n, p=p, k=k, degree=degree, rounds=a.rounds, reps=a.reps)

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("KernelAA on resident data: n = %d, p = %d, k = %d, degree %d  (rounds %d, reps %d)" % (n, p, k, degree, a.rounds, a.reps))
    # ---- kernel times (HIP events): the shape above, which fits the Infinity Cache (16 MB in float64), and one
    # 50 times as long, which does not
    big = np.random.RandomState(1).standard_normal((50 * n, p)).astype(np.float32)
    for dtype, data in (("float64", X), ("float32", X), ("float64", big), ("float32", big)):
        es = 8 if dtype == "float64" else 4
        n = data.shape[0]
        with _backend.Context(dtype=dtype) as ctx:
            ctx.set_data(np.asarray(data, dtype=dtype))
            Z = np.full((n, k), 1.0 / k)
            ctx.gpnh_set_factors(k, W=np.ones((p, k)), Z=Z)
            t = {w: [] for w in (13, 14, 2, 3, 4, 5)}
            for rnd in range(a.rounds + 1):
                for which in t:
                    ms = ctx.time_kernel(which, a.reps)
                    if rnd:
                        t[which].append(ms)
        floor = min(_stats(t[w])[0] for w in (2, 3, 4, 5))
        read_gbs = float(n) * p * es / floor / 1e6          # the probe reads the padded matrix; counted: the n x p payload
        g, f = _stats(t[13]), _stats(t[14])
        g_bytes, f_bytes = 2.0 * n * p * es + 8.0 * n, float(n) * p * (es + 8)
        say("%s  %d x %d  kernel times (HIP events)" % (dtype, n, p))
        say("  k_gather_rows (random permutation)  median %8.4f ms  [%8.4f, %8.4f]  %8.1f GB/s (read + write + indices)"
            % (g[0], g[1], g[2], g_bytes / g[0] / 1e6))
        say("  k_features_from_data (poly layout)  median %8.4f ms  [%8.4f, %8.4f]  %8.1f GB/s (read + float64 write)"
            % (f[0], f[1], f[2], f_bytes / f[0] / 1e6))
        say("  streaming read of the same matrix   median %8.4f ms                        %8.1f GB/s (payload; variants 2-5: %s)"
            % (floor, read_gbs, ", ".join("%.4f" % _stats(t[w])[0] for w in (2, 3, 4, 5))))
        record["%s %d" % (dtype, n)] = dict(gather_ms=g, features_ms=f, stream_ms=floor,
                                            gather_gbs=g_bytes / g[0] / 1e6, features_gbs=f_bytes / f[0] / 1e6,
                                            stream_gbs=read_gbs)

    del big
    n = X.shape[0]
    # ---- call times (host clock, every call ends in a device synchronise)
    with _block(X, "float64") as block:
        model = cdr.KernelAA(k, init="furthest_sum", random_state=0, max_iterations=3, tolerance=0,
                             require_monotonic_cost_decrease=False, dictionary_solver_kwargs=dict(max_iterations=1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.fit_transform(block, features=True, kernel="poly", gamma=gamma, degree=degree)
        weights = model.weights

        def download():
            block._host = None                               # to_host() caches: every round pays the download
            return block.to_host()

        def take_resident():
            with block.take(perm) as out:
                return out.shape

        def take_download():
            with _block(download()[perm], "float64") as out:
                return out.shape

        def features_resident():
            with _backend.Context(dtype="float64") as ctx, block.borrow() as owner:
                ctx.set_poly_features_resident(owner, gamma, 1.0, degree)

        def features_download():
            host = download()
            with _backend.Context(dtype="float64") as ctx:
                ctx.set_poly_features(host, gamma, 1.0, degree)

        pairs = (("take(random permutation)", take_resident, take_download),
                 ("polynomial feature build", features_resident, features_download),
                 ("kernel_scores", lambda: model.kernel_scores(block, weights=weights).cost,
                  lambda: model.kernel_scores(download(), weights=weights).cost))
        say("float64  call times (host clock around the synchronous call; the download route is to_host() + the host-array call)")
        for name, resident, route in pairs:
            tr, td, values = [], [], None
            for rnd in range(a.rounds + 1):
                s_r, v_r = _clock(resident)
                s_d, v_d = _clock(route)
                if rnd:
                    tr.append(s_r)
                    td.append(s_d)
                values = (v_r, v_d)
            r, d = _stats(tr), _stats(td)
            say("  %-26s resident  median %9.3f ms [%9.3f, %9.3f]   download route  median %9.3f ms [%9.3f, %9.3f]   ratio %.1f"
                % (name, 1e3 * r[0], 1e3 * r[1], 1e3 * r[2], 1e3 * d[0], 1e3 * d[1], 1e3 * d[2], d[0] / r[0]))
            if name == "kernel_scores":
                say("    cost resident %.15e, download route %.15e" % values)
            record[name] = dict(resident_s=r, download_s=d, ratio=d[0] / r[0])
        block._host = None
    say(json.dumps(record))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
