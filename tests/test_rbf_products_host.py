"""The RBF product tests' own machinery, checked on the host (tests/rbf_restatement.py): the NumPy emulation of
k_rbf_kv / k_rbf_cross_mfma / k_distance_rbf meets the derived bound against the long-double reference on every
case of tests/test_gpu_rbf_products.py, every planted fault is noticed on the inputs chosen for it, and the split
arithmetic of the two launchers gives the splits the cases are named for."""
import numpy as np
import pytest

import rbf_restatement as rr


def _kv_rows(pb):
    """All rows up to n = 900; above, the rows the GPU test selects."""
    if pb["n"] <= rr.KV_RANDOM_FACTORS_UP_TO:
        return np.arange(pb["n"])
    return np.unique(pb["rows"])


def _judge_kv(pb, rows, entries, out):
    """What the GPU test asserts, on the emulation's K[rows] and (K Z0)[rows]: the largest ratios to the entry
    and the product bound, and the exact facts as a list of the ones broken."""
    X, gamma, n = pb["X"], pb["gamma"], pb["n"]
    K, s = rr.reference(X, X, gamma, rows)
    E = rr.entry_E(X, X, gamma, s, rows)
    r_entry = rr.ratio(entries, K, rr.entry_bound(K, E))
    r_prod = rr.ratio(out, K.dot(pb["Z0"].astype(rr.LD)), rr.entry_bound(K, E, n).dot(pb["Z0"].astype(rr.LD)))
    broken = []
    if entries.max() > 1.0:
        broken.append("an entry above 1")
    if not np.all(entries[np.arange(len(rows)), rows] == 1.0):
        broken.append("diagonal")
    where = {int(r): i for i, r in enumerate(rows)}
    for a, b in pb["twins"]:
        if entries[where[a], b] != 1.0 or entries[where[b], a] != 1.0:
            broken.append("twins %d %d" % (a, b))
    if pb["name"] == "d":
        if not np.array_equal(entries, (rows[:, None] == np.arange(n)[None, :]).astype(np.float64)):
            broken.append("identity")
        if not np.array_equal(out, pb["Z0"][rows]):
            broken.append("K Z0 is not Z0")
    return r_entry, r_prod, broken


@pytest.mark.parametrize("case", rr.KV_CASES, ids=str)
def test_emulated_kv_meets_the_bound(case):
    pb = rr.kv_problem(case)
    rows = _kv_rows(pb)
    entries, out = rr.emulate_product(pb["X"], pb["X"], pb["gamma"], pb["Z0"], rows)
    r_entry, r_prod, broken = _judge_kv(pb, rows, entries, out)
    print("emulated K V %s: max |got - want| / bound: entries %.3f, product %.3f" % (case, r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0 and not broken, (r_entry, r_prod, broken)


@pytest.mark.parametrize("case", rr.CROSS_CASES, ids=str)
def test_emulated_cross_meets_the_bound(case):
    pb = rr.cross_problem(case)
    rows = np.arange(pb["m"]) if pb["rows"] is None else pb["rows"]
    entries, out = rr.emulate_product(pb["Y"], pb["XS"], pb["gamma"], pb["V"], rows, same_set=False)
    K, s = rr.reference(pb["Y"], pb["XS"], pb["gamma"], rows)
    E = rr.entry_E(pb["Y"], pb["XS"], pb["gamma"], s, rows)
    V = pb["V"].astype(rr.LD)
    r_entry = rr.ratio(entries, K, rr.entry_bound(K, E))
    r_prod = rr.ratio(out, K.dot(V), rr.entry_bound(K, E, pb["s"]).dot(V))
    print("emulated cross %s: max |got - want| / bound: entries %.3f, product %.3f" % (case, r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0
    # the inputs are what the case says: copies at d2 about 0, far rows whose whole output row is tiny
    kind = pb["kind"][rows]
    small = np.abs(K.dot(V)).astype(np.float64)
    if np.any(kind == 1):
        assert small[kind == 1].max() < 1e-30 * small[kind == 0].max()


@pytest.mark.parametrize("case", rr.DISTANCE_CASES, ids=str)
def test_emulated_distance_meets_the_bound(case):
    for j in case[2]:
        X, gamma = rr.distance_problem(case, j)
        d = rr.emulate_distance(X, gamma, j)
        t, bound = rr.distance_reference(X, gamma, j)
        r = rr.ratio(d * d, t, bound)
        print("emulated distance column %s j %d: max |d^2 - t| / bound %.3f" % (case[:2], j, r))
        assert r <= 1.0 and d[j] == 0.0 and d[(j + 1) % case[0]] == 0.0


@pytest.mark.parametrize("case", rr.RESIDENT_CASES, ids=str)
def test_emulated_resident_meets_the_bound(case):
    pb = rr.resident_problem(case)
    pb.update(X=pb["Xs"], twins=[], name="a")
    rows = np.arange(pb["n"])
    entries, out = rr.emulate_product(pb["Xs"], pb["Xs"], pb["gamma"], pb["Z0"], rows)
    r_entry, r_prod, broken = _judge_kv(pb, rows, entries, out)
    print("emulated resident %s: max |got - want| / bound: entries %.3f, product %.3f" % (case, r_entry, r_prod))
    assert r_entry <= 1.0 and r_prod <= 1.0 and not broken


# fault -> the case whose inputs notice it, and how: "bound" (a ratio above 1) or the exact fact that breaks
PLANTED = {"drop_last_feature": ((130, 17, 3, "c"), "bound"),
           "skip_last_tile": ((4200, 17, 3, "a"), "bound"),
           "padding_tile_as_data": ((64, 16, 32, "a"), "bound"),
           "neighbour_norm": ((130, 17, 3, "c"), "bound"),
           "no_clamp": ((130, 17, 3, "c"), "an entry above 1"),
           "diagonal_value": ((130, 16, 40, "d"), "K Z0 is not Z0"),
           "diagonal_local": ((130, 16, 40, "d"), "identity"),
           "sum_leaves_out_split": ((130, 17, 3, "c"), "bound")}


def test_every_fault_is_planted():
    assert sorted(PLANTED) == sorted(rr.FAULTS)
    assert all(case in rr.KV_CASES for case, _ in PLANTED.values())


@pytest.mark.parametrize("fault", sorted(PLANTED), ids=str)
def test_planted_faults_are_caught(fault):
    """The unclamped d2 stays inside the bound by the bound's own derivation (rbf_restatement, exact fact 2):
    that fault is noticed by an entry above 1 between rows one ulp apart.  A diagonal one ulp below 1 is inside
    any rounding bound too: family (d) notices it bit for bit."""
    case, how = PLANTED[fault]
    pb = rr.kv_problem(case)
    rows = _kv_rows(pb)
    entries, out = rr.emulate_product(pb["X"], pb["X"], pb["gamma"], pb["Z0"], rows, fault=fault)
    r_entry, r_prod, broken = _judge_kv(pb, rows, entries, out)
    print("planted %s on %s: ratios %.3g (entries) %.3g (product), exact facts broken: %s"
          % (fault, case, r_entry, r_prod, broken))
    if how == "bound":
        assert max(r_entry, r_prod) > 1.0
    else:
        assert how in broken


def test_split_arithmetic():
    """kernel_kv and kernel_cross (launch_kernel_product), restated: the splits the cases are named for.  k_rbf_kv's grid
    covers n_pad = n rounded up to 128, so n = 64 has two splits (the second leaves its loop at once) and n = 130
    four, three of one data tile each and an empty one."""
    def kv(n):
        nsplit, tps = rr.kv_splits(n)
        return nsplit, tps, rr.tiles_done(n, rr.round_up(n, 128) // 64, nsplit, tps, True)

    assert kv(1) == (2, 1, [1, 0])
    assert kv(63) == (2, 1, [1, 0]) and kv(64) == (2, 1, [1, 0]) and kv(65) == (2, 1, [1, 1])
    assert kv(128) == (2, 1, [1, 1]) and kv(129) == (4, 1, [1, 1, 1, 0]) and kv(130) == (4, 1, [1, 1, 1, 0])
    assert kv(900) == (16, 1, [1] * 15 + [0])
    assert kv(4200) == (14, 5, [5] * 13 + [1])

    def cross(m, s):
        nsplit, tps = rr.cross_splits(m, s)
        return nsplit, tps, rr.tiles_done(s, rr.round_up(s, 64) // 64, nsplit, tps, False)

    assert cross(1, 1) == (1, 1, [1]) and cross(63, 64) == (1, 1, [1]) and cross(64, 65) == (2, 1, [1, 1])
    assert cross(65, 129) == (3, 1, [1, 1, 1]) and cross(200, 129) == (3, 1, [1, 1, 1])
    assert cross(16300, 300) == (3, 2, [2, 2, 1])          # the case with a partial last split
    assert all(cross(m, s)[1] == 1 for m, s, _, _ in rr.CROSS_CASES[:-1])
