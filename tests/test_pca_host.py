"""PCA of resident data, host side (no GPU needed).

* tests/pca_restatement.py -- the device's route in NumPy float64 -- against
  ``sklearn.decomposition.PCA(n_components=q, svd_solver='full')`` on the end-to-end inputs of
  tests/test_gpu_pca.py: eigenvalues, components, PCs and every sign.  The restatement is held to twice the
  perturbation bounds of its own Gram rounding error (Weyl / Davis-Kahan; scikit-learn's SVD commits an error of
  its own, no larger), and the figures are printed.
* the sign rule against scikit-learn's ``svd_flip(u_based_decision=False)``; ``truncate`` against a direct fit;
  every refusal with the device layer stubbed so that a call into it fails the test; ``copy.deepcopy``.
* the two new entry points are declared, exported and bound.
* csrc/gram_plan.h through tests/gram_plan_dump.cpp over the cross product of side, n and p at the tile, chunk and
  pad edges and far beyond, both element sizes and a few CU counts.
"""
import copy
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.decomposition import PCA
from sklearn.utils.extmath import svd_flip

import convex_dim_red as cdr
from convex_dim_red import _backend, pca
from convex_dim_red.preprocessing import DeviceData

import pca_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrix-factorization-case-studies_amd", "csrc")
NEW_SYMBOLS = ("aa_data_gram", "aa_set_data_projected")
SHAPES = [(40, 300, 8), (300, 40, 8), (129, 257, 12), (1000, 167, 12), (17, 16, 5)]


# ------------------------------------------------------------------ the restatement against scikit-learn
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,p,q", SHAPES)
def test_restatement_against_sklearn_full(n, p, q, dtype):
    Xd = pr.stored(pr.low_rank(n, p, q), dtype)
    sk = PCA(n_components=q, svd_solver="full").fit(Xd)
    sk_pcs = sk.transform(Xd)
    for side in ("rows", "cols"):
        m = pr.fit(Xd, q, side=side)
        lam_sk = sk.singular_values_ ** 2
        weyl, dk = pr.perturbation_bounds(Xd, m.mean_, side, m.eigenvalues_, q)
        d_lam = np.abs(m.eigenvalues_[:q] - lam_sk).max()
        sin = pr.sines(m.components_, sk.components_)
        cos = np.abs(np.sum(m.components_ * sk.components_, axis=1))
        pcs = pr.project(Xd, m.mean_, m.components_)
        d_pcs = np.abs(pcs - sk_pcs).max()
        print("%dx%d q=%d %s %s: eigenvalues %.2e of the largest (Weyl %.2e), max 1-|cos| %.2e, max sin %.2e "
              "(Davis-Kahan %.2e), PCs %.2e of the largest"
              % (n, p, q, dtype, side, d_lam / lam_sk[0], weyl / lam_sk[0], (1 - cos).max(), sin.max(), dk.max(),
                 d_pcs / np.abs(sk_pcs).max()))
        assert d_lam <= 2 * weyl
        assert np.all(sin <= 2 * dk)
        # the PCs: the component's error times the row's norm, and the projection's own rounding
        row_norm = np.linalg.norm(pr.centred(Xd, m.mean_), axis=1)
        assert np.all(np.abs(pcs - sk_pcs) <= 2 * (np.outer(row_norm, np.sqrt(2.0) * dk)
                                                   + pr.project_bound(Xd, m.mean_, m.components_)))
        assert np.array_equal(np.sign(np.sum(m.components_ * sk.components_, axis=1)), np.ones(q))   # every sign
        assert np.allclose(m.explained_variance_, sk.explained_variance_, rtol=1e-12, atol=0)
        assert np.allclose(m.explained_variance_ratio_, sk.explained_variance_ratio_, rtol=1e-12, atol=0)
        assert np.allclose(m.singular_values_, sk.singular_values_, rtol=1e-12, atol=0)
        assert np.isclose(m.noise_variance_, sk.noise_variance_, rtol=1e-9, atol=0)
        assert np.allclose(m.mean_, sk.mean_, rtol=1e-13, atol=1e-13)


def test_sign_rule():
    rng = np.random.RandomState(0)
    C = rng.standard_normal((6, 9))
    C[1] = -np.abs(C[1])
    C[2, 3], C[2, 7] = -5.0, 5.0                      # a tie of magnitudes: the first index decides
    C[3, 0], C[3, 8] = 7.0, -7.0
    out = pca.orient(C)
    _, want = svd_flip(np.eye(6), C.copy(), u_based_decision=False)
    assert np.array_equal(out, want)
    assert out[2, 3] == 5.0 and out[2, 7] == -5.0 and out[3, 0] == 7.0
    assert np.array_equal(np.abs(out), np.abs(C))
    assert np.array_equal(pca.orient(out), out)
    assert np.array_equal(pr.orient(C), out)          # the restatement's rule is the same one


def _host_model(Xd, q, side="auto", center=True):
    """A ResidentPCA from host arithmetic alone (the package's own host functions on the restatement's Gram)."""
    n, p = Xd.shape
    if side == "auto":
        side = "rows" if n <= p else "cols"
    mean = Xd.mean(axis=0) if center else np.zeros(p)
    lam, vec = pca.gram_eigen(pr.gram(Xd, mean if center else None, side), q, n, p)
    if side == "cols":
        comps = vec.T
    else:
        A = pca.row_side_coefficients(lam, vec)
        comps = A.dot(Xd) - np.outer(A.sum(axis=1), mean)
    return cdr.ResidentPCA(pca.orient(comps), mean, lam, n, center, side)


ATTRS = ("components_", "mean_", "explained_variance_", "explained_variance_ratio_", "singular_values_",
         "noise_variance_", "eigenvalues_", "n_samples_", "n_features_in_")


@pytest.mark.parametrize("n,p,q", SHAPES)
def test_truncate_is_a_direct_fit(n, p, q):
    Xd = pr.low_rank(n, p, q)
    full = _host_model(Xd, q)
    for k in range(1, q + 1):
        cut, direct, want = full.truncate(k), _host_model(Xd, k), pr.fit(Xd, k)
        assert cut.n_components_ == k and cut.components_.shape == (k, p)
        for name in ATTRS:
            # by rows the host's BLAS may sum A X in another order for another number of rows of A
            if name == "components_" and full.side_ == "rows":
                assert np.abs(cut.components_ - direct.components_).max() <= 1e-13, k
            else:
                assert np.array_equal(getattr(cut, name), getattr(direct, name)), (k, name)
            assert np.allclose(getattr(cut, name), getattr(want, name), rtol=1e-9, atol=1e-12), (k, name)
    cut = full.truncate(1)
    cut.components_[:] = 0.0                          # a copy: the parent keeps its arrays
    assert np.any(full.components_[0] != 0.0)
    for bad in (0, q + 1, 1.0, True, None):
        with pytest.raises(ValueError, match="truncate"):
            full.truncate(bad)


def test_model_is_deepcopy_safe_and_inverts():
    Xd = pr.low_rank(40, 30, 6)
    model = _host_model(Xd, 8)
    twin = copy.deepcopy(model)
    for name in ATTRS:
        assert np.array_equal(getattr(twin, name), getattr(model, name))
    assert twin.components_ is not model.components_
    pcs = pr.project(Xd, model.mean_, model.components_)
    back = model.inverse_transform(pcs)
    assert np.array_equal(back, pcs.dot(model.components_) + model.mean_)
    assert np.abs(back - Xd).max() < 0.1             # rank 8 + noise 1e-2, 8 components kept
    with pytest.raises(ValueError, match="inverse_transform"):
        model.inverse_transform(pcs[:, :7])


# ------------------------------------------------------------------ refusals, decided on the host
class _Handle(object):
    """Stands in for an open context behind a DeviceData: anything it is asked beyond these names fails the test."""
    h = 1
    device = 0
    implicit = False

    def __init__(self, code=_backend.AA_F64):
        self.dtype_code = code

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_backend, "Context", refuse)
    monkeypatch.setattr(_backend, "require_gpu", refuse)


def _resident(shape, code=_backend.AA_F64, **attrs):
    handle = _Handle(code)
    for name, value in attrs.items():
        setattr(handle, name, value)
    return DeviceData(handle, shape, None, shape[1:])


@pytest.mark.parametrize("shape,kw,match", [
    ((10, 4), dict(n_components=0), "positive integer"),
    ((10, 4), dict(n_components=-1), "positive integer"),
    ((10, 4), dict(n_components=2.0), "positive integer"),
    ((10, 4), dict(n_components=True), "positive integer"),
    ((10, 4), dict(n_components=None), "positive integer"),
    ((10, 4), dict(n_components=5), "at most 4"),
    ((4, 10), dict(n_components=4), "at most 3"),                     # centred: n - 1
    ((4, 10), dict(n_components=5, center=False), "at most 4"),
    ((1000, 400), dict(n_components=257), "at most 256"),
    ((9000, 8193), dict(n_components=3), "GRAM_MAX_D = 8192"),
    ((9000, 100), dict(n_components=3, side="rows"), "GRAM_MAX_D = 8192"),
    ((100, 9000), dict(n_components=3, side="cols"), "GRAM_MAX_D = 8192"),
    ((10, 4), dict(n_components=2, side="both"), "side must be"),
])
def test_pca_refuses_on_the_host(no_device, shape, kw, match):
    with pytest.raises(ValueError, match=match):
        _resident(shape).pca(**kw)


def test_pca_refuses_a_block_without_a_data_matrix(no_device):
    with pytest.raises(ValueError, match="data form"):
        _resident((10, 10), implicit=True).pca(2)


def test_pca_refuses_an_unresolved_component(no_device):
    """Rank 3 data, 5 components asked: the fourth eigenvalue is rounding noise of the Gram matrix.  The device layer
    is stubbed by the restatement's mean and Gram; nothing else may be called."""
    rng = np.random.RandomState(1)
    Xd = rng.standard_normal((30, 3)).dot(rng.standard_normal((3, 12)))
    Xd = Xd - Xd.mean(axis=0)                        # centred rank 3 (the mean is removed once more, exactly)
    calls = []

    def moments():
        calls.append("moments")
        return Xd.mean(axis=0), Xd.var(axis=0)

    def data_gram(side, shift=None):
        calls.append(side)
        return pr.gram(Xd, shift, side)
    for side in ("rows", "cols"):
        block = _resident(Xd.shape, data_column_moments=moments, data_gram=data_gram)
        with pytest.raises(ValueError, match=r"component 5 is not resolved.*3 components are resolved"):
            block.pca(5, side=side)
    assert calls == ["moments", "rows", "moments", "cols"]


def test_transform_and_score_refuse_on_the_host(no_device):
    model = _host_model(pr.low_rank(40, 30, 6), 6)
    wide = cdr.ResidentPCA(np.eye(70)[:64], np.zeros(70), np.ones(70), 100, True, "cols")
    with pytest.raises(ValueError, match="DeviceData block expected"):
        model.transform(np.zeros((5, 30)))
    with pytest.raises(ValueError, match="fitted on 30 features"):
        model.transform(_resident((5, 31)))
    with pytest.raises(ValueError, match="float32 or float64"):
        model.transform(_resident((5, 30)), dtype=np.int32)
    with pytest.raises(ValueError, match="only for a float32 block"):
        model.transform(_resident((5, 30)), dtype=np.float32)
    with pytest.raises(ValueError, match="fitted on 30 features"):
        model.score(_resident((5, 29)))
    with pytest.raises(ValueError, match=r"pcs must be \(5, 6\)"):
        model.score(_resident((5, 30)), pcs=np.zeros((5, 5)))
    with pytest.raises(ValueError, match="64 components; the scores pass takes 63"):
        wide.score(_resident((5, 70)))
    assert wide.truncate(63).n_components_ == 63
    closed = _resident((5, 30))
    closed._ctx.h = 0
    with pytest.raises(RuntimeError, match="closed"):
        model.transform(closed)
    with pytest.raises(RuntimeError, match="closed"):
        closed.pca(2)


# ------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aa_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(aa_ctx \*ctx, " % name, header, re.M), name
        assert name in _backend.EXPORTED_SYMBOLS
    assert "ResidentPCA" in cdr.__all__ and cdr.ResidentPCA is pca.ResidentPCA
    assert re.search(r"#define AA_MAX_PROJECTED\s+%d\b" % _backend.MAX_PROJECTED, header)
    assert re.search(r"#define AA_GRAM_ROWS\s+%d\b" % _backend.GRAM_SIDES.index("rows"), header)
    assert re.search(r"#define AA_GRAM_COLS\s+%d\b" % _backend.GRAM_SIDES.index("cols"), header)
    plan = open(os.path.join(CSRC, "gram_plan.h")).read()
    assert re.search(r"GRAM_MAX_D = %d;" % _backend.GRAM_MAX_D, plan)
    lib = ctypes.CDLL(_backend.library_path())       # the suite runs on a built tree, as tests/test_cpu_host.py assumes
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


# ------------------------------------------------------------------ gram_plan.h
TILE, CHUNK, BUDGET, BLOCKS_PER_CU = 64, 32, 64 << 20, 2
EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 167, 255, 256, 257, 1000, 1610, 4096, 8191, 8192, 25000,
         89120, 100000, 1000003)
CUS = (1, 64, 256, 304)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or (os.path.exists("/opt/rocm/llvm/bin/clang++") and "/opt/rocm/llvm/bin/clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gram_plan") / "gram_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "gram_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    cases = [c for c in itertools.product((0, 1), EDGES, EDGES, (4, 8), CUS)
             if (c[1] if c[0] == 0 else c[2]) <= 8192]                   # the side's d is capped by the entry point
    rows = run(["G %d %d %d %d %d" % c for c in cases])
    assert len(rows) == len(cases)
    fields = np.array([[int(v) for v in row.split()] for row in rows], dtype=np.int64)
    return run, np.array(cases, dtype=np.int64), fields


def test_gram_plan_covers_the_contraction_once(plans):
    _, cases, f = plans
    side, n, p = cases[:, 0], cases[:, 1], cases[:, 2]
    d, tiles, pairs, K, nsplit, split_len, partial_bytes, g_ld = f.T
    assert np.array_equal(d, np.where(side == 0, n, p)) and np.array_equal(K, np.where(side == 0, p, n))
    assert np.array_equal(tiles, (d + TILE - 1) // TILE) and np.array_equal(pairs, tiles * (tiles + 1) // 2)
    assert np.array_equal(g_ld, tiles * TILE)
    # split s takes [s split_len, min((s + 1) split_len, K)): every index in exactly one split, none empty, whole chunks
    assert np.all(split_len % CHUNK == 0) and np.all(split_len >= CHUNK) and np.all(nsplit >= 1)
    assert np.all((nsplit - 1) * split_len < K) and np.all(nsplit * split_len >= K)
    # the examples: few tiles over a long contraction split, and their last split is short
    for want in ((1, 89120, 167), (0, 64, 25000)):
        hit = np.all(cases[:, :3] == want, axis=1) & (cases[:, 4] == 256)
        assert hit.sum() == 2 and np.all(nsplit[hit] > 10) and np.all(nsplit[hit] * split_len[hit] > K[hit])


def test_gram_plan_partials_and_the_single_split(plans):
    _, cases, f = plans
    cus = cases[:, 4]
    d, tiles, pairs, K, nsplit, split_len, partial_bytes, g_ld = f.T
    assert np.array_equal(partial_bytes, np.where(nsplit > 1, nsplit * pairs * TILE * TILE * 8, 0))
    assert np.all(partial_bytes <= BUDGET)
    # from `cus` tile pairs on: one split, no partials
    full = pairs >= cus
    assert np.all(nsplit[full] == 1) and np.all(partial_bytes[full] == 0)
    for want in ((1, 100000, 4096), (0, 1610, 25000)):
        hit = np.all(cases[:, :3] == want, axis=1) & (cases[:, 4] == 256)
        assert hit.sum() == 2 and np.all(nsplit[hit] == 1)
    # below: never more blocks than aimed at (the rounding of the split length only lowers the count), and a split
    # wherever the contraction has the chunks for it and the budget the room
    few = ~full
    chunks = (K + CHUNK - 1) // CHUNK
    want = np.minimum(np.minimum((BLOCKS_PER_CU * cus + pairs - 1) // pairs, BUDGET // (pairs * TILE * TILE * 8)), chunks)
    assert np.all(nsplit[few] <= np.maximum(want[few], 1))
    assert np.all(nsplit[few & (want >= 2)] >= 2)
    assert np.all(split_len[few] == (chunks[few] + np.maximum(want[few], 1) - 1) // np.maximum(want[few], 1) * CHUNK)
    # the element size does not enter
    es4, es8 = cases[:, 3] == 4, cases[:, 3] == 8
    assert np.array_equal(f[es4], f[es8])


def test_gram_plan_splits_the_gpu_test_shapes(plans):
    """The shapes tests/test_gpu_pca.py runs for the split path: at 256 compute units (and at the other counts of an
    Instinct part) each is cut into more than one split and the last split is short, with the figures its table states."""
    run, _, _ = plans
    stated = {(0, 200, 3001): (47, 64, 57), (0, 65, 5000): (157, 32, 8), (1, 5000, 167): (79, 64, 8),
              (1, 2500, 257): (27, 96, 4)}
    shapes = [(s, n, p) for s, side in enumerate(("rows", "cols")) for n, p in pr.SPLIT_SHAPES[side]]
    assert sorted(shapes) == sorted(stated)
    for cus in (64, 256, 304):
        rows = run(["G %d %d %d %d %d" % (s, n, p, es, cus) for s, n, p in shapes for es in (4, 8)])
        for (s, n, p), row in zip([c for c in shapes for _ in (4, 8)], rows):
            d, tiles, pairs, K, nsplit, split_len, partial_bytes, g_ld = (int(v) for v in row.split())
            assert d <= 300 and nsplit > 1 and nsplit * split_len > K > (nsplit - 1) * split_len, (s, n, p, cus)
            assert partial_bytes == nsplit * pairs * TILE * TILE * 8
            if cus == 256:
                assert (nsplit, split_len, K - (nsplit - 1) * split_len) == stated[s, n, p], (s, n, p)


def test_gram_plan_names_every_tile_pair_once(plans):
    run, _, _ = plans
    sizes = (1, 2, 3, 4, 5, 26, 64, 127, 128)
    for tiles, row in zip(sizes, run(["P %d" % t for t in sizes])):
        got = [tuple(int(v) for v in item.split(":")) for item in row.split()]
        assert got == [(i, j) for i in range(tiles) for j in range(i, tiles)]
