"""Builds tests/host/small_eig_main.cpp over neutfem_amd/csrc/nf_small_eig.h (plain C++, no device) with
-fsanitize=address,undefined and runs it as a program of its own: the small eigen-solver and the Cholesky factor of the block outer
iteration (nf_solve_modes) against numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the build needs a host C++ compiler anyway"
    out = str(tmp_path_factory.mktemp("small_eig") / "small_eig")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "small_eig_main.cpp")])
    return out


def _run(exe, problems):
    """problems: list of (kind, matrix); returns one dict per problem"""
    text = "".join(f"{kind} {len(M)} " + " ".join(repr(float(v)) for v in np.asarray(M).ravel()) + "\n" for kind, M in problems)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    out, cur = [], None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] in ("eig", "chol"):
            cur = dict(kind=t[0], n=int(t[1]), rc=int(t[2]), w=[], v=[], l=[]); out.append(cur)
        elif t[0] in ("w", "v", "l"):
            cur[t[0]].append([float(x) for x in t[1:]])
        else:
            cur[t[0]] = float(t[1])
    assert len(out) == len(problems)
    return out


def _known_spectrum(n, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, n)) + 2.0 * np.eye(n)
    return X @ np.diag(lam) @ np.linalg.inv(X), X


def test_real_spectra(exe):
    rng = np.random.default_rng(1)
    probs, want = [], []
    probs.append(("eig", [[3.5]])); want.append([3.5])
    probs.append(("eig", np.diag([0.2, 1.7, -0.4, 1.1]))); want.append([1.7, 1.1, 0.2, -0.4])
    for seed in range(6):                                         # 8 x 8 nonsymmetric, known real spectrum
        lam = np.sort(rng.uniform(0.1, 1.1, 8))[::-1]
        probs.append(("eig", _known_spectrum(8, lam, seed)[0])); want.append(lam)
    lam = np.array([1.028986, 1.015486, 1.0154859, 0.999342, 0.97, 0.9])   # a close pair, as the leading spectrum of IAEA-2D
    probs.append(("eig", _known_spectrum(6, lam, 11)[0])); want.append(lam)
    for (kind, M), lam, res in zip(probs, want, _run(exe, probs)):
        M = np.asarray(M, dtype=float)
        assert res["rc"] == 0
        w = np.array(res["w"])
        assert np.all(w[:, 1] == 0.0) and np.all(np.diff(w[:, 0]) <= 0.0)
        # Bauer-Fike: a backward error of n eps ||A|| moves an eigenvalue by at most cond(X) times that; factor 10 for the constants
        tol = 10 * len(M) * np.finfo(float).eps * np.linalg.norm(M, 2) * np.linalg.cond(np.linalg.eig(M)[1])
        assert np.abs(w[:, 0] - lam).max() <= max(tol, 1e-15), (np.abs(w[:, 0] - lam).max(), tol)
        V = np.array(res["v"]).T
        assert np.abs(np.linalg.norm(V, axis=0) - 1.0).max() <= 1e-14
        assert res["res"] <= 1e-13 * np.abs(M).sum() and np.abs(M @ V - V * w[:, 0]).max() <= 1e-13 * np.abs(M).sum()


def test_eigenvalues_of_well_conditioned_8x8_to_1e12(exe):
    """X close to orthogonal, so the eigenvalues are determined to rounding: 1e-12 absolute on a spectrum of size 1"""
    rng = np.random.default_rng(5)
    probs, want = [], []
    for seed in range(8):
        Q, _ = np.linalg.qr(rng.standard_normal((8, 8)))
        X = Q @ (np.eye(8) + 0.2 * rng.standard_normal((8, 8)))
        lam = np.sort(rng.uniform(0.3, 1.05, 8))[::-1]
        probs.append(("eig", X @ np.diag(lam) @ np.linalg.inv(X))); want.append(lam)
    for lam, res in zip(want, _run(exe, probs)):
        assert res["rc"] == 0 and np.abs(np.array(res["w"])[:, 0] - lam).max() <= 1e-12


def test_repeated_eigenvalue_with_full_eigenspace(exe):
    A, X = _known_spectrum(5, np.array([1.2, 0.8, 0.8, 0.8, 0.1]), 3)
    sym = np.diag([2.0, 2.0, 1.0])                                # exactly repeated, already diagonal
    res = _run(exe, [("eig", A), ("eig", sym), ("eig", np.eye(4))])
    for r, M in zip(res, (A, sym, np.eye(4))):
        V = np.array(r["v"]).T
        assert r["rc"] == 0 and np.linalg.matrix_rank(V, tol=1e-6) == len(M)      # independent vectors inside the eigenspace
        assert r["res"] <= 1e-12
    w = np.array(res[0]["w"])
    assert np.abs(w[:, 0] - [1.2, 0.8, 0.8, 0.8, 0.1]).max() <= 1e-7 and np.abs(w[:, 1]).max() <= 1e-7   # a triple root moves like eps^(1/3) at worst


def test_rotation_block_is_reported_as_complex(exe):
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s], [s, c]])
    A = np.zeros((4, 4)); A[0, 0] = 2.0; A[1:3, 1:3] = 0.9 * R; A[3, 3] = 0.1; A[0, 2] = 0.3; A[1, 3] = -0.2
    res = _run(exe, [("eig", R), ("eig", A)])
    w = np.array(res[0]["w"])
    assert res[0]["rc"] == 0 and np.allclose(w[:, 0], c, atol=1e-15) and w[0, 1] > 0 > w[1, 1] and np.allclose(np.abs(w[:, 1]), s, atol=1e-15)
    w = np.array(res[1]["w"])
    assert np.allclose(w[:, 0], [2.0, 0.9 * c, 0.9 * c, 0.1], atol=1e-14) and np.allclose(w[:, 1], [0, 0.9 * s, -0.9 * s, 0], atol=1e-14)
    assert res[0]["res"] <= 1e-14 and res[1]["res"] <= 1e-14      # the two columns span the invariant plane: A [u w] = [u w] [[a, b], [-b, a]]


def test_cholesky_and_rank_loss(exe):
    rng = np.random.default_rng(2)
    Z = rng.standard_normal((50, 8)) * 10.0 ** rng.uniform(-3, 3, 8)
    G = Z.T @ Z
    Zd = Z.copy(); Zd[:, 5] = 2.0 * Zd[:, 1] - Zd[:, 3]           # rank-deficient Gram matrix: column 5 depends on 1 and 3
    Gd = Zd.T @ Zd
    res = _run(exe, [("chol", G), ("chol", Gd), ("chol", [[4.0]]), ("chol", [[0.0]]), ("chol", [[1.0, 2.0], [2.0, 1.0]])])
    assert res[0]["rc"] == 0 and np.abs(np.array(res[0]["l"]) - np.linalg.cholesky(G)).max() <= 1e-12 * np.abs(G).max() ** 0.5
    assert res[0]["orth"] <= 1e-9
    assert res[1]["rc"] == -6                                     # pivot 5 (0-based) is the one that vanishes
    assert res[2]["rc"] == 0 and res[2]["l"] == [[2.0]]
    assert res[3]["rc"] == -1 and res[4]["rc"] == -2
