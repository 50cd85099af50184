"""The fused ALS half-sweep kernel (K27, ops.als) against the normal equations formed row by row in numpy.

eps = 2^-52, k the rank, norms are max norms.
  exact Gram     integer factors and ratings make A and b exact in fp64 in any order, so the only error is the
                 Cholesky solve's: |A x - b| <= 8 k^2 eps |A| |x| (backward error gamma_{3k+1} | |R^T| |R| | with
                 | |R^T| |R| | <= k |A|, times 2); the residual is evaluated in long double
  plain solve    real inputs against numpy.linalg.solve: |x - x_ref| <= 16 k^2 eps cond(A) |x_ref|, both solvers
                 within the backward bound, the forward errors add; cond(A) < 1e4 is asserted
  ALS.fit        the model against the same sweeps in long double: the kernel's largest factor error is at most
                 4 x the dense body's own plus 1e-13 (another summation order over three sweeps)"""
import numpy as np
import pytest
import torch

from synapseml_amd.core import DataFrame
from synapseml_amd.ops import als as AO
from synapseml_amd.recommendation import ALS

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
LENS = (0, 1, 3, 4, 5, AO.L - 1, AO.L, AO.L + 1, 2 * AO.L + 3)


def _system(Y, y, v, lam, alpha, implicit):
    """A, b of a row with ratings v of the factor rows y (of all rows Y), in the dtype of the inputs"""
    eye = np.eye(Y.shape[1])
    if implicit:
        return Y.T @ Y + (y.T * (alpha * v)) @ y + lam * eye, ((1 + alpha * v) * (v > 0)) @ y
    return y.T @ y + lam * max(len(v), 1) * eye, v @ y


def _sweep(prep, side, X0, Y, lam, alpha, implicit, nonneg=False):
    X = AO.factors(torch.from_numpy(X0), "cuda")
    AO.half_sweep(prep, side, X, AO.factors(torch.from_numpy(Y.astype(np.float64)), "cuda"), lam, alpha, implicit,
                  nonneg)
    return X.cpu().numpy()


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 64])
def test_exact_gram(k, implicit):
    rng = np.random.default_rng(k)
    nI = max(LENS) + 50
    u = np.repeat(np.arange(len(LENS)), LENS)
    i = np.concatenate([rng.choice(nI, n, replace=False) for n in LENS])
    r = rng.integers(0 if implicit else -3, 6, len(u))
    Y, X0 = rng.integers(-3, 4, (nI, k)), rng.standard_normal((len(LENS), k))
    prep = AO.prepare(u, i, r, len(LENS), nI)
    x = _sweep(prep, 0, X0, Y, 0.5, 2.0, implicit)
    assert np.array_equal(x, _sweep(prep, 0, X0, Y, 0.5, 2.0, implicit), equal_nan=True)
    for row, n in enumerate(LENS):
        if n == 0 and not implicit:
            assert np.array_equal(x[row].view(np.int64), X0[row].view(np.int64))
            continue
        A, b = _system(Y, Y[i[u == row]], r[u == row], 0.5, 2, implicit)
        res = np.abs(A.astype(np.longdouble) @ x[row].astype(np.longdouble) - b).max()
        bound = 8 * k * k * EPS * np.abs(A).sum(1).max() * np.abs(x[row]).max()
        print(f"k={k} implicit={implicit} n={n}: residual {float(res):.3e} bound {bound:.3e}")
        assert res <= bound
        assert n > 0 or not x[row].any()


@pytest.mark.parametrize("mode", ["explicit", "implicit", "nonnegative"])
@pytest.mark.parametrize("k", [10, 48])
def test_against_linalg_solve(k, mode):
    rng = np.random.default_rng(k)
    nU, nI, implicit, lam = 150, 37, mode == "implicit", 2.0
    u, i = np.nonzero(rng.random((nU, nI)) < 0.3)
    r = rng.uniform(0.5, 5.0, len(u)) if implicit else 2.0 * rng.standard_normal(len(u))
    U, V0 = rng.standard_normal((nU, k)), rng.standard_normal((nI, k))
    x = _sweep(AO.prepare(u, i, r, nU, nI), 1, V0, U, lam, 0.7, implicit, mode == "nonnegative")
    for row in range(nI):
        A, b = _system(U, U[u[i == row]], r[i == row], lam, 0.7, implicit)
        ref, cond = np.linalg.solve(A, b), np.linalg.cond(A, np.inf)
        assert cond < 1e4
        if mode == "nonnegative":
            ref = np.maximum(ref, 0.0)
        assert np.abs(x[row] - ref).max() <= 16 * k * k * EPS * cond * np.abs(ref).max()


def _eliminate(A, b):
    """plain elimination without pivoting (A is positive definite), in the dtype of A"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for c in range(n):
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c]
        b[c + 1:] -= f * b[c]
    for c in range(n - 1, -1, -1):
        b[c] = (b[c] - A[c, c + 1:] @ b[c + 1:]) / A[c, c]
    return b


def _fit_reference(u, i, r, k, iters, lam, alpha, implicit, seed):
    g = torch.Generator().manual_seed(seed)
    F = [(torch.rand(int(ids.max()) + 1, k, generator=g, dtype=torch.float64) * 0.1).numpy().astype(np.longdouble)
         for ids in (u, i)]
    ids, r = (u, i), r.astype(np.longdouble)
    for _ in range(iters):
        for side in (0, 1):
            X, Y = F[side], F[1 - side]
            for row in range(len(X)):
                sel = ids[side] == row
                if sel.any() or implicit:
                    X[row] = _eliminate(*_system(Y, Y[ids[1 - side][sel]], r[sel], lam, alpha, implicit))
    return F


def _ratings(implicit):
    rng = np.random.default_rng(5)
    u, i = np.nonzero(rng.random((40, 25)) < 0.3)
    r = rng.integers(1, 6, len(u)).astype(np.float64) if implicit else rng.uniform(-2.0, 5.0, len(u))
    return u, i, r


def _fit(monkeypatch, u, i, r, flag, **params):
    """(user factors, item factors, sides of the kernel calls) of ALS.fit with SML_ALS=flag, or unset where flag
    is None; with "0" a kernel call fails"""
    calls, real = [], AO.half_sweep

    def counted(prep, side, *rest):
        calls.append(side)
        real(prep, side, *rest)

    if flag is None:
        monkeypatch.delenv("SML_ALS", raising=False)
    else:
        monkeypatch.setenv("SML_ALS", flag)
    monkeypatch.setattr(AO, "half_sweep", pytest.fail if flag == "0" else counted)
    m = ALS(maxIter=3, **params).fit(DataFrame({"user": u.astype(np.float64), "item": i.astype(np.float64),
                                                 "rating": r}))
    monkeypatch.setattr(AO, "half_sweep", real)
    return np.asarray(m.getUserFactors()), np.asarray(m.getItemFactors()), calls


@pytest.mark.parametrize("implicit", [False, True])
def test_fit_route(monkeypatch, implicit):
    u, i, r = _ratings(implicit)
    est = ALS(rank=5, implicitPrefs=implicit)
    ref = _fit_reference(u, i, r, 5, 3, est.getRegParam(), est.getAlpha(), implicit, est.getSeed())
    err = {}
    for flag in ("0", None):
        U, V, calls = _fit(monkeypatch, u, i, r, flag, rank=5, implicitPrefs=implicit)
        assert calls == ([] if flag == "0" else [0, 1] * 3)
        assert U.dtype == np.float64 and U.shape == ref[0].shape and U.flags.c_contiguous
        err[flag] = float(max(np.abs(U - ref[0]).max(), np.abs(V - ref[1]).max()))
    print(f"implicit={implicit}: dense body error {err['0']:.3e}, sparse kernel error {err[None]:.3e}")
    assert err[None] <= 4 * err["0"] + 1e-13


@pytest.mark.parametrize("case", ["rank65", "lam0", "negative"])
def test_fit_declined(monkeypatch, case):
    u, i, r = _ratings(case == "negative")
    params = {"rank65": dict(rank=65), "lam0": dict(rank=2, regParam=0.0),
              "negative": dict(rank=5, implicitPrefs=True)}[case]
    if case == "negative":
        r[3] = -1.0
    assert not AO.supported("cuda", params["rank"], params.get("regParam", 0.1), u, i, r, case == "negative")
    monkeypatch.setattr(AO, "half_sweep", pytest.fail)
    monkeypatch.delenv("SML_ALS", raising=False)
    m = ALS(maxIter=3, **params).fit(DataFrame({"user": u.astype(np.float64), "item": i.astype(np.float64),
                                                 "rating": r}))
    U, V, _ = _fit(monkeypatch, u, i, r, "0", **params)
    assert np.allclose(np.asarray(m.getUserFactors()), U, rtol=1e-9, atol=1e-12)
    assert np.allclose(np.asarray(m.getItemFactors()), V, rtol=1e-9, atol=1e-12)
