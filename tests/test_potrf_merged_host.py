"""The in-register 16x16 potrf + inverse of the fp32 solve kernels, emulated step by step on the host.

The kernels used to carry a second tile E (identity at the start, the same row operations as the tile being
eliminated) and read row J of W = L^-1 from it.  They now read it from the eliminated columns of the tile
itself:  W[r][col] = c[r][col] * (-1/d_col) / sqrt(d_r)  below the diagonal,  1/sqrt(d_r)  on it.  Both
recursions are written out here exactly as the device code orders them, and compared
  - in float64, where they must agree to 1e-12 (the identity is algebra, not luck), and
  - in float32, where both must stay within the same distance of the float64 inverse: twice the worst
    error of the form with E on these very matrices.
"""
import numpy as np
import pytest


def _fma(a, b, c, dt):
    # a * b + c rounded once (float32: product and sum are taken in float64, whose 53 bits hold the product exactly)
    if dt == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def potrf_inv_with_e(A, dt):
    """The earlier device recursion: tile c and identity-started tile e."""
    c = A.astype(dt).copy()
    e = np.eye(16, dtype=dt)
    W = np.zeros((16, 16), dtype=dt)
    one = dt(1)
    for J in range(16):
        ej = e[J].copy()
        inv = one / np.sqrt(c[J, J])
        nrd = -inv * inv
        if J < 15:
            m = c[J] * nrd
            m[J] = 0
            c = _fma(c[:, J:J + 1].copy(), m[None, :], c, dt)
        W[J] = ej * inv
        if J < 15:
            e = _fma(c[:, J:J + 1], (ej * nrd)[None, :], e, dt)
    return W


def potrf_inv_merged(A, dt, steps=16):
    """The device recursion: no e; row J of W from row J of c, the column scale in a tail."""
    c = A.astype(dt).copy()
    W = np.zeros((16, 16), dtype=dt)
    icol = np.ones(16, dtype=dt)
    one = dt(1)
    for J in range(steps):
        rowj = c[J].copy()
        inv = one / np.sqrt(c[J, J])
        if J < 15:
            nrd = -inv * inv
            m = rowj * nrd
            m[J] = 0
            c = _fma(c[:, J:J + 1].copy(), m[None, :], c, dt)
        W[J] = rowj * inv
        icol[J] = inv
    ncol = -icol * icol
    r, k = np.indices((16, 16))
    low = (k < r) & (r < steps)
    return np.where(low, W * ncol[None, :], np.where(r == k, icol[None, :], dt(0))).astype(dt)


def _matrices():
    rng = np.random.default_rng(20250)
    mats = []
    for i in range(300):
        B = rng.uniform(-0.5, 0.5, (16, 16))
        A = B @ B.T + np.eye(16)
        if i % 2:
            A += np.diag(10.0 ** rng.uniform(-3, 8, 16))                    # interior-point Sigma on every row
        elif i % 4 == 2:
            A += np.diag(np.where(rng.random(16) < 0.4, 10.0 ** rng.uniform(-3, 8, 16), 0.0))   # ... on a subset of rows
        mats.append(A)
    return mats


def _padded():
    rng = np.random.default_rng(7)
    B = rng.uniform(-0.5, 0.5, (8, 8))
    A = np.eye(16)
    A[:8, :8] = B @ B.T + np.eye(8) + np.diag(10.0 ** rng.uniform(-3, 8, 8))
    return A


def _w64(A):
    return np.linalg.inv(np.linalg.cholesky(A.astype(np.float64)))


def _rel(W, Wref):
    return np.abs(W.astype(np.float64) - Wref).max() / np.abs(Wref).max()


def test_float64_the_two_recursions_agree():
    worst = 0.0
    for A in _matrices() + [_padded()]:
        We = potrf_inv_with_e(A, np.float64)
        Wm = potrf_inv_merged(A, np.float64)
        worst = max(worst, _rel(Wm, We))
        assert np.all(np.triu(Wm, 1) == 0.0)
    print(f"float64: worst max|W_merged - W_e| / max|W_e| = {worst:.2e}")
    assert worst <= 1e-12
    # the eight-pivot form of the padded tile: rows 8..15 are rows of the identity
    A = _padded()
    Wh = potrf_inv_merged(A, np.float64, steps=8)
    assert _rel(Wh, potrf_inv_with_e(A, np.float64)) <= 1e-12
    assert np.array_equal(Wh[8:], np.eye(16)[8:])


def test_float32_both_within_the_same_bound_of_the_float64_inverse():
    mats = _matrices() + [_padded()]
    err_e = [_rel(potrf_inv_with_e(A.astype(np.float32), np.float32), _w64(A.astype(np.float32))) for A in mats]
    err_m = [_rel(potrf_inv_merged(A.astype(np.float32), np.float32), _w64(A.astype(np.float32))) for A in mats]
    bound = 2.0 * max(err_e)
    print(f"float32: worst error with e {max(err_e):.2e}, merged {max(err_m):.2e}, bound {bound:.2e}")
    assert max(err_e) <= bound and max(err_m) <= bound
    Ah = _padded().astype(np.float32)
    assert _rel(potrf_inv_merged(Ah, np.float32, steps=8), _w64(Ah)) <= bound


@pytest.mark.parametrize("bad", ["negative", "zero"])
def test_a_bad_pivot_reaches_the_last_diagonal_entry(bad):
    rng = np.random.default_rng(3)
    B = rng.uniform(-0.5, 0.5, (16, 16))
    A = (B @ B.T + np.eye(16)).astype(np.float32)
    if bad == "negative":
        A[3, 3] = -5.0
    else:
        A[0, :] = 0
        A[:, 0] = 0
    with np.errstate(all="ignore"):
        W = potrf_inv_merged(A, np.float32)
    assert not np.isfinite(W[15, 15])
