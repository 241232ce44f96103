"""fp64 numpy restatements of the kernel distance (rg_polykernel_tile_sums, rna_gan_amd.kid), for tests/test_kid_ops_gpu.py
and tests/test_kid_metric_gpu.py.  Nothing here comes from rna_gan_amd; tests/test_kid_refs_cpu.py pins these functions
against sklearn's polynomial_kernel, a plain double loop and exact rational arithmetic without a GPU.

The kernel's arithmetic contract, restated operation by operation:
  every operand converted to fp64;
  dot = sum_k a[k] * b[k] summed sequentially in ascending k (the product of two fp32 values is exact in fp64, so the
        kernel's fma and this multiply-then-add round identically);
  t = gamma * dot + coef0 as two separately rounded operations;
  v = t (degree 1), t * t (2), (t * t) * t (3).
So ``kernel_values`` returns the kernel's terms bit for bit; only the order in which a tile's up to 4096 terms are added is
the kernel's own, and ``tile_sums_ref`` adds them with math.fsum (the exactly rounded sum, an order of nobody)."""
import math

import numpy as np

TILE = 64
U = 2.0 ** -53


def kernel_values(a, b, gamma, coef0, degree):
    """(na, nb) fp64 matrix of k(a_r, b_s), with the kernel's roundings"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1] and degree in (1, 2, 3)
    dot = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    for k in range(a.shape[1]):                       # sequential in k, vectorised over the pairs
        dot = dot + a[:, k, None] * b[None, :, k]
    t = np.float64(gamma) * dot
    t = t + np.float64(coef0)
    if degree == 1:
        return t
    t2 = t * t
    return t2 if degree == 2 else t2 * t


def _tiles(n):
    return (n + TILE - 1) // TILE


def _tile_reduce(v, fn):
    out = np.zeros((_tiles(v.shape[0]), _tiles(v.shape[1])), dtype=np.float64)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            out[i, j] = fn(v[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE].ravel())
    return out


def tile_sums_ref(a, b, gamma, coef0, degree):
    """(sums, diag): sums[ti][tj] = fsum of k(a_r, b_s) over the 64 x 64 tile of row pairs; b=None: b = a and diag[ti] = fsum
    of k(a_r, a_r) over tile ti's rows (diag is None with two operands)"""
    v = kernel_values(a, a if b is None else b, gamma, coef0, degree)
    sums = _tile_reduce(v, math.fsum)
    if b is not None:
        return sums, None
    d = np.diagonal(v)
    return sums, np.array([math.fsum(d[i * TILE:(i + 1) * TILE]) for i in range(_tiles(len(d)))], dtype=np.float64)


def tile_abs_sums_ref(a, b, gamma, coef0, degree):
    """(abs_sums, abs_diag): the same sums of |k|, the scale of the summation-order bound used on the GPU"""
    v = np.abs(kernel_values(a, a if b is None else b, gamma, coef0, degree))
    sums = _tile_reduce(v, math.fsum)
    if b is not None:
        return sums, None
    d = np.diagonal(v)
    return sums, np.array([math.fsum(d[i * TILE:(i + 1) * TILE]) for i in range(_tiles(len(d)))], dtype=np.float64)


def mmd2_from_totals(sxx, dx, syy, dy, sxy, m, n):
    return (sxx - dx) / (m * (m - 1.0)) + (syy - dy) / (n * (n - 1.0)) - 2.0 * sxy / (m * float(n))


def mmd2_unbiased_ref(x, y, gamma=None, coef0=1.0, degree=3):
    """the unbiased MMD^2 of the (m, F) and (n, F) feature sets: every total the fsum of the restated kernel values"""
    x, y = np.asarray(x), np.asarray(y)
    m, n = x.shape[0], y.shape[0]
    if m < 2 or n < 2:
        raise ValueError("the unbiased MMD^2 needs at least 2 rows in each set")
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    kxx, kyy, kxy = (kernel_values(p, q, gamma, coef0, degree) for p, q in ((x, x), (y, y), (x, y)))
    return mmd2_from_totals(math.fsum(kxx.ravel()), math.fsum(np.diagonal(kxx)), math.fsum(kyy.ravel()),
                            math.fsum(np.diagonal(kyy)), math.fsum(kxy.ravel()), m, n)


def mmd2_matrix_form(x, y, gamma=None, coef0=1.0, degree=3):
    """the same estimator from fp64 BLAS Gram matrices (not the kernel's roundings): the host baseline of a measurement and an
    independent check of the estimator's formula"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m, n = x.shape[0], y.shape[0]
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    kxx, kyy, kxy = ((gamma * (p @ q.T) + coef0) ** degree for p, q in ((x, x), (y, y), (x, y)))
    return mmd2_from_totals(kxx.sum(), np.trace(kxx), kyy.sum(), np.trace(kyy), kxy.sum(), m, n)


def mmd2_abs_scale(x, y, gamma=None, coef0=1.0, degree=3):
    """(A_xx, A_yy, A_xy): sums of |k| over the three Gram matrices -- the scales the summation-order bound multiplies"""
    x, y = np.asarray(x), np.asarray(y)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    return tuple(math.fsum(np.abs(kernel_values(p, q, gamma, coef0, degree)).ravel()) for p, q in ((x, x), (y, y), (x, y)))


def integer_case(na, nb, F, seed):
    """integer features in [-3, 3] as fp32: with gamma = 1 / 64 at F = 64 or gamma = 1 at F = 70 every value and every sum of
    the contract is exact in fp64 (tests/test_kid_refs_cpu.py proves it with fractions.Fraction)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, size=(na, F)).astype(np.float32)
    b = rng.integers(-3, 4, size=(nb, F)).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b
