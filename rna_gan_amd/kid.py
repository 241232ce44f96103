"""Kernel distance (KID, Binkowski et al. 2018, "Demystifying MMD GANs") between two sets of feature vectors, evaluated on
the device.

The value is the UNBIASED estimator of MMD^2 under the polynomial kernel k(a, b) = (gamma <a, b> + coef0)^degree, by default
gamma = 1 / F, coef0 = 1, degree = 3:

    mmd2 = (S_xx - D_x) / (m (m - 1)) + (S_yy - D_y) / (n (n - 1)) - 2 S_xy / (m n)

with S_xx = sum_{i, j} k(x_i, x_j), D_x = sum_i k(x_i, x_i) and so on.  Unlike the Frechet distance it is unbiased at any
sample size, needs no covariance and no matrix square root; its whole cost is the three Gram sums, which
rg_polykernel_tile_sums computes in fp64 next to the features (sums of cubes that nearly cancel: fp32 would not do).  Per
evaluation the host receives one small buffer of per-tile sums (one double per 64 x 64 tile of row pairs) and adds them.

The reference (src/fid.py) has no kernel distance; the estimator is pinned against an fp64 numpy restatement under tests/.
"""
from __future__ import annotations

import math

import numpy as np
import torch

TILE = 64           # rows per tile of rg_polykernel_tile_sums


def _tiles(n):
    return (int(n) + TILE - 1) // TILE


def _rows(x, what, dtype=torch.float32, no_columns=ValueError):
    """(tensor, row stride) of an (n, F) device tensor of ``dtype`` (float32 or float64) as the row kernels take it: unit column
    stride, row stride >= F; any other form is copied once (a row slice or a column slice of a wider tensor is NOT copied).
    no_columns: the exception class for F = 0."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dtype and x.dim() == 2):
        raise TypeError("%s must be an (n, F) %s tensor on the GPU" % (what, str(dtype).replace("torch.", "")))
    if x.shape[1] < 1:
        raise no_columns("%s has no feature columns" % what)
    F = x.shape[1]
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < F):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else F)


def _row_pair(a, b, names=("a", "b"), dtype=torch.float32, no_columns=ValueError):
    """``_rows`` of two sets that must agree in F and lie on one device: (a, lda, b, ldb)"""
    a, lda = _rows(a, names[0], dtype, no_columns)
    b, ldb = _rows(b, names[1], dtype, no_columns)
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError("%s is %s on %s, %s is %s on %s" % (names[0], tuple(a.shape), a.device, names[1], tuple(b.shape), b.device))
    return a, lda, b, ldb


def _kernel_args(F, gamma, coef0, degree):
    gamma = 1.0 / F if gamma is None else float(gamma)
    coef0, degree = float(coef0), int(degree)
    if not (math.isfinite(gamma) and gamma > 0.0 and math.isfinite(coef0)):
        raise ValueError("the polynomial kernel needs a finite gamma > 0 and a finite coef0")
    if degree not in (1, 2, 3):
        raise ValueError("degree must be 1, 2 or 3")
    return gamma, coef0, degree


def _launch(a, lda, b, ldb, gamma, coef0, degree, sums, diag):
    """one rg_polykernel_tile_sums launch on the current stream; sums / diag: contiguous fp64 views that receive the result"""
    from . import _abi
    _abi.launch("rg_polykernel_tile_sums", a.device, a.data_ptr(), lda, a.shape[0], None if b is None else b.data_ptr(), ldb,
                0 if b is None else b.shape[0], a.shape[1], gamma, coef0, degree, sums.data_ptr(),
                None if diag is None else diag.data_ptr())


def polykernel_tile_sums(a, b=None, gamma=None, coef0=1.0, degree=3):
    """Per-tile sums of k(a_r, b_s) = (gamma <a_r, b_s> + coef0)^degree, fp64 on the device: ``(sums, diag)``.
    sums is (ceil(na / 64), ceil(nb / 64)); b=None is the symmetric form (b = a, each tile pair computed once) and diag
    (ceil(na / 64),) then holds the per-tile sums of k(a_r, a_r); with b given diag is None.  gamma=None: 1 / F.
    Rows are read where they lie (a row or column slice of a wider tensor is not copied)."""
    if b is None:
        a, lda = _rows(a, "a")
        ldb, Tb = lda, _tiles(a.shape[0])
    else:
        a, lda, b, ldb = _row_pair(a, b)
        Tb = _tiles(b.shape[0])
    kargs = _kernel_args(a.shape[1], gamma, coef0, degree)
    sums = torch.zeros(_tiles(a.shape[0]), Tb, dtype=torch.float64, device=a.device)
    diag = torch.zeros(Tb, dtype=torch.float64, device=a.device) if b is None else None
    _launch(a, lda, b, ldb, *kargs, sums, diag)
    return sums, diag


def mmd2_from_sums(sxx, dx, syy, dy, sxy, m, n):
    """the unbiased estimate from the five totals (host, fp64)"""
    if m < 2 or n < 2:
        raise ValueError("the unbiased MMD^2 needs at least 2 rows in each set, got %d and %d" % (m, n))
    return (sxx - dx) / (m * (m - 1.0)) + (syy - dy) / (n * (n - 1.0)) - 2.0 * sxy / (m * float(n))


def _pair_layout(m, n):
    """offsets of (S_xx tiles, D_x tiles, S_yy tiles, D_y tiles, S_xy tiles) of one (x, y) pair in a flat fp64 buffer"""
    tx, ty = _tiles(m), _tiles(n)
    sizes = (tx * tx, tx, ty * ty, ty, tx * ty)
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs


def _pair_launches(x, ldx, y, ldy, kargs, buf, at):
    """the three launches of one (x, y) pair, results into buf[at : at + size]; returns the size used"""
    offs = _pair_layout(x.shape[0], y.shape[0])
    part = [buf[at + offs[i]:at + offs[i + 1]] for i in range(5)]
    _launch(x, ldx, None, ldx, *kargs, part[0], part[1])
    _launch(y, ldy, None, ldy, *kargs, part[2], part[3])
    _launch(x, ldx, y, ldy, *kargs, part[4], None)
    return offs[-1]


def _pair_value(host, at, m, n):
    """the estimate of one pair from the downloaded buffer: each total is the exactly rounded sum (math.fsum) of its tile sums,
    so the value does not depend on an order"""
    offs = _pair_layout(m, n)
    tot = [math.fsum(host[at + offs[i]:at + offs[i + 1]]) for i in range(5)]
    return mmd2_from_sums(*tot, m, n)


def _check_pair(x, y):
    x, ldx, y, ldy = _row_pair(x, y, ("x", "y"))
    if x.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError("the unbiased MMD^2 needs at least 2 rows in each set, got %d and %d" % (x.shape[0], y.shape[0]))
    return x, ldx, y, ldy


def mmd2_unbiased(x, y, gamma=None, coef0=1.0, degree=3):
    """Unbiased MMD^2 between the (m, F) and (n, F) fp32 device feature sets x and y: three launches, one download of the tile
    sums, the totals added on the host in fp64.  m, n >= 2."""
    x, ldx, y, ldy = _check_pair(x, y)
    kargs = _kernel_args(x.shape[1], gamma, coef0, degree)
    buf = torch.empty(_pair_layout(x.shape[0], y.shape[0])[-1], dtype=torch.float64, device=x.device)      # written in full
    _pair_launches(x, ldx, y, ldy, kargs, buf, 0)
    return _pair_value(buf.cpu().numpy(), 0, x.shape[0], y.shape[0])


def subset_indices(m, n, num_subsets, subset_size, seed):
    """the row subsets of kernel_distance: for each subset, ``size`` rows of x and of y drawn WITHOUT replacement from a private
    torch.Generator(seed) (x's permutation first); size = min(subset_size, m, n).  The global generators are not touched."""
    size = min(int(subset_size), int(m), int(n))
    g = torch.Generator().manual_seed(int(seed))
    return [(torch.randperm(m, generator=g)[:size], torch.randperm(n, generator=g)[:size]) for _ in range(int(num_subsets))]


def kernel_distance(x, y, num_subsets=0, subset_size=1000, seed=0, gamma=None, coef0=1.0, degree=3):
    """{"mmd2": the full-set unbiased estimate, "subset_mean", "subset_std"} of the feature sets x (m, F) and y (n, F).
    num_subsets > 0 adds the published KID convention (100 subsets of 1000 rows): the estimate on row subsets drawn without
    replacement (subset_indices; subset_size is clamped to min(m, n)), their mean and their standard deviation (np.std, the
    population form).  The subsets' rows are gathered on the device and go through the same launches; every tile sum of the call
    lands in one buffer and comes back in one download.  num_subsets == 0: subset_mean and subset_std are None."""
    x, ldx, y, ldy = _check_pair(x, y)
    num_subsets, subset_size = int(num_subsets), int(subset_size)
    if num_subsets < 0:
        raise ValueError("num_subsets must be >= 0")
    if num_subsets and subset_size < 2:
        raise ValueError("subset_size must be >= 2")
    m, n, F = x.shape[0], y.shape[0], x.shape[1]
    kargs = _kernel_args(F, gamma, coef0, degree)
    subsets = subset_indices(m, n, num_subsets, subset_size, seed)
    size = min(subset_size, m, n)
    full, each = _pair_layout(m, n)[-1], _pair_layout(size, size)[-1]
    buf = torch.empty(full + num_subsets * each, dtype=torch.float64, device=x.device)                     # written in full
    _pair_launches(x, ldx, y, ldy, kargs, buf, 0)
    for s, (ix, iy) in enumerate(subsets):
        xs = x.index_select(0, ix.to(x.device))
        ys = y.index_select(0, iy.to(y.device))
        _pair_launches(xs, F, ys, F, kargs, buf, full + s * each)
    host = buf.cpu().numpy()
    out = {"mmd2": _pair_value(host, 0, m, n), "subset_mean": None, "subset_std": None}
    if num_subsets:
        values = [_pair_value(host, full + s * each, size, size) for s in range(num_subsets)]
        out["subset_mean"], out["subset_std"] = float(np.mean(values)), float(np.std(values))
        out["subset_values"] = values
    return out


def calculate_kid(images1, images2, feature_extractor, batch_size=2, device=None, **kwargs):
    """Counterpart of fid.calculate_fid(on_device=True): images (N, H, W, 3) uint8 / float in [0, 1] are uploaded once, resized
    to 299 and extracted on the device (``feature_extractor`` returns device tensors, e.g. fid.inception_features_device);
    returns kernel_distance(features1, features2, **kwargs)."""
    from .fid import device_feature_pair
    return kernel_distance(*device_feature_pair(images1, images2, feature_extractor, batch_size, device), **kwargs)
