"""Numpy restatements of the two kernels of rna_gan_amd/csrc/rg_fidstat.hip (include/rnagan_hip.h: rg_resize_bilinear01,
rg_moments_update), for tests/test_fid_device_ops_gpu.py and tests/test_metrics_gpu.py.  Nothing here comes from rna_gan_amd;
tests/test_fid_device_refs_cpu.py pins both without a GPU.

Resize: taps in fp32 exactly as the header states them, source coordinates in fp64, the weight lambda rounded to fp32, the
four-tap value in fp64 (the kernel evaluates it in fp32: eight roundings of values <= 1, each <= 2^-25, times 2 for
contraction differences = RESIZE_BOUND).  Moments: exact integer sums where the data are integers, np.longdouble otherwise.
"""
import numpy as np

RESIZE_BOUND = 8 * 2.0 ** -24


def tap_u8(v):
    """uint8 -> fp32 tap: (float)v / 255.0f, one fp32 division"""
    return np.asarray(v, dtype=np.uint8).astype(np.float32) / np.float32(255.0)


def tap_f32(v, mul, add):
    """fp32 -> fp32 tap: v * mul + add, two fp32 operations"""
    v = np.asarray(v, dtype=np.float32)
    return (v * np.float32(mul)).astype(np.float32) + np.float32(add)


def axis_taps(n_in, n_out):
    """(i0, i1, lambda as fp32) of every output index of one axis, coordinates in fp64"""
    d = np.arange(n_out, dtype=np.float64)
    s = np.maximum(0.0, (d + 0.5) * float(n_in) / float(n_out) - 0.5)
    i0 = np.minimum(np.floor(s), n_in - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (s - i0).astype(np.float32)
    return i0, i1, lam


def resize_ref(taps, Ho, Wo):
    """taps (N, C, H, W) fp32 -> (N, C, Ho, Wo) fp64, clamped into [0, 1]"""
    taps = np.asarray(taps)
    assert taps.dtype == np.float32 and taps.ndim == 4
    t = taps.astype(np.float64)
    y0, y1, ly = axis_taps(t.shape[2], Ho)
    x0, x1, lx = axis_taps(t.shape[3], Wo)
    ly = ly.astype(np.float64)[None, None, :, None]
    lx = lx.astype(np.float64)[None, None, None, :]
    top = (1.0 - lx) * t[:, :, y0][:, :, :, x0] + lx * t[:, :, y0][:, :, :, x1]
    bot = (1.0 - lx) * t[:, :, y1][:, :, :, x0] + lx * t[:, :, y1][:, :, :, x1]
    return np.clip((1.0 - ly) * top + ly * bot, 0.0, 1.0)


def moments_int(x):
    """exact (s1, s2) of integer-valued rows, as Python-exact int64 sums (|x| <= 2047: 259 rows stay far below 2^63)"""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi.astype(np.float32), np.asarray(x, dtype=np.float32))
    return xi.sum(axis=0), xi.T @ xi


def moments_ld(x):
    """(s1, s2, |X|^T |X|, sum |x|) of fp32 rows in np.longdouble (products of fp32 values are exact there)"""
    xl = np.asarray(x, dtype=np.float32).astype(np.longdouble)
    al = np.abs(xl)
    return xl.sum(axis=0), xl.T @ xl, al.T @ al, al.sum(axis=0)
