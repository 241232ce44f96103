"""Macenko stain normalisation (Macenko et al., ISBI 2009) of uint8 H&E tiles where they already are -- on the device.

Tiles from different scanning sites differ in the colour of haematoxylin and eosin.  The method estimates the two stain vectors of a
set of tiles from the optical density of its stained pixels (the plane of the two leading eigenvectors, the ALPHA-th and
(100 - ALPHA)-th percentile of the angle in it), the 99th percentile of each stain's concentration, and re-renders every pixel with
a target's stain vectors and concentrations.

The textbook form uses log, atan2, exp and float percentiles.  Here it is restated on fixed-point tables built on the host in fp64
(``od_table``, ``direction_table``, ``output_table``), so that everything the device computes is an INTEGER: the contract is stated
in include/rnagan_hip.h, restated in tests/stain_refs.py, and the kernels (rna_gan_amd/csrc/rg_stain.hip) are tested bit for bit.
tests/test_stain_refs_cpu.py measures the agreement with the fp64 textbook form; no parity with staintools, torchstain or
histomicstk is claimed (none was installed where this was written).

``fit`` is three launches with one small download after each (10 int64; K + 1 and 2 x CB uint64) and the host arithmetic between
them (eigh of a 3 x 3 covariance, two percentiles, a pseudo-inverse); ``normalize`` is one launch.  On a CPU tensor both compute the
same integers with numpy; on a CUDA tensor there is no fallback: the kernels run or the call raises.

Out of scope: per-slide normalisation inside DeviceTileSet.from_dataset or Trainer; the Vahadane and Reinhard methods; stain
augmentation.
"""
from __future__ import annotations

import ctypes
import json
import math

import numpy as np
import torch

from . import _abi
from .export import export_flags, rgb_numpy, tile_args

IO = 240
BETA = 0.15
ALPHA = 1
QOD = 12
QV = 14
K = 1024
QP = 20
CB, CSH = 4096, 3
QS, QH, QO = 16, 14, 8
CONC_PERCENTILE = 99
MIN_STAINED = 16
STAT_CHUNK = 32768          # pixels per workgroup of the three statistics kernels (SN_CHUNK of rg_stain.hip)
APPLY_CHUNK = 8192          # pixels per workgroup of rg_stain_apply (SN_APPLY_CHUNK)
MAX_PIXELS = 1 << 33        # per call


class StainFitError(ValueError):
    """A set that cannot be fitted: fewer than 16 stained pixels, a non-finite or rank-deficient covariance, or a 99th-percentile
    concentration that is not above zero.  ``counts`` holds n_pixels, n_stained and n_outside as far as they were known."""

    def __init__(self, message, **counts):
        super().__init__("%s (%s)" % (message, ", ".join("%s %d" % kv for kv in sorted(counts.items()))))
        self.counts = counts


class StainFit:
    """``he``: (3, 2) float64, the stain vectors as columns (haematoxylin, eosin), rows R, G, B; ``max_conc``: (2,) float64, the
    99th-percentile concentrations; ``n_pixels``, ``n_stained`` (all three optical densities >= BETA), ``n_outside`` (stained
    pixels with a non-positive projection on the leading eigenvector, left out of the angle histogram)."""

    def __init__(self, he, max_conc, n_pixels=0, n_stained=0, n_outside=0):
        self.he = np.array(he, dtype=np.float64).reshape(3, 2)
        self.max_conc = np.array(max_conc, dtype=np.float64).reshape(2)
        self.n_pixels, self.n_stained, self.n_outside = int(n_pixels), int(n_stained), int(n_outside)

    def to_json(self):
        return json.dumps({"he": self.he.tolist(), "max_conc": self.max_conc.tolist(), "n_pixels": self.n_pixels,
                           "n_stained": self.n_stained, "n_outside": self.n_outside})

    @classmethod
    def from_json(cls, text):
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        d = d.get("fit", d) if "he" not in d else d                       # a stain.json written by tile_slides.py holds the fit
        return cls(d["he"], d["max_conc"], d.get("n_pixels", 0), d.get("n_stained", 0), d.get("n_outside", 0))

    def __eq__(self, other):
        return (isinstance(other, StainFit) and np.array_equal(self.he, other.he) and np.array_equal(self.max_conc, other.max_conc)
                and (self.n_pixels, self.n_stained, self.n_outside) == (other.n_pixels, other.n_stained, other.n_outside))

    def __repr__(self):
        return "StainFit(he=%s, max_conc=%s, n_pixels=%d, n_stained=%d, n_outside=%d)" % (
            self.he.tolist(), self.max_conc.tolist(), self.n_pixels, self.n_stained, self.n_outside)


# the commonly published Macenko target (the constants of the method's reference implementation)
REFERENCE_TARGET = StainFit([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], [1.9705, 1.0308])


# ------------------------------------------------------------------ host tables (fp64, rint)
def od_table():
    """int32 [256]: rint(-ln((v + 1) / IO) 2^QOD); negative for v >= IO, not clamped"""
    v = np.arange(256, dtype=np.float64)
    return np.rint(-np.log((v + 1.0) / IO) * (1 << QOD)).astype(np.int32)


def beta_q():
    return int(np.rint(BETA * (1 << QOD)))


def direction_table(k=K):
    """int32 [k - 1][2]: (cos, sin) of theta_j = -pi/2 + j pi / k, j = 1 .. k - 1, in QV bits"""
    th = -np.pi / 2 + np.arange(1, k, dtype=np.float64) * np.pi / k
    return np.stack([np.rint(np.cos(th) * (1 << QV)), np.rint(np.sin(th) * (1 << QV))], axis=1).astype(np.int32)


def _out_value(d):
    return np.clip(np.rint(IO * np.exp(-np.asarray(d, dtype=np.float64) / (1 << QO))), 0, 255)


def output_table():
    """(uint8 [L], OFF): out_lut[j] = clip(rint(IO exp(-(j - OFF) / 2^QO)), 0, 255); OFF the smallest offset at which index 0 gives
    255, L the smallest length whose last entry is 0"""
    off = 0
    while _out_value(-off) < 255:
        off += 1
    last = 0
    while _out_value(last) > 0:
        last += 1
    return _out_value(np.arange(-off, last + 1)).astype(np.uint8), off


def histogram_percentile(hist, q):
    """The percentile rule of the contract: the first bin whose cumulative count exceeds (q (total - 1)) // 100.  q: an integer."""
    if int(q) != q or not 0 <= q <= 100:
        raise ValueError("a percentile is an integer in 0..100")
    total = sum(int(v) for v in hist)
    if total < 1:
        raise ValueError("the histogram is empty")
    rank = (int(q) * (total - 1)) // 100
    cum = 0
    for b, v in enumerate(hist):
        cum += int(v)
        if cum > rank:
            return b
    raise AssertionError("unreachable")


def angle_of_bin(b, k=K):
    return -math.pi / 2 + (b + 0.5) * math.pi / k


def conc_of_bin(b):
    return (b + 0.5) * (1 << CSH) / (1 << QOD)


# ------------------------------------------------------------------ the host arithmetic between the passes
def basis_from_moments(m, n_pixels=0):
    """10 integers (count, S1[3], S2 for RR RG RB GG GB BB) -> (e1, e2) float64, the two leading eigenvectors of the covariance."""
    m = [int(v) for v in m]
    n = m[0]
    if n < MIN_STAINED:
        raise StainFitError("fewer than %d stained pixels" % MIN_STAINED, n_pixels=n_pixels, n_stained=n)
    s1 = m[1:4]
    s2 = {(0, 0): m[4], (0, 1): m[5], (0, 2): m[6], (1, 1): m[7], (1, 2): m[8], (2, 2): m[9]}
    cov = np.empty((3, 3), dtype=np.float64)
    den = float(n * (n - 1))
    for c in range(3):
        for d in range(c, 3):
            cov[c, d] = cov[d, c] = float(n * s2[(c, d)] - s1[c] * s1[d]) / den / float(1 << (2 * QOD))       # exact integers above
    if not np.isfinite(cov).all():
        raise StainFitError("the covariance is not finite", n_pixels=n_pixels, n_stained=n)
    w, v = np.linalg.eigh(cov)
    if not np.isfinite(w).all() or not w[2] > 0 or not w[1] > 1e-12 * w[2]:
        raise StainFitError("the covariance is rank-deficient", n_pixels=n_pixels, n_stained=n)
    e1, e2 = v[:, 2].copy(), v[:, 1].copy()
    if e1.sum() < 0:
        e1 = -e1
    if e2.sum() < 0:
        e2 = -e2
    return e1, e2


def quantize_basis(e1, e2):
    return [int(x) for x in np.rint(np.concatenate([e1, e2]) * (1 << QV))]


def he_from_angles(e1, e2, hist, n_pixels=0, n_stained=0):
    """the K + 1 counts of pass 2 -> HE (3, 2)"""
    k = len(hist) - 1
    outside = int(hist[k])
    if sum(int(v) for v in hist[:k]) < 1:
        raise StainFitError("no stained pixel has a positive projection on the leading eigenvector", n_pixels=n_pixels,
                            n_stained=n_stained, n_outside=outside)
    cols = []
    for q in (ALPHA, 100 - ALPHA):
        phi = angle_of_bin(histogram_percentile(hist[:k], q), k)
        cols.append(e1 * math.cos(phi) + e2 * math.sin(phi))
    if cols[0][0] < cols[1][0]:
        cols.reverse()
    return np.stack(cols, axis=1)


def quantize_pinv(he):
    """Pq[stain][channel] = rint(pinv(HE) 2^QP) as six Python ints"""
    p = np.linalg.pinv(np.asarray(he, dtype=np.float64))
    if not np.isfinite(p).all():
        raise StainFitError("the stain matrix has no finite pseudo-inverse")
    return [int(x) for x in np.rint(p * (1 << QP)).reshape(-1)]


def max_conc_from_hist(hist, n_pixels=0, n_stained=0, n_outside=0):
    out = []
    for s in range(2):
        b = histogram_percentile(hist[s], CONC_PERCENTILE)
        if b == 0:
            raise StainFitError("the 99th-percentile concentration of stain %d is zero" % s, n_pixels=n_pixels, n_stained=n_stained,
                                n_outside=n_outside)
        out.append(conc_of_bin(b))
    return np.array(out, dtype=np.float64)


def apply_operands(fit, target):
    """(pinv6, scale2, href6): the host integers of rg_stain_apply"""
    if not (np.isfinite(fit.max_conc).all() and (fit.max_conc > 0).all()):
        raise StainFitError("the fit's max_conc is not positive")
    pinv6 = quantize_pinv(fit.he)
    scale2 = [int(x) for x in np.rint(target.max_conc / fit.max_conc * (1 << QS))]
    href6 = [int(x) for x in np.rint(target.he * (1 << QH)).reshape(-1)]
    return pinv6, scale2, href6


# ------------------------------------------------------------------ the numpy path (CPU tensors): the same integers
def _od_numpy(rgb):
    return od_table().astype(np.int64)[rgb.reshape(-1, 3)]


def _angle_bins_numpy(p1, p2, dirs):
    """binary search of the contract's count, vectorised: p1 > 0"""
    k = dirs.shape[0] + 1
    c = np.concatenate([[0], dirs[:, 0]]).astype(np.int64)
    s = np.concatenate([[0], dirs[:, 1]]).astype(np.int64)
    lo = np.zeros(p1.shape, dtype=np.int64)
    hi = np.full(p1.shape, k - 1, dtype=np.int64)
    while True:
        open_ = lo < hi
        if not open_.any():
            return lo
        mid = (lo + hi + 1) >> 1
        on = c[mid] * p2 - s[mid] * p1 >= 0
        lo = np.where(open_ & on, mid, lo)
        hi = np.where(open_ & ~on, mid - 1, hi)


def _moments_numpy(rgb):
    od = _od_numpy(rgb)
    od = od[(od >= beta_q()).all(axis=1)]
    out = [od.shape[0]] + [int(od[:, c].sum()) for c in range(3)]
    for c in range(3):
        for d in range(c, 3):
            out.append(int((od[:, c] * od[:, d]).sum()))
    return np.array(out, dtype=np.int64)


def _angle_hist_numpy(rgb, basis6, dirs):
    od = _od_numpy(rgb)
    od = od[(od >= beta_q()).all(axis=1)]
    b = np.array(basis6, dtype=np.int64)
    p1, p2 = od @ b[:3], od @ b[3:]
    k = dirs.shape[0] + 1
    hist = np.zeros(k + 1, dtype=np.int64)
    inside = p1 > 0
    hist[k] = int((~inside).sum())
    hist[:k] = np.bincount(_angle_bins_numpy(p1[inside], p2[inside], dirs), minlength=k).astype(np.int64)
    return hist


def _conc_numpy(od, pinv6):
    p = np.array(pinv6, dtype=np.int64).reshape(2, 3)
    return (od @ p.T) >> QP


def _conc_hist_numpy(rgb, pinv6):
    conc = _conc_numpy(_od_numpy(rgb), pinv6)
    bins = np.clip(conc >> CSH, 0, CB - 1)
    return np.stack([np.bincount(bins[:, s], minlength=CB) for s in range(2)]).astype(np.int64)


def _apply_numpy(rgb, pinv6, scale2, href6):
    table, off = output_table()
    shift = QH + QOD - QO
    conc2 = (_conc_numpy(_od_numpy(rgb), pinv6) * np.array(scale2, dtype=np.int64)) >> QS
    od2 = (conc2 @ np.array(href6, dtype=np.int64).reshape(3, 2).T + (1 << (shift - 1))) >> shift
    return table[np.clip(od2 + off, 0, len(table) - 1)].reshape(rgb.shape)


# ------------------------------------------------------------------ arguments and the device calls
def _tile_args(tiles, layout, order, what):
    N, H, W = tile_args(tiles, layout, order, what)
    if H < 1 or W < 1:
        raise ValueError("%s needs H, W >= 1" % what)
    return N, H, W


def _pieces(N, H, W, batch):
    """tile ranges of at most `batch` tiles and at most MAX_PIXELS pixels"""
    step = max(1, min(N if batch is None else int(batch), MAX_PIXELS // (H * W)))
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    return [(a, min(a + step, N)) for a in range(0, N, step)]


class _Device:
    """the tables of the contract on one device, and the three accumulators of a fit"""
    _cache = {}

    def __init__(self, dev):
        table, self.off = output_table()
        self.od = torch.from_numpy(od_table()).to(dev)
        self.dirs = torch.from_numpy(direction_table()).to(dev)
        self.out = torch.from_numpy(table).to(dev)
        self.L = int(table.shape[0])
        self.acc = torch.zeros(10 + (K + 1) + 2 * CB, dtype=torch.int64, device=dev)

    @classmethod
    def get(cls, dev):
        key = _abi.device_key(dev)
        if key not in cls._cache:
            cls._cache[key] = cls(dev)
        return cls._cache[key]


def _ll(values):
    return (ctypes.c_longlong * len(values))(*values)


def _ii(values):
    return (ctypes.c_int * len(values))(*values)


# ------------------------------------------------------------------ the public functions
def fit(tiles, layout="nhwc", order="rgb", batch=None):
    """uint8 tiles, (N, H, W, 3) ("nhwc") or (N, 3, H, W) ("nchw"), stored R, G, B ("rgb") or B, G, R ("bgr"), fitted TOGETHER as one
    set -> StainFit.  On a CUDA tensor: three launches on the current stream (rg_stain_moments, rg_stain_angle_hist,
    rg_stain_conc_hist) with one small download after each.  batch: feed the set through in pieces of that many tiles, each piece
    adding to the same integers (``accumulate``): the result does not depend on it."""
    N, H, W = _tile_args(tiles, layout, order, "stain.fit")
    n_pixels = N * H * W
    if N == 0:
        raise StainFitError("fewer than %d stained pixels" % MIN_STAINED, n_pixels=0, n_stained=0)
    pieces = _pieces(N, H, W, batch)
    cuda = tiles.device.type == "cuda"
    if cuda:
        src = tiles.contiguous()
        D = _Device.get(tiles.device)
        flags = export_flags(layout, order)
        mom, ang, con = D.acc[:10], D.acc[10:10 + K + 1], D.acc[10 + K + 1:]

        def run(name, *operands):
            """the pass `name` over the pieces: operands = what follows (tiles, N, H, W, flags, od_lut) up to the output"""
            for i, (a, b) in enumerate(pieces):
                _abi.launch(name, tiles.device, src[a:b].data_ptr(), b - a, H, W, flags, D.od.data_ptr(), *operands, int(i > 0))
    else:
        rgb = rgb_numpy(tiles, layout, order)

    # pass 1
    if cuda:
        run("rg_stain_moments", beta_q(), mom.data_ptr())
        m = mom.cpu().numpy()
    else:
        m = sum(_moments_numpy(rgb[a:b]) for a, b in pieces)
    n_stained = int(m[0])
    e1, e2 = basis_from_moments(m, n_pixels)
    basis6 = quantize_basis(e1, e2)
    # pass 2
    if cuda:
        run("rg_stain_angle_hist", beta_q(), _ii(basis6), D.dirs.data_ptr(), K, ang.data_ptr())
        hist = ang.cpu().numpy()
    else:
        dirs = direction_table()
        hist = sum(_angle_hist_numpy(rgb[a:b], basis6, dirs) for a, b in pieces)
    n_outside = int(hist[K])
    he = he_from_angles(e1, e2, hist, n_pixels, n_stained)
    pinv6 = quantize_pinv(he)
    # pass 3
    if cuda:
        run("rg_stain_conc_hist", _ll(pinv6), QP, CSH, CB, con.data_ptr())
        chist = con.cpu().numpy().reshape(2, CB)
    else:
        chist = sum(_conc_hist_numpy(rgb[a:b], pinv6) for a, b in pieces)
    max_conc = max_conc_from_hist(chist, n_pixels, n_stained, n_outside)
    return StainFit(he, max_conc, n_pixels, n_stained, n_outside)


def normalize(tiles, fit, target=REFERENCE_TARGET, out=None, layout="nhwc", order="rgb"):
    """Re-render `tiles` (fitted by `fit`) with the stain vectors and concentrations of `target` (a StainFit) -> uint8 tensor of the
    same shape, layout, channel order and device.  out: None (a new tensor), or a contiguous uint8 tensor of tiles' shape on its
    device; ``out=tiles`` normalises in place (tiles must then be contiguous).  One launch (rg_stain_apply) on a CUDA tensor."""
    N, H, W = _tile_args(tiles, layout, order, "stain.normalize")
    if not isinstance(fit, StainFit) or not isinstance(target, StainFit):
        raise ValueError("fit and target are StainFit objects")
    pinv6, scale2, href6 = apply_operands(fit, target)
    if out is None:
        out = torch.empty(tiles.shape, dtype=torch.uint8, device=tiles.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != tiles.shape or out.device != tiles.device
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor of shape %s on %s" % (tuple(tiles.shape), tiles.device))
    inplace = out.data_ptr() == tiles.data_ptr() and N > 0
    if inplace and not tiles.is_contiguous():
        raise ValueError("normalising in place needs contiguous tiles")
    if N == 0:
        return out
    if tiles.device.type != "cuda":
        res = _apply_numpy(np.ascontiguousarray(rgb_numpy(tiles, layout, order)), pinv6, scale2, href6)
        rgb_numpy(out, layout, order)[...] = res
        return out
    src = tiles if inplace else tiles.contiguous()
    D = _Device.get(tiles.device)
    p6, s2, h6 = _ll(pinv6), _ll(scale2), _ii(href6)
    for a, b in _pieces(N, H, W, None):
        _abi.launch("rg_stain_apply", tiles.device, src[a:b].data_ptr(), out[a:b].data_ptr(), b - a, H, W, export_flags(layout, order),
                    D.od.data_ptr(), p6, QP, s2, QS, h6, QH + QOD - QO, D.out.data_ptr(), D.L, D.off)
    return out


def normalize_tiles(tiles, target=REFERENCE_TARGET, layout="nhwc", order="rgb", batch=None):
    """fit + normalize -> (normalised tiles, the StainFit)"""
    f = fit(tiles, layout, order, batch)
    return normalize(tiles, f, target, None, layout, order), f


def load_target(spec):
    """``reference``, or the path of a JSON file holding a StainFit (``StainFit.to_json``, or the stain.json of an earlier run)"""
    if spec in (None, "reference"):
        return REFERENCE_TARGET
    with open(spec) as f:
        return StainFit.from_json(f.read())


def stain_report(fit, target, normalized, message=None):
    """what the programs write as stain.json beside a store"""
    d = {"method": "macenko", "normalized": bool(normalized), "fit": None if fit is None else json.loads(fit.to_json()),
         "target": json.loads(target.to_json())}
    if message:
        d["message"] = message
    return json.dumps(d, indent=1)
