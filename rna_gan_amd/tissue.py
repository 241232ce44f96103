"""Tile quality control: the acceptance rule of the reference's tiler (src/preprocess/patch_gen_grid.py: a tissue mask from
per-channel Otsu thresholds, an Otsu threshold on the HSV saturation and a floor on R, G and B, dilated three times, must cover
more than 20 % of the tile, and the tile must not be low-contrast), applied to uint8 tiles where they already are -- on the device.

``tile_stats`` (rg_tile_qc, rna_gan_amd/csrc/rg_tissue.hip) returns INTEGERS per tile: four thresholds, the raw and the dilated
mask counts and four order statistics of the integer luma L = 2125 R + 7154 G + 721 B.  The arithmetic contract is stated in
include/rnagan_hip.h and restated in tests/tissue_refs.py; every float decision (``tissue_fraction``, ``luma_percentiles``,
``low_contrast``, ``accept``) is made here, on the host, from those integers.

Two deliberate restatements, neither checkable without scikit-image (absent where this was written), so no parity with it is
claimed: the saturation is binned on a fixed 8-bit grid, s8 = (255 (mx - mn)) // mx, where the reference bins the float
saturation into 256 bins over the tile's own range (the threshold can differ by about one bin); and ``low_contrast`` divides by
``luma_range = 2.0``, what ``skimage.exposure.is_low_contrast`` effectively applies to a float grey image.

On a CPU tensor ``tile_stats`` computes the same integers with numpy (callers stay testable anywhere); on a CUDA tensor there is no
fallback: the kernels run or the call raises.  The slide-level closing (dilate, then erode) of the reference's thumbnail mask and the
tiler that applies this rule to a slide raster are rna_gan_amd.tiler; out of scope remains a reader for scanner formats.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi
from .export import RG_EXPORT_PLANAR, RG_EXPORT_REVERSE, export_flags, rgb_numpy, tile_args  # noqa: F401 (the flag bits: tests/test_tissue_refs_cpu.py reads them here)

MAX_DILATE = 8
MAX_PIXELS = 1 << 26
LUMA_WEIGHTS = (2125, 7154, 721)          # skimage's rgb2gray weights x 10 000
LUMA_SCALE = 10000.0 * 255.0
_WS = {}                                  # (device type, index) -> one cached uint8 workspace, grown on demand


class TileStats:
    """What ``tile_stats`` returns, all numpy on the host: ``thresholds`` (N, 4) int32 tR, tG, tB, tS; ``raw_count`` and
    ``dilated_count`` (N,) int32; ``luma`` (N, 4) int32, the order statistics of L at ``ranks``; ``ranks`` the four ranks;
    ``weights`` (len(percentiles), ) the interpolation weight of the upper statistic of each percentile; ``percentiles``;
    ``H``, ``W``; ``mask``: None, or the dilated mask, a uint8 (N, H, W) tensor of 0 / 1 on the tiles' device."""

    def __init__(self, stats, H, W, ranks, weights, percentiles, rgb_min, dilate, mask=None):
        stats = np.ascontiguousarray(stats, dtype=np.int32).reshape(-1, 12)
        self.stats = stats
        self.thresholds = stats[:, 0:4]
        self.raw_count = stats[:, 4]
        self.dilated_count = stats[:, 5]
        self.luma = stats[:, 6:10]
        self.H, self.W = int(H), int(W)
        self.ranks = tuple(int(r) for r in ranks)
        self.weights = tuple(float(w) for w in weights)
        self.percentiles = tuple(float(q) for q in percentiles)
        self.rgb_min, self.dilate = int(rgb_min), int(dilate)
        self.mask = mask

    def __len__(self):
        return self.stats.shape[0]


def percentile_ranks(n, percentiles=(1, 99)):
    """numpy's linear percentile on n sorted values: position q / 100 (n - 1), its floor, and floor + 1 clipped to n - 1.
    Returns (the four ranks lo0, hi0, lo1, hi1; the two weights of the upper statistic)."""
    if len(percentiles) != 2:
        raise ValueError("two percentiles are taken")
    ranks, weights = [], []
    for q in percentiles:
        q = float(q)
        if not 0.0 <= q <= 100.0:
            raise ValueError("a percentile must be in [0, 100]")
        pos = q / 100.0 * (n - 1)
        lo = int(np.floor(pos))
        ranks += [lo, min(lo + 1, n - 1)]
        weights.append(pos - lo)
    return tuple(ranks), tuple(weights)


def _check(tiles, layout, order, rgb_min, dilate):
    N, H, W = tile_args(tiles, layout, order, "tile_stats")
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError("tile_stats needs 1 <= H W <= 2^26, got H %d W %d" % (H, W))
    if not 0 <= int(rgb_min) <= 255:
        raise ValueError("rgb_min must be in 0..255")
    if not 0 <= int(dilate) <= MAX_DILATE:
        raise ValueError("dilate must be in 0..%d" % MAX_DILATE)
    return N, H, W


# ------------------------------------------------------------------ the numpy path (CPU tensors)
def _otsu(h):
    """The contract's Otsu threshold of an integer histogram of 256 bins."""
    h = np.asarray(h, dtype=np.int64)
    occ = np.flatnonzero(h)
    lo, hi = int(occ[0]), int(occ[-1])
    if lo == hi:
        return lo
    idx = np.arange(256, dtype=np.int64)
    w1 = np.cumsum(h)[lo:hi]
    s1 = np.cumsum(idx * h)[lo:hi]
    w2 = h.sum() - w1
    s2 = (idx * h).sum() - s1
    d = s1.astype(np.float64) / w1.astype(np.float64) - s2.astype(np.float64) / w2.astype(np.float64)
    v = ((w1.astype(np.float64) * w2.astype(np.float64)) * d) * d
    return lo + int(np.argmax(v))


def _dilate(m, d):
    m = m.copy()
    for _ in range(d):
        g = m.copy()
        g[1:] |= m[:-1]
        g[:-1] |= m[1:]
        g[:, 1:] |= m[:, :-1]
        g[:, :-1] |= m[:, 1:]
        m = g
    return m


def _tile_stats_numpy(rgb, rgb_min, dilate, ranks, want_mask):
    """rgb: (N, H, W, 3) uint8 numpy in R, G, B order -> (stats (N, 12) int32, mask (N, H, W) uint8 or None)"""
    N, H, W, _ = rgb.shape
    stats = np.zeros((N, 12), dtype=np.int32)
    mask = np.zeros((N, H, W), dtype=np.uint8) if want_mask else None
    for n in range(N):
        x = rgb[n].astype(np.int64)
        R, G, B = x[..., 0], x[..., 1], x[..., 2]
        mx, mn = x.max(axis=-1), x.min(axis=-1)
        s8 = np.where(mx == 0, 0, (255 * (mx - mn)) // np.maximum(mx, 1))
        t = [_otsu(np.bincount(c.reshape(-1), minlength=256)) for c in (R, G, B, s8)]
        raw = (s8 > t[3]) & ~((R > t[0]) & (G > t[1]) & (B > t[2])) & (R > rgb_min) & (G > rgb_min) & (B > rgb_min)
        dil = _dilate(raw, dilate)
        L = np.sort((LUMA_WEIGHTS[0] * R + LUMA_WEIGHTS[1] * G + LUMA_WEIGHTS[2] * B).reshape(-1))
        stats[n, :4] = t
        stats[n, 4], stats[n, 5] = int(raw.sum()), int(dil.sum())
        stats[n, 6:10] = L[list(ranks)]
        if want_mask:
            mask[n] = dil
    return stats, mask


# ------------------------------------------------------------------ the public functions
def tile_stats(tiles, layout="nhwc", order="rgb", rgb_min=50, dilate=3, percentiles=(1, 99), return_mask=False):
    """uint8 tiles, (N, H, W, 3) (layout "nhwc") or (N, 3, H, W) ("nchw"), channels stored R, G, B (order "rgb") or B, G, R
    ("bgr") -> TileStats.  On a CUDA tensor: five launches on the current stream (rg_tile_qc), then ONE download of
    12 int32 per tile; the mask, when asked for, stays on the device."""
    N, H, W = _check(tiles, layout, order, rgb_min, dilate)
    rgb_min, dilate = int(rgb_min), int(dilate)
    ranks, weights = percentile_ranks(H * W, percentiles)
    if N == 0:
        mask = torch.empty((0, H, W), dtype=torch.uint8, device=tiles.device) if return_mask else None
        return TileStats(np.zeros((0, 12), np.int32), H, W, ranks, weights, percentiles, rgb_min, dilate, mask)
    if tiles.device.type != "cuda":
        stats, mask = _tile_stats_numpy(rgb_numpy(tiles, layout, order), rgb_min, dilate, ranks, return_mask)
        return TileStats(stats, H, W, ranks, weights, percentiles, rgb_min, dilate, None if mask is None else torch.from_numpy(mask))
    stats, mask = tile_stats_device(tiles, layout, order, rgb_min, dilate, percentiles, return_mask)
    return TileStats(stats.cpu().numpy(), H, W, ranks, weights, percentiles, rgb_min, dilate, mask)


def tile_stats_device(tiles, layout="nhwc", order="rgb", rgb_min=50, dilate=3, percentiles=(1, 99), return_mask=False, out=None):
    """The launches of ``tile_stats`` alone, for a caller that schedules the download itself (export.synthesize_u8): CUDA uint8
    tiles -> (int32 (N, 12) stats ON THE DEVICE, mask or None).  No host synchronisation.  out: an optional contiguous int32
    (N, 12) device tensor that receives the rows.  ``stats_from_rows`` turns downloaded rows into a TileStats."""
    N, H, W = _check(tiles, layout, order, rgb_min, dilate)
    if tiles.device.type != "cuda":
        raise ValueError("tile_stats_device runs the HIP kernels: tiles must be on a CUDA device")
    ranks, _ = percentile_ranks(H * W, percentiles)
    dev = tiles.device
    if out is None:
        out = torch.empty((N, 12), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (N, 12) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int32 tensor of shape (%d, 12) on %s" % (N, dev))
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    if N == 0:
        return out, mask
    src = tiles.contiguous()
    need = int(_abi.load().rg_tile_qc_workspace_bytes(N, H, W))
    key = _abi.device_key(dev)
    ws = _WS.get(key)                       # one buffer per device: calls on one stream follow each other and each zeroes it first
    if ws is None or ws.numel() < need:
        ws = _WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    _abi.launch("rg_tile_qc", dev, src.data_ptr(), N, H, W, export_flags(layout, order), int(rgb_min), int(dilate),
                (ctypes.c_int * 4)(*ranks), out.data_ptr(), None if mask is None else mask.data_ptr(), ws.data_ptr(), ws.numel())
    return out, mask


def stats_from_rows(rows, H, W, rgb_min=50, dilate=3, percentiles=(1, 99)):
    """A TileStats from (N, 12) integer rows (downloaded from ``tile_stats_device``, or read back from a report) of H x W tiles."""
    ranks, weights = percentile_ranks(int(H) * int(W), percentiles)
    return TileStats(np.array(rows, dtype=np.int32).reshape(-1, 12), H, W, ranks, weights, percentiles, rgb_min, dilate)


def tissue_fraction(stats):
    """dilated_count / (H W), float64 (N,)"""
    return stats.dilated_count.astype(np.float64) / float(stats.H * stats.W)


def luma_percentiles(stats):
    """(N, 2) float64: the two percentiles of the grey image L / (10000 * 255) in [0, 1], interpolated linearly between the two
    order statistics of each as numpy's percentile does (lo + (hi - lo) * weight), then divided."""
    L = stats.luma.astype(np.float64)
    out = np.empty((len(stats), 2), dtype=np.float64)
    for j in range(2):
        lo, hi = L[:, 2 * j], L[:, 2 * j + 1]
        out[:, j] = (lo + (hi - lo) * stats.weights[j]) / LUMA_SCALE
    return out


def low_contrast(stats, fraction=0.05, luma_range=2.0):
    """True where (p_hi - p_lo) / luma_range < fraction.  luma_range = 2.0 is what skimage.exposure.is_low_contrast effectively
    applies to a float grey image (its dtype limits are -1 .. 1): restated from the documentation, NOT checkable here (scikit-image
    is absent), so no parity with it is claimed."""
    p = luma_percentiles(stats)
    return (p[:, 1] - p[:, 0]) / float(luma_range) < float(fraction)


def accept(stats, min_tissue=0.2, fraction=0.05, luma_range=2.0):
    """The tiler's rule: dilated_count > min_tissue * (H W) (the reference's comparison) and not low-contrast."""
    enough = stats.dilated_count.astype(np.float64) > float(min_tissue) * float(stats.H * stats.W)
    return enough & ~low_contrast(stats, fraction, luma_range)
