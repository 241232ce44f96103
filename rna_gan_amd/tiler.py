"""The tiler: from a slide raster to the tiles of a tile store, as the reference's src/preprocess/patch_gen_grid.py makes them -- a
closed tissue mask of a thumbnail, a shuffled grid of candidate windows, the acceptance rule of rna_gan_amd.tissue on every window
at the read size, and Pillow's ``Image.resize`` of the accepted windows to the patch size -- with the raster on the device.

The kernels (rna_gan_amd/csrc/rg_tiler.hip; contracts in include/rnagan_hip.h, restated in tests/tiler_refs.py) are integer-only:
  ``resize_windows``  rg_window_resize_u8: N windows cropped (zeros outside the raster) and resized in one launch, byte for byte
                      Pillow's 8-bit bicubic resize with antialiasing.  ``pillow_tables`` is the host half: Pillow's coefficients,
                      computed in fp64 and rounded to 22 fractional bits exactly as Resample.c does.
  ``erode``           rg_mask_erode: erosion by the L1 ball, outside counted as unset (scipy's ``binary_erosion(iterations=r)``).
  ``thumbnail``       rg_box_reduce_u8: a box average, for a raster that brings no pyramid level of its own.
``slide_mask`` is tissue.tile_stats' dilated mask followed by ``erode``: the reference's binary closing of the thumbnail mask.

The conventions are those of rna_gan_amd.tissue: on a CPU tensor every function computes the same bytes with numpy; on a CUDA tensor
there is no fallback, the kernels run or the call raises.  Out of scope: a reader for scanner formats (.svs), and rasters that do
not fit the device (no streaming in strips).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import _abi
from . import tissue
from .export import ORDERS, RG_EXPORT_REVERSE

PRECISION_BITS = 22            # Pillow's 32 - 8 - 2
MAX_K = 35                     # widest coefficient row the kernel takes: a scale up to 8.5
MAX_OUT = 1024
MAX_READ = 8192
MAX_FACTOR = 64
_TABLES = {}                   # (n_in, n_out, device) -> the device table of rg_window_resize_u8


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def _tables(n_in, n_out):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    K = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, K), dtype=np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = [_bicubic((j + xmin - center + 0.5) / fs) for j in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        for j, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coef[i, j] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[i] = (xmin, xmax - xmin)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def pillow_tables(n_in, n_out):
    """Pillow's resampling coefficients of one axis for its default filter of ``Image.resize`` (bicubic, antialiased), n_in -> n_out
    pixels: (bounds int32 (n_out, 2): xmin and count; coefficients int32 (n_out, K): k_j with 22 fractional bits, zero padded).
    Every step is a Python float (C double) operation in Resample.c's order.  The arrays are shared and read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("pillow_tables needs n_in, n_out >= 1")
    return _tables(n_in, n_out)


def _pair(v, what):
    if isinstance(v, (int, np.integer)):
        v = (int(v), int(v))
    v = tuple(int(x) for x in v)
    if len(v) != 2 or v[0] < 1 or v[1] < 1:
        raise ValueError("%s must be a positive int or a pair (rows, columns)" % what)
    return v


def _check_raster(raster, what):
    if not torch.is_tensor(raster) or raster.dim() != 3 or raster.dtype != torch.uint8 or raster.shape[2] != 3 \
            or raster.shape[0] < 1 or raster.shape[1] < 1:
        raise ValueError("%s takes a uint8 (RH, RW, 3) tensor" % what)
    if raster.shape[0] > 0x7fffffff or raster.shape[1] > 0x7fffffff:
        raise ValueError("%s: a raster side is limited to 2^31 - 1" % what)


def _origins_numpy(origins):
    if torch.is_tensor(origins):
        origins = origins.cpu().numpy()
    o = np.asarray(origins)
    if o.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError("origins must be integers of shape (N, 2): (x, y) per window")
    if o.min() < -(1 << 31) or o.max() > (1 << 31) - 1:
        raise ValueError("origins must fit int32")
    return np.ascontiguousarray(o, dtype=np.int32)


# ------------------------------------------------------------------ the numpy path (CPU tensors)
def _crop_numpy(a, origins, h, w):
    """(N, h, w, 3) windows of a (RH, RW, 3) array, zeros outside it"""
    RH, RW = a.shape[:2]
    out = np.zeros((len(origins), h, w, 3), dtype=np.uint8)
    for n, (x, y) in enumerate(origins):
        x, y = int(x), int(y)
        y0, y1, x0, x1 = max(y, 0), min(y + h, RH), max(x, 0), min(x + w, RW)
        if y0 < y1 and x0 < x1:
            out[n, y0 - y:y1 - y, x0 - x:x1 - x] = a[y0:y1, x0:x1]
    return out


def _pass_numpy(win, n_out):
    """one pass of the contract along axis 2 of (N, rows, n_in, 3) uint8 -> (N, rows, n_out, 3) uint8"""
    n_in = win.shape[2]
    if n_in == n_out:
        return win
    bounds, coef = _tables(n_in, n_out)
    out = np.empty(win.shape[:2] + (n_out, 3), dtype=np.uint8)
    for i in range(n_out):
        m, c = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (win[:, :, m:m + c].astype(np.int64) * coef[i, :c].astype(np.int64)[None, None, :, None]).sum(axis=2) + (1 << (PRECISION_BITS - 1))
        out[:, :, i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def _resize_numpy(win, oh, ow):
    mid = _pass_numpy(win, ow)                                                  # horizontal first, rounded to bytes
    return _pass_numpy(mid.transpose(0, 2, 1, 3), oh).transpose(0, 2, 1, 3)     # then vertical over those bytes


def _erode_numpy(m, r):
    m = m != 0
    for _ in range(r):
        g = m.copy()
        g[:, 1:] &= m[:, :-1]
        g[:, :-1] &= m[:, 1:]
        g[:, :, 1:] &= m[:, :, :-1]
        g[:, :, :-1] &= m[:, :, 1:]
        g[:, 0] = g[:, -1] = False                                              # outside counts as unset
        g[:, :, 0] = g[:, :, -1] = False
        m = g
    return m.astype(np.uint8)


def _box_numpy(a, f):
    RH, RW = a.shape[:2]
    TH, TW = -(-RH // f), -(-RW // f)
    pad = np.zeros((TH * f, TW * f, 3), dtype=np.int64)
    pad[:RH, :RW] = a
    s = pad.reshape(TH, f, TW, f, 3).sum(axis=(1, 3))
    cy = np.minimum(f, RH - np.arange(TH) * f)
    cx = np.minimum(f, RW - np.arange(TW) * f)
    cnt = (cy[:, None] * cx[None, :])[:, :, None]
    return ((s + cnt // 2) // cnt).astype(np.uint8)


# ------------------------------------------------------------------ the public functions
def _device_table(n_in, n_out, dev):
    key = (n_in, n_out) + _abi.device_key(dev)
    t = _TABLES.get(key)
    if t is None:
        bounds, coef = _tables(n_in, n_out)
        if len(_TABLES) >= 64:
            _TABLES.clear()
        t = _TABLES[key] = torch.from_numpy(np.concatenate([bounds, coef], axis=1)).to(dev)
    return t


def resize_windows(raster, origins, read_size, out_size, order="rgb"):
    """N windows of ``raster`` (uint8 (RH, RW, 3), R, G, B), window n at origins[n] = (x, y) with x the column, each read_size
    (rows, columns, or one int) pixels, a pixel outside the raster reading as 0 -- what ``read_region(...).convert('RGB')`` gives --
    resized to out_size as ``PIL.Image.resize`` with its default filter does; equal sizes: a plain crop.  order "bgr" writes B, G, R,
    the order of a tile store's records.  origins: integers (N, 2), on the host or an int32 tensor on the raster's device.
    -> uint8 (N, oh, ow, 3) on the raster's device.  One launch on the current stream, no synchronisation."""
    _check_raster(raster, "resize_windows")
    if order not in ORDERS:
        raise ValueError("order must be one of %s" % (ORDERS,))
    (h, w), (oh, ow) = _pair(read_size, "read_size"), _pair(out_size, "out_size")
    if oh > MAX_OUT or ow > MAX_OUT or h > MAX_READ or w > MAX_READ:
        raise ValueError("resize_windows: out_size is limited to %d, read_size to %d" % (MAX_OUT, MAX_READ))
    for a, b in ((h, oh), (w, ow)):
        if a != b and int(math.ceil(2.0 * max(a / b, 1.0))) * 2 + 1 > MAX_K:
            raise ValueError("resize_windows: %d -> %d needs more than %d coefficients per pixel (a scale above 8.5)" % (a, b, MAX_K))
    dev = raster.device
    if dev.type != "cuda":
        o = _origins_numpy(origins)
        out = _resize_numpy(_crop_numpy(raster.numpy(), o, h, w), oh, ow)
        if order == "bgr":
            out = out[..., ::-1]
        return torch.from_numpy(np.ascontiguousarray(out))
    if torch.is_tensor(origins) and origins.device == dev and origins.dtype == torch.int32 and origins.dim() == 2 \
            and origins.shape[1] == 2:
        o = origins.contiguous()
    else:
        o = torch.from_numpy(_origins_numpy(origins)).to(dev)
    N = o.shape[0]
    out = torch.empty((N, oh, ow, 3), dtype=torch.uint8, device=dev)
    if N == 0:
        return out
    src = raster.contiguous()
    xt = None if w == ow else _device_table(w, ow, dev)
    yt = None if h == oh else _device_table(h, oh, dev)
    _abi.launch("rg_window_resize_u8", dev, src.data_ptr(), src.shape[0], src.shape[1], o.data_ptr(), N, h, w, oh, ow,
                None if xt is None else xt.data_ptr(), 0 if xt is None else xt.shape[1] - 2,
                None if yt is None else yt.data_ptr(), 0 if yt is None else yt.shape[1] - 2,
                out.data_ptr(), RG_EXPORT_REVERSE if order == "bgr" else 0)
    return out


def erode(mask, radius):
    """uint8 masks (N, H, W) or (H, W), a byte != 0 set -> the same shape, 0 / 1: a pixel survives iff every pixel within L1
    distance ``radius`` (0..8) is set, everything outside the rectangle counting as unset -- ``radius`` iterations of scipy's
    binary_erosion."""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.dim() not in (2, 3):
        raise ValueError("erode takes a uint8 (N, H, W) or (H, W) tensor")
    radius = int(radius)
    if not 0 <= radius <= tissue.MAX_DILATE:
        raise ValueError("radius must be in 0..%d" % tissue.MAX_DILATE)
    m = mask if mask.dim() == 3 else mask[None]
    N, H, W = m.shape
    if H < 1 or W < 1:
        raise ValueError("erode needs H, W >= 1")
    if m.device.type != "cuda":
        out = torch.from_numpy(_erode_numpy(m.numpy(), radius)) if N else torch.empty_like(m)
    else:
        src = m.contiguous()
        out = torch.empty_like(src)
        if N:
            _abi.launch("rg_mask_erode", m.device, src.data_ptr(), out.data_ptr(), N, H, W, radius)
    return out if mask.dim() == 3 else out[0]


def thumbnail(raster, factor):
    """uint8 (RH, RW, 3) -> (ceil(RH / factor), ceil(RW / factor), 3): the rounded integer mean (sum + cnt / 2) // cnt of each
    factor x factor block, cnt the block's pixels inside the raster; 1 <= factor <= 64.  For a raster without a pyramid level of its
    own; no parity with a scanner's thumbnail is claimed."""
    _check_raster(raster, "thumbnail")
    factor = int(factor)
    if not 1 <= factor <= MAX_FACTOR:
        raise ValueError("factor must be in 1..%d" % MAX_FACTOR)
    if raster.device.type != "cuda":
        return torch.from_numpy(_box_numpy(raster.numpy(), factor))
    src = raster.contiguous()
    RH, RW = src.shape[:2]
    out = torch.empty((-(-RH // factor), -(-RW // factor), 3), dtype=torch.uint8, device=src.device)
    _abi.launch("rg_box_reduce_u8", src.device, src.data_ptr(), RH, RW, factor, out.data_ptr())
    return out


_thumbnail = thumbnail          # tile_raster has a parameter of that name


def slide_mask(thumbnail_u8, rgb_min=50, iterations=3):
    """The closed tissue mask of a thumbnail (uint8 (H, W, 3), rows = y): tissue.tile_stats' mask of the whole thumbnail as ONE
    tile, dilated ``iterations`` times, then eroded as often -- the reference's binary_dilation(iterations=3) followed by
    binary_erosion(iterations=3).  -> uint8 (H, W) of 0 / 1 on the thumbnail's device."""
    _check_raster(thumbnail_u8, "slide_mask")
    st = tissue.tile_stats(thumbnail_u8[None], rgb_min=rgb_min, dilate=iterations, return_mask=True)
    return erode(st.mask, iterations)[0]


def grid_origins(RW, RH, read, seed=5):
    """The reference's candidates in its order: (x, y) for x in range(0, RW, read[0]) for y in range(0, RH, read[0]) -- x the outer
    loop, BOTH steps read[0], as the reference has it -- shuffled by numpy's legacy generator seeded with ``seed``.
    -> int32 (M, 2)."""
    read = _pair(read, "read")
    indices = [(x, y) for x in range(0, int(RW), read[0]) for y in range(0, int(RH), read[0])]
    np.random.RandomState(seed).shuffle(indices)
    return np.array(indices, dtype=np.int32).reshape(-1, 2)


def synthetic_slide(RH=2048, RW=2560, seed=0, blobs=5, smears=2):
    """A stand-in for a scanned region, uint8 (RH, RW, 3) numpy from a seeded generator: a near-white, nearly grey ground with
    ``blobs`` stained ellipses whose pixels vary the way an H&E texture's histograms do, and ``smears`` flat, saturated ellipses (a
    pen mark: inside the slide mask, low-contrast to the tile rule).  For tile_slides.py --synthetic, the tests and the
    measurements; it claims no likeness to tissue beyond what the acceptance rule looks at."""
    rng = np.random.RandomState(seed)
    a = rng.randint(228, 250, (RH, RW, 1)).astype(np.int16) + rng.randint(-4, 5, (RH, RW, 3)).astype(np.int16)
    yy, xx = np.mgrid[0:RH, 0:RW].astype(np.float32)
    lo = np.array([120, 40, 110], dtype=np.int16)
    for _ in range(int(blobs)):
        cy, cx = rng.randint(0, RH), rng.randint(0, RW)
        ry, rx = rng.randint(RH // 10, RH // 4 + 2), rng.randint(RW // 10, RW // 4 + 2)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        stain = lo + rng.randint(0, 100, (int(inside.sum()), 3)).astype(np.int16)
        a[inside] = stain
    for _ in range(int(smears)):
        cy, cx = rng.randint(0, RH), rng.randint(0, RW)
        ry, rx = rng.randint(RH // 8, RH // 4 + 2), rng.randint(RW // 8, RW // 4 + 2)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        a[inside] = np.array([70, 110, 190], dtype=np.int16) + rng.randint(-2, 3, (int(inside.sum()), 3)).astype(np.int16)
    return np.clip(a, 0, 255).astype(np.uint8)


class Tiled:
    """What ``tile_raster`` returns: ``tiles`` uint8 (n, patch, patch, 3) on the raster's device in the order asked for;
    ``origins`` int32 (n, 2) numpy, (x, y) of each tile's window in the raster; ``qc`` int32 (n, 12) numpy, the rows of
    tissue.tile_stats of each tile's window at the read size; ``mask`` uint8 (H, W) on the device, the closed slide mask;
    ``read``; ``candidates`` / ``in_mask`` / ``examined``: how many windows the grid has, how many of them the slide mask keeps,
    how many of those went through the tile rule before max_patches was reached."""

    def __init__(self, tiles, origins, qc, mask, read, candidates, in_mask, examined):
        self.tiles, self.origins, self.qc, self.mask = tiles, origins, qc, mask
        self.read, self.candidates, self.in_mask, self.examined = read, candidates, in_mask, examined

    def __len__(self):
        return self.tiles.shape[0]


def tile_raster(raster, thumbnail=None, patch_size=256, app_mag=20.0, dezoom=1.0, max_patches=2000, batch=256, thumb_factor=32,
                min_tissue=0.2, order="rgb", mask=None):
    """The reference's extract_patches on a level-0 raster (uint8 (RH, RW, 3), R, G, B) -> Tiled.
    read = int(app_mag / 20 * dezoom * patch_size) is the window size at level 0.  The slide mask is ``mask`` (uint8 (H, W), rows = y)
    when given, else ``slide_mask`` of ``thumbnail`` (a lower level of the slide), else of ``thumbnail(raster, thumb_factor)``.  A
    candidate of ``grid_origins`` is kept where mask[int(y / ratio_y), int(x / ratio_x)] is set, ratio = raster size / mask size.
    The kept candidates go through in batches, in order: crop at the read size, tissue.tile_stats_device, ONE download of 12 ints per
    tile, tissue.accept on the host, then the resize of the accepted windows alone, read from the raster again.  It stops once
    max_patches are accepted and returns the first max_patches in candidate order: the reference's sequential result whatever
    ``batch`` is."""
    _check_raster(raster, "tile_raster")
    if order not in ORDERS:
        raise ValueError("order must be one of %s" % (ORDERS,))
    patch_size, max_patches, batch = int(patch_size), int(max_patches), int(batch)
    read = int(float(app_mag) / 20.0 * float(dezoom) * patch_size)
    if patch_size < 1 or read < 1 or max_patches < 0 or batch < 1:
        raise ValueError("tile_raster needs patch_size, read >= 1, max_patches >= 0 and batch >= 1")
    dev = raster.device
    RH, RW = int(raster.shape[0]), int(raster.shape[1])
    if mask is None:
        thumb = _thumbnail(raster, thumb_factor) if thumbnail is None else thumbnail.to(dev)
        mask = slide_mask(thumb)
    else:
        if not torch.is_tensor(mask) or mask.dim() != 2 or mask.dtype != torch.uint8 or mask.numel() == 0:
            raise ValueError("mask must be a uint8 (H, W) tensor")
        mask = mask.to(dev)
    m = mask.cpu().numpy()
    ratio_x, ratio_y = RW / m.shape[1], RH / m.shape[0]
    cand = grid_origins(RW, RH, (read, read))
    kept = np.array([c for c in cand if m[int(c[1] / ratio_y), int(c[0] / ratio_x)]], dtype=np.int32).reshape(-1, 2)
    tiles, origins, rows = [], [], []
    accepted = examined = 0
    for i in range(0, len(kept), batch):
        if accepted >= max_patches:
            break
        o = kept[i:i + batch]
        crops = resize_windows(raster, o, read, read)
        if dev.type == "cuda":
            r = tissue.tile_stats_device(crops)[0].cpu().numpy()
        else:
            r = tissue.tile_stats(crops).stats
        ok = np.flatnonzero(tissue.accept(tissue.stats_from_rows(r, read, read), min_tissue=min_tissue))
        room = max_patches - accepted
        if len(ok) >= room:                                                     # the sequential rule stops at the room-th accepted
            ok = ok[:room]
            examined += int(ok[-1]) + 1
        else:
            examined += len(o)
        if len(ok):
            tiles.append(resize_windows(raster, o[ok], read, patch_size, order))
            origins.append(o[ok])
            rows.append(r[ok])
            accepted += len(ok)
    if tiles:
        out, origins, rows = torch.cat(tiles), np.concatenate(origins), np.concatenate(rows)
    else:
        out = torch.empty((0, patch_size, patch_size, 3), dtype=torch.uint8, device=dev)
        origins, rows = np.zeros((0, 2), np.int32), np.zeros((0, 12), np.int32)
    return Tiled(out, origins, rows.astype(np.int32), mask, read, len(cand), len(kept), examined)
