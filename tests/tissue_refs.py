"""numpy restatement of rg_tile_qc's contract (include/rnagan_hip.h), shared by the tissue test files, and the tiles they use.

Per tile, nothing shared between tiles; every returned value is an integer:
  histograms  256 bins each of R, G, B and of s8 = (255 * (mx - mn)) // mx (0 where mx == 0)
  Otsu        lo / hi the smallest / largest occupied bin; for k = lo .. hi - 1, each step a separately rounded fp64 operation:
                w1 = sum_{i <= k} h[i], w2 = n - w1, s1 = sum_{i <= k} i h[i], s2 = S - s1
                m1 = s1 / w1, m2 = s2 / w2, d = m1 - m2, v = ((w1 * w2) * d) * d
              the first k with the largest v; lo == hi: lo
  raw mask    (s8 > tS) and not (R > tR and G > tG and B > tB) and R > rgb_min and G > rgb_min and B > rgb_min
  dilation    `dilate` iterations of the 4-connected cross, background outside the tile
  luma        L = 2125 R + 7154 G + 721 B; the values at four ranks of the ascending sorted L
  stats       tR, tG, tB, tS, raw_count, dilated_count, L[rank 0..3], 0, 0
The Otsu loop below is written one candidate at a time with Python floats (IEEE doubles, one rounding per operation);
tests/test_tissue_refs_cpu.py pins it against an exact fractions.Fraction argmax on every histogram the GPU tests use."""
from fractions import Fraction

import numpy as np

PLANAR, REVERSE = 1, 2
COARSE_SHIFT = 10                 # the device's two-level selection: coarse bin L >> 10, fine bin L & 1023
SHAPES = [(1, 8, 8), (3, 16, 20), (2, 64, 64), (1, 256, 256), (1, 300, 260), (5, 33, 7)]
DILATES = (0, 1, 3, 8)


def flags_of(layout, order):
    return (PLANAR if layout == "nchw" else 0) | (REVERSE if order == "bgr" else 0)


def s8_ref(rgb):
    x = rgb.astype(np.int64)
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    out = np.zeros(mx.shape, dtype=np.int64)
    nz = mx > 0
    out[nz] = (255 * (mx[nz] - mn[nz])) // mx[nz]
    return out


def luma_ref(rgb):
    x = rgb.astype(np.int64)
    return 2125 * x[..., 0] + 7154 * x[..., 1] + 721 * x[..., 2]


def histograms_ref(rgb):
    """rgb (H, W, 3) uint8 -> (4, 256) int64: R, G, B, s8"""
    chans = [rgb[..., 0], rgb[..., 1], rgb[..., 2], s8_ref(rgb)]
    return np.stack([np.bincount(np.asarray(c, dtype=np.int64).reshape(-1), minlength=256) for c in chans])


def otsu_ref(h):
    h = [int(v) for v in h]
    occ = [i for i, v in enumerate(h) if v]
    lo, hi = occ[0], occ[-1]
    if lo == hi:
        return lo
    n, S = sum(h), sum(i * v for i, v in enumerate(h))
    w1 = s1 = 0                                  # nothing lies below lo
    best, bestk = -1.0, None
    for k in range(lo, hi):
        w1 += h[k]
        s1 += k * h[k]
        w2, s2 = n - w1, S - s1
        m1 = float(s1) / float(w1)
        m2 = float(s2) / float(w2)
        d = m1 - m2
        v = ((float(w1) * float(w2)) * d) * d
        if v > best:
            best, bestk = v, k
    return bestk


def otsu_exact(h):
    """The same rule in exact rational arithmetic: the first k with the largest exact v."""
    h = [int(v) for v in h]
    occ = [i for i, v in enumerate(h) if v]
    lo, hi = occ[0], occ[-1]
    if lo == hi:
        return lo
    n, S = sum(h), sum(i * v for i, v in enumerate(h))
    best, bestk = None, None
    w1 = s1 = 0
    for k in range(lo, hi):
        w1 += h[k]
        s1 += k * h[k]
        w2, s2 = n - w1, S - s1
        d = Fraction(s1, w1) - Fraction(s2, w2)
        v = w1 * w2 * d * d
        if best is None or v > best:
            best, bestk = v, k
    return bestk


def dilate_ref(mask, iterations):
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    for _ in range(iterations):
        p = np.zeros((H + 2, W + 2), dtype=bool)
        p[1:-1, 1:-1] = m
        m = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return m


def ranks_ref(n, percentiles=(1, 99)):
    ranks = []
    for q in percentiles:
        lo = int(np.floor(q / 100.0 * (n - 1)))
        ranks += [lo, min(lo + 1, n - 1)]
    return tuple(ranks)


def tile_ref(rgb, rgb_min=50, dilate=3, ranks=None):
    """rgb (H, W, 3) uint8 in R, G, B order -> (12 ints, raw mask, dilated mask)"""
    H, W, _ = rgb.shape
    ranks = ranks_ref(H * W) if ranks is None else ranks
    x = rgb.astype(np.int64)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    s8 = s8_ref(rgb)
    tR, tG, tB, tS = (otsu_ref(h) for h in histograms_ref(rgb))
    raw = (s8 > tS) & ~((R > tR) & (G > tG) & (B > tB)) & (R > rgb_min) & (G > rgb_min) & (B > rgb_min)
    dil = dilate_ref(raw, dilate)
    L = np.sort(luma_ref(rgb).reshape(-1), kind="stable")
    row = [tR, tG, tB, tS, int(raw.sum()), int(dil.sum())] + [int(L[r]) for r in ranks] + [0, 0]
    return row, raw, dil


_REF_CACHE = {}


def batch_ref(rgb, rgb_min=50, dilate=3, ranks=None, key=None):
    """rgb (N, H, W, 3) -> (stats (N, 12) int32, dilated masks (N, H, W) uint8); cached under `key` when one is given (the
    references are computed once and never modified)"""
    N, H, W, _ = rgb.shape
    ranks = ranks_ref(H * W) if ranks is None else tuple(ranks)
    ck = None if key is None else (key, rgb_min, dilate, ranks)
    if ck is not None and ck in _REF_CACHE:
        return _REF_CACHE[ck]
    stats = np.zeros((N, 12), dtype=np.int32)
    masks = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        row, _, dil = tile_ref(rgb[n], rgb_min, dilate, ranks)
        stats[n] = row
        masks[n] = dil
    stats.setflags(write=False)
    masks.setflags(write=False)
    if ck is not None:
        _REF_CACHE[ck] = (stats, masks)
    return stats, masks


def stored(rgb, layout, order):
    """The bytes a caller stores for (N, H, W, 3) RGB tiles under a layout and a channel order."""
    a = rgb[..., ::-1] if order == "bgr" else rgb
    if layout == "nchw":
        a = a.transpose(0, 3, 1, 2)
    return np.array(a, order="C")              # always a fresh, writable copy


# ------------------------------------------------------------------ the tiles of the tests
_TILES = {}


def tissue_like(N, H, W, seed):
    """Random tiles with structure: a bright, unsaturated background (R, G, B in 200..255, nearly grey) and pink / purple blobs
    (saturated, darker) in random rectangles, so that the mask is neither empty nor full; plus uniform noise in the last tile."""
    rng = np.random.default_rng([41, N, H, W, seed])
    base = rng.integers(215, 256, size=(N, H, W, 1), dtype=np.int64) + rng.integers(-6, 7, size=(N, H, W, 3))
    out = np.clip(base, 0, 255)
    for n in range(N):
        for _ in range(3):
            r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            r1, c1 = r0 + 1 + int(rng.integers(0, max(H // 2, 1))), c0 + 1 + int(rng.integers(0, max(W // 2, 1)))
            blob = np.stack([rng.integers(120, 220, size=(H, W)), rng.integers(40, 140, size=(H, W)),
                             rng.integers(110, 200, size=(H, W))], axis=-1)
            out[n, r0:r1, c0:c1] = blob[r0:r1, c0:c1]
    if N > 1:
        out[N - 1] = rng.integers(0, 256, size=(H, W, 3))
    return out.astype(np.uint8)


def random_tiles(N, H, W):
    key = ("random", N, H, W)
    if key not in _TILES:
        a = tissue_like(N, H, W, 0)
        a.setflags(write=False)
        _TILES[key] = a
    return _TILES[key]


def constant_tile(H, W, rgb=(200, 120, 180)):
    a = np.empty((1, H, W, 3), dtype=np.uint8)
    a[...] = np.array(rgb, dtype=np.uint8)
    return a


def two_level_tile(H, W, a=(230, 228, 231), b=(150, 60, 140)):
    """Two colours with equal populations (H W even): every Otsu candidate between the two occupied bins ties exactly."""
    t = np.empty((H * W, 3), dtype=np.uint8)
    t[0::2] = np.array(a, dtype=np.uint8)
    t[1::2] = np.array(b, dtype=np.uint8)
    return t.reshape(1, H, W, 3)


def single_pixel_tile(H, W, r, c, on=(150, 60, 140), bg=(230, 230, 230)):
    """A grey background (s8 = 0) with ONE saturated pixel: the raw mask is that pixel alone."""
    t = constant_tile(H, W, bg)
    t[0, r, c] = np.array(on, dtype=np.uint8)
    return t


def _boundary_colours():
    if "boundary" not in _TILES:
        g = np.arange(256, dtype=np.int64)
        L = (2125 * g[:, None, None] + 7154 * g[None, :, None] + 721 * g[None, None, :]).reshape(-1)
        order = np.argsort(L, kind="stable")
        Ls = L[order]
        cols = []
        for mult in (3, 700, 1301, 2489):
            edge = mult << COARSE_SHIFT
            i = int(np.searchsorted(Ls, edge, side="left"))
            for j in (i - 2, i - 1, i, i + 1):
                idx = int(order[j])
                cols.append((idx >> 16, (idx >> 8) & 255, idx & 255))
            assert Ls[i - 1] < edge <= Ls[i]
        _TILES["boundary"] = cols
    return _TILES["boundary"]


def luma_boundary_tile(H, W):
    """Pixels whose luma lies on both sides of coarse-bin boundaries (multiples of 1 << COARSE_SHIFT): for boundaries spread over
    the range, the colours with the largest L below and the smallest L at or above, filling the tile in equal shares, so the
    1st / 99th percentile ranks and rank 0 / n - 1 fall next to a boundary."""
    cols = _boundary_colours()
    t = np.empty((H * W, 3), dtype=np.uint8)
    for p in range(H * W):
        t[p] = cols[(p * len(cols)) // (H * W)]
    return t.reshape(1, H, W, 3)


def all_test_histograms():
    """Every 256-bin histogram whose Otsu threshold a GPU test expects: the four histograms of every tile of every content."""
    out = []
    for (N, H, W) in SHAPES:
        for n in range(N):
            out += list(histograms_ref(random_tiles(N, H, W)[n]))
    for t in special_tiles():
        out += list(histograms_ref(t[0]))
    return out


def special_tiles():
    H, W = 16, 20
    tiles = [constant_tile(H, W), constant_tile(H, W, (0, 0, 0)), constant_tile(256, 256, (201, 201, 201)), two_level_tile(H, W),
             two_level_tile(64, 64), luma_boundary_tile(H, W), luma_boundary_tile(64, 64)]
    for (r, c) in ((8, 10), (0, 10), (8, 0), (0, 0), (15, 19)):
        tiles.append(single_pixel_tile(H, W, r, c))
    return tiles
