"""MS-SSIM between pairs of uint8 RGB tiles where they already are -- on the device (Wang, Simoncelli & Bovik 2003).

The mean MS-SSIM over random pairs of generated tiles is the pixel-space diversity score of Odena et al. 2017: it needs no feature
extractor, it is read next to the same figure over pairs of real tiles (generated pairs clearly more similar than real pairs:
collapse), and a sudden rise between epochs is the earliest cheap sign of collapse.  The same functions compare paired tiles byte for
byte -- a stain-normalised tile with its source, one resize with another.

Definition (include/rnagan_hip.h states it for the kernels, tests/msssim_refs.py restates it in numpy): an 11-tap Gaussian window,
sigma 1.5, separable, VALID extent (no padding); C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; level s is the exact 2^s x 2^s block mean of
the bytes (a last odd row or column dropped level by level); per level and channel ``cs`` and ``l * cs`` are averaged over the window
positions, then over the three channels, giving CS_s and SSIM_s;

    MS-SSIM = prod_{s < S - 1} max(CS_s, 0)^w_s * max(SSIM_{S-1}, 0)^w_{S-1}

with w the first S of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) renormalised to sum 1.  S is in 1..5 and needs
min(H, W) >> (S - 1) >= 11; the default is the largest such S (5 at 256 x 256, 3 at 64 x 64); S = 1 is plain SSIM.  The device returns
the SUMS of cs and l cs per pair, level and channel (rg_msssim_pairs, fp64, a fixed summation order); the division by the position
count, the clamp, the powers and the product run here in fp64.  The only download is P * S * 6 doubles.

No parity with scikit-image, TensorFlow or pytorch-msssim is claimed (none was installed where this was written): implementations
differ in padding (valid here) and in what they do with a negative cs (clamped to 0 here, so the score of such a pair is 0).

There is no CPU path and no fallback: the kernels run or the call raises.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi
from .export import export_flags, tile_args

BAND, COLS = _abi.CONSTANTS["RG_MSSSIM_BAND"], _abi.CONSTANTS["RG_MSSSIM_COLS"]      # window positions per workgroup
TAPS, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_SCALES = len(WEIGHTS)
PAIR_CHUNK = 4096                    # pairs per launch: the partials of a chunk take 16 bytes per workgroup


def taps():
    """the window: float64 [11], exp(-d^2 / (2 sigma^2)) for d = -5 .. 5, normalised to sum 1"""
    d = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def default_scales(H, W):
    """the largest S in 1..5 with min(H, W) >> (S - 1) >= 11"""
    if min(int(H), int(W)) < TAPS:
        raise ValueError("MS-SSIM needs tiles of at least %d x %d, got %d x %d" % (TAPS, TAPS, H, W))
    S = 1
    while S < MAX_SCALES and (min(int(H), int(W)) >> S) >= TAPS:
        S += 1
    return S


def check_scales(H, W, scales):
    S = default_scales(H, W) if scales is None else int(scales)
    if not 1 <= S <= MAX_SCALES or (min(int(H), int(W)) >> (S - 1)) < TAPS:
        raise ValueError("scales must be in 1..%d for %d x %d tiles" % (default_scales(H, W), H, W))
    return S


def level_weights(S):
    w = np.array(WEIGHTS[:int(S)], dtype=np.float64)
    return w / w.sum()


def positions(H, W, S):
    """float64 [S]: window positions of the levels"""
    return np.array([((int(H) >> s) - TAPS + 1) * ((int(W) >> s) - TAPS + 1) for s in range(S)], dtype=np.float64)


def finish(comp):
    """[P][S][2] (CS_s, SSIM_s) -> [P] MS-SSIM"""
    comp = np.asarray(comp, dtype=np.float64)
    S = comp.shape[1]
    w = level_weights(S)
    base = np.concatenate([comp[:, :S - 1, 0], comp[:, S - 1:, 1]], axis=1)
    return np.prod(np.maximum(base, 0.0) ** w[None, :], axis=1)


def random_pairs(n, p, seed):
    """(i, j): int64 [p] each, i uniform in [0, n) and j = (i + offset) % n with offset uniform in 1 .. n - 1, so never i == j.
    Drawn from numpy.random.default_rng([seed, 0xD1F5]) alone, pair by pair: a function of (n, seed) whose first p pairs do not depend
    on p, and no global generator is touched."""
    n, p = int(n), int(p)
    if n < 2:
        raise ValueError("a pair needs two tiles, n is %d" % n)
    if p < 0:
        raise ValueError("p must be >= 0")
    rng = np.random.default_rng([int(seed), 0xD1F5])
    draw = rng.integers(np.array([0, 1]), np.array([n, n]), size=(p, 2), dtype=np.int64)
    i = draw[:, 0]
    return i, (i + draw[:, 1]) % n


def _tile_set(x, layout, order, what):
    """(tensor, N, H, W, flags) of a uint8 device tensor or a DeviceTileSet (planar, R G B)"""
    if hasattr(x, "tiles") and not torch.is_tensor(x):
        x, layout, order = x.tiles, "nchw", "rgb"
    N, H, W = tile_args(x, layout, order, what)
    if x.device.type != "cuda":
        raise ValueError("%s runs on the device: the tiles must be on a CUDA device" % what)
    return x.contiguous(), N, H, W, export_flags(layout, order)


def _plan(H, W, S, P):
    lib = _abi.load()
    pyr, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _abi.check(lib.rg_msssim_plan(H, W, S, P, None, ctypes.byref(pyr), ctypes.byref(ws)), "rg_msssim_plan")
    return int(pyr.value), int(ws.value)


def pyramid(tiles, N, H, W, flags, S):
    """levels 1 .. S - 1 of a contiguous tile set as exact block sums (one launch; None for S == 1)"""
    if S == 1 or N == 0:
        return None
    per_tile, _ = _plan(H, W, S, 0)
    pyr = torch.empty(N * per_tile, dtype=torch.uint8, device=tiles.device)
    _abi.launch("rg_msssim_pyramid", tiles.device, tiles.data_ptr(), N, H, W, flags, S, pyr.data_ptr(), N * per_tile)
    return pyr


def pair_sums(a, pyr_a, Na, b, pyr_b, Nb, ia, ib, H, W, flags, S, out=None):
    """rg_msssim_pairs over device index tensors (int32): -> float64 [P][S][3][2] on the device, the sums of cs and l cs"""
    P = int(ia.shape[0])
    if out is None:
        out = torch.empty((P, S, 3, 2), dtype=torch.float64, device=a.device)
    g = (ctypes.c_double * TAPS)(*taps())
    for p0 in range(0, P, PAIR_CHUNK):
        n = min(PAIR_CHUNK, P - p0)
        _, need = _plan(H, W, S, n)
        ws = torch.empty(need, dtype=torch.uint8, device=a.device)
        _abi.launch("rg_msssim_pairs", a.device, a.data_ptr(), None if pyr_a is None else pyr_a.data_ptr(), Na, b.data_ptr(),
                    None if pyr_b is None else pyr_b.data_ptr(), Nb, ia[p0:].data_ptr(), ib[p0:].data_ptr(), n, H, W, flags, S, g,
                    ws.data_ptr(), need, out[p0:].data_ptr())
    return out


def components(a, b=None, pairs=None, scales=None, layout="nhwc", order="rgb"):
    """CS_s and SSIM_s of pairs of tiles -> numpy float64 [P][S][2].

    a, b    uint8 tiles on a CUDA device, (N, H, W, 3) ("nhwc") or (N, 3, H, W) ("nchw"), stored R, G, B ("rgb") or B, G, R ("bgr"),
            or a resident.DeviceTileSet.  b = None: pairs within a.  Both sets have one shape and one layout.
    pairs   (i, j): two integer sequences of P entries, tile i[k] of a against tile j[k] of b, checked here on the host.  None with two
            sets of equal length: row k against row k.
    scales  S (default_scales(H, W) when None)."""
    A, Na, H, W, flags = _tile_set(a, layout, order, "msssim.components")
    if b is None:
        B, Nb = A, Na
    else:
        B, Nb, Hb, Wb, fb = _tile_set(b, layout, order, "msssim.components")
        if (Hb, Wb, fb) != (H, W, flags) or B.device != A.device:
            raise ValueError("both tile sets need one shape, one layout and one device")
    if min(H, W) < TAPS:
        raise ValueError("MS-SSIM needs tiles of at least %d x %d, got %d x %d" % (TAPS, TAPS, H, W))
    S = check_scales(H, W, scales)
    if pairs is None:
        if b is None or Na != Nb:
            raise ValueError("pairs=None needs two sets of equal length (row k against row k)")
        i = j = np.arange(Na, dtype=np.int64)
    else:
        i, j = (np.asarray(v) for v in pairs)
        if i.ndim != 1 or i.shape != j.shape or (i.size and not (np.issubdtype(i.dtype, np.integer) and np.issubdtype(j.dtype, np.integer))):
            raise ValueError("pairs is two integer sequences of equal length")
        i, j = i.astype(np.int64), j.astype(np.int64)
        if i.size and (i.min() < 0 or i.max() >= Na or j.min() < 0 or j.max() >= Nb):
            raise ValueError("a pair points outside its tile set (%d and %d tiles)" % (Na, Nb))
    P = int(i.shape[0])
    if P == 0:
        return np.zeros((0, S, 2), dtype=np.float64)
    pyr_a = pyramid(A, Na, H, W, flags, S)
    pyr_b = pyr_a if B is A else pyramid(B, Nb, H, W, flags, S)
    ia = torch.from_numpy(i.astype(np.int32)).to(A.device)
    ib = torch.from_numpy(j.astype(np.int32)).to(A.device)
    sums = pair_sums(A, pyr_a, Na, B, pyr_b, Nb, ia, ib, H, W, flags, S).cpu().numpy()        # the one download: P S 6 doubles
    return sums.mean(axis=2) / positions(H, W, S)[None, :, None]


def ms_ssim(a, b=None, pairs=None, scales=None, layout="nhwc", order="rgb"):
    """the MS-SSIM of every pair -> numpy float64 [P] (arguments: ``components``)"""
    return finish(components(a, b, pairs, scales, layout, order))


def ssim(a, b=None, pairs=None, layout="nhwc", order="rgb"):
    """plain SSIM: ``ms_ssim`` at S = 1"""
    return ms_ssim(a, b, pairs, 1, layout, order)


def diversity_of(comp):
    """[P][S][2] -> {"mean", "std" (of the per-pair MS-SSIM, population), "per_scale" ([S][2]: the means of CS_s and SSIM_s)}"""
    score = finish(comp)
    return {"mean": float(score.mean()), "std": float(score.std()), "per_scale": np.asarray(comp).mean(axis=0).tolist()}


def pair_diversity(tiles, n_pairs, seed=0, scales=None, layout="nhwc", order="rgb"):
    """The mean MS-SSIM over ``random_pairs(len(tiles), n_pairs, seed)`` of one tile set (``diversity_of``): near 1 for a set of
    near-copies, lower for a diverse set; to be read next to the same figure over real tiles."""
    n = len(tiles) if not torch.is_tensor(tiles) else tiles.shape[0]
    if int(n_pairs) < 1:
        raise ValueError("n_pairs must be >= 1")
    return diversity_of(components(tiles, None, random_pairs(n, n_pairs, seed), scales, layout, order))
