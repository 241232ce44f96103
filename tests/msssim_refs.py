"""A plain fp64 numpy restatement of the MS-SSIM definition of include/rnagan_hip.h (rna_gan_amd.msssim, rg_msssim.hip), written
without looking at either: the window, the pyramid, the five windowed moments, the two ratios, the means and the final product.
tests/test_msssim_refs_cpu.py pins it against exact rationals, scipy's filter and closed forms; the GPU tests compare with it.

Tiles here are uint8 (H, W, 3) arrays in R, G, B order."""
from fractions import Fraction

import numpy as np

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SDS = (4, 16, 48)
# the shapes on which the correlated inputs are checked to keep every CS at or above CS_FLOOR
CORRELATED_SHAPES = ((11, 11), (12, 13), (22, 22), (23, 25), (45, 47), (176, 176), (177, 191), (256, 256))
CS_FLOOR = 0.05


def taps():
    d = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(d * d) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def default_scales(H, W):
    S = 1
    while S < 5 and (min(H, W) >> S) >= 11:
        S += 1
    return S


def weights(S):
    w = np.array(WEIGHTS[:S], dtype=np.float64)
    return w / w.sum()


def pyramid(x, S):
    """the S levels of one tile as float64 (h_s, w_s, 3): the 2 x 2 mean of the level before, a last odd row or column dropped.
    Exact in fp64: a level-s pixel is an integer below 2^16 divided by 4^s."""
    levels = [np.asarray(x, dtype=np.float64)]
    for _ in range(1, S):
        p = levels[-1]
        h, w = p.shape[0] // 2, p.shape[1] // 2
        p = p[:2 * h, :2 * w]
        levels.append((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0)
    return levels


def window(a):
    """the 11-tap window along axes 0 and 1 with valid extent: (h, w, ...) -> (h - 10, w - 10, ...)"""
    g = taps()
    h, w = a.shape[0], a.shape[1]
    rows = sum(g[j] * a[:, j:j + w - 10] for j in range(11))
    return sum(g[j] * rows[j:j + h - 10] for j in range(11))


def level_maps(x, y):
    """(cs, l) maps of one level: float64 (h - 10, w - 10, 3) each"""
    mx, my = window(x), window(y)
    vx, vy, cxy = window(x * x) - mx * mx, window(y * y) - my * my, window(x * y) - mx * my
    return (2.0 * cxy + C2) / (vx + vy + C2), (2.0 * mx * my + C1) / (mx * mx + my * my + C1)


def components(x, y, S=None):
    """float64 [S][2]: (CS_s, SSIM_s), means over the window positions, then over the channels"""
    S = default_scales(x.shape[0], x.shape[1]) if S is None else S
    out = np.empty((S, 2), dtype=np.float64)
    for s, (px, py) in enumerate(zip(pyramid(x, S), pyramid(y, S))):
        cs, l = level_maps(px, py)
        out[s, 0] = cs.mean(axis=(0, 1)).mean()
        out[s, 1] = (l * cs).mean(axis=(0, 1)).mean()
    return out


def finish(comp):
    comp = np.asarray(comp, dtype=np.float64)
    S = comp.shape[0]
    base = np.concatenate([comp[:S - 1, 0], comp[S - 1:, 1]])
    return float(np.prod(np.maximum(base, 0.0) ** weights(S)))


def ms_ssim(x, y, S=None):
    return finish(components(x, y, S))


def batch_components(a, b, pairs, S=None):
    """[P][S][2] over tile sets (N, H, W, 3)"""
    return np.stack([components(a[i], b[j], S) for i, j in zip(*pairs)])


# ------------------------------------------------------------------ exact rationals, not separable
def components_exact(x, y, S):
    """the same numbers in exact rationals by brute force over the 11 x 11 window (no separable pass); the taps are the fp64 taps taken
    as the rationals they are.  For small tiles only."""
    g = [Fraction(float(v)) for v in taps()]
    w2 = [[g[i] * g[j] for j in range(11)] for i in range(11)]
    c1, c2 = Fraction(C1), Fraction(C2)
    out = []
    lx = [[[Fraction(int(v)) for v in row] for row in np.asarray(x)[:, :, c]] for c in range(3)]
    ly = [[[Fraction(int(v)) for v in row] for row in np.asarray(y)[:, :, c]] for c in range(3)]
    for s in range(S):
        if s:
            lx = [_halve(p) for p in lx]
            ly = [_halve(p) for p in ly]
        cs_c, ss_c = [], []
        for px, py in zip(lx, ly):
            h, w = len(px), len(px[0])
            cs_sum = ss_sum = Fraction(0)
            for r in range(h - 10):
                for c in range(w - 10):
                    mx = my = exx = eyy = exy = Fraction(0)
                    for i in range(11):
                        for j in range(11):
                            k, a, b = w2[i][j], px[r + i][c + j], py[r + i][c + j]
                            mx += k * a
                            my += k * b
                            exx += k * a * a
                            eyy += k * b * b
                            exy += k * a * b
                    cs = (2 * (exy - mx * my) + c2) / ((exx - mx * mx) + (eyy - my * my) + c2)
                    l = (2 * mx * my + c1) / (mx * mx + my * my + c1)
                    cs_sum += cs
                    ss_sum += l * cs
            n = (h - 10) * (w - 10)
            cs_c.append(cs_sum / n)
            ss_c.append(ss_sum / n)
        out.append((float(sum(cs_c) / 3), float(sum(ss_c) / 3)))
    return np.array(out, dtype=np.float64)


def _halve(p):
    h, w = len(p) // 2, len(p[0]) // 2
    return [[(p[2 * r][2 * c] + p[2 * r][2 * c + 1] + p[2 * r + 1][2 * c] + p[2 * r + 1][2 * c + 1]) / 4 for c in range(w)] for r in range(h)]


# ------------------------------------------------------------------ inputs
def random_tiles(n, H, W, seed):
    return np.random.default_rng([seed, n, H, W]).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def two_scale_tile(H, W, seed):
    """one random tile with variance at every level of the pyramid: half fine uniform noise, half uniform noise that is constant
    over 16 x 16 blocks.  Against its complement 255 - x every CS is negative.  (White noise alone does not do that: 2^s x 2^s means
    shrink its variance by 4^s, below C2 / 2 at the deep levels, where CS of tile and complement turns positive.)"""
    rng = np.random.default_rng([seed, H, W, 3])
    fine = rng.integers(0, 256, size=(H, W, 3))
    coarse = rng.integers(0, 256, size=((H + 15) // 16, (W + 15) // 16, 3)).repeat(16, axis=0).repeat(16, axis=1)[:H, :W]
    return (fine // 2 + coarse // 2).astype(np.uint8)


def smooth_tiles(n, H, W, seed):
    """n seeded tiles: a smooth field (a few low-frequency waves per channel) plus N(0, 30) noise, clipped and rounded"""
    rng = np.random.default_rng([seed, n, H, W, 1])
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((n, H, W, 3), dtype=np.float64)
    for k in range(n):
        for c in range(3):
            f = np.full((H, W), 128.0)
            for _ in range(3):
                fy, fx = rng.uniform(0.5, 3.0, size=2) * 2.0 * np.pi / 256.0
                f += 25.0 * np.sin(fy * yy + fx * xx + rng.uniform(0.0, 2.0 * np.pi))
            out[k, :, :, c] = f
    out += rng.normal(0.0, 30.0, size=out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def correlated_sets(n, H, W, sd, seed=0):
    """(a, b): b[k] is a[k] plus N(0, sd) noise, clipped and rounded -- pairs whose every CS stays well above the clamp"""
    a = smooth_tiles(n, H, W, seed)
    rng = np.random.default_rng([seed, n, H, W, sd, 2])
    b = np.clip(np.rint(a.astype(np.float64) + rng.normal(0.0, float(sd), size=a.shape)), 0, 255).astype(np.uint8)
    return a, b


def stored(rgb, layout, order):
    """(N, H, W, 3) R G B -> the contiguous array a tile store of that layout and channel order holds"""
    a = rgb[..., ::-1] if order == "bgr" else rgb
    if layout == "nchw":
        a = a.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(a)
