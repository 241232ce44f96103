"""numpy restatement of the stain-normalisation contract (include/rnagan_hip.h: rg_stain_moments, rg_stain_angle_hist,
rg_stain_conc_hist, rg_stain_apply), the fp64 textbook form of Macenko's method it is measured against, and the synthetic
Beer-Lambert sets the stain test files share.

The restatement is written from the contract, in its most literal form (the angle bin is the COUNT of the predicate over the whole
direction table, not a search; tables are rebuilt with the math module), and shares no arithmetic with rna_gan_amd.stain.
"""
import math

import numpy as np

IO, BETA, ALPHA = 240, 0.15, 1
QOD, QV, K, QP, CB, CSH, QS, QH, QO = 12, 14, 1024, 20, 4096, 3, 16, 14, 8
SHIFT = QH + QOD - QO
# The gate on the largest byte difference between the integer form and the fp64 textbook form: the largest difference measured over
# 40 unselected synthetic sets (seeds 0..19 x two source stain matrices: 2, profiles/stain_textbook_agreement.txt) plus one byte --
# the fit's histogram bins move the scale by a fraction of a percent.
TEXTBOOK_MEASURED = 2
TEXTBOOK_GATE = TEXTBOOK_MEASURED + 1
AGREEMENT_SEEDS = tuple(range(20))


def rint(x):
    return int(np.rint(np.float64(x)))


# ------------------------------------------------------------------ tables
def od_lut():
    return np.array([rint(-math.log((v + 1) / IO) * 2 ** QOD) for v in range(256)], dtype=np.int32)


BETA_Q = rint(BETA * 2 ** QOD)


def dirs(k=K):
    out = []
    for j in range(1, k):
        th = -math.pi / 2 + j * math.pi / k
        out.append((rint(math.cos(th) * 2 ** QV), rint(math.sin(th) * 2 ** QV)))
    return np.array(out, dtype=np.int32).reshape(k - 1, 2)


def _out(j, off):
    return min(255, max(0, rint(IO * math.exp(-(j - off) / 2 ** QO))))


def out_lut():
    off = 0
    while _out(0, off) != 255:
        off += 1
    table = [_out(0, off)]
    while table[-1] != 0:
        table.append(_out(len(table), off))
    return np.array(table, dtype=np.uint8), off


# ------------------------------------------------------------------ pixels
def rgb_of(tiles, layout, order):
    """numpy uint8 tiles in the stored layout / order -> (pixels, 3) R, G, B"""
    a = np.asarray(tiles)
    if layout == "nchw":
        a = a.transpose(0, 2, 3, 1)
    if order == "bgr":
        a = a[..., ::-1]
    return a.reshape(-1, 3)


def store_as(rgb_nhwc, layout, order):
    """the inverse: (N, H, W, 3) R, G, B -> contiguous array in the stored layout / order"""
    a = rgb_nhwc[..., ::-1] if order == "bgr" else rgb_nhwc
    if layout == "nchw":
        a = a.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(a)


def od_of(rgb, lut=None):
    return (od_lut() if lut is None else lut).astype(np.int64)[rgb]


def stained(od, beta_q=BETA_Q):
    return (od >= beta_q).all(axis=1)


# ------------------------------------------------------------------ the four passes
def moments(rgb, lut=None, beta_q=BETA_Q):
    od = od_of(rgb, lut)
    od = od[stained(od, beta_q)]
    out = [od.shape[0], od[:, 0].sum(), od[:, 1].sum(), od[:, 2].sum()]
    for c, d in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append((od[:, c] * od[:, d]).sum())
    return np.array(out, dtype=np.int64)


def angle_bin_count(p1, p2, d):
    """the contract's bin: #{k : cos_k p2 - sin_k p1 >= 0}, evaluated for every k"""
    p1, p2 = np.asarray(p1, dtype=np.int64), np.asarray(p2, dtype=np.int64)
    out = np.empty(p1.shape[0], dtype=np.int64)
    c, s = d[:, 0].astype(np.int64), d[:, 1].astype(np.int64)
    for a in range(0, p1.shape[0], 4096):
        out[a:a + 4096] = (c[None, :] * p2[a:a + 4096, None] - s[None, :] * p1[a:a + 4096, None] >= 0).sum(axis=1)
    return out


def angle_bin_search(p1, p2, d):
    """the same count by binary search, one pixel at a time (what the kernel does)"""
    k = d.shape[0] + 1
    lo, hi = 0, k - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if int(d[mid - 1, 0]) * int(p2) - int(d[mid - 1, 1]) * int(p1) >= 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def angle_hist(rgb, basis6, d=None, lut=None, beta_q=BETA_Q):
    d = dirs() if d is None else d
    k = d.shape[0] + 1
    od = od_of(rgb, lut)
    od = od[stained(od, beta_q)]
    b = np.array(basis6, dtype=np.int64)
    p1, p2 = od @ b[:3], od @ b[3:]
    hist = np.zeros(k + 1, dtype=np.int64)
    hist[k] = (p1 <= 0).sum()
    hist[:k] = np.bincount(angle_bin_count(p1[p1 > 0], p2[p1 > 0], d), minlength=k)
    return hist


def conc_of(od, pinv6, qp=QP):
    return (od @ np.array(pinv6, dtype=np.int64).reshape(2, 3).T) >> qp


def conc_hist(rgb, pinv6, qp=QP, csh=CSH, bins=CB, lut=None):
    b = np.clip(conc_of(od_of(rgb, lut), pinv6, qp) >> csh, 0, bins - 1)
    return np.stack([np.bincount(b[:, s], minlength=bins) for s in range(2)]).astype(np.int64)


def apply(rgb, pinv6, scale2, href6, qp=QP, qs=QS, shift=SHIFT, table=None, off=None, lut=None):
    """(pixels, 3) R, G, B -> (pixels, 3) R, G, B"""
    if table is None:
        table, off = out_lut()
    conc2 = (conc_of(od_of(rgb, lut), pinv6, qp) * np.array(scale2, dtype=np.int64)) >> qs
    od2 = (conc2 @ np.array(href6, dtype=np.int64).reshape(3, 2).T + ((1 << (shift - 1)) if shift > 0 else 0)) >> shift
    return table[np.clip(od2 + off, 0, len(table) - 1)]


# ------------------------------------------------------------------ the host arithmetic
def percentile_bin(hist, q):
    total = int(np.sum(hist))
    rank = (q * (total - 1)) // 100
    return int(np.searchsorted(np.cumsum(np.asarray(hist, dtype=np.int64)), rank, side="right"))


def basis(m):
    n = int(m[0])
    s1 = [int(v) for v in m[1:4]]
    s2 = [int(v) for v in m[4:10]]
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    cov = np.zeros((3, 3))
    for (c, d), i in idx.items():
        cov[c, d] = cov[d, c] = float(n * s2[i] - s1[c] * s1[d]) / float(n * (n - 1)) / float(2 ** (2 * QOD))
    _, v = np.linalg.eigh(cov)
    e1, e2 = v[:, 2], v[:, 1]
    return (-e1 if e1.sum() < 0 else e1), (-e2 if e2.sum() < 0 else e2)


def fit(rgb):
    """(pixels, 3) -> dict with every intermediate of the contract's fit"""
    m = moments(rgb)
    e1, e2 = basis(m)
    basis6 = [rint(x * 2 ** QV) for x in list(e1) + list(e2)]
    ah = angle_hist(rgb, basis6)
    cols = []
    for q in (ALPHA, 100 - ALPHA):
        phi = -math.pi / 2 + (percentile_bin(ah[:K], q) + 0.5) * math.pi / K
        cols.append(e1 * math.cos(phi) + e2 * math.sin(phi))
    if cols[0][0] < cols[1][0]:
        cols.reverse()
    he = np.stack(cols, axis=1)
    pinv6 = [rint(x) for x in (np.linalg.pinv(he) * 2 ** QP).reshape(-1)]
    ch = conc_hist(rgb, pinv6)
    max_conc = np.array([(percentile_bin(ch[s], 99) + 0.5) * 2 ** CSH / 2 ** QOD for s in range(2)])
    return {"moments": m, "basis6": basis6, "angle_hist": ah, "he": he, "pinv6": pinv6, "conc_hist": ch, "max_conc": max_conc,
            "n_stained": int(m[0]), "n_outside": int(ah[K])}


def operands(he, max_conc, he_t, max_t):
    pinv6 = [rint(x) for x in (np.linalg.pinv(np.asarray(he)) * 2 ** QP).reshape(-1)]
    scale2 = [rint(x) for x in np.asarray(max_t) / np.asarray(max_conc) * 2 ** QS]
    href6 = [rint(x) for x in (np.asarray(he_t) * 2 ** QH).reshape(-1)]
    return pinv6, scale2, href6


# ------------------------------------------------------------------ the fp64 textbook form
def textbook_fit(rgb):
    """Macenko et al. (2009) as the method's reference implementation computes it, in fp64: OD = -ln((I + 1) / Io); the pixels with
    every OD >= beta; eigh of their covariance; the angle atan2(p2, p1) in the plane of the two leading eigenvectors (each signed to
    a non-negative component sum, p1 on the leading one); its alpha-th and (100 - alpha)-th numpy percentile; the vector with the
    larger R component first; least-squares concentrations of ALL pixels; their 99th percentiles.  -> (HE, max_conc)"""
    od = -np.log((rgb.astype(np.float64) + 1.0) / IO)
    odh = od[(od >= BETA).all(axis=1)]
    _, v = np.linalg.eigh(np.cov(odh.T))
    e1, e2 = v[:, 2], v[:, 1]
    e1 = -e1 if e1.sum() < 0 else e1
    e2 = -e2 if e2.sum() < 0 else e2
    phi = np.arctan2(odh @ e2, odh @ e1)
    cols = [e1 * np.cos(p) + e2 * np.sin(p) for p in (np.percentile(phi, ALPHA), np.percentile(phi, 100 - ALPHA))]
    if cols[0][0] < cols[1][0]:
        cols.reverse()
    he = np.stack(cols, axis=1)
    conc = np.linalg.lstsq(he, od.T, rcond=None)[0]
    return he, np.percentile(conc, 99, axis=1)


def textbook_apply(rgb, he, max_conc, he_t, max_t):
    """the bytes: Io exp(-HE_t (C max_t / max_conc)), rounded to nearest and clipped to 0..255 (the reference implementation
    truncates and maps values above 255 to 254; the contract's output table rounds, and so does this form)"""
    od = -np.log((rgb.astype(np.float64) + 1.0) / IO)
    conc = np.linalg.lstsq(np.asarray(he), od.T, rcond=None)[0]
    conc2 = conc * (np.asarray(max_t) / np.asarray(max_conc))[:, None]
    return np.clip(np.rint(IO * np.exp(-(np.asarray(he_t) @ conc2))), 0, 255).astype(np.uint8).T


# ------------------------------------------------------------------ synthetic Beer-Lambert sets
SOURCE_STAINS = (
    ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11)),            # Ruifrok & Johnston's H and E
    ((0.55, 0.76, 0.35), (0.21, 0.91, 0.36)),            # a bluer haematoxylin, a redder eosin
)


def synthetic_set(seed, stains=0, n=8, size=64, noise=1.5, background=0.25, shape=None, strength=1.0):
    """(n, size, size, 3) uint8 R, G, B: I = Io exp(-HE C) + N(0, noise), C gamma-distributed per stain, a `background` share of
    the pixels with C = 0"""
    rng = np.random.default_rng(seed)
    he = np.array(SOURCE_STAINS[stains], dtype=np.float64).T
    he = he / np.linalg.norm(he, axis=0)
    shape = (n, size, size) if shape is None else tuple(shape)
    px = int(np.prod(shape))
    conc = strength * np.stack([rng.gamma(2.0, 0.45, px), rng.gamma(2.0, 0.3, px)], axis=1)
    conc[rng.random(px) < background] = 0.0
    img = IO * np.exp(-(conc @ he.T))
    if noise:
        img = img + rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(shape + (3,))
