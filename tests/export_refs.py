"""numpy restatement of rg_tile_export_u8's contract (include/rnagan_hip.h), shared by the export test files.

Every step is an explicit fp32 operation (numpy rounds each float32 operation separately: no contraction, a true division); the
clamp is written as the contract's comparisons; the layouts and the channel reversal are index expressions."""
import numpy as np

F32 = np.float32
PLANAR, REVERSE, TRUNC = 1, 2, 4


def denominator(lo, hi):
    """max(hi - lo, 1e-5) as torch computes it from Python scalars: in double, rounded once to fp32."""
    return F32(max(float(hi) - float(lo), 1e-5))


def export_value_ref(x, sub=-1.0, div=2.0):
    """v = (x - sub) / div: two fp32 operations."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        return ((x - F32(sub)).astype(F32) / F32(div)).astype(F32)


def export_byte_ref(x, sub=-1.0, div=2.0, rounding="round"):
    """The byte of every element of x, same shape."""
    v = export_value_ref(x, sub, div)
    with np.errstate(all="ignore"):
        t = (v * F32(255.0)).astype(F32)
        if rounding == "round":
            t = (t + F32(0.5)).astype(F32)
        elif rounding != "trunc":
            raise ValueError(rounding)
        ge0 = t >= F32(0.0)                       # False for NaN; -0.0 >= 0 is True and truncates to 0 as well
        ge255 = t >= F32(255.0)
        inner = np.where(ge0 & ~ge255, t, F32(0.0)).astype(F32)
        b = np.trunc(inner).astype(np.uint8)      # 0 <= inner < 255: truncation toward zero
    return np.where(ge255, np.uint8(255), np.where(ge0, b, np.uint8(0))).astype(np.uint8)


def tile_export_ref(x, layout="nhwc", order="rgb", rounding="round", sub=-1.0, div=2.0):
    """x [N][C][H][W] fp32 -> uint8 [N][H][W][C] (layout "nhwc") or [N][C][H][W] ("nchw"); order "bgr": destination channel c
    takes source channel C - 1 - c."""
    x = np.asarray(x, dtype=F32)
    N, C, H, W = x.shape
    b = export_byte_ref(x, sub, div, rounding)
    src_c = [C - 1 - c for c in range(C)] if order == "bgr" else list(range(C))
    if order not in ("rgb", "bgr"):
        raise ValueError(order)
    if layout == "nchw":
        out = np.empty((N, C, H, W), dtype=np.uint8)
        for c in range(C):
            out[:, c, :, :] = b[:, src_c[c], :, :]
    elif layout == "nhwc":
        out = np.empty((N, H, W, C), dtype=np.uint8)
        for c in range(C):
            out[:, :, :, c] = b[:, src_c[c], :, :]
    else:
        raise ValueError(layout)
    return out


def flags_of(layout, order, rounding):
    return (PLANAR if layout == "nchw" else 0) | (REVERSE if order == "bgr" else 0) | (TRUNC if rounding == "trunc" else 0)


def host_transform(b):
    """((b / 255 - 0.5) / 0.5): the three fp32 operations of the input transform (rg_u8_to_norm, ToTensor + Normalize)."""
    b = np.asarray(b, dtype=np.uint8)
    return (((b.astype(F32) / F32(255.0)).astype(F32) - F32(0.5)).astype(F32) / F32(0.5)).astype(F32)


# the bytes that the truncating rule returns one lower after the host transform: 63 of the 256 (checked exhaustively by
# tests/test_export_refs_cpu.py; the rounding rule returns all 256 unchanged)
TRUNC_ONE_LOWER = tuple(range(1, 64))


def neighbours(v, k=2):
    """v and its +-1 .. +-k ulp neighbours (fp32)."""
    v = np.asarray(v, dtype=F32).reshape(-1)
    out = [v]
    up, dn = v, v
    for _ in range(k):
        up = np.nextafter(up, F32(np.inf)).astype(F32)
        dn = np.nextafter(dn, F32(-np.inf)).astype(F32)
        out += [up, dn]
    return np.concatenate(out)


def edge_values():
    """Per byte k: the transform value, the rounding threshold 2 (k + 1/2) / 255 - 1 and the truncation threshold 2 k / 255 - 1,
    each with its +-1 and +-2 ulp neighbours; then the specials."""
    k = np.arange(256, dtype=np.float64)
    parts = [neighbours(host_transform(np.arange(256, dtype=np.uint8))),
             neighbours((2.0 * (k + 0.5) / 255.0 - 1.0).astype(F32)),
             neighbours((2.0 * k / 255.0 - 1.0).astype(F32)),
             np.array([-1.5, 1.5, np.inf, -np.inf, np.nan, 0.0, -0.0, -1.0, 1.0], dtype=F32)]
    return np.concatenate(parts).astype(F32)
