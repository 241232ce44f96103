"""numpy restatements of the optimizer-step kernels (include/rnagan_hip.h: rg_adam_step, rg_adam_step_dev, rg_adam_step_slabs,
rg_grad_to_wire, rg_adam_hyper_dev*), shared by tests/test_adam_refs_cpu.py (which pins them without a GPU) and
tests/test_adam_ops_gpu.py (which compares the kernels with them bit for bit).

The library is built with -ffp-contract=off and fp32 denormals kept, sqrtf and the division are the correctly rounded IEEE
sequences: every operation of rg_adam_upd (rna_gan_amd/csrc/rg_common.h) is ONE correctly rounded fp32 operation, and numpy's
float32 arithmetic, which rounds every operation separately too, reproduces it BIT FOR BIT for every finite input whose results
are finite (the bit pattern of a NaN is not specified).  The 16-bit conversions are the compiler's casts: round to nearest even.
No torch on the computing path."""
import math

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24                                   # fp32's unit round-off


def adam_hyper_ref(step, lr, b1, b2, eps, wd=0.0, ginv=1.0, skip=0):
    """The 12 floats of the hyper buffer at the 1-based `step`: the constants are formed in Python doubles exactly as
    adam_hyper_advance (rg_misc.hip) forms them in C doubles, each rounded to fp32 once."""
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    return np.array([b1, b2, 1.0 - b1, 1.0 - b2, eps, lr / bc1, 1.0 / math.sqrt(bc2), wd, ginv, float(skip), 0.0, 0.0],
                    dtype=np.float64).astype(np.float32)


def adam_upd_ref(p, g, m, v, hyper):
    """rg_adam_upd behind the g * ginv of Adam::upd, one float32 operation per line.  Returns new (p, m, v); the inputs are not
    modified.  hyper[9] (the skip word) is the kernels' business, not the expression's: it is not looked at here."""
    p, g, m, v = (np.array(a, dtype=np.float32) for a in (p, g, m, v))
    h = np.asarray(hyper, dtype=np.float32)
    b2, omb1, omb2, eps, ss, isb, wd, ginv = h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]
    with np.errstate(all="ignore"):
        g = g * ginv
        if wd != 0:
            t = wd * p
            g = g + t
        t = g - m
        t = omb1 * t
        m = m + t
        a = b2 * v
        t = omb2 * g
        t = t * g
        v = a + t
        d = np.sqrt(v)
        d = d * isb
        d = d + eps
        q = m / d
        q = ss * q
        p = p - q
    for x in (g, t, a, d, q, p, m, v):
        assert x.dtype == np.float32
    return p, m, v


def round_h16_ref(x, half):
    """fp32 -> the bits (uint16) of the nearest bf16 / fp16 value, ties to even.  Overflow gives infinity (fp16: from 65520 on),
    fp16 denormals are kept, a NaN stays a (quiet) NaN with its sign."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if half == "f16":
        with np.errstate(all="ignore"):
            return x.astype(np.float16).view(np.uint16)            # numpy's conversion is IEEE round-to-nearest-even
    assert half == "bf16"
    b = x.view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def widen_h16_ref(bits, half):
    """bf16 / fp16 bits (uint16) -> fp32, exact."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if half == "f16":
        return bits.view(np.float16).astype(np.float32)
    assert half == "bf16"
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def slab_lanes(nsplit):
    """threads per 16-byte column in adam_slab_segment / wire_slab_segment"""
    return 1 if nsplit <= 4 else 4 if nsplit <= 32 else 16


def slab_sum_ref(slabs, nsplit):
    """The kernels' summation order over float32 slabs [nsplit][n] (already widened if 16-bit): lane l starts from +0.0f and
    adds slabs l, l + SL, ... in that order (the 8-deep unrolled loop adds in the same order), then the lanes are combined as
    ((lane0 + lane1) + lane2) + ..."""
    slabs = np.asarray(slabs, dtype=np.float32)
    assert slabs.ndim == 2 and slabs.shape[0] == nsplit and nsplit >= 1
    SL = slab_lanes(nsplit)
    lanes = []
    with np.errstate(all="ignore"):
        for l in range(SL):
            s = np.zeros(slabs.shape[1], dtype=np.float32)
            for z in range(l, nsplit, SL):
                s = s + slabs[z]
            lanes.append(s)
        tot = lanes[0]
        for k in range(1, SL):
            tot = tot + lanes[k]
    assert tot.dtype == np.float32
    return tot


# A segment table is a list of (off, n, slabs, nsplit):
#   plain    slabs = None, nsplit = 0:   the gradient is g[off : off + n]
#   slab     slabs = float32 [nsplit][n], or uint16 [nsplit][n] (the bits of the build's 16-bit type): g is not read
#   skipped  slabs = None, nsplit = -1:  nothing of the segment is read or written
def _segment_gradient(g, seg, half):
    off, n, slabs, nsplit = seg
    if slabs is None:
        return np.asarray(g[off:off + n], dtype=np.float32)
    slabs = np.asarray(slabs)
    assert slabs.shape == (nsplit, n)
    return slab_sum_ref(widen_h16_ref(slabs, half) if slabs.dtype == np.uint16 else slabs, nsplit)


def adam_table_ref(p, g, m, v, hyper, table, half, shadow=None):
    """rg_adam_step_slabs: returns new (p, m, v, shadow bits).  `shadow` = the bits before the call (zeros by default); a skipped
    segment keeps them, as it keeps p, m and v."""
    p, m, v = (np.array(a, dtype=np.float32) for a in (p, m, v))
    sh = np.zeros(p.size, dtype=np.uint16) if shadow is None else np.array(shadow, dtype=np.uint16)
    for seg in table:
        off, n, slabs, nsplit = seg
        if slabs is None and nsplit < 0:
            continue
        s = slice(off, off + n)
        p[s], m[s], v[s] = adam_upd_ref(p[s], _segment_gradient(g, seg, half), m[s], v[s], hyper)
        sh[s] = round_h16_ref(p[s], half)
    return p, m, v, sh


def wire_table_ref(g, table, half, wire=None):
    """rg_grad_to_wire: the wire's bits (uint16): one rounding of the fp32 gradient or slab sum; a skipped segment keeps `wire`."""
    total = sum(seg[1] for seg in table)
    w = np.zeros(total, dtype=np.uint16) if wire is None else np.array(wire, dtype=np.uint16)
    for seg in table:
        off, n, slabs, nsplit = seg
        if slabs is None and nsplit < 0:
            continue
        w[off:off + n] = round_h16_ref(_segment_gradient(g, seg, half), half)
    return w


# ---------------------------------------------------------------------------- the inputs of the GPU tests (pinned on the CPU)
HYPER = dict(lr=4e-4, b1=0.5, b2=0.999, eps=1e-8)
SLAB_NSPLITS = [1, 3, 4, 5, 8, 28, 29, 32, 33, 64, 127, 128, 129, 200]


def slab_inputs(nsplit, n, seed=0):
    """fp32 slabs [nsplit][n]: standard normal times 2^k, k uniform in -6 .. 6.  The spread of magnitudes makes the sum depend on
    the order in which it is taken (tests/test_adam_refs_cpu.py asserts by how much)."""
    rng = np.random.default_rng(7000 + 13 * nsplit + seed)
    k = rng.integers(-6, 7, size=(nsplit, n))
    return (rng.standard_normal((nsplit, n)) * np.exp2(k)).astype(np.float32)


def slab_inputs_h16(nsplit, n, half, seed=0):
    """the same values rounded to the build's 16-bit type, as bits (uint16)"""
    return round_h16_ref(slab_inputs(nsplit, n, seed), half)


def normal_inputs(n, later, seed=0):
    """(p, g, m, v): a first step (m = v = 0) or a later one (random m, v >= 0)"""
    rng = np.random.default_rng(100 + n % 997 + seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    if later:
        m = (rng.standard_normal(n) * 0.01).astype(np.float32)
        v = (rng.random(n) * 1e-4).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, g, m, v


def special_inputs(n, wd=0.0):
    """(p, g, m, v) tiled to n: g = 0 with v = 0 (denom = eps); +-0 everywhere; fp32 denormals in g, m and v and a g whose square
    underflows; a large g whose square stays finite; p at +-3e38 stepping away from overflow.  With weight decay the last pair is
    p = +-1e17 instead: wd * 3e38 squared leaves fp32's range, and the reference must stay finite."""
    big = 3e38 if wd == 0.0 else 1e17
    p = np.array([1.0, 0.0, -0.0, -0.0, 0.5, -0.25, 1e-40, 2.0, 1.0, -1.0, big, -big, 0.0, 1e-38, -1e-45, 3.0], dtype=np.float32)
    g = np.array([0.0, 0.0, -0.0, 0.0, 1e-40, -1e-45, 1e-30, -1e-30, 1e18, -1e18, 1.0, -1.0, 1e-45, -1e-38, 1e-20, 0.0], dtype=np.float32)
    m = np.array([0.0, 0.0, -0.0, -0.0, 1e-41, 1e-45, 0.0, -1e-39, 0.0, 1e10, 1.0, -1.0, -1e-45, 1e-38, 0.0, 1e-42], dtype=np.float32)
    v = np.array([0.0, 0.0, -0.0, 0.0, 1e-42, 1e-45, 0.0, 1e-44, 0.0, 1e30, 1.0, 1.0, 1e-45, 0.0, 1e-39, 1e-38], dtype=np.float32)
    reps = -(-n // p.size)
    return tuple(np.tile(a, reps)[:n].copy() for a in (p, g, m, v))
