"""numpy reference of rg_ema_update (include/rnagan_hip.h), shared by tests/test_ema_refs_cpu.py, tests/test_ema_ops_gpu.py and
tests/test_ema_train_gpu.py.

The kernel computes, per element and in fp32,
    omd = 1.f - d;   e <- e + omd * (p - e)
as three separately rounded IEEE operations in that order (the library is built with -ffp-contract=off, fp32 denormals kept),
with d = decay, or d = fminf(decay, (1.f + (float)t) / (10.f + (float)t)) when the warm-up reads Adam's step counter t
(correctly rounded division).  numpy's float32 arithmetic rounds every operation separately too, so the functions below
reproduce the kernel BIT FOR BIT for every finite input whose result is finite (the bit pattern of a NaN is not specified).
One consequence of the formula worth knowing: e == p leaves e unchanged bit for bit, except e = p = -0.0, which becomes +0.0
((-0) - (-0) = +0, (-0) + (+0) = +0).
"""
import numpy as np

F32 = np.float32
U32 = 2.0 ** -24                                   # fp32's unit round-off


def decay_at(decay, t=None):
    """The decay the kernel uses at Adam step t (1-based, read after the step's hyper launch); t=None: no warm-up."""
    d = F32(decay)
    if t is None:
        return d
    tf = F32(np.int32(t))                          # (float)t of an int32: round to nearest even
    return np.minimum(d, (F32(1.0) + tf) / (F32(10.0) + tf)).astype(np.float32)


def ema_update_ref(p, e, decay, t=None):
    """One rg_ema_update on numpy float32 arrays: returns the new e (p and e are not modified)."""
    p = np.asarray(p, dtype=np.float32)
    e = np.asarray(e, dtype=np.float32)
    omd = F32(1.0) - decay_at(decay, t)
    diff = p - e
    prod = omd * diff
    out = e + prod
    assert out.dtype == np.float32
    return out


def ema_closed_form(p, e0, decays):
    """fp64: p + (e0 - p) * prod_j d_j for a CONSTANT p, with d_j = 1 - omd_j the decay the kernel effectively applies (omd_j is
    the fp32 number it multiplies by, so its rounding is not part of the error budget below)."""
    prod = 1.0
    for d in decays:
        prod *= 1.0 - float(F32(1.0) - F32(d))
    return np.asarray(p, dtype=np.float64) + (np.asarray(e0, dtype=np.float64) - np.asarray(p, dtype=np.float64)) * prod


def ema_closed_form_bound(p, e_seq, decays):
    """Counted roundings of k updates against ema_closed_form, per element.  One update computes
        s = fl(p - e), q = fl(omd * s), e' = fl(e + q):
    three roundings, each relative U32: |s - (p - e)| <= U32 |p - e|, q adds U32 omd |s|, e' adds U32 |e'|.  An error B already in e
    is carried as d * B (e' - p = d (e - p) exactly).  So  B' <= d B + U32 (2 omd |p - e| (1 + U32) + |e'|),  evaluated on the
    computed sequence e_seq[0..k] (fp32 values, exact in fp64).  Values are O(1): no underflow term."""
    p = np.asarray(p, dtype=np.float64)
    B = np.zeros_like(p)
    for j, d in enumerate(decays):
        omd = float(F32(1.0) - F32(d))
        e, e1 = e_seq[j].astype(np.float64), e_seq[j + 1].astype(np.float64)
        B = (1.0 - omd) * B + U32 * (2.0 * omd * np.abs(p - e) * (1.0 + U32) + np.abs(e1))
    return B
