"""numpy restatements of rg_linear_scores_f64, rg_softmax_residual_f64 and rg_rows_weighted_colsums_f64 (include/rnagan_hip.h,
rna_gan_amd/csrc/rg_linprobe.hip) and a ``fit`` that runs rna_gan_amd.linprobe's own optimiser on them.  Pinned without a GPU by
tests/test_linprobe_refs_cpu.py; the GPU tests compare the kernels with these.

The contracts state CHAINS: acc = fma(a, b, acc) in a stated order.  numpy has no fused multiply-add, and an fp32 value times an
fp64 value does not fit an fp64 (nor an x87 long double), so ``fma`` below computes it from error-free transformations: the
product as an exact pair (Dekker / Veltkamp), the sum of product and addend as an exact pair (Knuth's TwoSum), the two low parts
added ROUNDED TO ODD and the final addition rounded to nearest -- Boldo & Melquiond 2008, "Emulation of a FMA and
correctly-rounded sums: proved algorithms using rounding to odd", Theorem 1: the result is the correctly rounded a b + c as
long as nothing overflows or falls into the subnormal range.  The chains run at the Python level in the stated order (one
Python step per feature, or per row of a block), vectorised only ACROSS independent chains."""
import numpy as np

from rna_gan_amd import linprobe as LP

COLSUM_ROWS = 256
U = 2.0 ** -53                     # unit roundoff of fp64
_SPLIT = 134217729.0               # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    s, e = _two_sum(a, b)
    s = np.array(s, dtype=np.float64)
    fix = (e != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
    if fix.any():
        # the exact sum lies strictly between s and its neighbour on e's side; s is even, so that neighbour is the odd one --
        # unless s is exactly the rounding of a tie-free sum, which is this same case
        s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s


def fma(a, b, c):
    """correctly rounded a * b + c, element by element on fp64 arrays (see the module docstring)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    ph, pl = _two_prod(a, b)
    th, tl = _two_sum(c, ph)
    out = th + _add_round_to_odd(tl, pl)
    bad = ~np.isfinite(out)
    if bad.any():                                            # NaN / inf operands: the error terms are NaN, the plain form is right
        out = np.where(bad, a * b + c, out)
    return out


def scores_ref(x, w, bias=None):
    """z (n, C) fp64: per (row, class) ONE chain acc = fma((double)x[r][f], w[c][f], acc) in ascending f from 0.0, then
    acc + bias[c] as one rounded addition (bias None: acc)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    acc = np.zeros((x.shape[0], w.shape[0]))
    for f in range(x.shape[1]):
        acc = fma(x[:, f:f + 1], w[None, :, f], acc)
    return acc if bias is None else acc + np.asarray(bias, dtype=np.float64)[None, :]


def softmax_residual_ref(z, label, weight=None, dtype=np.float64):
    """(resid (n, C), row_loss (n,)) in ``dtype`` (np.longdouble: the reference the device's exp / log are bounded against).
    m = max z_c (a NaN logit makes it NaN); e_c = exp(z_c - m); s = sum e_c in ascending c from 0; p_c = e_c / s;
    resid = wt (p_c - [c == y]); row_loss = wt (log(s) - (z_y - m)); a label outside [0, C): exact zeros."""
    z = np.asarray(z, dtype=np.float64).astype(dtype)
    n, C = z.shape
    label = np.asarray(label)
    wt = np.ones(n, dtype=dtype) if weight is None else np.asarray(weight, dtype=np.float64).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(np.isnan(z).any(axis=1), dtype(np.nan), z.max(axis=1))
        e = np.exp(z - m[:, None])
        s = np.zeros(n, dtype=dtype)
        for c in range(C):
            s = s + e[:, c]
        ok = (label >= 0) & (label < C)
        y = np.where(ok, label, 0)
        onehot = (np.arange(C)[None, :] == y[:, None]).astype(dtype)
        resid = wt[:, None] * (e / s[:, None] - onehot)
        loss = wt * (np.log(s) - (z[np.arange(n), y] - m))
    resid[~ok] = 0
    loss[~ok] = 0
    return resid, loss


def colsums_ref(x, r, power=1):
    """out (C, F) fp64: rows in blocks of 256; inside a block one chain acc = fma(r[row][c], t(x[row][f]), acc) per entry in
    ascending row order from 0.0; the block partials of an entry added in ascending block order from 0.0.  The blocks are
    independent chains and are walked side by side."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    r = np.asarray(r, dtype=np.float64)
    assert power in (1, 2) and x.shape[0] == r.shape[0]
    t = x * x if power == 2 else x                           # the square of an fp32 value is exact in fp64
    n, F = x.shape
    C = r.shape[1]
    blocks = (n + COLSUM_ROWS - 1) // COLSUM_ROWS
    tp = np.zeros((blocks * COLSUM_ROWS, F)); tp[:n] = t
    rp = np.zeros((blocks * COLSUM_ROWS, C)); rp[:n] = r     # rows past the end: fma(0, 0, acc) = acc (acc is never -0.0)
    tp, rp = tp.reshape(blocks, COLSUM_ROWS, F), rp.reshape(blocks, COLSUM_ROWS, C)
    ones = bool((t == 1.0).all())                            # fma(r, 1, acc) IS the rounded sum r + acc: skip the emulation
    acc = np.zeros((blocks, C, F))
    for row in range(min(n, COLSUM_ROWS)):
        a, b = rp[:, row, :, None], tp[:, row, None, :]
        acc = (a + acc) if ones else fma(a, b, acc)
    out = np.zeros((C, F))
    for blk in range(blocks):
        out = out + acc[blk]
    return out


class NumpyOps:
    """linprobe.fit_with_ops' operations on the restatements: the composition rna_gan_amd.linprobe._DeviceOps launches"""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float32)
        self.ones = np.ones((self.x.shape[0], 1), dtype=np.float32)

    def moments(self, mask01):
        r = np.asarray(mask01, dtype=np.float64)[:, None]
        return colsums_ref(self.x, r, 1)[0], colsums_ref(self.x, r, 2)[0]

    def set_rows(self, label, weight):
        self.label, self.weight = np.array(label, dtype=np.int32), (None if weight is None else np.array(weight, dtype=np.float64))

    def evaluate(self, W, b):
        resid, loss = softmax_residual_ref(scores_ref(self.x, W, b), self.label, self.weight)
        return (colsums_ref(self.x, resid, 1), colsums_ref(self.ones, resid, 1)[:, 0],
                float(colsums_ref(self.ones, loss[:, None], 1)[0, 0]))


def fit(x, y, n_classes, l2=1e-3, sample_weight=None, mask=None, max_iter=200, gtol=1e-6):
    """rna_gan_amd.linprobe.fit with the restatements in place of the kernels: the same optimiser, the same host arithmetic"""
    x = np.asarray(x, dtype=np.float32)
    return LP.fit_with_ops(NumpyOps(x), x.shape[0], x.shape[1], np.asarray(y), n_classes, l2, sample_weight, mask, max_iter, gtol)


def objective(x, y, W_std, b_std, mean, scale, l2, sample_weight=None, mask=None):
    """(f, gradient (C (F + 1),)) of the fit's objective at standardised-coordinate parameters, in plain vectorised numpy fp64
    (no chains): what the strong-convexity comparisons evaluate at somebody else's solution"""
    from scipy.special import log_softmax
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    keep = np.ones(n, dtype=bool) if mask is None else np.asarray(mask)
    wt = (np.ones(n) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64))[keep]
    xs, yk = (x[keep] - mean) / scale, np.asarray(y)[keep]
    lp = log_softmax(xs @ W_std.T + b_std, axis=1)
    total = wt.sum()
    f = -(wt * lp[np.arange(len(yk)), yk]).sum() / total + 0.5 * l2 * float((W_std * W_std).sum())
    R = np.exp(lp)
    R[np.arange(len(yk)), yk] -= 1.0
    R *= wt[:, None]
    return f, np.concatenate([(R.T @ xs / total + l2 * W_std).reshape(-1), R.sum(axis=0) / total])


def strong_convexity_gap(probe, l2):
    """the bound of the issue: f(probe) - min f <= |grad f(probe)|^2 / (2 l2), plus a few eps |f| for evaluating f itself.
    The penalty makes the objective l2-strongly convex in W; in the bias it is convex with the curvature the data supply (the
    common shift of all biases is flat, and the gradient has no component along it)."""
    return probe.grad_norm ** 2 / (2.0 * l2) + 8.0 * np.finfo(np.float64).eps * abs(probe.objective)


def blobs(n, F, C, sep=4.0, seed=0):
    """(x fp32 (n, F), y int64 (n,)): C <= F unit-variance normal clouds, class c centred at (sep / sqrt 2) e_c: every two
    centroids are ``sep`` sigma apart"""
    assert C <= F
    rng = np.random.default_rng([seed, n, F, C])
    y = np.arange(n) % C
    x = rng.standard_normal((n, F))
    for c in range(C):
        x[y == c, c] += sep / np.sqrt(2.0)
    return x.astype(np.float32), y.astype(np.int64)
