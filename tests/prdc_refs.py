"""fp64 numpy restatements of precision / recall / density / coverage (rg_knn_radii2, rg_radius_hits, rna_gan_amd.prdc), for
tests/test_prdc_ops_gpu.py and tests/test_prdc_metric_gpu.py.  Nothing here comes from rna_gan_amd; tests/test_prdc_refs_cpu.py
pins these functions against a brute-force definition in exact rational arithmetic and hand-worked cases without a GPU.

The contract, restated:
  d2(a, b) = sum_f ((double)a_f - (double)b_f)^2, accumulated sequentially in ascending f (the kernel fuses the square into the
             addition, this restatement rounds it: one rounding more per term, both inside the bound GAMMA(F) below; on integer
             features every intermediate is an exact integer and the two agree bit for bit);
  radius     r2_A[i] = k-th smallest of { d2(a_i, a_j) : j != i }, row i excluded BY INDEX (a duplicate row counts);
  hit        b_s hits a_r when d2(a_r, b_s) <= r2_B[s]  (<= on squared distances);
  a NaN d2 never hits and counts as +inf in the selection and in the minimum.
"""
import numpy as np

U = 2.0 ** -53


def GAMMA(F):
    """each d2 is a sum of F non-negative terms through at most F + 2 roundings: within (F+2)u / (1 - (F+2)u) of the exact value"""
    return (F + 2) * U / (1.0 - (F + 2) * U)


def dist2(a, b):
    """(na, nb) fp64 matrix of d2(a_r, b_s), summed sequentially in ascending f"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(a.shape[1]):
            diff = a[:, f, None] - b[None, :, f]
            acc = acc + diff * diff
    return acc


def _inf_for_nan(d):
    return np.where(np.isnan(d), np.inf, d)


def radii2_ref(a, k):
    """(n,) squared k-th nearest-neighbour radii, own INDEX excluded"""
    d = _inf_for_nan(dist2(a, a))
    n = d.shape[0]
    assert 1 <= k <= n - 1
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        out[i] = np.sort(np.delete(d[i], i))[k - 1]
    return out


def hits_ref(a, b, rb2=None, scale=1.0):
    """(count int32 or None, mind2): count[r] = #{ s : d2(a_r, b_s) * scale <= rb2[s] }, mind2[r] = min_s d2(a_r, b_s).
    scale = 1 + 2 GAMMA gives the strict count, 1 - 2 GAMMA the loose one, of the general-float interval."""
    d = dist2(a, b)
    mind2 = _inf_for_nan(d).min(axis=1)
    if rb2 is None:
        return None, mind2
    with np.errstate(invalid="ignore"):
        count = (d * scale <= np.asarray(rb2, dtype=np.float64)[None, :]).sum(axis=1).astype(np.int32)
    return count, mind2


def prdc_ref(x, y, k):
    """the four values of the real set x (m rows) and the generated set y (n rows)"""
    m, n = len(x), len(y)
    rx2, ry2 = radii2_ref(x, k), radii2_ref(y, k)
    in_real, _ = hits_ref(y, x, rx2)
    in_fake, nearest = hits_ref(x, y, ry2)
    return {"precision": float(np.float64((in_real > 0).sum()) / n),
            "recall": float(np.float64((in_fake > 0).sum()) / m),
            "density": float(np.float64(in_real.astype(np.int64).sum()) / (float(k) * n)),
            "coverage": float(np.float64((nearest <= rx2).sum()) / m)}


def integer_case(na, nb, F, seed):
    """(a, b): integer features in [-3, 3] as fp32 -- every d2 is an exact integer in fp64 whatever the order or fusing.  With so
    few values exact ties abound; duplicates are planted on purpose: a's last row repeats its first (in another tile once
    na > 64), b's middle row repeats a's first and b's last row repeats b's first."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, size=(na, F)).astype(np.float32)
    b = rng.integers(-3, 4, size=(nb, F)).astype(np.float32)
    if na > 2:
        a[na - 1] = a[0]
    if nb > 0 and na > 0:
        b[nb // 2] = a[0]
    if nb > 2:
        b[nb - 1] = b[0]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b
