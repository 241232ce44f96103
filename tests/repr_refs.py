"""fp64 numpy restatements of the per-group sums, the partner ranks and the retrieval scores (rg_group_sums_update,
rg_match_ranks, rna_gan_amd.representation), for tests/test_repr_ops_gpu.py and tests/test_repr_metric_gpu.py.  Nothing here
comes from rna_gan_amd; tests/test_repr_refs_cpu.py pins these functions against independent formulations without a GPU.

The contract, restated:
  sums[g][j]  the value already there, then (double)x[r][j] added for the rows r with group[r] == g in ascending r: ONE chain of
              fp64 additions per entry; ids outside [0, G) are skipped, neither summed nor counted;
  d2(a, b)    sum_f (a_f - b_f)^2 on fp64 rows, one rounded subtraction per feature, accumulated in ascending f (the kernel
              fuses the square into the addition, this restatement rounds it: both within prdc_refs.GAMMA(F) of the exact value;
              on integer features every intermediate is an exact integer and the two agree bit for bit);
  rank[r]     #{ s != t : d2(a_r, b_s) < d* } + #{ s < t : d2(a_r, b_s) == d* } with t = target[r], d* = d2(a_r, b_t); a NaN
              d2 never counts, a NaN d* gives nb - 1.
"""
import numpy as np


def group_sums_ref(x, group, G, sums=None, counts=None):
    """(sums (G, F) fp64, counts (G,) int64) continued from the given ones (zeros when None): the sequential chain, row by row"""
    x = np.asarray(x, dtype=np.float32)
    group = np.asarray(group)
    n, F = x.shape
    sums = np.zeros((G, F), dtype=np.float64) if sums is None else np.array(sums, dtype=np.float64)
    counts = np.zeros(G, dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64)
    assert sums.shape == (G, F) and counts.shape == (G,) and group.shape == (n,)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(n):
            g = int(group[r])
            if 0 <= g < G:
                sums[g] = sums[g] + x[r].astype(np.float64)
                counts[g] += 1
    return sums, counts


def dist2_f64(a, b):
    """(na, nb) fp64 matrix of d2(a_r, b_s) of fp64 rows, summed sequentially in ascending f"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(a.shape[1]):
            diff = a[:, f, None] - b[None, :, f]
            acc = acc + diff * diff
    return acc


def ranks_from_d2(d, target, scale=1.0):
    """(rank int32, dtarget) from a d2 matrix.  scale != 1: the threshold d* is scaled (d* itself is returned unscaled) -- the
    brackets of the general-float test; a scaled threshold has no ties to break, so s != t entries count when d2 <= d* scale
    for scale > 1 and when d2 < d* scale for scale < 1."""
    na, nb = d.shape
    target = np.arange(na) if target is None else np.asarray(target)
    rank = np.empty(na, dtype=np.int32)
    dstar = np.empty(na, dtype=np.float64)
    s = np.arange(nb)
    with np.errstate(invalid="ignore"):
        for r in range(na):
            t = int(target[r])
            ds = d[r, t]
            dstar[r] = ds
            if np.isnan(ds):
                rank[r] = nb - 1
            elif scale == 1.0:
                rank[r] = int(((d[r] < ds) & (s != t)).sum() + ((d[r] == ds) & (s < t)).sum())
            elif scale > 1.0:
                rank[r] = int(((d[r] <= ds * scale) & (s != t)).sum())
            else:
                rank[r] = int(((d[r] < ds * scale) & (s != t)).sum())
    return rank, dstar


def match_ranks_ref(a, b, target=None):
    return ranks_from_d2(dist2_f64(a, b), target)


def retrieval_scores_ref(rank, n_ref):
    rank = np.asarray(rank, dtype=np.int64)
    return {"top1": float(np.mean(rank == 0)), "top5": float(np.mean(rank < min(5, n_ref))),
            "mrr": float(np.mean(1.0 / (rank + 1.0))), "median_rank": float(np.median(rank)), "chance_top1": 1.0 / n_ref}


def wide_floats(n, F, seed):
    """general fp32 values over 80 binades with both signs.  fp32 values within 29 binades of each other add exactly in fp64
    (24 + 29 = 53 bits); only a wider spread makes the fp64 additions round, so that their order shows in the low bits."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, F)) * np.exp2(rng.integers(-40, 41, size=(n, F)))
    return x.astype(np.float32)


def integer_rows(na, nb, F, seed):
    """(a, b, target): integer-valued fp64 rows in [-3, 3] (every d2 an exact integer), a permuted target, planted duplicates of
    the target row at a lower AND a higher index of b (exact ties on both sides of the target index) and a duplicate query"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, size=(na, F)).astype(np.float64)
    b = rng.integers(-3, 4, size=(nb, F)).astype(np.float64)
    target = rng.integers(0, nb, size=na).astype(np.int32)
    if nb >= 3:
        t = nb // 2
        target[0] = t
        b[0] = b[t]
        b[nb - 1] = b[t]
        if na > 1:
            target[na - 1] = t
            a[na - 1] = a[0]
    return a, b, target
