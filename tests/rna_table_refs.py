"""Plain-loop restatements for the resident expression table (rna_gan_amd.rna_tables, rg_rows_gather_f32 in
include/rnagan_hip.h): the gather with clamp and zero pad, the epoch order, the split rule.  Written as loops over single
elements on purpose -- nothing here shares an expression with the code under test."""
import math

import numpy as np


def rows_gather_ref(table, F, index, n=None, ld_dst=None):
    """table [M][ld_table] float32 (columns [0, F) are the data), index a list of ints or None (= 0 .. n - 1) -> [N][ld_dst]:
    dst[k][c] = table[clamp(index[k])][c] for c < F, 0 behind.  Bits are moved, never recomputed."""
    table = np.asarray(table, dtype=np.float32)
    M = table.shape[0]
    src = table.view(np.uint32)
    if index is None:
        index = list(range(n))
    ld = F if ld_dst is None else ld_dst
    out = np.zeros((len(index), ld), dtype=np.uint32)
    for k, t in enumerate(index):
        t = int(t)
        if t < 0:
            t = 0
        if t > M - 1:
            t = M - 1
        for c in range(F):
            out[k, c] = src[t, c]
    return out.view(np.float32)


def epoch_order_ref(seed, epoch, items):
    perm = np.random.default_rng([seed, 0, epoch]).permutation(len(items))
    return [int(items[int(p)]) for p in perm]


def batches_ref(order, batch_size, drop_last):
    out, t = [], 0
    while t < len(order):
        b = order[t:t + batch_size]
        if len(b) == batch_size or not drop_last:
            out.append(list(b))
        t += batch_size
    return out


def split_ref(m):
    """(train, test) positions of one 80/20 split of m rows: one permutation of numpy's global legacy generator."""
    n_test = int(math.ceil(0.2 * m))
    n_train = int(math.floor(0.8 * m))
    p = np.random.permutation(m)
    test = [int(p[i]) for i in range(n_test)]
    train = [int(p[i]) for i in range(n_test, n_test + n_train)]
    return train, test


def split_tables_ref(sizes, seed):
    """Per table {train, val, test} positions: the test split first, then the train part split again."""
    np.random.seed(seed)
    out = []
    for m in sizes:
        train, test = split_ref(m)
        tr2, va2 = split_ref(len(train))
        out.append({"train": [train[i] for i in tr2], "val": [train[i] for i in va2], "test": test})
    return out
