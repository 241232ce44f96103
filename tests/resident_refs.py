"""numpy restatement of rg_tile_gather_transform's contract (include/rnagan_hip.h) and of the two index rules of
rna_gan_amd.resident, shared by the resident-set test files.

The gather is tile_transform_ref of tests/augment_refs.py (imported, not edited) applied to store[clip(index, 0, M - 1)]; the
epoch order and the shard rule are written as explicit loops, so that the module under test is compared with something that
shares no code with it.  tests/test_resident_refs_cpu.py pins these against the augment_refs functions on a pre-gathered copy."""
import numpy as np

from augment_refs import tile_transform_ref


def gather_transform_ref(store, index=None, codes=None, n=None, mean=0.5, std=0.5):
    """store [M][C][S][S] uint8 -> [N][C][S][S] float32: sample k is tile clip(index[k], 0, M - 1) (index None: tile k, N = n)
    under codes[k] & 7 (None: 0)."""
    M = store.shape[0]
    assert store.dtype == np.uint8 and store.ndim == 4
    if index is None:
        N = M if n is None else n
        assert N <= M
        index = np.arange(N, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64)
    picked = np.empty((len(index),) + store.shape[1:], dtype=np.uint8)
    for k in range(len(index)):
        t = int(index[k])
        t = 0 if t < 0 else M - 1 if t >= M else t
        picked[k] = store[t]
    return tile_transform_ref(picked, codes, mean, std)


def epoch_order_ref(seed, rank, epoch, m):
    """The order of one epoch: the permutation numpy's counter-seeded generator draws, copied out element by element."""
    p = np.random.default_rng([seed, rank, epoch]).permutation(m)
    out = []
    for k in range(m):
        out.append(int(p[k]))
    return out


def shard_ref(n_items, rank, world, batch_size):
    """Strided shard, truncated to an equal whole number of batches per rank."""
    per_rank = n_items // world
    per_rank -= per_rank % batch_size
    out = []
    i = rank
    while i < n_items and len(out) < per_rank:
        out.append(i)
        i += world
    return out
