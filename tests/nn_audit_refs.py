"""numpy int64 restatements of rg_tile_descriptor_i8 and rg_nn_topk_i8 (include/rnagan_hip.h) and of the audit's host arithmetic
(rna_gan_amd.nearest), written for reading, not speed: the descriptor by explicit block loops, the top-k by a stable sort of the
packed keys.  tests/test_nn_audit_refs_cpu.py pins them against brute-force Python."""
import numpy as np

NONE = np.iinfo(np.int64).max


def ldd_of(D):
    return (D + 63) // 64 * 64


def descriptor(tiles, f, ldd=None):
    """tiles uint8 [N][C][S][S] -> (desc int8 [N][ldd], norm2 int32 [N])"""
    tiles = np.asarray(tiles)
    N, C, S, _ = tiles.shape
    assert S % f == 0
    P = S // f
    D = C * P * P
    ldd = ldd_of(D) if ldd is None else ldd
    desc = np.zeros((N, ldd), np.int64)
    for c in range(C):
        for y in range(P):
            for x in range(P):
                block = tiles[:, c, y * f:(y + 1) * f, x * f:(x + 1) * f].astype(np.int64).reshape(N, -1).sum(axis=1)
                desc[:, c * P * P + y * P + x] = (block + (f * f) // 2) // (f * f) - 128
    assert desc.min(initial=0) >= -128 and desc.max(initial=0) <= 127
    return desc.astype(np.int8), (desc * desc).sum(axis=1).astype(np.int32)


def norms(a):
    a = np.asarray(a).astype(np.int64)
    return (a * a).sum(axis=1).astype(np.int32)


def d2_matrix(a, na2, b, nb2, D):
    """int64 [Q][N]: na2[q] + nb2[r] - 2 <a_q[:D], b_r[:D]>"""
    a = np.asarray(a)[:, :D].astype(np.int64)
    b = np.asarray(b)[:, :D].astype(np.int64)
    return np.asarray(na2).astype(np.int64)[:, None] + np.asarray(nb2).astype(np.int64)[None, :] - 2 * (a @ b.T)


def topk_keys(a, na2, b, nb2, D, k, exclude=None):
    """uint64 [Q][k]: per query, ascending, the k smallest (d2 << 32) | r over the candidate rows"""
    d2 = d2_matrix(a, na2, b, nb2, D)
    Q, N = d2.shape
    assert d2.min(initial=0) >= 0 and d2.max(initial=0) < 2 ** 31
    keys = (d2 << 32) | np.arange(N, dtype=np.int64)[None, :]
    out = np.empty((Q, k), np.int64)
    for q in range(Q):
        row = keys[q]
        if exclude is not None and 0 <= int(exclude[q]) < N:
            row = np.delete(row, int(exclude[q]))
        assert row.size >= k
        out[q] = np.sort(row, kind="stable")[:k]
    return out.astype(np.uint64)


def split_keys(keys):
    keys = np.asarray(keys).astype(np.uint64)
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xffffffff)).astype(np.int64)


def d4(x, code):
    """the symmetry `code` of rna_gan_amd.augment on the last two axes: flip left-right if code & 4, then rotate by code & 3"""
    x = np.asarray(x)
    return np.ascontiguousarray(np.rot90(x[..., ::-1] if code & 4 else x, code & 3, axes=(-2, -1)))


def copied(d2_nearest, loo_d2):
    return np.array([int(d) < int(l) for d, l in zip(d2_nearest, loo_d2)], dtype=bool)


def closer_than_heldout(dg, dh):
    less = sum(1 for g in dg for h in dh if g < h)
    equal = sum(1 for g in dg for h in dh if g == h)
    return (less + 0.5 * equal) / (len(dg) * len(dh))


def audit(generated, train, f, k, use_d4=False, heldout=None):
    """the whole audit on uint8 arrays: dict of d2 [G][k], index [G][k], loo_d2 [G], copied [G], copy_rate, exact [G] and
    closer_than_heldout (None without held-out tiles)"""
    tdesc, tn = descriptor(train, f)
    D = tdesc.shape[1]

    def search(tiles, kk):
        best = []
        for code in (range(8) if use_d4 else (0,)):
            qd, qn = descriptor(np.stack([d4(t, code) for t in tiles]), f)
            best.append(d2_matrix(qd, qn, tdesc, tn, D))
        d2 = np.minimum.reduce(best)                                   # a row counts once, at its smallest distance
        keys = np.sort((d2 << 32) | np.arange(d2.shape[1], dtype=np.int64)[None, :], axis=1, kind="stable")[:, :kk]
        return keys >> 32, keys & 0xffffffff

    d2, ix = search(generated, k)
    tt = d2_matrix(tdesc, tn, tdesc, tn, D)
    np.fill_diagonal(tt, NONE)
    loo = tt.min(axis=1)[ix[:, 0]]
    out = {"d2": d2, "index": ix, "loo_d2": loo, "copied": copied(d2[:, 0], loo), "exact": d2[:, 0] == 0}
    out["copy_rate"] = float(out["copied"].mean())
    out["closer_than_heldout"] = None if heldout is None else closer_than_heldout(d2[:, 0].tolist(), search(heldout, 1)[0][:, 0].tolist())
    return out
