"""numpy restatement of rg_tile_transform's contract (include/rnagan_hip.h), shared by the augmentation test files.

The eight codes are written as explicit index loops over the table of the header -- no rot90, no flip -- so the kernel and the
torch path of rna_gan_amd.augment are compared with something that shares no code with either; tests/test_augment_refs_cpu.py
pins the table itself against np.rot90."""
import functools

import numpy as np

# code -> (source row, source column) of output pixel (i, j), T = S - 1
SOURCE_INDEX = {
    0: lambda i, j, T: (i, j),
    1: lambda i, j, T: (j, T - i),
    2: lambda i, j, T: (T - i, T - j),
    3: lambda i, j, T: (T - j, i),
    4: lambda i, j, T: (i, T - j),
    5: lambda i, j, T: (j, i),
    6: lambda i, j, T: (T - i, j),
    7: lambda i, j, T: (T - j, T - i),
}


def d4_plane_ref(plane, code):
    """One [S][S] plane under ``code & 7``, pixel by pixel."""
    S = plane.shape[0]
    assert plane.shape == (S, S)
    src = SOURCE_INDEX[int(code) & 7]
    out = np.empty_like(plane)
    for i in range(S):
        for j in range(S):
            out[i, j] = plane[src(i, j, S - 1)]
    return out


@functools.lru_cache(maxsize=None)
def d4_index_ref(S, code):
    """(rows, cols) int arrays [S][S]: the source index of every output pixel (the loop above as a gather, for large S; computed
    once per (S, code) and shared)."""
    rows = np.empty((S, S), dtype=np.int64)
    cols = np.empty((S, S), dtype=np.int64)
    src = SOURCE_INDEX[int(code) & 7]
    for i in range(S):
        for j in range(S):
            rows[i, j], cols[i, j] = src(i, j, S - 1)
    rows.setflags(write=False)
    cols.setflags(write=False)
    return rows, cols


def normalize_ref(u8, mean=0.5, std=0.5):
    """((float)b / 255.0f - mean) / std: three separately rounded fp32 operations."""
    assert u8.dtype == np.uint8
    f = np.float32
    return ((u8.astype(f) / f(255.0)) - f(mean)) / f(std)


def tile_transform_ref(src, codes=None, mean=0.5, std=0.5):
    """src [N][C][S][S] uint8 or float32 -> float32: uint8 normalised, float32 copied; sample n mapped by codes[n] & 7 (None: 0)."""
    N, C, S, S2 = src.shape
    assert S == S2 and src.dtype in (np.uint8, np.float32)
    x = normalize_ref(src, mean, std) if src.dtype == np.uint8 else src.copy()
    if codes is None:
        return x
    assert len(codes) == N
    out = np.empty_like(x)
    for n in range(N):
        rows, cols = d4_index_ref(S, int(codes[n]) & 7)
        out[n] = x[n][:, rows, cols]
    return out


def asymmetric_tile(S, dtype=np.float32):
    """An [S][S] plane without any symmetry: all S * S values differ."""
    return np.arange(S * S, dtype=np.int64).reshape(S, S).astype(dtype)
