"""Memorisation audit: is the generator reproducing its training tiles?

Every quality score of this project (Fréchet, kernel distance, precision / recall / density / coverage, conditioning fidelity, tissue
yield) IMPROVES when the generator copies training tiles, so none of them can see the one failure that matters where synthetic
histology is shared in place of patient tiles.  This module answers "which training tiles are closest to these samples, and are the
samples closer to them than real tiles are to each other?" with an exact all-pairs search on the device.

Tiles are compared through int8 DESCRIPTORS -- the tile averaged over ``factor`` x ``factor`` blocks, minus 128 -- so every distance
is an integer, computed exactly by rg_tile_descriptor_i8 and rg_nn_topk_i8 (rna_gan_amd/csrc/rg_nn.hip, the contract in
include/rnagan_hip.h): the dot products on the int8 matrix cores, ties to the lower training index, one result whatever the launch
plan.  On a CPU tensor the same integers come from torch integer ops; on a CUDA tensor there is no fallback: the kernels run or the
call raises.

    descriptors(tiles_u8, factor)            (desc int8 [N][ldd], norm2 int32 [N]); ldd = D rounded up to 64, the pad columns 0
    nearest(query, ref, k, exclude)          (d2 int64 [Q][k], index int64 [Q][k]), ascending in (d2, index)
    TrainIndex(tiles or DeviceTileSet)       the descriptors of a whole training set, built once, chunk by chunk
    audit(generated_u8, index, ...)          an AuditResult (below)

Out of scope: feature-space search (rna_gan_amd.prdc serves small feature sets), sets that do not fit the device, an index across
the ranks of a data-parallel run.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi
from .augment import d4_apply
from .resident import RESERVE_BYTES

FACTORS = (1, 2, 4, 8, 16, 32)
D_MAX = 32768            # D 255^2 < 2^31: every squared distance fits int32
K_MAX = 8


def descriptor_shape(C, S, factor):
    """(D, ldd) of [C][S][S] tiles."""
    if factor not in FACTORS or S % factor:
        raise ValueError("factor must be one of %s and divide the tile size %d" % (FACTORS, S))
    P = S // factor
    D = C * P * P
    if D > D_MAX:
        raise ValueError("a descriptor of %d bytes is more than %d (squared distances would leave int32): raise factor" % (D, D_MAX))
    return D, (D + 63) // 64 * 64


def _check_tiles(tiles_u8):
    if not torch.is_tensor(tiles_u8) or tiles_u8.dtype != torch.uint8 or tiles_u8.dim() != 4 or tiles_u8.shape[2] != tiles_u8.shape[3]:
        raise ValueError("tiles must be an [N][C][S][S] uint8 tensor (export.tiles_u8(layout='nchw'), DeviceTileSet.tiles)")


def _descriptors_into(tiles_u8, factor, desc, norm2):
    """desc [N][ldd] int8 and norm2 [N] int32 (views of the caller's buffers) of tiles_u8 [N][C][S][S]."""
    N, C, S, _ = tiles_u8.shape
    D, ldd = descriptor_shape(C, S, factor)
    if N == 0:
        return
    tiles_u8 = tiles_u8.contiguous()
    if tiles_u8.device.type != "cuda":
        P = S // factor
        s = tiles_u8.view(N, C, P, factor, P, factor).long().sum(dim=(3, 5))
        v = torch.div(s + (factor * factor) // 2, factor * factor, rounding_mode="floor") - 128
        desc.zero_()
        desc[:, :D] = v.reshape(N, D).to(torch.int8)
        norm2.copy_((v * v).sum(dim=(1, 2, 3)).to(torch.int32))
        return
    _abi.launch("rg_tile_descriptor_i8", tiles_u8.device, tiles_u8.data_ptr(), N, C, S, factor, desc.data_ptr(), ldd, norm2.data_ptr())


def descriptors(tiles_u8, factor=4):
    """(desc int8 [N][ldd], norm2 int32 [N]) of uint8 [N][C][S][S] tiles, on their device."""
    _check_tiles(tiles_u8)
    N, C, S, _ = tiles_u8.shape
    _, ldd = descriptor_shape(C, S, int(factor))
    desc = torch.empty((N, ldd), dtype=torch.int8, device=tiles_u8.device)
    norm2 = torch.empty((N,), dtype=torch.int32, device=tiles_u8.device)
    _descriptors_into(tiles_u8, int(factor), desc, norm2)
    return desc, norm2


def _pair(x):
    """(desc, norm2) from what descriptors() returned, a TrainIndex, or a bare descriptor tensor (norms by integer ops)."""
    if isinstance(x, TrainIndex):
        return x.desc, x.norm2
    if isinstance(x, (tuple, list)):
        desc, norm2 = x
    else:
        desc, norm2 = x, None
    if not torch.is_tensor(desc) or desc.dtype != torch.int8 or desc.dim() != 2 or desc.shape[1] % 64 or not desc.shape[1]:
        raise ValueError("descriptors are an int8 [N][ldd] tensor with ldd a positive multiple of 64")
    if desc.shape[1] > D_MAX:
        raise ValueError("descriptors of %d bytes are more than %d" % (desc.shape[1], D_MAX))
    desc = desc.contiguous()
    if norm2 is None:
        norm2 = (desc.to(torch.int32) ** 2).sum(dim=1, dtype=torch.int32)
    if norm2.dtype != torch.int32 or tuple(norm2.shape) != (desc.shape[0],) or norm2.device != desc.device:
        raise ValueError("norm2 is int32 [N] on the descriptors' device")
    return desc, norm2.contiguous()


def nearest(query_desc, ref_desc, k=4, exclude=None):
    """The k nearest rows of ``ref_desc`` to every row of ``query_desc``: (d2 int64 [Q][k], index int64 [Q][k]), ascending in the
    total order (d2, index) -- ties go to the lower index.  Both arguments are what ``descriptors`` returned (or a TrainIndex).
    exclude: None, or [Q] integers: row exclude[q] is no candidate for query q (a value outside [0, N) excludes nothing)."""
    a, na = _pair(query_desc)
    b, nb = _pair(ref_desc)
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("k must be in 1..%d" % K_MAX)
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError("query and reference descriptors differ in width or device")
    Q, N, ldd = a.shape[0], b.shape[0], a.shape[1]
    if exclude is not None:
        exclude = torch.as_tensor(exclude).to(device=a.device, dtype=torch.int32).contiguous()
        if tuple(exclude.shape) != (Q,):
            raise ValueError("exclude holds one row index per query")
    if N - (1 if exclude is not None else 0) < k:
        raise ValueError("%d reference rows%s are fewer than k = %d candidates" % (N, " less an excluded one" if exclude is not None else "", k))
    if Q == 0:
        z = torch.zeros((0, k), dtype=torch.int64, device=a.device)
        return z, z.clone()
    if a.device.type != "cuda":
        keys = torch.empty((Q, k), dtype=torch.int64)
        bl, nbl, rows = b.long(), nb.long(), torch.arange(N, dtype=torch.int64)
        for i in range(0, Q, 256):
            d2 = na[i:i + 256].long()[:, None] + nbl[None, :] - 2 * (a[i:i + 256].long() @ bl.t())
            key = (d2 << 32) | rows[None, :]
            if exclude is not None:
                key = torch.where(rows[None, :] == exclude[i:i + 256].long()[:, None], torch.iinfo(torch.int64).max, key)
            keys[i:i + 256] = torch.topk(key, k, dim=1, largest=False, sorted=True).values
    else:
        need = _abi.load().rg_nn_topk_ws_bytes(Q, N, k)
        ws = torch.empty((max(need, 8),), dtype=torch.uint8, device=a.device)
        keys = torch.empty((Q, k), dtype=torch.int64, device=a.device)          # the uint64 keys are below 2^63
        _abi.launch("rg_nn_topk_i8", a.device, a.data_ptr(), na.data_ptr(), Q, b.data_ptr(), nb.data_ptr(), N, ldd, ldd, k,
                    0 if exclude is None else exclude.data_ptr(), keys.data_ptr(), ws.data_ptr(), ws.numel())
    return keys >> 32, keys & 0xffffffff


class TrainIndex:
    """The descriptors of a whole training set -- an [N][C][S][S] uint8 tensor or a resident.DeviceTileSet -- on the tiles' device:
    ``desc`` int8 [N][ldd], ``norm2`` int32 [N].  Built once, ``chunk`` tiles per descriptor call.  Raises MemoryError BEFORE
    allocating when the N ldd descriptor bytes exceed ``max_bytes`` (default on a CUDA device: its free memory minus the 8 GiB
    reserve of rna_gan_amd.resident; no limit on a CPU device)."""

    def __init__(self, tiles, factor=4, chunk=4096, max_bytes=None):
        tiles = getattr(tiles, "tiles", tiles)
        _check_tiles(tiles)
        self.factor, chunk = int(factor), max(int(chunk), 1)
        N, C, S, _ = tiles.shape
        self.D, self.ldd = descriptor_shape(C, S, self.factor)
        self.tile_shape = (C, S, S)
        device = tiles.device
        if max_bytes is None and device.type == "cuda":
            max_bytes = torch.cuda.mem_get_info(device)[0] - RESERVE_BYTES
        need = N * self.ldd + N * 4
        if max_bytes is not None and need > max_bytes:
            raise MemoryError("TrainIndex: %d descriptors of %d bytes need %d bytes on %s, the budget is %d bytes (free memory minus "
                              "%d GiB unless given): raise factor or audit a subset" % (N, self.ldd, need, device, max_bytes,
                                                                                        RESERVE_BYTES >> 30))
        self.desc = torch.empty((N, self.ldd), dtype=torch.int8, device=device)
        self.norm2 = torch.empty((N,), dtype=torch.int32, device=device)
        for i in range(0, N, chunk):
            _descriptors_into(tiles[i:i + chunk], self.factor, self.desc[i:i + chunk], self.norm2[i:i + chunk])

    def __len__(self):
        return self.desc.shape[0]

    @property
    def device(self):
        return self.desc.device

    def rows(self, index):
        """(desc, norm2) of the given training rows."""
        index = torch.as_tensor(index, dtype=torch.int64).to(self.device)
        return self.desc.index_select(0, index), self.norm2.index_select(0, index)


# ---------------------------------------------------------------------------------------------- host arithmetic
def copied_flags(d2_nearest, loo_d2):
    """copied[g] = d2_nearest[g] < loo_d2[g]: the sample is closer to its nearest training tile than any OTHER training tile is
    (the authenticity test of Alaa et al. 2022).  Equality is not a copy."""
    return np.asarray(d2_nearest, dtype=np.int64) < np.asarray(loo_d2, dtype=np.int64)


def closer_than_heldout(d_generated, d_heldout):
    """(#{(g, h): d_g < d_h} + 0.5 #{d_g == d_h}) / (G H) over nearest-training distances (the data-copying statistic of Meehan et
    al. 2020): 0.5 when generated and held-out tiles are equally close to the training set, towards 1 under copying."""
    dg = np.asarray(d_generated, dtype=np.int64).reshape(-1)
    dh = np.sort(np.asarray(d_heldout, dtype=np.int64).reshape(-1))
    if dg.size == 0 or dh.size == 0:
        raise ValueError("closer_than_heldout needs generated and held-out distances")
    above = dh.size - np.searchsorted(dh, dg, side="right")            # held-out distances strictly larger than d_g
    equal = np.searchsorted(dh, dg, side="right") - np.searchsorted(dh, dg, side="left")
    return float((2 * int(above.sum()) + int(equal.sum())) / (2.0 * dg.size * dh.size))


def merge_symmetries(d2_list, index_list, k):
    """Per query the k nearest DISTINCT rows over several searches of the same queries ([Q][k'] int64 arrays each): a row found
    under several symmetries counts once, at its smallest distance; ascending in (d2, index)."""
    d2 = np.concatenate([np.asarray(d, dtype=np.int64) for d in d2_list], axis=1)
    ix = np.concatenate([np.asarray(i, dtype=np.int64) for i in index_list], axis=1)
    Q = d2.shape[0]
    out_d, out_i = np.empty((Q, k), np.int64), np.empty((Q, k), np.int64)
    for q in range(Q):
        order = np.argsort((d2[q] << 32) | ix[q], kind="stable")
        _, first = np.unique(ix[q][order], return_index=True)
        keep = order[np.sort(first)][:k]
        if keep.size < k:
            raise ValueError("fewer than k distinct rows among the merged lists")
        out_d[q], out_i[q] = d2[q][keep], ix[q][keep]
    return out_d, out_i


class AuditResult:
    """d2, index        int64 [G][k]: the k nearest training tiles of every generated tile and their squared descriptor distances
    loo_d2           int64 [G]: from the generated tile's nearest training tile to ITS nearest other training tile
    copied           bool [G]: d2[:, 0] < loo_d2;   copy_rate: its mean
    exact            bool [G]: d2[:, 0] == 0;       exact_rate: its mean
    closer_than_heldout   float or None (no held-out tiles given);  heldout_d2 int64 [H] or None
    All numpy arrays on the host."""

    def __init__(self, d2, index, loo_d2, heldout_d2=None):
        self.d2, self.index, self.loo_d2, self.heldout_d2 = d2, index, loo_d2, heldout_d2
        self.copied = copied_flags(d2[:, 0], loo_d2)
        self.exact = d2[:, 0] == 0
        G = max(d2.shape[0], 1)
        self.copy_rate = float(self.copied.sum()) / G
        self.exact_rate = float(self.exact.sum()) / G
        self.closer_than_heldout = None if heldout_d2 is None else closer_than_heldout(d2[:, 0], heldout_d2)

    def summary(self):
        s = {"copy_rate": self.copy_rate, "exact": self.exact_rate, "min_d2": int(self.d2[:, 0].min()),
             "median_d2": float(np.median(self.d2[:, 0]))}
        if self.closer_than_heldout is not None:
            s["closer_than_heldout"] = self.closer_than_heldout
        return s


def _search(tiles_u8, index, k, d4):
    """(d2, index) int64 numpy [n][k] of uint8 tiles against a TrainIndex, under the identity or all eight symmetries."""
    _check_tiles(tiles_u8)
    if tuple(tiles_u8.shape[1:]) != tuple(index.tile_shape):
        raise ValueError("tiles of shape %s against an index of %s tiles" % (tuple(tiles_u8.shape[1:]), index.tile_shape))
    tiles_u8 = tiles_u8.to(index.device)
    ds, ixs = [], []
    for code in (range(8) if d4 else (0,)):
        t = tiles_u8 if code == 0 else d4_apply(tiles_u8, code).contiguous()          # exact: a permutation of the bytes
        d, i = nearest(descriptors(t, index.factor), index, k)
        ds.append(d.cpu().numpy())
        ixs.append(i.cpu().numpy())
    return (ds[0], ixs[0]) if len(ds) == 1 else merge_symmetries(ds, ixs, k)


def audit(generated_u8, index, k=4, d4=False, heldout_u8=None):
    """Audit uint8 [G][C][S][S] generated tiles (export.tiles_u8(layout="nchw")) against a TrainIndex: an AuditResult.

    ``loo_d2`` is one more search over the distinct matched training rows with ``exclude`` set to their own index.  A sample is
    ``copied`` when it is closer to a training tile than any other training tile is.  d4=True: every generated (and held-out) tile
    is searched under all eight symmetries of the square -- training under ``--augment d4`` can return a memorised tile rotated --
    and the eight lists are merged on the host.  heldout_u8: real tiles the generator never saw; ``closer_than_heldout`` compares
    the two sets' nearest-training distances.

    READING copy_rate: a sample drawn from the training distribution itself is flagged about half of the time -- its distance to
    the nearest training tile and that tile's distance to its own neighbour are then two draws of one distribution -- so a
    generator that does not memorise sits near 0.5 (below it while its samples are still far from the data) and copying pushes the
    rate towards 1.  A blurry, mean-like sample is closer to every tile than tiles are to each other and is flagged as well, so
    read the rate next to the distances themselves.  ``closer_than_heldout`` calibrates the same question against real tiles the generator never saw.

    EXACT DUPLICATES: an exact duplicate pair inside the training set has loo_d2 = 0, so a copy of either is never flagged by
    ``copied`` (nothing is below 0); it shows in d2 == 0, which is reported separately as ``exact``."""
    if not isinstance(index, TrainIndex):
        raise TypeError("index must be a TrainIndex")
    k = int(k)
    if len(index) < max(k, 2):
        raise ValueError("an audit needs at least max(k, 2) training tiles")
    d2, ix = _search(generated_u8, index, k, d4)
    matched, inverse = np.unique(ix[:, 0], return_inverse=True)
    loo, _ = nearest(index.rows(matched), index, 1, exclude=torch.from_numpy(matched))
    loo_d2 = loo.cpu().numpy()[:, 0][inverse.reshape(-1)]
    held = None
    if heldout_u8 is not None:
        held = _search(heldout_u8, index, 1, d4)[0][:, 0]
    return AuditResult(d2, ix, loo_d2, held)
