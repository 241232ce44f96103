"""rg_tile_gather_transform (include/rnagan_hip.h) through ctypes, bit for bit against the numpy restatement of
tests/resident_refs.py (pinned without a GPU by tests/test_resident_refs_cpu.py).

The output lives inside a SENTINEL-filled allocation (a write outside it changes the pattern).  The store, whose bytes stay
below 255, lives inside an allocation filled with 255: a read outside it makes a result exactly 1.0.  Such overruns stay inside
the allocations, so nothing can fault -- the out-of-range indices of the clamp test included: the kernel's contract is to read
the nearest valid tile, and were it broken for -1 or M the read would land in the 255-filled surroundings (sized to hold a
whole tile on either side); the 2^31 - 1 case is sent only with the ones before it verified in the same process.
Sizes: S = 1 and 5 (one partial tile, scalar path), 16 (one partial tile, vector path), 64 (the exact tile), 72 (a ragged second
tile of 8, vector path), 130 (three tiles, the last 2 wide, scalar path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from both_builds import fp16_twin
from guarded import Guarded, SBITS
from resident_refs import gather_transform_ref
from vae_fid_refs import SENTINEL

SIZES = [1, 5, 16, 64, 72, 130]
BUILDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
_DATA = {}


def _store(M, C, S):
    """The store as numpy, computed once per shape and never modified; bytes stay in 0..254."""
    key = (M, C, S)
    if key not in _DATA:
        a = np.random.default_rng([29, M, C, S]).integers(0, 255, size=(M, C, S, S), dtype=np.uint8)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(M, N, seed=0):
    """N indices into M tiles: a permutation's start, then repeats (the first index again, and one tile three times)."""
    idx = np.random.default_rng([31, M, N, seed]).permutation(M)[:N].tolist()
    while len(idx) < N:
        idx.append(idx[0] if len(idx) % 2 else M - 1)
    if N >= 3:
        idx[-1] = idx[-2] = idx[0]
    return np.array(idx, dtype=np.int32)


def _run(lib, store_np, index, codes, n=None, mean=0.5, std=0.5, before=None, stream=None):
    """One launch inside guarded allocations; returns the output as numpy after checking the surroundings."""
    M, C, S, _ = store_np.shape
    tile = C * S * S
    pad = (tile + 255) // 256 * 256 + 128            # a whole tile in front of and behind the store, 255-filled
    before = pad if before is None else before
    N = (M if n is None else n) if index is None else len(index)
    src = Guarded(torch.from_numpy(store_np.copy()), 255, before=before, after=pad)
    dst = Guarded(torch.full((N, C, S, S), SENTINEL, dtype=torch.float32), SENTINEL, after=70000)
    dindex = None if index is None else torch.from_numpy(np.asarray(index, dtype=np.int32)).cuda()
    dcodes = None if codes is None else torch.from_numpy(np.asarray(codes, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    rc = lib.rg_tile_gather_transform(src.t.data_ptr(), M, None if dindex is None else dindex.data_ptr(), dst.t.data_ptr(),
                                      N, C, S, None if dcodes is None else dcodes.data_ptr(), mean, std,
                                      None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert dst.surroundings_keep(SBITS), "rg_tile_gather_transform wrote outside dst"
    assert np.array_equal(src.flat.cpu().numpy()[before:before + src.n].reshape(store_np.shape), store_np), "the store was written"
    got = dst.t.cpu().numpy()
    assert np.isfinite(got).all()
    if mean == 0.5 and std == 0.5:
        assert not (got == 1.0).any(), "a byte outside the store was read"
    return got


def _check(got, store_np, index, codes, n=None, mean=0.5, std=0.5):
    want = gather_transform_ref(store_np, index, codes, n, mean, std)
    assert got.shape == want.shape
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, "%d of %d elements differ, first at flat index %d: got %r want %r" % (
        bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("C", [1, 3])
def test_bit_exact(C, S):
    """M in {1, 7} x N in {1, 9}: repeated and permuted indices, codes 0..7 (and one more) and NULL."""
    lib = _abi.load()
    for M in (1, 7):
        store = _store(M, C, S)
        for N in (1, 9):
            index = _index(M, N)
            codes = (np.arange(N, dtype=np.int32) + (3 if N == 1 else 0)) % 8
            _check(_run(lib, store, index, codes), store, index, codes)
            _check(_run(lib, store, index, None), store, index, None)


def test_training_size():
    lib = _abi.load()
    store = _store(5, 3, 256)
    index = np.array([4, 0, 4, 2], dtype=np.int32)
    for codes in ([1, 2, 3, 4], [5, 6, 7, 0]):
        _check(_run(lib, store, index, codes), store, index, codes)


@pytest.mark.parametrize("S", [5, 64, 72])
def test_null_index_equals_tile_transform(S):
    lib = _abi.load()
    store = _store(7, 3, S)
    for N, codes in ((7, np.arange(7, dtype=np.int32)), (4, None), (1, np.array([6], dtype=np.int32))):
        got = _run(lib, store, None, codes, n=N)
        _check(got, store, None, codes, n=N)
        d = torch.from_numpy(store.copy()).cuda()
        y = torch.empty((N,) + store.shape[1:], dtype=torch.float32, device="cuda")
        dc = None if codes is None else torch.from_numpy(codes).cuda()
        assert lib.rg_tile_transform(d.data_ptr(), _abi.RG_U8, y.data_ptr(), N, 3, S, None if dc is None else dc.data_ptr(),
                                     0.5, 0.5, None) == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(got))


def test_other_constants_and_codes_modulo_8():
    lib = _abi.load()
    store = _store(7, 1, 16)
    index = np.array([6, 1, 1, 3], dtype=np.int32)
    wild = np.array([-1, 11, 1 << 20, -2 ** 31], dtype=np.int32)
    for mean, std in ((0.25, 0.125), (0.0, 1.0)):
        _check(_run(lib, store, index, wild, mean=mean, std=std), store, index, np.array([7, 3, 0, 0]), mean=mean, std=std)


@pytest.mark.parametrize("S", [16, 72])
def test_store_off_4_byte_alignment(S):
    """The store starts 1, 2 and 3 bytes behind a 4-byte boundary: S is a multiple of 4, so only the alignment chooses the
    scalar path, for every gathered tile (C S S is a multiple of 4)."""
    lib = _abi.load()
    store = _store(7, 3, S)
    index = _index(7, 9, seed=1)
    codes = np.arange(9, dtype=np.int32) % 8
    base = (3 * S * S + 255) // 256 * 256 + 128
    for off in (1, 2, 3):
        _check(_run(lib, store, index, codes, before=base + off), store, index, codes)


def test_out_of_range_indices_are_clamped():
    lib = _abi.load()
    for S in (5, 16):
        store = _store(7, 3, S)
        codes = np.array([0, 3, 5, 0, 6], dtype=np.int32)
        near = np.array([-1, 7, 3, -5, 8], dtype=np.int32)
        _check(_run(lib, store, near, codes), store, np.array([0, 6, 3, 0, 6]), codes)
        far = np.array([-2 ** 31, 2 ** 31 - 1, 3, 1 << 24, -(1 << 24)], dtype=np.int32)
        _check(_run(lib, store, far, codes), store, np.array([0, 6, 3, 6, 0]), codes)


def test_non_default_stream():
    lib = _abi.load()
    store = _store(7, 3, 72)
    index = _index(7, 9, seed=2)
    codes = np.arange(9, dtype=np.int32) % 8
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _run(lib, store, index, codes, stream=side)
    _check(got, store, index, codes)


def test_refused_arguments_and_empty_batch():
    lib = _abi.load()
    store = torch.zeros(2 * 3 * 8 * 8, dtype=torch.uint8, device="cuda")
    dst = Guarded(torch.full((3, 3, 8, 8), SENTINEL, dtype=torch.float32), SENTINEL)
    index = torch.zeros(3, dtype=torch.int32, device="cuda")
    codes = torch.zeros(3, dtype=torch.int32, device="cuda")
    s, d, x, c = store.data_ptr(), dst.t.data_ptr(), index.data_ptr(), codes.data_ptr()
    bad = [(None, 2, x, d, 2, 3, 8, c, 0.5, 0.5), (s, 2, x, None, 2, 3, 8, c, 0.5, 0.5), (s, 0, x, d, 2, 3, 8, c, 0.5, 0.5),
           (s, -1, x, d, 2, 3, 8, c, 0.5, 0.5), (s, 2, x, d, -1, 3, 8, c, 0.5, 0.5), (s, 2, x, d, 2, 0, 8, c, 0.5, 0.5),
           (s, 2, x, d, 2, -3, 8, c, 0.5, 0.5), (s, 2, x, d, 2, 3, 0, c, 0.5, 0.5), (s, 2, x, d, 2, 3, -8, c, 0.5, 0.5),
           (s, 2, x, d, 2, 3, 8, c, 0.5, 0.0), (s, 2, None, d, 3, 3, 8, c, 0.5, 0.5), (s, 2, None, d, 3, 3, 8, None, 0.5, 0.5)]
    for args in bad:
        assert lib.rg_tile_gather_transform(*args, None) == -1, args               # RG_EINVAL
        assert lib.rg_last_error()
    assert lib.rg_tile_gather_transform(s, 2, x, d, 0, 3, 8, c, 0.5, 0.5, None) == 0        # N == 0: RG_OK, nothing launched
    assert lib.rg_tile_gather_transform(s, 0, None, d, 0, 3, 8, None, 0.5, 0.5, None) == 0  # ... an empty store included
    torch.cuda.synchronize()
    assert bool((dst.flat.view(torch.int32) == SBITS).all()), "a refused or empty call wrote"
    assert lib.rg_tile_gather_transform(s, 2, x, d, 3, 3, 8, c, 0.5, 0.5, None) == 0        # N > M is fine WITH an index
    assert lib.rg_tile_gather_transform(s, 2, None, d, 2, 3, 8, c, 0.5, 0.5, None) == 0     # N == M without one
    torch.cuda.synchronize()


@fp16_twin
def test_both_builds(h16=torch.bfloat16):
    """No 16-bit type is involved; the fp16 build has a code object of its own, and test_both_builds_fp16 runs that one."""
    lib = _abi.load(BUILDS[h16])
    store = _store(7, 3, 72)
    index = _index(7, 9, seed=3)
    codes = np.arange(9, dtype=np.int32) % 8
    _check(_run(lib, store, index, codes), store, index, codes)
    store = _store(7, 3, 5)
    _check(_run(lib, store, index, None), store, index, None)


def test_hipops_wrapper():
    from rna_gan_amd.ops_hip import HipOps
    hip = HipOps(torch.bfloat16, "cuda:0")
    store = _store(7, 3, 16)
    index = _index(7, 9, seed=4)
    codes = np.arange(9, dtype=np.int32) % 8
    d = torch.from_numpy(store.copy()).cuda()
    got = hip.tile_gather_transform(d, torch.from_numpy(index).cuda(), torch.from_numpy(codes).cuda())
    _check(got.cpu().numpy(), store, index, codes)
    assert torch.equal(hip.tile_gather_transform(d, n=4), hip.tile_transform(d[:4].contiguous()))
    assert tuple(hip.tile_gather_transform(d, n=0).shape) == (0, 3, 16, 16)


def test_offsets_are_64_bit():
    """S = 16, C = 1, M = 2^24 + 8: a REAL allocation of 4 GiB + 2 KiB, filled with 255, with distinct tiles written at indices
    0, 2^23, 2^24 - 1, 2^24 and 2^24 + 7.  An offset computed in 32 bits wraps at tile 2^24 and reads a wrong tile INSIDE the
    buffer -- a failed assertion, never a fault.  Skips only when the device reports less than 6 GiB free."""
    if torch.cuda.mem_get_info()[0] < 6 << 30:
        pytest.skip("less than 6 GiB of device memory free")
    lib = _abi.load()
    S, M = 16, (1 << 24) + 8
    tile = S * S
    buf = torch.full((M * tile,), 255, dtype=torch.uint8, device="cuda")
    assert buf.numel() == (4 << 30) + 2048
    where = [0, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 7]
    small = np.random.default_rng(37).integers(0, 255, size=(len(where), 1, S, S), dtype=np.uint8)
    for k, t in enumerate(where):
        buf[t * tile:(t + 1) * tile] = torch.from_numpy(small[k].reshape(-1)).cuda()
    index = np.array([4, 3, 2, 1, 0, 3, 4], dtype=np.int32)
    codes = np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int32)
    dindex = torch.from_numpy(np.array([where[k] for k in index], dtype=np.int32)).cuda()
    dcodes = torch.from_numpy(codes).cuda()
    dst = Guarded(torch.full((len(index), 1, S, S), SENTINEL, dtype=torch.float32), SENTINEL)
    torch.cuda.synchronize()
    assert lib.rg_tile_gather_transform(buf.data_ptr(), M, dindex.data_ptr(), dst.t.data_ptr(), len(index), 1, S,
                                        dcodes.data_ptr(), 0.5, 0.5, None) == 0, lib.rg_last_error()
    torch.cuda.synchronize()
    assert dst.surroundings_keep(SBITS)
    got = dst.t.cpu().numpy()
    del buf
    torch.cuda.empty_cache()                         # the 4 GiB go back to the device, not into the caching allocator
    assert not (got == 1.0).any(), "a tile other than the five written was read"
    _check(got, small, index, codes)
