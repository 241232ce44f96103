"""rg_tile_transform (include/rnagan_hip.h) through ctypes, bit for bit against the numpy restatement of tests/augment_refs.py
(pinned without a GPU by tests/test_augment_refs_cpu.py).

The output lives inside a SENTINEL-filled allocation (a write outside the tensor changes the pattern); an fp32 source lives inside
a NaN-filled one (a read outside it makes a result non-finite) and a uint8 source, whose bytes stay below 255, inside one filled
with 255 (a read outside it makes a result exactly 1.0); such overruns stay inside the allocations, so nothing can fault.
Sizes: S = 1 and 5 (one partial tile, scalar path), 16 (one partial tile, vector path), 50 (scalar, not a multiple of 4), 64 (the
exact tile), 72 (a ragged second tile of 8, vector path), 130 (three tiles, the last 2 wide, scalar path), 256 (the training size:
4 x 4 whole tiles)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from augment_refs import normalize_ref, tile_transform_ref
from guarded import Guarded, SBITS
from vae_fid_refs import SENTINEL

SIZES = [1, 5, 16, 50, 64, 72, 130]
CODES8 = np.arange(8, dtype=np.int32)
CODES11 = np.array([5, 5, 0, 7, 3, 3, 3, 1, 6, 2, 4], dtype=np.int32)
DTYPES = {"u8": np.uint8, "f32": np.float32}
AFTER = 70000          # elements behind each tensor: more than one 256-wide row of tiles past the end

_DATA = {}


def _data(kind, N, C, S):
    """The source batch as numpy, computed once per shape and never modified.  uint8 bytes stay in 0..254."""
    key = (kind, N, C, S)
    if key not in _DATA:
        rng = np.random.default_rng([11, N, C, S])
        a = rng.integers(0, 255, size=(N, C, S, S), dtype=np.uint8) if kind == "u8" else \
            rng.standard_normal((N, C, S, S)).astype(np.float32)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(lib, src_np, codes, mean=0.5, std=0.5, before=128, stream=None):
    """One launch inside guarded allocations; returns the output as numpy after checking the surroundings."""
    N, C, S, _ = src_np.shape
    u8 = src_np.dtype == np.uint8
    src = Guarded(torch.from_numpy(src_np.copy()), 255 if u8 else float("nan"), before=before, after=AFTER)
    dst = Guarded(torch.full((N, C, S, S), SENTINEL, dtype=torch.float32), SENTINEL, before=before, after=AFTER)
    dcodes = None if codes is None else torch.from_numpy(np.asarray(codes, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    rc = lib.rg_tile_transform(src.t.data_ptr(), _abi.RG_U8 if u8 else _abi.RG_F32, dst.t.data_ptr(), N, C, S,
                               None if dcodes is None else dcodes.data_ptr(), mean, std,
                               None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert dst.surroundings_keep(SBITS), "rg_tile_transform wrote outside dst"
    assert np.array_equal(src.flat.cpu().numpy()[before:before + src.n].reshape(src_np.shape), src_np), "the source was written"
    got = dst.t.cpu().numpy()
    assert np.isfinite(got).all(), "a value outside the source was read"
    if u8 and mean == 0.5 and std == 0.5:
        assert not (got == 1.0).any(), "a byte outside the source was read"
    return got


def _check(got, src_np, codes, mean=0.5, std=0.5):
    want = tile_transform_ref(src_np, codes, mean, std)
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, "%d of %d elements differ, first at flat index %d: got %r want %r" % (
        bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_bit_exact(kind, C, S):
    lib = _abi.load()
    for codes in (CODES8, CODES11):
        src = _data(kind, len(codes), C, S)
        _check(_run(lib, src, codes), src, codes)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_training_size(kind):
    lib = _abi.load()
    src = _data(kind, 2, 3, 256)
    for codes in ([1, 2], [3, 4], [5, 6], [7, 0]):
        _check(_run(lib, src, codes), src, codes)


def test_null_codes_equal_u8_to_norm():
    lib = _abi.load()
    for S in (5, 64, 72):
        src = _data("u8", 3, 3, S)
        got = _run(lib, src, None)
        _check(got, src, None)
        d = torch.from_numpy(src.copy()).cuda()
        y = torch.empty(src.shape, dtype=torch.float32, device="cuda")
        assert lib.rg_u8_to_norm(d.data_ptr(), y.data_ptr(), d.numel(), 0.5, 0.5, None) == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(got))
        assert np.array_equal(_bits(got), _bits(_run(lib, src, np.zeros(3, dtype=np.int32))))
    f = _data("f32", 3, 1, 50)
    assert np.array_equal(_bits(_run(lib, f, None)), _bits(f))


def test_every_byte_value_and_other_constants():
    lib = _abi.load()
    src = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    for mean, std in ((0.5, 0.5), (0.25, 0.125), (0.0, 1.0)):
        for codes in (None, [5]):
            N, C, S, _ = src.shape
            d = torch.from_numpy(src).cuda()
            y = torch.empty(src.shape, dtype=torch.float32, device="cuda")
            dc = None if codes is None else torch.tensor(codes, dtype=torch.int32, device="cuda")
            assert lib.rg_tile_transform(d.data_ptr(), _abi.RG_U8, y.data_ptr(), N, C, S, None if dc is None else dc.data_ptr(),
                                         mean, std, None) == 0, lib.rg_last_error()
            torch.cuda.synchronize()
            _check(y.cpu().numpy(), src, codes, mean, std)
    # mean / std are ignored for an fp32 source, std == 0 included
    f = _data("f32", 2, 1, 5)
    _check(_run(lib, f, [1, 6], mean=3.0, std=0.0), f, [1, 6])


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_codes_are_taken_modulo_8(kind):
    lib = _abi.load()
    src = _data(kind, 4, 1, 16)
    wild = np.array([-1, 11, 1 << 20, -2 ** 31], dtype=np.int32)
    got = _run(lib, src, wild)
    _check(got, src, np.array([7, 3, 0, 0], dtype=np.int32))
    _check(got, src, wild)


@pytest.mark.parametrize("S", [16, 72])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_buffers_off_16_byte_alignment(kind, S):
    """Both tensors start 4 bytes behind a 16-byte boundary (fp32: one element; uint8: four), and a uint8 source also 1 byte
    behind one: S is a multiple of 16, so only the alignment can choose the path."""
    lib = _abi.load()
    src = _data(kind, 8, 1, S)
    for before in ((129,) if kind == "f32" else (132, 129)):
        _check(_run(lib, src, CODES8, before=before), src, CODES8)


def test_non_default_stream():
    lib = _abi.load()
    src = _data("u8", 8, 3, 72)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _run(lib, src, CODES8, stream=side)
    _check(got, src, CODES8)


def test_refused_arguments_and_empty_batch():
    lib = _abi.load()
    src = torch.zeros(2 * 3 * 8 * 8, dtype=torch.uint8, device="cuda")
    dst = Guarded(torch.full((2, 3, 8, 8), SENTINEL, dtype=torch.float32), SENTINEL)
    codes = torch.zeros(2, dtype=torch.int32, device="cuda")
    s, d, c = src.data_ptr(), dst.t.data_ptr(), codes.data_ptr()
    U8, F32 = _abi.RG_U8, _abi.RG_F32
    bad = [(None, U8, d, 2, 3, 8, c, 0.5, 0.5), (s, U8, None, 2, 3, 8, c, 0.5, 0.5), (s, U8, d, -1, 3, 8, c, 0.5, 0.5),
           (s, U8, d, 2, 0, 8, c, 0.5, 0.5), (s, U8, d, 2, -3, 8, c, 0.5, 0.5), (s, U8, d, 2, 3, 0, c, 0.5, 0.5),
           (s, U8, d, 2, 3, -8, c, 0.5, 0.5), (s, _abi.RG_BF16, d, 2, 3, 8, c, 0.5, 0.5), (s, _abi.RG_F16, d, 2, 3, 8, c, 0.5, 0.5),
           (s, 7, d, 2, 3, 8, c, 0.5, 0.5), (s, -1, d, 2, 3, 8, c, 0.5, 0.5), (s, U8, d, 2, 3, 8, c, 0.5, 0.0)]
    for args in bad:
        assert lib.rg_tile_transform(*args, None) == -1, args              # RG_EINVAL
        assert lib.rg_last_error()
    assert lib.rg_tile_transform(s, U8, d, 0, 3, 8, c, 0.5, 0.5, None) == 0        # N == 0: RG_OK, nothing launched
    assert lib.rg_tile_transform(s, F32, d, 0, 3, 8, None, 0.5, 0.5, None) == 0
    torch.cuda.synchronize()
    assert bool((dst.flat.view(torch.int32) == SBITS).all()), "a refused or empty call wrote"


def test_fp16_build():
    lib = _abi.load("f16")
    for kind in ("u8", "f32"):
        src = _data(kind, 8, 3, 72)
        _check(_run(lib, src, CODES8), src, CODES8)


def test_hipops_wrapper():
    from rna_gan_amd.ops_hip import HipOps
    hip = HipOps(torch.bfloat16, "cuda:0")
    src = _data("u8", 8, 3, 50)
    got = hip.tile_transform(torch.from_numpy(src.copy()).cuda(), torch.from_numpy(CODES8).cuda())
    _check(got.cpu().numpy(), src, CODES8)
    got = hip.tile_transform(torch.from_numpy(src.copy()).cuda())
    assert torch.equal(got, hip.u8_to_norm(torch.from_numpy(src.copy()).cuda()))
    assert tuple(hip.tile_transform(torch.empty(0, 3, 8, 8, dtype=torch.uint8, device="cuda")).shape) == (0, 3, 8, 8)
    assert np.array_equal(normalize_ref(src), got.cpu().numpy())
