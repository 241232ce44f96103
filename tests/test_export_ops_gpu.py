"""rg_tile_export_u8 (include/rnagan_hip.h) through ctypes, byte for byte against the numpy restatement of tests/export_refs.py
(pinned without a GPU by tests/test_export_refs_cpu.py), on both builds of the library.

The output lives inside a byte allocation filled with one pattern (a write outside the tensor changes it; a refused call leaves it
inside as well); the source lives inside a NaN-filled allocation, at a 16-byte-aligned offset and at an offset of one float, and
is checked to be unchanged.  Overruns would stay inside the allocations, so nothing can fault.
Sizes: 1 x 1 and 5 x 5 (scalar path), 16 x 16 (vector paths, less than one workgroup), 50 x 50 (W % 4 != 0 but H W % 4 == 0: the
interleaved form is scalar, the planar form vector), 64 x 64 (whole workgroups), 130 x 130 (more than one workgroup, ragged),
3 x 20 and 20 x 3 (W % 4 == 0 with an odd H; the reverse), 256 x 256 (the generator's size).  dst offsets 1..3 and the source
offset of one float take the scalar path at every size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
import export_refs as X

DEV = "cuda:0"
PATTERN = 0xA5
BEFORE, AFTER = 4096, 16384          # guard bytes around dst: more than a workgroup's reach (1024 quads x 4 bytes) on either side
SIZES = [(1, 1), (5, 5), (16, 16), (50, 50), (64, 64), (130, 130), (3, 20), (20, 3)]
LAYOUTS, ORDERS, RULES = ("nhwc", "nchw"), ("rgb", "bgr"), ("round", "trunc")
EINVAL, EUNSUPPORTED = -1, -2

_DATA = {}


def _data(N, C, H, W):
    """The source batch, computed once per shape and never modified: N(0, 0.7) draws, the edge values of the contract in front
    where they fit."""
    key = (N, C, H, W)
    if key not in _DATA:
        rng = np.random.default_rng([17, N, C, H, W])
        a = (rng.standard_normal(N * C * H * W) * 0.7).astype(np.float32)
        e = X.edge_values()
        if e.size <= a.size:
            a[:e.size] = e
        a = a.reshape(N, C, H, W)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def _minmax(x):
    fin = x[np.isfinite(x)]
    lo, hi = float(fin.min()), float(fin.max())
    return lo, max(hi - lo, 1e-5)


class Src:
    """The source inside a NaN-filled allocation: float_offset 0 -> 16-byte aligned, 1 -> one float behind a boundary."""

    def __init__(self, x, float_offset=0):
        self.x = x
        self.before = 128 + float_offset
        self.flat = torch.full((self.before + x.size + 4096,), float("nan"), dtype=torch.float32, device=DEV)
        self.flat[self.before:self.before + x.size] = torch.from_numpy(x.reshape(-1).copy()).to(DEV)
        self.ptr = self.flat.data_ptr() + 4 * self.before
        assert self.ptr % 16 == (4 * float_offset) % 16

    def unchanged(self):
        got = self.flat.cpu().numpy().view(np.uint32)
        want = np.full(got.shape, np.float32("nan")).view(np.uint32)
        want[self.before:self.before + self.x.size] = self.x.reshape(-1).view(np.uint32)
        return np.array_equal(got, want)


class Dst:
    """n output bytes inside a PATTERN-filled byte allocation, `offset` bytes behind a 256-byte boundary."""

    def __init__(self, n, offset=0):
        self.n, self.before = n, BEFORE + offset
        self.flat = torch.full((self.before + n + AFTER,), PATTERN, dtype=torch.uint8, device=DEV)
        self.ptr = self.flat.data_ptr() + self.before
        assert self.ptr % 256 == offset

    def refill(self):
        self.flat.fill_(PATTERN)

    def read(self):
        """(the output bytes, whether the surroundings kept the pattern)"""
        a = self.flat.cpu().numpy()
        keep = bool((a[:self.before] == PATTERN).all()) and bool((a[self.before + self.n:] == PATTERN).all())
        return a[self.before:self.before + self.n].copy(), keep


def _launch(lib, src, dst, shape, sub, div, flags, stream=None):
    N, C, H, W = shape
    return lib.rg_tile_export_u8(src.ptr, dst.ptr, N, C, H, W, sub, div, flags, None if stream is None else stream.cuda_stream)


def _sweep(lib, x, src_offsets=(0, 1), dst_offsets=(0, 1, 2, 3), pairs=None):
    """Every layout, order and rule at every placement, against the restatement."""
    pairs = pairs or ((-1.0, 2.0), _minmax(x))
    want = {(l, o, r, p): X.tile_export_ref(x, l, o, r, *p).reshape(-1) for l in LAYOUTS for o in ORDERS for r in RULES for p in pairs}
    for so in src_offsets:
        src = Src(x, so)
        for do in dst_offsets:
            dst = Dst(x.size, do)
            for (l, o, r, p), w in want.items():
                dst.refill()
                rc = _launch(lib, src, dst, x.shape, p[0], p[1], X.flags_of(l, o, r))
                torch.cuda.synchronize()
                assert rc == 0, lib.rg_last_error()
                got, keep = dst.read()
                assert keep, "rg_tile_export_u8 wrote outside dst: %s" % ((x.shape, so, do, l, o, r),)
                bad = np.flatnonzero(got != w)
                assert bad.size == 0, "%s: %d of %d bytes differ, first at %d: got %d want %d" % (
                    (x.shape, so, do, l, o, r, p), bad.size, w.size, bad[0], got[bad[0]], w[bad[0]])
        assert src.unchanged(), "the source or its surroundings were written"


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H,W", SIZES)
def test_bytes_equal_the_restatement(H, W, C):
    lib = _abi.load()
    for N in (1, 5):
        _sweep(lib, _data(N, C, H, W))


def test_generator_size():
    _sweep(_abi.load(), _data(2, 3, 256, 256), dst_offsets=(0, 3))


def test_threshold_values():
    """Every byte's transform value, rounding threshold and truncation threshold with their +-1 and +-2 ulp neighbours, the
    out-of-range values, the infinities, NaN and the two zeros: on the vector paths and (dst offset 1) on the scalar path."""
    e = X.edge_values()
    x = _data(1, 3, 36, 40)
    assert x.size >= e.size and np.array_equal(x.reshape(-1)[:e.size].view(np.uint32), e.view(np.uint32))
    assert np.isnan(x).any() and np.isinf(x).any()
    _sweep(_abi.load(), x, src_offsets=(0,), dst_offsets=(0, 1), pairs=((-1.0, 2.0), (0.0, 1.0), (-1.0, 2.0000002)))


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_transform_then_export_returns_the_bytes(half):
    """(-1, 2) with the rounding rule on rg_tile_transform's output of all byte values returns the bytes; the truncating rule
    returns exactly the stated 63 one lower."""
    lib = _abi.load(half)
    b = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    d = torch.from_numpy(b).to(DEV)
    y = torch.empty(b.shape, dtype=torch.float32, device=DEV)
    assert lib.rg_tile_transform(d.data_ptr(), _abi.RG_U8, y.data_ptr(), 1, 1, 16, None, 0.5, 0.5, None) == 0, lib.rg_last_error()
    out = torch.full((2, 256), PATTERN, dtype=torch.uint8, device=DEV)
    assert lib.rg_tile_export_u8(y.data_ptr(), out[0].data_ptr(), 1, 1, 16, 16, -1.0, 2.0, 0, None) == 0, lib.rg_last_error()
    assert lib.rg_tile_export_u8(y.data_ptr(), out[1].data_ptr(), 1, 1, 16, 16, -1.0, 2.0, X.TRUNC, None) == 0, lib.rg_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[0], b.reshape(-1))
    lower = np.flatnonzero(got[1] != b.reshape(-1))
    assert tuple(int(k) for k in lower) == X.TRUNC_ONE_LOWER
    assert np.array_equal(got[1][lower].astype(np.int64), lower - 1)


def test_fp16_build():
    lib = _abi.load("f16")
    for shape in ((5, 3, 16, 16), (1, 4, 5, 5)):
        _sweep(lib, _data(*shape), dst_offsets=(0, 1))


def test_empty_batch_side_stream_and_graph_replay():
    lib = _abi.load()
    x = _data(5, 3, 64, 64)
    src, dst = Src(x), Dst(x.size)
    assert lib.rg_tile_export_u8(src.ptr, dst.ptr, 0, 3, 64, 64, -1.0, 2.0, 0, None) == 0             # N == 0: RG_OK, no launch
    torch.cuda.synchronize()
    assert bool((dst.flat == PATTERN).all())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for flags, (l, o, r) in ((0, ("nhwc", "rgb", "round")), (7, ("nchw", "bgr", "trunc"))):
        dst.refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert _launch(lib, src, dst, x.shape, -1.0, 2.0, flags, stream=side) == 0, lib.rg_last_error()
        side.synchronize()
        got, keep = dst.read()
        assert keep and np.array_equal(got, X.tile_export_ref(x, l, o, r).reshape(-1))
    # graph replay == eager
    eager = {}
    for flags in (0, 1, 2):
        dst.refill()
        assert _launch(lib, src, dst, x.shape, -1.0, 2.0, flags) == 0
        torch.cuda.synchronize()
        eager[flags] = dst.read()[0]
    outs = {f: Dst(x.size) for f in eager}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        st = torch.cuda.current_stream()
        for f, d in outs.items():
            assert _launch(lib, src, d, x.shape, -1.0, 2.0, f, stream=st) == 0, lib.rg_last_error()
    for _ in range(2):
        for d in outs.values():
            d.refill()
        graph.replay()
        torch.cuda.synchronize()
        for f, d in outs.items():
            got, keep = d.read()
            assert keep and np.array_equal(got, eager[f]), f
    assert src.unchanged()


def test_refused_arguments_write_nothing():
    lib = _abi.load()
    x = _data(2, 3, 8, 8)
    src, dst = Src(x), Dst(x.size)
    s, d = src.ptr, dst.ptr
    nan = float("nan")
    bad = [(None, d, 2, 3, 8, 8, -1.0, 2.0, 0), (s, None, 2, 3, 8, 8, -1.0, 2.0, 0), (s, d, -1, 3, 8, 8, -1.0, 2.0, 0),
           (s, d, 2, 0, 8, 8, -1.0, 2.0, 0), (s, d, 2, -3, 8, 8, -1.0, 2.0, 0), (s, d, 2, 3, 0, 8, -1.0, 2.0, 0),
           (s, d, 2, 3, -8, 8, -1.0, 2.0, 0), (s, d, 2, 3, 8, 0, -1.0, 2.0, 0), (s, d, 2, 3, 8, -8, -1.0, 2.0, 0),
           (s, d, 2, 3, 8, 8, -1.0, 0.0, 0), (s, d, 2, 3, 8, 8, -1.0, -0.0, 0), (s, d, 2, 3, 8, 8, -1.0, nan, 0),
           (s, d, 2, 3, 8, 8, -1.0, 2.0, 8), (s, d, 2, 3, 8, 8, -1.0, 2.0, -1), (s, d, 2, 3, 8, 8, -1.0, 2.0, 1 << 20),
           (s, d, 0, 0, 8, 8, -1.0, 2.0, 0)]
    for args in bad:
        assert lib.rg_tile_export_u8(*args, None) == EINVAL, args
        assert lib.rg_last_error()
    big = 2 ** 31 - 1
    for args in ((s, d, big, 1, 1, 257, -1.0, 2.0, 0),            # the scalar path: (2^31 - 1) * 257 / 256 workgroups
                 (s, d, big, 3, big, big, -1.0, 2.0, 0),          # a product past 2^64
                 (s, d, big, 3, 1 << 12, 1 << 12, -1.0, 2.0, 0), (s, d, big, 3, 1 << 12, 1 << 12, -1.0, 2.0, 1)):
        assert lib.rg_tile_export_u8(*args, None) == EUNSUPPORTED, args
        assert lib.rg_last_error()
    torch.cuda.synchronize()
    assert bool((dst.flat == PATTERN).all()), "a refused call wrote"
    assert src.unchanged()
