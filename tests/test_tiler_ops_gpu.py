"""rg_window_resize_u8, rg_mask_erode and rg_box_reduce_u8 (include/rnagan_hip.h) through ctypes: every byte EQUAL to the numpy
restatements of tests/tiler_refs.py, which tests/test_tiler_refs_cpu.py pins to PIL.Image.resize and scipy without a GPU.

Every output lives inside a larger allocation filled with one pattern (tests/guarded.py): a write outside it changes the pattern, a
refused call leaves it inside as well.  Overruns would stay inside the allocations, so nothing can fault.  The rasters are small
except one: 37 838 x 37 838 x 3 bytes, just over 2^32, uninitialised but for a patch at its far end, where 32-bit byte offsets would
wrap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from rna_gan_amd import tiler as TL
from guarded import DEV, Guarded
import tiler_refs as R

PATTERN = 0xA5
EINVAL, EUNSUPPORTED = -1, -2


def _kept(g):
    return bool((g.flat[:g.before] == PATTERN).all()) and bool((g.flat[g.before + g.n:] == PATTERN).all())


def _guarded(shape):
    return Guarded(torch.full(shape, PATTERN, dtype=torch.uint8), PATTERN)


def _tables(h, w, oh, ow):
    """(xtab, kx, ytab, ky) on the device; None / 0 for an axis that is copied"""
    xt = None if w == ow else torch.from_numpy(R.table_ref(w, ow)).to(DEV)
    yt = None if h == oh else torch.from_numpy(R.table_ref(h, oh)).to(DEV)
    return xt, (0 if xt is None else xt.shape[1] - 2), yt, (0 if yt is None else yt.shape[1] - 2)


class Raster:
    """a raster inside a larger device buffer, `offset` bytes behind a 256-byte boundary"""

    def __init__(self, a, offset=0):
        self.a = a
        self.buf = torch.full((256 + a.size + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        self.at = 256 + offset
        assert (self.buf.data_ptr() + self.at) % 4 == offset % 4
        self.buf[self.at:self.at + a.size] = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
        self.ptr = self.buf.data_ptr() + self.at


def _run(lib, raster, origins, h, w, oh, ow, flags=0, out=None, stream=None, origins_dev=None, tables=None):
    o = torch.tensor(origins, dtype=torch.int32, device=DEV).reshape(-1, 2) if origins_dev is None else origins_dev
    out = _guarded((o.shape[0], oh, ow, 3)) if out is None else out
    xt, kx, yt, ky = _tables(h, w, oh, ow) if tables is None else tables
    rc = lib.rg_window_resize_u8(raster.ptr, raster.a.shape[0], raster.a.shape[1], o.data_ptr(), o.shape[0], h, w, oh, ow,
                                 None if xt is None else xt.data_ptr(), kx, None if yt is None else yt.data_ptr(), ky,
                                 out.t.data_ptr(), flags, None if stream is None else stream.cuda_stream)
    return rc, out, (o, xt, yt)


def _read(out, what):
    torch.cuda.synchronize()
    assert _kept(out), "%s: written outside out" % (what,)
    return out.t.cpu().numpy().copy()


def _same(got, want, what):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %d (got %d, want %d)" % (
        what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ------------------------------------------------------------------ rg_window_resize_u8
@pytest.mark.parametrize("case", R.SIZE_CASES)
def test_windows_equal_the_restatement(case):
    """every size case at every window position: inside, across each edge and corner, wholly outside, negative origins, overlapping;
    random bytes and 0 / 255 (sums that clip at both ends); both channel orders"""
    lib = _abi.load()
    h, w, oh, ow = case
    RH, RW = h + 13, w + 10
    pos = R.window_positions(RH, RW, h, w)
    for kind in ("bytes", "binary"):
        a = R.content(kind, RH, RW, seed=1)
        want = R.windows_ref(a, pos, h, w, oh, ow)
        raster = Raster(a)
        for flags in (0, R.REVERSE):
            rc, out, _ = _run(lib, raster, pos, h, w, oh, ow, flags)
            assert rc == 0, lib.rg_last_error()
            _same(_read(out, case), want[..., ::-1] if flags else want, (case, kind, flags))
    white = Raster(R.content("white", RH, RW))
    rc, out, _ = _run(lib, white, [(3, 2), (5, 4)], h, w, oh, ow)
    assert rc == 0 and bool((_read(out, case) == 255).all())


@pytest.mark.parametrize("case", R.BIG_CASES)
def test_the_two_production_sizes(case):
    lib = _abi.load()
    h, w, oh, ow = case
    RH, RW = 900, 1000
    a = R.content("bytes", RH, RW, seed=2)
    a[:300, :400] = R.content("binary", 300, 400, seed=2)
    pos = [(0, 0), (RW - w // 2, RH - h // 3), (-100, -200), (37, 101)]
    want = R.windows_ref(a, pos, h, w, oh, ow)
    rc, out, _ = _run(lib, Raster(a), pos, h, w, oh, ow)
    assert rc == 0, lib.rg_last_error()
    _same(_read(out, case), want, case)


def test_one_window_many_windows_and_a_subset():
    lib = _abi.load()
    rng = np.random.default_rng(3)
    a = R.content("bytes", 90, 75, seed=3)
    raster = Raster(a)
    h, w, oh, ow = 32, 32, 16, 16
    pos = [(int(x), int(y)) for x, y in zip(rng.integers(-40, 85, 67), rng.integers(-40, 100, 67))]
    want = R.windows_ref(a, pos, h, w, oh, ow)
    rc, out, _ = _run(lib, raster, pos, h, w, oh, ow)
    assert rc == 0, lib.rg_last_error()
    full = _read(out, "N = 67")
    _same(full, want, "N = 67")
    rc, out, _ = _run(lib, raster, pos[:1], h, w, oh, ow)
    assert rc == 0
    _same(_read(out, "N = 1"), want[:1], "N = 1")
    pick = [5, 66, 0, 31, 31]
    rc, out, _ = _run(lib, raster, [pos[k] for k in pick], h, w, oh, ow)
    assert rc == 0
    _same(_read(out, "subset"), full[pick], "a subset of the windows")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_raster_off_the_dword_grid(offset):
    lib = _abi.load()
    RH, RW = 50, 61                                    # RW * 3 = 183: no row starts where the one before did, modulo 4
    a = R.content("bytes", RH, RW, seed=4)
    raster = Raster(a, offset)
    for (h, w, oh, ow) in ((8, 8, 8, 8), (37, 53, 16, 16), (48, 48, 16, 16)):
        pos = R.window_positions(RH, RW, h, w)
        rc, out, _ = _run(lib, raster, pos, h, w, oh, ow)
        assert rc == 0, lib.rg_last_error()
        _same(_read(out, offset), R.windows_ref(a, pos, h, w, oh, ow), (offset, h, w, oh, ow))


def test_a_raster_of_more_than_4_gib():
    """byte offsets at the far end exceed 2^32; only a 138 x 138 patch there is written, and no window reads outside it (except
    beyond the raster, where zeros are read)"""
    lib = _abi.load()
    S, P = 37838, 138
    assert S * S * 3 > 1 << 32
    big = torch.empty((S, S, 3), dtype=torch.uint8, device=DEV)
    patch = R.content("bytes", P, P, seed=5)
    big[S - P:, S - P:] = torch.from_numpy(patch).to(DEV)

    class Far:
        a = np.empty((S, S, 0), dtype=np.uint8)        # the shape alone is used
        ptr = big.data_ptr()

    local = [(0, 0), (P - 64, P - 64), (P - 30, 40), (50, P - 10), (P - 1, P - 1), (P + 5, 3)]
    want = R.windows_ref(np.pad(patch, ((0, 64), (0, 64), (0, 0))), local, 64, 64, 32, 32)
    rc, out, _ = _run(lib, Far, [(x + S - P, y + S - P) for x, y in local], 64, 64, 32, 32)
    assert rc == 0, lib.rg_last_error()
    _same(_read(out, "4 GiB"), want, "the far end of a raster of more than 4 GiB")
    crop = R.windows_ref(np.pad(patch, ((0, 64), (0, 64), (0, 0))), local, 64, 64, 64, 64)
    rc, out, _ = _run(lib, Far, [(x + S - P, y + S - P) for x, y in local], 64, 64, 64, 64)
    assert rc == 0
    _same(_read(out, "4 GiB crop"), crop, "crops at the far end")


def test_fp16_build_side_stream_and_graph_replay():
    a = R.content("bytes", 60, 70, seed=6)
    raster = Raster(a)
    h, w, oh, ow = 37, 53, 16, 16
    pos = R.window_positions(60, 70, h, w)
    want = R.windows_ref(a, pos, h, w, oh, ow)
    rc, out, _ = _run(_abi.load("f16"), raster, pos, h, w, oh, ow)
    assert rc == 0
    _same(_read(out, "f16"), want, "fp16 build")
    lib = _abi.load()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc, out, keep = _run(lib, raster, pos, h, w, oh, ow, stream=side)
    side.synchronize()
    assert rc == 0
    _same(_read(out, "side"), want, "side stream")
    eager = _read(out, "eager")
    o, xt, yt = keep
    out.t.fill_(PATTERN)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        rc, _, _ = _run(lib, raster, None, h, w, oh, ow, out=out, stream=torch.cuda.current_stream(), origins_dev=o,
                        tables=(xt, xt.shape[1] - 2, yt, yt.shape[1] - 2))
        assert rc == 0, lib.rg_last_error()
    for _ in range(2):
        out.t.fill_(PATTERN)
        graph.replay()
        _same(_read(out, "replay"), eager, "graph replay")


def test_the_two_launch_probe_gives_the_same_bytes():
    """rg_probe_window_resize_2pass, what tools/ab_tiler.py measures the kernel against, computes the same thing"""
    lib = _abi.load()
    a = R.content("binary", 60, 70, seed=10)
    raster = Raster(a)
    for (h, w, oh, ow) in ((37, 53, 16, 16), (8, 8, 8, 8), (100, 40, 16, 48)):
        pos = R.window_positions(60, 70, h, w)
        o = torch.tensor(pos, dtype=torch.int32, device=DEV)
        xt, kx, yt, ky = _tables(h, w, oh, ow)
        out = _guarded((len(pos), oh, ow, 3))
        ws = _guarded((len(pos) * h * ow * 3,))
        for flags in (0, R.REVERSE):
            rc = lib.rg_probe_window_resize_2pass(raster.ptr, 60, 70, o.data_ptr(), len(pos), h, w, oh, ow,
                                                  None if xt is None else xt.data_ptr(), kx, None if yt is None else yt.data_ptr(), ky,
                                                  out.t.data_ptr(), flags, ws.t.data_ptr(), ws.n, None)
            assert rc == 0, lib.rg_last_error()
            want = R.windows_ref(a, pos, h, w, oh, ow, reverse=bool(flags))
            _same(_read(out, "2pass"), want, ("two launches", h, w, oh, ow, flags))
            assert _kept(ws)
        assert lib.rg_probe_window_resize_2pass(raster.ptr, 60, 70, o.data_ptr(), len(pos), h, w, oh, ow,
                                                None if xt is None else xt.data_ptr(), kx, None if yt is None else yt.data_ptr(), ky,
                                                out.t.data_ptr(), 0, ws.t.data_ptr(), ws.n - 1, None) == EINVAL


def test_python_functions_on_the_device_equal_the_cpu_path():
    a = R.content("bytes", 90, 75, seed=7)
    pos = R.window_positions(90, 75, 32, 48)
    cpu, dev = torch.from_numpy(a), torch.from_numpy(a).to(DEV)
    for read, size, order in (((32, 48), (16, 16), "rgb"), ((32, 48), (32, 48), "bgr"), ((32, 48), (40, 16), "bgr")):
        got = TL.resize_windows(dev, pos, read, size, order)
        assert got.is_cuda and torch.equal(got.cpu(), TL.resize_windows(cpu, pos, read, size, order)), (read, size, order)
    o = torch.tensor(pos, dtype=torch.int32, device=DEV)
    assert torch.equal(TL.resize_windows(dev, o, 32, 16).cpu(), TL.resize_windows(cpu, pos, 32, 16))
    assert tuple(TL.resize_windows(dev, [], 32, 16).shape) == (0, 16, 16, 3)
    assert torch.equal(TL.thumbnail(dev, 7).cpu(), TL.thumbnail(cpu, 7))
    m = torch.from_numpy(R.mask_cases(64, 65)["dense"])
    assert torch.equal(TL.erode(m.to(DEV), 3).cpu(), TL.erode(m, 3)) and tuple(TL.erode(m.to(DEV), 3).shape) == (64, 65)
    thumb = TL.thumbnail(torch.from_numpy(R.slide().copy()), 8)
    assert torch.equal(TL.slide_mask(thumb.to(DEV)).cpu(), TL.slide_mask(thumb))


# ------------------------------------------------------------------ rg_mask_erode
@pytest.mark.parametrize("shape", R.ERODE_SHAPES)
def test_erode_equals_the_restatement(shape):
    lib = _abi.load()
    H, W = shape
    cases = R.mask_cases(H, W)
    stack = np.stack(list(cases.values())[:3])
    src1 = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    src3 = torch.from_numpy(stack).to(DEV)
    out1, out3 = _guarded((1, H, W)), _guarded((3, H, W))
    for r in range(9):
        for name, m in cases.items():
            src1.copy_(torch.from_numpy(m))
            out1.t.fill_(PATTERN)
            assert lib.rg_mask_erode(src1.data_ptr(), out1.t.data_ptr(), 1, H, W, r, None) == 0, lib.rg_last_error()
            _same(_read(out1, (name, r))[0], R.erode_ref(m, r), (shape, name, r))
        out3.t.fill_(PATTERN)
        assert lib.rg_mask_erode(src3.data_ptr(), out3.t.data_ptr(), 3, H, W, r, None) == 0, lib.rg_last_error()
        _same(_read(out3, ("N = 3", r)), np.stack([R.erode_ref(m, r) for m in stack]), (shape, "N = 3", r))
    # any non-zero byte is set
    src1.copy_(torch.from_numpy(cases["holes"] * 200))
    assert lib.rg_mask_erode(src1.data_ptr(), out1.t.data_ptr(), 1, H, W, 1, None) == 0
    _same(_read(out1, "200")[0], R.erode_ref(cases["holes"], 1), (shape, "bytes of 200"))


# ------------------------------------------------------------------ rg_box_reduce_u8
@pytest.mark.parametrize("f", R.BOX_FACTORS)
def test_box_reduce_equals_the_restatement(f):
    lib = _abi.load()
    for (RH, RW, kind) in ((13, 29, "bytes"), (130, 67, "bytes"), (64, 128, "bytes"), (70, 33, "white")):
        a = R.content(kind, RH, RW, seed=8)
        raster = Raster(a, offset=1)
        want = R.box_ref(a, f)
        out = _guarded(want.shape)
        assert lib.rg_box_reduce_u8(raster.ptr, RH, RW, f, out.t.data_ptr(), None) == 0, lib.rg_last_error()
        got = _read(out, (RH, RW, f))
        _same(got, want, (RH, RW, f, kind))
        if kind == "white":
            assert bool((got == 255).all())


# ------------------------------------------------------------------ refusals
def test_refused_arguments_launch_nothing():
    lib = _abi.load()
    a = R.content("bytes", 40, 40, seed=9)
    raster = Raster(a)
    out = _guarded((2, 16, 16, 3))
    o = torch.tensor([(0, 0), (3, 3)], dtype=torch.int32, device=DEV)
    xt, kx, yt, ky = _tables(32, 32, 16, 16)
    r, op, x, y, dst = raster.ptr, o.data_ptr(), xt.data_ptr(), yt.data_ptr(), out.t.data_ptr()
    good = [r, 40, 40, op, 2, 32, 32, 16, 16, x, kx, y, ky, dst, 0]
    assert kx == ky == 9

    def call(**kw):
        names = ["raster", "RH", "RW", "origins", "N", "h", "w", "oh", "ow", "xtab", "kx", "ytab", "ky", "out", "flags"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.rg_window_resize_u8(*args, None)

    for kw in (dict(raster=None), dict(origins=None), dict(out=None), dict(xtab=None), dict(ytab=None), dict(N=-1), dict(RH=0),
               dict(RW=-4), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=0), dict(flags=1), dict(flags=4), dict(flags=-1),
               dict(flags=1 << 20), dict(kx=8), dict(ky=36), dict(origins=op + 2), dict(xtab=x + 1), dict(out=r + 64)):
        assert call(**kw) == EINVAL, kw
        assert lib.rg_last_error()
    for kw in (dict(oh=1025, h=1025), dict(ow=1025, w=1025), dict(h=8193, oh=8193), dict(w=8193), dict(h=280), dict(w=140, kx=35),
               dict(N=(1 << 31) - 1, oh=1024, ow=1024, h=1024, w=1024)):
        assert call(**kw) == EUNSUPPORTED, kw
        assert lib.rg_last_error()
    assert call(N=0) == 0
    m = torch.ones((2, 8, 8), dtype=torch.uint8, device=DEV)
    eo = _guarded((2, 8, 8))
    for args in ((None, eo.t.data_ptr(), 2, 8, 8, 1), (m.data_ptr(), None, 2, 8, 8, 1), (m.data_ptr(), eo.t.data_ptr(), -1, 8, 8, 1),
                 (m.data_ptr(), eo.t.data_ptr(), 2, 0, 8, 1), (m.data_ptr(), eo.t.data_ptr(), 2, 8, 8, 9),
                 (m.data_ptr(), eo.t.data_ptr(), 2, 8, 8, -1), (m.data_ptr(), m.data_ptr() + 8, 2, 8, 8, 1)):
        assert lib.rg_mask_erode(*args, None) == EINVAL, args
    bo = _guarded((20, 20, 3))
    for args in ((None, 40, 40, 2, bo.t.data_ptr()), (r, 40, 40, 2, None), (r, 0, 40, 2, bo.t.data_ptr()), (r, 40, 40, 0, bo.t.data_ptr()),
                 (r, 40, 40, 65, bo.t.data_ptr()), (r, 40, 40, 2, r + 4000)):
        assert lib.rg_box_reduce_u8(*args, None) == EINVAL, args
    torch.cuda.synchronize()
    for g in (out, eo, bo):
        assert bool((g.flat == PATTERN).all()), "a refused call wrote"
    assert bool((m == 1).all())
