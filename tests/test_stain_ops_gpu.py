"""rg_stain_moments, rg_stain_angle_hist, rg_stain_conc_hist and rg_stain_apply (include/rnagan_hip.h, rna_gan_amd/csrc/rg_stain.hip)
through ctypes on both builds of the library: every count, sum and byte EQUAL to the numpy restatement of tests/stain_refs.py.

Outputs live inside a larger allocation filled with one pattern (tests/guarded.py): a write outside them changes the pattern, and a
refused call must leave the output itself untouched too.  The host operands of passes 2 to 4 (basis, pseudo-inverse, scale, target)
come from ONE restated fit of a synthetic Beer-Lambert set and are used for every shape: the kernels do not care where they came from.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import stain_refs as R
from both_builds import H16
from guarded import DEV, Guarded

pytestmark = pytest.mark.gpu
both_builds = pytest.mark.parametrize("h16", H16, ids=["bfloat16", "float16"])
PATTERN = 0xA5
SEED64 = 0x5A5A5A5A5A5A5A5A                    # the pattern of the int64 / uint64 outputs
EINVAL, EUNSUPPORTED = -1, -2
PLANAR, REVERSE = 1, 2
# N x H x W: one pixel; fewer pixels than a quad's tail leaves; an odd size over several tiles; a multiple of 4; one pixel more than
# a statistics workgroup's chunk (4 apply chunks + 1): interleaved takes the vector path with a tail, planar the byte path
SHAPES = [(1, 1, 1), (1, 5, 7), (3, 33, 130), (2, 64, 64), (1, 99, 331)]
LAYOUTS = [("nhwc", "rgb"), ("nhwc", "bgr"), ("nchw", "rgb"), ("nchw", "bgr")]


def _lib(h16):
    from rna_gan_amd import _abi
    return _abi.load("bf16" if h16 == torch.bfloat16 else "f16")


def _flags(layout, order):
    return (PLANAR if layout == "nchw" else 0) | (REVERSE if order == "bgr" else 0)


def _kept(g, pattern):
    return bool((g.flat[:g.before] == pattern).all()) and bool((g.flat[g.before + g.n:] == pattern).all())


def _bytes(a, offset=0):
    """uint8 numpy -> a guarded device copy whose data starts `offset` bytes after a 256-byte boundary"""
    a = np.ascontiguousarray(a)
    g = Guarded(torch.full((a.size + offset,), PATTERN, dtype=torch.uint8), PATTERN)
    g.data = g.t[offset:offset + a.size]
    g.data.copy_(torch.from_numpy(a.reshape(-1)))
    g.ptr = g.t.data_ptr() + offset
    return g


def _words(n, seed=SEED64):
    g = Guarded(torch.full((n,), seed, dtype=torch.int64), SEED64)
    g.ptr = g.t.data_ptr()
    return g


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ll(v):
    return ctypes.cast((ctypes.c_longlong * len(v))(*v), ctypes.c_void_p)


def _ii(v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _tables():
    table, off = R.out_lut()
    return {"od": _dev(R.od_lut()), "dirs": _dev(R.dirs()), "out": _dev(table), "L": len(table), "off": off}


@functools.lru_cache(maxsize=None)
def _operands():
    """basis6, pinv6, scale2, href6 of one restated fit, normalised to the published target"""
    f = R.fit(R.synthetic_set(7).reshape(-1, 3))
    pinv6, scale2, href6 = R.operands(f["he"], f["max_conc"], [[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], [1.9705, 1.0308])
    return tuple(f["basis6"]), tuple(pinv6), tuple(scale2), tuple(href6)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(rgb (N, H, W, 3), the restated results of the four passes)"""
    rgb = R.synthetic_set(sum(shape), stains=shape[0] % 2, shape=shape)
    if shape == (1, 1, 1):
        rgb[...] = (120, 60, 150)
    b6, p6, s2, h6 = _operands()
    px = rgb.reshape(-1, 3)
    want = {"moments": R.moments(px), "angle": R.angle_hist(px, b6), "conc": R.conc_hist(px, p6).reshape(-1),
            "apply": R.apply(px, p6, s2, h6).reshape(rgb.shape)}
    for v in want.values():
        v.setflags(write=False)
    return rgb, want


class _Call:
    """the four entry points on one stored set"""

    def __init__(self, lib, stored, N, H, W, flags, offset=0):
        self.lib, self.N, self.H, self.W, self.flags = lib, N, H, W, flags
        self.src = _bytes(stored, offset)
        self.T = _tables()
        self.stream = None

    def _st(self):
        return (self.stream or torch.cuda.current_stream()).cuda_stream

    def moments(self, out, acc=0, ptr=None, n=None):
        return self.lib.rg_stain_moments(ptr or self.src.ptr, self.N if n is None else n, self.H, self.W, self.flags,
                                         self.T["od"].data_ptr(), R.BETA_Q, out.ptr, acc, self._st())

    def angle(self, out, acc=0, ptr=None, n=None, basis6=None, K=R.K):
        return self.lib.rg_stain_angle_hist(ptr or self.src.ptr, self.N if n is None else n, self.H, self.W, self.flags,
                                            self.T["od"].data_ptr(), R.BETA_Q, _ii(basis6 or _operands()[0]),
                                            self.T["dirs"].data_ptr(), K, out.ptr, acc, self._st())

    def conc(self, out, acc=0, ptr=None, n=None, pinv6=None, qp=R.QP, csh=R.CSH, bins=R.CB):
        return self.lib.rg_stain_conc_hist(ptr or self.src.ptr, self.N if n is None else n, self.H, self.W, self.flags,
                                           self.T["od"].data_ptr(), _ll(pinv6 or _operands()[1]), qp, csh, bins, out.ptr, acc,
                                           self._st())

    def apply(self, dst_ptr, pinv6=None, qp=R.QP, scale2=None, qs=R.QS, href6=None, shift=R.SHIFT, L=None, off=None, n=None):
        _, p6, s2, h6 = _operands()
        return self.lib.rg_stain_apply(self.src.ptr, dst_ptr, self.N if n is None else n, self.H, self.W, self.flags,
                                       self.T["od"].data_ptr(), _ll(pinv6 or p6), qp, _ll(scale2 or s2), qs, _ii(href6 or h6), shift,
                                       self.T["out"].data_ptr(), self.T["L"] if L is None else L, self.T["off"] if off is None else off,
                                       self._st())


def _ok(lib, rc, what):
    torch.cuda.synchronize()
    assert rc == 0, "%s: %d %s" % (what, rc, lib.rg_last_error())


def _equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %d, expected %d" % (
        what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _all_four(lib, rgb, layout, order, offset=0, what=""):
    """run the four passes on rgb stored in (layout, order) -> dict of numpy results; asserts the surroundings"""
    N, H, W = rgb.shape[:3]
    stored = R.store_as(rgb, layout, order)
    call = _Call(lib, stored, N, H, W, _flags(layout, order), offset)
    m, a, c = _words(10), _words(R.K + 1), _words(2 * R.CB)
    dst = _bytes(np.full(stored.shape, PATTERN, np.uint8), offset)
    _ok(lib, call.moments(m), what + " moments")
    _ok(lib, call.angle(a), what + " angle_hist")
    _ok(lib, call.conc(c), what + " conc_hist")
    _ok(lib, call.apply(dst.ptr), what + " apply")
    for g, pat in ((m, SEED64), (a, SEED64), (c, SEED64), (dst, PATTERN), (call.src, PATTERN)):
        assert _kept(g, pat), what + ": a write outside a buffer"
    if offset:
        assert bool((dst.t[:offset] == PATTERN).all()), what + ": a write in front of dst"
    assert bool((call.src.data.cpu() == torch.from_numpy(stored.reshape(-1))).all()), what + ": the source was written"
    got = dst.data.cpu().numpy().reshape(stored.shape)
    return {"moments": m.t.cpu().numpy(), "angle": a.t.cpu().numpy(), "conc": c.t.cpu().numpy(),
            "apply": R.rgb_of(got, layout, order).reshape(rgb.shape)}


# ------------------------------------------------------------------ every shape, layout, order, build
@both_builds
@pytest.mark.parametrize("layout,order", LAYOUTS, ids=["%s-%s" % lo for lo in LAYOUTS])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_four_passes_equal_the_restatement(shape, layout, order, h16):
    from rna_gan_amd import stain
    assert SHAPES[-1][0] * SHAPES[-1][1] * SHAPES[-1][2] == stain.STAT_CHUNK + 1 == 4 * stain.APPLY_CHUNK + 1
    rgb, want = _case(shape)
    got = _all_four(_lib(h16), rgb, layout, order, what="%s %s %s" % (shape, layout, order))
    for k in ("moments", "angle", "conc", "apply"):
        _equal(got[k], want[k], "%s %s %s %s" % (k, shape, layout, order))
    assert int(got["angle"].sum()) == int(got["moments"][0]) and int(got["conc"].sum()) == 2 * shape[0] * shape[1] * shape[2]


@both_builds
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(3, 33, 130), (2, 64, 64)], ids=["3x33x130", "2x64x64"])
def test_base_offset_by_one_byte_and_byte_path_equals_vector_path(shape, layout, h16):
    """src and dst one byte past a dword boundary: no lane may use a dword access, and the bytes equal those of the aligned call"""
    rgb, want = _case(shape)
    lib = _lib(h16)
    odd = _all_four(lib, rgb, layout, "rgb", offset=1, what="offset 1")
    even = _all_four(lib, rgb, layout, "rgb", offset=0, what="offset 0")
    for k in ("moments", "angle", "conc", "apply"):
        _equal(odd[k], want[k], "%s at offset 1" % k)
        _equal(odd[k], even[k], "%s: byte path against vector path" % k)


@both_builds
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_accumulate_over_two_halves_and_the_64_bit_carry(layout, h16):
    """tiles [0, 1) then [1, 3), and the other way round, equal one call; an output pre-seeded with 2^32 - 5 comes back as the
    seed plus the counts"""
    shape = (3, 33, 130)
    rgb, want = _case(shape)
    lib = _lib(h16)
    stored = R.store_as(rgb, layout, "rgb")
    call = _Call(lib, stored, 3, 33, 130, _flags(layout, "rgb"))
    tile = 3 * 33 * 130
    halves = [(call.src.ptr, 1), (call.src.ptr + tile, 2)]
    seed = (1 << 32) - 5
    for order in (halves, halves[::-1]):
        for name, fn, n in (("moments", call.moments, 10), ("angle", call.angle, R.K + 1), ("conc", call.conc, 2 * R.CB)):
            out = _words(n)
            for i, (ptr, cnt) in enumerate(order):
                _ok(lib, fn(out, acc=int(i > 0), ptr=ptr, n=cnt), name)
            _equal(out.t.cpu().numpy(), want[name], name + " over two halves")
            assert _kept(out, SEED64)
    for name, fn, n in (("moments", call.moments, 10), ("angle", call.angle, R.K + 1), ("conc", call.conc, 2 * R.CB)):
        out = _words(n)
        out.t.fill_(seed)
        _ok(lib, fn(out, acc=1), name)
        _equal(out.t.cpu().numpy(), want[name] + seed, name + " on a seed of 2^32 - 5")
        assert int(out.t.max()) > (1 << 32) and _kept(out, SEED64)


@both_builds
def test_all_background_and_all_stained(h16):
    lib = _lib(h16)
    for value, stained in (((255, 255, 255), 0), ((250, 238, 241), 0), ((60, 30, 90), 1)):
        rgb = np.empty((2, 9, 13, 3), np.uint8)
        rgb[...] = value
        px = rgb.reshape(-1, 3)
        got = _all_four(lib, rgb, "nhwc", "rgb", what=str(value))
        assert int(got["moments"][0]) == stained * px.shape[0]
        _equal(got["moments"], R.moments(px), "moments")
        _equal(got["angle"], R.angle_hist(px, _operands()[0]), "angle")
        _equal(got["conc"], R.conc_hist(px, _operands()[1]).reshape(-1), "conc")
        _equal(got["apply"], R.apply(px, *_operands()[1:]).reshape(rgb.shape), "apply")
        if not stained:
            assert int(np.abs(got["moments"]).sum()) == 0 and int(got["angle"].sum()) == 0


@both_builds
def test_outside_counter_with_a_hand_made_basis(h16):
    """p1 <= 0 lands in hist[K] alone: a basis whose first vector is -R (every stained pixel outside), R - B (both signs; p1 == 0
    for the grey pixels added), and +R (none outside)"""
    rgb, _ = _case((2, 64, 64))
    rgb = rgb.copy()
    rgb[0, 0, :8] = (77, 77, 77)
    px = rgb.reshape(-1, 3)
    lib = _lib(h16)
    call = _Call(lib, rgb, 2, 64, 64, 0)
    n = int(R.moments(px)[0])
    for basis6, outside in (((-16384, 0, 0, 0, 16384, 0), n), ((16384, 0, -16384, 0, 16384, 0), None), ((16384, 0, 0, 0, 16384, 0), 0)):
        out = _words(R.K + 1)
        _ok(lib, call.angle(out, basis6=basis6), "angle")
        got, want = out.t.cpu().numpy(), R.angle_hist(px, basis6)
        _equal(got, want, "angle %s" % (basis6,))
        assert outside is None or int(got[R.K]) == outside
        assert outside is not None or (0 < int(got[R.K]) < n and int(got[R.K]) >= 8)
        assert int(got.sum()) == n and _kept(out, SEED64)
    out = _words(5)                                                 # a smaller K: no bin past it is touched
    d = _dev(R.dirs(4))
    rc = lib.rg_stain_angle_hist(call.src.ptr, 2, 64, 64, 0, call.T["od"].data_ptr(), R.BETA_Q, _ii(_operands()[0]), d.data_ptr(), 4,
                                 out.ptr, 0, torch.cuda.current_stream().cuda_stream)
    _ok(lib, rc, "angle K = 4")
    _equal(out.t.cpu().numpy(), R.angle_hist(px, _operands()[0], R.dirs(4)), "angle K = 4")
    assert _kept(out, SEED64)


@both_builds
def test_concentrations_are_clamped_and_wide_operands(h16):
    """a stain whose concentrations all exceed the last bin, one whose are all negative; operands beyond int32 (the kernels'
    64-bit instantiation) give the bits of the same contract"""
    rgb, want = _case((3, 33, 130))
    px = rgb.reshape(-1, 3)
    lib = _lib(h16)
    call = _Call(lib, rgb, 3, 33, 130, 0)
    for pinv6, qp, bins in (((1 << 26, 1 << 26, 1 << 26, -(1 << 20), -(1 << 20), -(1 << 20)), R.QP, R.CB),
                            ((1 << 26, 1 << 26, 1 << 26, -(1 << 20), -(1 << 20), -(1 << 20)), R.QP, 7),
                            (tuple(v << 13 for v in _operands()[1]), R.QP + 13, R.CB)):
        out = _words(2 * bins)
        _ok(lib, call.conc(out, pinv6=pinv6, qp=qp, bins=bins), "conc")
        got = out.t.cpu().numpy()
        _equal(got, R.conc_hist(px, pinv6, qp, R.CSH, bins).reshape(-1), "conc %s" % (pinv6,))
        assert _kept(out, SEED64)
        if qp == R.QP:
            stained = int(R.moments(px)[0])
            assert int(got[bins - 1]) >= stained > 0 and int(got[bins]) >= stained
        else:
            assert max(abs(v) for v in pinv6) > (1 << 31)
            _equal(got, want["conc"], "conc with operands of 33 bits")
    _, p6, s2, h6 = _operands()
    dst = _bytes(np.full(rgb.shape, PATTERN, np.uint8))
    _ok(lib, call.apply(dst.ptr, pinv6=tuple(v << 13 for v in p6), qp=R.QP + 13), "apply wide")
    _equal(dst.data.cpu().numpy().reshape(rgb.shape), want["apply"], "apply with operands of 33 bits")
    wide_scale = tuple(v << 20 for v in s2)
    _ok(lib, call.apply(dst.ptr, scale2=wide_scale, qs=R.QS + 20), "apply wide scale")
    _equal(dst.data.cpu().numpy().reshape(rgb.shape), want["apply"], "apply with a scale of 36 bits")
    assert _kept(dst, PATTERN)


@both_builds
@pytest.mark.parametrize("layout,order", LAYOUTS, ids=["%s-%s" % lo for lo in LAYOUTS])
def test_apply_in_place(layout, order, h16):
    lib = _lib(h16)
    for shape in ((3, 33, 130), (2, 64, 64)):
        rgb, want = _case(shape)
        stored = R.store_as(rgb, layout, order)
        for offset in (0, 1):
            call = _Call(lib, stored, shape[0], shape[1], shape[2], _flags(layout, order), offset)
            _ok(lib, call.apply(call.src.ptr), "apply in place")
            got = R.rgb_of(call.src.data.cpu().numpy().reshape(stored.shape), layout, order).reshape(rgb.shape)
            _equal(got, want["apply"], "in place %s %s %s offset %d" % (shape, layout, order, offset))
            assert _kept(call.src, PATTERN)


@both_builds
def test_two_runs_a_side_stream_and_graph_replay(h16):
    shape = (3, 33, 130)
    rgb, want = _case(shape)
    lib = _lib(h16)
    call = _Call(lib, rgb, 3, 33, 130, 0)
    outs = {"moments": _words(10), "angle": _words(R.K + 1), "conc": _words(2 * R.CB)}
    dst = _bytes(np.full(rgb.shape, PATTERN, np.uint8))

    def run():
        assert call.moments(outs["moments"]) == 0 and call.angle(outs["angle"]) == 0 and call.conc(outs["conc"]) == 0, lib.rg_last_error()
        assert call.apply(dst.ptr) == 0, lib.rg_last_error()

    def read(what):
        torch.cuda.synchronize()
        for k, g in outs.items():
            _equal(g.t.cpu().numpy(), want[k], "%s %s" % (k, what))
            assert _kept(g, SEED64)
        _equal(dst.data.cpu().numpy().reshape(rgb.shape), want["apply"], "apply " + what)

    def refill():
        for g in outs.values():
            g.t.fill_(SEED64)
        dst.data.fill_(PATTERN)

    for k in range(2):
        refill()
        run()
        read("run %d" % k)
    refill()
    torch.cuda.synchronize()
    call.stream = torch.cuda.Stream()
    with torch.cuda.stream(call.stream):
        run()
    call.stream.synchronize()
    read("side stream")
    call.stream = None
    refill()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    for k in range(2):
        refill()
        graph.replay()
        read("graph replay %d" % k)


@both_builds
def test_refused_arguments_write_nothing(h16):
    lib = _lib(h16)
    rgb, _ = _case((2, 64, 64))
    call = _Call(lib, rgb, 2, 64, 64, 0)
    T = call.T
    st = torch.cuda.current_stream().cuda_stream
    m, a, c = _words(10 + 1), _words(R.K + 2), _words(2 * R.CB + 1)
    dst = _bytes(np.full(rgb.shape, PATTERN, np.uint8))
    od, dirs, out = T["od"].data_ptr(), T["dirs"].data_ptr(), T["out"].data_ptr()
    b6, p6, s2, h6 = _operands()
    big = (1 << 31) - 1
    src = call.src.ptr

    def mom(tiles=src, N=2, H=64, W=64, flags=0, lut=od, o=m.ptr):
        return lib.rg_stain_moments(tiles, N, H, W, flags, lut, R.BETA_Q, o, 0, st)

    def ang(tiles=src, N=2, H=64, W=64, flags=0, lut=od, basis=b6, d=dirs, K=R.K, o=a.ptr):
        return lib.rg_stain_angle_hist(tiles, N, H, W, flags, lut, R.BETA_Q, _ii(basis) if basis else None, d, K, o, 0, st)

    def con(tiles=src, N=2, H=64, W=64, flags=0, lut=od, pinv=p6, qp=R.QP, csh=R.CSH, bins=R.CB, o=c.ptr):
        return lib.rg_stain_conc_hist(tiles, N, H, W, flags, lut, _ll(pinv) if pinv else None, qp, csh, bins, o, 0, st)

    def app(s=src, d=dst.ptr, N=2, H=64, W=64, flags=0, lut=od, pinv=p6, qp=R.QP, scale=s2, qs=R.QS, href=h6, shift=R.SHIFT, table=out,
            L=T["L"], off=T["off"]):
        return lib.rg_stain_apply(s, d, N, H, W, flags, lut, _ll(pinv) if pinv else None, qp, _ll(scale) if scale else None, qs,
                                  _ii(href) if href else None, shift, table, L, off, st)

    refused = [
        (mom(tiles=None), EINVAL), (mom(lut=None), EINVAL), (mom(o=None), EINVAL), (mom(N=-1), EINVAL), (mom(H=0), EINVAL),
        (mom(W=-3), EINVAL), (mom(flags=4), EINVAL), (mom(lut=od + 2), EINVAL), (mom(o=m.ptr + 4), EINVAL),
        (mom(N=big, H=8, W=1), EUNSUPPORTED), (mom(N=1, H=1 << 17, W=(1 << 16) + 1), EUNSUPPORTED),
        (ang(tiles=None), EINVAL), (ang(basis=None), EINVAL), (ang(d=None), EINVAL), (ang(o=None), EINVAL), (ang(K=1), EINVAL),
        (ang(K=2049), EINVAL), (ang(d=dirs + 2), EINVAL), (ang(o=a.ptr + 4), EINVAL), (ang(flags=8), EINVAL),
        (ang(basis=(30001, 0, 0, 0, 0, 0)), EINVAL), (ang(N=big, H=8, W=1), EUNSUPPORTED),
        (con(tiles=None), EINVAL), (con(pinv=None), EINVAL), (con(o=None), EINVAL), (con(bins=0), EINVAL), (con(bins=4097), EINVAL),
        (con(qp=41), EINVAL), (con(qp=-1), EINVAL), (con(csh=32), EINVAL), (con(o=c.ptr + 4), EINVAL),
        (con(pinv=((1 << 40) + 1, 0, 0, 0, 0, 0)), EINVAL), (con(N=big, H=8, W=1), EUNSUPPORTED),
        (app(s=None), EINVAL), (app(d=None), EINVAL), (app(lut=None), EINVAL), (app(pinv=None), EINVAL), (app(scale=None), EINVAL),
        (app(href=None), EINVAL), (app(table=None), EINVAL), (app(L=0), EINVAL), (app(L=8193), EINVAL), (app(off=T["L"]), EINVAL),
        (app(off=-1), EINVAL), (app(qp=41), EINVAL), (app(qs=-1), EINVAL), (app(shift=41), EINVAL), (app(flags=16), EINVAL),
        (app(scale=(-1, 1)), EINVAL), (app(scale=(1 << 62, 1)), EINVAL), (app(href=(big, big, big, big, big, big), scale=(1 << 40, 1 << 40)), EINVAL),
        (app(N=1, d=src + 3 * 64 * 64), 0), (app(N=1, d=src + 3 * 64 * 64 - 1), EINVAL), (app(N=1, s=src + 5, d=src), EINVAL),
        (app(N=big, H=8, W=1), EUNSUPPORTED),
        (mom(N=0), 0), (ang(N=0), 0), (con(N=0), 0), (app(N=0), 0),
    ]
    torch.cuda.synchronize()
    allowed = 0
    for i, (rc, want) in enumerate(refused):
        assert rc == want, "call %d returned %d, expected %d: %s" % (i, rc, want, lib.rg_last_error())
        allowed += rc == 0 and want == 0
    for g, pat in ((m, SEED64), (a, SEED64), (c, SEED64), (dst, PATTERN)):
        assert _kept(g, pat) and bool((g.t == pat).all()), "a refused call wrote"
    assert lib.rg_last_error()
    # the one accepted call above wrote tile 0 over tile 1 (disjoint halves of src): it is there to show the overlap rule's edge
    assert allowed == 5
    got = call.src.data.cpu().numpy().reshape(rgb.shape)
    _equal(got[0], rgb[0], "src tile 0")
    _equal(got[1], R.apply(rgb[0].reshape(-1, 3), p6, s2, h6).reshape(rgb[0].shape), "dst = the second tile of src")
