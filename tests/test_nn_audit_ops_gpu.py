"""rg_tile_descriptor_i8 and rg_nn_topk_i8 (include/rnagan_hip.h, rna_gan_amd/csrc/rg_nn.hip) through ctypes on both builds of the
library: every descriptor byte, norm and key EQUAL to the numpy restatement of tests/nn_audit_refs.py.

Outputs live inside a larger allocation filled with one pattern (tests/guarded.py): a write outside them changes the pattern, and a
refused call must leave the output itself untouched too.  Operands live inside allocations of finite garbage, and descriptor rows
wider than D carry garbage in their slack: a read past the operand or past column D changes a key."""
import functools

import numpy as np
import pytest
import torch

import nn_audit_refs as R
from both_builds import H16
from guarded import DEV, Guarded

pytestmark = pytest.mark.gpu
both_builds = pytest.mark.parametrize("h16", H16, ids=["bfloat16", "float16"])
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
P8, P32, P64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A        # the patterns around and inside int8 / int32 / int64 outputs
GARBAGE = 0x33                                               # around operands


def _lib(h16):
    from rna_gan_amd import _abi
    return _abi.load("bf16" if h16 == torch.bfloat16 else "f16")


def _kept(g, pattern):
    return bool((g.flat[:g.before] == pattern).all()) and bool((g.flat[g.before + g.n:] == pattern).all())


def _operand(a, offset=0):
    """numpy -> a device copy inside garbage, `offset` elements after a 256-byte boundary"""
    a = np.array(a, order="C")                              # a writable copy: the cached rows are read-only
    t = torch.from_numpy(a.reshape(-1))
    g = Guarded(torch.full((a.size + offset,), GARBAGE, dtype=t.dtype), GARBAGE)
    g.t[offset:offset + a.size].copy_(t)
    g.ptr = g.t.data_ptr() + offset * t.element_size()
    return g


def _output(shape, dtype, pattern):
    g = Guarded(torch.full(shape, pattern, dtype=dtype), pattern)
    g.ptr = g.t.data_ptr()
    return g


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(lib, rc, what):
    torch.cuda.synchronize()
    assert rc == 0, "%s: %d %s" % (what, rc, lib.rg_last_error())


# ---------------------------------------------------------------------------------------------- descriptors
def _tiles(N, C, S, f, seed):
    """random tiles; tile 0 all 0 (-> -128), tile 1 all 255 (-> 127) where they exist, and in the last tile the first blocks'
    sums are exactly f f / 2 modulo f f: the rounding tie"""
    t = np.random.default_rng(seed).integers(0, 256, size=(N, C, S, S), dtype=np.uint8)
    if N > 0:
        t[0] = 0
    if N > 1:
        t[1] = 255
    if N > 0 and f > 1:
        P, half = S // f, f * f // 2
        for x in range(min(P, 4)):
            blk = np.zeros(f * f, np.int64)
            total = x * f * f + half                         # mean x + 1/2 exactly: rounds up to x + 1
            blk[:] = total // (f * f)
            blk[:total % (f * f)] += 1
            t[N - 1, 0, :f, x * f:(x + 1) * f] = blk.reshape(f, f).astype(np.uint8)
    return t


def _descriptor(lib, tiles, f, ldd=None, offset=0, N=None):
    Nt, C, S, _ = tiles.shape
    N = Nt if N is None else N
    P = S // f
    ldd = R.ldd_of(C * P * P) if ldd is None else ldd
    src = _operand(tiles, offset)
    desc = _output((max(N, 1), ldd), torch.int8, P8)
    norm2 = _output((max(N, 1),), torch.int32, P32)
    rc = lib.rg_tile_descriptor_i8(src.ptr, N, C, S, f, desc.ptr, ldd, norm2.ptr, _stream())
    _ok(lib, rc, "rg_tile_descriptor_i8")
    assert _kept(desc, P8) and _kept(norm2, P32), "written outside the outputs"
    return desc.t.cpu().numpy(), norm2.t.cpu().numpy()


@both_builds
@pytest.mark.parametrize("S,f,C", [(8, 1, 3), (8, 2, 3), (16, 4, 1), (64, 8, 3), (256, 4, 3), (32, 16, 3), (64, 32, 3), (48, 2, 2)])
def test_descriptor_equals_the_restatement(h16, S, f, C):
    """(8, 2, 3): D = 48 against ldd = 64, the pad columns are zero; S = 8: the single-byte path; (64, 32, 3): f = 32"""
    tiles = _tiles(3, C, S, f, S + f)
    desc, norm2 = _descriptor(_lib(h16), tiles, f)
    wd, wn = R.descriptor(tiles, f)
    assert np.array_equal(desc, wd), "%d bytes differ" % int((desc != wd).sum())
    assert np.array_equal(norm2, wn)
    D = C * (S // f) ** 2
    assert (desc[0, :D] == -128).all() and (desc[1, :D] == 127).all() and not desc[:, D:].any()
    if f > 1:
        assert desc[2, :min(S // f, 4)].tolist() == [x + 1 - 128 for x in range(min(S // f, 4))]


@both_builds
@pytest.mark.parametrize("N", [0, 1, 5])
def test_descriptor_counts_a_wider_row_and_an_unaligned_source(h16, N):
    lib = _lib(h16)
    tiles = _tiles(max(N, 1), 3, 16, 4, 40 + N)
    for ldd, offset in ((64, 0), (128, 0), (64, 3)):               # D = 48; offset 3: the single-byte path on a vector shape
        desc, norm2 = _descriptor(lib, tiles, 4, ldd=ldd, offset=offset, N=N)
        if N == 0:
            assert (desc == P8).all() and (norm2 == P32).all()
            continue
        wd, wn = R.descriptor(tiles, 4, ldd=ldd)
        assert np.array_equal(desc, wd) and np.array_equal(norm2, wn)


@both_builds
def test_descriptor_refusals_write_nothing(h16):
    lib = _lib(h16)
    tiles = _tiles(2, 3, 16, 4, 9)
    src = _operand(tiles)
    desc = _output((2, 64), torch.int8, P8)
    norm2 = _output((2,), torch.int32, P32)
    st = _stream()
    bad = [(None, 2, 3, 16, 4, desc.ptr, 64, norm2.ptr), (src.ptr, 2, 3, 16, 4, None, 64, norm2.ptr),
           (src.ptr, 2, 3, 16, 4, desc.ptr, 64, None), (src.ptr, 2, 3, 16, 3, desc.ptr, 64, norm2.ptr),
           (src.ptr, 2, 3, 16, 0, desc.ptr, 64, norm2.ptr), (src.ptr, 2, 3, 16, 64, desc.ptr, 64, norm2.ptr),
           (src.ptr, 2, 3, 12, 8, desc.ptr, 64, norm2.ptr),                         # S % f != 0
           (src.ptr, 2, 3, 16, 4, desc.ptr, 48, norm2.ptr),                         # ldd % 64 != 0
           (src.ptr, 2, 3, 16, 2, desc.ptr, 128, norm2.ptr),                        # ldd < D = 192
           (src.ptr, -1, 3, 16, 4, desc.ptr, 64, norm2.ptr), (src.ptr, 2, 0, 16, 4, desc.ptr, 64, norm2.ptr),
           (src.ptr, 2, 3, 16, 4, src.ptr + 64, 64, norm2.ptr)]                     # desc overlaps tiles
    for args in bad:
        assert lib.rg_tile_descriptor_i8(*args, st) == EINVAL, args
        assert lib.rg_last_error()
    # D = 65 536 > 32 768 (nothing is read or written: the refusal comes first)
    assert lib.rg_tile_descriptor_i8(src.ptr, 1, 1, 256, 1, desc.ptr, 65536, norm2.ptr, st) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (desc.t == P8).all() and (norm2.t == P32).all() and _kept(desc, P8) and _kept(norm2, P32)
    assert (src.t.cpu().numpy()[:tiles.size] == tiles.reshape(-1)).all()


# ---------------------------------------------------------------------------------------------- top-k
@functools.lru_cache(maxsize=None)
def _rows(n, ldd, seed):
    a = np.random.default_rng(seed).integers(-128, 128, size=(n, ldd), dtype=np.int8)
    a.setflags(write=False)
    return a


def _ws_bytes(lib, Q, N, k):
    return int(lib.rg_nn_topk_ws_bytes(Q, N, k))


def _topk(lib, a, b, D, k, exclude=None, na=None, nb=None, twice=False):
    """the keys of one call (uint64 [Q][k]) on operands in garbage, a patterned output and a dirty workspace; twice: a second call
    on the workspace as the first left it, refilled with other bytes -- the same bits"""
    Q, ldd = a.shape
    N = b.shape[0]
    na = R.norms(a[:, :D]) if na is None else na
    nb = R.norms(b[:, :D]) if nb is None else nb
    ga, gb, gna, gnb = _operand(a), _operand(b), _operand(na), _operand(nb)
    ge = None if exclude is None else _operand(np.asarray(exclude, np.int32))
    keys = _output((Q, k), torch.int64, P64)
    need = _ws_bytes(lib, Q, N, k)
    ws = _output((max(need, 8),), torch.uint8, 0xA5)

    def call():
        rc = lib.rg_nn_topk_i8(ga.ptr, gna.ptr, Q, gb.ptr, gnb.ptr, N, D, ldd, k, None if ge is None else ge.ptr, keys.ptr, ws.ptr,
                               need, _stream())
        _ok(lib, rc, "rg_nn_topk_i8")
        assert _kept(keys, P64) and _kept(ws, 0xA5), "written outside keys or the workspace"
        return keys.t.cpu().numpy().view(np.uint64).copy()
    got = call()
    if twice:
        ws.t.copy_(torch.randint(0, 256, ws.t.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV))
        keys.t.fill_(P64)
        again = call()
        assert np.array_equal(got, again), "a second call on a dirtied workspace gave other bits"
    return got


def _check(lib, a, b, D, k, exclude=None, **kw):
    got = _topk(lib, a, b, D, k, exclude, **kw)
    want = R.topk_keys(a, R.norms(a[:, :D]), b, R.norms(b[:, :D]), D, k, exclude)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d keys differ, first at %s: got (d2 %d, row %d), want (d2 %d, row %d)" % (
        len(bad), bad[0], int(got[tuple(bad[0])]) >> 32, int(got[tuple(bad[0])]) & 0xffffffff,
        int(want[tuple(bad[0])]) >> 32, int(want[tuple(bad[0])]) & 0xffffffff)
    return got


@both_builds
@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("N", [8, 63, 129, 1000])
@pytest.mark.parametrize("Q", [1, 17, 130])
def test_topk_equals_the_restatement(h16, Q, N, D):
    """distinct random queries and references (a row / column swap changes every key); N = 129 and 1000: several tiles, and with
    them several shares; Q = 130: two query blocks, the second with two live rows"""
    lib = _lib(h16)
    a, b = _rows(Q, D, 100 + Q), _rows(N, D, 200 + N)
    for k in (1, 4, 8):
        _check(lib, a, b, D, k)


@both_builds
def test_topk_long_descriptors(h16):
    _check(_lib(h16), _rows(64, 12288, 1), _rows(512, 12288, 2), 12288, 4)


@both_builds
def test_topk_does_not_read_beyond_D(h16):
    """ldd = 256 > D = 192: the slack columns hold garbage that differs per row; the norms are those of the first D columns"""
    _check(_lib(h16), _rows(17, 256, 3), _rows(300, 256, 4), 192, 4)


@both_builds
def test_topk_largest_distance_int32_holds(h16):
    """all -128 against all 127 at D = 32 768: d2 = 32 768 * 255^2 = 2 130 739 200; rows 2 and 5 of b equal the query (d2 = 0)"""
    D = 32768
    a = np.full((2, D), -128, np.int8)
    b = np.full((9, D), 127, np.int8)
    b[2] = b[5] = -128
    got = _check(_lib(h16), a, b, D, 4)
    d2, ix = R.split_keys(got)
    assert d2.tolist() == [[0, 0, 2130739200, 2130739200]] * 2 and ix.tolist() == [[2, 5, 0, 1]] * 2


@both_builds
def test_topk_ties_go_to_the_lower_row_and_exclusions(h16):
    lib = _lib(h16)
    D, N = 64, 300
    b = _rows(N, D, 11).copy()
    b[150] = b[20]
    b[299] = b[20]
    b[260] = b[131]                              # across a tile boundary: rows 131 and 260 are in tiles 1 and 2
    a = np.stack([b[20], b[131], b[7], b[299], b[0]])
    d2, ix = R.split_keys(_check(lib, a, b, D, 4))
    assert ix[0, :3].tolist() == [20, 150, 299] and ix[1, :2].tolist() == [131, 260] and d2[:, 0].tolist() == [0] * 5
    # the query's own row excluded: its exact duplicates remain; the unduplicated row 7 loses its zero
    excl = [20, 131, 7, 299, -1]
    d2, ix = R.split_keys(_check(lib, a, b, D, 4, exclude=excl))
    assert ix[0, :2].tolist() == [150, 299] and ix[1, 0] == 260 and d2[2, 0] > 0 and ix[3, :2].tolist() == [20, 150] and ix[4, 0] == 0
    # values outside [0, N) exclude nothing
    free = _check(lib, a, b, D, 4)
    out = _check(lib, a, b, D, 4, exclude=[-1, N, 2 ** 31 - 1, -2 ** 31, N + 128])
    assert np.array_equal(free, out)


@both_builds
@pytest.mark.parametrize("k", [1, 4, 8])
def test_topk_with_as_many_rows_as_candidates(h16, k):
    lib = _lib(h16)
    a = _rows(5, 64, 31)
    # N = k: every row comes back, in order; N = k + 1 with a valid exclusion: the k others
    got = _check(lib, a, _rows(k, 64, 32), 64, k)
    assert sorted(R.split_keys(got)[1][0].tolist()) == list(range(k))
    _check(lib, a, _rows(k + 1, 64, 33), 64, k)
    excl = [0, k, 1 % (k + 1), -1, k + 1]                       # the last two exclude nothing: the k nearest of k + 1
    got = _check(lib, a, _rows(k + 1, 64, 33), 64, k, exclude=excl)
    assert sorted(R.split_keys(got)[1][1].tolist()) == list(range(k))
    # N = k with an exclusion list: one row counts as excluded whatever the device values are (the host does not read them)
    b = _operand(_rows(k, 64, 32))
    ga, gn, ge = _operand(a), _operand(R.norms(a)), _operand(np.full(5, -1, np.int32))
    keys = _output((5, k), torch.int64, P64)
    ws = _output((4096,), torch.uint8, 0xA5)
    rc = lib.rg_nn_topk_i8(ga.ptr, gn.ptr, 5, b.ptr, gn.ptr, k, 64, 64, k, ge.ptr, keys.ptr, ws.ptr, 4096, _stream())
    assert rc == EINVAL and lib.rg_last_error()
    torch.cuda.synchronize()
    assert (keys.t == P64).all()


@both_builds
def test_topk_shares_a_querys_references_among_workgroups(h16):
    """the sharing rule of the header: Q = 3 is one query block, N = 5 000 is 40 tiles, 1024 / 1 >= 40: 40 shares of one tile, the
    workspace holds 40 x 8 x 3 keys; Q = 700 is 6 query blocks, 170 wanted shares, 40 tiles: one tile each again; a second call on
    the dirtied workspace gives the same bits"""
    lib = _lib(h16)
    assert _ws_bytes(lib, 3, 5000, 8) == 40 * 8 * 3 * 8 and _ws_bytes(lib, 3, 128, 8) == 1 * 8 * 3 * 8
    assert _ws_bytes(lib, 3, 129, 1) == 2 * 8 * 3 * 8
    assert _ws_bytes(lib, 128 * 512, 128 * 7, 4) == 2 * 8 * 128 * 512 * 8          # 512 query blocks: 2 shares of ceil(7 / 2) = 4 tiles
    b = _rows(5000, 64, 41).copy()
    b[4999] = b[3]                               # a tie between the first and the last share
    a = np.stack([b[3], b[2500], _rows(1, 64, 42)[0]])
    got = _check(lib, a, b, 64, 8, twice=True)
    assert R.split_keys(got)[1][0, :2].tolist() == [3, 4999]
    _check(lib, _rows(700, 64, 43), b, 64, 4, twice=True)


@both_builds
def test_topk_refusals_write_nothing(h16):
    lib = _lib(h16)
    a, b = _rows(4, 128, 51), _rows(40, 128, 52)
    ga, gb, gna, gnb = _operand(a), _operand(b), _operand(R.norms(a)), _operand(R.norms(b))
    keys = _output((4, 4), torch.int64, P64)
    need = _ws_bytes(lib, 4, 40, 4)
    ws = _output((need + 8,), torch.uint8, 0xA5)
    st = _stream()

    def call(a_=ga.ptr, na=gna.ptr, Q=4, b_=gb.ptr, nb=gnb.ptr, N=40, D=128, ldd=128, k=4, ex=None, keys_=keys.ptr, ws_=ws.ptr, wsb=need):
        return lib.rg_nn_topk_i8(a_, na, Q, b_, nb, N, D, ldd, k, ex, keys_, ws_, wsb, st)
    for kw in (dict(a_=None), dict(na=None), dict(b_=None), dict(nb=None), dict(keys_=None), dict(D=32), dict(D=0), dict(D=96),
               dict(ldd=64), dict(ldd=136), dict(k=0), dict(k=9), dict(k=-1), dict(N=3), dict(Q=-1), dict(N=-1),
               dict(keys_=keys.ptr + 4), dict(ws_=ws.ptr + 4), dict(a_=ga.ptr + 8), dict(nb=gnb.ptr + 2)):
        assert call(**kw) == EINVAL, kw
        assert lib.rg_last_error()
    assert call(wsb=need - 1) == EWORKSPACE and call(ws_=None) == EWORKSPACE
    assert call(D=32832, ldd=32832) == EUNSUPPORTED
    assert call(Q=0, a_=None, na=None, keys_=None, ws_=None, wsb=0) == 0          # Q == 0: RG_OK, nothing launched
    torch.cuda.synchronize()
    assert (keys.t == P64).all() and (ws.t == 0xA5).all() and _kept(keys, P64) and _kept(ws, 0xA5)
    assert call() == 0
    torch.cuda.synchronize()
    want = R.topk_keys(a, R.norms(a), b, R.norms(b), 128, 4)
    assert np.array_equal(keys.t.cpu().numpy().view(np.uint64), want)


@both_builds
def test_descriptor_and_topk_on_a_side_stream_and_under_graph_replay(h16):
    lib = _lib(h16)
    tiles = _tiles(40, 3, 16, 2, 61)                         # D = 192
    src = _operand(tiles)
    desc = _output((40, 192), torch.int8, P8)
    norm2 = _output((40,), torch.int32, P32)
    keys = _output((40, 3), torch.int64, P64)
    need = _ws_bytes(lib, 40, 40, 3)
    ws = _output((need,), torch.uint8, 0xA5)
    excl = torch.arange(40, dtype=torch.int32, device=DEV)
    wd, wn = R.descriptor(tiles, 2)
    want = R.topk_keys(wd, wn, wd, wn, 192, 3, np.arange(40))

    def run():
        s = _stream()
        assert lib.rg_tile_descriptor_i8(src.ptr, 40, 3, 16, 2, desc.ptr, 192, norm2.ptr, s) == 0, lib.rg_last_error()
        assert lib.rg_nn_topk_i8(desc.ptr, norm2.ptr, 40, desc.ptr, norm2.ptr, 40, 192, 192, 3, excl.data_ptr(), keys.ptr, ws.ptr, need,
                                 s) == 0, lib.rg_last_error()

    def refill():
        desc.t.fill_(P8), norm2.t.fill_(P32), keys.t.fill_(P64)

    def read(what):
        torch.cuda.synchronize()
        assert np.array_equal(desc.t.cpu().numpy(), wd) and np.array_equal(norm2.t.cpu().numpy(), wn), what
        assert np.array_equal(keys.t.cpu().numpy().view(np.uint64), want), what
        assert _kept(desc, P8) and _kept(norm2, P32) and _kept(keys, P64) and _kept(ws, 0xA5), what
    run()
    read("default stream")
    refill()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    read("side stream")
    refill()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    for i in range(2):
        refill()
        graph.replay()
        read("graph replay %d" % i)
