"""rg_tile_qc (include/rnagan_hip.h) through ctypes: every returned integer and every mask byte EQUAL to the numpy restatement of
tests/tissue_refs.py (pinned without a GPU by tests/test_tissue_refs_cpu.py, which also checks that no expected Otsu threshold
hinges on an fp64 rounding).

``stats``, ``mask`` and the workspace each live inside a larger allocation filled with one pattern (tests/guarded.py): a write
outside them changes it, a refused call leaves it inside as well, and the workspace's own pattern is the "any content" the
contract allows -- the call has to zero what it accumulates into.  Overruns would stay inside the allocations, so nothing can
fault.
Shapes: 1 x 8 x 8 (less than a wave), 3 x 16 x 20, 2 x 64 x 64 (one mask block wider than the tile, every halo outside it), 1 x 256 x 256
(4 histogram chunks, 8 x 2 mask blocks), 1 x 300 x 260 (ragged in both directions: 5 chunks, 10 x 3 blocks with partial last ones),
5 x 33 x 7 (H W % 4 != 0: the scalar histogram path); a source one to three bytes behind a dword boundary takes the scalar path at
every shape."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from rna_gan_amd import tissue as TQ
from guarded import DEV, SBITS, Guarded
import tissue_refs as T

PATTERN = 0xA5
EINVAL, EUNSUPPORTED = -1, -2
LAYOUTS, ORDERS = ("nhwc", "nchw"), ("rgb", "bgr")


def _kept(g, fill):
    return bool((g.flat[:g.before] == fill).all()) and bool((g.flat[g.before + g.n:] == fill).all())


class Call:
    """One set of guarded buffers for a shape, reused by the calls of a test (the workspace is deliberately NOT reset between
    calls: it holds the previous call's counters)."""

    def __init__(self, lib, N, H, W, src_offset=0):
        self.lib, self.N, self.H, self.W = lib, N, H, W
        self.need = int(lib.rg_tile_qc_workspace_bytes(N, H, W))
        assert self.need > 0 and self.need % 4 == 0
        self.stats = Guarded(torch.full((N, 12), SBITS, dtype=torch.int32), SBITS)
        self.mask = Guarded(torch.full((N, H, W), PATTERN, dtype=torch.uint8), PATTERN)
        self.ws = Guarded(torch.full((self.need,), PATTERN, dtype=torch.uint8), PATTERN)
        self.src = torch.full((256 + N * H * W * 3 + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        self.src_at = 256 + src_offset
        assert (self.src.data_ptr() + self.src_at) % 4 == src_offset % 4

    def refill(self):
        self.stats.t.fill_(SBITS)
        self.mask.t.fill_(PATTERN)

    def upload(self, stored):
        self.src[self.src_at:self.src_at + stored.size] = torch.from_numpy(stored.reshape(-1).copy()).to(DEV)

    def run(self, stored, flags, rgb_min=50, dilate=3, ranks=None, with_mask=True, stream=None, ws_bytes=None):
        """stored = None: launch on what was uploaded before (under graph capture nothing may be copied from the host)"""
        if stored is not None:
            self.upload(stored)
        ranks = T.ranks_ref(self.H * self.W) if ranks is None else ranks
        r4 = (ctypes.c_int * 4)(*ranks)
        return self.lib.rg_tile_qc(self.src.data_ptr() + self.src_at, self.N, self.H, self.W, flags, rgb_min, dilate,
                                   ctypes.cast(r4, ctypes.c_void_p), self.stats.t.data_ptr(),
                                   self.mask.t.data_ptr() if with_mask else None, self.ws.t.data_ptr(),
                                   self.need if ws_bytes is None else ws_bytes, None if stream is None else stream.cuda_stream)

    def read(self):
        torch.cuda.synchronize()
        assert self.stats.surroundings_keep(SBITS), "rg_tile_qc wrote outside stats"
        assert _kept(self.mask, PATTERN), "rg_tile_qc wrote outside mask"
        assert _kept(self.ws, PATTERN), "rg_tile_qc wrote outside the workspace"
        return self.stats.t.cpu().numpy().copy(), self.mask.t.cpu().numpy().copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.stats.flat == SBITS).all()) and bool((self.mask.flat == PATTERN).all()) and \
            bool((self.ws.flat == PATTERN).all())


def _compare(got, want, what):
    (gs, gm), (ws, wm) = got, want
    assert np.array_equal(gs, ws), "%s: stats differ\ngot\n%s\nwant\n%s" % (what, gs, ws)
    bad = np.flatnonzero(gm.reshape(-1) != wm.reshape(-1))
    assert bad.size == 0, "%s: %d mask bytes differ, first at %d" % (what, bad.size, bad[0])


# 2 x 131 x 127: 16637 pixels per tile, odd -- two histogram chunks on the byte path, the second of 253 pixels; a chunk that ran past
# its tile's end would count into the second tile
@pytest.mark.parametrize("N,H,W", T.SHAPES + [(2, 131, 127)])
def test_stats_and_mask_equal_the_restatement(N, H, W):
    lib = _abi.load()
    rgb = T.random_tiles(N, H, W)
    call = Call(lib, N, H, W)
    for d in T.DILATES:
        want = T.batch_ref(rgb, dilate=d, key=("random", N, H, W))
        print("%s dilate %d: %s" % ((N, H, W), d, want[0][0].tolist()))
        for layout in LAYOUTS:
            for order in ORDERS:
                call.refill()
                rc = call.run(T.stored(rgb, layout, order), T.flags_of(layout, order), dilate=d)
                assert rc == 0, lib.rg_last_error()
                _compare(call.read(), want, (N, H, W, d, layout, order))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_source_off_the_dword_grid(offset):
    lib = _abi.load()
    for (N, H, W) in ((2, 64, 64), (1, 300, 260)):
        rgb = T.random_tiles(N, H, W)
        want = T.batch_ref(rgb, key=("random", N, H, W))
        call = Call(lib, N, H, W, src_offset=offset)
        for layout, order in (("nhwc", "rgb"), ("nchw", "bgr")):
            call.refill()
            assert call.run(T.stored(rgb, layout, order), T.flags_of(layout, order)) == 0, lib.rg_last_error()
            _compare(call.read(), want, (N, H, W, offset, layout, order))


def test_special_contents():
    """A constant tile (every lo == hi), an all-black tile (mx = 0), a constant 256 x 256 tile (65 536 in one bin), two-level
    tiles with equal populations (every Otsu candidate ties: the first wins), a single raw-mask pixel at the centre, at the
    middle of two edges and in two corners (25, 16, 16, 10, 10 dilated pixels), with rgb_min below, at and above the data."""
    lib = _abi.load()
    calls = {}
    for t in T.special_tiles():
        _, H, W, _ = t.shape
        call = calls.setdefault((H, W), Call(lib, 1, H, W))
        for rgb_min in (50, 0, 229):
            want = T.batch_ref(t, rgb_min=rgb_min)
            for layout, order in (("nhwc", "rgb"), ("nchw", "bgr"), ("nhwc", "bgr")):
                call.refill()
                assert call.run(T.stored(t, layout, order), T.flags_of(layout, order), rgb_min=rgb_min) == 0, lib.rg_last_error()
                _compare(call.read(), want, (t[0, 0, 0].tolist(), H, W, rgb_min, layout, order))
    counts = [int(T.batch_ref(T.single_pixel_tile(16, 20, r, c))[0][0, 5]) for (r, c) in ((8, 10), (0, 10), (8, 0), (0, 0), (15, 19))]
    assert counts == [25, 16, 16, 10, 10]
    big = T.batch_ref(T.constant_tile(256, 256, (201, 201, 201)))[0][0].tolist()
    assert big == [201, 201, 201, 0, 0, 0] + [2010000] * 4 + [0, 0]


def test_order_statistics_next_to_coarse_bin_boundaries_and_at_the_end_ranks():
    """The selection is two-level (coarse bin L >> 10, fine bin L & 1023): luma values on both sides of four coarse boundaries, the
    ranks chosen so that one statistic is the last value below a boundary and the next the first at or above it; ranks 0 and
    n - 1; four equal ranks; ranks in descending order."""
    lib = _abi.load()
    for (H, W) in ((16, 20), (64, 64)):
        n = H * W
        t = T.luma_boundary_tile(H, W)
        L = np.sort(T.luma_ref(t[0]).reshape(-1))
        steps = np.flatnonzero((L[1:] >> T.COARSE_SHIFT) != (L[:-1] >> T.COARSE_SHIFT))
        crossing = [int(s) for s in steps if (L[s + 1] >> T.COARSE_SHIFT) - (L[s] >> T.COARSE_SHIFT) == 1]
        assert len(crossing) >= 4, "the tile must cross coarse boundaries between neighbouring bins"
        call = Call(lib, 1, H, W)
        rank_sets = [(crossing[0], crossing[0] + 1, crossing[1], crossing[1] + 1),
                     (crossing[2], crossing[2] + 1, crossing[3], crossing[3] + 1),
                     (0, n - 1, 0, n - 1), (n - 1, n - 1, n - 1, n - 1), (n - 1, n // 2, 1, 0), (0, 0, 0, 0)]
        for ranks in rank_sets:
            want = T.batch_ref(t, ranks=ranks)
            assert want[0][0, 6:10].tolist() == [int(L[r]) for r in ranks]
            for layout, order in (("nhwc", "rgb"), ("nchw", "bgr")):
                call.refill()
                assert call.run(T.stored(t, layout, order), T.flags_of(layout, order), ranks=ranks) == 0, lib.rg_last_error()
                _compare(call.read(), want, (H, W, ranks, layout, order))
    # the same end ranks on random tiles, one of them larger than a histogram chunk
    for (N, H, W) in ((3, 16, 20), (1, 300, 260)):
        rgb = T.random_tiles(N, H, W)
        n = H * W
        call = Call(lib, N, H, W)
        for ranks in ((0, n - 1, n // 2, n // 2 + 1), (n - 1, 0, n - 2, 1)):
            want = T.batch_ref(rgb, ranks=ranks)
            call.refill()
            assert call.run(T.stored(rgb, "nhwc", "rgb"), 0, ranks=ranks) == 0, lib.rg_last_error()
            _compare(call.read(), want, (N, H, W, ranks))


@pytest.mark.parametrize("N,H,W", [(5, 33, 7), (3, 16, 20), (2, 64, 64)])
def test_independence(N, H, W):
    """A batch of distinct tiles equals each tile run alone; the same call twice on one workspace gives equal results; mask = NULL
    changes nothing in stats and writes no mask."""
    lib = _abi.load()
    rgb = T.random_tiles(N, H, W)
    want = T.batch_ref(rgb, key=("random", N, H, W))
    call = Call(lib, N, H, W)
    assert call.run(T.stored(rgb, "nhwc", "rgb"), 0) == 0, lib.rg_last_error()
    first = call.read()
    _compare(first, want, "batch")
    call.refill()
    assert call.run(T.stored(rgb, "nhwc", "rgb"), 0) == 0, lib.rg_last_error()          # the workspace holds the first call's counters
    _compare(call.read(), first, "second call on the same workspace")
    call.refill()
    assert call.run(T.stored(rgb, "nhwc", "rgb"), 0, with_mask=False) == 0, lib.rg_last_error()
    s, m = call.read()
    assert np.array_equal(s, want[0]) and bool((m == PATTERN).all()), "mask = NULL"
    one = Call(lib, 1, H, W)
    for n in range(N):
        one.refill()
        assert one.run(T.stored(rgb[n:n + 1], "nhwc", "rgb"), 0) == 0, lib.rg_last_error()
        s, m = one.read()
        assert np.array_equal(s[0], want[0][n]) and np.array_equal(m[0], want[1][n]), "tile %d alone" % n
    # reversed batch order: every tile's row moves with it
    call.refill()
    assert call.run(T.stored(rgb[::-1], "nhwc", "rgb"), 0) == 0, lib.rg_last_error()
    s, m = call.read()
    assert np.array_equal(s, want[0][::-1]) and np.array_equal(m, want[1][::-1])


def test_fp16_build_side_stream_and_graph_replay():
    rgb = T.random_tiles(3, 16, 20)
    want = T.batch_ref(rgb, key=("random", 3, 16, 20))
    f16 = Call(_abi.load("f16"), 3, 16, 20)
    assert f16.run(T.stored(rgb, "nchw", "bgr"), 3) == 0
    _compare(f16.read(), want, "fp16 build")
    lib = _abi.load()
    call = Call(lib, 3, 16, 20)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert call.run(T.stored(rgb, "nhwc", "rgb"), 0, stream=side) == 0, lib.rg_last_error()
    side.synchronize()
    _compare(call.read(), want, "side stream")
    call.refill()
    torch.cuda.synchronize()
    call.upload(T.stored(rgb, "nhwc", "rgb"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        assert call.run(None, 0, stream=torch.cuda.current_stream()) == 0, lib.rg_last_error()
    for _ in range(2):
        call.refill()
        graph.replay()
        _compare(call.read(), want, "graph replay")


def test_refused_arguments_launch_nothing():
    lib = _abi.load()
    N, H, W = 2, 8, 8
    rgb = T.random_tiles(1, 8, 8).repeat(2, axis=0)
    call = Call(lib, N, H, W)
    st = T.stored(rgb, "nhwc", "rgb")
    n = H * W
    ok = T.ranks_ref(n)
    bad = [dict(dilate=9), dict(dilate=-1), dict(ranks=(0, 1, 2, n)), dict(ranks=(n, 0, 0, 0)), dict(ranks=(0, -1, 0, 0)),
           dict(ranks=(0, 0, 1 << 30, 0)), dict(ws_bytes=call.need - 1), dict(ws_bytes=0), dict(flags=4), dict(flags=8),
           dict(flags=-1), dict(flags=1 << 20), dict(rgb_min=256), dict(rgb_min=-1)]
    for kw in bad:
        flags = kw.pop("flags", 0)
        assert call.run(st, flags, **kw) == EINVAL, kw
        assert lib.rg_last_error()
    r4 = ctypes.cast((ctypes.c_int * 4)(*ok), ctypes.c_void_p)
    s, m, w, src = call.stats.t.data_ptr(), call.mask.t.data_ptr(), call.ws.t.data_ptr(), call.src.data_ptr() + call.src_at
    for args in ((None, N, H, W, 0, 50, 3, r4, s, m, w, call.need), (src, N, H, W, 0, 50, 3, None, s, m, w, call.need),
                 (src, N, H, W, 0, 50, 3, r4, None, m, w, call.need), (src, N, H, W, 0, 50, 3, r4, s, m, None, call.need),
                 (src, -1, H, W, 0, 50, 3, r4, s, m, w, call.need), (src, N, 0, W, 0, 50, 3, r4, s, m, w, call.need),
                 (src, N, H, -8, 0, 50, 3, r4, s, m, w, call.need), (src, N, H, W, 0, 50, 3, r4, s + 2, m, w, call.need),
                 (src, N, H, W, 0, 50, 3, r4, s, m, w + 1, call.need)):
        assert lib.rg_tile_qc(*args, None) == EINVAL, args
        assert lib.rg_last_error()
    big = 1 << 50
    assert lib.rg_tile_qc(src, 1, 8193, 8192, 0, 50, 3, r4, s, m, w, big, None) == EUNSUPPORTED            # H W > 2^26
    assert lib.rg_tile_qc(src, 1, 1 << 20, 1 << 20, 0, 50, 3, r4, s, m, w, big, None) == EUNSUPPORTED
    assert lib.rg_tile_qc(src, (1 << 31) - 1, 8192, 8192, 0, 50, 3, r4, s, m, w, big, None) == EUNSUPPORTED   # too many workgroups
    assert lib.rg_tile_qc(src, 0, H, W, 0, 50, 3, r4, s, m, w, 0, None) == 0                                # N == 0: RG_OK, no launch
    assert call.untouched(), "a refused call wrote"


def test_python_tile_stats_on_the_device():
    """tissue.tile_stats on a CUDA tensor equals its CPU path (which tests/test_tissue_refs_cpu.py pins to the restatement), mask
    included; the decisions follow; the workspace is one cached buffer per device."""
    for (N, H, W) in ((3, 16, 20), (5, 33, 7), (1, 300, 260)):
        rgb = T.random_tiles(N, H, W)
        for layout, order, d in (("nhwc", "rgb", 3), ("nchw", "bgr", 8), ("nchw", "rgb", 0)):
            x = torch.from_numpy(T.stored(rgb, layout, order))
            cpu = TQ.tile_stats(x, layout=layout, order=order, dilate=d, return_mask=True)
            dev = TQ.tile_stats(x.to(DEV), layout=layout, order=order, dilate=d, return_mask=True)
            assert np.array_equal(dev.stats, cpu.stats) and np.array_equal(dev.stats, T.batch_ref(rgb, dilate=d)[0])
            assert dev.mask.is_cuda and dev.mask.dtype == torch.uint8 and torch.equal(dev.mask.cpu(), cpu.mask)
            assert (dev.ranks, dev.weights, dev.H, dev.W) == (cpu.ranks, cpu.weights, H, W)
            assert np.array_equal(TQ.accept(dev), TQ.accept(cpu)) and np.array_equal(TQ.tissue_fraction(dev), TQ.tissue_fraction(cpu))
            assert np.array_equal(TQ.luma_percentiles(dev), TQ.luma_percentiles(cpu))
    ws = TQ._WS[("cuda", 0)]
    assert TQ.tile_stats(torch.from_numpy(T.stored(T.random_tiles(1, 8, 8), "nhwc", "rgb")).to(DEV)).mask is None
    assert TQ._WS[("cuda", 0)] is ws
    # a strided view is made contiguous, the answer is the view's
    rgb = T.random_tiles(3, 16, 20)
    wide = torch.from_numpy(T.stored(rgb, "nhwc", "rgb")).to(DEV)
    got = TQ.tile_stats(wide[::2])
    assert np.array_equal(got.stats, T.batch_ref(rgb[::2])[0])
