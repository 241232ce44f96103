"""rg_msssim_plan / rg_msssim_pyramid / rg_msssim_pairs (include/rnagan_hip.h) through ctypes against the fp64 numpy restatement of
tests/msssim_refs.py (pinned without a GPU by tests/test_msssim_refs_cpu.py).

Tolerance.  CS_s and SSIM_s: absolute 1e-9.  Derived, not observed: the fp64 unit roundoff 1.1e-16 times the second-moment magnitude
6.5e4 over C2 = 58.5, times a few hundred operations, is about 1e-11; two decades of margin.  The FINAL score is held to the same 1e-9
on the correlated sets (every pair, none left out): the CPU file asserts that every CS of those inputs is at least 0.05, so the power
0.0448 is nowhere ill-conditioned (d/dx x^0.0448 at 0.05 is 0.78).  On independent uniform noise only the components are compared:
CS_0 there is about 1e-3 of either sign, next to the clamp.  The pyramid is demanded EQUAL (integers).  The worst observed errors go to
profiles/msssim_op_errors.txt.

The tile sets, the pyramids, the workspace and the output each live inside a larger allocation filled with one pattern
(tests/guarded.py): a write outside them changes it, and a refused call leaves it inside as well.  The workspace's pattern is the
"any content" the contract allows.  Overruns would stay inside the allocations, so nothing can fault.

Shapes, the smallest at which each mechanism can go wrong: S = 1 at 11 x 11 (one window position), 11 x 12, 12 x 11, 13 x 17; S = 2 at
22 x 22, 23 x 23, 22 x 25 (a dropped odd row / column); S = 3 at 45 x 47; S = 5 at 176 x 176 (the minimum), 177 x 191, 256 x 256; and
heights / widths at k * BAND + 10 + {-1, 0, 1} and k * COLS + 10 + {-1, 0, 1}, k = 1, 2, around the seams of the launch plan, whose
constants are read from the library."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from rna_gan_amd import msssim as MS
from guarded import DEV, Guarded
import msssim_refs as R

TOL = 1e-9
FILL = -7.25                       # the pattern of the output's allocation
PATTERN = 0xA5
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def _plan(lib, H, W, S, P):
    info = (ctypes.c_int32 * (2 + 2 * S))()
    pyr, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.rg_msssim_plan(H, W, S, P, ctypes.cast(info, ctypes.c_void_p), ctypes.byref(pyr), ctypes.byref(ws))
    assert rc == 0, lib.rg_last_error()
    return list(info), int(pyr.value), int(ws.value)


def _kept(g, fill):
    return bool((g.flat[:g.before] == fill).all()) and bool((g.flat[g.before + g.n:] == fill).all())


class TileSet:
    """N tiles of one layout inside a guarded byte allocation, `offset` bytes behind a 256-byte boundary, with their pyramid"""

    def __init__(self, lib, rgb, S, layout="nhwc", order="rgb", offset=0):
        self.lib, self.S = lib, S
        self.N, self.H, self.W = rgb.shape[:3]
        self.flags = (1 if layout == "nchw" else 0) | (2 if order == "bgr" else 0)
        st = R.stored(rgb, layout, order).reshape(-1)
        self.buf = torch.full((256 + st.size + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        self.at = 256 + offset
        self.buf[self.at:self.at + st.size] = torch.from_numpy(st).to(DEV)
        self.ptr = self.buf.data_ptr() + self.at
        assert self.ptr % 256 == offset
        _, self.per_tile, _ = _plan(lib, self.H, self.W, S, 0)
        self.pyr = Guarded(torch.full((max(self.N * self.per_tile, 2),), PATTERN, dtype=torch.uint8), PATTERN)
        rc = lib.rg_msssim_pyramid(self.ptr, self.N, self.H, self.W, self.flags, S, self.pyr.t.data_ptr(), self.N * self.per_tile, None)
        assert rc == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        assert _kept(self.pyr, PATTERN), "rg_msssim_pyramid wrote outside the pyramid"

    def levels(self):
        """the pyramid as numpy: a list over s = 1 .. S - 1 of uint16 (N, 3, h_s, w_s)"""
        raw = self.pyr.t[:self.N * self.per_tile].cpu().numpy().view(np.uint16).reshape(self.N, -1)
        out, at = [], 0
        for s in range(1, self.S):
            h, w = self.H >> s, self.W >> s
            out.append(raw[:, at:at + 3 * h * w].reshape(self.N, 3, h, w))
            at += 3 * h * w
        assert at == raw.shape[1]
        return out


class Pairs:
    """guarded index arrays, workspace and output of up to `cap` pairs"""

    def __init__(self, lib, a, b, cap):
        self.lib, self.a, self.b, self.cap, self.S = lib, a, b, cap, a.S
        _, _, self.need = _plan(lib, a.H, a.W, a.S, cap)
        self.ws = Guarded(torch.full((self.need,), PATTERN, dtype=torch.uint8), PATTERN)
        self.out = Guarded(torch.full((cap, a.S, 3, 2), FILL, dtype=torch.float64), FILL)
        self.ia = torch.zeros(cap, dtype=torch.int32, device=DEV)
        self.ib = torch.zeros(cap, dtype=torch.int32, device=DEV)
        self.taps = (ctypes.c_double * 11)(*MS.taps())

    def set_pairs(self, i, j):
        self.P = len(i)
        self.ia[:self.P] = torch.tensor(list(i), dtype=torch.int32)
        self.ib[:self.P] = torch.tensor(list(j), dtype=torch.int32)

    def launch(self, stream=None, **kw):
        a, b = self.a, self.b
        args = dict(a=a.ptr, pyr_a=a.pyr.t.data_ptr() if a.S > 1 else None, Na=a.N, b=b.ptr, pyr_b=b.pyr.t.data_ptr() if a.S > 1 else None,
                    Nb=b.N, ia=self.ia.data_ptr(), ib=self.ib.data_ptr(), P=self.P, H=a.H, W=a.W, flags=a.flags, S=a.S,
                    taps=ctypes.cast(self.taps, ctypes.c_void_p), ws=self.ws.t.data_ptr(), ws_bytes=self.need, out=self.out.t.data_ptr())
        args.update(kw)
        return self.lib.rg_msssim_pairs(*[args[k] for k in ("a", "pyr_a", "Na", "b", "pyr_b", "Nb", "ia", "ib", "P", "H", "W", "flags", "S",
                                                            "taps", "ws", "ws_bytes", "out")], None if stream is None else stream.cuda_stream)

    def run(self, i, j):
        """the sums [P][S][3][2] (numpy) of the pairs (i, j)"""
        self.set_pairs(i, j)
        self.out.t.fill_(FILL)
        assert self.launch() == 0, self.lib.rg_last_error()
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        assert _kept(self.out, FILL), "rg_msssim_pairs wrote outside out"
        assert _kept(self.ws, PATTERN), "rg_msssim_pairs wrote outside the workspace"
        assert bool((self.out.t[self.P:] == FILL).all()), "rg_msssim_pairs wrote behind its P pairs"
        assert _kept(self.a.pyr, PATTERN) and _kept(self.b.pyr, PATTERN)
        return self.out.t[:self.P].cpu().numpy().copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out.flat == FILL).all()) and bool((self.ws.flat == PATTERN).all())


def _components(sums, H, W):
    return sums.mean(axis=2) / MS.positions(H, W, sums.shape[1])[None, :, None]


def _note(kind, shape, err):
    key = (kind,) + tuple(shape)
    WORST[key] = max(WORST.get(key, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _write_the_worst_errors():
    yield
    if WORST:
        with open(os.path.join(ROOT, "profiles", "msssim_op_errors.txt"), "w") as f:
            f.write("# worst absolute error of rg_msssim_pairs against tests/msssim_refs.py (fp64 numpy); tolerance %.0e\n" % TOL)
            f.write("# written by tests/test_msssim_ops_gpu.py\n")
            for key in sorted(WORST, key=str):
                f.write("%-12s %4d x %-4d  %.3e\n" % (key[0], key[1], key[2], WORST[key]))


def _check_pyramid(ts, rgb):
    for s, lev in enumerate(ts.levels(), start=1):
        h, w = ts.H >> s, ts.W >> s
        want = rgb[:, :h << s, :w << s].astype(np.int64).reshape(ts.N, h, 1 << s, w, 1 << s, 3).sum(axis=(2, 4)).transpose(0, 3, 1, 2)
        assert np.array_equal(lev.astype(np.int64), want), "pyramid level %d of %d x %d" % (s, ts.H, ts.W)


def _lib_plan_constants():
    info, _, _ = _plan(_abi.load(), 64, 64, 1, 0)
    return info[0], info[1]


BAND, COLS = 32, 16                # asserted equal to the library's in test_plan
SEAMS = [(k * BAND + 10 + dh, kc * COLS + 10 + dw) for (k, dh, kc, dw) in
         ((1, -1, 1, -1), (1, 0, 1, 0), (1, 1, 1, 1), (2, -1, 2, -1), (2, 0, 2, 0), (2, 1, 2, 1), (1, 1, 2, -1), (2, -1, 1, 1))]
SHAPES = [(11, 11), (11, 12), (12, 11), (13, 17), (22, 22), (23, 23), (22, 25), (45, 47), (176, 176), (177, 191), (256, 256)]


def test_plan():
    lib = _abi.load()
    assert _lib_plan_constants() == (BAND, COLS) == (MS.BAND, MS.COLS)
    for (H, W) in SHAPES + SEAMS:
        S = R.default_scales(H, W)
        assert MS.default_scales(H, W) == S
        info, pyr, ws = _plan(lib, H, W, S, 3)
        assert info[2:] == [v for s in range(S) for v in (H >> s, W >> s)]
        assert pyr == 2 * 3 * sum((H >> s) * (W >> s) for s in range(1, S))
        groups = sum(3 * -(-((H >> s) - 10) // BAND) * -(-((W >> s) - 10) // COLS) for s in range(S))
        assert ws == 3 * groups * 16
    for bad in ((10, 64, 1), (64, 10, 1), (64, 64, 0), (64, 64, 6), (64, 64, 4), (21, 400, 2)):
        assert lib.rg_msssim_plan(*bad, 1, None, None, None) == EINVAL and lib.rg_last_error()
    assert lib.rg_msssim_plan(64, 64, 1, -1, None, None, None) == EINVAL
    assert lib.rg_msssim_plan(4097, 64, 1, 1, None, None, None) == EUNSUPPORTED
    assert lib.rg_msssim_plan(4096, 4096, 5, 1 << 20, None, None, None) == EUNSUPPORTED


@pytest.mark.parametrize("H,W", SHAPES + SEAMS)
def test_components_and_scores_on_correlated_pairs(H, W):
    """two distinct sets: a[k] against b[k], b = a + N(0, sd), sd over SDS; every pair's components AND final score"""
    lib = _abi.load()
    S = R.default_scales(H, W)
    big = H * W > 40000
    parts = [R.correlated_sets(1 if big else 2, H, W, sd) for sd in R.SDS]
    a, b = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    A, B = TileSet(lib, a, S), TileSet(lib, b, S)
    _check_pyramid(A, a)
    _check_pyramid(B, b)
    n = a.shape[0]
    i = list(range(n))
    got = _components(Pairs(lib, A, B, n).run(i, i), H, W)
    want = R.batch_components(a, b, (i, i), S)
    err = np.abs(got - want).max()
    _note("components", (H, W), err)
    assert want[:, :, 0].min() >= R.CS_FLOOR
    score, wscore = MS.finish(got), np.array([R.finish(c) for c in want])
    serr = np.abs(score - wscore).max()
    _note("score", (H, W), serr)
    print("%d x %d S %d: components %.3g, score %.3g (scores %s)" % (H, W, S, err, serr, np.round(wscore, 4).tolist()))
    assert err <= TOL, (H, W, err)
    assert serr <= TOL and len(score) == n, (H, W, serr)


@pytest.mark.parametrize("H,W", [(13, 17), (23, 23), (45, 47), (177, 191)])
def test_components_on_independent_noise(H, W):
    """one set against itself, repeated indices, a pair with i == j"""
    lib = _abi.load()
    S = R.default_scales(H, W)
    x = R.random_tiles(3, H, W, 11)
    X = TileSet(lib, x, S)
    _check_pyramid(X, x)
    i, j = [0, 1, 2, 1, 0, 2], [1, 2, 0, 1, 1, 0]
    got = _components(Pairs(lib, X, X, 6).run(i, j), H, W)
    want = R.batch_components(x, x, (i, j), S)
    err = np.abs(got - want).max()
    _note("noise", (H, W), err)
    assert err <= TOL, (H, W, err)
    assert np.array_equal(got[3], np.ones((S, 2))), "a tile against itself: every ratio is x / x"
    assert MS.finish(got)[3] == 1.0


@pytest.mark.parametrize("layout,order,offset", [("nhwc", "rgb", 1), ("nhwc", "bgr", 0), ("nchw", "rgb", 0), ("nchw", "bgr", 1),
                                                 ("nhwc", "rgb", 3), ("nchw", "rgb", 2)])
def test_layouts_and_a_misaligned_base(layout, order, offset):
    lib = _abi.load()
    for (H, W) in ((23, 25), (45, 47)):
        S = R.default_scales(H, W)
        a, b = R.correlated_sets(3, H, W, 16, seed=2)
        a[..., 1] = a[..., 1] // 2                                    # the channels differ, so a wrong order shows
        base = Pairs(lib, TileSet(lib, a, S), TileSet(lib, b, S), 3).run([0, 1, 2], [2, 1, 0])
        A, B = TileSet(lib, a, S, layout, order, offset), TileSet(lib, b, S, layout, order, offset)
        _check_pyramid(A, a)
        got = Pairs(lib, A, B, 3).run([0, 1, 2], [2, 1, 0])
        assert np.array_equal(got, base), "the doubles depend on the bytes, not on where and how they are stored"
        want = R.batch_components(a, b, ([0, 1, 2], [2, 1, 0]), S)
        assert np.abs(_components(got, H, W) - want).max() <= TOL
        assert not np.allclose(got[:, :, 0], got[:, :, 1])


@pytest.mark.parametrize("H,W", [(11, 11), (23, 25), (64, 64), (177, 191)])
def test_closed_forms_on_the_device(H, W):
    lib = _abi.load()
    S = R.default_scales(H, W)
    x = R.two_scale_tile(H, W, 7)
    consts = [(0, 255), (17, 200), (128, 128), (0, 0)]
    tiles = np.stack([x, 255 - x] + [np.full((H, W, 3), c, np.uint8) for c in (0, 255, 17, 200, 128)])
    index = {0: 2, 255: 3, 17: 4, 200: 5, 128: 6}
    X = TileSet(lib, tiles, S)
    i = [0, 0] + [index[c1] for c1, _ in consts]
    j = [0, 1] + [index[c2] for _, c2 in consts]
    comp = _components(Pairs(lib, X, X, len(i)).run(i, j), H, W)
    assert np.array_equal(comp[0], np.ones((S, 2))) and MS.finish(comp)[0] == 1.0
    assert (comp[1, :, 0] < 0).all() and MS.finish(comp)[1] == 0.0, comp[1]
    for k, (c1, c2) in enumerate(consts, start=2):
        l = (2.0 * c1 * c2 + R.C1) / (c1 * c1 + c2 * c2 + R.C1)
        assert np.abs(comp[k, :, 0] - 1.0).max() <= TOL and np.abs(comp[k, :, 1] - l).max() <= TOL, (c1, c2, comp[k])


def test_batch_independence_and_graph_replay():
    """the doubles of a pair: alone, at every position of a batch of 8, with the list reversed, read from either set, under replay"""
    lib = _abi.load()
    H, W, S = 45, 47, 3
    a, b = R.correlated_sets(4, H, W, 16, seed=5)
    A, B = TileSet(lib, a, S), TileSet(lib, b, S)
    call = Pairs(lib, A, B, 8)
    alone = call.run([2], [3])
    filler_i, filler_j = [0, 1, 3, 0, 1, 3, 2], [0, 1, 2, 3, 3, 0, 1]
    for pos in range(8):
        i, j = filler_i[:pos] + [2] + filler_i[pos:], filler_j[:pos] + [3] + filler_j[pos:]
        got = call.run(i, j)
        assert np.array_equal(got[pos], alone[0]), pos
        back = call.run(i[::-1], j[::-1])
        assert np.array_equal(back[::-1], got)
    # tile b[3] read from set A's side: the same bytes in the other set
    both = np.concatenate([a, b])
    AB = TileSet(lib, both, S)
    assert np.array_equal(Pairs(lib, AB, AB, 1).run([2], [7]), alone)
    assert np.array_equal(Pairs(lib, AB, A, 2).run([7, 2], [2, 2])[0], Pairs(lib, B, A, 1).run([3], [2])[0])
    # a side stream, then graph replay
    i, j = filler_i[:3] + [2] + filler_i[3:], filler_j[:3] + [3] + filler_j[3:]
    want = call.run(i, j)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    call.out.t.fill_(FILL)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert call.launch(stream=side) == 0, lib.rg_last_error()
    side.synchronize()
    assert np.array_equal(call.read(), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        assert call.launch(stream=torch.cuda.current_stream()) == 0, lib.rg_last_error()
    for _ in range(2):
        call.out.t.fill_(FILL)
        call.ws.t.fill_(PATTERN)
        graph.replay()
        assert np.array_equal(call.read(), want)


def test_fp16_build_and_an_index_outside_its_set():
    H, W, S = 23, 25, 2
    a, b = R.correlated_sets(2, H, W, 16, seed=6)
    lib = _abi.load()
    want = Pairs(lib, TileSet(lib, a, S), TileSet(lib, b, S), 2).run([0, 1], [1, 0])
    f16 = _abi.load("f16")
    assert np.array_equal(Pairs(f16, TileSet(f16, a, S), TileSet(f16, b, S), 2).run([0, 1], [1, 0]), want)
    # the host cannot see the indices: one outside its set is never an address, its pair comes back NaN and the others as they were
    got = Pairs(lib, TileSet(lib, a, S), TileSet(lib, b, S), 4).run([0, 2, 1, -1], [1, 0, 0, 0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1])
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()


def test_refused_arguments_launch_nothing():
    lib = _abi.load()
    H, W, S = 23, 25, 2
    a, b = R.correlated_sets(2, H, W, 16, seed=6)
    A, B = TileSet(lib, a, S), TileSet(lib, b, S)
    call = Pairs(lib, A, B, 2)
    call.set_pairs([0, 1], [1, 0])
    bad = [dict(a=None), dict(b=None), dict(ia=None), dict(ib=None), dict(taps=None), dict(out=None), dict(pyr_a=None), dict(pyr_b=None),
           dict(H=10), dict(W=10), dict(H=10, W=10), dict(S=0), dict(S=6), dict(S=3), dict(S=-1), dict(flags=4), dict(flags=8),
           dict(flags=-1), dict(flags=1 << 20), dict(P=-1), dict(Na=0), dict(Nb=0), dict(Nb=-2), dict(ia=call.ia.data_ptr() + 2),
           dict(out=call.out.t.data_ptr() + 4), dict(pyr_a=A.pyr.t.data_ptr() + 1)]
    for kw in bad:
        assert call.launch(**kw) == EINVAL, kw
        assert lib.rg_last_error(), kw
        assert call.untouched(), kw
    for kw in (dict(ws_bytes=call.need - 1), dict(ws_bytes=0), dict(ws=None), dict(ws=call.ws.t.data_ptr() + 4)):
        assert call.launch(**kw) == EWORKSPACE, kw
        assert call.untouched(), kw
    assert call.launch(H=4097, S=1) == EUNSUPPORTED and call.untouched()
    # P == 0 is a valid call that writes nothing, whatever the pointers are
    assert call.launch(P=0) == 0 and call.launch(P=0, a=None, b=None, ia=None, ib=None, out=None, ws=None, ws_bytes=0) == 0
    assert call.untouched()
    assert call.launch(P=0, S=6) == EINVAL and call.launch(P=0, flags=4) == EINVAL
    # the pyramid launch
    pyr = Guarded(torch.full((2 * A.per_tile,), PATTERN, dtype=torch.uint8), PATTERN)

    def pyramid(**kw):
        args = dict(tiles=A.ptr, N=2, H=H, W=W, flags=0, S=S, pyr=pyr.t.data_ptr(), pyr_bytes=2 * A.per_tile)
        args.update(kw)
        return lib.rg_msssim_pyramid(*[args[k] for k in ("tiles", "N", "H", "W", "flags", "S", "pyr", "pyr_bytes")], None)
    for kw in (dict(tiles=None), dict(pyr=None), dict(N=-1), dict(H=10), dict(S=0), dict(S=3), dict(flags=4), dict(pyr=pyr.t.data_ptr() + 1)):
        assert pyramid(**kw) == EINVAL, kw
    assert pyramid(pyr_bytes=2 * A.per_tile - 1) == EWORKSPACE and pyramid(pyr_bytes=0) == EWORKSPACE
    assert pyramid(N=0) == 0 and pyramid(S=1, pyr=None, pyr_bytes=0) == 0
    torch.cuda.synchronize()
    assert bool((pyr.flat == PATTERN).all())
    assert pyramid() == 0
    torch.cuda.synchronize()
    assert torch.equal(pyr.t, A.pyr.t[:2 * A.per_tile]) and _kept(pyr, PATTERN)
    # what was refused left the call usable
    assert np.array_equal(call.run([0, 1], [1, 0]), Pairs(lib, A, B, 2).run([0, 1], [1, 0]))
