"""The image-side kernels op by op, through the C ABI on both builds of the library: the first conv of the critic and the last
transposed conv of the generator (rna_gan_amd/csrc/rg_skinny.hip, with their generic routes and the dispatch of rg_api.hip) and
the critic head kernels (rg_misc.hip).  References, operand builders, bounds and case tables are in tests/image_side_refs.py;
tests/test_image_side_refs_cpu.py checks every condition on the same operands.

A  EXACT INTEGERS, torch.equal against fp32 matrix products of the same integers: one unit row per chunk size, two and three
   chunks per row (the seam), every strip length of last_up, work lists longer than the grid, the rows128 kernels and the general
   ones at 256 x 256, the vector and generic routes; per geometry every form the dispatch offers (sign bits out, sign-bit mask
   in, BatchNorm + LeakyReLU on the staged input, tanh backward and per-workgroup partial rows on the stored output, the three
   weight-gradient entry points); the head kernels on both sides of the rule between their two weight-gradient kernels.
B  GAUSSIAN OPERANDS against fp64 under the element-wise worst-case bound, and tanh on part A's operands (where the
   pre-activation is known exactly) against a bound derived from the recipe.  Each prints "RATIO <op> <case> <build> <value>"
   (profiles/image_side_op_errors.txt records them) and asserts ratio <= 1.
Every case prints "KERNEL <op> <case> <options> <kernel>": the kernel the dispatch gives it (mirrored in image_side_refs and checked
against the library's own queries).  Outputs, workspaces, slabs, partial rows and sign-bit words are exactly as large as their
query says, inside a pattern-filled allocation whose surroundings must keep the pattern; operands sit inside NaN.
"""
import ctypes
import math

import pytest
import torch

import image_side_refs as R
from both_builds import H16
from guarded import DEV, SBITS, Guarded
from test_ops_exact_gpu import _Options

pytestmark = pytest.mark.gpu
both_builds = pytest.mark.parametrize("h16", H16, ids=["bfloat16", "float16"])
NAN = float("nan")
RG_EINVAL, RG_EUNSUPPORTED, RG_EWORKSPACE = -1, -2, -3
INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
PAT = {2: 0xc6c1 - 65536, 4: SBITS, 8: (SBITS << 32) | SBITS}      # finite in bf16 (-24704), fp16 (-6.75), fp32 (SENTINEL)
I = R.I
_ENV = {}


class _Env:
    def __init__(self, h16):
        from rna_gan_amd import _abi
        from rna_gan_amd.ops_hip import HipOps
        self.abi, self.h16 = _abi, h16
        self.ops = HipOps(h16, DEV)
        self.lib = self.ops.lib
        self.H16, self.F32 = self.ops.H16, _abi.RG_F32
        self.other = _abi.RG_F16 if self.H16 == _abi.RG_BF16 else _abi.RG_BF16       # the other build's 16-bit code
        self.build = "bf16" if h16 == torch.bfloat16 else "fp16"
        assert self.lib.rg_storage_dtype() == self.H16

    @property
    def stream(self):
        return self.ops.stream

    def dt(self, c):
        """(dtype code, torch dtype) of a case's activation storage"""
        return (self.F32, torch.float32) if c.storage == "f32" else (self.H16, self.h16)


def _env(h16):
    if h16 not in _ENV:
        _ENV[h16] = _Env(h16)
    return _ENV[h16]


class _G(Guarded):
    """guarded.Guarded for any element size, built on the device: `fill` = NaN around an operand, None = the finite bit pattern
    around (and in) an output"""

    def __init__(self, shape, dtype, fill=None, after=4096, before=128):
        n = int(math.prod(shape))
        self.before, self.n = before, n
        self.flat = torch.empty(before + n + after, dtype=dtype, device=DEV)
        self.ints = self.flat.view(INT[self.flat.element_size()])
        self.pat = PAT[self.flat.element_size()]
        if fill is None:
            self.ints.fill_(self.pat)
        else:
            self.flat.fill_(fill)
        self.t = self.flat[before:before + n].view(shape)

    def surroundings_keep(self, pattern=None):
        head, tail = self.ints[:self.before], self.ints[self.before + self.n:]
        return bool((head == self.pat).all()) and bool((tail == self.pat).all())

    def reset(self):
        self.ints.fill_(self.pat)

    def kept(self, lo=0, hi=None):
        """elements [lo, hi) of the buffer still hold the pattern"""
        return bool((self.ints[self.before + lo:self.before + (self.n if hi is None else hi)] == self.pat).all())

    @property
    def ptr(self):
        return self.t.data_ptr()


def _operand(t, dtype=torch.float32):
    g = _G(tuple(t.shape), dtype, NAN)
    g.t.copy_(t.to(DEV))
    assert torch.equal(g.t.float().cpu(), t.float().cpu()), "the operand is a number of the storage type"
    return g


def _same(got, want, what, layout=None):
    """torch.equal with a report: the first mismatch, and for an image-shaped output its low-resolution column modulo 128 (a
    mistake at a chunk seam sits at 0 or 127)"""
    got, want = got.float(), want.float().to(got.device)
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), what + ": non-finite output"
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = bad[0].tolist()
    where = ""
    if layout == "nhwc":
        where = ", low-resolution column %d = %d (mod 128)" % (first[2], first[2] % 128)
    elif layout == "nchw":
        where = ", low-resolution column %d = %d (mod 128)" % (first[3] // 2, (first[3] // 2) % 128)
    assert False, "%s: %d of %d outputs differ, first at %s%s: got %g, expected %g" % (
        what, bad.shape[0], want.numel(), first, where, float(got[tuple(first)]), float(want[tuple(first)]))


def _ok(E, rc, what):
    torch.cuda.synchronize()
    E.abi.check(rc, what)


def _dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def _tag(c, opts):
    return "%s %s" % (c.name, ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "-")


CASE_IDS = lambda c: c.name


# =============================================================================================================== A: first_down
def _first_down(E, c, xg, wg, bias, slope, bits=None):
    dt, tdt = E.dt(c)
    y = _G((c.N, c.Ho, c.Wo, c.O), tdt)
    if bits is None:
        rc = E.lib.rg_first_down(xg.ptr, wg.ptr, bias.ptr if bias else None, y.ptr, c.N, 2 * c.Ho, 2 * c.Wo, I, c.O, slope, dt, E.stream)
    else:
        rc = E.lib.rg_first_down_bits(xg.ptr, wg.ptr, bias.ptr if bias else None, y.ptr, bits.ptr, c.N, 2 * c.Ho, 2 * c.Wo, I, c.O, slope,
                                      dt, E.stream)
    _ok(E, rc, "rg_first_down")
    assert y.surroundings_keep(), c.name + ": first_down wrote outside y"
    return y.t


@both_builds
@pytest.mark.parametrize("c", R.cases("d"), ids=CASE_IDS)
def test_first_down_exact(c, h16):
    E = _env(h16)
    dt, tdt = E.dt(c)
    p = _dev(R.operands(c))
    r = R.down_refs(c, p)                                          # (conditions asserted again, on the device)
    xg, wg, bg = _operand(p["x"]), _operand(p["w"]), _operand(p["bd"])
    H, W, npix = 2 * c.Ho, 2 * c.Wo, c.N * c.Ho * c.Wo
    masked = E.lib.rg_first_down_masked_supported(H, W, I, c.O, dt)
    assert masked == int(R.rows(c)), "the mirror of the dispatch disagrees with rg_first_down_masked_supported"
    for opts in R.variants(c):
        with _Options(E.lib, **opts):
            tag = _tag(c, opts)
            print("KERNEL first_down %s %s" % (tag, R.kernel_first_down(c, opts)))
            _same(_first_down(E, c, xg, wg, bg, R.SLOPE), r["plain"].to(tdt), tag + " first_down (slope 0.5, bias)", "nhwc")
            _same(_first_down(E, c, xg, wg, None, 1.0), r["lin"].to(tdt), tag + " first_down (slope 1, no bias)", "nhwc")
            if c.O == 64 and c.storage == "h16":
                bits = _G((npix,), torch.int64)
                y = _first_down(E, c, xg, wg, bg, R.SLOPE, bits)
                _same(y, r["plain"].to(tdt), tag + " first_down_bits", "nhwc")
                assert bits.surroundings_keep(), tag + ": wrote outside the sign-bit words"
                stored = R.sign_words(r["plain"].to(tdt).float()).reshape(-1)
                assert torch.equal(stored, r["plain_words"].reshape(-1))
                bad = (bits.t != stored).nonzero()
                assert bad.numel() == 0, "%s: %d sign-bit words differ from the reference's stored values, first at pixel %d" % (
                    tag, bad.shape[0], int(bad[0]))
                packed = _G((npix,), torch.int64)
                _ok(E, E.lib.rg_sign_pack(y.data_ptr(), packed.ptr, npix, 64, dt, E.stream), "rg_sign_pack")
                assert packed.surroundings_keep() and torch.equal(packed.t, bits.t), tag + ": rg_sign_pack of the output differs"
            if masked:
                mb = _G((npix,), torch.int64, 0)
                mb.ints.fill_(-1)                                  # (all-ones around the mask words: a word read past the end multiplies by 1)
                mb.t.copy_(r["m_words"].reshape(-1))
                y = _G((c.N, c.Ho, c.Wo, c.O), tdt)
                _ok(E, E.lib.rg_first_down_masked(xg.ptr, wg.ptr, y.ptr, mb.ptr, R.MSLOPE, c.N, H, W, I, c.O, dt, E.stream),
                    "rg_first_down_masked")
                assert y.surroundings_keep()
                _same(y.t, r["masked"].to(tdt), tag + " first_down_masked", "nhwc")
    if not masked:
        y = _G((c.N, c.Ho, c.Wo, c.O), tdt)
        one = torch.zeros(npix, dtype=torch.int64, device=DEV)
        rc = E.lib.rg_first_down_masked(xg.ptr, wg.ptr, y.ptr, one.data_ptr(), R.MSLOPE, c.N, H, W, I, c.O, dt, E.stream)
        torch.cuda.synchronize()
        assert rc == RG_EUNSUPPORTED and y.kept() and y.surroundings_keep(), c.name + ": rg_first_down_masked where the query says no"


@both_builds
@pytest.mark.parametrize("npix", [1, 31, 32, 33, 257])
def test_sign_pack_alone(npix, h16):
    """sign_pack64_kernel: 8 lanes per pixel, the last block ragged; +0 and -0 are "not positive" """
    E = _env(h16)
    a = R.signed_zeros((npix, 64), torch.Generator().manual_seed(300 + npix))
    a[0, 0], a[0, 63], a[-1, 1], a[-1, 62] = 1.0, -0.0, 0.0, 1.0
    ag = _operand(a, h16)
    assert torch.equal(torch.signbit(ag.t.float()).cpu(), torch.signbit(a)), "the signed zeros survive the copy"
    bits = _G((npix,), torch.int64)
    _ok(E, E.lib.rg_sign_pack(ag.ptr, bits.ptr, npix, 64, E.H16, E.stream), "rg_sign_pack")
    assert bits.surroundings_keep(), "wrote outside the words"
    assert torch.equal(bits.t.cpu(), R.sign_words(a))
    for C, dtype in ((32, E.H16), (64, E.F32)):
        bits.reset()
        rc = E.lib.rg_sign_pack(ag.ptr, bits.ptr, npix, C, dtype, E.stream)
        torch.cuda.synchronize()
        assert rc == RG_EUNSUPPORTED and bits.kept()


# =============================================================================================================== A: last_up
def _last_up(E, c, ag, wg, bias, tanh=0):
    dt, _ = E.dt(c)
    y = _G((c.N, I, 2 * c.Ho, 2 * c.Wo), torch.float32)
    _ok(E, E.lib.rg_last_up(ag.ptr, wg.ptr, bias.ptr if bias else None, y.ptr, c.N, c.Ho, c.Wo, c.O, I, tanh, dt, E.stream), "rg_last_up")
    assert y.surroundings_keep(), c.name + ": last_up wrote outside y"
    return y.t


def _post(E, c, ag, wg, tb, want_part, what):
    """rg_last_up_post -> (y, the partial rows or None)"""
    dt, _ = E.dt(c)
    nb = E.lib.rg_last_up_post_blocks(c.N, c.Ho, c.Wo, c.O, I, dt)
    assert nb == R.post_blocks(c) > 0
    y = _G((c.N, I, 2 * c.Ho, 2 * c.Wo), torch.float32)
    part = _G((nb, 4), torch.float32) if want_part else None
    _ok(E, E.lib.rg_last_up_post(ag.ptr, wg.ptr, y.ptr, c.N, c.Ho, c.Wo, c.O, I, dt, tb.ptr if tb else None, part.ptr if part else None,
                                 E.stream), "rg_last_up_post")
    assert y.surroundings_keep(), what + ": wrote outside y"
    assert part is None or (part.surroundings_keep() and not bool((part.ints[part.before:part.before + part.n] == part.pat).any())), \
        what + ": wrote outside the partial rows, or left one unwritten"
    return y.t, (part.t if part else None)


def _check_rows(c, part, v, grain, what):
    """the partial rows [blocks][4] against the reference v (fp64, NCHW).  grain: v is a multiple of 1 / grain (4 with the 0.75 of
    the tanh backward).  Channel sums: exact where sum |v| < 2^24 / grain; the sum of squares: exact where sum v^2 < 2^24 / grain^2,
    otherwise within n 2^-24 sum v^2 -- both asked of the rows summed in fp64, and row by row of the rows the reference predicts."""
    v = v.double()
    got, want = part.double().sum(0), R.post_sums(v)
    assert part.shape == (R.post_blocks(c), 4)
    sabs = float(v.abs().sum((0, 2, 3)).max())
    if sabs < 2 ** 24 / grain:
        assert torch.equal(got[:3], want[:3]), "%s: channel sums %s, expected %s" % (what, got[:3].tolist(), want[:3].tolist())
    else:
        assert float((got[:3] - want[:3]).abs().max()) <= v[:, 0].numel() * 2.0 ** -24 * sabs, what + ": channel sums"
    if float(want[3]) < 2 ** 24 / grain ** 2:
        assert float(got[3]) == float(want[3]), "%s: sum of squares %r, expected %r" % (what, float(got[3]), float(want[3]))
    else:
        assert abs(float(got[3] - want[3])) <= v.numel() * 2.0 ** -24 * float(want[3]), what + ": sum of squares"
    rows = R.post_rows(c, v)
    rabs = R.post_rows(c, v.abs())
    ex = rabs[:, :3].max(1).values < 2 ** 24 / grain
    assert torch.equal(part.double()[ex][:, :3], rows[ex][:, :3]), what + ": a workgroup's channel sums"
    ex = rows[:, 3] < 2 ** 24 / grain ** 2
    assert torch.equal(part.double()[ex][:, 3], rows[ex][:, 3]), what + ": a workgroup's sum of squares"
    return int(ex.sum())


@both_builds
@pytest.mark.parametrize("c", R.cases("u"), ids=CASE_IDS)
def test_last_up_exact(c, h16):
    E = _env(h16)
    dt, tdt = E.dt(c)
    p = _dev(R.operands(c))
    r = R.up_refs(c, p)
    ag, wg, bg = _operand(p["a"], tdt), _operand(p["w"]), _operand(p["bu"])
    fused = R.rows(c)
    assert E.lib.rg_last_up_pre_supported(c.Wo, c.O, I, dt) == int(fused)
    assert E.lib.rg_last_up_post_blocks(c.N, c.Ho, c.Wo, c.O, I, dt) == R.post_blocks(c)
    if fused:
        bn = [_operand(p[k]) for k in ("mean", "invstd", "gamma", "beta")]
        tb = _operand(p["tb"])
        zg = _operand(r["a_zero"], tdt)
        assert torch.equal(r["act"].to(tdt).float(), r["act"])
    for opts in R.variants(c):
        with _Options(E.lib, **opts):
            tag = _tag(c, opts)
            print("KERNEL last_up %s %s" % (tag, R.kernel_last_up(c, opts)))
            _same(_last_up(E, c, ag, wg, None), r["plain"], tag + " last_up", "nchw")
            _same(_last_up(E, c, ag, wg, bg), r["bias"], tag + " last_up (bias)", "nchw")
            if not fused:
                continue
            y = _G((c.N, I, 2 * c.Ho, 2 * c.Wo), torch.float32)
            _ok(E, E.lib.rg_last_up_pre(ag.ptr, wg.ptr, bg.ptr, y.ptr, bn[0].ptr, bn[1].ptr, bn[2].ptr, bn[3].ptr, R.SLOPE, c.N, c.Ho,
                                        c.Wo, c.O, I, 0, dt, E.stream), "rg_last_up_pre")
            assert y.surroundings_keep()
            _same(y.t, r["pre"], tag + " last_up_pre (padding must stay zero: BN(0) != 0)", "nchw")
            y, part = _post(E, c, ag, wg, None, True, tag)
            _same(y, r["plain"], tag + " last_up_post (partial rows)", "nchw")
            n = _check_rows(c, part, r["plain"], 1, tag + " last_up_post")
            y, part = _post(E, c, ag, wg, tb, True, tag)
            _same(y, r["post_tb"], tag + " last_up_post (tanh backward, partial rows)", "nchw")
            n += _check_rows(c, part, r["post_tb"], 4, tag + " last_up_post (tanh backward)")
            print("ROWS last_up_post %s: %d sums of squares of %d workgroups compared exactly" % (tag, n, 2 * part.shape[0]))
            y, _ = _post(E, c, ag, wg, tb, False, tag)
            _same(y, r["post_tb"], tag + " last_up_post (tanh backward alone)", "nchw")
            y, part = _post(E, c, zg, wg, None, True, tag)
            _same(y, r["zero"], tag + " last_up_post (first strip of the input zero)", "nchw")
            _check_rows(c, part, r["zero"], 1, tag + " last_up_post (first strip of the input zero)")
    if not fused:
        y = _G((c.N, I, 2 * c.Ho, 2 * c.Wo), torch.float32)
        part = _G((4, 4), torch.float32)
        ch = _operand(torch.ones(c.O))
        rc = E.lib.rg_last_up_pre(ag.ptr, wg.ptr, bg.ptr, y.ptr, ch.ptr, ch.ptr, ch.ptr, ch.ptr, R.SLOPE, c.N, c.Ho, c.Wo, c.O, I, 0, dt, E.stream)
        torch.cuda.synchronize()
        assert rc == RG_EUNSUPPORTED and y.kept() and y.surroundings_keep(), c.name + ": rg_last_up_pre where the query says no"
        rc = E.lib.rg_last_up_post(ag.ptr, wg.ptr, y.ptr, c.N, c.Ho, c.Wo, c.O, I, dt, None, part.ptr, E.stream)
        torch.cuda.synchronize()
        assert rc == RG_EUNSUPPORTED and y.kept() and part.kept(), c.name + ": rg_last_up_post where the query says no"


# =============================================================================================================== A: weight gradient
def _slab_sum(buf, n, elems):
    return buf.t[:n * elems].view(n, elems).double().sum(0)


@both_builds
@pytest.mark.parametrize("c", R.cases("w"), ids=CASE_IDS)
def test_skinny_wgrad_exact(c, h16):
    E = _env(h16)
    lib = E.lib
    dt, tdt = E.dt(c)
    p = _dev(R.operands(c))
    r = R.wgrad_refs(c, p)
    dw_ref, db_ref = r["dw"], r["db"]
    ag, xg = _operand(p["a"], tdt), _operand(p["x"])
    dims = (c.N, c.Ho, c.Wo, c.O, I)
    elems = c.O * 48
    for opts in R.variants(c):
        with _Options(lib, **opts):
            tag = _tag(c, opts)
            print("KERNEL skinny_wgrad %s %s" % (tag, R.kernel_wgrad(c, opts)))
            wsb = int(lib.rg_skinny_wgrad_workspace_bytes(*dims))
            ws = _G((wsb // 4,), torch.float32, after=8192) if wsb else None
            wp = ws.ptr if ws else None
            # rg_skinny_wgrad: over the 7.0 fill, then accumulated
            dw = _G((c.O, I, 4, 4), torch.float32)
            dw.t.fill_(7.0)
            _ok(E, lib.rg_skinny_wgrad(ag.ptr, xg.ptr, dw.ptr, *dims, dt, 0, wp, wsb, E.stream), "rg_skinny_wgrad")
            _same(dw.t, dw_ref, tag + " skinny_wgrad")
            _ok(E, lib.rg_skinny_wgrad(ag.ptr, xg.ptr, dw.ptr, *dims, dt, 1, wp, wsb, E.stream), "rg_skinny_wgrad")
            _same(dw.t, 2 * dw_ref, tag + " skinny_wgrad (accumulate)")
            assert dw.surroundings_keep() and (ws is None or ws.surroundings_keep()), tag + ": wrote outside dw or the workspace"
            # rg_skinny_wgrad_bias
            done = ctypes.c_int(-1)
            db = _G((c.O,), torch.float32)
            dw.t.fill_(7.0)
            _ok(E, lib.rg_skinny_wgrad_bias(ag.ptr, xg.ptr, dw.ptr, db.ptr, *dims, dt, 0, 0, wp, wsb, ctypes.addressof(done), E.stream),
                "rg_skinny_wgrad_bias")
            _same(dw.t, dw_ref, tag + " skinny_wgrad_bias")
            want_done = int(R.kernel_wgrad(c, opts) == "skinny_wgrad_rows128_kernel")
            assert done.value == want_done, tag + ": *bias_done_out = %d" % done.value
            if done.value:
                _same(db.t, db_ref, tag + " bias gradient")
                _ok(E, lib.rg_skinny_wgrad_bias(ag.ptr, xg.ptr, dw.ptr, db.ptr, *dims, dt, 1, 1, wp, wsb, ctypes.addressof(done), E.stream),
                    "rg_skinny_wgrad_bias")
                _same(dw.t, 2 * dw_ref, tag + " skinny_wgrad_bias (accumulate)")
                _same(db.t, 2 * db_ref, tag + " bias gradient (accumulate)")
            else:
                assert db.kept(), tag + ": the bias gradient was written although *bias_done_out = 0"
            assert dw.surroundings_keep() and db.surroundings_keep() and (ws is None or ws.surroundings_keep())
            # a workspace one byte short
            if wsb:
                dw.reset()
                ws.reset()
                rc = lib.rg_skinny_wgrad(ag.ptr, xg.ptr, dw.ptr, *dims, dt, 0, wp, wsb - 1, E.stream)
                torch.cuda.synchronize()
                assert rc == RG_EWORKSPACE and dw.kept() and ws.kept(), tag + ": rg_skinny_wgrad with a workspace one byte short: %d" % rc
                done.value = -1
                rc = lib.rg_skinny_wgrad_bias(ag.ptr, xg.ptr, dw.ptr, db.ptr, *dims, dt, 0, 0, wp, wsb - 1, ctypes.addressof(done), E.stream)
                torch.cuda.synchronize()
                assert rc == RG_EWORKSPACE and done.value == 0 and dw.kept() and ws.kept(), tag + ": rg_skinny_wgrad_bias, one byte short"
            # rg_skinny_wgrad_slabs
            nslab_want = R.wgrad_slabs(c, opts)
            slab = _G((max(wsb, 4 * elems) // 4,), torch.float32, after=8192)
            bslab = _G((R.SK_ROWS_BLOCKS, c.O), torch.float32)
            ns, done = ctypes.c_int(-1), ctypes.c_int(-1)
            _ok(E, lib.rg_skinny_wgrad_slabs(ag.ptr, xg.ptr, *dims, dt, slab.ptr, slab.n * 4, ctypes.addressof(ns), bslab.ptr,
                                             ctypes.addressof(done), E.stream), "rg_skinny_wgrad_slabs")
            assert ns.value == nslab_want, "%s: *nslab_out = %d, the mirror of the dispatch says %d" % (tag, ns.value, nslab_want)
            assert slab.surroundings_keep() and slab.kept(ns.value * elems), tag + ": wrote behind the slabs it reports"
            assert not bool((slab.ints[slab.before:slab.before + ns.value * elems] == slab.pat).any()), tag + ": a slab entry left unwritten"
            if ns.value:
                got = _slab_sum(slab, ns.value, elems).view(c.O, I, 4, 4)
                assert torch.equal(got, dw_ref.double()), "%s: the slabs summed in fp64 differ in %d entries" % (tag, int((got != dw_ref.double()).sum()))
                assert done.value == want_done
                if done.value:
                    assert torch.equal(bslab.t[:ns.value].double().sum(0), db_ref.double()), tag + ": bias slabs"
                assert bslab.surroundings_keep() and bslab.kept(ns.value * c.O if done.value else 0)
                slab.reset()
                need = ns.value * elems * 4
                rc = lib.rg_skinny_wgrad_slabs(ag.ptr, xg.ptr, *dims, dt, slab.ptr, need - 1, ctypes.addressof(ns), None, None, E.stream)
                torch.cuda.synchronize()
                assert rc == RG_EWORKSPACE and ns.value == 0 and slab.kept(), tag + ": rg_skinny_wgrad_slabs, one byte short"
            else:
                assert done.value == 0 and bslab.kept(), tag + ": no slab form, yet something was written"


# =============================================================================================================== A: contracts
@both_builds
def test_supported_queries_on_both_sides_of_each_rule(h16):
    """host side only: O = 64 against 128 and 32, Wo = 32 against 16 (and 48, 128, 256, 192), the build's 16-bit type against
    fp32 and against the other build's code, I = 3 against 4"""
    E = _env(h16)
    lib, Hh = E.lib, E.H16
    md = lambda Wo, O, dt, I_=3: lib.rg_first_down_masked_supported(16, 2 * Wo, I_, O, dt)
    pre = lambda Wo, O, dt, I_=3: lib.rg_last_up_pre_supported(Wo, O, I_, dt)
    post = lambda Wo, O, dt, I_=3: int(lib.rg_last_up_post_blocks(2, 8, Wo, O, I_, dt) > 0)
    for q in (md, pre, post):
        assert q(32, 64, Hh) == 1 and q(32, 128, Hh) == 0 and q(32, 32, Hh) == 0
        assert q(16, 64, Hh) == 0 and q(48, 64, Hh) == 0 and q(64, 64, Hh) == 1 and q(128, 64, Hh) == 1
        assert q(256, 64, Hh) == 1 and q(192, 64, Hh) == 0
        assert q(32, 64, E.F32) == 0 and q(32, 64, E.other) == 0 and q(32, 64, Hh, 4) == 0
    blocks = lambda N, Ho, Wo: lib.rg_last_up_post_blocks(N, Ho, Wo, 64, 3, Hh)
    assert blocks(1, 1, 32) == 1 and blocks(1, 32, 32) == 2 and blocks(1, 17, 32) == 17 and blocks(2, 24, 64) == 4
    assert blocks(5, 113, 32) == 512 and blocks(7, 128, 128) == 56 and blocks(2, 2, 384) == 6 and blocks(64, 128, 128) == 512
    # the workspace query covers every kernel the entry points may pick: the row kernels' grid and the bias partials behind it
    for c in R.cases("w"):
        wsb = int(lib.rg_skinny_wgrad_workspace_bytes(c.N, c.Ho, c.Wo, c.O, 3))
        if R.skinny(c.O):
            assert wsb >= R.SK_ROWS_BLOCKS * (c.O * 48 + 64) * 4, c.name


# =============================================================================================================== A: head
def _head_a(E, a, tdt, off=0):
    """a [N, 16, C] in the storage type inside NaN, `off` elements past a 256-byte boundary"""
    g = _G((a.numel() + off,), tdt, NAN)
    g.t[off:].copy_(a.reshape(-1).to(DEV))
    return g, g.ptr + off * g.t.element_size()


@both_builds
@pytest.mark.parametrize("storage", ["h16", "f32"])
@pytest.mark.parametrize("C", R.HEAD_C)
@pytest.mark.parametrize("N", R.HEAD_N)
def test_head_kernels_exact(N, C, storage, h16):
    E = _env(h16)
    lib = E.lib
    dt, tdt = (E.F32, torch.float32) if storage == "f32" else (E.H16, h16)
    a, w, gh = R.head_operands(N, C)
    ad, wd, ghd = a.to(DEV), w.to(DEV), gh.to(DEV)
    wg, ghg = _operand(w), _operand(gh)
    bias = _operand(torch.tensor([R.HEAD_BIAS]))
    offsets = [0, 4] if storage == "h16" else [0]                   # 4 elements = 8 bytes off a 16-byte boundary
    for off in offsets:
        _, ap = _head_a(E, a, tdt, off)
        kernel = "head_wgrad_bf16_kernel" if storage == "h16" and ap % 16 == 0 and C % 8 == 0 else "head_wgrad_kernel<T>"
        assert (kernel == "head_wgrad_bf16_kernel") == (storage == "h16" and off == 0 and C % 8 == 0)
        print("KERNEL head_wgrad N=%d,C=%d,%s,offset=%d %s" % (N, C, storage, 2 * off, kernel))
        for with_bias in (False, True):
            h, out = _G((N,), torch.float32), _G((N,), torch.float32)
            if with_bias:
                rc = lib.rg_head_fwd_bias(ap, wg.ptr, bias.ptr, h.ptr, out.ptr, N, C, R.SLOPE, dt, E.stream)
            else:
                rc = lib.rg_head_fwd(ap, wg.ptr, h.ptr, out.ptr, N, C, R.SLOPE, dt, E.stream)
            _ok(E, rc, "rg_head_fwd")
            h_ref, out_ref = R.head_fwd(ad, wd, R.HEAD_BIAS if with_bias else None, R.SLOPE)
            assert float((ad.abs().reshape(N, -1) @ R.head_wq(wd).abs()).max()) + 3 <= R.L32
            _same(h.t, h_ref, "head_fwd h (N %d, C %d, bias %s)" % (N, C, with_bias))
            _same(out.t, out_ref, "head_fwd out (N %d, C %d, bias %s)" % (N, C, with_bias))
            assert h.surroundings_keep() and out.surroundings_keep()
        dw_ref = R.head_wgrad(ghd, ad)
        dw = _G((C, 16), torch.float32)
        dw.t.fill_(7.0)
        _ok(E, lib.rg_head_wgrad(ghg.ptr, ap, dw.ptr, N, C, dt, 0, E.stream), "rg_head_wgrad")
        _same(dw.t, dw_ref, "head_wgrad (N %d, C %d, %s)" % (N, C, kernel))
        _ok(E, lib.rg_head_wgrad(ghg.ptr, ap, dw.ptr, N, C, dt, 1, E.stream), "rg_head_wgrad")
        _same(dw.t, 2 * dw_ref, "head_wgrad accumulate (N %d, C %d, %s)" % (N, C, kernel))
        assert dw.surroundings_keep()
    ga = _G((N, 16 * C), tdt)
    _ok(E, lib.rg_head_bwd_data(ghg.ptr, wg.ptr, ga.ptr, N, C, dt, E.stream), "rg_head_bwd_data")
    _same(ga.t, R.head_bwd_data(ghd, wd).to(tdt), "head_bwd_data (N %d, C %d)" % (N, C))
    assert ga.surroundings_keep()


@both_builds
@pytest.mark.parametrize("N", R.HEAD_N + [257])
def test_head_grad_exact(N, h16):
    E = _env(h16)
    h = R.head_h_values(N)
    hg = _operand(h)
    assert torch.equal(torch.signbit(hg.t).cpu(), torch.signbit(h))
    gh = _G((N,), torch.float32)
    _ok(E, E.lib.rg_head_grad(hg.ptr, gh.ptr, N, R.HEAD_COEF, R.SLOPE, E.stream), "rg_head_grad")
    _same(gh.t, R.head_grad(h, R.HEAD_COEF, R.SLOPE), "head_grad (N %d)" % N)
    assert gh.surroundings_keep()


# =============================================================================================================== B: fp64 bounds
def _ratio(op, c, E, got, ref, bnd, tag=""):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (op, c.name)
    ratio = float(((got - ref).abs() / bnd).max())
    print("RATIO %s %s%s %s %.4f" % (op, c.name, tag, E.build, ratio))
    assert ratio <= 1.0, "%s %s%s (%s): worst |err| / bound = %.3f" % (op, c.name, tag, E.build, ratio)
    return ratio


B_CASES = ["row32_h2", "row128", "seam2", "seam3", "strips1", "units775", "strips565", "r128_n1", "o4", "o128", "w16", "f32_o64"]


@both_builds
@pytest.mark.parametrize("name", B_CASES)
def test_gaussian_operands_within_the_worst_case_bound_of_fp64(name, h16):
    """|got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25 element by element.  The row kernels and the vector kernels of
    rg_skinny.hip on 16-bit storage round the image and the weights to the storage type (exact products: K roundings); the generic
    GEMM, fp32 storage and the vector weight-gradient kernel use the fp32 operands as they are (every product rounded too: 2 K)."""
    E = _env(h16)
    c = R.BY_NAME[name]
    dt, tdt = E.dt(c)
    u = R.UNIT[tdt]
    p = _dev(R.gauss_operands(c))
    x, w = p["x"], p["w"]
    a = p["a"].to(tdt)
    xg, wg, ag = _operand(x), _operand(w), _operand(a, tdt)
    D = torch.float64
    xq, wq = x.to(tdt).to(D), w.to(tdt).to(D)                      # (fp32 storage: as they are)
    xf, wf, ad = x.to(D), w.to(D), a.to(D)
    opts_list = [{"f32mma": 0}, {"f32mma": 1}] if c.storage == "f32" else R.variants(c)
    for opts in opts_list:
        with _Options(E.lib, **opts):
            tag = "" if not opts else "[%s]" % ",".join("%s=%d" % kv for kv in sorted(opts.items()))
            if "d" in c.ops:
                as_is = R.kernel_first_down(c, opts) == "rg_generic_first_down" or c.storage == "f32"
                xs, ws, K = (xf, wf, 2 * R.K_DOWN) if as_is else (xq, wq, R.K_DOWN)
                got = _first_down(E, c, xg, wg, None, 1.0)
                _ratio("first_down", c, E, got, R.first_down(xs, ws), R.bound(R.first_down(xs, ws), R.first_down(xs.abs(), ws.abs()), K, u), tag)
            if "u" in c.ops:
                as_is = R.kernel_last_up(c, opts) == "rg_generic_last_up" or c.storage == "f32"
                ws, K = (wf, 8 * c.O) if as_is else (wq, 4 * c.O)
                got = _last_up(E, c, ag, wg, None)
                _ratio("last_up", c, E, got, R.last_up(ad, ws), R.bound(R.last_up(ad, ws), R.last_up(ad.abs(), ws.abs()), K, 0.0), tag)
            if "w" in c.ops:
                rowk = R.kernel_wgrad(c, opts).startswith("skinny_wgrad_rows")
                xs, K = (xq, c.N * c.Ho * c.Wo) if rowk else (xf, 2 * c.N * c.Ho * c.Wo)
                dims = (c.N, c.Ho, c.Wo, c.O, I)
                wsb = int(E.lib.rg_skinny_wgrad_workspace_bytes(*dims))
                ws_ = _G((max(wsb, 4) // 4,), torch.float32, after=8192)
                dw = _G((c.O, I, 4, 4), torch.float32)
                _ok(E, E.lib.rg_skinny_wgrad(ag.ptr, xg.ptr, dw.ptr, *dims, dt, 0, ws_.ptr, wsb, E.stream), "rg_skinny_wgrad")
                assert dw.surroundings_keep() and ws_.surroundings_keep()
                _ratio("skinny_wgrad", c, E, dw.t, R.wgrad(ad, xs), R.bound(R.wgrad(ad, xs), R.wgrad(ad.abs(), xs.abs()), K, 0.0), tag)


TANH_CASES = ["row64", "seam2", "strips1", "r128_n1", "o128", "w16", "f32_o64", "o4"]


@both_builds
@pytest.mark.parametrize("name", TANH_CASES)
def test_tanh_of_last_up_on_exact_pre_activations(name, h16):
    """part A's integer operands with a bias of k 2^-6: the pre-activation is an fp32 number known exactly, so |got - tanh64(pre)|
    is the error of the function alone.  Row kernels: the recipe on the hardware units against R.TANH_RECIPE_BOUND (absolute);
    vector and generic kernels call tanhf: R.TANH_LIBM_ULPS ulp of the result."""
    E = _env(h16)
    c = R.BY_NAME[name]
    dt, tdt = E.dt(c)
    p = _dev(R.operands(c))
    bias = R.TANH_BIAS.to(DEV)
    pre = R.last_up(p["a"], p["w"], bias)
    assert torch.equal(pre * 64, (pre * 64).round()) and float(pre.abs().max()) * 64 < 2 ** 24
    small = int((pre.abs() < 4).sum())
    assert small >= 200 and int(torch.unique(pre[pre.abs() < 4]).numel()) >= 20, "the case has pre-activations where tanh is not saturated"
    ref = torch.tanh(pre.double())
    ag, wg, bg = _operand(p["a"], tdt), _operand(p["w"]), _operand(bias)
    for opts in R.variants(c):
        with _Options(E.lib, **opts):
            kernel = R.kernel_last_up(c, opts)
            libm = "rows" not in kernel
            got = _last_up(E, c, ag, wg, bg, tanh=1)
            assert float(got.abs().max()) <= 1.0
            bnd = R.tanh_bound(ref, libm) + (2.0 ** -149 if libm else 0.0)
            _ratio("tanh", c, E, got, ref, bnd, "[%s]" % kernel)
