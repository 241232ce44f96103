"""rg_resize_bilinear01 and rg_moments_update (include/rnagan_hip.h, rna_gan_amd/csrc/rg_fidstat.hip) op by op through ctypes,
on both builds of the library, against the numpy restatements of tests/fid_device_refs.py (pinned without a GPU by
tests/test_fid_device_refs_cpu.py).

Outputs live inside allocations pre-filled with one finite pattern (a write outside the output changes it); operands live
inside allocations whose remainder is NaN (fp32) or 255 (uint8 drawn from [0, 200]): a tap, row or column read outside the
operand shows in the result.  Those reads stay inside the allocations, so nothing can fault.

Resize shapes: (1,1)->(3,3) and (2,3)->(5,4) both clamps; (5,7)->(7,5) up on one axis, down on the other; (40,24)->(17,11)
downscale with taps skipped; (8,8)->(8,8) identity, bit-exact; (16,16)->(19,19); (13,9)->(299,299); (256,256)->(299,299) at
N = 1, the one shape at which fp32 coordinates would show (1.4e-5 against the 4.8e-7 bound).
Moments shapes: F below, at and above the 16-wide thread tile, around the kernel's 64-wide workgroup tile (63, 64, 65, 80)
and across two of them (130: three tiles per side, off-diagonal tiles with a ragged edge); n around the 4-row register
step and the 32-row staging pass (0, 1, 3, 4, 5, 37) and over several passes (259); ldx = F and F + 5 (unaligned rows)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from fid_device_refs import RESIZE_BOUND, moments_int, moments_ld, resize_ref, tap_f32, tap_u8
from guarded import DEV, SBITS, Guarded
from vae_fid_refs import SENTINEL, bits

BUILDS = ["bf16", "f16"]
RESIZE_CASES = [(1, 1, 3, 3), (2, 3, 5, 4), (5, 7, 7, 5), (40, 24, 17, 11), (8, 8, 8, 8), (16, 16, 19, 19), (13, 9, 299, 299),
                (256, 256, 299, 299)]
FORMS = ["u8_nchw", "u8_nhwc", "f32_nchw_pm1", "f32_nhwc_01"]
U8_MAX = 200


# ------------------------------------------------------------------ resize
_SRC = {}


def _logical(form, N, H, W, seed_extra=0):
    """the batch as a logical (N, 3, H, W) numpy array (computed once per key, never modified) and its (mul, add)"""
    key = ("u8" if form.startswith("u8") else form.split("_")[-1], N, H, W, seed_extra)
    if key not in _SRC:
        rng = np.random.default_rng(7000 + 131 * H + 17 * W + N + seed_extra)
        if form.startswith("u8"):
            a = rng.integers(0, U8_MAX + 1, size=(N, 3, H, W), dtype=np.uint8)
        elif form.endswith("pm1"):
            a = rng.uniform(-1, 1, size=(N, 3, H, W)).astype(np.float32)
        else:
            a = rng.uniform(0, 1, size=(N, 3, H, W)).astype(np.float32)
        a.setflags(write=False)
        _SRC[key] = a
    return _SRC[key]


def _taps(form, a):
    if form.startswith("u8"):
        return tap_u8(a), (1.0, 0.0)
    mul, add = (0.5, 0.5) if form.endswith("pm1") else (1.0, 0.0)
    return tap_f32(a, mul, add), (mul, add)


def _place(form, a):
    """(guarded allocation, data pointer, element strides (sn, sc, sh, sw), dtype code) of the logical batch `a` in the memory
    layout of `form`; the surroundings are NaN / 255"""
    N, C, H, W = a.shape
    nhwc = "nhwc" in form
    mem = np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1))) if nhwc else a
    g = Guarded(torch.from_numpy(mem.copy()), 255 if form.startswith("u8") else float("nan"), before=256, after=8192)
    strides = (H * W * C, 1, W * C, C) if nhwc else (C * H * W, H * W, W, 1)
    return g, g.t.data_ptr(), strides, (_abi.RG_U8 if form.startswith("u8") else _abi.RG_F32)


def _out(N, Ho, Wo):
    return Guarded(torch.full((N, 3, Ho, Wo), SENTINEL, dtype=torch.float32), SENTINEL, before=256, after=8192)


def _resize(lib, ptr, dtype, strides, mul, add, out, N, C, H, W, Ho, Wo):
    rc = lib.rg_resize_bilinear01(ptr, dtype, strides[0], strides[1], strides[2], strides[3], mul, add,
                                  None if out is None else out.t.data_ptr(), N, C, H, W, Ho, Wo, None)
    torch.cuda.synchronize()
    return rc


def _check_resize(got, taps, Ho, Wo, form, what):
    want = resize_ref(taps, Ho, Wo)
    assert np.isfinite(got).all(), "%s: a tap outside the image was read (non-finite output)" % what
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: max |got - restatement| %.3g (bound %.3g)" % (what, err, RESIZE_BOUND))
    assert err <= RESIZE_BOUND, what
    assert got.min() >= 0.0 and got.max() <= 1.0, what
    if form.startswith("u8"):
        assert float(got.max()) <= U8_MAX / 255.0 + RESIZE_BOUND, "%s: a 255 outside the image leaked in" % what
    if (taps.shape[2], taps.shape[3]) == (Ho, Wo):
        assert np.array_equal(got.view(np.uint32), taps.view(np.uint32)), "%s: identity sizes must return the taps bit for bit" % what


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_resize(half, form, case):
    lib = _abi.load(half)
    H, W, Ho, Wo = case
    for N in ((1,) if H == 256 else (1, 2)):
        a = _logical(form, N, H, W)
        taps, (mul, add) = _taps(form, a)
        src, ptr, strides, dtype = _place(form, a)
        out = _out(N, Ho, Wo)
        rc = _resize(lib, ptr, dtype, strides, mul, add, out, N, 3, H, W, Ho, Wo)
        assert rc == 0, lib.rg_last_error()
        assert out.surroundings_keep(SBITS), "rg_resize_bilinear01 wrote outside its output"
        _check_resize(out.t.cpu().numpy(), taps, Ho, Wo, form, "%s %s N=%d %s" % (half, form, N, case))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("form", ["u8_nchw", "f32_nchw_pm1"])
def test_resize_slice_of_a_larger_batch(half, form):
    """channels 1..3 of images 1..2 of a (4, 5, H, W) batch: sn = 5 H W > C H W, the data pointer inside the allocation"""
    lib = _abi.load(half)
    H, W, Ho, Wo = 13, 9, 17, 21
    rng = np.random.default_rng(99)
    big = rng.integers(0, U8_MAX + 1, size=(4, 5, H, W), dtype=np.uint8) if form.startswith("u8") else \
        rng.uniform(-1, 1, size=(4, 5, H, W)).astype(np.float32)
    a = np.ascontiguousarray(big[1:3, 1:4])
    taps, (mul, add) = _taps(form, a)
    g = Guarded(torch.from_numpy(big), 255 if form.startswith("u8") else float("nan"), before=256, after=8192)
    view = g.t[1:3, 1:4]
    assert view.stride(0) == 5 * H * W > 3 * H * W
    out = _out(2, Ho, Wo)
    rc = _resize(lib, view.data_ptr(), _abi.RG_U8 if form.startswith("u8") else _abi.RG_F32, view.stride(), mul, add, out,
                 2, 3, H, W, Ho, Wo)
    assert rc == 0, lib.rg_last_error()
    assert out.surroundings_keep(SBITS)
    _check_resize(out.t.cpu().numpy(), taps, Ho, Wo, form, "%s %s slice" % (half, form))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("form", ["u8_nchw", "u8_nhwc"])
def test_resize_of_a_white_image_stays_white(half, form):
    lib = _abi.load(half)
    for H, W, Ho, Wo in [(5, 7, 7, 5), (13, 9, 299, 299), (40, 24, 17, 11)]:
        a = np.full((2, 3, H, W), 255, dtype=np.uint8)
        src, ptr, strides, dtype = _place(form, a)
        out = _out(2, Ho, Wo)
        assert _resize(lib, ptr, dtype, strides, 1.0, 0.0, out, 2, 3, H, W, Ho, Wo) == 0, lib.rg_last_error()
        got = out.t.cpu().numpy()
        assert float(got.min()) >= 1.0 - RESIZE_BOUND and float(got.max()) <= 1.0 and out.surroundings_keep(SBITS)


@pytest.mark.parametrize("half", BUILDS)
def test_resize_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    N, H, W, Ho, Wo = 2, 5, 7, 7, 5
    a = _logical("f32_nchw_pm1", N, H, W)
    src, ptr, strides, dtype = _place("f32_nchw_pm1", a)
    out = _out(N, Ho, Wo)
    good = dict(ptr=ptr, dtype=dtype, N=N, C=3, H=H, W=W, Ho=Ho, Wo=Wo, out=out)
    bad_calls = {"src = NULL": dict(ptr=None), "dst = NULL": dict(out=None), "N < 0": dict(N=-1), "C = 0": dict(C=0),
                 "H = 0": dict(H=0), "W = -3": dict(W=-3), "Ho = 0": dict(Ho=0), "Wo = 0": dict(Wo=0),
                 "16-bit source": dict(dtype=_abi.RG_BF16), "fp16 source": dict(dtype=_abi.RG_F16), "dtype 7": dict(dtype=7)}
    for what, change in bad_calls.items():
        k = dict(good, **change)
        rc = _resize(lib, k["ptr"], k["dtype"], strides, 0.5, 0.5, k["out"], k["N"], k["C"], k["H"], k["W"], k["Ho"], k["Wo"])
        assert rc == -1, what
        assert b"resize_bilinear01" in lib.rg_last_error(), what
        assert bool((bits(out.t) == SBITS).all()) and out.surroundings_keep(SBITS), what
    # N == 0: a no-op that needs no buffers
    assert _resize(lib, ptr, dtype, strides, 0.5, 0.5, out, 0, 3, H, W, Ho, Wo) == 0
    assert _resize(lib, None, dtype, strides, 0.5, 0.5, None, 0, 3, H, W, Ho, Wo) == 0
    assert bool((bits(out.t) == SBITS).all()) and out.surroundings_keep(SBITS)


# ------------------------------------------------------------------ moments
F_SIZES = [1, 15, 16, 17, 48, 63, 64, 65, 80, 130]
N_ROWS = [0, 1, 3, 4, 5, 37, 259]
DSENT = float(SENTINEL)                     # the same finite pattern, widened: fills the fp64 allocations


class GuardedD:
    """fp64 zeros (or `value`) of `shape` in the middle of an allocation filled with DSENT"""

    def __init__(self, shape, value=0.0, pad=512):
        n = int(np.prod(shape))
        self.flat = torch.full((pad + n + pad,), DSENT, dtype=torch.float64, device=DEV)
        self.t = self.flat[pad:pad + n].view(shape)
        self.t.fill_(value)
        self.pad, self.n = pad, n

    def intact(self):
        return bool((self.flat[:self.pad] == DSENT).all()) and bool((self.flat[self.pad + self.n:] == DSENT).all())


def _rows_dev(x, ldx):
    """x (n, F) fp32 inside a NaN-filled allocation with row stride ldx: columns past F and rows past n are NaN"""
    n, F = x.shape
    g = Guarded(torch.full((n + 40, ldx), float("nan"), dtype=torch.float32), float("nan"), before=128, after=4096)
    if n:
        g.t[:n, :F] = torch.from_numpy(x.copy()).to(DEV)
    return g


def _update(lib, g, ldx, n, F, s1, s2, row0=0):
    rc = lib.rg_moments_update(g.t.data_ptr() + 4 * row0 * ldx, ldx, n, F, s1.t.data_ptr(), s2.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert s1.intact() and s2.intact(), "rg_moments_update wrote outside s1 / s2"


def _moments(lib, x, ldx, blocks=None):
    n, F = x.shape
    g = _rows_dev(x, ldx)
    s1, s2 = GuardedD((F,)), GuardedD((F, F))
    row0 = 0
    for b in (blocks or [n]):
        _update(lib, g, ldx, b, F, s1, s2, row0)
        row0 += b
    assert row0 == n
    return s1.t.cpu().numpy(), s2.t.cpu().numpy()


_ROWS = {}


def _rows(n, F, kind):
    if (n, F, kind) not in _ROWS:
        rng = np.random.default_rng(31 * n + F + (0 if kind == "int" else 5000))
        x = rng.integers(-2047, 2048, size=(n, F)).astype(np.float32) if kind == "int" else \
            (rng.standard_normal((n, F)) * rng.uniform(0.01, 30.0, size=F) + rng.uniform(-2, 2, size=F)).astype(np.float32)
        x.setflags(write=False)
        _ROWS[(n, F, kind)] = x
    return _ROWS[(n, F, kind)]


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_moments(half, F):
    lib = _abi.load(half)
    for n in N_ROWS:
        for ldx in (F, F + 5):
            what = "%s F=%d n=%d ldx=%d" % (half, F, n, ldx)
            if n == 0:                                  # writes nothing, whatever s1 / s2 hold
                g = _rows_dev(np.zeros((0, F), dtype=np.float32), ldx)
                s1, s2 = GuardedD((F,), 1.5), GuardedD((F, F), -2.5)
                _update(lib, g, ldx, 0, F, s1, s2)
                assert bool((s1.t == 1.5).all()) and bool((s2.t == -2.5).all()), what
                continue
            # 1. integer rows: exact
            xi = _rows(n, F, "int")
            want1, want2 = moments_int(xi)
            s1, s2 = _moments(lib, xi, ldx)
            assert np.isfinite(s1).all() and np.isfinite(s2).all(), what + ": a row or column outside x was read"
            assert np.array_equal(s1, want1.astype(np.float64)), what
            bad = np.argwhere(s2 != want2.astype(np.float64))
            assert bad.size == 0, "%s: %d of %d entries of s2 differ from the integer sums, first at %s" % (
                what, len(bad), F * F, bad[0])
            # 2. three successive calls on row blocks = one call on the concatenation (integers: exactness again)
            if n >= 3:
                b = [n // 3, n // 3, n - 2 * (n // 3)]
                t1, t2 = _moments(lib, xi, ldx, blocks=b)
                assert np.array_equal(t1, s1) and np.array_equal(t2, s2), what + " in three calls"
            # 3. real-valued rows against the longdouble sums
            xr = _rows(n, F, "real")
            e1, e2, a2, a1 = moments_ld(xr)
            r1, r2 = _moments(lib, xr, ldx)
            assert np.isfinite(r1).all() and np.isfinite(r2).all(), what + ": a row or column outside x was read"
            u = np.longdouble(n) * np.longdouble(2.0 ** -53)
            assert np.all(np.abs(r2.astype(np.longdouble) - e2) <= u * a2), what
            assert np.all(np.abs(r1.astype(np.longdouble) - e1) <= u * a1), what
            # 4. bit-symmetric
            assert np.array_equal(r2.view(np.uint64), r2.T.copy().view(np.uint64)), what + ": s2 is not bit-symmetric"
            # 5. a second run from the same zeroed state: identical bits
            q1, q2 = _moments(lib, xr, ldx)
            assert np.array_equal(q1.view(np.uint64), r1.view(np.uint64)) and np.array_equal(q2.view(np.uint64), r2.view(np.uint64)), what
            # real rows in three calls: the bound holds with n_total
            if n >= 3:
                t1, t2 = _moments(lib, xr, ldx, blocks=[n // 3, n // 3, n - 2 * (n // 3)])
                assert np.all(np.abs(t2.astype(np.longdouble) - e2) <= u * a2), what
                assert np.all(np.abs(t1.astype(np.longdouble) - e1) <= u * a1), what
                assert np.array_equal(t2.view(np.uint64), t2.T.copy().view(np.uint64)), what


@pytest.mark.parametrize("half", BUILDS)
def test_moments_asymmetric_exact_map(half):
    """one-hot rows: row r has a single 1 in column c(r) times a row-specific weight, so s2 is diagonal with known entries and
    an entry written to a transposed or shifted place shows; plus a rank-one case x = [1, 2, ..., F] whose s2[i][j] = (i+1)(j+1)
    n is asymmetric in nothing but position"""
    lib = _abi.load(half)
    F, n = 130, 37
    x = np.zeros((n, F), dtype=np.float32)
    for r in range(n):
        x[r, (7 * r) % F] = r + 1
        x[r, (7 * r + 3) % F] = -(r + 2)
    w1, w2 = moments_int(x)
    s1, s2 = _moments(lib, x, F + 5)
    assert np.array_equal(s1, w1.astype(np.float64)) and np.array_equal(s2, w2.astype(np.float64))
    x = np.tile(np.arange(1, F + 1, dtype=np.float32), (n, 1))
    s1, s2 = _moments(lib, x, F)
    assert np.array_equal(s2, n * np.outer(np.arange(1, F + 1), np.arange(1, F + 1)).astype(np.float64))
    assert np.array_equal(s1, n * np.arange(1, F + 1, dtype=np.float64))


@pytest.mark.parametrize("half", BUILDS)
def test_moments_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    F, n, ldx = 17, 5, 22
    g = _rows_dev(_rows(n, F, "int"), ldx)
    s1, s2 = GuardedD((F,), 1.5), GuardedD((F, F), -2.5)
    x, p1, p2 = g.t.data_ptr(), s1.t.data_ptr(), s2.t.data_ptr()
    bad_calls = {"F = 0": (x, ldx, n, 0, p1, p2), "F < 0": (x, ldx, n, -4, p1, p2), "n < 0": (x, ldx, -1, F, p1, p2),
                 "ldx < F": (x, F - 1, n, F, p1, p2), "x = NULL": (None, ldx, n, F, p1, p2), "s1 = NULL": (x, ldx, n, F, None, p2),
                 "s2 = NULL": (x, ldx, n, F, p1, None)}
    for what, args in bad_calls.items():
        rc = lib.rg_moments_update(*args, None)
        torch.cuda.synchronize()
        assert rc == -1, what
        assert b"moments_update" in lib.rg_last_error(), what
        assert bool((s1.t == 1.5).all()) and bool((s2.t == -2.5).all()) and s1.intact() and s2.intact(), what
    assert lib.rg_moments_update(None, F, 0, F, None, None, None) == 0          # n == 0 needs no buffers
