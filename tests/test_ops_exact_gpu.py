"""Checks of the conv kernels that do not rest on a relative tolerance (both builds of the library unless stated).

C1  EXACT-INTEGER convolutions.  max|err| / max|ref| <= tol on Gaussian inputs cannot see one dropped k-term at the deep
    layers' reduction lengths (K = 16 384, 32 768): the accumulation allowance swallows it.  Exact arithmetic can.  Operands are
    integers in {-1, 0, +1} stored in the build's 16-bit type, as sparse as it takes that for every output S = sum |a||b| <= L:
        L = 2048 (fp16 results), 256 (bf16 results), 2^24 (fp32 results: weight gradients, BatchNorm partial sums),
        L / 2 where the fused LeakyReLU mask multiplies by 0.5 (one more bit).
    Then every product, every partial sum in any order, every 16-bit split-K slab value and every stored result is an exactly
    representable number, and the kernel's output must be torch.equal to the reference: fp32 matrix products of the same
    integers (im2col / col2im written out below; exact for the same reason, so they run on the device as "checker only", and a
    test without the GPU mark pins them against torch's own convolutions).  S <= L and "the case is not trivial" (at most 10 % of
    the reference outputs are zero, at least 50 distinct values) are CONDITIONS, asserted on the reference before comparing.
C2  Element-wise worst-case bound against fp64 at K <= 1024 (fp16 build): |got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25.
C3  The number range of fp16: overflow stores infinity, non-finite operands stay non-finite and local, subnormals are honoured.
"""
import pytest
import torch
import torch.nn.functional as F

from rna_gan_amd.engine import ConvW

gpu = pytest.mark.gpu
H16 = [torch.bfloat16, torch.float16]
both_builds = pytest.mark.parametrize("h16", H16, ids=["bfloat16", "float16"])
LIMIT = {torch.float16: 2048, torch.bfloat16: 256}         # integers up to here are exact in the type (11 / 8 significant bits)
U16 = 2.0 ** -11                                           # fp16's unit round-off


def _hip(h16):
    from rna_gan_amd.ops_hip import HipOps
    return HipOps(h16, "cuda:0")


# ------------------------------------------------------------------ the reference: matrix products of the operands
def _patches(x):
    """x [N, H, W, I] -> the stride-2, pad-1, 4 x 4 patches [N * H/2 * W/2, (kh, kw, i)]."""
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    p = xp.unfold(1, 4, 2).unfold(2, 4, 2)                  # [N, Ho, Wo, I, kh, kw]
    return p.permute(0, 1, 2, 4, 5, 3).reshape(-1, 16 * x.shape[-1])


def ref_down(x, w):
    """y[n, ho, wo, o] = sum x_pad[n, 2 ho + kh, 2 wo + kw, i] w[o, kh, kw, i]  (w tap-major [O, 4, 4, I])"""
    N, H, W, _ = x.shape
    return (_patches(x) @ w.reshape(w.shape[0], -1).t()).reshape(N, H // 2, W // 2, w.shape[0])


def ref_up(g, w):
    """The adjoint of ref_down in x: u[n, 2 ho + kh - 1, 2 wo + kw - 1, i] += g[n, ho, wo, o] w[o, kh, kw, i]."""
    N, Ho, Wo, O = g.shape
    I = w.shape[-1]
    cols = (g.reshape(-1, O) @ w.reshape(O, -1)).reshape(N, Ho, Wo, 4, 4, I)
    out = torch.zeros(N, 2 * Ho + 2, 2 * Wo + 2, I, dtype=g.dtype, device=g.device)
    for kh in range(4):
        for kw in range(4):
            out[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += cols[:, :, :, kh, kw]
    return out[:, 1:-1, 1:-1].contiguous()


def ref_wgrad(g, x):
    """dw[o, kh, kw, i] = sum over (n, ho, wo) of g[n, ho, wo, o] x_pad[n, 2 ho + kh, 2 wo + kw, i]"""
    O, I = g.shape[-1], x.shape[-1]
    return (g.reshape(-1, O).t() @ _patches(x)).reshape(O, 4, 4, I)


def test_reference_products_equal_torch_convolutions():
    """(no GPU) the three matrix-product references above against torch's conv2d / conv_transpose2d / conv2d_weight in fp64."""
    gen = torch.Generator().manual_seed(5)
    for N, H, W, I, O in ((2, 8, 8, 3, 5), (1, 4, 12, 6, 4), (3, 2, 2, 2, 2)):
        x = torch.randn(N, H, W, I, generator=gen, dtype=torch.float64)
        g = torch.randn(N, H // 2, W // 2, O, generator=gen, dtype=torch.float64)
        w = torch.randn(O, 4, 4, I, generator=gen, dtype=torch.float64)
        xc, gc, wc = x.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
        assert torch.allclose(ref_down(x, w), F.conv2d(xc, wc, stride=2, padding=1).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        assert torch.allclose(ref_up(g, w), F.conv_transpose2d(gc, wc, stride=2, padding=1).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        dw = torch.nn.grad.conv2d_weight(xc, (O, I, 4, 4), gc, stride=2, padding=1).permute(0, 2, 3, 1)
        assert torch.allclose(ref_wgrad(g, x), dw, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ operands
def _density(K, L):
    """Per-operand density of non-zeros so that S = sum |a||b| over K products has mean L - 6.5 sqrt(L): S is close to a binomial
    with a standard deviation below sqrt(L), so its maximum over millions of outputs stays below L (which the test asserts)."""
    return min(1.0, (L - 6.5 * L ** 0.5) / K) ** 0.5


def _ints(shape, density, seed, h16, dev="cuda:0"):
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = torch.rand(shape, device=dev, generator=gen)
    return ((r < density / 2).float() - (r > 1 - density / 2).float()).to(h16)


def _ints12(shape, seed, h16, dev="cuda:0"):
    """Dense operands in {-2, -1, +1, +2} (weight gradients: fp32 results; sums of dense +-1 alone would all share one parity)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = torch.randint(0, 4, shape, device=dev, generator=gen)
    return ((r % 2 + 1).float() * (1 - 2 * (r // 2)).float()).to(h16)


def _conditions(ref, S, L, what):
    """The bound is a condition of the test, not a measurement: asserted on the reference alone, before any comparison."""
    assert float(S.max()) <= L, "%s: S = %g > L = %g: not every partial sum is exact" % (what, float(S.max()), L)
    assert torch.equal(ref, ref.round()) or torch.equal(2 * ref, (2 * ref).round())
    zeros = float((ref == 0).float().mean())
    distinct = int(torch.unique(ref).numel())
    assert zeros <= 0.10 and distinct >= 50, "%s: trivial case (%.1f %% zeros, %d distinct values)" % (what, 100 * zeros, distinct)


def _cw(w):
    assert w.is_cuda                                         # (the library takes raw pointers: never hand it a host tensor)
    return ConvW(w.float().contiguous(), None, torch.full_like(w.float(), 7.0), None, "OHWI")


class _Options:
    """rg_set_option on the library of the build under test (the option table is per library), restored on exit."""

    def __init__(self, lib, **opts):
        self.lib, self.opts = lib, opts

    def __enter__(self):
        from rna_gan_amd import _abi
        for k, v in self.opts.items():
            _abi.check(self.lib.rg_set_option(k.encode(), v), "rg_set_option")

    def __exit__(self, *exc):
        for k in self.opts:
            self.lib.rg_set_option(k.encode(), -1)


def _down_case(N, Hi, Wi, I, O, h16, seed=1, L=None):
    d = _density(16 * I, L or LIMIT[h16])
    x, w = _ints((N, Hi, Wi, I), d, seed, h16), _ints((O, 4, 4, I), d, seed + 1, h16)
    y, S = ref_down(x.float(), w.float()), ref_down(x.float().abs(), w.float().abs())
    _conditions(y, S, L or LIMIT[h16], "conv_down")
    return x, w, y


def _up_case(N, Ho, Wo, O, I, h16, seed=11, L=None):
    """Two operand sets: S <= L for the plain transposed conv, and S <= L / 2 for the masked form (x 0.5 where the mask is not
    positive: one more bit), each with its conditions asserted on its own reference.  The mask holds +1 / -1 / +0 / -0 (zero
    counts as "not positive")."""
    L = L or LIMIT[h16]
    d = _density(4 * O, L)
    g, w = _ints((N, Ho, Wo, O), d, seed, h16), _ints((O, 4, 4, I), d, seed + 1, h16)
    u, S = ref_up(g.float(), w.float()), ref_up(g.float().abs(), w.float().abs())
    _conditions(u, S, L, "conv_up")
    d = _density(4 * O, L // 2)
    gm, wm = _ints((N, Ho, Wo, O), d, seed + 3, h16), _ints((O, 4, 4, I), d, seed + 4, h16)
    m = _ints((N, 2 * Ho, 2 * Wo, I), 0.9, seed + 2, h16)
    m[0, 0, :2, :8] = -0.0
    um = ref_up(gm.float(), wm.float()) * torch.where(m.float() > 0, 1.0, 0.5)
    _conditions(um, ref_up(gm.float().abs(), wm.float().abs()), L // 2, "conv_up (masked)")
    return g, w, u, (gm, wm, m), um


def _check_stats(st, y_ref, what):
    """Epilogue BatchNorm partial sums [rows][2][C]: sums of exact integers.  Every partial (a sum over some of the rows, in any
    order) is exact when the column's sum of |y| is below 2^24; likewise for y^2 -- checked only where the reference says so."""
    if st is None:
        print(what + ": this launch writes no epilogue partial sums -- nothing checked")
        return 0
    C = y_ref.shape[-1]
    yr = y_ref.reshape(-1, C).double()
    if float(yr.abs().sum(0).max()) >= 2 ** 24:              # (the caller repeats the launch with sparser operands)
        return -1
    assert torch.equal(st[:, 0, :].double().sum(0), yr.sum(0)), what + " epilogue sum"
    if float((yr * yr).sum(0).max()) < 2 ** 24:
        assert torch.equal(st[:, 1, :].double().sum(0), (yr * yr).sum(0)), what + " epilogue sum of squares"
        return 2
    return 1


def _exact(got, ref, what):
    assert torch.equal(got.float(), ref), "%s: %d of %d outputs differ, first at %s" % (
        what, int((got.float() != ref).sum()), ref.numel(), (got.float() != ref).nonzero()[:4].tolist())


def _run_down(hip, x, w, y_ref, what):
    y, st = hip.conv_down(x, _cw(w), want_stats=True)
    _exact(y, y_ref, what + " conv_down")
    _exact(hip.conv_down(x, _cw(w)), y_ref, what + " conv_down (no statistics)")
    return _check_stats(st, y_ref, what + " conv_down")


def _run_up(hip, g, w, u_ref, m, um_ref, what, packed=False):
    u, st = hip.conv_up(g, _cw(w), want_stats=True)
    _exact(u, u_ref, what + " conv_up")
    n = _check_stats(st, u_ref, what + " conv_up")
    gm, wm, mask = m
    _exact(hip.conv_up(gm, _cw(wm), mask.clone(), 0.5), um_ref, what + " conv_up (dense mask)")
    if packed:
        mp = mask.clone()
        mp._rg_sign_bits = hip.sign_pack(mp)
        _exact(hip.conv_up(gm, _cw(wm), mp, 0.5), um_ref, what + " conv_up (packed sign bits)")
    return n


def _run_wgrad(hip, N, Hi, Wi, I, O, h16, what, two=True):
    """fp32 results: dense operands in {+-1, +-2}, S <= 4 x the number of pixels."""
    x, g = _ints12((N, Hi, Wi, I), 21, h16), _ints12((N, Hi // 2, Wi // 2, O), 22, h16)
    dw = ref_wgrad(g.float(), x.float())
    assert 4 * 4 * N * (Hi // 2) * (Wi // 2) <= 2 ** 24                # S <= L = 2^24 also for two segments, accumulated
    assert float((dw == 0).float().mean()) <= 0.10 and int(torch.unique(dw).numel()) >= 50, what + ": trivial case"
    cw = _cw(torch.zeros(O, 4, 4, I, device=x.device))
    hip.conv_wgrad(g, x, cw, False)                                    # overwrites the 7.0 fill
    _exact(cw.dw, dw, what + " conv_wgrad")
    hip.conv_wgrad(g, x, cw, True)
    _exact(cw.dw, 2 * dw, what + " conv_wgrad (accumulate)")
    if two:
        x2, g2 = _ints12((N, Hi, Wi, I), 23, h16), _ints12((N, Hi // 2, Wi // 2, O), 24, h16)
        both = dw + ref_wgrad(g2.float(), x2.float())
        cw.dw.fill_(-5.0)
        hip.conv_wgrad2(g, x, g2, x2, cw, False)
        _exact(cw.dw, both, what + " conv_wgrad2")
        hip.conv_wgrad2(g, x, g2, x2, cw, True)
        _exact(cw.dw, 2 * both, what + " conv_wgrad2 (accumulate)")


# ------------------------------------------------------------------ C1
FULL = [(64, 128, 128), (128, 256, 64), (256, 512, 32), (512, 1024, 16), (1024, 2048, 8)]        # the LAYERS of test_fullsize_gpu.py
MFMA_SHAPES = [(2, 16, 16, 64, 128), (3, 8, 8, 128, 256), (1, 8, 8, 256, 128), (4, 32, 32, 64, 128)]     # of test_ops_gpu.CONV_CASES
CONV8_CASES = [(2, 32, 32, 64, 256), (5, 16, 16, 128, 256), (3, 32, 32, 64, 128), (3, 32, 32, 128, 256), (2, 32, 32, 256, 128)]
WGRAD8_CASES = [(2, 32, 32, 64, 256), (3, 16, 16, 128, 256), (5, 16, 16, 64, 512), (1, 32, 32, 256, 256)]


@gpu
@both_builds
@pytest.mark.parametrize("I,O,hs", FULL)
def test_exact_integer_convs_full_size(I, O, hs, h16):
    """The five layer shapes of the 256 x 256 model at batch 64, default dispatch: what the benchmark runs (256 x 256 tiles,
    split-K -- with 16-bit slabs in the bf16 build, fp32 slabs in the fp16 build --, XCD order, K up to 32 768)."""
    hip, N = _hip(h16), 64
    x, w, y = _down_case(N, hs, hs, I, O, h16)
    if _run_down(hip, x, w, y, "full size") < 0:
        # a million rows of values up to +-200: the column sums of |y| leave fp32's exact range -- the partial sums are checked
        # on operands as sparse as the bf16 build's (S <= 256), where every conceivable partial sum is exact
        x, w, y = _down_case(N, hs, hs, I, O, h16, seed=5, L=256)
        assert _run_down(hip, x, w, y, "full size, sparse") >= 0
    del x, y
    g, w2, u, m, um = _up_case(N, hs // 2, hs // 2, O, I, h16)
    packed = hip.lib.rg_conv_up_maskbits_supported(N, hs // 2, hs // 2, O, I, hip.H16, hip.algo) == 1
    if _run_up(hip, g, w2, u, m, um, "full size", packed=packed) < 0:
        g, w2, u, m, um = _up_case(N, hs // 2, hs // 2, O, I, h16, seed=15, L=256)
        assert _run_up(hip, g, w2, u, m, um, "full size, sparse", packed=packed) >= 0
    del g, u, m, um
    _run_wgrad(hip, N, hs, hs, I, O, h16, "full size")
    torch.cuda.synchronize()
    assert hip._sb_sync is None or int(hip._sb_sync[0]) == 0


@gpu
@both_builds
@pytest.mark.parametrize("N,Hi,Wi,I,O", MFMA_SHAPES)
def test_exact_integer_convs_small_mfma_shapes(N, Hi, Wi, I, O, h16):
    hip = _hip(h16)
    x, w, y = _down_case(N, Hi, Wi, I, O, h16)
    _run_down(hip, x, w, y, "default")
    g, w2, u, m, um = _up_case(N, Hi // 2, Wi // 2, O, I, h16)
    _run_up(hip, g, w2, u, m, um, "default")
    _run_wgrad(hip, N, Hi, Wi, I, O, h16, "default")


@gpu
@both_builds
@pytest.mark.parametrize("N,Hi,Wi,I,O", CONV8_CASES)
def test_exact_integer_conv8_variants(N, Hi, Wi, I, O, h16):
    """conv8 in {1, 5, 7} x conv8_mfma in {16, 32} (both tiles, both MFMA shapes, split-K forced, parity classes fastest): all six
    variants bit-identical to the reference, hence to each other."""
    hip = _hip(h16)
    x, w, y = _down_case(N, Hi, Wi, I, O, h16)
    g, w2, u, m, um = _up_case(N, Hi // 2, Wi // 2, O, I, h16)
    for mode in (1, 5, 7):
        for mfma in (16, 32):
            with _Options(hip.lib, conv8=mode, conv8_mfma=mfma, conv8_blocks=8, narrow8=1):
                what = "conv8 = %d, conv8_mfma = %d:" % (mode, mfma)
                _run_down(hip, x, w, y, what)
                _run_up(hip, g, w2, u, m, um, what)


@gpu
@both_builds
@pytest.mark.parametrize("blocks", [256, 3])
@pytest.mark.parametrize("N,Hs", [(1, 128), (3, 128), (2, 32), (5, 8)])
def test_exact_integer_convd(N, Hs, blocks, h16):
    """The plane-resident 64 -> 128 stride-2 conv (convd = 1) and the implicit-GEMM kernel it replaces (convd = 0)."""
    hip = _hip(h16)
    x, w, y = _down_case(N, Hs, 128, 64, 128, h16)
    for on in (1, 0):
        with _Options(hip.lib, conv8_blocks=1, convd_blocks=blocks, convd=on):
            n_stats = _run_down(hip, x, w, y, "convd = %d:" % on)
            assert n_stats >= 1 or not on, "the plane-resident kernel writes the BatchNorm partial sums"


@gpu
@both_builds
@pytest.mark.parametrize("blocks", [256, 3])
@pytest.mark.parametrize("N,Ws", [(1, 16), (3, 16), (2, 32), (1, 64), (5, 64)])
def test_exact_integer_convp(N, Ws, blocks, h16):
    """The patch-resident 128 -> 64 transposed conv (convp = 1) and the implicit-GEMM kernel (convp = 0): plain, BatchNorm
    partial sums, dense mask and packed sign bits."""
    hip = _hip(h16)
    assert hip.lib.rg_conv_up_maskbits_supported(N, Ws, Ws, 128, 64, hip.H16, 0) == 1
    g, w, u, m, um = _up_case(N, Ws, Ws, 128, 64, h16)
    for on in (1, 0):
        with _Options(hip.lib, convp_blocks=blocks, convp=on):
            n_stats = _run_up(hip, g, w, u, m, um, "convp = %d:" % on, packed=True)
            assert n_stats >= 1 or not on, "the patch-resident kernel writes the BatchNorm partial sums"


@gpu
@both_builds
@pytest.mark.parametrize("blocks", [1, 8, 256])
@pytest.mark.parametrize("N,Hi,Wi,I,O", WGRAD8_CASES)
def test_exact_integer_wgrad8(N, Hi, Wi, I, O, blocks, h16):
    """The 8-wave weight-gradient kernel: direct write (one split) and split-K slabs, one and two segments."""
    hip = _hip(h16)
    with _Options(hip.lib, wgrad8=1, wgrad8_blocks=blocks):
        _run_wgrad(hip, N, Hi, Wi, I, O, h16, "wgrad8_blocks = %d:" % blocks, two=(N * Hi * Wi // 4) % 64 == 0)


@gpu
@both_builds
@pytest.mark.parametrize("wslab16", [0, 1])
@pytest.mark.parametrize("I,O,hs", [(256, 512, 16), (64, 128, 64)])
def test_exact_integer_deferred_weight_gradient_slabs(I, O, hs, wslab16, h16):
    """rg_conv_wgrad_slabs + rg_grad_to_wire: the split-K slabs left unreduced, as fp32 (wslab16 = 0) and in the build's 16-bit
    type (wslab16 = 1), summed and rounded by the wire kernel.  The operands are sparse enough that S <= L of the 16-bit type:
    every slab value and the rounded sum are exact."""
    import ctypes as C
    from rna_gan_amd import _abi
    hip, N = _hip(h16), 64
    lib = hip.lib
    L = LIMIT[h16]
    d = _density(N * hs * hs, L)
    low, high = _ints((N, hs, hs, O), d, 31, h16), _ints((N, 2 * hs, 2 * hs, I), d, 32, h16)
    dw = ref_wgrad(low.float(), high.float())
    S = ref_wgrad(low.float().abs(), high.float().abs())
    _conditions(dw, S, L, "conv_wgrad_slabs")
    nw = O * 16 * I
    wsb = int(lib.rg_conv_wgrad_workspace_bytes(N, hs, hs, O, I, hip.dt, hip.algo))
    slab = torch.empty(max(wsb, 256) + 4096, dtype=torch.uint8, device="cuda:0")
    gbuf = torch.full((nw,), float("nan"), device="cuda:0")
    ns, sdt = C.c_int(0), C.c_int(-1)
    with _Options(lib, wslab16=wslab16):
        _abi.check(lib.rg_conv_wgrad_slabs(low.data_ptr(), high.data_ptr(), 0, 0, gbuf.data_ptr(), N, hs, hs, O, I, hip.dt, hip.algo,
                                           slab.data_ptr(), slab.numel(), C.addressof(ns), C.addressof(sdt), hip.stream), "slabs")
    assert ns.value > 1, "this shape is expected to run split-K"
    assert sdt.value in (hip.H16, _abi.RG_F32) and (sdt.value == _abi.RG_F32 or wslab16 == 1)
    offs, lens = (C.c_ulonglong * 1)(0), (C.c_ulonglong * 1)(nw)
    sl, nsp, sdts = (C.c_void_p * 1)(slab.data_ptr()), (C.c_int * 1)(ns.value), (C.c_int * 1)(sdt.value)
    wire = torch.full((nw,), 7.0, dtype=h16, device="cuda:0")
    _abi.check(lib.rg_grad_to_wire(gbuf.data_ptr(), wire.data_ptr(), nw, 1, C.addressof(offs), C.addressof(lens), C.addressof(sl),
                                   C.addressof(nsp), C.addressof(sdts), hip.stream), "rg_grad_to_wire")
    torch.cuda.synchronize()
    _exact(wire.view(O, 4, 4, I), dw, "wire from %d slabs (dtype code %d)" % (ns.value, sdt.value))


# ------------------------------------------------------------------ C2: worst-case bound against fp64 at K <= 1024
def _gauss(shape, seed, scale=1.0, dev="cuda:0"):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, device=dev, generator=gen) * scale


def _bound_check(got, ref, S, K, u, what, report=None):
    """|got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25: products of two fp16 numbers are exact in fp32, K fp32 additions in any
    order, one rounding to the stored type (u = 0: an fp32 result).  Nothing in it is measured."""
    assert K <= 1025, "the bound is vacuous above K = 1024 (+ 1 where an epilogue factor adds a rounding)"
    got, ref, S = got.double(), ref.double(), S.double()
    assert torch.isfinite(got).all(), what + ": non-finite output"
    bound = u * ref.abs() + K * 2.0 ** -24 * (1 + u) * S + 2.0 ** -25
    ratio = float(((got - ref).abs() / bound).max())
    print("%s: worst |err| / bound = %.3f" % (what, ratio))
    if report is not None:
        report.append(ratio)
    bad = (got - ref).abs() > bound
    assert not bool(bad.any()), "%s: %d of %d outputs outside the worst-case bound (worst ratio %.2f), first at %s" % (
        what, int(bad.sum()), bad.numel(), ratio, bad.nonzero()[:4].tolist())


@gpu
@pytest.mark.parametrize("N,Hi,Wi,I,O", MFMA_SHAPES)
def test_fp16_convs_within_the_worst_case_bound_of_fp64(N, Hi, Wi, I, O):
    h16 = torch.float16
    hip = _hip(h16)
    w = _gauss((O, 4, 4, I), 1, (2.0 / (I * 16)) ** 0.5)
    wq = w.to(h16).double()                                  # the kernels compute with the weights rounded to the storage type
    x, g = _gauss((N, Hi, Wi, I), 2).to(h16), _gauss((N, Hi // 2, Wi // 2, O), 3).to(h16)
    xd, gd = x.double(), g.double()
    did = 0
    if 16 * I <= 1024:
        _bound_check(hip.conv_down(x, _cw(w)), ref_down(xd, wq), ref_down(xd.abs(), wq.abs()), 16 * I, U16, "conv_down")
        did += 1
    if 4 * O <= 1024:
        u_ref, S = ref_up(gd, wq), ref_up(gd.abs(), wq.abs())
        _bound_check(hip.conv_up(g, _cw(w)), u_ref, S, 4 * O, U16, "conv_up")
        m = _gauss((N, Hi, Wi, I), 21).to(h16)
        # (the factor multiplies the fp32 sum: K - 1 additions, one multiplication and the fp32 image of 0.2 -- K + 1 roundings)
        f = torch.where(m.double() > 0, 1.0, 0.2)
        _bound_check(hip.conv_up(g, _cw(w), m, 0.2), u_ref * f, S * f, 4 * O + 1, U16, "conv_up (masked)")
        did += 1
    K = N * (Hi // 2) * (Wi // 2)
    if K <= 1024:
        cw = _cw(w)
        hip.conv_wgrad(g, x, cw, False)
        _bound_check(cw.dw, ref_wgrad(gd, xd), ref_wgrad(gd.abs(), xd.abs()), K, 0.0, "conv_wgrad")
        did += 1
    assert did >= 1


@gpu
@pytest.mark.parametrize("O,W", [(4, 32), (64, 32), (128, 32), (64, 128), (64, 64)])
def test_fp16_image_side_layers_within_the_worst_case_bound_of_fp64(O, W):
    """first_down (K = 48), last_up (K = 4 O <= 512) and the image-side weight gradient (K = the pixels, where <= 1024)."""
    h16 = torch.float16
    hip = _hip(h16)
    N, H, I = 3, 16, 3
    w = _gauss((O, I, 4, 4), 4, 0.2)
    wq = w.to(h16).double().permute(0, 2, 3, 1).contiguous()            # [O, 4, 4, I]
    x = _gauss((N, I, H, W), 6)
    xq = x.to(h16).double().permute(0, 2, 3, 1).contiguous()            # the image is rounded to the storage type too
    cw = ConvW(w, None)
    xf, wf = x.double().permute(0, 2, 3, 1).contiguous(), w.double().permute(0, 2, 3, 1).contiguous()

    def either(vector, got, ref_q, S_q, ref_f, S_f, K, u, what):
        """The matrix-core row kernels round the fp32 image and the weights to the storage type (exact products, K roundings);
        the vector kernels of the shapes those do not take use them as they are (every product rounded too: 2 K roundings).
        Which one a shape takes is fixed by the dispatch (rg_api.hip) and stated per case here: `vector`."""
        if vector:
            _bound_check(got, ref_f, S_f, 2 * K, u, what + " (vector kernel: fp32 operands as they are)")
        else:
            _bound_check(got, ref_q, S_q, K, u, what + " (row kernel: operands rounded to fp16)")
    generic = O % 64 != 0                                    # rg_skinny_supported: 3 image channels, 64 or 128 on the other side
    either(generic, hip.first_down(x, cw, None, 1.0), ref_down(xq, wq), ref_down(xq.abs(), wq.abs()), ref_down(xf, wf),
           ref_down(xf.abs(), wf.abs()), 16 * I, U16, "first_down")
    a = _gauss((N, H // 2, W // 2, O), 7).to(h16)
    ad = a.double()
    y = hip.last_up(a, cw, None, False)                                 # NCHW fp32
    either(generic, y.permute(0, 2, 3, 1), ref_up(ad, wq), ref_up(ad.abs(), wq.abs()), ref_up(ad, wf), ref_up(ad.abs(), wf.abs()), 4 * O, 0.0,
           "last_up")
    K = N * (H // 2) * (W // 2)
    vec_w = not (O == 64 and W // 2 in (32, 64))             # (rg_skinny_wgrad_impl: the row kernel takes 64 channels, rows of 32 / 64 / 128 k)
    if (2 * K if vec_w else K) <= 1024:
        dw = torch.full((O, I, 4, 4), 3.0, device="cuda:0")
        hip.skinny_wgrad(a, x, dw, False)
        either(vec_w, dw.permute(0, 2, 3, 1), ref_wgrad(ad, xq), ref_wgrad(ad.abs(), xq.abs()), ref_wgrad(ad, xf), ref_wgrad(ad.abs(), xf.abs()),
               K, 0.0, "skinny_wgrad")


# ------------------------------------------------------------------ C3: the number range of fp16
F16 = torch.float16


def _overflow_expect(exact64):
    """What one rounding of the exact value to fp16 stores: +-inf from 65 520 up (never 65 504, never NaN)."""
    want = exact64.to(F16)
    assert bool(torch.isinf(want).any()) and not bool(torch.isnan(want).any())
    return want


def _same_with_inf(got, want, what):
    assert got.dtype == F16 and not bool(torch.isnan(got).any()), what + ": NaN"
    assert torch.equal(torch.isinf(got), torch.isinf(want)), "%s: isinf differs at %d outputs (saturated or spurious)" % (
        what, int((torch.isinf(got) != torch.isinf(want)).sum()))
    assert torch.equal(got, want), what + ": a finite output is not the exact value"


@gpu
@pytest.mark.parametrize("kernel,N,Hi,Wi,I,O,opts", [
    ("implicit GEMM", 4, 16, 16, 64, 128, {}),
    ("conv8", 2, 32, 32, 64, 256, {"conv8": 5, "conv8_blocks": 8}),
    ("convd", 3, 128, 128, 64, 128, {"conv8_blocks": 1, "convd": 1}),
])
def test_fp16_conv_down_overflow_stores_infinity(kernel, N, Hi, Wi, I, O, opts):
    """Dense +-1 operands at K = 1024, ONE sample scaled by 2^10: its outputs are 1024 x an integer sum -- infinity from |sum| = 64
    (65 536), the exact finite value up to 63 (64 512); every other sample bit-exact.  Not saturated to 65 504, not NaN: the loss
    scaler's skip decision rests on this."""
    hip = _hip(F16)
    assert 16 * I == 1024
    x, w = _ints((N, Hi, Wi, I), 1.0, 41, F16), _ints((O, 4, 4, I), 1.0, 42, F16)
    x[1] *= 1024
    want = _overflow_expect(ref_down(x.double(), w.double()))
    assert bool(torch.isinf(want[1]).any()) and not bool(torch.isinf(want[0]).any()) and not bool(torch.isinf(want[2:]).any())
    with _Options(hip.lib, **opts):
        _same_with_inf(hip.conv_down(x, _cw(w)), want, kernel)
        y, st = hip.conv_down(x, _cw(w), want_stats=True)
        _same_with_inf(y, want, kernel + " (with statistics)")


@gpu
@pytest.mark.parametrize("kernel,N,Ho,Wo,O,I,opts", [
    ("conv8", 3, 16, 16, 256, 128, {"conv8": 5, "conv8_blocks": 8}),
    ("convp", 3, 16, 16, 128, 64, {"convp": 1}),
    ("implicit GEMM", 3, 16, 16, 128, 64, {"convp": 0}),
])
def test_fp16_conv_up_overflow_stores_infinity(kernel, N, Ho, Wo, O, I, opts):
    hip = _hip(F16)
    g, w = _ints((N, Ho, Wo, O), 1.0, 43, F16), _ints((O, 4, 4, I), 1.0, 44, F16)
    g[1] *= 1024
    u = ref_up(g.double(), w.double())
    m = _ints((N, 2 * Ho, 2 * Wo, I), 0.9, 45, F16)
    want, want_m = _overflow_expect(u), _overflow_expect(u * torch.where(m.double() > 0, 1.0, 0.5))
    assert not bool(torch.isinf(want[0]).any()) and not bool(torch.isinf(want[2]).any())
    with _Options(hip.lib, **opts):
        _same_with_inf(hip.conv_up(g, _cw(w)), want, kernel)
        _same_with_inf(hip.conv_up(g, _cw(w), m.clone(), 0.5), want_m, kernel + " (masked)")
        if I == 64:
            mp = m.clone()
            mp._rg_sign_bits = hip.sign_pack(mp)
            _same_with_inf(hip.conv_up(g, _cw(w), mp, 0.5), want_m, kernel + " (packed sign bits)")


@gpu
def test_fp16_g0_overflow_stores_infinity():
    hip = _hip(F16)
    N, E, C = 8, 1024, 64
    z, w = _ints((N, E), 1.0, 46, F16).float(), _ints((E, C, 4, 4), 1.0, 47, F16).float()
    z[3] *= 1024
    want = _overflow_expect(torch.einsum("ne,ecij->nijc", z.double(), w.double()))
    assert int(torch.isinf(want).reshape(N, -1).any(1).sum()) == 1
    _same_with_inf(hip.g0_fwd(z, ConvW(w, None)), want, "g0_fwd")


def _away_from_zero(shape, seed, floor):
    """sign * (floor + |Gaussian|): symmetric about zero, no element closer to it than `floor`."""
    g = _gauss(shape, seed)
    return (torch.where(g >= 0, 1.0, -1.0) * (floor + g.abs())).to(F16)


def _inf_subset(got, ref64, what, sign_from=0.0):
    """Point-wise kernels: the reference puts a known subset above 2^17 and everything else below 2^15 (asserted: nothing lies
    between); infinity exactly on that subset, with the reference's sign (judged from |ref| >= sign_from up: where a hot value
    is the fp32 difference of nearly equal terms, its sign is not defined by the reference)."""
    big = ref64.abs() > 2.0 ** 17
    assert bool(big.any()) and bool((~big).any()) and not bool(((ref64.abs() >= 2.0 ** 15) & ~big).any())
    assert not bool(torch.isnan(got).any()), what + ": NaN"
    assert torch.equal(torch.isinf(got), big), "%s: isinf differs from the reference's subset at %d outputs" % (
        what, int((torch.isinf(got) != big).sum()))
    sgn = big & (ref64.abs() >= sign_from)
    assert torch.equal(torch.sign(got.double())[sgn], torch.sign(ref64)[sgn]), what + ": sign of an infinity"


@gpu
def test_fp16_pointwise_kernels_overflow_to_infinity():
    """bn_act / bn_forward, bn_act_bwd, lrelu_bwd, head_bwd_data, first_down: outputs whose fp64 value is above 2^17 are stored
    as infinity, the others stay finite.  Channels (or samples) are made "hot" through an fp32 parameter, so the 16-bit inputs
    themselves are ordinary numbers."""
    hip = _hip(F16)
    M, C = 4096, 128
    z = (_gauss((1, M, 1, C), 51) * 1.5 + 0.3).to(F16)
    zd = z.double()
    mean, var = zd.reshape(M, C).mean(0), zd.reshape(M, C).var(0, unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    hot = torch.arange(C, device="cuda:0") % 8 == 3
    # |xh| >= 2^-4 on the hot channels (the few elements closer to the mean are moved away), so |y| >= 2^26 * 2^-4 * 0.2 > 2^17
    xh = (zd - mean) * invstd
    near = (xh.abs() < 0.25) & hot
    z = torch.where(near, (mean + 0.5 / invstd).to(F16).expand_as(z), z)
    zd = z.double()
    xh = (zd - mean) * invstd
    gamma = torch.where(hot, 2.0 ** 26, 1.0).float()
    beta = torch.zeros(C, device="cuda:0")
    y = xh * gamma.double()
    ref_a = torch.where(y > 0, y, 0.2 * y)
    _inf_subset(hip.bn_act(z, mean.float(), invstd.float(), gamma, beta, 0.2), ref_a, "bn_act")
    # lrelu_bwd: g * (a > 0 ? 1 : slope) with a slope above 1 that lifts the masked half over the range
    gq = (_gauss((1, M, 1, C), 52).abs() + 1.0).to(F16) * 256            # 256 .. ~1500
    a = _gauss((1, M, 1, C), 53).to(F16)
    ref_l = gq.double() * torch.where(a.double() > 0, 1.0, 1024.0)
    _inf_subset(hip.lrelu_bwd(gq, a, 1024.0), ref_l, "lrelu_bwd")
    # bn_act_bwd: gz = gamma invstd (gy - mean(gy) - xh mean(gy xh)); hot channels through gamma
    z2, ga = _away_from_zero((1, M, 1, C), 54, 1.0), _away_from_zero((1, M, 1, C), 55, 4.0)
    z2d, gad = z2.double().reshape(M, C), ga.double().reshape(M, C)
    mean2, inv2 = z2d.mean(0), torch.rsqrt(z2d.var(0, unbiased=False) + 1e-5)
    gam2 = torch.where(hot, 2.0 ** 26, 1.0).float()
    xh2 = (z2d - mean2) * inv2
    # |ga| >= 4 and slope 0.5: |gy| >= 2, far above the two mean terms (a few tenths), so no gz of a hot channel is near zero
    gy = gad * torch.where(xh2 * gam2.double() > 0, 1.0, 0.5)
    ref_gz = gam2.double() * inv2 * (gy - gy.mean(0) - xh2 * (gy * xh2).mean(0))
    gz, _, _ = hip.bn_act_bwd(z2, ga, mean2.float(), inv2.float(), gam2, torch.zeros(C, device="cuda:0"), 0.5)
    _inf_subset(gz.reshape(M, C), ref_gz, "bn_act_bwd")
    # head_bwd_data: ga[n, tap, c] = gh[n] w[c, tap]; one hot sample through the fp32 gh
    Cn = 256
    wh = (torch.sign(_gauss((1, Cn, 4, 4), 56)) * (1.0 + _gauss((1, Cn, 4, 4), 57).abs())).float()
    gh = torch.ones(16, device="cuda:0")
    gh[5] = 2.0 ** 18
    ref_h = torch.einsum("n,cij->nijc", gh.double(), wh.to(F16).double()[0])
    _inf_subset(hip.head_bwd_data(gh, ConvW(wh, None)), ref_h, "head_bwd_data")
    # first_down: one sample of the fp32 image is large (rounded to fp16 operands: +-4096, exact), bias-free, slope 1
    img = torch.sign(_gauss((4, 3, 64, 64), 58))
    img[2] *= 4096
    w0 = torch.sign(_gauss((64, 3, 4, 4), 59)) * 64.0
    ref_f = ref_down(img.double().permute(0, 2, 3, 1).contiguous(), w0.double().permute(0, 2, 3, 1).contiguous())
    # every output is 64 x an integer sum (below 2^12), x 4096 on the hot sample: 0 or at least 2^18 -- the band is empty
    _inf_subset(hip.first_down(img, ConvW(w0, None), None, 1.0), ref_f, "first_down")


def _plant(t, idx, value):
    t = t.clone()
    t[idx] = value
    return t


def _nonfinite_like(got, ref64, what):
    bad_ref = ~torch.isfinite(ref64)
    bad = ~torch.isfinite(got)
    assert bool(bad_ref.any()) and bool((~bad_ref).any()), what + ": the case plants nothing / everything"
    assert torch.equal(bad, bad_ref), "%s: %d outputs non-finite, the reference has %d (%d differ)" % (
        what, int(bad.sum()), int(bad_ref.sum()), int((bad != bad_ref).sum()))


@gpu
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_fp16_non_finite_operands_stay_non_finite_and_local(value):
    """The fp16 counterpart of test_f32_mode_non_finite_operands_stay_non_finite_and_local: ONE non-finite element in the input
    of a backward-chain op.  Every output the fp64 reference makes non-finite is non-finite, everything it keeps finite stays
    finite (for BatchNorm backward: the other channels).  Weights are strictly non-zero (no 0 x inf)."""
    hip = _hip(F16)
    N, Hi, I, O = 4, 32, 64, 128
    w = torch.sign(_gauss((O, 4, 4, I), 61)) * (0.01 + _gauss((O, 4, 4, I), 62).abs() * 0.03)
    wq = w.to(F16).double()
    g = _plant(_gauss((N, Hi // 2, Hi // 2, O), 63).to(F16), (1, 3, 5, 17), value)
    x = _gauss((N, Hi, Hi, I), 64).to(F16)
    m = torch.sign(_gauss((N, Hi, Hi, I), 65)).to(F16)
    u_ref = ref_up(g.double(), wq)
    _nonfinite_like(hip.conv_up(g, _cw(w)), u_ref, "conv_up")
    _nonfinite_like(hip.conv_up(g, _cw(w), m, 0.2), u_ref * torch.where(m.double() > 0, 1.0, 0.2), "conv_up (masked)")
    for kernel, opts in (("convp", {"convp": 1}), ("conv8", {"conv8": 5, "conv8_blocks": 8})):
        with _Options(hip.lib, **opts):
            _nonfinite_like(hip.conv_up(g, _cw(w)), u_ref, "conv_up, " + kernel)
    # weight gradients: the planted element of `low` reaches one output channel's 16 x I weights
    xnz = torch.where(x == 0, torch.ones_like(x), x)
    cw = _cw(w)
    hip.conv_wgrad(g, xnz, cw, False)
    _nonfinite_like(cw.dw, ref_wgrad(g.double(), xnz.double()), "conv_wgrad")
    g2 = _gauss((N, Hi // 2, Hi // 2, O), 66).to(F16)
    hip.conv_wgrad2(g2, xnz, g, xnz, cw, False)
    _nonfinite_like(cw.dw, ref_wgrad(g.double(), xnz.double()) + ref_wgrad(g2.double(), xnz.double()), "conv_wgrad2")
    with _Options(hip.lib, wgrad8=1, wgrad8_blocks=8):
        hip.conv_wgrad(g, xnz, cw, False)
        _nonfinite_like(cw.dw, ref_wgrad(g.double(), xnz.double()), "conv_wgrad, wgrad8 with slabs")
    # lrelu_bwd
    a = _gauss((N, Hi // 2, Hi // 2, O), 67).to(F16)
    _nonfinite_like(hip.lrelu_bwd(g, a, 0.2), g.double() * torch.where(a.double() > 0, 1.0, 0.2), "lrelu_bwd")
    # BatchNorm backward: the planted element's channel becomes non-finite (its sums are), every other channel stays finite
    M, C = N * (Hi // 2) ** 2, O
    z = (_gauss((N, Hi // 2, Hi // 2, O), 68) * 1.5 + 0.3).to(F16)
    zd = z.double().reshape(M, C)
    mean, inv = zd.mean(0), torch.rsqrt(zd.var(0, unbiased=False) + 1e-5)
    gam, bet = (1 + 0.1 * _gauss((C,), 69)), 0.1 * _gauss((C,), 70)
    xh = (zd - mean) * inv
    gy = g.double().reshape(M, C) * torch.where(xh * gam.double() + bet.double() > 0, 1.0, 0.2)
    ref_gz = gam.double() * inv * (gy - gy.mean(0) - xh * (gy * xh).mean(0))
    dg, db = torch.zeros(C, device="cuda:0"), torch.zeros(C, device="cuda:0")
    gz, s1, s2 = hip.bn_act_bwd(z, g, mean.float(), inv.float(), gam, bet, 0.2, dg, db, False)
    _nonfinite_like(gz.reshape(M, C), ref_gz, "bn_act_bwd.gz")
    _nonfinite_like(dg, (gy * xh).sum(0), "bn_act_bwd.dgamma")
    _nonfinite_like(db, gy.sum(0), "bn_act_bwd.dbeta")
    # two batch groups: the planted element sits in the first group; the second group's rows of that channel stay finite
    z4 = torch.cat([z, z.flip(0)]).contiguous()
    g4 = torch.cat([g, g2]).contiguous()
    _, mean4, inv4 = hip.bn_forward2(z4.clone(), gam, bet, 0.2, 1e-5, 0.1)
    gz4 = hip.bn_act_bwd2(z4, g4, mean4, inv4, gam, bet, 0.2, dg, db, False)
    bad4 = ~torch.isfinite(gz4)
    assert bool(bad4[:N, :, :, 17].all()) and int(bad4.sum()) == M, "bn_act_bwd2: non-finite outside the planted group / channel"
    # head: gh[n] fp32, planted in one sample
    Cn = 256
    wh = torch.sign(_gauss((1, Cn, 4, 4), 71)) * (0.05 + _gauss((1, Cn, 4, 4), 72).abs() * 0.1)
    gh = _plant(_gauss((8,), 73), (2,), value)
    _nonfinite_like(hip.head_bwd_data(gh, ConvW(wh, None)), torch.einsum("n,cij->nijc", gh.double(), wh.to(F16).double()[0]),
                    "head_bwd_data")
    act = _gauss((8, 4, 4, Cn), 74).to(F16)
    act = _plant(torch.where(act == 0, torch.ones_like(act), act), (6, 1, 2, 33), value)
    dwh = torch.zeros(1, Cn, 4, 4, device="cuda:0")
    gh_ok = _gauss((8,), 75) + 3.0
    hip.head_wgrad(gh_ok, act, dwh, False)
    _nonfinite_like(dwh, torch.einsum("n,nijc->cij", gh_ok.double(), act.double()).unsqueeze(0), "head_wgrad")
    # generator layer 0's weight gradient: dw[e, c, tap] = sum_n z[n, e] gy[n, tap, c]
    E, C0 = 128, 64
    zl = _gauss((8, E), 76)
    zl = torch.where(zl == 0, torch.ones_like(zl), zl)
    gy0 = _plant(_gauss((8, 4, 4, C0), 77).to(F16), (4, 2, 1, 9), value)
    dw0 = torch.zeros(E, C0, 4, 4, device="cuda:0")
    hip.g0_wgrad(zl, gy0, dw0, False)
    _nonfinite_like(dw0, torch.einsum("ne,nijc->ecij", zl.to(F16).double(), gy0.double()), "g0_wgrad")


@gpu
def test_fp16_subnormals_are_honoured():
    """Gradual underflow, as DESIGN 6.2 assumes (a gradient of 2^-24 survives): (a) the activations are all fp16 SUBNORMALS with
    normal weights, (b) the operands are scaled so that the reference outputs fall into the subnormal range [2^-24, 2^-14] --
    both against fp64 under the worst-case bound of C2, whose absolute term 2^-25 is half a subnormal step.  A kernel (or a
    matrix instruction) that flushed subnormal operands or results to zero would miss it by the whole value."""
    hip = _hip(F16)
    N, Hi, I, O = 2, 16, 64, 128
    w = _gauss((O, 4, 4, I), 81, (2.0 / (I * 16)) ** 0.5)
    wq = w.to(F16).double()
    sub = 2.0 ** -17                                                 # Gaussian x 2^-17: |x| < 2^-14 (8 sigma), i.e. all subnormal
    x = (_gauss((N, Hi, Hi, I), 82) * sub).to(F16)
    g = (_gauss((N, Hi // 2, Hi // 2, O), 83) * sub).to(F16)
    assert float(x.abs().max()) < 2.0 ** -14 and float(g.abs().max()) < 2.0 ** -14 and float((x != 0).float().mean()) > 0.9
    xd, gd = x.double(), g.double()
    # (a) subnormal activations, normal weights; the results are subnormal as well
    y_ref = ref_down(xd, wq)
    assert float(y_ref.abs().max()) < 2.0 ** -14 and float((y_ref.abs() >= 2.0 ** -24).float().mean()) > 0.9
    _bound_check(hip.conv_down(x, _cw(w)), y_ref, ref_down(xd.abs(), wq.abs()), 16 * I, U16, "conv_down, subnormal activations")
    u_ref = ref_up(gd, wq)
    _bound_check(hip.conv_up(g, _cw(w)), u_ref, ref_up(gd.abs(), wq.abs()), 4 * O, U16, "conv_up, subnormal activations")
    # weight gradient: subnormal `low` against normal `high` (fp32 result: products of 2^-17-sized and unit-sized numbers)
    xn = _gauss((N, Hi, Hi, I), 84).to(F16)
    cw = _cw(w)
    hip.conv_wgrad(g, xn, cw, False)
    K = N * (Hi // 2) ** 2
    dw_ref = ref_wgrad(gd, xn.double())
    assert float((dw_ref.abs() > 2.0 ** -20).float().mean()) > 0.5
    got, S = cw.dw.double(), ref_wgrad(gd.abs(), xn.double().abs())
    bad = (got - dw_ref).abs() > K * 2.0 ** -24 * S + 2.0 ** -60      # (fp32 result, far from fp32's own underflow: no absolute term)
    assert not bool(bad.any()), "conv_wgrad, subnormal low: %d outputs outside the bound" % int(bad.sum())
    # (b) normal operands scaled down so that the OUTPUTS are subnormal: x * 2^-9, w as it is (sigma_y ~ 1.4 * 2^-9 * ... )
    xs = (_gauss((N, Hi, Hi, I), 85) * 2.0 ** -8).to(F16)
    ws = w * 2.0 ** -10
    wsq = ws.to(F16).double()
    y2 = ref_down(xs.double(), wsq)
    inside = float(((y2.abs() >= 2.0 ** -24) & (y2.abs() <= 2.0 ** -14)).float().mean())
    assert inside > 0.9, inside
    _bound_check(hip.conv_down(xs, _cw(ws)), y2, ref_down(xs.double().abs(), wsq.abs()), 16 * I, U16, "conv_down, subnormal results")
    gs = (_gauss((N, Hi // 2, Hi // 2, O), 86) * 2.0 ** -8).to(F16)
    u2 = ref_up(gs.double(), wsq)
    assert float(((u2.abs() >= 2.0 ** -24) & (u2.abs() <= 2.0 ** -14)).float().mean()) > 0.9
    _bound_check(hip.conv_up(gs, _cw(ws)), u2, ref_up(gs.double().abs(), wsq.abs()), 4 * O, U16, "conv_up, subnormal results")
    # lrelu_bwd on subnormal gradients: g (exact) and 0.25 g (one rounding of a subnormal)
    a = _gauss((N, Hi // 2, Hi // 2, O), 87).to(F16)
    l_ref = gd * torch.where(a.double() > 0, 1.0, 0.25)
    got = hip.lrelu_bwd(g, a, 0.25).double()
    assert float((got - l_ref).abs().max()) <= 2.0 ** -25, "lrelu_bwd: a subnormal gradient moved by more than half a subnormal step"
    assert float((got != 0).float().mean()) > 0.85
    # bn_act_bwd with subnormal incoming gradients: gz = gamma invstd (gy - mean(gy) - xh mean(gy xh)), gz subnormal as well
    M, C = N * (Hi // 2) ** 2, O
    z = (_gauss((N, Hi // 2, Hi // 2, O), 88) * 1.5 + 0.3).to(F16)
    zd = z.double().reshape(M, C)
    mean, inv = zd.mean(0), torch.rsqrt(zd.var(0, unbiased=False) + 1e-5)
    gam, bet = (1 + 0.1 * _gauss((C,), 89)), 0.1 * _gauss((C,), 90)
    xh = (zd - mean) * inv
    mask = torch.where(xh * gam.double() + bet.double() > 0, 1.0, 0.2)
    away = (xh * gam.double() + bet.double()).abs() > 1e-3            # (elements at the LeakyReLU kink are not judged)
    gy = gd.reshape(M, C) * mask
    ref_gz = gam.double() * inv * (gy - gy.mean(0) - xh * (gy * xh).mean(0))
    gz, _, _ = hip.bn_act_bwd(z, g, mean.float(), inv.float(), gam, bet, 0.2)
    err = (gz.double().reshape(M, C) - ref_gz).abs()
    # fp32 arithmetic on numbers of size 2^-17 (M-term means in any order and a handful of operations: (M + 8) 2^-24 of the
    # terms' magnitudes), one rounding to a subnormal (2^-25)
    bound = 2.0 ** -25 + (M + 8) * 2.0 ** -24 * (gy.abs() + gy.abs().mean(0) + xh.abs() * (gy * xh).abs().mean(0)) * (gam.double().abs() * inv)
    assert not bool(((err > bound) & away).any()), "bn_act_bwd: %d subnormal gradients outside the bound" % int(((err > bound) & away).sum())
    assert float((gz != 0).float().mean()) > 0.85


# ------------------------------------------------------------------ C3, continued: the rest of the BatchNorm family and the slab consumers
@gpu
def test_fp16_batchnorm_family_overflows_to_infinity():
    """bn_forward (statistics by the pass itself), bn_tangent and bn_double_bwd: hot channels through the fp32 gamma.  z, zt and the
    cotangent are sign * (floor + |Gaussian|), so no element of a hot channel comes out near zero and the reference has nothing
    between 2^15 and 2^17 (asserted by _inf_subset)."""
    hip = _hip(F16)
    M, C = 4096, 128
    dev = "cuda:0"
    hot = torch.arange(C, device=dev) % 8 == 5
    gamma = torch.where(hot, 2.0 ** 26, 1.0).float()
    beta = torch.zeros(C, device=dev)
    z = _away_from_zero((1, M, 1, C), 101, 1.0)
    zd = z.double().reshape(M, C)
    mean, inv = zd.mean(0), torch.rsqrt(zd.var(0, unbiased=False) + 1e-5)
    xh = (zd - mean) * inv
    assert float(xh.abs().min()) > 0.4
    y = xh * gamma.double()
    a, mean_k, inv_k = hip.bn_forward(z, gamma, beta, 0.2, 1e-5, 0.1)
    _inf_subset(a.reshape(M, C), torch.where(y > 0, y, 0.2 * y), "bn_forward")
    assert float((mean_k.double() - mean).abs().max()) < 1e-4 and float((inv_k.double() / inv - 1).abs().max()) < 1e-4
    # tangent: at = gamma invstd (zt - mean(zt) - xh mean(xh zt)) lrelu'(y)
    zt = _away_from_zero((1, M, 1, C), 102, 4.0)
    ztd = zt.double().reshape(M, C)
    mask = torch.where(y > 0, 1.0, 0.5)
    ref_t = gamma.double() * inv * (ztd - ztd.mean(0) - xh * (xh * ztd).mean(0)) * mask
    at, s_zt, s_xhzt = hip.bn_tangent(z, zt, mean.float(), inv.float(), gamma, beta, 0.5)
    _inf_subset(at.reshape(M, C), ref_t, "bn_tangent")
    # double backward with a zero first-backward gradient: pz = gamma invstd (qy - mean(qy) - xh mean(qy xh)), qy = qa lrelu'(y)
    qa = _away_from_zero((1, M, 1, C), 103, 4.0)
    qy = qa.double().reshape(M, C) * mask
    ref_p = gamma.double() * inv * (qy - qy.mean(0) - xh * (qy * xh).mean(0))
    zero = torch.zeros(C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    pz = hip.bn_double_bwd(z, qa, zt, torch.zeros_like(z), mean.float(), inv.float(), gamma, beta, 0.5, zero, zero.clone(),
                           s_zt, s_xhzt, dg, db, False)
    _inf_subset(pz.reshape(M, C), ref_p, "bn_double_bwd")


def _slab_layer(hip, up):
    """A layer shape whose conv launch runs split-K at batch 64 (asked of the library), as (I, O, hs)."""
    for I, O, hs in ((512, 1024, 16), (1024, 2048, 8), (256, 512, 32)):
        if hip.lib.rg_conv_split(up, 64, hs // 2, hs // 2, O, I, hip.dt, hip.algo) > 1:
            return I, O, hs
    pytest.skip("rg_conv_split: no layer shape with a split-K plan in this direction")


@gpu
def test_fp16_slab_consumers_overflow_to_infinity():
    """rg_bn_forward_slabs / rg_bn_act_bwd_slabs (reached through HipOps with defer = 1): the z / ga they write from the fp32 slabs
    of exact-integer operands with ONE sample scaled by 2^10 -- infinity from |sum| = 64, the exact value below, every other
    sample bit-exact; and their a / gz with hot channels through gamma (2^60: whatever the distance of an element from the mean,
    the reference has nothing between 2^15 and 2^17 -- asserted)."""
    hip, N, dev = _hip(F16), 64, "cuda:0"
    # forward: conv_down -> bn_forward
    I, O, hs = _slab_layer(hip, 0)
    x, w, y = _down_case(N, hs, hs, I, O, F16)
    M = N * (hs // 2) ** 2
    hot = torch.arange(O, device=dev) % 8 == 2
    gam = torch.where(hot, 2.0 ** 60, 1.0).float()
    bet = torch.zeros(O, device=dev)
    zf = hip.conv_down(x, _cw(w), want_stats=True, defer=1)[0]
    assert getattr(zf, "_rg_slabs", None) is not None
    a, mean_k, inv_k = hip.bn_forward(zf, gam, bet, 0.2, 1e-5, 0.1)
    _exact(zf, y, "z written by bn_forward from the slabs")
    yd = y.double().reshape(M, O)
    mean, inv = yd.mean(0), torch.rsqrt(yd.var(0, unbiased=False) + 1e-5)
    pre = (yd - mean) * inv * gam.double()
    _inf_subset(a.reshape(M, O), torch.where(pre > 0, pre, 0.2 * pre), "a written by bn_forward from the slabs")
    xs = x.clone()
    xs[1] *= 1024
    want = _overflow_expect(ref_down(xs.double(), w.double()))
    zf = hip.conv_down(xs, _cw(w), want_stats=True, defer=1)[0]
    assert getattr(zf, "_rg_slabs", None) is not None
    hip.bn_forward(zf, gam, bet, 0.2, 1e-5, 0.1)
    _same_with_inf(zf, want, "z written by bn_forward from the slabs")
    del x, xs, y, yd, pre, a, zf, want
    # backward: conv_up -> bn_act_bwd
    I, O, hs = _slab_layer(hip, 1)
    g, w, u, _, _ = _up_case(N, hs // 2, hs // 2, O, I, F16)
    M = N * hs * hs
    hot = torch.arange(I, device=dev) % 8 == 2
    gam = torch.where(hot, 2.0 ** 60, 1.0).float()
    bet = torch.zeros(I, device=dev)
    zb = _away_from_zero((N, hs, hs, I), 111, 1.0)
    zd = zb.double().reshape(M, I)
    mean, inv = zd.mean(0), torch.rsqrt(zd.var(0, unbiased=False) + 1e-5)
    xh = (zd - mean) * inv
    ga = hip.conv_up(g, _cw(w), defer=1)
    assert getattr(ga, "_rg_slabs", None) is not None
    dg, db = torch.zeros(I, device=dev), torch.zeros(I, device=dev)
    gz, _, _ = hip.bn_act_bwd(zb, ga, mean.float(), inv.float(), gam, bet, 0.5, dg, db, False, keep_ga=True)
    _exact(ga, u, "ga written by bn_act_bwd from the slabs")
    gy = u.double().reshape(M, I) * torch.where(xh > 0, 1.0, 0.5)
    _inf_subset(gz.reshape(M, I), gam.double() * inv * (gy - gy.mean(0) - xh * (gy * xh).mean(0)), "gz written by bn_act_bwd from the slabs",
                sign_from=2.0 ** 50)                         # (|gy - means| above 2^-10: beyond the fp32 error of the three terms)
    gs = g.clone()
    gs[1] *= 1024
    want = _overflow_expect(ref_up(gs.double(), w.double()))
    ga = hip.conv_up(gs, _cw(w), defer=1)
    assert getattr(ga, "_rg_slabs", None) is not None
    hip.bn_act_bwd(zb, ga, mean.float(), inv.float(), gam, bet, 0.5, dg, db, False, keep_ga=True)
    _same_with_inf(ga, want, "ga written by bn_act_bwd from the slabs")
    torch.cuda.synchronize()
    assert int(hip._sb_sync[0]) == 0, "no hand-off timed out"


@gpu
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_fp16_non_finite_operands_slab_form_image_side_and_resize_conv(value):
    """The remaining backward-chain ops: bn_act_bwd in its slab form (the transposed conv leaves fp32 slabs), the image-side weight
    gradient, upconv3_bwd_data and upconv3_wgrad -- one planted element each; the non-finite outputs are the reference's."""
    from oracle.ops_ref import RefOps
    hip, dev = _hip(F16), "cuda:0"
    # slab form: the planted element of g reaches 4 x 4 pixels of ga in every channel (weights non-zero), so every channel's
    # sums and the whole gz are non-finite in the reference; ga itself stays local
    N = 64
    I, O, hs = _slab_layer(hip, 1)
    w = torch.sign(_gauss((O, 4, 4, I), 121)) * (0.01 + _gauss((O, 4, 4, I), 122).abs() * 0.03)
    g = _plant(_gauss((N, hs // 2, hs // 2, O), 123).to(F16), (7, 3, 2, 17), value)
    zb = _away_from_zero((N, hs, hs, I), 124, 1.0)
    zd = zb.double().reshape(-1, I)
    mean, inv = zd.mean(0), torch.rsqrt(zd.var(0, unbiased=False) + 1e-5)
    gam, bet = 1 + 0.1 * _gauss((I,), 125), 0.1 * _gauss((I,), 126)
    ga = hip.conv_up(g, _cw(w), defer=1)
    assert getattr(ga, "_rg_slabs", None) is not None
    dg, db = torch.zeros(I, device=dev), torch.zeros(I, device=dev)
    gz, _, _ = hip.bn_act_bwd(zb, ga, mean.float(), inv.float(), gam, bet, 0.2, dg, db, False, keep_ga=True)
    u_ref = ref_up(g.double(), w.to(F16).double())
    _nonfinite_like(ga, u_ref, "ga from the slabs")
    assert bool((~torch.isfinite(u_ref)).reshape(-1, I).any(0).all())          # the reference: every channel's sums are non-finite
    assert not bool(torch.isfinite(gz).any()) and not bool(torch.isfinite(dg).any()) and not bool(torch.isfinite(db).any())
    torch.cuda.synchronize()
    assert int(hip._sb_sync[0]) == 0, "no hand-off timed out"
    # image-side weight gradient (row kernel shape: 64 channels, 128-pixel image rows): one channel's 3 x 16 weights
    Ni, H, W, Oi = 3, 16, 128, 64
    img = _gauss((Ni, 3, H, W), 127)
    img = torch.where(img.abs() < 0.01, torch.ones_like(img), img)
    low = _plant(_gauss((Ni, H // 2, W // 2, Oi), 128).to(F16), (1, 3, 20, 41), value)
    dw = torch.zeros(Oi, 3, 4, 4, device=dev)
    hip.skinny_wgrad(low, img, dw, False)
    _nonfinite_like(dw.permute(0, 2, 3, 1), ref_wgrad(low.double(), img.to(F16).double().permute(0, 2, 3, 1).contiguous()), "skinny_wgrad")
    # resize-convolution block: data gradient (local around the planted pixel) and weight gradient (one output channel)
    Nu, Hu, Cin, Cout = 2, 8, 64, 64
    w3 = torch.sign(_gauss((Cout, Cin, 3, 3), 129)) * (0.02 + _gauss((Cout, Cin, 3, 3), 130).abs() * 0.05)
    xu = _gauss((Nu, Hu, Hu, Cin), 131).to(F16)
    gy = _plant(_gauss((Nu, 2 * Hu, 2 * Hu, Cout), 132).to(F16), (1, 7, 9, 5), value)
    ref = RefOps(torch.float64)
    cr = ConvW(w3.to(F16).double().cpu(), None, torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64))
    ch = ConvW(w3, None, torch.zeros_like(w3))
    gx_ref = ref.upconv3_bwd_data(gy.double().cpu(), cr)
    _nonfinite_like(hip.upconv3_bwd_data(gy, ch).cpu(), gx_ref, "upconv3_bwd_data")
    ref.upconv3_wgrad(gy.double().cpu(), xu.double().cpu(), cr, False)
    hip.upconv3_wgrad(gy, xu, ch, False)
    _nonfinite_like(ch.dw.cpu(), cr.dw, "upconv3_wgrad")
