"""The three conv forms of the BatchNorm-free critic (rna_gan_amd.ops_hip.HipOps.conv_down_bias_act / conv_down_mask /
conv_up_mask) on both builds of the library: the fused forms -- a split-K launch whose slabs one of the two finishing kernels of
rg_plainact.hip sums, or the bias + LeakyReLU / the mask in the unsplit conv's epilogue -- against an fp64 reference on the
16-bit-rounded operands and against the same library's conv followed by the separate elementwise pass."""
import pytest
import torch
import torch.nn.functional as F

from both_builds import fp16_twin, ru

pytestmark = pytest.mark.gpu

SLOPE = 0.2
# (I, O, hs, n): the smallest shapes at which a launch splits K (those of test_split_k_batchnorm_fusion_small_shapes) ...
# ... plus the smallest shape whose stride-2 conv does NOT split (64 output columns: the 256 x 64-tile kernel's epilogue)
SMALL = [(64, 128, 16, 8), (128, 256, 8, 8), (256, 512, 4, 8), (64, 64, 16, 8)]
# ... and the benchmark's five critic layers at batch 8 (no CPU convolution at these sizes: library against library only)
# ... plus layer 1 at batch 32, where its tile count fills the chip and the 8-wave kernel's epilogue takes the bias / the mask
BENCH = [(64, 128, 128, 8), (128, 256, 64, 8), (256, 512, 32, 8), (512, 1024, 16, 8), (1024, 2048, 8, 8), (64, 128, 128, 32)]
OPS = ("down_bias", "down_mask", "up_mask")


def _dims(op, I, O, hs, n):
    """(up, N, Hlow, Wlow, O, I, rows of the result, its channels)"""
    ho = hs // 2
    return (1 if op == "up_mask" else 0, n, ho, ho, O, I, n * hs * hs if op == "up_mask" else n * ho * ho, I if op == "up_mask" else O)


def _predict(ops, op, I, O, hs, n):
    up, N, Hl, Wl, O_, I_, M, C = _dims(op, I, O, hs, n)
    kind = ops._plain_fused(up, N, Hl, Wl, O_, I_, M, C, None)[0]
    # (an unsplit masked transposed conv is conv_up's own epilogue: counted as "epilogue" too)
    return kind


def _case(I, O, hs, n, h16, dev):
    from rna_gan_amd.engine import ConvW
    gen = torch.Generator().manual_seed(11 * I + hs + n)
    ho = hs // 2
    w = (torch.randn(O, 4, 4, I, generator=gen) * (2.0 / (I * 16)) ** 0.5).to(h16).float()       # exact in the build's type
    x = torch.randn(n, hs, hs, I, generator=gen).to(h16)
    y = torch.randn(n, ho, ho, O, generator=gen).to(h16)
    bias = torch.randn(O, generator=gen) * 1.5              # conv outputs have a standard deviation near 1.4: signs flip
    bias[::7] = -3.0

    def mask(*shape):
        m = torch.randn(*shape, generator=gen)
        m.view(-1)[::5] = 0.0                               # a <= 0 takes the slope, +0 and -0 included
        m.view(-1)[1::11] = -0.0
        return m.to(h16)
    cw = ConvW(w.clone().to(dev), None, torch.zeros_like(w).to(dev), None, "OHWI")
    return cw, w, x, y, bias, mask(n, ho, ho, O), mask(n, hs, hs, I)


def _lmask(a):
    return torch.where(a.double() > 0, 1.0, SLOPE)


def _ref64(op, w, x, y, bias, m_lo, m_hi):
    """fp64 on the 16-bit-rounded operands (NHWC in, NHWC out)."""
    w64 = w.double().permute(0, 3, 1, 2)                    # [O][I][4][4]
    if op == "up_mask":
        z = F.conv_transpose2d(y.double().permute(0, 3, 1, 2), w64, None, stride=2, padding=1).permute(0, 2, 3, 1)
        return z * _lmask(m_hi)
    z = F.conv2d(x.double().permute(0, 3, 1, 2), w64, None, stride=2, padding=1).permute(0, 2, 3, 1)
    return F.leaky_relu(z + bias.double(), SLOPE) if op == "down_bias" else z * _lmask(m_lo)


def _run(ops, op, cw, x, y, bias, m_lo, m_hi, path, dbias=None):
    if op == "down_bias":
        return ops.conv_down_bias_act(x, cw, bias, SLOPE, path=path)
    if op == "down_mask":
        return ops.conv_down_mask(x, cw, m_lo, SLOPE, path=path)
    return ops.conv_up_mask(y, cw, m_hi, SLOPE, dbias, False, path=path)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _check(op, I, O, hs, n, h16, with_ref64):
    from rna_gan_amd.ops_hip import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps(h16, dev)
    cw, w, x, y, bias, m_lo, m_hi = _case(I, O, hs, n, h16, dev)
    xd, yd, bd, mld, mhd = x.to(dev), y.to(dev), bias.to(dev), m_lo.to(dev), m_hi.to(dev)
    C = I if op == "up_mask" else O
    want_kind = _predict(ops, op, I, O, hs, n)
    db_f = torch.full((C,), 7.0, device=dev)                # written, not added to
    db_u = torch.full((C,), -7.0, device=dev)
    got = _run(ops, op, cw, xd, yd, bd, mld, mhd, None, db_f if op == "up_mask" else None)
    assert ops.plain_paths == {want_kind: 1}, (ops.plain_paths, want_kind)
    assert want_kind in ("slab", "epilogue")
    unf = _run(ops, op, cw, xd, yd, bd, mld, mhd, "unfused", db_u if op == "up_mask" else None)
    torch.cuda.synchronize()
    assert ops.plain_paths == {want_kind: 1, "unfused": 1}
    r16 = ru(h16, 8e-3)
    assert got.dtype == h16 and got.shape == unf.shape and bool(torch.isfinite(got.float()).all())
    d_unf = _rel(got, unf)
    print("%s I=%d O=%d hs=%d n=%d %s path=%s: vs unfused %.3e (gate %.3e)" % (op, I, O, hs, n, h16, want_kind, d_unf, r16))
    assert d_unf <= r16
    if with_ref64:
        ref = _ref64(op, w, x, y, bias, m_lo, m_hi)
        d_ref = _rel(got.cpu(), ref)
        print("    vs fp64 %.3e" % d_ref)
        assert d_ref <= r16
        # masked-out / flipped elements are the point: the reference has both signs and the slope applied somewhere
        assert float(ref.min()) < 0 < float(ref.max())
    if op == "up_mask":
        # the column sums are those of the STORED result, in fp32, to summation order
        want = got.double().reshape(-1, C).sum(0)
        d_cs = _rel(db_f, want)
        d_cu = _rel(db_u, unf.double().reshape(-1, C).sum(0))
        print("    column sums %.3e (unfused path %.3e)" % (d_cs, d_cu))
        assert d_cs <= 1e-4 and d_cu <= 1e-4


@fp16_twin
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("I,O,hs,n", SMALL)
def test_small_shapes_vs_fp64_and_unfused(I, O, hs, n, op, h16=torch.bfloat16):
    _check(op, I, O, hs, n, h16, with_ref64=True)


@fp16_twin
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("I,O,hs,n", BENCH)
def test_benchmark_layers_vs_unfused(I, O, hs, n, op, h16=torch.bfloat16):
    _check(op, I, O, hs, n, h16, with_ref64=False)


@fp16_twin
def test_parameter_list_reaches_both_fused_forms(h16=torch.bfloat16):
    """A dispatch change must not empty a case: over this file's parameter list every op takes the slab path at least once and
    the in-epilogue path at least once (each case above also asserts that the path it predicted here is the one that ran)."""
    from rna_gan_amd.ops_hip import HipOps
    ops = HipOps(h16, torch.device("cuda:0"))
    for op in OPS:
        kinds = {_predict(ops, op, *s) for s in SMALL + BENCH}
        assert kinds == {"slab", "epilogue"}, (op, kinds)


@fp16_twin
def test_finishing_kernels_on_their_own(h16=torch.bfloat16):
    """rg_slab_bias_act / rg_slab_mask / rg_parts_col_sum on slabs written by the test: fp32 and 16-bit slabs, 1..5 of them
    (a fixed-order sum), a row count that is no multiple of the rows a workgroup owns, the narrowest and a > 2048-channel
    width, a slab stride larger than a slab, accumulate on and off."""
    from rna_gan_amd import _abi
    from rna_gan_amd.ops_hip import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps(h16, dev)
    lib = ops.lib
    gen = torch.Generator().manual_seed(3)
    for M, C, ns, s16 in ((37, 8, 1, False), (1000, 64, 3, True), (129, 128, 5, False), (70, 4096, 2, True), (64, 2048, 4, False)):
        stride = M * C + 64
        sl = torch.randn(ns, stride, generator=gen)
        sl = sl.to(h16) if s16 else sl
        bias = torch.randn(C + 1, generator=gen)[1:].clone()        # (4-byte aligned only)
        mask = torch.randn(M, C, generator=gen).to(h16)
        mask.view(-1)[::3] = 0.0
        sld, bd, md = sl.to(dev), torch.randn(C + 1, device=dev)[1:], mask.to(dev)
        bd.copy_(bias)
        sdt = ops.H16 if s16 else _abi.RG_F32
        tot = sl[:, :M * C].double().sum(0).reshape(M, C)
        rows = int(lib.rg_slab_finish_rows(M, C))
        assert rows > 0
        y = torch.empty(M, C, dtype=h16, device=dev)
        _abi.check(lib.rg_slab_bias_act(sld.data_ptr(), ns, stride, sdt, bd.data_ptr(), y.data_ptr(), M, C, SLOPE, ops.stream), "a")
        want = F.leaky_relu(tot + bias.double(), SLOPE)
        assert _rel(y.cpu(), want) <= ru(h16, 4e-3), (M, C, ns, s16)
        parts = torch.full((rows + 1, C), 5.0, device=dev)
        _abi.check(lib.rg_slab_mask(sld.data_ptr(), ns, stride, sdt, md.data_ptr(), SLOPE, y.data_ptr(), parts.data_ptr(), M, C,
                                    ops.stream), "b")
        want = tot * _lmask(mask)
        assert _rel(y.cpu(), want) <= ru(h16, 4e-3), (M, C, ns, s16)
        assert bool((parts[rows] == 5.0).all())                 # nothing written past the promised rows
        cs = y.double().sum(0)
        for acc in (0, 1):
            out = torch.full((C + 1,), 2.0, device=dev)[1:]
            _abi.check(lib.rg_parts_col_sum(parts.data_ptr(), rows, C, out.data_ptr(), acc, ops.stream), "c")
            assert _rel(out, cs + 2.0 * acc) <= 1e-4, (M, C, ns, s16, acc)
    assert lib.rg_slab_finish_rows(10, 12) == 0 and lib.rg_slab_finish_rows(10, 8 * 96) == 0     # widths the layout does not cover


def test_fp32_storage_takes_the_elementwise_pass():
    """fp32 precision: the conv as it stands, then one elementwise bias + LeakyReLU / mask pass."""
    from rna_gan_amd.ops_hip import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps(torch.float32, dev)
    I, O, hs, n = 64, 128, 16, 8
    cw, w, x, y, bias, m_lo, m_hi = _case(I, O, hs, n, torch.bfloat16, dev)
    x, y, m_lo, m_hi = x.float(), y.float(), m_lo.float(), m_hi.float()
    for op in OPS:
        db = torch.zeros(I, device=dev)
        got = _run(ops, op, cw, x.to(dev), y.to(dev), bias.to(dev), m_lo.to(dev), m_hi.to(dev), None, db if op == "up_mask" else None)
        assert got.dtype == torch.float32
        assert _rel(got.cpu(), _ref64(op, w, x, y, bias, m_lo, m_hi)) <= 1e-5, op
        if op == "up_mask":
            assert _rel(db, got.double().reshape(-1, I).sum(0)) <= 1e-4
    assert set(ops.plain_paths) == {"unfused"}


@fp16_twin
def test_head_bias_and_its_gradient(h16=torch.bfloat16):
    from rna_gan_amd.engine import ConvW
    from rna_gan_amd.ops_hip import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps(h16, dev)
    gen = torch.Generator().manual_seed(1)
    N, C = 37, 96
    a = torch.randn(N, 4, 4, C, generator=gen).to(h16)
    w = (torch.randn(1, C, 4, 4, generator=gen) * 0.05).to(h16).float()
    b = torch.tensor([-0.7])
    cw = ConvW(w.to(dev), b.to(dev))
    h, out = ops.head_fwd_bias(a.to(dev), cw, cw.bias, SLOPE)
    h0, _ = ops.head_fwd(a.to(dev), cw, SLOPE)
    want = torch.einsum("nijc,cij->n", a.double(), w.double()[0]) - 0.7
    assert _rel(h.cpu(), want) <= 1e-5 and _rel(out.cpu(), F.leaky_relu(want, SLOPE)) <= 1e-5
    assert float(((h - h0).cpu().double() + 0.7).abs().max()) <= 1e-6        # the same kernel, the bias added once
    gh = torch.randn(300, generator=gen)
    for acc in (False, True):
        db = torch.full((1,), 3.0, device=dev)
        ops.vec_sum(gh.to(dev), db, acc)
        assert abs(float(db) - (float(gh.double().sum()) + 3.0 * acc)) <= 1e-4
