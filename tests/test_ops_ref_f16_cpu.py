"""The torch twin (oracle/ops_ref.RefOps) as a 16-bit twin of EITHER build of the library: with act_dtype = float16 every
operand the kernels hold as a 16-bit MFMA operand -- weights, the NCHW image, the up-sampled + padded image -- is rounded to
fp16, exactly as the bf16 twin rounds them to bf16.  Pinned per op in three ways:
  * on fp32 masters the op equals, bit for bit, the same op on masters pre-rounded to the storage type;
  * it differs from the op evaluated on the un-rounded masters (a twin whose operand rounding is switched off), on inputs
    where that rounding matters (weights of ordinary size: about half of them are not fp16 numbers);
  * the fp32 / fp64 twins do not round at all.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle.ops_ref import RefOps
from rna_gan_amd.engine import ConvW

H16 = [torch.float16, torch.bfloat16]


class _Unrounded(RefOps):
    """The twin as it was for fp16 before: activations rounded on store, operands formed from fp32 data used as they are."""

    def _q16(self, t):
        return t.to(self.f)


def _rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tm(w):
    wt = w.permute(0, 2, 3, 1).contiguous()
    return ConvW(wt, None, torch.zeros_like(wt), None, "OHWI")


def _cases(dt):
    """name -> fn(ops, q) with q = the rounding applied to the MASTERS by the caller (identity or to dt)."""
    w = _rnd((16, 8, 4, 4), 1, 0.09)
    x = _rnd((2, 8, 8, 8), 2).to(dt)
    g = _rnd((2, 4, 4, 16), 3).to(dt)
    m = _rnd((2, 8, 8, 8), 4).to(dt)
    w3 = _rnd((5, 8, 3, 3), 5, 0.12)
    b3 = _rnd((5,), 6, 0.1)
    gy3 = _rnd((2, 16, 16, 5), 7).to(dt)
    wi = _rnd((16, 3, 4, 4), 8, 0.2)
    bi = _rnd((16,), 9, 0.1)
    img = _rnd((2, 3, 8, 8), 10)
    a_lo = _rnd((2, 4, 4, 16), 11).to(dt)
    w0 = _rnd((24, 8, 4, 4), 12, 0.09)
    z = _rnd((5, 24), 13)
    wh = _rnd((1, 8, 4, 4), 14, 0.1)
    a4 = _rnd((5, 4, 4, 8), 15).to(dt)
    gh = _rnd((5,), 16)
    lw, lx = _rnd((12, 40), 17, 0.15), _rnd((6, 40), 18)
    return {
        "conv_down": lambda o, q: o.conv_down(x, _tm(q(w))),
        "conv_up": lambda o, q: o.conv_up(g, _tm(q(w))),
        "conv_up(masked)": lambda o, q: o.conv_up(g, _tm(q(w)), m, 0.2),
        "upconv3": lambda o, q: o.upconv3(x, ConvW(q(w3), b3), b3),
        "upconv3(nchw)": lambda o, q: o.upconv3(x, ConvW(q(w3), b3), b3, out_nchw=True),
        "upconv3_bwd_data": lambda o, q: o.upconv3_bwd_data(gy3, ConvW(q(w3), None)),
        "first_down": lambda o, q: o.first_down(q(img), ConvW(q(wi), None), bi, 0.2),
        "first_down_tangent": lambda o, q: o.first_down_tangent(q(img), ConvW(q(wi), None), a_lo, 0.2),
        "last_up": lambda o, q: o.last_up(a_lo, ConvW(q(wi), None), None, False),
        "last_up(tanh)": lambda o, q: o.last_up(a_lo, ConvW(q(wi), None), _rnd((3,), 19, 0.1), True),
        "g0_fwd": lambda o, q: o.g0_fwd(z, ConvW(q(w0), None)),
        "head_fwd": lambda o, q: o.head_fwd(a4, ConvW(q(wh), None), 0.2)[0],
        "head_bwd_data": lambda o, q: o.head_bwd_data(gh, ConvW(q(wh), None)),
        "linear_affine_act": lambda o, q: o.linear_affine_act(lx, q(lw), 1.0, 0.0, 0.2),
    }


@pytest.mark.parametrize("dt", H16, ids=["float16", "bfloat16"])
def test_sixteen_bit_twin_rounds_the_operands_formed_from_fp32_data(dt):
    ident = lambda t: t
    pre = lambda t: t.to(dt).float()
    twin, plain = RefOps(dt), _Unrounded(dt)
    for name, fn in _cases(dt).items():
        on_masters, on_rounded, unrounded = fn(twin, ident), fn(twin, pre), fn(plain, ident)
        assert on_masters.dtype == on_rounded.dtype and on_masters.shape == on_rounded.shape
        assert torch.equal(on_masters, on_rounded), name + ": the twin does not round its operands to the storage type"
        if name not in ("upconv3", "upconv3(nchw)"):             # (these also round the up-sampled image: next test)
            assert torch.equal(fn(plain, pre), on_masters), name + ": rounding the masters by hand gives something else"
        assert not torch.equal(on_masters, unrounded), name + ": the case does not depend on the operand rounding"


@pytest.mark.parametrize("dt", H16, ids=["float16", "bfloat16"])
def test_sixteen_bit_twin_rounds_the_upsampled_image(dt):
    """The up-sampled + reflection-padded image has no master to pre-round: the twin's result is compared with the same
    convolution / weight gradient written out here over the explicitly rounded image."""
    twin, plain = RefOps(dt), _Unrounded(dt)
    x = _rnd((2, 6, 6, 8), 21).to(dt)
    w = _rnd((5, 8, 3, 3), 22, 0.12).to(dt).float()              # exact in the storage type: only the image's rounding is left
    gy = _rnd((2, 12, 12, 5), 23).to(dt)
    up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    pad = F.pad(up, (1, 1, 1, 1), mode="reflect")
    assert not torch.equal(pad, pad.to(dt).float())              # interpolation weights 1/16 .. 9/16: more bits than stored
    padq = pad.to(dt).float()
    want = F.conv2d(padq, w).permute(0, 2, 3, 1).contiguous().to(dt)
    assert torch.equal(twin.upconv3(x, ConvW(w, None), None), want)
    assert not torch.equal(plain.upconv3(x, ConvW(w, None), None), want)
    cw, cp = ConvW(w, None, torch.zeros_like(w)), ConvW(w, None, torch.zeros_like(w))
    twin.upconv3_wgrad(gy, x, cw, False)
    plain.upconv3_wgrad(gy, x, cp, False)
    dw = torch.nn.grad.conv2d_weight(padq, w.shape, gy.float().permute(0, 3, 1, 2))
    assert torch.equal(cw.dw, dw) and not torch.equal(cp.dw, dw)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_wide_twins_use_the_masters_as_they_are(dt):
    twin = RefOps(dt)
    w = _rnd((16, 8, 4, 4), 1, 0.09).to(dt)
    assert torch.equal(twin._wq(w), w) and torch.equal(twin._q16(w), w)
    x = _rnd((2, 8, 8, 8), 2).to(dt)
    y = twin.conv_down(x, _tm(w))
    assert y.dtype == dt
    assert torch.equal(y, F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=2, padding=1).permute(0, 2, 3, 1).contiguous())
