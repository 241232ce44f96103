"""(no GPU) The fp64 reference helpers of tests/test_vae_fid_ops_gpu.py against torch itself, and the exactness / bound
conditions of the GPU cases asserted on the very operands those cases build -- without a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_fid_refs as R
from oracle.ref_cpu import oracle_vae_loss

WINDOWS = [(3, 3, 2, 2, 0, 0), (3, 3, 1, 1, 1, 1), (5, 5, 1, 1, 2, 2), (1, 7, 1, 1, 0, 3), (7, 1, 1, 1, 3, 0),
           (1, 3, 1, 1, 0, 1), (3, 1, 1, 1, 1, 0)]


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "k%dx%d_s%d%d_p%d%d" % w)
def test_im2col_reference_times_weight_is_conv2d(win):
    kh, kw, sh, sw, ph, pw = win
    for C in (8, 3):
        x = R.gauss((2, 9, 7, C), 3).numpy()
        w = R.gauss((5, C, kh, kw), 4)
        cols = torch.from_numpy(R.im2col_ref(x, kh, kw, sh, sw, ph, pw))
        y = cols @ w.permute(0, 2, 3, 1).reshape(5, -1).t()               # weight as [Cout][(i, j, c)], inception.py's fold
        ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), w, stride=(sh, sw), padding=(ph, pw)).permute(0, 2, 3, 1)
        assert torch.allclose(y.reshape(ref.shape), ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W", [(9, 7), (8, 8)])
def test_pool_references_are_torch_pools(H, W):
    x = R.gauss((2, H, W, 5), 7)
    xc = x.permute(0, 3, 1, 2)
    mx = F.max_pool2d(xc, 3, 2, 0).permute(0, 2, 3, 1)
    av = F.avg_pool2d(xc, 3, 1, 1, count_include_pad=True).permute(0, 2, 3, 1)
    assert np.array_equal(R.pool_ref(x.numpy(), 3, 2, 0, 0), mx.numpy())
    assert np.allclose(R.pool_ref(x.numpy(), 3, 1, 1, 1), av.numpy(), rtol=0, atol=1e-14)
    neg = -x.abs() - 1.0                                                   # all negative: a max that starts at 0 would show
    assert np.array_equal(R.pool_ref(neg.numpy(), 3, 2, 0, 0), F.max_pool2d(neg.permute(0, 3, 1, 2), 3, 2, 0).permute(0, 2, 3, 1).numpy())


def test_average_pool_inputs_sum_exactly_in_fp32():
    """the GPU case's inputs: multiples of 2^-8 up to 4 -- nine of them sum exactly in fp32 in any order"""
    x = R.dyadic((2, 9, 7, 5), 11)
    assert torch.equal(x.float().double(), x) and float(x.abs().max()) * 9 * 2 ** 8 < 2 ** 24
    s = R.pool_ref(x.numpy(), 3, 1, 1, 1) * 9
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)


LOSS_SHAPES = [(3, 50, 64, 8), (12, 1030, 1088, 136), (40, 19198, 19264, 16)]


@pytest.mark.parametrize("N,Fe,ld,Z", LOSS_SHAPES)
def test_loss_reference_is_the_oracle_and_autograd(N, Fe, ld, Z):
    x, xr, mu, lv = R.loss_inputs(N, Fe, ld, Z, 100 + N)
    R.loss_exact_condition(x, xr, N, Fe, ld)
    L = R.loss_kl_path(N, ld, Z)
    assert L <= 64
    for training in (True, False):
        xd = x[:, :Fe].double()
        xrd, mud, lvd = (t.double().requires_grad_(True) for t in (xr[:, :Fe], mu, lv))
        o = oracle_vae_loss(xd, xrd, mud, lvd, 0.75, training=training)
        r = R.loss_ref(xd, xrd.detach(), mud.detach(), lvd.detach(), 0.75, training)
        for a, b in (("total", "total_loss"), ("recons", "reconstruction_loss"), ("kl", "kl_loss")):
            assert abs(float(r[a]) - float(o[b].detach())) <= 1e-12 * max(1.0, abs(float(o[b].detach())))
        g = torch.autograd.grad(o["total_loss"], (xrd, mud, lvd), allow_unused=True)
        for name, gg, like in (("g_recons", g[0], xrd), ("g_mean", g[1], mud), ("g_logvar", g[2], lvd)):
            gg = torch.zeros_like(like) if gg is None else gg
            assert torch.allclose(r[name] + torch.zeros_like(like), gg, rtol=1e-12, atol=1e-15), name
    # the divisor: N F and N ld give different losses on these inputs
    d = (xr - x).double()
    assert float((d * d).sum()) / (N * Fe) != float((d * d).sum()) / (N * ld)


def test_kl_path_lengths():
    """nb and the serial lengths for the three shapes, by hand: (3, 64, 8): 1 block, 24 terms over 256 threads;
    (40, 19264, 16): 753 blocks, 640 terms, 3 partials per thread of the final block"""
    assert R.loss_kl_path(3, 64, 8) == 1 + 9 + 1 + 9 + 4
    assert R.loss_kl_path(12, 1088, 136) == 1 + 9 + 1 + 9 + 4
    assert R.loss_kl_path(40, 19264, 16) == 1 + 9 + 3 + 9 + 4


def test_reparam_backward_reference_is_autograd():
    for with_loss in (True, False):
        mu, eps, gz = R.gauss((257,), 1), R.gauss((257,), 2), R.gauss((257,), 3)
        lv = R.finite_lv((257,), 4).double()
        gml, glvl = (R.gauss((257,), 5), R.gauss((257,), 6)) if with_loss else (None, None)
        mud, lvd = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
        z, big = R.reparam_ref(mud, lvd, eps)
        assert torch.equal(z.detach(), mu + eps * torch.exp(0.5 * lv)) and bool((big >= 0).all())
        obj = (z * gz).sum()
        if with_loss:
            obj = obj + (mud * gml).sum() + (lvd * glvl).sum()
        g = torch.autograd.grad(obj, (mud, lvd))
        gmu, glv, _ = R.reparam_bwd_ref(gz, lv, eps, gml, glvl)
        assert torch.allclose(gmu, g[0], rtol=1e-13, atol=0) and torch.allclose(glv, g[1], rtol=1e-12, atol=1e-15)
    assert float(torch.exp(0.5 * R.finite_lv((1000,), 9).double()).max()) < 21 and float(R.finite_lv((1000,), 9).min()) >= -6


# ------------------------------------------------------------------ (E) / (B) conditions of the GEMM cases, on their operands
def test_gemm_exactness_conditions_hold_for_every_case():
    import test_vae_fid_ops_gpu as G
    for case in G.GEMM_CASES:
        name, M, Kp, Nout, ldy = case
        a, b = G.gemm_operands_int(M, Kp, Nout)
        assert 9 * Kp * 2 + 4 <= 2 ** 24                                  # operands in {-3..3}, |scale| <= 2, |shift| <= 4
        sc, sh = R.pow2_affine(Nout, 7)
        for scale, shift in ((None, None), (sc, sh), (None, sh), (sc, None)):
            ref, S = R.gemm_ref(a, b, scale, shift)
            R.exact_condition(ref, S, name)
        assert torch.equal(a.bfloat16().double(), a) and torch.equal(b.bfloat16().double(), b)
    for M, K, Nout in G.LINEAR_EXACT_SHAPES:
        a, b = R.ints((M, K), 21), R.ints((Nout, K), 22)
        ref, S = R.gemm_ref(a, b, *R.pow2_affine(Nout, 7))
        R.exact_condition(ref, S, "linear %d x %d x %d" % (M, K, Nout))


def test_bound_conditions_hold_for_every_case():
    """(B): K (+ 1 per epilogue factor) <= 1025 for the epilogues each case runs -- at least two per GEMM case, every generic and
    packed linear case -- and the bound itself is the C2 formula."""
    import test_vae_fid_ops_gpu as G
    for name, M, Kp, Nout, ldy in G.GEMM_CASES:
        ks = [Kp + int(sc) + int(sh) + int(slope not in (0.0, 1.0)) for _, sc, sh, slope in G.EPILOGUES]
        assert sum(k <= 1025 for k in ks) >= 2, name
    for M, K, ldx, c0, Nout, ldy, d0 in G.SLICES:
        assert K + 2 <= 1025 and c0 + K <= ldx and d0 + Nout <= ldy
    ref, S = R.gemm_ref(R.gauss((3, 8), 1), R.gauss((4, 8), 2))
    assert torch.equal(R.bound(ref, S, 8), R.U32 * ref.abs() + 8 * 2.0 ** -24 * (1 + R.U32) * S + 2.0 ** -25)
    with pytest.raises(AssertionError):
        R.bound(ref, S, 1026)


def test_lrelu32_is_the_epilogue_activation():
    v = torch.tensor([-3.0, -0.0, 0.0, 2.5, -1e-30], dtype=torch.float32)
    assert torch.equal(R.lrelu32(v, 1.0), v)
    assert bool((R.lrelu32(v, 0.0) == torch.tensor([0.0, 0.0, 0.0, 2.5, 0.0])).all())
    s = np.float32(0.01)
    assert torch.equal(R.lrelu32(v, 0.01)[:1], torch.tensor([np.float32(-3.0) * s]))


def test_ulps_and_sentinel():
    assert R.ulps32(np.float32(1.0) + np.spacing(np.float32(1.0)), 1.0) == 1.0
    t = torch.full((4,), R.SENTINEL, dtype=torch.float32)
    assert bool((R.bits(t) == 0x5e59e2d3).all())
    assert R.bits(torch.tensor([-0.0]))[0] != R.bits(torch.tensor([0.0]))[0]
