"""fp64 references and operand builders of tests/test_vae_fid_ops_gpu.py (the betaVAE-training and FID kernels, op by op).

Everything here runs on the CPU in numpy / torch fp64 and takes nothing from rna_gan_amd; tests/test_vae_fid_refs_cpu.py pins
each helper against torch itself (conv2d, max_pool2d, avg_pool2d, autograd) and asserts the exactness conditions of the
GPU cases on the same operands, so that the conditions are checked without a kernel.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24                                   # fp32's unit round-off
SENTINEL = float.fromhex("0x1.b3c5a6p+61")         # a finite fp32 pattern no kernel here produces (0x5e59e2d3)


def ceil64(v):
    return (v + 63) // 64 * 64


def bits(t):
    """the int32 image of an fp32 tensor (bit-for-bit comparisons: tells -0.0 from +0.0, never touches NaN arithmetic)"""
    return t.contiguous().view(torch.int32)


def ints(shape, seed, lo=-3, hi=3):
    """small integers as fp64 (exact in bf16, fp16 and fp32)"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def gauss(shape, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen, dtype=torch.float64) * scale


def pow2_affine(n, seed):
    """scale in {+-0.5, +-1, +-2}, shift small integers: an exact epilogue on integer sums"""
    gen = torch.Generator().manual_seed(seed)
    e = torch.randint(-1, 2, (n,), generator=gen).double()
    s = torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    return s * 2.0 ** e, torch.randint(-4, 5, (n,), generator=gen).double()


def lrelu32(v, slope):
    """The epilogue's activation on an fp32 tensor, in fp32: v > 0 ? v : v * slope -- one IEEE multiplication by fl32(slope),
    reproduced bit for bit by the CPU (slope 0 leaves -0.0 for negative v: compare by value)."""
    assert v.dtype == torch.float32
    if slope == 1.0:
        return v
    return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))


def gemm_ref(a, b, scale=None, shift=None):
    """(ref, S) in fp64: ref = (a . b^T) * scale + shift, S = (|a| . |b|^T) * |scale| + |shift|"""
    a, b = a.double(), b.double()
    ref, S = a @ b.t(), a.abs() @ b.abs().t()
    if scale is not None:
        ref, S = ref * scale.double(), S * scale.double().abs()
    if shift is not None:
        ref, S = ref + shift.double(), S + shift.double().abs()
    return ref, S


def exact_condition(ref, S, what, nontrivial=True):
    """(E): every partial sum in any order (and through split-K slabs) is an integer multiple of the smallest scale below 2^24,
    so the fp32 result equals the fp64 one.  A condition of the test, asserted on the reference alone."""
    assert float(S.max()) <= 2 ** 24, "%s: S = %g > 2^24" % (what, float(S.max()))
    assert torch.equal(ref.float().double(), ref), what + ": the reference is not an fp32 number"
    if nontrivial:
        assert float((ref == 0).double().mean()) <= 0.25 and int(torch.unique(ref).numel()) >= 8, what + ": trivial case"


def bound(ref, S, K, u=U32):
    """(B), the project's C2 bound: u |ref| + K 2^-24 (1 + u) S + 2^-25; vacuous above K = 1024 (+ 1 per epilogue factor)"""
    assert K <= 1025, "the bound is vacuous above K = 1024 (+ 1 where an epilogue factor adds a rounding)"
    return u * ref.double().abs() + K * 2.0 ** -24 * (1 + u) * S.double() + 2.0 ** -25


# ------------------------------------------------------------------ Inception data movement (index arithmetic, numpy)
def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def im2col_ref(x, kh, kw, sh, sw, ph, pw):
    """x [N, H, W, C] -> cols [(n, ho, wo)][(i, j, c)] = x[n][ho sh - ph + i][wo sw - pw + j][c] or 0 outside the image"""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, kh, sh, ph), out_size(W, kw, sw, pw)
    cols = np.zeros((N, Ho, Wo, kh, kw, C), dtype=x.dtype)
    for ho in range(Ho):
        for wo in range(Wo):
            for i in range(kh):
                for j in range(kw):
                    hi, wi = ho * sh - ph + i, wo * sw - pw + j
                    if 0 <= hi < H and 0 <= wi < W:
                        cols[:, ho, wo, i, j, :] = x[:, hi, wi, :]
    return cols.reshape(N * Ho * Wo, kh * kw * C)


def pool_ref(x, k, s, p, mode):
    """x [N, H, W, C] fp64.  mode 0: max over the in-range taps; mode 1: sum of the in-range taps / (k k) (padding counted)"""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    y = np.empty((N, Ho, Wo, C))
    for ho in range(Ho):
        for wo in range(Wo):
            h0, w0 = max(ho * s - p, 0), max(wo * s - p, 0)
            h1, w1 = min(ho * s - p + k, H), min(wo * s - p + k, W)
            win = x[:, h0:h1, w0:w1, :].reshape(N, -1, C)
            y[:, ho, wo, :] = win.max(1) if mode == 0 else win.sum(1) / (k * k)
    return y


def dyadic(shape, seed, lo=-1024, hi=1024, q=2.0 ** -8):
    """multiples of 2^-8 in [-4, 4]: sums of nine are exact in fp32, so the average pool's only rounding is its division"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=gen).double() * q


# ------------------------------------------------------------------ VAE element-wise kernels and the loss
def reparam_ref(mu, lv, eps):
    """(z, largest term of the sum) in fp64"""
    t = eps * torch.exp(0.5 * lv)
    return mu + t, torch.maximum(mu.abs(), t.abs())


def reparam_bwd_ref(gz, lv, eps, gmu_loss, glv_loss):
    """(gmu, glv, largest term of glv's sum) in fp64"""
    t = gz * eps * 0.5 * torch.exp(0.5 * lv)
    gmu = gz + (gmu_loss if gmu_loss is not None else 0.0)
    big = t.abs() if glv_loss is None else torch.maximum(t.abs(), glv_loss.abs())
    return gmu, t + (glv_loss if glv_loss is not None else 0.0), big


def loss_ref(x, xr, mu, lv, beta, training):
    """betaVAEloss in fp64 on the UNPADDED [N][F] rows, with the analytic gradients of `total`:
    recons = mean (xr - x)^2 over N F;  kl = mean_n -0.5 sum_z (1 + lv - mu^2 - e^lv);  total = recons + beta kl (training)"""
    N, F = x.shape
    d = xr - x
    recons = (d * d).sum() / (N * F)
    kl = -0.5 * (1 + lv - mu * mu - lv.exp()).sum() / N
    b = beta if training else 0.0
    return {"total": recons + b * kl, "recons": recons, "kl": kl, "g_recons": 2.0 * d / (N * F), "g_mean": b * mu / N,
            "g_logvar": b * 0.5 * (lv.exp() - 1.0) / N}


def loss_inputs(N, F, ld, Z, seed):
    """x, xr [N][ld] with xr - x in {0, +-0.5, +-1} and zero pad columns (sum d^2 is then exact in fp32 while 4 N ld < 2^24);
    mu, lv [N][Z] with |lv| <= 3 (no overflow / underflow of exp)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (N, ld), generator=gen).double() * 0.25
    d = torch.randint(-2, 3, (N, ld), generator=gen).double() * 0.5
    x[:, F:] = 0.0
    d[:, F:] = 0.0
    mu = torch.randn((N, Z), generator=gen, dtype=torch.float64)
    lv = (torch.rand((N, Z), generator=gen, dtype=torch.float64) * 6.0 - 3.0)
    return x.float(), (x + d).float(), mu.float(), lv.float()


def loss_exact_condition(x, xr, N, F, ld):
    d = xr.double() - x.double()
    assert 4 * N * ld < 2 ** 24, "sum d^2 (multiples of 0.25 up to N ld) leaves fp32's exact range"
    assert set(torch.unique(d).tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    assert bool((d[:, F:] == 0).all()) and bool((x[:, F:] == 0).all()) and bool((xr[:, F:] == 0).all())
    assert float((d * d).sum()) > 0                       # a non-zero loss tells the divisor N F from N ld (ld > F)


def loss_kl_path(N, ld, Z):
    """Additions on the longest path of rg_vae_loss's two-stage reduction of the KL sum, plus 4 (the three additions and the
    product inside a term), from the launch geometry of rg_vae.hip: nb = min(ceil(max(N ld, N Z) / 1024), 1024) blocks of 256
    threads; a thread sums ceil(N Z / (256 nb)) terms serially; a block tree is 6 shuffle steps + 3 additions of the wave
    partials; the final block sums ceil(nb / 256) partials per thread serially and runs the same tree."""
    nb = min(max(-(-max(N * ld, N * Z) // 1024), 1), 1024)
    serial1 = -(-(N * Z) // (256 * nb))
    serial2 = -(-nb // 256)
    return serial1 + 9 + serial2 + 9 + 4


def ulps32(got, ref64):
    """|got - fl32(ref)| in units in the last place of fl32(ref)  (numpy arrays)"""
    r32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    sp = np.spacing(np.abs(r32)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - r32.astype(np.float64)) / sp


def finite_lv(shape, seed):
    """log-variances in [-6, 6]: exp(0.5 lv) in [0.05, 20]"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=gen) * 12.0 - 6.0).float()


assert math.isfinite(SENTINEL) and float(np.float32(SENTINEL)) == SENTINEL
