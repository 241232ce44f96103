"""References and operand builders of tests/test_f32_planes_ops_gpu.py (the fp32 mode's convolutions and weight gradients on
bf16 planes: rna_gan_amd/csrc/rg_conv8f.hip, rg_wgrad8f.hip, rg_mfma_conv_up_planes64), pinned on the CPU by
tests/test_f32_planes_refs_cpu.py.

The C ABI takes the planes as plain buffers, so a test can hand the kernels planes it built itself.  With small integers (times
powers of two) in the planes every product and every partial sum -- in any order, in any split-K slab -- is an fp32 number, and
the kernel's output must be torch.equal to the reference below:

  planes_expected   sum over PAIRS[products] of the convolution of plane p of A with plane q of B (fp64; the matrix-product
                    references of tests/test_ops_exact_gpu.py).  A is the activation operand (x of the conv, gy of the transposed
                    conv, `low` of the weight gradient), B the other one (the weights, `high`).
  one-hot form      plane p of A holds X, plane q of B holds W, every other plane is zero: ref(X, W) when (p, q) is a pair of
                    the tier, EXACTLY zero otherwise -- says WHICH pair a kernel reads.
  all-live form     three independent sparse {-1, 0, +1} tensors per operand, scaled 2^0, 2^-2, 2^-4 (A) and 2^0, 2^-6, 2^-12 (B):
                    the nine pair weights 2^-(2p + 6q) are distinct, so a swapped, duplicated or dropped pair changes the result;
                    every term is a multiple of 2^-16, and with sum_pairs weight * sum |a||b| <= 2^8 everything is exact.
  unit-weight form  all scales 1 (the output is an integer): for the BatchNorm column sums of the fp32 epilogue, exact while the
                    column sums of |y| and y^2 stay <= 2^24.

The conditions (the bounds, the non-trivial-case rule of test_ops_exact_gpu._conditions, and "every (pair, k-tile) group
contributes a non-zero term to some output of every tile") are asserted on the reference alone, before any comparison.
Operands are drawn on the CPU from fixed seeds, so the CPU test checks the very tensors the GPU tests use.
"""
import torch

from test_ops_exact_gpu import _conditions, _density, ref_down, ref_up, ref_wgrad

PAIRS = {6: [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)],        # hh hm mh hl lh mm   (A plane, B plane)
         3: [(0, 0), (0, 1), (1, 0)]}                                # hh hm mh
OPS = {"down": ref_down, "up": ref_up, "wgrad": ref_wgrad}
A_SCALE = [1.0, 2.0 ** -2, 2.0 ** -4]
B_SCALE = [1.0, 2.0 ** -6, 2.0 ** -12]
WSUM = {k: sum(A_SCALE[p] * B_SCALE[q] for p, q in v) for k, v in PAIRS.items()}
UNIT = 2.0 ** 16                                                     # every term of the all-live form is a multiple of 1 / UNIT
L_EXACT = 2.0 ** 8                                                   # ... and all of them below this: 24 bits


def operand_shapes(op, N, Hl, Wl, O, I):
    """(shape of A, shape of B, reduction length) at the low-resolution plane Hl x Wl"""
    if op == "down":
        return (N, 2 * Hl, 2 * Wl, I), (O, 4, 4, I), 16 * I
    if op == "up":
        return (N, Hl, Wl, O), (O, 4, 4, I), 4 * O
    return (N, Hl, Wl, O), (N, 2 * Hl, 2 * Wl, I), N * Hl * Wl


def planes_expected(op, A_planes, B_planes, products):
    """sum over the tier's pairs (p, q) of op(plane p of A, plane q of B) in fp64 -- formed per A plane as op(A_p, sum of the B_q
    paired with p): the same by linearity, and for the builders' operands (multiples of 2^-12 below 2) every sum is exact"""
    out = None
    for p in sorted({p for p, _ in PAIRS[products]}):
        b = sum(B_planes[q].double() for pp, q in PAIRS[products] if pp == p)
        t = OPS[op](A_planes[p].double(), b)
        out = t if out is None else out + t
    return out


def split_ref(v):
    """rg_split_planes by its definition (rg_conv8f.hip): h = bf16_rne(v), m = bf16_rne(v - h), l = bf16_rne(v - h - m), the
    residuals zero where h is not finite.  [3, ...] bf16 from torch's CPU casts; the subtractions are fp32, as the kernel's."""
    v = v.detach().cpu().float()
    h = v.bfloat16()
    r1 = torch.where(torch.isfinite(h.float()), v - h.float(), torch.zeros_like(v))
    m = r1.bfloat16()
    r2 = r1 - m.float()
    return torch.stack([h, m, r2.bfloat16()])


# ------------------------------------------------------------------ the cases, as (N, Hlow, Wlow, O, I)
KERNELS = {"down256": ("down", 256, 256), "down512": ("down", 512, 128), "up256": ("up", 256, 256), "up512": ("up", 512, 128),
           "up64": ("up", 256, 64),                         # rg_mfma_conv_up_planes64: never split, no statistics, fused mask
           "wgrad_wide": ("wgrad", 256, 256), "wgrad_narrow": ("wgrad", 128, 512)}        # (op, tile rows, tile columns)
PAIR_TABLE = {"down256": (1, 16, 16, 256, 64), "down512": (2, 16, 16, 128, 64), "up256": (1, 16, 16, 64, 256),
              "up512": (2, 16, 16, 64, 128), "up64": (1, 16, 16, 64, 64), "wgrad_wide": (1, 16, 16, 256, 16),
              "wgrad_narrow": (1, 16, 16, 128, 32)}
# the smallest unsplit launches of the tiled kernels (tiles >= 256), each with a row tail; up512: 4 classes x 64 row tiles x 1
UNSPLIT = {"down256": (257, 8, 8, 1024, 64), "down512": (681, 8, 8, 384, 64), "up256": (257, 8, 8, 64, 256),
           "up512": (505, 8, 8, 64, 128)}
# row tail (M = 320 / 768), rectangular planes (the 512-row tile needs M >= 512: N = 4), two channel blocks per tap (Cin = 128),
# several column tiles (a non-power-of-two count for the 128-wide tile), unsplit
SWEEP = {
    "down256": [(5, 8, 8, 256, 64), (2, 4, 32, 256, 64), (2, 32, 4, 256, 64), (1, 16, 16, 256, 128), (1, 16, 16, 512, 64),
                UNSPLIT["down256"]],
    "down512": [(3, 16, 16, 128, 64), (4, 4, 32, 128, 64), (4, 32, 4, 128, 64), (2, 16, 16, 128, 128), (2, 16, 16, 384, 64),
                UNSPLIT["down512"]],
    # (64 input channels at 3 products are 12 k-tiles, never split: the row tail also at 128, where both tiers split)
    "up256": [(5, 8, 8, 64, 256), (2, 4, 32, 64, 256), (2, 32, 4, 64, 256), (1, 16, 16, 128, 256), (5, 8, 8, 128, 256),
              (1, 16, 16, 64, 512), UNSPLIT["up256"]],
    "up512": [(3, 16, 16, 64, 128), (4, 4, 32, 64, 128), (4, 32, 4, 64, 128), (2, 16, 16, 128, 128), (3, 16, 16, 128, 128),
              (2, 16, 16, 64, 384), UNSPLIT["up512"]],
    "up64": [(1, 16, 16, 64, 64), (5, 8, 8, 64, 64), (2, 4, 32, 64, 64), (2, 32, 4, 64, 64), (1, 16, 16, 128, 64)],
}
SWEEP_CASES = [(k, d) for k, v in SWEEP.items() for d in v]
MASK_CASES = [(1, 16, 16, 64, 64), (5, 8, 8, 64, 64)]                                    # M = 256 and M = 320
# statistics epilogue: the unsplit launches -- the four above, and the small transposed convs of 64 input channels at 3 products
# (nkt = 12 is never split), both with a row tail
STATS_CASES = [(k, d, p) for k, d in UNSPLIT.items() for p in (6, 3)] + [("up256", (5, 8, 8, 64, 256), 3), ("up512", (3, 16, 16, 64, 128), 3)]
# weight gradient: K = 256, 320 (five pixel tiles), 1024 x the narrowest and a three-tile I (wide), I = 32 (narrow)
WGRAD_K = [(1, 16, 16), (5, 8, 8), (4, 16, 16)]
WGRAD_CASES = [("wgrad_wide", n + (O, I)) for n in WGRAD_K for O in (256, 512) for I in (16, 48)] + \
              [("wgrad_narrow", n + (O, 32)) for n in WGRAD_K for O in (128, 384)]


def case_id(v):
    """pytest id of one parameter value"""
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------ operands
def sparse_ints(shape, density, gen):
    """{-1, 0, +1} with P(non-zero) = density (the C1 operands of test_ops_exact_gpu.py), fp32 on the CPU"""
    r = torch.rand(shape, generator=gen)
    return (r < density / 2).float() - (r > 1 - density / 2).float()


def one_hot(op, dims, p, q, seed=1):
    """X in plane p of A, W in plane q of B, zeros elsewhere; returns (A planes, B planes, ref(X, W)) with its conditions
    asserted (S <= 256: the C1 bound of bf16 results, far inside fp32's)."""
    sa, sb, K = operand_shapes(op, *dims)
    gen = torch.Generator().manual_seed(seed)
    d = _density(K, 256)
    X, W = sparse_ints(sa, d, gen), sparse_ints(sb, d, gen)
    ref = OPS[op](X.double(), W.double())
    _conditions(ref, OPS[op](X.double().abs(), W.double().abs()), 256, "one-hot " + op)
    A, B = torch.zeros((3,) + tuple(sa)), torch.zeros((3,) + tuple(sb))
    A[p], B[q] = X, W
    return A, B, ref


def all_live(op, dims, seed=1, L=L_EXACT, scaled=True, products=6, var=64.0, kmul=1):
    """Three independent sparse integer planes per operand.  scaled: plane scales A_SCALE / B_SCALE and a density for
    sum_pairs weight * sum |a||b| <= L (the 6-pair weight sum: the same operands serve both tiers).  Not scaled (unit-weight
    form): a density for an output variance of `var` under the tier's pairs.  kmul: segments summed into one result."""
    sa, sb, K = operand_shapes(op, *dims)
    K *= kmul
    gen = torch.Generator().manual_seed(seed)
    d = _density(K * WSUM[6], L) if scaled else min(1.0, var / (len(PAIRS[products]) * K)) ** 0.5
    A = torch.stack([sparse_ints(sa, d, gen) * (A_SCALE[p] if scaled else 1.0) for p in range(3)])
    B = torch.stack([sparse_ints(sb, d, gen) * (B_SCALE[q] if scaled else 1.0) for q in range(3)])
    return A, B


def live_reference(op, A, B, products, L=L_EXACT, factor=None, what=""):
    """The all-live reference with its conditions: bound and non-trivial-case rule through _conditions (in units of 2^-16, or
    2^-17 under a mask factor of 1 / 0.5, so that its integer test applies).  A and B may be lists of segments (weight gradient
    of two segments: the sum)."""
    segs = list(zip(A, B)) if isinstance(A, (list, tuple)) else [(A, B)]
    ref = sum(planes_expected(op, a, b, products) for a, b in segs)
    S = sum(planes_expected(op, a.abs(), b.abs(), products) for a, b in segs)
    unit = UNIT
    if factor is not None:
        ref, unit = ref * factor.double(), 2 * UNIT
    _conditions(ref * unit, S * unit, L * unit, "all-live %s %s, %d products" % (op, what, products))
    return ref


L_MASK = 2.0 ** 7                 # the fused mask multiplies by 0.5: one more bit
L_WGRAD = L_EXACT - 4             # the weight gradient accumulates onto integers in -3 .. 3
SLOPE = 0.5


def sweep_operands(kernel, dims):
    return all_live(KERNELS[kernel][0], dims, seed=101)


def mask_operands(dims):
    """(A, B, mask [N, 2 Hl, 2 Wl, I] fp32 holding positive and negative values, +0.0 and -0.0, the factor 1 / SLOPE)"""
    A, B = all_live("up", dims, seed=103, L=L_MASK)
    N, Hl, Wl, O, I = dims
    gen = torch.Generator().manual_seed(104)
    m = torch.randn((N, 2 * Hl, 2 * Wl, I), generator=gen)
    r = torch.rand(m.shape, generator=gen)
    m = torch.where(r < 0.1, torch.zeros_like(m), m)
    m = torch.where((r >= 0.1) & (r < 0.2), -torch.zeros_like(m), m)
    return A, B, m, torch.where(m > 0, 1.0, SLOPE)


def stats_operands(kernel, dims, products):
    return all_live(KERNELS[kernel][0], dims, seed=105, scaled=False, products=products)


def wgrad_operands(dims, two):
    """([A segments], [B segments], the integers dw holds before an accumulating launch)"""
    segs = [all_live("wgrad", dims, seed=107 + 2 * s, L=L_WGRAD, kmul=2 if two else 1) for s in range(2 if two else 1)]
    N, Hl, Wl, O, I = dims
    dw0 = torch.randint(-3, 4, (O, 4, 4, I), generator=torch.Generator().manual_seed(111)).double()
    return [a for a, _ in segs], [b for _, b in segs], dw0


# ------------------------------------------------------------------ every (pair, k-tile) group is visible
UP_SHIFT = (-1, 0, 0, 1)          # transposed conv: tap kh of source row ho lands on output row 2 ho + kh - 1 = 2 hq + ph, hq = ho + shift


def _tap_rows(op, Hl, Wl, M, kh, kw):
    """the source pixel of every row of tap (kh, kw) in the kernels' row order m = (n, hl, wl): (n, hs, ws, inside the plane).
    conv: x[n, 2 hl + kh - 1, 2 wl + kw - 1]; transposed conv, parity class ((kh + 1) % 2, (kw + 1) % 2): g[n, hl - shift(kh),
    wl - shift(kw)]"""
    m = torch.arange(M)
    n, hl, wl = m // (Hl * Wl), (m // Wl) % Hl, m % Wl
    if op == "down":
        hs, ws, Hs, Ws = 2 * hl + kh - 1, 2 * wl + kw - 1, 2 * Hl, 2 * Wl
    else:
        hs, ws, Hs, Ws = hl - UP_SHIFT[kh], wl - UP_SHIFT[kw], Hl, Wl
    return n, hs, ws, (hs >= 0) & (hs < Hs) & (ws >= 0) & (ws < Ws)


def assert_conv_groups_live(op, A, B, products, bm, bn, rows=16):
    """Every (pair, tap, 64-channel block) k-tile of the conv kernels contributes a non-zero term to at least one output of
    every (row tile, column tile[, parity class]) in which the tap reads anything at all (the one-pixel tail tile of the
    unsplit cases sits in a corner: seven of its sixteen taps are padding), so that a k-tile dropped for one pair changes some
    output of every such block.  Above 4096 rows this is judged on the first `rows` rows of each row tile only, which is
    sufficient (a tile whose tap is live only beyond them fails).  Returns the number of groups."""
    N, Hl, Wl = A.shape[1], A.shape[2] // (2 if op == "down" else 1), A.shape[3] // (2 if op == "down" else 1)
    M = N * Hl * Wl
    ntiles = (M + bm - 1) // bm
    idx = torch.arange(M)
    sel = idx if M <= 4096 else idx[(idx % bm) < rows]
    Ad, Bd = A.double(), B.double()
    count = 0
    for kh in range(4):
        for kw in range(4):
            n, hs, ws, valid = _tap_rows(op, Hl, Wl, M, kh, kw)
            needed = torch.zeros(ntiles, dtype=torch.int32).index_add_(0, idx // bm, valid.int()) > 0
            assert bool(needed.any())
            for p, q in PAIRS[products]:
                src = Ad[p][n[sel], hs[sel].clamp(min=0, max=A.shape[2] - 1), ws[sel].clamp(min=0, max=A.shape[3] - 1)]
                src = src * valid[sel, None]
                for c0 in range(0, src.shape[1], 64):
                    wk = Bd[q][:, kh, kw, c0:c0 + 64].t() if op == "down" else Bd[q][c0:c0 + 64, kh, kw, :]
                    part = src[:, c0:c0 + 64] @ wk                                            # [selected rows, columns]
                    nz = (part != 0).reshape(part.shape[0], -1, bn).any(2)                    # per row, per column tile
                    live = torch.zeros(ntiles, nz.shape[1], dtype=torch.int32).index_add_(0, sel // bm, nz.int()) > 0
                    missing = needed[:, None] & ~live
                    assert not bool(missing.any()), "%s: pair (%d, %d), tap (%d, %d), channels %d..: no visible term in %d tiles" % (
                        op, p, q, kh, kw, c0, int(missing.sum()))
                    count += 1
    return count


def assert_wgrad_groups_live(A, B, products, to, tc):
    """Weight gradient: every (pair, 64-pixel tile) group contributes a non-zero term to every to x tc output tile."""
    from test_ops_exact_gpu import _patches
    n = 0
    for p, q in PAIRS[products]:
        g, P = A[p].double().reshape(-1, A.shape[-1]), _patches(B[q].double())
        for k0 in range(0, g.shape[0], 64):
            part = g[k0:k0 + 64].t() @ P[k0:k0 + 64]                                       # [O, 16 I]
            nz = (part != 0).reshape(part.shape[0] // to, to, part.shape[1] // tc, tc).any(3).any(1)
            assert bool(nz.all()), "wgrad: pair (%d, %d), pixels %d..: no visible term in %d tiles" % (p, q, k0, int((~nz).sum()))
            n += 1
    return n


def unit_reference(op, A, B, products, what=""):
    """Unit-weight form: the integer output and its column sums (of y and of y^2 over all rows), every partial of which is
    exact in fp32 because the column sums of |y| and of y^2 stay <= 2^24 (asserted)."""
    y = planes_expected(op, A, B, products)
    C = y.shape[-1]
    yr = y.reshape(-1, C)
    assert torch.equal(y, y.round())
    assert float(yr.abs().sum(0).max()) <= 2 ** 24 and float((yr * yr).sum(0).max()) <= 2 ** 24, what + ": column sums beyond 2^24"
    zeros, distinct = float((y == 0).float().mean()), int(torch.unique(y).numel())
    assert zeros <= 0.10 and distinct >= 50, "%s: trivial case (%.1f %% zeros, %d distinct values)" % (what, 100 * zeros, distinct)
    return y, torch.stack([yr.sum(0), (yr * yr).sum(0)])


# ------------------------------------------------------------------ rg_split_planes: the structured set
MANTISSAS = (0, 1, 0x7fff, 0x8000, 0x8001, 0x18000, 0x7fffff)        # 0x8000 and 0x18000: the two round-to-even ties


def _from_bits(exps, mants):
    b = [(s << 31) | ((e + 127) << 23) | m for e in exps for m in mants for s in (0, 1)]
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in b], dtype=torch.int32).view(torch.float32)


def structured_values():
    """every exponent 2^-100 .. 2^127 x MANTISSAS x both signs, then +-0, +-inf, NaN, +-3.4e38"""
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4e38, -3.4e38])
    return torch.cat([special, _from_bits(range(-100, 128), MANTISSAS)])


def tiny_values():
    """|v| < 2^-100 down to the fp32 subnormals: the residual planes can be bf16 subnormals (outside the asserted set)"""
    sub = torch.tensor([1, 0x8000, 0x18000, 0x7fffff, 0x400000], dtype=torch.int32).view(torch.float32)
    return torch.cat([_from_bits(range(-126, -100), MANTISSAS), sub, -sub])


def tiled(values, n):
    """`values` repeated to n elements"""
    return values.repeat((n + values.numel() - 1) // values.numel())[:n].contiguous()


def bf16_rne_bits(x64):
    """An independent round-to-nearest-even of finite fp64 values that are fp32 numbers, in integer arithmetic on the fp32 bit
    image: the upper 16 bits after adding 0x7fff + (bit 16).  Returns the bf16 bit pattern as int32 (overflow gives 0x7f80)."""
    b = x64.float().view(torch.int32).to(torch.int64) & 0xffffffff
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    return (r & 0xffff).to(torch.int32)
